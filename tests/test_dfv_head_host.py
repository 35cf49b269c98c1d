"""CPU: the host side of the cost-volume depth head (csrc/dfv_head.hip, aadff/ops.py, aadff/dfv_head.py) - the oracle of
tests/dfv_head_common.py against what the reference's own disparityregression computed on F.softmax(F.interpolate(...))
(tests/golden/g20_dfv_head.npz, written by tests/golden/make_dfv_head_golden.py), every argument error of the two C entries without a
GPU, the fake-tensor shapes of the ops, the public functions' errors and empty results.

Oracle against golden: in float32 within d32 of each case and tensor, the oracle's own float32-to-float64 distance (the two bilinear
cases are the same torch composition, the trilinear one keeps the depth and differs from it by rounding at most); in float64 to 1e-6
relative L2 (the golden arrays are float32 results: their own rounding is about 1e-7)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import dfv_head_common as dc
from aadff import _abi, dfv_head

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
ENTRIES = ("aadff_dfv_head_fwd", "aadff_dfv_head_bwd")
KEYS = ("pred", "std", "d_cost", "d_foc_dists")


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_dfv_head.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else z[k]) for k in z.files}


def test_golden_file_is_small_and_complete(gold, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g20_dfv_head.npz")) < 400 << 10
    assert [str(c) for c in gold["cases"]] == ["bilinear|8|12|32|48", "bilinear|9|13|37|54", "trilinear|4|5|32|40"]
    foc = gold["foc_dists"]
    assert foc.shape == (2, 5) and not torch.equal(foc[0], foc[1]) and bool((foc[1][1:] < foc[1][:-1]).all())
    for i, case in enumerate(gold["cases"]):
        _, h, w, H, W = str(case).split("|")
        cost = gold[f"case{i}_cost"]
        assert cost.shape == (2, 5, int(h), int(w)) and float(cost.min()) <= -5 and float(cost.max()) >= 5
        assert gold[f"case{i}_pred"].shape == gold[f"case{i}_std"].shape == gold[f"case{i}_g_pred"].shape == (2, 1, int(H), int(W))
        assert gold[f"case{i}_d_cost"].shape == cost.shape and gold[f"case{i}_d_foc_dists"].shape == (2, 5)


@pytest.mark.parametrize("i", range(3))
def test_oracle_reproduces_the_reference(gold, i):
    _, _, _, H, W = str(gold["cases"][i]).split("|")
    args = (gold[f"case{i}_cost"], gold["foc_dists"], gold[f"case{i}_g_pred"], (int(H), int(W)))
    f64, f32 = dc.head_grads(*args, dtype=torch.float64), dc.head_grads(*args, dtype=torch.float32)
    for k in KEYS:
        want = gold[f"case{i}_{k}"]
        d64, d32, got = dc.rel_l2(want, f64[k]), dc.rel_l2(f32[k], f64[k]), dc.rel_l2(f32[k], want)
        print(f"case {i} {k}: float64 oracle vs golden {d64:.2e}; float32 oracle vs golden {got:.2e}, its d32 {d32:.2e}")
        assert d64 <= 1e-6, f"case {i} {k}: float64 oracle is {d64:.2e} from the golden array"
        # The bound is the issue's.  In the trilinear case it holds with little room (d_foc_dists 1.31e-7 against 1.35e-7): both sides
        # are float32 roundings of the installed torch's CPU kernels, so another torch build can move either without any change here.
        assert got <= d32, f"case {i} {k}: float32 oracle is {got:.2e} from the golden array, d32 = {d32:.2e}"


def test_oracle_std_carries_no_gradient_and_extremes_stay_finite():
    t = dc.head_inputs(2, 10, 9, 19, 36, 76, seed=3, extremes=True)
    assert sorted(v for v in t["cost"].flatten().tolist() if abs(v) >= 79) == sorted(dc.EXTREMES)
    c, u = t["cost"].clone().requires_grad_(True), t["foc_dists"].clone().requires_grad_(True)
    pred, std, prob = dc.head(c, u, t["size"])
    assert pred.requires_grad and not std.requires_grad and std.grad_fn is None
    r = dc.head_grads(t["cost"], t["foc_dists"], t["g_pred"], t["size"], dtype=torch.float32)
    assert all(bool(torch.isfinite(r[k]).all()) for k in KEYS)
    # the form of std: sum p (pred - f)^2, which is the variance of f under p
    p, f = r["prob"].double(), t["foc_dists"].double().reshape(2, 10, 1, 1)
    var = (p * f * f).sum(1, keepdim=True) - (p * f).sum(1, keepdim=True) ** 2
    assert torch.allclose(r["std"].double() ** 2, var, atol=1e-5)


def test_symbols_are_exported_bound_and_declared(repo_root):
    lib = C.CDLL(_abi.LIB_PATH)
    header = open(os.path.join(repo_root, "include", "aadff.h")).read()
    declared = set(re.findall(r"^\s*int\s+(aadff_\w+)\s*\(", header, flags=re.M))
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _abi.PROTOTYPES and name in declared
    proto = {name: re.search(r"^\s*int\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M | re.S).group(1).split(",") for name in ENTRIES}
    assert all(len(proto[name]) == len(_abi.PROTOTYPES[name]) for name in ENTRIES)                # as many arguments bound as declared
    assert _abi.load_library().aadff_abi_version() == _abi.ABI_VERSION == 9                       # additions only


def test_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    err = lambda: lib.aadff_last_error()                                          # noqa: E731

    def fwd(cost=P8, foc=P8, pred=P8, std=P8, prob=None, B=2, S=5, h=9, w=13, H=37, W=54):
        return lib.aadff_dfv_head_fwd(cost, foc, pred, std, prob, B, S, h, w, H, W, None)

    def bwd(cost=P8, foc=P8, g=P8, dc_=P8, du=P8, ws=P8, nbytes=1 << 20, B=2, S=5, h=9, w=13, H=37, W=54):
        return lib.aadff_dfv_head_bwd(cost, foc, g, dc_, du, ws, nbytes, B, S, h, w, H, W, None)

    for call, names in ((fwd, ("cost", "foc", "pred", "std")), (bwd, ("cost", "foc", "g"))):
        for name in names:
            assert call(**{name: None}) == -1 and b"is NULL" in err()
        assert call(S=0) == -1 and b"S = 0" in err()
        assert call(S=-2) == -1 and b"S = -2" in err()
        assert call(B=0) == -1 and b"B = 0" in err()
        assert call(h=0) == -1 and b"0 x 13" in err()
        assert call(w=-1) == -1 and b"9 x -1" in err()
        assert call(H=8) == -1 and b"shrinking" in err() and b"8 x 54" in err()
        assert call(W=12) == -1 and b"shrinking" in err()
        assert call(H=0, W=0) == -1 and b"shrinking" in err()
        assert call(H=70000, W=70000) == -1 and b"too large" in err()
    assert bwd(dc_=None, du=None) == -1 and b"no gradient" in err()
    assert bwd(ws=None) == -1 and b"workspace" in err()
    # ratio ceil(54 / 13) = 5: TC = 8 cells, R = 256 // 46 = 5 rows -> 2 x 8 workgroups per image: 4 * 2 * 5 * (37 * 13 + 16) bytes
    from aadff import ops
    assert ops.dfv_bwd_tiling(13, 54) == (8, 5)
    need = ops.dfv_bwd_workspace_bytes(2, 5, 9, 13, 37, 54)
    assert need == 4 * 2 * 5 * (37 * 13 + 16)
    assert bwd(nbytes=need - 1) == -1 and b"workspace" in err() and b"%d are needed" % need in err()
    only_foc = ops.dfv_bwd_workspace_bytes(2, 5, 9, 13, 37, 54, need_cost=False)
    assert only_foc == 4 * 2 * 5 * 16 and bwd(dc_=None, nbytes=only_foc - 1) == -1 and b"%d are needed" % only_foc in err()
    assert ops.dfv_bwd_tiling(4, 128) == (6, 1) and ops.dfv_bwd_tiling(18, 18) == (8, 8) and ops.dfv_bwd_tiling(3, 1000) == (1, 1)


def test_ops_and_fake_shapes():
    from aadff import ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("dfv_regress", "dfv_regress_bwd"):
        assert hasattr(torch.ops.aadff, name)
    with FakeTensorMode():
        new = lambda *s: torch.empty(*s, device="cuda")                            # noqa: E731
        c, u = new(2, 5, 9, 13), new(2, 5)
        pred, std, prob = torch.ops.aadff.dfv_regress(c, u, 37, 54, False)
        assert pred.shape == std.shape == (2, 1, 37, 54) and prob.shape == (0,) and pred.dtype == std.dtype == torch.float32
        pred, std, prob = torch.ops.aadff.dfv_regress(c, u, 37, 54, True)
        assert prob.shape == (2, 5, 37, 54) and prob.dtype == torch.float32
        d_c, d_u = torch.ops.aadff.dfv_regress_bwd(c, u, pred, True, True)
        assert d_c.shape == c.shape and d_u.shape == (2, 5)
        d_c, d_u = torch.ops.aadff.dfv_regress_bwd(c, u, pred, False, True)
        assert d_c.shape == (0,) and d_u.shape == (2, 5)


def test_public_value_errors():
    c, u = torch.zeros(2, 4, 8, 8), torch.ones(2, 4)
    for bad in (dict(cost=c[0]), dict(cost=[[1.0]]), dict(cost=torch.zeros(2, 2, 4, 8, 8)), dict(cost=torch.zeros(2, 1, 1, 4, 8, 8)),
                dict(cost=c[:, :0], foc_dists=u[:, :0]), dict(foc_dists=u[:, :3]), dict(foc_dists=u[0]), dict(foc_dists=u.reshape(2, 2, 2)),
                dict(foc_dists=torch.ones(2, 5)),                                             # a cost depth other than S
                dict(size=16), dict(size=(16,)), dict(size=(16, 16, 16)), dict(size=(16.0, 16)), dict(size=(True, 16)),
                dict(size=(7, 16)), dict(size=(16, 7)), dict(size=(0, 0)),
                dict(cost=c[:, :, :0], size=(4, 8))):
        with pytest.raises(ValueError, match="cost_volume_depth"):
            dfv_head.cost_volume_depth(**{**dict(cost=c, foc_dists=u), **bad})
    for bad in (dict(size=(np.float32(16), 16)), dict(size=(np.bool_(True), 16)), dict(size="ab"), dict(size=(np.int64(7), np.int64(16)))):
        with pytest.raises(ValueError, match="cost_volume_depth"):
            dfv_head.cost_volume_depth(**{**dict(cost=c, foc_dists=u), **bad})
    for bad in (c, [], ()):
        with pytest.raises(ValueError, match="cost_volume_depth_levels"):
            dfv_head.cost_volume_depth_levels(bad, u, (16, 16))
    with pytest.raises(ValueError, match="cost_volume_depth"):
        dfv_head.cost_volume_depth_levels([c[0], c], u, (16, 16))


def test_empty_shapes_need_no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    for (B, S, h, w), size in (((0, 4, 8, 8), (16, 16)), ((2, 4, 0, 8), None), ((2, 4, 8, 0), None), ((2, 4, 0, 0), (0, 0))):
        H, W = (h, w) if size is None else size
        c, u = torch.zeros(B, S, h, w, requires_grad=True), torch.ones(B, S, requires_grad=True)
        pred, std = dfv_head.cost_volume_depth(c, u, size)
        assert pred.shape == std.shape == (B, 1, H, W) and pred.dtype == std.dtype == torch.float32
        assert pred.requires_grad and not std.requires_grad
        pred.sum().backward()
        assert c.grad.shape == c.shape and u.grad.shape == u.shape
        pred, std, prob = dfv_head.cost_volume_depth(c[:, None], u, size, return_prob=True)       # the 5-D form
        assert prob.shape == (B, S, H, W) and not prob.requires_grad
    pred, std = dfv_head.cost_volume_depth(torch.zeros(0, 3, 4, 4), torch.ones(0, 3), (np.int64(8), np.int32(9)))      # any integer type
    assert pred.shape == (0, 1, 8, 9) and dfv_head.cost_volume_depth(torch.zeros(0, 3, 4, 4), torch.ones(0, 3), torch.Size([8, 9]))[1].shape == (0, 1, 8, 9)
    preds, stds = dfv_head.cost_volume_depth_levels([torch.zeros(0, 3, 4, 4), torch.zeros(0, 3, 2, 2)], torch.ones(0, 3), (8, 8))
    assert [p.shape for p in preds] == [s.shape for s in stds] == [(0, 1, 8, 8)] * 2
    m = dfv_head.CostVolumeHead(size=(8, 8), return_prob=True)
    assert "size=(8, 8)" in repr(m) and "return_prob=True" in repr(m) and m(torch.zeros(0, 3, 4, 4), torch.ones(0, 3))[2].shape == (0, 3, 8, 8)
    with pytest.raises(RuntimeError, match="no HIP device"):                        # and no CPU fallback for the rest
        dfv_head.cost_volume_depth(torch.zeros(1, 3, 4, 4), torch.ones(3), (8, 8))
