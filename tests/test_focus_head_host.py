"""CPU: the host side of the differentiable depth head and its loss (csrc/focus_head.hip, aadff/ops.py, aadff/focus_head.py) - the oracle
of tests/focus_head_common.py against what the reference's own AiFDepthNet computed (tests/golden/g18_focus_head.npz, written by
tests/golden/make_focus_head_golden.py), every argument error of the four C entries without a GPU, the fake-tensor shapes of the ops, the
public functions' errors and empty results, and the `dff` stubs, which stay stubs.

Oracle against golden: in float64 to 1e-6 relative L2 (the golden arrays are float32 results: their own rounding is about 1e-7); in
float32 within 4 x the oracle's own float32-vs-float64 distance d32, the project's allowance for another order of the same float32 steps.
A loss dict is compared as one vector of its values."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import focus_head_common as fc
from aadff import _abi, focus_head

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
ENTRIES = ("aadff_attention_depth", "aadff_attention_depth_bwd", "aadff_dff_loss_sums", "aadff_dff_loss_bwd")


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "g18_focus_head.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else z[k]) for k in z.files}


def _against_golden(name, want, f32, f64):
    d64, d32, got = fc.rel_l2(want, f64), fc.rel_l2(f32, f64), fc.rel_l2(f32, want)
    print(f"{name}: float64 oracle vs golden {d64:.2e}; float32 oracle vs golden {got:.2e}, its d32 {d32:.2e}")
    assert d64 <= 1e-6, f"{name}: float64 oracle is {d64:.2e} from the golden array"
    assert got <= 4 * d32, f"{name}: float32 oracle is {got:.2e} from the golden array, 4 x d32 = {4 * d32:.2e}"


def test_golden_file_is_small_and_complete(gold, golden_dir):
    assert os.path.getsize(os.path.join(golden_dir, "g18_focus_head.npz")) < 1 << 20
    assert gold["stack"].shape == (2, 3, 4, 32, 32) and gold["foc_dists"].shape == (2, 4)
    assert not torch.equal(gold["foc_dists"][0], gold["foc_dists"][1])
    assert [tuple(r) for r in gold["nets"]] == [(1, 0), (1, 1), (2, 0), (2, 1)]
    for i in range(4):
        z = gold[f"net{i}_logits"]
        assert float(z.min()) <= -5 and float(z.max()) >= 5
    assert float(gold["net3_logits"].max()) > 20                                   # past softplus's threshold, normalised variant
    zeros = float((gold["gt_depth"] == 0).float().mean())
    assert 0.05 < zeros < 0.15
    assert [str(c) for c in gold["loss_cases"]] == ["D_FS|0|32|32", "D_FS|1|32|32", "A_FS|0|32|32", "A_FS|1|32|32", "DA_FS|0|32|32", "DA_FS|1|32|32",
                                                    "DA_FS|0|30|31"]


@pytest.mark.parametrize("i", range(4))
def test_oracle_head_reproduces_the_reference(gold, i):
    K, norm = (int(v) for v in gold["nets"][i])
    args = (gold[f"net{i}_logits"], gold["stack"], gold["foc_dists"], gold["g_depth"], gold["g_aif"], bool(norm))
    assert args[0].shape[1] == K
    f64, f32 = fc.head_grads(*args, dtype=torch.float64), fc.head_grads(*args, dtype=torch.float32)
    for key, name in (("depth", "depth"), ("aif", "aif"), ("d_scores", "d_logits")):
        _against_golden(f"net {i} {name}", gold[f"net{i}_{name}"], f32[key], f64[key])


@pytest.mark.parametrize("j", range(7))
def test_oracle_loss_reproduces_the_reference(gold, j):
    task, mr, h, w = str(gold["loss_cases"][j]).split("|")
    h, w = int(h), int(w)
    disp_w, aif_w, smooth_w = (float(v) for v in gold["weights"])
    gd = gold["gt_depth"][:, :, :h, :w]
    ga = gold["gt_aif"][:, :, :h, :w] if task == "A_FS" else gold["gt_aif"]
    kw = dict(task=task, foc_dists=gold["foc_dists"], mask_range=bool(int(mr)), disp_w=disp_w, aif_w=aif_w, smooth_w=smooth_w)
    f64 = fc.loss_grads(gold["net0_depth"], gold["net0_aif"], gd, ga, dtype=torch.float64, **kw)
    f32 = fc.loss_grads(gold["net0_depth"], gold["net0_aif"], gd, ga, dtype=torch.float32, **kw)
    keys = [str(k) for k in gold[f"loss{j}_keys"]]
    assert list(f64["losses"]) == keys
    vec = lambda r: torch.stack([r["losses"][k] for k in keys])                    # noqa: E731
    _against_golden(f"loss {j} values", gold[f"loss{j}_values"], vec(f32), vec(f64))
    _against_golden(f"loss {j} d_depth", gold[f"loss{j}_d_depth"], f32["d_depth"], f64["d_depth"])
    _against_golden(f"loss {j} d_aif", gold[f"loss{j}_d_aif"], f32["d_aif"], f64["d_aif"])
    if (h, w) != (32, 32):                                                         # nothing flows outside the window
        assert not f64["d_depth"][:, :, h:].any() and not f64["d_depth"][:, :, :, w:].any() and not f64["d_aif"][:, :, h:].any()


def test_oracle_sums_make_the_dict():
    t = fc.loss_inputs(2, 3, 9, 11, seed=4)
    for task in focus_head.TASKS:
        for mr in (False, True):
            r = fc.loss_grads(t["depth"], t["aif"], t["gt_depth"], t["gt_aif"], task=task, foc_dists=t["foc_dists"], mask_range=mr)
            s, L = r["sums"], r["losses"]
            if task != "A_FS":
                assert torch.allclose(L["depth"], s[0] / s[1], rtol=1e-13) and 0 < float(s[1]) < 2 * 9 * 11
            if task == "D_FS":
                assert torch.allclose(L["disp_MSE"], s[2] / s[1], rtol=1e-13)
            if task != "D_FS":
                assert torch.allclose(L["AiF"], s[3] / (2 * 3 * 9 * 11), rtol=1e-13)
                assert torch.allclose(L["smooth"], (s[4] / (2 * 8 * 11) + s[5] / (2 * 9 * 10)) / 2, rtol=1e-13)
                assert 0.05 < float(L["smooth"]) < 1.0                               # the edge weights are neither all 0 nor all 1


def test_symbols_are_exported_and_bound():
    lib = C.CDLL(_abi.LIB_PATH)
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _abi.PROTOTYPES
    assert _abi.load_library().aadff_abi_version() == _abi.ABI_VERSION == 9         # additions only


def test_head_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    err = lambda: lib.aadff_last_error()                                          # noqa: E731

    def fwd(scores=P8, stack=P8, foc=P8, depth=P8, aif=P8, N=2, K=1, Ct=3, Ca=3, S=4, H=16, W=16):
        return lib.aadff_attention_depth(scores, stack, foc, depth, aif, N, K, Ct, Ca, S, H, W, 0, None)

    def bwd(scores=P8, stack=P8, foc=P8, gd=P8, ga=P8, dz=P8, dx=P8, du=P8, ws=P8, nbytes=1 << 20, N=2, K=1, Ct=3, Ca=3, S=4, H=16, W=16):
        return lib.aadff_attention_depth_bwd(scores, stack, foc, gd, ga, dz, dx, du, ws, nbytes, N, K, Ct, Ca, S, H, W, 0, None)

    for call, names in ((fwd, ("scores", "stack", "foc", "depth", "aif")), (bwd, ("scores", "stack", "foc", "gd", "ga"))):
        for name in names:
            assert call(**{name: None}) == -1 and b"is NULL" in err()
        for K in (0, 3):
            assert call(K=K) == -1 and b"K = %d" % K in err()
        assert call(Ct=0) == -1 and b"Ct = 0" in err()
        assert call(Ct=5, Ca=3) == -1 and b"Ct = 5" in err()
        assert call(Ct=2, Ca=3) == -1 and b"Ca = 3" in err()
        assert call(Ca=0) == -1 and b"Ca = 0" in err()
        assert call(S=0) == -1 and b"S = 0" in err()
        assert call(N=0) == -1 and b"N = 0" in err()
        assert call(H=0) == -1 and b"H = 0" in err()
        assert call(W=-3) == -1 and b"W = -3" in err()
        assert call(N=70000, H=70000, W=70000) == -1 and b"too large" in err()
    assert bwd(dz=None, dx=None, du=None) == -1 and b"no gradient" in err()
    assert bwd(ws=None) == -1 and b"workspace" in err()
    assert bwd(nbytes=2 * 4 * 4 * 4 - 1) == -1 and b"workspace" in err()           # N S 4 ceil(16 * 4 / 256) floats are needed


def test_loss_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    err = lambda: lib.aadff_last_error()                                          # noqa: E731

    def sums(depth=P8, aif=P8, gtd=P8, gta=P8, out=P8, ws=P8, nbytes=1 << 20, N=2, Ca=3, dims=(16, 16) * 4):
        return lib.aadff_dff_loss_sums(depth, aif, gtd, gta, None, out, ws, nbytes, N, Ca, *dims, None)

    def bwd(depth=P8, aif=P8, gtd=P8, gta=P8, g=P8, dd=P8, da=P8, N=2, Ca=3, dims=(16, 16) * 4):
        return lib.aadff_dff_loss_bwd(depth, aif, gtd, gta, None, g, dd, da, N, Ca, *dims, None)

    for call in (sums, bwd):
        assert call(depth=None) == -1 and b"depth is NULL" in err()
        assert call(gtd=None, gta=None) == -1 and b"neither" in err()
        assert call(aif=None) == -1 and b"aif is NULL" in err()
        assert call(N=0) == -1 and b"N = 0" in err()
        for Ca in (0, 5):
            assert call(Ca=Ca) == -1 and b"Ca = %d" % Ca in err()
        assert call(dims=(0, 16) + (16, 16) * 3) == -1 and b"depth is 0 x 16" in err()
        assert call(dims=(16, 16, 16, 16, 16, -1, 16, 16)) == -1 and b"gt_depth is 16 x -1" in err()
        assert call(dims=(16, 16) * 3 + (0, 4)) == -1 and b"gt_aif is 0 x 4" in err()
    assert sums(out=None) == -1 and b"sums is NULL" in err()
    assert sums(ws=None) == -1 and b"workspace" in err()
    assert sums(nbytes=47) == -1 and b"workspace" in err()
    assert bwd(g=None) == -1 and b"g_sums is NULL" in err()
    assert bwd(dd=None, da=None) == -1 and b"no gradient" in err()


def test_ops_and_fake_shapes():
    from aadff import ops  # noqa: F401
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("attention_depth", "attention_depth_bwd", "dff_loss_sums", "dff_loss_bwd"):
        assert hasattr(torch.ops.aadff, name)
    with FakeTensorMode():
        new = lambda *s: torch.empty(*s, device="cuda")                            # noqa: E731
        z, x, u = new(2, 2, 5, 40, 56), new(2, 4, 5, 40, 56), new(2, 5)
        d, a = torch.ops.aadff.attention_depth(z, x, u, True, 3)
        assert d.shape == (2, 1, 40, 56) and a.shape == (2, 3, 40, 56) and d.dtype == a.dtype == torch.float32
        dz, dx, du = torch.ops.aadff.attention_depth_bwd(z, x, u, d, a, True, 3, True, True, True)
        assert dz.shape == z.shape and dx.shape == x.shape and du.shape == (2, 5)
        dz, dx, du = torch.ops.aadff.attention_depth_bwd(z, x, u, d, a, False, 3, False, True, False)
        assert dz.shape == (0,) and dx.shape == x.shape and du.shape == (0,)
        s = torch.ops.aadff.dff_loss_sums(d, a, new(2, 1, 38, 50), new(2, 3, 40, 56), new(0))
        assert s.shape == (6,) and s.dtype == torch.float64
        dd, da = torch.ops.aadff.dff_loss_bwd(d, a, new(2, 1, 38, 50), new(2, 3, 40, 56), new(2), s, True, True)
        assert dd.shape == d.shape and da.shape == a.shape and dd.dtype == torch.float32
        dd, da = torch.ops.aadff.dff_loss_bwd(d, a, new(2, 1, 38, 50), new(0), new(0), s, True, False)
        assert dd.shape == d.shape and da.shape == (0,)
    assert focus_head.ops.attention_bwd_workspace_bytes(2, 4, 16, 16) == 2 * 4 * 4 * 4
    assert focus_head.ops.attention_bwd_workspace_bytes(1, 10, 37, 70) == 10 * 4 * 4 * 3      # 37 rows of 18 groups: 666 threads, 3 workgroups


def test_public_value_errors():
    z, x, u = torch.zeros(2, 1, 4, 8, 8), torch.zeros(2, 3, 4, 8, 8), torch.ones(2, 4)
    for bad in (dict(scores=z[0]), dict(stack=x[0]), dict(scores=torch.zeros(2, 3, 4, 8, 8)), dict(stack=torch.zeros(2, 5, 4, 8, 8)),
                dict(stack=x[:, :, :3]), dict(stack=x[:, :, :, :7]), dict(aif_channels=4), dict(aif_channels=0), dict(aif_channels=2.0),
                dict(foc_dists=u[:, :3]), dict(foc_dists=u[0]), dict(foc_dists=u.reshape(2, 2, 2)),
                dict(scores=z[:, :, :0], stack=x[:, :, :0], foc_dists=u[:, :0])):
        with pytest.raises(ValueError, match="attention_depth"):
            focus_head.attention_depth(**{**dict(scores=z, stack=x, foc_dists=u), **bad})
    d, a, gd, ga = torch.zeros(2, 1, 8, 8), torch.zeros(2, 3, 8, 8), torch.ones(2, 1, 8, 8), torch.zeros(2, 3, 8, 8)
    with pytest.raises(NotImplementedError):
        focus_head.dff_losses(d, a, gd, ga, task="FS")
    for task, bad in (("D_FS", dict(gt_depth=None)), ("D_FS", dict(depth=d[0])), ("D_FS", dict(depth=a)), ("D_FS", dict(gt_depth=ga)),
                      ("A_FS", dict(gt_aif=None)), ("A_FS", dict(gt_aif=ga[:, :2])), ("A_FS", dict(aif=a[0])), ("DA_FS", dict(gt_depth=None)),
                      ("DA_FS", dict(gt_aif=ga[:1])), ("D_FS", dict(gt_depth=gd[:1])), ("D_FS", dict(mask_range=True)),
                      ("A_FS", dict(aif=torch.zeros(2, 5, 8, 8), gt_aif=torch.zeros(2, 5, 8, 8)))):
        with pytest.raises(ValueError, match="dff_losses"):
            focus_head.dff_losses(**{**dict(depth=d, aif=a, gt_depth=gd, gt_aif=ga, task=task), **bad})


def test_empty_shapes_need_no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    for shape in ((0, 4, 8, 8), (2, 4, 0, 8), (2, 4, 8, 0)):
        N, S, H, W = shape
        z = torch.zeros(N, 2, S, H, W, requires_grad=True)
        d, a = focus_head.attention_depth(z, torch.zeros(N, 4, S, H, W), torch.ones(N, S))
        assert d.shape == (N, 1, H, W) and a.shape == (N, 3, H, W) and d.dtype == a.dtype == torch.float32
        (d.sum() + a.sum()).backward()
        assert z.grad.shape == z.shape
        out = focus_head.dff_losses(d, a, torch.ones(N, 1, H, W), torch.zeros(N, 3, H, W), task="DA_FS", pred_name="disp")
        assert list(out) == ["disp", "AiF", "smooth", "total"] and all(v.dim() == 0 and torch.isnan(v) for v in out.values())
    assert list(focus_head.dff_losses(torch.zeros(0, 1, 4, 4), None, torch.zeros(0, 1, 4, 4))) == ["depth", "disp_MSE", "total"]
    m = focus_head.AttentionHead(normalize_attention=True)
    assert m.normalize_attention and "normalize_attention=True" in repr(m) and m(torch.zeros(0, 1, 3, 4, 4), torch.zeros(0, 3, 3, 4, 4), torch.ones(0, 3))[0].shape == (0, 1, 4, 4)
    with pytest.raises(RuntimeError, match="no HIP device"):                        # and no CPU fallback for the rest
        focus_head.attention_depth(torch.zeros(1, 1, 3, 4, 4), torch.zeros(1, 3, 3, 4, 4), torch.ones(3))
    with pytest.raises(RuntimeError, match="no HIP device"):
        focus_head.dff_losses(torch.zeros(1, 1, 4, 4), None, torch.ones(1, 1, 4, 4))


def test_dff_stubs_still_raise():
    import dff
    if not os.environ.get("AADFF_REFERENCE_ROOT"):
        with pytest.raises(ImportError, match="AADFF_REFERENCE_ROOT"):
            dff.AiFDepthNet(n_classes=1, n_stack=4)
        with pytest.raises(ImportError, match="dff/metrics.py"):
            dff.mask_mae(None, None, None)
    assert not hasattr(dff, "attention_depth") and not hasattr(dff, "dff_losses")   # the head lives under aadff only
