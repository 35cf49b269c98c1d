"""GPU tests (run with `-m gpu` on an MI355X) of the fused cost-volume depth head (csrc/dfv_head.hip) through torch.ops.aadff.dfv_regress and
aadff.dfv_head, against the torch CPU oracle of tests/dfv_head_common.py evaluated in float64 on the same float32 inputs.

Budget of every parity comparison: relative L2 per tensor <= 4 x d32, where d32 is the distance of the SAME
oracle evaluated in float32 on the CPU from its float64 evaluation, computed here for the very inputs of the case - the project's
standing allowance for another summation order of the same float32 terms.  Against the reference's golden arrays, themselves float32
results at distance d32 from the float64 oracle, the budget is (4 + 1) x d32 by the triangle inequality.  Nothing is measured against
the code under test and no element is excluded.  Where d32 is exactly 0 the kernel must be exact too.  Every (error, budget) pair goes
through the `margin` fixture.

Shapes (B, S, h, w, H, W) and the tiles they meet:
  * head_fwd: a workgroup owns 64 x 4 output pixels.  37 x 54 gives 1 x 10 workgroups per image, ragged on both axes; 36 x 76 gives
    2 x 9, the second column 12 pixels wide; 96 x 128 gives 2 x 24 full ones.
  * bwd_reduce_x: a workgroup owns TC cells of a cost row for R output rows and 16 slices, TC and R from the integer ratio
    (include/aadff.h).  9 x 13 -> 37 x 54: TC 8, R 5, so 2 x 8 workgroups per image with a ragged last one on both axes (5 cells, 2 rows)
    and pixels between the two cell tiles read by both; 9 x 19 -> 36 x 76: TC 8, R 6, so 3 x 6 with a last tile of 3 cells; S = 17
    (12 x 18, ratio 1, TC 8, R 8: 3 x 2 workgroups) needs a second slab of one slice; 3 x 4 -> 96 x 128: TC 6, R 1, a footprint of 128
    pixels per row.  1 x 6 -> 1 x 23, 5 x 1 -> 19 x 1, 1 x 1 -> 5 x 7 and 1 x 1 -> 1 x 1 are the degenerate extents.
  * bwd_reduce_y: a thread per element of d_cost, a workgroup per 256 neighbouring elements of one plane (b, s).  The issue's shapes all
    have planes of at most 216 elements, one ragged workgroup per plane, so 23 x 29 -> 47 x 59 is added to them: a plane of 667 elements
    is three workgroups with a last one of 155, the decomposition every real size takes (120 x 160 is 75 per plane).  It also gives
    head_fwd 1 x 12 ragged workgroups and bwd_reduce_x (ratio 3: TC 8, R 8) 4 x 6 with a last tile of 5 cells and 7 rows.
  * the extreme costs (+-80, +-1e4) sit in the 9 x 19 -> 36 x 76 case: at ratio 4 the interpolation weights are multiples of 1/8,
    exact in float32 and float64 alike, so a cell of 1e4 either is not read or outweighs every other slice by more than 150 and d32
    measures the softmax; at a ratio that float32 rounds, d32 would be the rounding of a few weights times 1e4, a matter of chance.
  * one case has 2.3e9 elements per tensor: offsets past 2^31 show only there.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import dfv_head_common as dc                                 # noqa: E402
from aadff import ops  # noqa: E402,F401
from aadff.dfv_head import CostVolumeHead, cost_volume_depth, cost_volume_depth_levels      # noqa: E402

DEV = "cuda:0"
SHAPES = [(2, 1, 1, 1, 1, 1), (2, 3, 1, 1, 5, 7), (2, 4, 1, 6, 1, 23), (2, 4, 5, 1, 19, 1), (2, 6, 7, 9, 10, 13), (2, 5, 9, 13, 37, 54),
          (2, 10, 9, 19, 36, 76), (2, 17, 12, 18, 12, 18), (1, 8, 3, 4, 96, 128), (2, 3, 23, 29, 47, 59)]
IDS = ["%dx%dx%dx%d_to_%dx%d" % s for s in SHAPES]
ODD, RATIO4, RATIO32 = SHAPES[5], SHAPES[6], SHAPES[8]
KEYS = ("pred", "std", "prob", "d_cost", "d_foc_dists")

_CASES = {}


def _case(shape, extremes=False):
    """Seeded inputs of a case with the oracle in float64 and float32 (cached, read-only)."""
    if (shape, extremes) not in _CASES:
        t = dc.head_inputs(*shape, seed=20 + SHAPES.index(shape), extremes=extremes)
        args = (t["cost"], t["foc_dists"], t["g_pred"], t["size"])
        _CASES[(shape, extremes)] = (t, dc.head_grads(*args, dtype=torch.float64), dc.head_grads(*args, dtype=torch.float32))
    return _CASES[(shape, extremes)]


def _gpu(t, need=(True, True), want_prob=True):
    """The op and its backward for the cotangent of `t`; a gradient that is not needed comes back as None."""
    c, u = (t[k].to(DEV).requires_grad_(n) for k, n in zip(("cost", "foc_dists"), need))
    pred, std, prob = torch.ops.aadff.dfv_regress(c, u, *t["size"], want_prob)
    assert not std.requires_grad and not prob.requires_grad
    if any(need):
        pred.backward(t["g_pred"].to(DEV))
    torch.cuda.synchronize()
    cpu = lambda v: None if v is None else v.detach().cpu()                        # noqa: E731
    return {"pred": cpu(pred), "std": cpu(std), "prob": cpu(prob), "d_cost": cpu(c.grad), "d_foc_dists": cpu(u.grad)}


def _budget(margin, name, got, f64, f32, factor=4.0):
    err, d32 = dc.rel_l2(got, f64), dc.rel_l2(f32, f64)
    print(f"{name}: error {err:.3e}, d32 {d32:.3e}")
    if d32 == 0.0:
        assert err == 0.0, f"{name}: the float32 oracle is exact, the kernel is {err:.3e} off"
    else:
        margin(name, err, factor * d32)


def _check(margin, tag, t, f64, f32):
    got = _gpu(t)
    B, S, h, w = t["cost"].shape
    H, W = t["size"]
    assert got["pred"].shape == got["std"].shape == (B, 1, H, W) and got["prob"].shape == (B, S, H, W)
    assert got["d_cost"].shape == (B, S, h, w) and got["d_foc_dists"].shape == (B, S)
    for k in KEYS:
        assert got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k
        _budget(margin, f"{tag} {k}", got[k], f64[k], f32[k])
    return got


@pytest.mark.parametrize("shape", SHAPES, ids=IDS)
def test_against_the_oracle(shape, margin):
    t, f64, f32 = _case(shape)
    _check(margin, f"dfv head {IDS[SHAPES.index(shape)]}", t, f64, f32)


def test_extreme_costs_stay_finite_and_within_budget(margin):
    t, f64, f32 = _case(RATIO4, extremes=True)
    assert sorted(v for v in t["cost"].flatten().tolist() if abs(v) >= 79) == sorted(dc.EXTREMES)
    got = _check(margin, "dfv head 9x19_to_36x76 costs of +-80, +-1e4", t, f64, f32)
    assert float(got["prob"].max()) == 1.0 and float(got["prob"].min()) == 0.0        # a cell of +-1e4 decides its pixels alone


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "g20_dfv_head.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else z[k]) for k in z.files}


@pytest.mark.parametrize("i", range(3))
def test_against_the_reference_golden(gold, i, margin):
    mode, _, _, H, W = str(gold["cases"][i]).split("|")
    t = {"cost": gold[f"case{i}_cost"], "foc_dists": gold["foc_dists"], "g_pred": gold[f"case{i}_g_pred"], "size": (int(H), int(W))}
    args = (t["cost"], t["foc_dists"], t["g_pred"], t["size"])
    f64, f32 = dc.head_grads(*args, dtype=torch.float64), dc.head_grads(*args, dtype=torch.float32)
    got = _gpu(t, want_prob=False)
    assert got["prob"].numel() == 0
    for k in ("pred", "std", "d_cost", "d_foc_dists"):
        err, d32 = dc.rel_l2(got[k], gold[f"case{i}_{k}"]), dc.rel_l2(f32[k], f64[k])
        print(f"golden case {i} {mode} {k}: kernel vs reference {err:.3e}, d32 {d32:.3e}")
        margin(f"dfv head golden case{i} {mode} {k}", err, 5.0 * d32)


@pytest.mark.parametrize("shape", [(2, 1, 1, 1, 1, 1), (2, 1, 9, 13, 37, 54), (1, 1, 3, 4, 96, 128)], ids=["1x1", "37x54", "ratio32"])
def test_one_slice_is_exact(shape):
    t = dc.head_inputs(*shape, seed=3)
    B, S, h, w, H, W = shape
    got = _gpu(t)
    assert torch.equal(got["pred"], t["foc_dists"].reshape(B, 1, 1, 1).expand(B, 1, H, W))
    assert bool((got["std"] == 0).all()) and bool((got["prob"] == 1).all())
    assert bool((got["d_cost"] == 0).all()) and got["d_cost"].shape == (B, 1, h, w)


@pytest.mark.parametrize("shape", [ODD, RATIO32], ids=[IDS[5], IDS[8]])
def test_runs_repeat_bit_for_bit(shape):
    t, _, _ = _case(shape)
    first, again = _gpu(t), _gpu(t)
    assert all(torch.equal(first[k], again[k]) for k in KEYS)


@pytest.mark.parametrize("shape", [ODD, SHAPES[7], RATIO32], ids=[IDS[5], IDS[7], IDS[8]])
def test_skipped_gradients_and_probabilities_change_nothing(shape):
    t, _, _ = _case(shape)
    full = _gpu(t)
    for need in ((True, False), (False, True), (False, False)):
        got = _gpu(t, need, want_prob=False)
        assert torch.equal(got["pred"], full["pred"]) and torch.equal(got["std"], full["std"]) and got["prob"].numel() == 0
        for k, n in zip(("d_cost", "d_foc_dists"), need):
            assert torch.equal(got[k], full[k]) if n else got[k] is None, (k, need)


def test_offsets_past_2_to_the_31_elements():
    """cost, prob, the backward's row sums and d_cost of 2 x 17 x 8192^2 = 2.3e9 elements each (9.1 GB): the second batch item ends past
    element 2^31, where a 32-bit offset wraps, the first lies below it.  Both items get the same inputs, drawn on the device, so every
    output of the second must equal that of the first bit for bit."""
    B, S, n = 2, 17, 8192
    assert B * S * n * n >= 2 ** 31 > S * n * n
    g = torch.Generator(device=DEV).manual_seed(9)
    cost = torch.randn(1, S, n, n, device=DEV, generator=g).mul_(2.0).expand(B, S, n, n).contiguous().requires_grad_(True)
    u = torch.rand(1, S, device=DEV, generator=g).add_(0.5).expand(B, S).contiguous().requires_grad_(True)
    gp = torch.randn(1, 1, n, n, device=DEV, generator=g).expand(B, 1, n, n).contiguous()
    pred, std, prob = torch.ops.aadff.dfv_regress(cost, u, n, n, True)
    pred.backward(gp)
    torch.cuda.synchronize()
    for name, v in (("pred", pred), ("std", std), ("prob", prob), ("d_cost", cost.grad), ("d_foc_dists", u.grad)):
        assert torch.equal(v[0], v[1]), name
    assert bool(torch.isfinite(cost.grad[1, -1]).all()) and float(cost.grad[1, -1].abs().max()) > 0
    assert float(pred.detach().min()) >= 0.5 - 1e-6 and float(pred.detach().max()) <= 1.5 + 1e-6
    assert float((prob[1].sum(0) - 1).abs().max()) < 1e-5
    del cost, prob, pred, std
    torch.cuda.empty_cache()


def test_public_function_devices_dtypes_module_and_levels(margin):
    t, _, _ = _case(ODD)
    want = _gpu(t)
    size = t["size"]
    # float64, non-contiguous input on the CPU: converted, results and gradients on the CPU, in the inputs' dtypes and layouts
    c = t["cost"].double().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    u = t["foc_dists"].double().requires_grad_(True)
    assert not c.is_contiguous()
    pred, std, prob = cost_volume_depth(c, u, size, return_prob=True)
    assert pred.device.type == std.device.type == prob.device.type == "cpu" and pred.dtype == std.dtype == prob.dtype == torch.float32
    assert not std.requires_grad and not prob.requires_grad
    pred.backward(t["g_pred"])
    assert torch.equal(pred, want["pred"]) and torch.equal(std, want["std"]) and torch.equal(prob, want["prob"])
    assert c.grad.dtype == torch.float64 and torch.equal(c.grad.float(), want["d_cost"]) and torch.equal(u.grad.float(), want["d_foc_dists"])
    # the 5-D cost the reference gives its trilinear call, on the device, through the module
    head = CostVolumeHead(size=size)
    p5, s5 = head(t["cost"][:, None].to(DEV), t["foc_dists"].to(DEV))
    assert p5.device == torch.device(DEV) and torch.equal(p5.cpu(), want["pred"]) and torch.equal(s5.cpu(), want["std"])
    # [S] focus distances for B == 1, size None: the cost's own resolution
    t1, _, _ = _case(RATIO32)
    p1, s1 = cost_volume_depth(t1["cost"].to(DEV), t1["foc_dists"][0].to(DEV), t1["size"])
    assert torch.equal(p1.cpu(), _gpu(t1)["pred"])
    p0, s0 = cost_volume_depth(t1["cost"].to(DEV), t1["foc_dists"].to(DEV))
    assert p0.shape == s0.shape == (1, 1, 3, 4)
    # two levels, as the training branch returns them
    coarse = torch.nn.functional.avg_pool2d(t["cost"], 2)
    preds, stds = cost_volume_depth_levels([t["cost"].to(DEV), coarse.to(DEV)], t["foc_dists"].to(DEV), size)
    assert len(preds) == len(stds) == 2 and all(v.shape == (2, 1, *size) for v in preds + stds)
    assert torch.equal(preds[0].cpu(), want["pred"]) and torch.equal(stds[0].cpu(), want["std"])
    f64, f32 = (dc.head_grads(coarse, t["foc_dists"], t["g_pred"], size, dtype=d) for d in (torch.float64, torch.float32))
    _budget(margin, "dfv head levels, second level pred", preds[1], f64["pred"], f32["pred"])
    _budget(margin, "dfv head levels, second level std", stds[1], f64["std"], f32["std"])


def test_opcheck():
    t, _, _ = _case(ODD)
    c, u, g = t["cost"].to(DEV), t["foc_dists"].to(DEV), t["g_pred"].to(DEV)
    utils = ("test_schema", "test_faketensor")
    for want_prob in (False, True):
        torch.library.opcheck(torch.ops.aadff.dfv_regress.default, (c, u, *t["size"], want_prob), test_utils=utils)
    for need in ((True, True), (False, True), (True, False)):
        torch.library.opcheck(torch.ops.aadff.dfv_regress_bwd.default, (c, u, g, *need), test_utils=utils)
