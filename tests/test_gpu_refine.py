"""GPU tests (run with `-m gpu` on an MI355X) of the confidence-guided depth refinement (csrc/depth_refine.hip) through
torch.ops.aadff.depth_refine and aadff.refine, against the torch CPU oracle of tests/refine_common.py evaluated in float64 on the same
float32 inputs.

Forward, on the pixels with D > 0: |u'_k - u'_o| <= K 2^-24 (sum w c |u| / D) and |c'_k - c'_o| <= K 2^-24 c'_o with K = n + 4 * 64 + 8,
n = (2r+1)^2: n for any order of an n-term float32 sum; 4 * 64 because the argument of the exponential carries about four roundings
and its absolute error, at most at the clamp of -64, becomes the relative error of the weight; 8 for expf, the products and the
division.  On the cases below the float32 CPU composition and the kernel both use 2 .. 23 of these units, 27 (u') and 67 (c') with most weights at
the clamp; the figures go through `margin`.  Pass-through pixels (D = 0) are the input bit
for bit and their c' is exactly 0.

Backward: per gradient tensor max |difference| / max |float64 gradient| against float64 autograd of the oracle; the yardstick is the
same figure of the float32 CPU oracle's own autograd on the same inputs, computed here, and the kernel may use 4 x that (another expf,
another summation order).  Every (figure, budget) pair goes through the `margin` fixture.

Shapes (N, C, H, W, r) against the kernels' 16 x 64 tile (a wave owns 4 rows of it, a lane one column; templates for r <= 4 and r <= 8
and for every C):
  * 37 x 70 and 37 x 76: 3 x 2 tiles per image, the last row of tiles 5 rows high (one ragged wave and three idle ones), the last
    column 6 or 12 wide; W % 4 != 0 and W % 4 == 0;
  * 1 x 1, 1 x 7, 5 x 1, 3 x 3 at r 8: images smaller than the window, every tap clipped;
  * N 2 throughout (the second image's offsets), C in {1, 2, 3, 4}, r in {1, 4, 8}, and r 2 and 5 for the templates' inner range;
  * the confidence has about 30 % exact zeros, a value below 2^-30 and a block of zeros of (2r+4)^2 that crosses the tile boundary at
    x = 64 and y = 16 and touches the right border: its middle passes through on the device; the forward cases put nan (and an inf)
    into u under a part of it;
  * a guide of 3 x the range in one case drives most arguments into the clamp;
  * one case has 2^31 + 4 M pixels: offsets past 2^31 (and past 2^32 in the backward's workspace) show only there.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import refine_common as rc                                   # noqa: E402
from aadff import ops  # noqa: E402,F401
from aadff.refine import DepthRefiner, RefinedDepth, confidence_from_peak, refine_depth      # noqa: E402

DEV = "cuda:0"
SS, SR = 2.0, 0.1                                             # sigma_space, sigma_range of the cases
CASES = [(2, 3, 37, 70, 4), (2, 3, 37, 76, 4), (2, 1, 37, 70, 1), (2, 4, 37, 70, 8), (2, 1, 37, 76, 8), (2, 4, 37, 76, 1),
         (2, 2, 37, 70, 2), (2, 3, 37, 70, 5), (2, 1, 1, 1, 8), (2, 3, 1, 7, 8), (2, 4, 5, 1, 8), (2, 3, 3, 3, 8)]
IDS = ["N%d_C%d_%dx%d_r%d" % s for s in CASES]
ODD, WIDE = CASES[0], CASES[3]

_CACHE = {}


def _k(radius):
    return (2 * radius + 1) ** 2 + 4 * 64 + 8


def _case(case, nan, guide_scale=1.0):
    """Seeded inputs of a case with the oracle in float64 and float32 (cached, read-only)."""
    key = (case, nan, guide_scale)
    if key not in _CACHE:
        N, C, H, W, r = case
        t = rc.case_inputs(N, C, H, W, r, seed=40 + CASES.index(case), nan=nan, guide_scale=guide_scale)
        ks, kr = rc.constants(C, SS, SR)
        o = {d: rc.refine_step(t["u"], t["c"], t["g"], r, ks, kr, d) for d in (torch.float64, torch.float32)}
        g = None if nan else {d: rc.grads(t["u"], t["c"], t["g"], r, ks, kr, t["g_u"], t["g_c"], d) for d in (torch.float64, torch.float32)}
        _CACHE[key] = (t, o, g)
    return _CACHE[key]


def _gpu(t, r, need=(True, True), backward=True):
    u, c = (t[k].to(DEV).requires_grad_(n and backward) for k, n in zip(("u", "c"), need))
    uo, co = torch.ops.aadff.depth_refine(u, c, t["g"].to(DEV), r, SS, SR)
    out = {"u": uo.detach().cpu(), "c": co.detach().cpu(), "d_u": None, "d_c": None}
    if backward and any(need):
        torch.autograd.backward((uo, co), (t["g_u"].to(DEV), t["g_c"].to(DEV)))
        out["d_u"], out["d_c"] = (None if v.grad is None else v.grad.cpu() for v in (u, c))
    torch.cuda.synchronize()
    return out


def _forward_check(margin, tag, t, o, got, r):
    o64, o32 = o[torch.float64], o[torch.float32]
    some = o64["some"]
    assert torch.equal(some, o32["some"])
    assert got["u"].dtype == got["c"].dtype == torch.float32 and got["u"].shape == got["c"].shape == t["u"].shape
    # pass-through: the input bit for bit (nan compared as bits), c' exactly 0
    assert torch.equal(got["u"][~some].view(torch.int32), t["u"][~some].view(torch.int32)) and bool((got["c"][~some] == 0).all())
    if not bool(some.any()):
        return
    assert bool(torch.isfinite(got["u"][some]).all()) and bool((got["c"][some] > 0).all())
    unit_u, unit_c = 2.0 ** -24 * o64["scale"][some], 2.0 ** -24 * o64["c"][some]
    for name, res in (("kernel", got), ("float32 oracle", o32)):
        eu = float(((res["u"].double() - o64["u"])[some].abs() / unit_u).max())
        ec = float(((res["c"].double() - o64["c"])[some].abs() / unit_c).max())
        print(f"{tag}: {name} uses {eu:.1f} (u') and {ec:.1f} (c') of K = {_k(r)} units")
        if name == "kernel":
            margin(f"{tag} u' [units of 2^-24 scale]", eu, _k(r))
            margin(f"{tag} c' [units of 2^-24 c']", ec, _k(r))


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_forward_against_the_oracle(case, margin):
    t, o, _ = _case(case, nan=True)
    if case[2] >= 2 * case[4] + 4:
        assert int((~o[torch.float64]["some"]).sum()) >= 2 * 16 and bool(torch.isnan(t["u"]).any())   # pass-through runs on the device
    _forward_check(margin, f"refine {IDS[CASES.index(case)]}", t, o, _gpu(t, case[4], backward=False), case[4])


def test_forward_with_most_weights_at_the_clamp(margin):
    t, o, _ = _case(ODD, nan=True, guide_scale=3.0)
    _forward_check(margin, "refine N2_C3_37x70_r4, guide x 3", t, o, _gpu(t, ODD[4], backward=False), ODD[4])


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_backward_against_the_oracle(case, margin):
    t, o, g = _case(case, nan=False)
    got = _gpu(t, case[4])
    _forward_check(margin, f"refine {IDS[CASES.index(case)]} finite u", t, o, got, case[4])
    for k in ("d_u", "d_c"):
        g64, g32 = g[torch.float64][k], g[torch.float32][k]
        assert got[k].shape == g64.shape and got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all())
        top = float(g64.abs().max())
        err, d32 = float((got[k].double() - g64).abs().max()), float((g32.double() - g64).abs().max())
        if top > 0:
            err, d32 = err / top, d32 / top
        print(f"refine {IDS[CASES.index(case)]} {k}: kernel {err:.3e}, float32 autograd {d32:.3e} of max |g64| = {top:.3e}")
        if d32 == 0.0:
            assert err == 0.0, f"{k}: the float32 oracle is exact, the kernel is {err:.3e} off"
        else:
            margin(f"refine {IDS[CASES.index(case)]} {k}", err, 4.0 * d32)
    some = o[torch.float64]["some"]
    assert torch.equal(got["d_u"][~some], t["g_u"][~some])                          # [D = 0] gu', as it is


@pytest.mark.parametrize("case", [ODD, WIDE], ids=[IDS[0], IDS[3]])
def test_runs_repeat_bit_for_bit(case):
    t, _, _ = _case(case, nan=False)
    first, again = _gpu(t, case[4]), _gpu(t, case[4])
    assert all(torch.equal(first[k], again[k]) for k in ("u", "c", "d_u", "d_c"))


@pytest.mark.parametrize("case", [ODD, WIDE], ids=[IDS[0], IDS[3]])
def test_a_skipped_gradient_changes_nothing(case):
    t, _, _ = _case(case, nan=False)
    full = _gpu(t, case[4])
    only_u, only_c = _gpu(t, case[4], need=(True, False)), _gpu(t, case[4], need=(False, True))
    assert torch.equal(only_u["d_u"], full["d_u"]) and only_u["d_c"] is None
    assert torch.equal(only_c["d_c"], full["d_c"]) and only_c["d_u"] is None
    assert torch.equal(only_u["u"], full["u"]) and torch.equal(only_c["c"], full["c"])


def test_recovery_fixture_end_to_end():
    fx = rc.recovery_fixture()
    want, _ = rc.refine(fx["inp"], fx["conf"], fx["guide"], **rc.RECOVERY)
    out = refine_depth(fx["inp"], fx["conf"], fx["guide"], space="linear", **rc.RECOVERY)
    assert isinstance(out, RefinedDepth) and out.depth.device.type == "cpu" and out.depth.dtype == torch.float32
    rc.check_recovery(fx, out.depth, "refine_depth, two iterations")
    rc.check_recovery(fx, want, "oracle, two iterations")
    assert float((out.depth.double() - want).abs().max()) <= 1e-5                  # (values near 2: a few hundred float32 roundings)
    assert float(out.confidence.min()) > 0 and float(out.confidence.max()) <= 1


def test_inverse_space_layouts_devices_and_module():
    t, _, _ = _case(ODD, nan=False)
    r = ODD[4]
    depth = -1.0 / (t["u"].abs() + 0.2)                                             # negative depths, as the renderers use them
    kw = dict(radius=r, sigma_space=SS, sigma_range=SR, iterations=2)
    by_hand = refine_depth(1.0 / depth, t["c"], t["g"], space="linear", **kw)
    out = refine_depth(depth, t["c"], t["g"], space="inverse", **kw)
    assert torch.equal(out.depth, 1.0 / by_hand.depth) and torch.equal(out.confidence, by_hand.confidence)
    assert bool((out.depth < 0).all())
    # float64, non-contiguous inputs on the CPU: converted; results on the CPU, gradients in the inputs' dtypes and layouts
    d = depth.double().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    c = t["c"].double().permute(0, 1, 3, 2).contiguous().permute(0, 1, 3, 2).requires_grad_(True)
    g = t["g"].permute(0, 2, 3, 1).contiguous().permute(0, 3, 1, 2).requires_grad_(True)
    assert not d.is_contiguous() and not c.is_contiguous() and not g.is_contiguous()
    again = refine_depth(d, c, g, space="inverse", **kw)
    assert torch.equal(again.depth, out.depth) and torch.equal(again.confidence, out.confidence) and again.depth.device.type == "cpu"
    (again.depth.sum() + again.confidence.sum()).backward()
    assert d.grad.dtype == torch.float64 and d.grad.shape == d.shape and bool(torch.isfinite(d.grad).all()) and float(d.grad.abs().max()) > 0
    assert c.grad.shape == c.shape and bool(torch.isfinite(c.grad).all()) and g.grad is None   # the guide is a constant
    # on the device through the module; sigma_space defaults to radius / 2 = SS here; zero iterations return the input
    m = DepthRefiner(radius=r, sigma_range=SR, iterations=2, space="inverse")
    on = m(depth.to(DEV), t["c"].to(DEV), t["g"].to(DEV))
    assert on.depth.device == torch.device(DEV) and torch.equal(on.depth.cpu(), out.depth)
    same = refine_depth(depth, t["c"], t["g"], iterations=0, space="linear")
    assert torch.equal(same.depth, depth) and torch.equal(same.confidence, t["c"])
    conf = confidence_from_peak(t["c"].to(DEV))
    assert conf.device == torch.device(DEV) and float(conf.max()) < 1


def test_two_iterations_backward_against_the_oracle(margin):
    """The Python loop of refine_depth: gradients through two chained iterations, against float64 autograd of two oracle iterations."""
    N, C, H, W, r = ODD
    t, _, _ = _case(ODD, nan=False)
    res = {}
    for dtype in (torch.float64, torch.float32):
        u, c = t["u"].to(dtype).clone().requires_grad_(True), t["c"].to(dtype).clone().requires_grad_(True)   # (the case is shared)
        uo, co = rc.refine(u, c, t["g"].to(dtype), r, SS, SR, 2, dtype)
        res[dtype] = torch.autograd.grad((uo, co), (u, c), (t["g_u"].to(dtype), t["g_c"].to(dtype)))
    u, c = t["u"].clone().requires_grad_(True), t["c"].clone().requires_grad_(True)
    out = refine_depth(u, c, t["g"], r, SS, SR, 2, "linear")
    torch.autograd.backward((out.depth, out.confidence), (t["g_u"], t["g_c"]))
    for name, got, g64, g32 in zip(("d_u", "d_c"), (u.grad, c.grad), res[torch.float64], res[torch.float32]):
        top = float(g64.abs().max())
        margin(f"refine two iterations {name}", float((got.double() - g64).abs().max()) / top, 4.0 * float((g32.double() - g64).abs().max()) / top)


def test_offsets_past_2_to_the_31_pixels():
    """u, c, g, both outputs and both gradients of 2 x 32768 x 32832 = 2^31 + 4.2 M elements each (8.6 GB), the backward's workspace
    four times that: the end of the second image lies past element 2^31, where a 32-bit offset wraps, and three of the workspace's
    planes past 2^32.  Both images get the same inputs, drawn on the device, so every output of the second must equal that of the first."""
    N, H, W = 2, 32768, 32832
    assert N * H * W > 2 ** 31 > H * W
    gen = torch.Generator(device=DEV).manual_seed(9)
    u = torch.randn(1, 1, H, W, device=DEV, generator=gen).expand(N, 1, H, W).contiguous().requires_grad_(True)
    c = torch.rand(1, 1, H, W, device=DEV, generator=gen).expand(N, 1, H, W).contiguous().requires_grad_(True)
    g = torch.rand(1, 1, H, W, device=DEV, generator=gen).expand(N, 1, H, W).contiguous()
    uo, co = torch.ops.aadff.depth_refine(u, c, g, 1, 1.0, 0.5)
    torch.autograd.backward((uo, co), (uo.detach(), co.detach()))                  # the outputs as their own cotangents: no more memory
    torch.cuda.synchronize()
    for name, v in (("u'", uo), ("c'", co), ("d_u", u.grad), ("d_c", c.grad)):
        assert torch.equal(v[0], v[1]), name
        assert bool(torch.isfinite(v[1, 0, -1]).all()) and float(v[1, 0, -1].abs().max()) > 0, name
    assert float(co.detach().min()) > 0 and float(co.detach().max()) < 1
    del u, c, g, uo, co
    torch.cuda.empty_cache()


def test_opcheck():
    t, _, _ = _case(ODD, nan=False)
    u, c, g, gu, gc = (t[k].to(DEV) for k in ("u", "c", "g", "g_u", "g_c"))
    utils = ("test_schema", "test_faketensor")
    torch.library.opcheck(torch.ops.aadff.depth_refine.default, (u, c, g, ODD[4], SS, SR), test_utils=utils)
    for need in ((True, True), (False, True), (True, False)):
        torch.library.opcheck(torch.ops.aadff.depth_refine_bwd.default, (u, c, g, gu, gc, ODD[4], SS, SR, *need), test_utils=utils)
