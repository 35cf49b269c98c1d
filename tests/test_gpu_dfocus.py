"""GPU tests (run with `-m gpu` on an MI355X) of the fused depth-from-focus kernel (csrc/dfocus.hip) through
torch.ops.aadff.depth_from_stack and aadff.dfocus.depth_from_stack, against the torch CPU oracle of tests/dfocus_common.py.

The bounds are derived, not tuned:
  volume  window 1: bit-equal (ML is exactly rounded operation by operation).  Otherwise |F_k - F_o| <= n 2^-24 F_o, n = window^2: any
          order of a float32 sum of n non-negative terms is within (n - 1) 2^-24 relative of the exact sum.
  index   the first argmax of the kernel's own volume, exactly; peak and aif are bit-equal gathers at it.
  depth   against the float64 fit on the kernel's own volume: |d| <= k 2^-24 max(|h-|, |h+|) + 2^-23 |u*|.  none: exactly u0.
          parabola: k = 16 (about six rounded operations, no cancelling denominator).  gaussian: k = GAUSS_K below.
Shapes: the tile is 32 x 64, so 37 x 70 and 37 x 76 have two tiles in each direction with ragged remainders; a width of 70 takes the
scalar access path, 76 the 16-byte one; 1 x 1 ... 3 x 3 are smaller than the window and the halo.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import dfocus_common as dc                                   # noqa: E402
from aadff import ops  # noqa: E402,F401
from aadff.dfocus import depth_from_stack                    # noqa: E402

DEV = "cuda:0"
EPS = 1e-8
U24 = 2.0 ** -24
PARABOLA_K = 16.0
# device log1pf: measured on the cases below (MI355X), |depth - float64 fit| never exceeds the output-rounding term 2^-23 |u*| alone
# - the excess over it is 0.00 in units of 2^-24 max(|h-|, |h+|) - and the largest error is 28 % of the bound with k = 16; four times
# the measured excess is below the floor of 16.
GAUSS_K = 16.0

# (N, C, S, H, W, window)
CASES = [(2, 1, 1, 1, 1, 1), (2, 3, 3, 1, 1, 9),
         (2, 4, 2, 1, 7, 3), (2, 3, 8, 1, 7, 9),
         (2, 1, 8, 5, 1, 3), (2, 4, 3, 5, 1, 9),
         (2, 3, 2, 3, 3, 1), (2, 1, 3, 3, 3, 9), (2, 4, 8, 3, 3, 3),
         (2, 3, 8, 37, 70, 9), (2, 1, 3, 37, 70, 1), (2, 4, 2, 37, 70, 3),
         (2, 3, 8, 37, 76, 9), (2, 4, 1, 37, 76, 3), (2, 1, 8, 37, 76, 1),
         (1, 3, 4, 37, 76, 5), (2, 2, 4, 33, 68, 7)]
IDS = ["%dx%dx%dx%dx%d_w%d" % c for c in CASES]


def _op(stack, coords, window, interp, want_aif=True, want_volume=True):
    out = torch.ops.aadff.depth_from_stack(stack.to(DEV), coords.to(DEV), window, interp, EPS, want_aif, want_volume)
    torch.cuda.synchronize()
    return [t.cpu() for t in out]


_INPUTS = {}


def _inputs(case):
    """Seeded stack and coords of a case with the oracle's float64 focus volume (cached, read-only)."""
    if case not in _INPUTS:
        N, C, S, H, W, window = case
        stack, coords = dc.random_stack(N, C, S, H, W, seed=100 + CASES.index(case)), dc.random_coords(N, S, seed=7)
        _INPUTS[case] = (stack, coords, dc.focus_volume(stack, window)[1])
    return _INPUTS[case]


def _check_depth(tag, depth, vol, coords, index, interp, margin):
    """depth against the float64 fit on the kernel's volume; returns the excess over the output rounding in units of 2^-24 max|h|."""
    fit = dc.peak_fit(vol, coords, interp, EPS)
    assert torch.equal(fit["index"], index)
    if interp == "none":
        N, S = coords.shape
        u0 = coords.reshape(N, S, 1, 1).expand(N, S, *depth.shape[-2:]).gather(1, index.to(torch.int64))
        assert torch.equal(depth, u0)
        return 0.0
    k = PARABOLA_K if interp == "parabola" else GAUSS_K
    h = torch.maximum(fit["hm"].abs(), fit["hp"].abs())
    delta = (depth.double() - fit["u"]).abs()
    tol = k * U24 * h + 2.0 * U24 * fit["u"].abs()
    S = coords.shape[1]
    if S == 1:                                                # no neighbour: h = 0 and the depth is u0 exactly
        assert float(delta.max()) == 0.0
        return 0.0
    excess = float(((delta - 2.0 * U24 * fit["u"].abs()).clamp(min=0) / (U24 * h).clamp(min=1e-300)).max())
    print(f"{tag} {interp}: largest excess over the output rounding {excess:.2f} x 2^-24 max|h| (k = {k:.0f})")
    margin(f"dfocus depth {tag} {interp}", float((delta / tol).max()), 1.0)
    return excess


@pytest.mark.parametrize("case", CASES, ids=IDS)
def test_against_the_oracle(case, margin):
    N, C, S, H, W, window = case
    stack, coords, vol_o = _inputs(case)
    tag = IDS[CASES.index(case)]
    ref = None
    for interp in dc.INTERPS:
        depth, index, peak, aif, vol = _op(stack, coords, window, interp)
        assert depth.shape == index.shape == peak.shape == (N, 1, H, W) and aif.shape == (N, C, H, W) and vol.shape == (N, S, H, W)
        assert index.dtype == torch.int32 and depth.dtype == peak.dtype == aif.dtype == vol.dtype == torch.float32
        # 1. the focus volume
        if window == 1:
            assert torch.equal(vol.double(), vol_o)
        else:
            n = window * window
            worst = float(((vol.double() - vol_o).abs() / (n * U24 * vol_o).clamp(min=1e-300)).max())
            if interp == "none":
                margin(f"dfocus volume {tag}", worst, 1.0)
            assert worst <= 1.0
        # 2. index, peak and aif follow from the kernel's own volume, on every pixel
        assert torch.equal(index.to(torch.int64), dc.first_argmax(vol))
        assert torch.equal(peak, vol.gather(1, index.to(torch.int64)))
        assert torch.equal(aif, dc.gather_aif(stack, index))
        # 3. the fit
        _check_depth(tag, depth, vol, coords, index, interp, margin)
        # the interpolation changes nothing but depth
        if ref is None:
            ref = (index, peak, aif, vol)
        else:
            assert all(torch.equal(a, b) for a, b in zip(ref, (index, peak, aif, vol)))


@pytest.mark.parametrize("case", [CASES[8], CASES[9], CASES[12]], ids=[IDS[8], IDS[9], IDS[12]])
def test_optional_outputs_change_nothing_and_runs_repeat(case):
    N, C, S, H, W, window = case
    stack, coords, _ = _inputs(case)
    full = _op(stack, coords, window, "gaussian")
    again = _op(stack, coords, window, "gaussian")
    assert all(torch.equal(a, b) for a, b in zip(full, again))
    for want_aif, want_volume in ((False, False), (True, False), (False, True)):
        got = _op(stack, coords, window, "gaussian", want_aif, want_volume)
        assert all(torch.equal(a, b) for a, b in zip(full[:3], got[:3]))
        assert torch.equal(got[3], full[3]) if want_aif else got[3].shape == (0,)
        assert torch.equal(got[4], full[4]) if want_volume else got[4].shape == (0,)


@pytest.mark.parametrize("shape", [(2, 3, 4, 3, 3), (2, 3, 5, 37, 76)], ids=["3x3", "37x76"])
def test_constant_image(shape):
    N, C, S, H, W = shape
    stack = torch.full(shape, 0.3)
    stack[1] = 0.7
    coords = dc.random_coords(N, S, seed=3)
    for interp in dc.INTERPS:
        depth, index, peak, aif, vol = _op(stack, coords, 9, interp)
        assert (vol == 0).all() and (index == 0).all() and (peak == 0).all()
        assert torch.equal(depth, coords[:, 0].reshape(N, 1, 1, 1).expand(N, 1, H, W))
        assert torch.equal(aif, stack[:, :, 0])


@pytest.mark.parametrize("where", ["first", "last"])
def test_peak_at_an_end_of_the_stack(where):
    N, C, S, H, W = 2, 3, 5, 37, 70
    stack = dc.random_stack(N, C, S, H, W, seed=41)
    k = 0 if where == "first" else S - 1
    stack[:, :, k] *= 16.0                                    # F scales with the image: slice k wins everywhere
    coords = dc.random_coords(N, S, seed=5)
    for interp in dc.INTERPS:
        depth, index, peak, aif, vol = _op(stack, coords, 3, interp)
        assert (index == k).all()
        assert torch.equal(depth, coords[:, k].reshape(N, 1, 1, 1).expand(N, 1, H, W))      # no fit at an end: exactly u0
        assert torch.equal(aif, stack[:, :, k]) and torch.equal(peak, vol[:, k:k + 1])


@pytest.mark.parametrize("window", [5, 9])
def test_built_stack_recovery(window, margin):
    """The recovery fixture: its smallest top-two margin of F is 9.7e-4 relative, a hundred times the volume bound, so the kernel's
    index is the oracle's on every pixel; the median error is <= 0.5 slice spacings for both fits, gaussian below parabola."""
    stack, coords, truth = dc.built_stack()
    med = {}
    for interp in ("parabola", "gaussian"):
        o = dc.oracle(stack, coords, window, interp, EPS)
        depth, index, peak, aif, vol = _op(stack, coords, window, interp)
        assert torch.equal(index, o["index"])
        assert torch.equal(aif, o["aif"])
        _check_depth(f"built_w{window}", depth, vol, coords, index, interp, margin)
        err, _ = dc.recovery_error(depth, peak, coords, truth)
        med[interp] = float(err.median())
        print(f"built stack window {window} {interp}: median {med[interp]:.3f} p90 {float(err.quantile(0.9)):.3f} slice spacings")
        assert med[interp] <= 0.5
    assert med["gaussian"] < med["parabola"]


def test_public_function_spaces_devices_and_dtypes():
    N, C, S, H, W = 2, 3, 6, 37, 70
    stack = dc.random_stack(N, C, S, H, W, seed=77)
    fd = -1.0 / dc.random_coords(N, S, seed=9).double()       # row 0 negative, row 1 positive focus distances, float64
    fd32 = fd.to(torch.float32)
    for interp in dc.INTERPS:
        u, index, peak, aif, vol = _op(stack, 1.0 / fd32, 9, interp)
        got = depth_from_stack(stack.to(DEV), fd.to(DEV), window=9, interp=interp, return_volume=True)
        assert got.depth.device == got.volume.device == torch.device(DEV) and not got.depth.requires_grad
        assert torch.equal(got.depth.cpu(), (1.0 / u.to(DEV)).cpu()) and torch.equal(got.index.cpu(), index) and torch.equal(got.peak.cpu(), peak)
        assert torch.equal(got.aif.cpu(), aif) and torch.equal(got.volume.cpu(), vol)
        assert bool((got.depth[0] < 0).all()) and bool((got.depth[1] > 0).all())             # the sign convention is kept
        lin, index_l, *_ = _op(stack, fd32, 9, interp)
        got = depth_from_stack(stack.to(DEV), fd32, window=9, interp=interp, space="linear")
        assert torch.equal(got.depth.cpu(), lin) and torch.equal(got.index.cpu(), index_l) and got.volume.shape == (0,)
    # defaults; float64, non-contiguous input on the CPU: converted, results on the CPU
    u, index, peak, aif, vol = _op(stack, 1.0 / fd32, 9, "gaussian")
    x = stack.double().permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3).requires_grad_(True)
    assert not x.is_contiguous()
    got = depth_from_stack(x, fd)
    assert all(t.device.type == "cpu" for t in got) and not got.depth.requires_grad
    assert torch.equal(got.depth, (1.0 / u.to(DEV)).cpu()) and torch.equal(got.aif, aif) and got.volume.shape == (0,)
    one = depth_from_stack(stack[:1], fd[0])                  # [S] for N == 1
    assert torch.equal(one.depth, got.depth[:1])


def test_opcheck():
    stack, coords = dc.random_stack(2, 3, 4, 9, 12, seed=1).to(DEV), dc.random_coords(2, 4, seed=2).to(DEV)
    for args in ((9, "gaussian", EPS, True, True), (3, "none", EPS, False, False), (1, "parabola", EPS, True, False)):
        torch.library.opcheck(torch.ops.aadff.depth_from_stack.default, (stack, coords, *args), test_utils=("test_schema", "test_faketensor"))
