"""CPU: the host side of the confidence-guided depth refinement (csrc/depth_refine.hip, aadff/ops.py, aadff/refine.py) - the oracle of
tests/refine_common.py against the properties of the specification, the closed-form gather backward against float64
autograd, the recovery fixture, every argument error of the two C entries and of the public functions without a GPU, the fake-tensor
shapes of the ops and the empty results.

Recovery fixture, oracle in float64, measured with this file's generator calls (mean |error|):
    raw input   low-confidence 0.3965   confident 0.0163
    refined     low-confidence 0.0048   confident 0.0031   the four columns around the step 0.0070
Conditions: low <= 0.05 x raw, confident <= raw, step band <= 0.02."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import refine_common as rc
from aadff import _abi, ops, refine

P8, P16, P24, P32, P40 = (C.c_void_p(8 * i) for i in range(1, 6))   # non-NULL pointers that are never dereferenced: validation comes first
ENTRIES = ("aadff_depth_refine_fwd", "aadff_depth_refine_bwd")


@pytest.fixture(scope="module")
def small():
    """11 x 13, r 2, C 2, a 6 x 6 block of zero confidence: larger than the 5 x 5 window, so the 2 x 2 pixels in its middle pass
    through; every other confidence is at least 0.05; finite u."""
    gen = torch.Generator().manual_seed(5)
    u = torch.randn(1, 1, 11, 13, generator=gen, dtype=torch.float64)
    c = torch.rand(1, 1, 11, 13, generator=gen, dtype=torch.float64) + 0.05
    g = torch.rand(1, 2, 11, 13, generator=gen, dtype=torch.float64)
    c[:, :, 3:9, 4:10] = 0
    ks, kr = rc.constants(2, 1.0, 0.3)
    return {"u": u, "c": c, "g": g, "g_u": torch.randn(1, 1, 11, 13, generator=gen, dtype=torch.float64),
            "g_c": torch.randn(1, 1, 11, 13, generator=gen, dtype=torch.float64), "r": 2, "ks": ks, "kr": kr}


def test_closed_form_backward_is_the_autograd_of_the_oracle(small):
    s = small
    o = rc.refine_step(s["u"], s["c"], s["g"], s["r"], s["ks"], s["kr"])
    assert int((~o["some"]).sum()) == 4                                           # the pass-through pixels take part
    want = rc.grads(s["u"], s["c"], s["g"], s["r"], s["ks"], s["kr"], s["g_u"], s["g_c"])
    got = rc.closed_form_backward(s["u"], s["c"], s["g"], s["r"], s["ks"], s["kr"], s["g_u"], s["g_c"])
    for k in ("d_u", "d_c"):
        err = float((got[k] - want[k]).abs().max())
        print(f"closed form {k}: max |difference| to float64 autograd {err:.2e}")
        assert err <= 1e-12, (k, err)
    assert torch.equal(got["d_u"][~o["some"]], s["g_u"][~o["some"]])              # [D = 0] gu'


def test_weights_are_symmetric_and_the_clamp_acts():
    gen = torch.Generator().manual_seed(2)
    g = torch.rand(1, 3, 6, 7, generator=gen, dtype=torch.float64) * 10            # differences far beyond the clamp
    ks, kr = rc.constants(3, 1.0, 0.1)
    floor, lowest = float(torch.exp(torch.tensor(-64.0, dtype=torch.float64))), 1.0
    for dy, dx, P, Q, _ in rc._shifts(6, 7, 2):
        w, wt = rc._weight(g, dy, dx, P, Q, ks, kr), rc._weight(g, -dy, -dx, Q, P, ks, kr)
        assert torch.equal(w, wt) and float(w.float().min()) >= float(np.finfo(np.float32).tiny)
        lowest = min(lowest, float(w.min()))
    assert lowest == floor


def test_constant_depth_is_kept(small):
    """u' = A / D with A = sum w (c u) and D = sum w c: for a constant u the two differ by the rounding of c u, of the products and of two
    sums of the same positive terms in the same order.  Four units of 2^-53 are the bound for the shortest window, the 9 taps of r 1:
    a sequential n-term sum gathers roundings with n, so the longer windows use more (r 2 about 5 units, r 4 about 10)."""
    s = small
    for value in (1.0, -0.37, 3.0e-4):
        o = rc.refine_step(torch.full_like(s["u"], value), s["c"], s["g"], 1, s["ks"], s["kr"])
        assert int(o["some"].sum()) == 11 * 13 - 16                               # the 6 x 6 block leaves 4 x 4 windows without confidence
        rel = ((o["u"] - value).abs() / abs(value))[o["some"]]
        assert float(rel.max()) <= 4 * 2.0 ** -53, float(rel.max())


def test_zero_confidence_passes_through_bit_for_bit(small):
    s = small
    for dtype in (torch.float64, torch.float32):
        u = s["u"].to(dtype)
        o = rc.refine_step(u, torch.zeros_like(s["c"]), s["g"], s["r"], s["ks"], s["kr"], dtype)
        assert torch.equal(o["u"], u) and bool((o["c"] == 0).all()) and not bool(o["some"].any())
    # below the threshold is zero
    o = rc.refine_step(s["u"], torch.full_like(s["c"], 2.0 ** -31), s["g"], s["r"], s["ks"], s["kr"])
    assert torch.equal(o["u"], s["u"]) and bool((o["c"] == 0).all())
    o = rc.refine_step(s["u"], torch.full_like(s["c"], 2.0 ** -30), s["g"], s["r"], s["ks"], s["kr"])
    assert bool(o["some"].all()) and bool((o["c"] > 0).all())


def test_nan_under_zero_confidence_reaches_no_filtered_pixel(small):
    s = small
    u = s["u"].clone()
    u[:, :, 3:9, 4:10] = float("nan")
    u[:, :, 5, 6] = float("inf")
    o, clean = (rc.refine_step(v, s["c"], s["g"], s["r"], s["ks"], s["kr"]) for v in (u, s["u"]))
    some = o["some"]
    assert torch.equal(some, clean["some"]) and bool(torch.isfinite(o["u"][some]).all())
    assert torch.equal(o["u"][some], clean["u"][some]) and torch.equal(o["c"], clean["c"])
    assert bool(torch.isnan(o["u"][~some]).sum() == 3) and bool(torch.isinf(o["u"][~some]).sum() == 1)   # passed through as they are


def test_recovery_fixture():
    fx = rc.recovery_fixture()
    out, conf = rc.refine(fx["inp"], fx["conf"], fx["guide"], **rc.RECOVERY)
    raw, got = rc.check_recovery(fx, out, "oracle, float64")
    assert abs(raw[0] - 0.3965) < 5e-4 and abs(raw[1] - 0.0163) < 5e-4, raw      # the draw the docstring's figures belong to
    assert float(conf.min()) > 0 and float(conf.max()) <= 1
    # a filter that ignores the guide blurs the step and misses the last condition by far
    blurred, _ = rc.refine(fx["inp"], fx["conf"], torch.zeros_like(fx["guide"]), **rc.RECOVERY)
    assert rc.recovery_errors(fx, blurred)[2] > 0.1


def test_symbols_are_exported_bound_and_declared(repo_root):
    lib = C.CDLL(_abi.LIB_PATH)
    header = open(os.path.join(repo_root, "include", "aadff.h")).read()
    for name in ENTRIES:
        assert hasattr(lib, name) and name in _abi.PROTOTYPES
        args = re.search(r"^\s*int\s+%s\s*\(([^;]*)\);" % name, header, flags=re.M | re.S).group(1).split(",")
        assert len(args) == len(_abi.PROTOTYPES[name])                            # as many arguments bound as declared
    assert _abi.load_library().aadff_abi_version() == _abi.ABI_VERSION == 9       # additions only


def test_argument_errors_of_the_entries_need_no_gpu():
    lib = _abi.load_library()
    err = lambda: lib.aadff_last_error()                                          # noqa: E731

    def fwd(u=P8, c=P16, g=P24, uo=P32, co=P40, N=2, Cn=3, H=37, W=70, r=4, ks=0.125, kr=16.0):
        return lib.aadff_depth_refine_fwd(u, c, g, uo, co, N, Cn, H, W, r, ks, kr, None)

    def bwd(u=P8, c=P16, g=P24, gu=P32, gc=P40, du=P8, dc_=P8, ws=P8, nbytes=1 << 20, N=2, Cn=3, H=37, W=70, r=4, ks=0.125, kr=16.0):
        return lib.aadff_depth_refine_bwd(u, c, g, gu, gc, du, dc_, ws, nbytes, N, Cn, H, W, r, ks, kr, None)

    for call, names in ((fwd, ("u", "c", "g", "uo", "co")), (bwd, ("u", "c", "g", "gu", "gc"))):
        for name in names:
            assert call(**{name: None}) == -1 and b"is NULL" in err(), name
        for bad in (0, 5, -1):
            assert call(Cn=bad) == -1 and b"C = %d" % bad in err()
        for bad in (0, 9, -3):
            assert call(r=bad) == -1 and b"radius = %d" % bad in err()
        for bad in (0.0, -1.0, float("nan"), float("inf")):
            assert call(ks=bad) == -1 and b"ks =" in err()
            assert call(kr=bad) == -1 and b"kr =" in err()
        assert call(N=0) == -1 and b"N = 0" in err()
        assert call(H=0) == -1 and b"H = 0" in err()
        assert call(W=-2) == -1 and b"W = -2" in err()
        assert call(H=70000, W=70000) == -1 and b"too large" in err()
    assert fwd(uo=P8) == -1 and b"aliases" in err()                               # u_out may not be u: every pixel reads its neighbours
    assert fwd(co=P16) == -1 and b"aliases" in err() and fwd(uo=P40) == -1 and b"aliases" in err()
    assert bwd(du=None, dc_=None) == -1 and b"no gradient" in err()
    assert bwd(ws=None) == -1 and b"workspace" in err()
    need = ops.depth_refine_bwd_workspace_bytes(2, 37, 70)
    assert need == 16 * 2 * 37 * 70
    assert bwd(nbytes=need - 1) == -1 and b"workspace" in err() and b"%d are needed" % need in err()


def test_constants_are_float32_roundings_of_float64():
    for Cn, ss, sr in ((3, 2.0, 0.1), (1, 0.7, 0.033), (4, 3.0, 1.7)):
        ks, kr = ops.depth_refine_constants(Cn, ss, sr)
        assert (ks, kr) == rc.constants(Cn, ss, sr)
        assert ks == float(np.float32(ks)) and kr == float(np.float32(1.0 / (2.0 * sr * sr * Cn)))


def test_ops_and_fake_shapes():
    from torch._subclasses.fake_tensor import FakeTensorMode
    for name in ("depth_refine", "depth_refine_bwd"):
        assert hasattr(torch.ops.aadff, name)
    with FakeTensorMode():
        new = lambda *s: torch.empty(*s, device="cuda")                            # noqa: E731
        u, c, g = new(2, 1, 37, 70), new(2, 1, 37, 70), new(2, 3, 37, 70)
        uo, co = torch.ops.aadff.depth_refine(u, c, g, 4, 2.0, 0.1)
        assert uo.shape == co.shape == (2, 1, 37, 70) and uo.dtype == co.dtype == torch.float32
        d_u, d_c = torch.ops.aadff.depth_refine_bwd(u, c, g, uo, co, 4, 2.0, 0.1, True, True)
        assert d_u.shape == d_c.shape == (2, 1, 37, 70)
        d_u, d_c = torch.ops.aadff.depth_refine_bwd(u, c, g, uo, co, 4, 2.0, 0.1, True, False)
        assert d_u.shape == (2, 1, 37, 70) and d_c.shape == (0,)


def test_public_value_errors_need_no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    d, c, g = torch.ones(2, 1, 8, 9), torch.ones(2, 1, 8, 9), torch.zeros(2, 3, 8, 9)
    neg = c.clone()
    neg[0, 0, 1, 1] = -0.1
    nanc = c.clone()
    nanc[1, 0, 2, 2] = float("nan")
    zero = d.clone()
    zero[0, 0, 3, 3] = 0.0
    for bad in (dict(depth=d[0]), dict(depth=[[1.0]]), dict(depth=d.long()), dict(confidence=c[:, :, :7]), dict(depth=d.expand(2, 2, 8, 9)),
                dict(guide=g[:, :0]), dict(guide=torch.zeros(2, 5, 8, 9)), dict(guide=g[:1]), dict(guide=g[0]),
                dict(radius=0), dict(radius=9), dict(radius=2.0), dict(radius=True), dict(iterations=-1), dict(iterations=1.5),
                dict(sigma_space=0.0), dict(sigma_space=-1.0), dict(sigma_space=float("nan")), dict(sigma_space="a"),
                dict(sigma_range=0.0), dict(sigma_range=float("inf")), dict(sigma_range=None), dict(space="log"),
                dict(confidence=neg), dict(confidence=nanc), dict(depth=zero)):
        with pytest.raises(ValueError, match="refine_depth"):
            refine.refine_depth(**{**dict(depth=d, confidence=c, guide=g), **bad})
    with pytest.raises(RuntimeError, match="no HIP device"):                       # valid arguments: only now is the GPU asked for
        refine.refine_depth(zero, c, g, space="linear")                            # (a zero depth is fine in linear space)
    with pytest.raises(ValueError, match="DepthRefiner"):
        refine.DepthRefiner(radius=12)
    m = refine.DepthRefiner(radius=3, sigma_range=0.2, iterations=1, space="linear")
    assert "radius=3" in repr(m) and "sigma_range=0.2" in repr(m) and "space='linear'" in repr(m)


def test_confidence_maps():
    gen = torch.Generator().manual_seed(1)
    peak = torch.rand(2, 1, 5, 7, generator=gen)
    peak[1] *= 10
    med = peak.flatten(1).median(1).values.reshape(2, 1, 1, 1)
    assert torch.equal(refine.confidence_from_peak(peak), peak / (peak + med))
    assert torch.equal(refine.confidence_from_peak(peak, 0.25), peak / (peak + 0.25))
    assert torch.equal(refine.confidence_from_peak(peak, torch.tensor([0.5, 2.0])), peak / (peak + torch.tensor([0.5, 2.0]).reshape(2, 1, 1, 1)))
    sparse = peak * (peak > med * 3)                                               # more than half zero: the median, and so tau, is 0
    assert float(sparse.flatten(1).median(1).values.max()) == 0
    assert torch.equal(refine.confidence_from_peak(sparse), (sparse > 0).float())
    assert torch.equal(refine.confidence_from_peak(peak, 0.0), torch.ones_like(peak))
    std = peak + 0.1
    smed = std.flatten(1).median(1).values.reshape(2, 1, 1, 1)
    assert torch.equal(refine.confidence_from_std(std), 1.0 / (1.0 + (std / smed) ** 2))
    assert torch.equal(refine.confidence_from_std(std, 2.0), 1.0 / (1.0 + (std / 2.0) ** 2))
    assert float(refine.confidence_from_std(torch.zeros(1, 1, 2, 2), 1.0).min()) == 1.0
    p = peak.clone().requires_grad_(True)                                          # differentiable; the median is a constant
    refine.confidence_from_peak(p).sum().backward()
    assert torch.allclose(p.grad, med / (peak + med) ** 2)
    for fn, kw in ((refine.confidence_from_peak, "tau"), (refine.confidence_from_std, "scale")):
        for bad in (dict(x=peak[0]), dict(x=-peak), dict(x=peak.long()), dict(k=-1.0), dict(k=float("nan")), dict(k=torch.ones(3)),
                    dict(k=torch.ones(2, 1))):
            with pytest.raises(ValueError, match=fn.__name__):
                fn(bad.get("x", peak), **({kw: bad["k"]} if "k" in bad else {}))
    with pytest.raises(ValueError, match="confidence_from_std"):
        refine.confidence_from_std(std, 0.0)
    with pytest.raises(ValueError, match="confidence_from_std"):
        refine.confidence_from_std(sparse)                                         # a median of 0 is no scale
    assert refine.confidence_from_peak(torch.zeros(0, 1, 4, 4)).shape == (0, 1, 4, 4)
    assert refine.confidence_from_std(torch.zeros(2, 1, 0, 4)).shape == (2, 1, 0, 4)


def test_empty_shapes_need_no_gpu(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    for N, H, W in ((0, 8, 8), (2, 0, 8), (2, 8, 0), (0, 0, 0)):
        d, c = torch.ones(N, 1, H, W, requires_grad=True), torch.ones(N, 1, H, W, requires_grad=True)
        for space in refine.SPACES:
            out = refine.refine_depth(d, c, torch.zeros(N, 3, H, W), space=space)
            assert isinstance(out, refine.RefinedDepth) and out.depth.shape == out.confidence.shape == (N, 1, H, W)
            assert out.depth.dtype == out.confidence.dtype == torch.float32 and out.depth.requires_grad
        (out.depth.sum() + out.confidence.sum()).backward()
        assert d.grad.shape == d.shape and c.grad.shape == c.shape
    assert refine.DepthRefiner()(torch.ones(0, 1, 4, 4), torch.ones(0, 1, 4, 4), torch.ones(0, 1, 4, 4)).depth.shape == (0, 1, 4, 4)
