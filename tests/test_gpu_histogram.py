"""GPU: the bilinear splat (`splat_hit` through aadff_psf_splat) and the normalisation (`normalise_and_write` through aadff_psf_normalise),
csrc/trace.hip, element by element against float64 (tests/focus_hist_common.py, parts B and C: the reference, the synthetic hits and the
bounds, derived there from the kernels' arithmetic; tests/test_focus_hist_host.py shows the inputs' conditions and that the bounds reject
seven mutated references)."""
import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import focus_hist_common as fh                            # noqa: E402
from aadff import _abi                                    # noqa: E402

DEV = "cuda:0"
SENTINEL = -7.0


def splat(o, ra, centre, ps, ks, with_raw):
    """aadff_psf_splat -> (raw or None, psf) as numpy; the outputs start as SENTINEL: every element has to be written"""
    spp, N = ra.shape
    o_, ra_, c_ = (torch.from_numpy(np.ascontiguousarray(a)).to(DEV) for a in (o, ra, centre))
    raw = torch.full((N, ks, ks), SENTINEL, device=DEV) if with_raw else None
    psf = torch.full((N, ks, ks), SENTINEL, device=DEV)
    _abi.call("aadff_psf_splat", _abi.ptr(o_), _abi.ptr(ra_), _abi.ptr(c_), spp, N, float(ps), ks, None if raw is None else _abi.ptr(raw), _abi.ptr(psf),
              _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return None if raw is None else raw.cpu().numpy(), psf.cpu().numpy()


@pytest.mark.parametrize("ks", fh.SPLAT_KS)
def test_splat_against_float64(margin, ks):
    """every bin of the raw histogram and of the normalised PSF within its bound, for both lenses' pixel sizes, spp in (1, 255, 257,
    1000) - below, beside and above the 256 lanes - and N in (1, 3), with and without psf_raw; a point without a ray inside is all 0 in
    raw and all NaN in the PSF"""
    worst_raw = worst_psf = 0.0
    for name in fh.LENSES:
        for spp in fh.SPLAT_SPP:
            for N in fh.SPLAT_N:
                o, ra, centre, ps, _ = fh.splat_case(name, ks, spp, N)
                raw, A, cnt = fh.splat_reference(o[..., :2], ra, centre, ps, ks)
                ref = (raw, A, cnt, ks)
                for with_raw in (True, False):
                    got_raw, got_psf = splat(o, ra, centre, ps, ks, with_raw)
                    assert not (got_psf == SENTINEL).any() and (got_raw is None or not (got_raw == SENTINEL).any())
                    r_raw, r_psf, nan_ok = fh.splat_check(got_raw, got_psf, ref)
                    print(f"splat {name} ks {ks} spp {spp} N {N} psf_raw {'yes' if with_raw else 'NULL'}: worst |d| / bound: raw {r_raw:.3f}, psf {r_psf:.3f}")
                    assert nan_ok, "NaN positions of the PSF differ from the reference's"
                    if N == 3:
                        assert np.isnan(got_psf[fh.EMPTY_POINT]).all() and (got_raw is None or (got_raw[fh.EMPTY_POINT] == 0).all())
                        assert np.isfinite(got_psf[0]).all() and np.isfinite(got_psf[2]).all()
                    assert r_raw <= 1 and r_psf <= 1, f"{name} ks {ks} spp {spp} N {N}: raw {r_raw:.3f}, psf {r_psf:.3f} of the bound"
                    worst_raw, worst_psf = max(worst_raw, r_raw), max(worst_psf, r_psf)
    margin(f"splat ks {ks}: raw histogram vs float64, worst |d| / bound over 32 launches", worst_raw, 1.0)
    margin(f"splat ks {ks}: normalised PSF vs float64, worst |d| / bound over 32 launches", worst_psf, 1.0)


def test_splat_ks_1_window_is_empty():
    """at ks = 1 the reference's window |x| < hi - 0.01 ps = -0.01 ps holds no ray: raw 0, PSF 0/0 (no oracle: its bin coordinate is 0/0)"""
    o, ra, centre, ps, _ = fh.splat_case("rf50mm", 3, 257, 3)
    raw, psf = splat(o, ra, centre, ps, 1, True)
    assert raw.shape == (3, 1, 1) and (raw == 0).all() and np.isnan(psf).all()


def normalise(raw, N, ks, layout, shape):
    S, L = fh.NORM_S, fh.NORM_L
    r = torch.from_numpy(raw).to(DEV)
    out = torch.full(shape, SENTINEL, device=DEV)
    rc = _abi.require_gpu().aadff_psf_normalise(_abi.ptr(r), S, N, L, fh.pixel_size("rf50mm"), ks, layout, _abi.ptr(out), _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    return rc, out.cpu().numpy()


@pytest.mark.parametrize("layout", [0, 1])
@pytest.mark.parametrize("ks", fh.NORM_KS)
@pytest.mark.parametrize("N", fh.NORM_N)
def test_normalise_against_float64(margin, N, ks, layout):
    """S = 2, L = 3, every tile on a scale of its own, in the point layout and in the psf_map tiling; ks = 51: six strided passes of the
    512 threads.  Relative (depth + 2) eps32 per element; the all-zero tile is NaN, and only it"""
    raw, zero = fh.normalise_case(N, ks)
    want = fh.normalise_reference(raw, N, ks, layout)
    rc, got = normalise(raw, N, ks, layout, want.shape)
    assert rc == 0 and not (got == SENTINEL).any()
    assert np.array_equal(np.isnan(got), np.isnan(want)) and np.isnan(want).sum() == ks * ks
    ok = ~np.isnan(want)
    rel = np.abs(got.astype(np.float64)[ok] - want[ok]) / want[ok]
    tol = (fh.normalise_depth(ks) + 2) * fh.EPS32
    print(f"normalise N {N} ks {ks} layout {layout}: worst relative error {rel.max():.3e}, bound {tol:.3e} (depth {fh.normalise_depth(ks)})")
    margin(f"normalise N {N} ks {ks} layout {layout}: worst relative error vs float64", rel.max(), tol)


def test_normalise_refuses_a_map_that_is_no_square():
    raw = np.ones((fh.NORM_S * fh.NORM_L, 5, 9), np.float32)
    rc, got = normalise(raw, 5, 3, 1, (fh.NORM_S, fh.NORM_L, 9, 9))
    assert rc != 0 and b"N = g*g" in _abi.require_gpu().aadff_last_error()
    assert (got == SENTINEL).all(), "a refused call wrote to its output"
    rc, got = normalise(raw, 5, 3, 0, (fh.NORM_S, 5, fh.NORM_L, 3, 3))            # the point layout takes any N
    assert rc == 0 and np.allclose(got, 1 / 9, rtol=1e-6)
