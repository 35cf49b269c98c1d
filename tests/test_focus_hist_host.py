"""CPU: the inputs, references and bounds of tests/test_gpu_focus_stage.py and tests/test_gpu_histogram.py (tests/focus_hist_common.py)
hold what they promise without a GPU - the draws' conditions under the float64 oracle, the float32 oracle's distance from it (which
sets the GPU tolerances), and every mutated reference rejected by the checks the GPU tests apply."""
import numpy as np
import pytest
import torch

import focus_hist_common as fh
from raytrace_common import default_dtype

SETS = [pytest.param(name, entry, spp, id=f"{name}-{entry}-spp{spp}") for name in fh.LENSES
        for entry, spps in (("plain", fh.PLAIN_SPP), ("staged", fh.STAGED_SPP)) for spp in spps]


# ------------------------------------------------------------------------------------------------------------------ focus stage
def test_tail_positions_are_the_lanes_the_kernel_masks():
    """parts / last_second_ray against refocus_kernel's loop written out: for i = begin + tid; i < end; i += 2 NT, second ray i + NT"""
    for entry, spps in (("plain", fh.PLAIN_SPP), ("staged", fh.STAGED_SPP)):
        nt = fh.NT[entry]
        for spp in spps:
            seen = []
            for begin, end in fh.parts(spp, entry):
                second = [i + nt for tid in range(nt) for i in range(begin + tid, end, 2 * nt) if i + nt < end]
                first = [i for tid in range(nt) for i in range(begin + tid, end, 2 * nt)]
                seen += first + second
                assert fh.last_second_ray(begin, end, nt) == (max(second) if second else None)
            assert sorted(seen) == list(range(spp)), "every ray in exactly one lane"
            pos = fh.tail_positions(spp, entry)
            assert pos[0] == spp - 1 and all(e - 1 in pos for b, e in fh.parts(spp, entry) if b < e)
    assert [b >= e for b, e in fh.parts(1, "staged")] == [False, True, True, True]           # empty quarters
    assert fh.parts(5, "staged") == [(0, 2), (2, 4), (4, 5), (6, 5)]                         # ragged chunk, one empty
    assert fh.last_second_ray(0, 3000, 1024) == 2047 and fh.last_second_ray(0, 1025, 1024) == 1024


@pytest.mark.parametrize("name,entry,spp", SETS)
def test_draws_make_the_count_decidable(name, entry, spp):
    d = fh.draw_sets(name)[(entry, spp)]
    with default_dtype(torch.float64):
        lens = fh.oracle_lens(name, torch.float64)
        for s, dep in enumerate(fh.DEPTHS):
            # the walk that measures the clearances is the oracle's trace: same rays, bit for bit, alone as in the batch
            fd, ok, clear = fh.trace_focus(lens, dep, d.ut[s], d.ur[s], clear=True)
            fd0, ok0 = fh.trace_focus(lens, dep, d.ut[s], d.ur[s])
            assert np.array_equal(ok, ok0) and np.array_equal(fd[ok], fd0[ok])
            assert clear.all(), "a draw within the margin of a validity decision"
            assert np.array_equal(ok, d.ok[s]) and d.count[s] == ok.sum() >= 1
            assert np.allclose(fd[ok], d.fd[s][ok], rtol=1e-12, atol=0)
    assert d.clear.all()
    assert np.array_equal(d.ok32, d.ok), "the float32 oracle decides a ray differently"
    share = float((~d.ok).mean())
    print(f"{name} {entry} spp {spp}: invalid {100 * share:.1f} %, counts {d.count.tolist()}, float32 oracle vs float64: d_sensor "
          f"{d.floor_d.max():.2e}, " + ", ".join(f"{f} {d.floor[f].max():.2e}" for f in fh.FIELDS))
    if spp > 1:                                                      # one ray per state: it has to be valid (flags == 0)
        assert fh.INVALID_MIN <= share <= fh.INVALID_MAX
    # the outliers sit at the tail: the last ray is valid and the furthest from the mean of all valid rays but those placed with it
    for s in range(len(fh.DEPTHS)):
        pos = fh.tail_positions(spp, entry)[:int(d.count[s])]
        assert d.ok[s][pos].all()
        dist = np.abs(d.fd[s] - d.fd[s][d.ok[s]].mean())
        others = np.setdiff1d(np.flatnonzero(d.ok[s]), pos)
        assert len(others) == 0 or dist[pos].min() >= dist[others].max()
    u = d.block()
    assert u.dtype == np.float32 and len(u) == 3 * d.stride and np.isfinite(u).all() and 0 <= u.min() and u.max() < 1
    assert np.array_equal(u[d.stride + spp:d.stride + 2 * spp], d.ur[1]) and set(u[2 * spp:d.stride].tolist()) == {np.float32(0.25), np.float32(0.04)}


def test_tolerances_come_from_the_float32_oracle():
    tol = fh.tolerances()
    floors = {k: max(float((d.floor_d if k == "d_sensor" else d.floor[k]).max()) for n in fh.LENSES for d in fh.draw_sets(n).values()) for k in tol}
    for k, v in tol.items():
        print(f"{k}: float32 oracle vs float64, largest over every state of every draw set {floors[k]:.3e}; GPU tolerance {v:.3e}")
        assert v == min(fh.PROJECT_TOL, 4 * floors[k]) and 0 < v <= fh.PROJECT_TOL
        assert floors[k] < 2e-6, "the floor measured when the tests were written: d_sensor per ray <= 1.3e-6"


@pytest.mark.parametrize("name,entry,spp", SETS)
def test_focus_check_rejects_every_tail_bug(name, entry, spp):
    d = fh.draw_sets(name)[(entry, spp)]
    tol = fh.tolerances()["d_sensor"]
    lens = fh.oracle_lens(name, torch.float64)
    for s in range(len(fh.DEPTHS)):
        assert fh.focus_check(d.count[s], d.d_sensor[s], d.count[s], d.d_sensor[s], tol)
        assert fh.focus_check(d.count[s], d.d_sensor[s] * (1 + 0.9 * tol), d.count[s], d.d_sensor[s], tol)
        for what in fh.MUTATIONS:
            m = fh.mutated_reference(d, s, what, lens)
            if m is None:
                assert what == "drop_second_of_last_pair" and all(e - b <= fh.NT[entry] for b, e in fh.parts(spp, entry))
                continue
            moved = abs(m[1] - d.d_sensor[s]) / d.d_sensor[s] if m[0] else float("inf")
            assert not fh.focus_check(d.count[s], d.d_sensor[s], m[0], m[1], tol), f"state {s}: {what} passes (count {m[0]} vs {d.count[s]}, value moved {moved:.2e})"
            if what != "u_r_at_2048" and d.count[s] > 1:
                assert m[0] != d.count[s] and moved > 0, "the tail ray is valid and off the mean: count and value both move"


# ------------------------------------------------------------------------------------------------------------------ histogram
SPLATS = [pytest.param(name, ks, spp, N, id=f"{name}-ks{ks}-spp{spp}-N{N}") for name in fh.LENSES for ks in fh.SPLAT_KS for spp in fh.SPLAT_SPP
          for N in fh.SPLAT_N]


@pytest.mark.parametrize("name,ks,spp,N", SPLATS)
def test_synthetic_hits_and_mutations(name, ks, spp, N):
    o, ra, centre, ps, kind = fh.splat_case(name, ks, spp, N)
    assert o.dtype == ra.dtype == centre.dtype == np.float32 and o.shape == (spp, N, 3)
    assert fh.clear_hits(o[..., :2], ra, centre, ps, ks).all()
    assert len({tuple(c) for c in centre.tolist()}) == N and (centre != 0).all() and np.abs(centre).max() < 5
    rowf, colf, w, shift = fh.bin_coordinates(o[..., :2], ra, centre, ps, ks)
    lo, hi, lim = fh.window(ps, ks)
    ax, ay = np.abs(shift[..., 0]), np.abs(shift[..., 1])
    if spp >= 255:                                                    # every kind of hit is there
        ring = (ax > lim) & (ax < hi) & (ay < lim)
        one = ((ax > hi) ^ (ay > hi))
        dead = (ra == 0) & (ax < lim) & (ay < lim)
        assert ring.any() and one.any() and dead.any() and (w[ring] == 0).all() and (w > 0).any()
        if ks % 2:
            assert ((shift == 0).any(-1) & (w > 0)).any() and ((shift == 0).all(-1) & (w > 0)).any(), "hits exactly on the centre tap"
            on = (shift[..., 0] == 0) & (w > 0)
            assert (colf[on] == (ks - 1) / 2).all()
    assert ((ra != 0) & (ra != 1)).any() == ((ks, spp, N) == fh.FRACTIONAL_CASE)
    raw, A, cnt = fh.splat_reference(o[..., :2], ra, centre, ps, ks)
    assert np.isclose(raw.sum(), w.sum(), rtol=1e-12) and (raw >= 0).all()
    if N == 3:
        assert (raw[fh.EMPTY_POINT] == 0).all() and (raw[0] > 0).any() and (raw[2] > 0).any()
    ref = (raw, A, cnt, ks)
    with np.errstate(invalid="ignore", divide="ignore"):
        psf = raw / raw.sum((1, 2), keepdims=True)
    r_raw, r_psf, nan_ok = fh.splat_check(raw, psf, ref)
    assert r_raw == 0 and r_psf == 0 and nan_ok
    # a float32 evaluation of the same formula is inside the bound (what the bound is for) ...
    r32 = splat_float32(o, ra, centre, ps, ks)
    with np.errstate(invalid="ignore"):
        ratio = fh.splat_check(r32, r32 / r32.sum((1, 2), keepdims=True), ref)
    print(f"{name} ks {ks} spp {spp} N {N}: float32 numpy evaluation / bound: raw {ratio[0]:.3f}, psf {ratio[1]:.3f}")
    assert ratio[0] <= 1 and ratio[1] <= 1 and ratio[2]
    # ... and every mutated reference is outside it
    for what in fh.SPLAT_MUTATIONS:
        applies = {"window_at_hi": spp >= 255, "ra0_counted": spp >= 255, "previous_centre": N > 1}.get(what, True)
        if not applies:
            continue
        m = fh.splat_reference(o[..., :2], ra, centre, ps, ks, mutate=what)[0]
        with np.errstate(invalid="ignore", divide="ignore"):
            mr = fh.splat_check(m, m / m.sum((1, 2), keepdims=True), ref)
        assert mr[0] > 1, f"{what}: raw passes ({mr[0]:.3f} of the bound)"
        assert mr[1] > 1 or not mr[2], f"{what}: the normalised PSF passes ({mr[1]:.3f} of the bound)"


def splat_float32(o, ra, centre, ps, ks):
    """splat_hit's steps in numpy float32 (division in place of the reciprocal, serial accumulation)"""
    f = np.float32
    lo, hi, lim = (f(v) for v in fh.window(ps, ks))
    N = ra.shape[1]
    X, Y = -o[..., 0] - centre[None, :, 0], -o[..., 1] - centre[None, :, 1]
    keep = (np.abs(X) < lim) & (np.abs(Y) < lim) & (ra > 0)
    X, Y = X * ra, Y * ra
    den = f(np.float64(hi) - np.float64(lo))
    rowf, colf = (Y - hi) / f(-den) * f(ks - 1), (X - lo) / den * f(ks - 1)
    fr, fc = np.floor(rowf), np.floor(colf)
    wb, wr = rowf - fr, colf - fc
    raw = np.zeros((N, ks, ks), f)
    for n in range(N):
        k = keep[:, n]
        for r, c, v in ((fr, fc, (1 - wb) * (1 - wr) * ra), (fr, np.floor(colf + f(1)), (1 - wb) * wr * ra), (np.floor(rowf + f(1)), fc, wb * (1 - wr) * ra),
                        (fr + 1, fc + 1, wb * wr * ra)):
            np.add.at(raw[n], (r[k, n].astype(np.int64), c[k, n].astype(np.int64)), v[k, n])
    return raw


def test_ks_1_has_no_reference():
    o, ra, centre, ps, _ = fh.splat_case("rf50mm", 3, 1, 1)
    with pytest.raises(ValueError, match="window is empty"):
        fh.bin_coordinates(o[..., :2], ra, centre, ps, 1)
    assert fh.window(ps, 1)[2] < 0


# ------------------------------------------------------------------------------------------------------------------ normalise
@pytest.mark.parametrize("N", fh.NORM_N)
@pytest.mark.parametrize("ks", fh.NORM_KS)
def test_normalise_reference_and_depth(N, ks):
    raw, zero = fh.normalise_case(N, ks)
    assert raw.dtype == np.float32 and (raw >= 0).all() and (raw[zero] == 0).all()
    sums = raw.astype(np.float64).sum(-1).reshape(-1)
    assert (np.diff(sums[sums > 0]) > 0.05 * sums[sums > 0][:-1]).all() and (sums > 0).sum() == len(sums) - 1, "every tile on a scale of its own"
    assert fh.normalise_depth(ks) == {3: 13, 12: 13, 51: 18}[ks]      # 1, 1 and 6 strided passes of 512 threads
    p0, p1 = fh.normalise_reference(raw, N, ks, 0), fh.normalise_reference(raw, N, ks, 1)
    g = int(round(N ** 0.5))
    assert p0.shape == (fh.NORM_S, N, fh.NORM_L, ks, ks) and p1.shape == (fh.NORM_S, fh.NORM_L, g * ks, g * ks)
    for s in range(fh.NORM_S):
        for l in range(fh.NORM_L):
            for n in range(N):
                gi, gj = divmod(n, g)
                tile = p1[s, l, gi * ks:(gi + 1) * ks, gj * ks:(gj + 1) * ks]
                assert np.array_equal(tile, p0[s, n, l], equal_nan=True)
                assert np.isnan(tile).all() == ((s * fh.NORM_L + l, n) == zero) == bool(np.isnan(tile).any())
                if not np.isnan(tile).any():
                    assert abs(tile.sum() - 1) < 1e-12
    # a mis-tiled element (the same bin of the neighbouring tile) is far outside the bound
    tol = (fh.normalise_depth(ks) + 2) * fh.EPS32
    if N > 1:
        a, b = p0[0, 0, 0], p0[0, 1, 0]
        assert (np.abs(raw[0, 0].reshape(ks, ks) / raw[0, 1].astype(np.float64).sum() - a) > tol * a).any() and not np.array_equal(a, b)
