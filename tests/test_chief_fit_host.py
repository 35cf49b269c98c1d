"""CPU: the chief-centre fit restated in float64 - the library's node and fit tables against a numpy recomputation,
and the method itself with the oracle lens: the weighted node hits against the mean over the very draws the weights were built
from, the vignetting guard, and the truncation guard."""
import ctypes as C
import os
import sys

import numpy as np
import pytest
import torch

from aadff import _abi
from oracle.lens import GEO_SPP, OracleLens, Rays

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_chief_fit_tables as gen                                   # noqa: E402

K, RAYS = _abi.CHIEF_NODES, _abi.CHIEF_RAYS
GRID = 5
# The fit against the sample mean of the same draws, where every node and ring ray is alive.  The float64 study this method rests on
# found a truncation of 1.6e-8 mm at worst over the 1210 (point, state) pairs of the bench configuration, with degree 8 at 3.2e-7 mm
# (a factor 20 per two degrees).  This reduced set (75 pairs of the same lens, plane and focus range) may not be worse than three times
# that figure: 5e-8 mm, 1/400 of the 2e-5 mm a chief centre is allowed and 1/50 of the float32 noise of the 2048-ray mean itself.
FIT_BOUND = 5e-8


def test_tables_equal_numpy_recomputation():
    lib = _abi.load_library()
    xy = np.empty((RAYS, 2), np.float64)
    fit = np.empty((66, K), np.float64)
    low = np.empty((45, K), np.float64)
    assert lib.aadff_chief_fit_tables(xy.ctypes.data_as(C.c_void_p), fit.ctypes.data_as(C.c_void_p), low.ctypes.data_as(C.c_void_p)) == 0
    want_xy, want_fit, want_low = gen.tables()
    assert (gen.N_NODES, gen.N_RAYS, gen.DEGREE) == (K, RAYS, _abi.CHIEF_DEGREE)
    assert np.abs(xy - want_xy).max() <= 1e-15
    # pinv through another LAPACK may differ by cond(V) x eps x |pinv| = 1.7e5 x 2.2e-16 x 4 = 1.5e-10
    assert np.abs(fit - want_fit.T).max() <= 1e-9 and np.abs(low - want_low.T).max() <= 1e-9
    # what the tables are for: they reproduce the mean of every monomial of the basis over an arbitrary point set
    rng = np.random.default_rng(3)
    r, a = np.sqrt(rng.random(300)), 2 * np.pi * rng.random(300)
    m = gen.vandermonde(np.stack([r * np.cos(a), r * np.sin(a)], 1), gen.DEGREE).mean(0)
    V = gen.vandermonde(xy[:K], gen.DEGREE)
    assert np.abs((fit.T @ m) @ V - m).max() <= 1e-11
    assert np.abs((low.T @ m[:45]) @ V[:, :45] - m[:45]).max() <= 1e-11


def test_binding_constants_are_the_headers(repo_root):
    """_abi.py restates AADFF_CHIEF_* by hand: they must be the header's."""
    import re
    text = open(os.path.join(repo_root, "include", "aadff.h")).read()
    got = {m.group(1): m.group(2) for m in re.finditer(r"#define\s+AADFF_CHIEF_(\w+)\s+([0-9.eE+-]+)f?", text)}
    assert (int(got["NODES"]), int(got["RAYS"]), int(got["DEGREE"])) == (_abi.CHIEF_NODES, _abi.CHIEF_RAYS, _abi.CHIEF_DEGREE)
    assert float(got["FIT_TOL"]) == _abi.CHIEF_FIT_TOL


@pytest.fixture(scope="module")
def experiment(repo_root):
    """rf50mm, 5 x 5 field points (corners included), three of the bench's ten focus distances, one draw per state, float64:
    per (state, point) the 2048 hits and the RAYS node / ring hits."""
    from aadff.synth import synth_depth_mm
    depth = synth_depth_mm(1024, 1024, seed=5678)
    dbar, fds = -float(depth.mean()), -np.linspace(depth.min(), depth.max(), 10)
    old = torch.get_default_dtype()
    torch.set_default_dtype(torch.float64)
    try:
        torch.manual_seed(0)
        lens = OracleLens(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(1024, 1024))
        nodes = torch.from_numpy(gen.nodes())
        out = []
        for f in (fds[0], fds[4], fds[9]):
            lens.refocus(float(f))
            pobj = lens.object_points(lens.point_source_grid(dbar, GRID).reshape(-1, 3))
            pz, pr = lens.entrance_pupil(shrink_pupil=True)
            ut, ur = torch.rand(GEO_SPP), torch.rand(GEO_SPP)
            unit = torch.stack((torch.sqrt(ur) * torch.cos(2 * np.pi * ut), torch.sqrt(ur) * torch.sin(2 * np.pi * ut)), 1)

            def hits(xy):
                o2 = torch.cat((xy * pr, torch.full((len(xy), 1), pz)), 1)
                o = pobj.unsqueeze(0).repeat(len(xy), 1, 1)
                ray = lens.trace2sensor(Rays(o, o2.unsqueeze(1) - o))
                return ray.o[..., :2].numpy(), ray.ra.numpy() > 0

            out.append((unit.numpy(), hits(unit), hits(nodes)))
        return out
    finally:
        torch.set_default_dtype(old)


def weights(unit, degree):
    m = gen.vandermonde(unit, degree).mean(0)
    return gen.fit_matrix(degree) @ m


def fitted(w, h):
    """h_0 + sum_k w_k (h_k - h_0) per point: h [RAYS, N, 2]"""
    return h[0] + np.einsum("k,knc->nc", w, h[:K] - h[0])


def test_fit_against_sample_mean_and_vignetting_guard(experiment):
    n_pass = n_refused = 0
    worst = 0.0
    for unit, (h, alive), (hn, alive_n) in experiment:
        w = weights(unit, gen.DEGREE)
        guard_a = alive_n.all(0)                                     # every node and ring ray of the point
        # guard (a) never passes a point one of whose 2048 chief rays is vignetted
        assert not (guard_a & ~alive.all(0)).any()
        n_pass += int(guard_a.sum())
        n_refused += int((~guard_a).sum())
        err = np.abs(fitted(w, hn) - h.mean(0))[guard_a]
        worst = max(worst, float(err.max()))
    print(f"fit vs sample mean where guard (a) passes ({n_pass} of {n_pass + n_refused} point-states): max {worst:.3e} mm")
    assert n_pass > 0 and n_refused > 0                              # the axis passes, the corners are vignetted
    assert worst <= FIT_BOUND


def test_truncation_guard_refuses_a_low_degree_fit(experiment):
    """Guard (b) compares two fits of different degree; with degree 4 in place of degree d - 2 the centres of an edge point whose node
    rays are all alive are further apart than the guard allows, so such a pair would be refused and the point traced in full."""
    unit, _, (hn, alive_n) = experiment[1]
    guard_a = alive_n.all(0)
    pts = OracleLens.point_source_grid(None, 0.0, GRID).reshape(-1, 3).numpy()
    edge = guard_a & (np.abs(pts[:, :2]).max(1) > 0.4)              # off-axis points that pass guard (a)
    assert edge.any()
    d = np.abs(fitted(weights(unit, gen.DEGREE), hn) - fitted(weights(unit, 4), hn))[edge].max()
    d_ok = np.abs(fitted(weights(unit, gen.DEGREE), hn) - fitted(weights(unit, gen.DEGREE - 2), hn))[guard_a].max()
    print(f"|c_10 - c_4| {d:.3e} mm, |c_10 - c_8| {d_ok:.3e} mm, tolerance {_abi.CHIEF_FIT_TOL:.1e} mm")
    assert d > _abi.CHIEF_FIT_TOL
    assert d_ok <= _abi.CHIEF_FIT_TOL                                # and in float64 the shipped pair is accepted
