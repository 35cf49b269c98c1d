"""GPU: the chief-centre fit of the PSF-grid launch (aadff_chief_fit_weights, aadff_psf_points_fit,
aadff_psf_points_staged_fit) against the full chief pass of the same launch (AADFF_PSF_CHIEF=full), numpy float64 and the float64
oracle on the same draws."""
import contextlib
import ctypes as C
import json
import os
import sys

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aadff import _abi                                    # noqa: E402
from aadff.focal_stack import GEO_SPP, StackPlan          # noqa: E402
from deeplens.optics import Lensgroup                     # noqa: E402
from oracle.lens import OracleLens, Rays                  # noqa: E402

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
import gen_chief_fit_tables as gen                        # noqa: E402

DEV = "cuda:0"
RES = (256, 256)
KS, SPP, FOCUS, PLANE, L = 11, 256, [-1000.0, -3000.0], -1500.0, 3
K = _abi.CHIEF_NODES
CENTRE_TOL, PSF_TOL = 2e-5, 2e-3                          # the project's bounds on a chief centre [mm] and on a PSF (rel-L2)
# The weights kernel against numpy float64 on the same uniforms.  The kernel maps a draw to the unit disc as the trace does: float32
# square root, and the hardware sine / cosine of an angle in revolutions, whose absolute error is about 2^-20 = 1e-6 for arguments in
# [0, 1).  A monomial of degree <= 10 of one draw moves by at most 10 x that, 1e-5; the errors of the 2048 draws are independent,
# so their mean moves by 1e-5 / 2048^0.5 = 2.2e-7, and a weight by at most the row sum of |pinv(V)^T| (4.0) times that: 9e-7,
# rounded up.  (A weight is O(0.05) and multiplies a hit offset of a spot size, 0.05 mm: an error of 1e-6 in every one of the 85
# weights moves a centre by 4e-6 mm at most, a fifth of CENTRE_TOL.)  Observed: 1.4e-7.
WEIGHT_TOL = 1e-6


@contextlib.contextmanager
def env(name, value):
    old = os.environ.pop(name, None)
    if value is not None:
        os.environ[name] = value
    try:
        yield
    finally:
        os.environ.pop(name, None)
        if old is not None:
            os.environ[name] = old


def lens_file(repo_root, tmp_path, name):
    """Shipped lenses by name; 'rf50mm_narrow': rf50mm with the element behind the stop stopped down to 0.45 x the stop radius, which
    vignettes the guard ring of every field point, the axial one included (the pupil follows the stop itself: narrowing that would
    shrink the node set with it).  In the float64 oracle 67-100 % of the chief rays of the points within 0.3 of the field survive."""
    path = os.path.join(repo_root, "lenses", "rf50mm" if name == "rf50mm_narrow" else name, "lens.json")
    if name != "rf50mm_narrow":
        return path
    d = json.load(open(path))
    d["surfaces"][6]["r"] = 0.45 * d["surfaces"][5]["r"]
    path = str(tmp_path / "rf50mm_narrow.json")
    json.dump(d, open(path, "w"))
    return path


class Case:
    """One draw and one refocus of both focus states; `launch` runs the fit entry on them."""

    def __init__(self, path, grid, spp_chief=GEO_SPP, field=1.0):
        self.path, self.grid, self.N, self.S, self.spp_chief = path, grid, grid * grid, len(FOCUS), spp_chief
        self.lens = Lensgroup(path, sensor_res=RES, device=DEV)
        self.plan = plan = StackPlan(self.lens, self.S, RES[0], RES[1], grid=grid, ks=KS, spp=SPP)
        torch.manual_seed(11)
        self.u = plan.uniforms(self.lens.sampler)
        self.ub = self.u.data_ptr()
        self.dep, self.pts = plan.geometry(FOCUS, PLANE)
        self.pts = self.pts.clone()
        self.pts[..., :2] *= field                                   # the field points, pulled towards the axis
        self.st = _abi.stream_ptr(torch.device(DEV))
        _abi.call("aadff_refocus", _abi.ptr(self.dep), self.S, C.c_void_p(self.ub), GEO_SPP, plan.per, _abi.ptr(plan.tab_green), plan.lc,
                  _abi.ptr(plan.states), self.st)
        self.w = torch.full((self.S, L, 2, K), float("nan"), device=DEV)
        self.fitc = torch.full((self.S * L * self.N * 4,), float("nan"), device=DEV)
        _abi.call("aadff_chief_fit_weights", C.c_void_p(self.ub + 4 * plan.o_chief), self.S, L, spp_chief, plan.per, plan.per_l, None,
                  _abi.ptr(self.w), self.st)

    def launch(self, weights, trace="seq", chief=None, stage=None, ub=None):
        plan, S, N = self.plan, self.S, self.N
        ub = self.ub if ub is None else ub
        psf = torch.full((S, N, L, KS, KS), float("nan"), device=DEV)
        cen = torch.full((S, L, N, 2), float("nan"), device=DEV)
        args = [_abi.ptr(self.pts), S, N, L, _abi.ptr(plan.tab_rgb), _abi.ptr(plan.tab_green), plan.lc, _abi.ptr(plan.states),
                C.c_void_p(ub + 4 * plan.o_main), SPP, plan.per, plan.per_l, C.c_void_p(ub + 4 * plan.o_chief), self.spp_chief, plan.per, plan.per_l,
                KS, 1, 0, _abi.ptr(psf), _abi.ptr(cen), _abi.ptr(plan.flags)]
        tail = [None if weights is None else _abi.ptr(weights), _abi.ptr(self.fitc), self.st]
        with env("AADFF_PSF_TRACE", "loop" if trace == "loop" else None), env("AADFF_PSF_CHIEF", chief):
            if stage is None:
                _abi.call("aadff_psf_points_fit", *args, *tail)
            else:
                _abi.call("aadff_psf_points_staged_fit", *args, C.byref(stage), *tail)
        plan.check_flags()
        return psf.cpu().numpy(), cen.cpu().numpy()

    def ok(self):
        """[S,L,N] bool: the flag the node-ray kernel of the last fit launch left - the guards passed, the fitted centre stands"""
        return self.fitc.view(self.S, L, self.N, 4)[..., 2].cpu().numpy() != 0

    def oracle_centres(self):
        """[S,L,N,2] float64: -(mean sensor hit) of the spp_chief chief rays of the same uniforms, through the float64 oracle lens
        focused where the GPU's states are, from the object points and to the pupil the kernel uses."""
        plan, lc = self.plan, self.plan.lc
        states = (_abi.LensState * self.S).from_buffer_copy(bytes(plan.states.cpu().numpy()))
        uh = self.u.cpu().numpy().astype(np.float64).reshape(self.S, plan.per)
        pts = self.pts.cpu().numpy().astype(np.float64)
        out = np.empty((self.S, L, self.N, 2))
        self.vignetted = np.zeros((self.S, L, self.N), bool)          # a chief ray of the point is invalid in the oracle
        old = torch.get_default_dtype()
        torch.set_default_dtype(torch.float64)
        try:
            ol = OracleLens(self.path, sensor_res=RES)
            for s in range(self.S):
                ol.d_sensor = float(states[s].d_sensor)
                scale = -pts[s, :, 2] * float(states[s].tan_hfov) / lc.r_last
                pobj = torch.from_numpy(np.stack([pts[s, :, 0] * scale * lc.sensor_w / 2, pts[s, :, 1] * scale * lc.sensor_h / 2, pts[s, :, 2]], 1))
                for l in range(L):
                    o0 = plan.o_chief + l * plan.per_l
                    ut, ur = uh[s, o0:o0 + self.spp_chief], uh[s, o0 + self.spp_chief:o0 + 2 * self.spp_chief]
                    rr = np.sqrt(ur * lc.enp_r2_shrunk)
                    o2 = torch.from_numpy(np.stack([rr * np.cos(2 * np.pi * ut), rr * np.sin(2 * np.pi * ut), np.full_like(ut, lc.enp_z)], 1))
                    o = pobj.unsqueeze(0).repeat(len(ut), 1, 1)
                    ray = ol.trace2sensor(Rays(o, o2.unsqueeze(1) - o))
                    ra = ray.ra.unsqueeze(-1)
                    out[s, l] = -((ray.o * ra).sum(0) / ra.sum(0))[:, :2].numpy()
                    self.vignetted[s, l] = (ray.ra == 0).any(0).numpy()
        finally:
            torch.set_default_dtype(old)
        return out


_CASES = {}


def case(repo_root, tmp_path, name, grid):
    key = (name, grid)
    if key not in _CASES:
        c = Case(lens_file(repo_root, tmp_path, name), grid, field=0.3 if name == "rf50mm_narrow" else 1.0)
        c.full = {t: c.launch(c.w, t, chief="full") for t in ("seq", "loop")}
        c.fit, c.ok_flag = {}, {}
        for t in ("seq", "loop"):
            c.fitc.fill_(float("nan"))
            c.fit[t] = c.launch(c.w, t)
            c.ok_flag[t] = c.ok()
        _CASES[key] = c
    return _CASES[key]


@pytest.mark.parametrize("name", ["rf50mm", "50mm_f2.8"])
def test_weights_kernel_against_numpy(repo_root, tmp_path, name):
    c = case(repo_root, tmp_path, name, 3)
    wh = c.w.cpu().numpy().astype(np.float64)
    uh = c.u.cpu().numpy().astype(np.float64).reshape(c.S, c.plan.per)
    _, fd, fd2 = gen.tables()
    worst = 0.0
    for s in range(c.S):
        for l in range(L):
            o = c.plan.o_chief + l * c.plan.per_l
            ut, ur = uh[s, o:o + GEO_SPP], uh[s, o + GEO_SPP:o + 2 * GEO_SPP]
            unit = np.stack([np.sqrt(ur) * np.cos(2 * np.pi * ut), np.sqrt(ur) * np.sin(2 * np.pi * ut)], 1)
            m = gen.vandermonde(unit, gen.DEGREE).mean(0)
            worst = max(worst, np.abs(fd @ m - wh[s, l, 0]).max(), np.abs(fd2 @ m[:fd2.shape[1]] - wh[s, l, 1]).max())
    print(f"{name}: weights kernel vs numpy float64, max |d| {worst:.3e}")
    assert np.isfinite(wh).all() and worst <= WEIGHT_TOL
    assert np.abs(wh.sum(-1) - 1.0).max() <= 1e-6                    # the constant is in both bases: the weights sum to one


@pytest.mark.parametrize("trace", ["seq", "loop"])
@pytest.mark.parametrize("grid", [3, 5])
@pytest.mark.parametrize("name", ["rf50mm", "50mm_f2.8"])
def test_fit_against_full_pass_and_oracle(repo_root, tmp_path, margin, name, grid, trace):
    c = case(repo_root, tmp_path, name, grid)
    (psf_f, cen_f), (psf, cen) = c.full[trace], c.fit[trace]
    assert np.isfinite(psf).all() and np.isfinite(cen).all()
    fell_back = ~c.ok_flag[trace]                                    # [S,L,N], from the node-ray kernel's own flag
    assert np.array_equal(cen[fell_back], cen_f[fell_back])          # a workgroup that fell back traced every draw: the full pass's bits
    if not hasattr(c, "want"):
        c.want = c.oracle_centres()
    centre, corner = (c.N - 1) // 2, 0
    assert not fell_back[:, :, centre].any(), "the axial point must take the fitted centre"
    # Neither "always falls back" nor "never falls back" may pass.  A point must fall back wherever one of its 2048 chief rays is
    # invalid (the hit is no polynomial of the pupil position there); rf50mm vignettes its corners inside the shrunk pupil, so there a
    # corner must fall back.  50mm_f2.8 at this plane does not (every chief ray of every point is valid in the float64 oracle, and
    # the fitted corners are as close to the oracle as the full pass), so for it the condition is the general one alone.
    assert not (c.vignetted & ~fell_back).any(), "a point with an invalid chief ray took the fitted centre"
    if name == "rf50mm":
        assert c.vignetted[:, :, corner].any()
    if c.vignetted[:, :, corner].any():
        assert fell_back[:, :, corner].any(), "a corner point is vignetted: it must fall back"
    d_fit = np.abs(cen - c.want).max(-1)
    d_full = np.abs(cen_f - c.want).max(-1)
    print(f"{name} grid {grid} {trace}: fitted {(~fell_back).sum()} of {fell_back.size}; vs float64 oracle: fitted {d_fit[~fell_back].max():.3e} mm, "
          f"the same workgroups' full pass {d_full[~fell_back].max():.3e} mm, all workgroups' full pass {d_full.max():.3e} mm")
    # every workgroup that took the fitted centre, none excluded; beside it what the full pass gives for the same workgroups (a
    # workgroup that fell back has the full pass's bits, and a vignetted point's centre moves by spot size / 2048 = 2e-5 mm with
    # every ray whose validity float32 and float64 decide differently: that is the full pass's matter, printed above)
    margin(f"chief fit {name} g{grid} {trace}: full-pass centres vs f64 oracle [mm]", d_full[~fell_back].max(), CENTRE_TOL)
    margin(f"chief fit {name} g{grid} {trace}: fitted centres vs f64 oracle [mm]", d_fit[~fell_back].max(), CENTRE_TOL)
    rel = float(np.linalg.norm(psf.astype(np.float64) - psf_f) / np.linalg.norm(psf_f.astype(np.float64)))
    margin(f"chief fit {name} g{grid} {trace}: PSFs vs full pass, rel-L2", rel, PSF_TOL)


def test_every_point_falls_back_gives_the_full_pass_bits(repo_root, tmp_path):
    c = case(repo_root, tmp_path, "rf50mm_narrow", 3)
    for t in ("seq", "loop"):
        assert not c.ok_flag[t].any()
        assert np.array_equal(c.fit[t][1], c.full[t][1])
        assert np.array_equal(c.full[t][1], c.launch(None, t)[1])    # AADFF_PSF_CHIEF=full is the launch without weights
    # the histogram is summed with float atomics, so two launches of one kernel agree to their order only: 2048^0.5 x 2^-24 per bin
    # (tests/test_gpu_psf_sequence.py: ORDER_TOL); the centres above are what the chief pass decides
    d = np.abs(c.fit["seq"][0].astype(np.float64) - c.full["seq"][0]).max()
    assert d <= 2048 ** 0.5 * 2.0 ** -24


def test_below_the_switch_over_the_full_pass_is_taken(repo_root, tmp_path):
    c = Case(lens_file(repo_root, tmp_path, "rf50mm"), 3, spp_chief=256)
    got, want = c.launch(c.w), c.launch(None)
    assert np.array_equal(got[1], want[1]) and np.isnan(c.fitc.cpu().numpy()).all()      # no node ray was traced at all
    # the PSFs: the same kernel on the same centres; the histogram is summed with float atomics, so two launches agree to their
    # order only, 2048^0.5 x 2^-24 relative (tests/test_gpu_psf_sequence.py: ORDER_TOL, the bound of one trace launched twice there)
    assert np.isfinite(got[0]).all()
    assert np.linalg.norm(got[0].astype(np.float64) - want[0]) / np.linalg.norm(want[0].astype(np.float64)) <= 2048 ** 0.5 * 2.0 ** -24


def test_staged_entry_same_centres(repo_root, tmp_path):
    """States >= first_slice reach the weights kernel through pinned memory and the PSF kernel through the staged copy."""
    c = case(repo_root, tmp_path, "rf50mm", 3)
    plan, first = c.plan, 1
    assert plan.per % 4 == 0
    u_pin = torch.empty(c.S * plan.per, dtype=torch.float32).pin_memory()
    u_pin.copy_(c.u.cpu())
    u_dev = torch.full((c.S * plan.per,), float("nan"), device=DEV)
    u_dev[:first * plan.per] = c.u[:first * plan.per]
    counters = torch.zeros(c.S, dtype=torch.int32, device=DEV)
    stage = _abi.Stage(u_pin.data_ptr(), u_dev.data_ptr(), plan.per, first, 1, counters.data_ptr())
    w = torch.full_like(c.w, float("nan"))
    _abi.call("aadff_chief_fit_weights", C.c_void_p(u_dev.data_ptr() + 4 * plan.o_chief), c.S, L, GEO_SPP, plan.per, plan.per_l, C.byref(stage),
              _abi.ptr(w), c.st)
    assert torch.equal(w, c.w)
    _, cen = c.launch(w, stage=stage, ub=u_dev.data_ptr())
    assert np.array_equal(cen, c.fit["seq"][1])
    assert torch.equal(u_dev, c.u)                                   # and the staged copy delivered the late state's draws
