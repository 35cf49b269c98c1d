"""GPU: pupil points once per stack (aadff_chief_fit_prologue, aadff_psf_points_fit_pts, aadff_psf_points_staged_fit_pts)
and the node rays traced once per (point, state): the points against a float64 restatement of the mapping, the node-ray centres
against the kernel with a wave per wavelength, and the PSFs of a launch that loads points against the launch of the same build that
maps raw draws in every workgroup."""
import contextlib
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from aadff import _abi                                                        # noqa: E402
from aadff.focal_stack import GEO_SPP, STAGE_FIRST, StackPlan, pupil_xy_layout    # noqa: E402
from deeplens.optics import Lensgroup                                          # noqa: E402

DEV = "cuda:0"
RES = (256, 256)
GRID, KS, L, PLANE = 3, 11, 3, -1500.0
N, K = GRID * GRID, _abi.CHIEF_NODES
CENTRE, CORNER = (N - 1) // 2, 0
FOCUS = [-1000.0, -3000.0, -800.0, -2000.0, -6000.0]
CENTRE_TOL, PSF_TOL = 2e-5, 2e-3                  # the project's bounds on a chief centre [mm] and on PSFs (rel-L2): tests/test_gpu_chief_fit.py
# A point against float64, x = sqrt(u_r R^2) cos(2 pi u_theta) (y: sin), from the errors csrc/trace_core.h quotes for its primitives.
# With rr = sqrt(u_r R^2): the product u_r R^2 is rounded once (2^-24 relative, half of that behind the root), the hardware square
# root is good to 1 ulp (2^-23), the hardware sine and cosine of an angle in revolutions differ from those of the exact angle as by an
# angle error of 4e-7 rad (slope <= 1) and round their result (<= 1) once (2^-24), and the product rr x cos is rounded once (2^-24):
#   |dx| <= rr (2^-25 + 2^-23 + 4e-7 + 2^-24 + 2^-24) = 6.7e-7 rr       (8e-6 mm at the rim of rf50mm's pupil)
POINT_REL = 2.0 ** -25 + 2.0 ** -23 + 4e-7 + 2.0 ** -24 + 2.0 ** -24


@contextlib.contextmanager
def env(**kv):
    old = {k: os.environ.pop(k, None) for k in kv}
    os.environ.update({k: v for k, v in kv.items() if v is not None})
    try:
        yield
    finally:
        for k, v in old.items():
            os.environ.pop(k, None)
            if v is not None:
                os.environ[k] = v


class Case:
    """One draw and one refocus of S focus states; `run` is the prologue and the PSF launch of the plan path on them, unstaged or with
    the states >= STAGE_FIRST staged (their draws in the pinned block only when the launches start)."""

    def __init__(self, repo_root, spp, S, staged):
        self.spp, self.S, self.staged = spp, S, staged
        self.lens = Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=RES, device=DEV)
        self.plan = plan = StackPlan(self.lens, S, RES[0], RES[1], grid=GRID, ks=KS, spp=spp)
        torch.manual_seed(5)
        self.u = plan.uniforms(self.lens.sampler)
        self.dep, self.pts = plan.geometry(FOCUS[:S], PLANE)
        self.st = _abi.stream_ptr(torch.device(DEV))
        _abi.call("aadff_refocus", _abi.ptr(self.dep), S, _abi.ptr(self.u), GEO_SPP, plan.per, _abi.ptr(plan.tab_green), plan.lc,
                  _abi.ptr(plan.states), self.st)
        self.first = min(S, STAGE_FIRST)
        if staged:
            assert plan.per % 4 == 0 and self.first < S
            self.u_pin = torch.empty(S * plan.per, dtype=torch.float32).pin_memory()
            self.u_pin.copy_(self.u.cpu())
            self.u_dev = torch.full((S * plan.per,), float("nan"), device=DEV)
            self.u_dev[:self.first * plan.per] = self.u[:self.first * plan.per]       # what the refocus launch uploads
            self.counters = torch.zeros(S, dtype=torch.int32, device=DEV)
            self.generation = 0
        self.w_old = torch.full((S, L, 2, K), float("nan"), device=DEV)               # aadff_chief_fit_weights, every draw on the device
        ub = self.u.data_ptr()
        _abi.call("aadff_chief_fit_weights", C.c_void_p(ub + 4 * plan.o_chief), S, L, GEO_SPP, plan.per, plan.per_l, None, _abi.ptr(self.w_old), self.st)
        # points first: on the staged case they must leave the late states' draws uncopied, and the raw launch after them must find
        # the counters where its generation expects them
        self.pts_run = self.run()
        self.late_untouched = bool(torch.isnan(self.u_dev[self.first * plan.per:]).all()) if staged else None
        self.per_l_run = self.run(per_wavelength=True)
        self.raw_run = self.run(points=False)

    def run(self, points=True, per_wavelength=False):
        plan, S, spp = self.plan, self.S, self.spp
        nan = float("nan")
        out = {"w": torch.full((S, L, 2, K), nan, device=DEV), "xy": torch.full((S * pupil_xy_layout(spp, L)[0],), nan, device=DEV),
               "fitc": torch.full((S, L, N, 4), nan, device=DEV), "psf": torch.full((S, N, L, KS, KS), nan, device=DEV),
               "cen": torch.full((S, L, N, 2), nan, device=DEV)}
        stage = None
        ub = self.u.data_ptr()
        if self.staged:
            self.generation += 1
            stage = _abi.Stage(self.u_pin.data_ptr(), self.u_dev.data_ptr(), plan.per, self.first, self.generation, self.counters.data_ptr())
            ub = self.u_dev.data_ptr()
        um, uc = C.c_void_p(ub + 4 * plan.o_main), C.c_void_p(ub + 4 * plan.o_chief)
        with env(AADFF_PSF_POINTS=None if points else "raw", AADFF_CHIEF_CENTRES="per_wavelength" if per_wavelength else None, AADFF_PSF_LAUNCHES=None,
                 AADFF_PSF_CHIEF=None, AADFF_PSF_TRACE=None):
            _abi.call("aadff_chief_fit_prologue", um, spp, plan.per, plan.per_l, uc, S, L, GEO_SPP, plan.per, plan.per_l, plan.lc,
                      None if stage is None else C.byref(stage), _abi.ptr(out["w"]), _abi.ptr(out["xy"]), self.st)
            args = [_abi.ptr(self.pts), S, N, L, _abi.ptr(plan.tab_rgb), _abi.ptr(plan.tab_green), plan.lc, _abi.ptr(plan.states), um, spp, plan.per, plan.per_l,
                    uc, GEO_SPP, plan.per, plan.per_l, KS, 1, 0, _abi.ptr(out["psf"]), _abi.ptr(out["cen"]), _abi.ptr(plan.flags)]
            tail = [_abi.ptr(out["w"]), _abi.ptr(out["fitc"]), _abi.ptr(out["xy"]), self.st]
            if stage is None:
                _abi.call("aadff_psf_points_fit_pts", *args, *tail)
            else:
                _abi.call("aadff_psf_points_staged_fit_pts", *args, C.byref(stage), *tail)
        out = {k: v.cpu().numpy() for k, v in out.items()}
        out["flags"] = int(plan.flags.item())                                         # check (d): read, not raised, and left as found
        return out

    def points_float64(self):
        """[S,L,per_l] float64: sqrt(u_r R^2) cos / sin (2 pi u_theta) of every main (R^2 = enp_r2) and chief (enp_r2_shrunk) draw, and
        the rr of each element for the bound"""
        plan, spp = self.plan, self.spp
        rest = self.u.cpu().numpy().astype(np.float64).reshape(self.S, plan.per)[:, plan.o_main:].reshape(self.S, L, plan.per_l)
        want, rr_all = np.empty_like(rest), np.empty_like(rest)
        for o, n, r2 in ((0, spp, plan.lc.enp_r2), (2 * spp, GEO_SPP, plan.lc.enp_r2_shrunk)):
            ut, ur = rest[:, :, o:o + n], rest[:, :, o + n:o + 2 * n]
            rr = np.sqrt(ur * float(r2))
            want[:, :, o:o + n], want[:, :, o + n:o + 2 * n] = rr * np.cos(2 * np.pi * ut), rr * np.sin(2 * np.pi * ut)
            rr_all[:, :, o:o + n] = rr_all[:, :, o + n:o + 2 * n] = rr
        return want, rr_all


_CASES = {}
CASES = [pytest.param(2048, 2, False, id="spp2048-S2"), pytest.param(300, 2, False, id="spp300-S2"),
         pytest.param(2048, 5, True, id="spp2048-S5-staged"), pytest.param(300, 5, True, id="spp300-S5-staged")]


def case(repo_root, spp, S, staged):
    key = (spp, S, staged)
    if key not in _CASES:
        _CASES[key] = Case(repo_root, spp, S, staged)
    return _CASES[key]


@pytest.mark.parametrize("spp,S,staged", CASES)
def test_points_against_float64_and_weights_to_the_bit(repo_root, margin, spp, S, staged):
    """(a): every row of every state, the late ones of a staged launch included; and the prologue's weights are aadff_chief_fit_weights'"""
    c = case(repo_root, spp, S, staged)
    got = c.pts_run["xy"].astype(np.float64).reshape(S, L, -1)
    want, rr = c.points_float64()
    assert got.shape == want.shape and np.isfinite(got).all()
    ratio = np.abs(got - want) / (POINT_REL * rr + 1e-30)
    s, l, e = np.unravel_index(ratio.argmax(), ratio.shape)
    print(f"spp {spp} S {S} staged {staged}: points vs float64, max |d| {np.abs(got - want).max():.3e} mm; worst |d| / bound {ratio.max():.3f} at state {s}, "
          f"wavelength {l}, element {e} (rr {rr[s, l, e]:.3f} mm); late states alone {ratio[c.first:].max() if staged else float('nan'):.3f}")
    margin(f"pupil points spp {spp} S {S}{' staged' if staged else ''}: worst |d| / (6.7e-7 rr)", ratio.max(), 1.0)
    for run in (c.pts_run, c.per_l_run, c.raw_run):
        assert np.array_equal(run["w"].view(np.int32), c.w_old.cpu().numpy().view(np.int32))
    assert np.isnan(c.raw_run["xy"]).all()                           # AADFF_PSF_POINTS=raw: no points written, none read


@pytest.mark.parametrize("spp,S,staged", CASES)
def test_node_rays_once_per_state_equal_the_wave_per_wavelength(repo_root, spp, S, staged):
    """(b): bit for bit, every record; a corner's guard (a) fails (rf50mm vignettes it inside the shrunk pupil), the axial point's passes"""
    c = case(repo_root, spp, S, staged)
    once, per_l = c.pts_run["fitc"], c.per_l_run["fitc"]
    assert np.isfinite(once).all() and np.array_equal(once.view(np.int32), per_l.view(np.int32))
    assert np.array_equal(once.view(np.int32), c.raw_run["fitc"].view(np.int32))
    ok = once[..., 2] != 0
    assert ok[:, :, CENTRE].all(), "the axial point's node and ring rays are all alive: guard (a) passes, the fitted centre stands"
    assert not ok[:, :, CORNER].all(), "a corner of rf50mm at grid 3 is vignetted: guard (a) fails"


@pytest.mark.parametrize("spp,S,staged", CASES)
def test_psfs_from_points_against_raw_draws(repo_root, margin, spp, S, staged):
    """(c) and (d): fitted workgroups (main pass from points) and fallback workgroups (chief pass from points too), both present"""
    c = case(repo_root, spp, S, staged)
    new, raw = c.pts_run, c.raw_run
    ok = np.transpose(new["fitc"][..., 2] != 0, (0, 2, 1))           # [S,N,L], as the PSFs
    assert ok.any() and (~ok).any(), "both fitted and fallback workgroups must occur"
    assert np.isfinite(new["psf"]).all() and np.isfinite(raw["psf"]).all() and np.isfinite(new["cen"]).all()
    tag = f"spp {spp} S {S}{' staged' if staged else ''}"
    for name, sel in (("fitted", ok), ("fallback", ~ok)):
        a, b = new["psf"][sel].astype(np.float64), raw["psf"][sel].astype(np.float64)
        margin(f"pupil points {tag}: {name} workgroups' PSFs vs raw draws, rel-L2", np.linalg.norm(a - b) / np.linalg.norm(b), PSF_TOL)
        margin(f"pupil points {tag}: {name} PSFs, worst single PSF rel-L2", max(np.linalg.norm(x - y) / np.linalg.norm(y) for x, y in zip(a, b)), PSF_TOL)
    okc = np.transpose(ok, (0, 2, 1))                                # [S,L,N], as the centres
    assert np.array_equal(new["cen"][okc], raw["cen"][okc])          # a fitted centre is the node-ray kernel's: no draw enters it
    margin(f"pupil points {tag}: fallback centres vs raw draws [mm]", np.abs(new["cen"][~okc] - raw["cen"][~okc]).max(), CENTRE_TOL)
    d = np.abs(new["psf"].astype(np.float64) - raw["psf"]).max()
    print(f"{tag}: PSFs from points vs raw draws, max |d| of an element {d:.3e} (largest element {raw['psf'].max():.3e}); fitted {ok.sum()} of {ok.size}")
    for run in (c.pts_run, c.per_l_run, c.raw_run):
        assert run["flags"] == 0, f"flags word {run['flags']:#x} (bit 3: a staged block came late)"
    if staged:
        assert c.late_untouched, "a launch with points must not copy the late states' draws"
        assert torch.equal(c.u_dev, c.u)                             # the raw launch after it staged them, on the same counters
