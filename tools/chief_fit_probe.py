"""The chief-centre fit at the bench configuration, one launch of 121 points x 3 wavelengths x 10 states: weights kernel
against numpy float64, share of workgroups that pass guard (a) and that take the fitted centre, fitted against full-pass centres and
PSFs, and |c_d - c_(d-2)| among the guard-(a) passers (what AADFF_CHIEF_FIT_TOL is held against).  Needs a GPU.

    python tools/chief_fit_probe.py [lens name] > profiles/chief_fit_probe_bench_config.txt
"""
import ctypes as C
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd"), os.path.join(REPO, "tools")]
import gen_chief_fit_tables as gen                         # noqa: E402
from aadff import _abi                                    # noqa: E402
from aadff.focal_stack import GEO_SPP, StackPlan           # noqa: E402
from aadff.synth import synth_depth_mm                     # noqa: E402
from deeplens.optics import Lensgroup                      # noqa: E402

DEV = "cuda:0"
H = W = 1024
S, GRID, KS, SPP = 10, 11, 11, 2048
K = _abi.CHIEF_NODES
lens_name = sys.argv[1] if len(sys.argv) > 1 else "rf50mm"
depth = synth_depth_mm(H, W, seed=5678)
dbar = -float(depth.mean())
fds = [float(f) for f in -np.linspace(depth.min(), depth.max(), S)]
lens = Lensgroup(os.path.join(REPO, "lenses", lens_name, "lens.json"), sensor_res=(H, W), device=DEV)
N = GRID * GRID
plan = StackPlan(lens, S, H, W, grid=GRID, ks=KS, spp=SPP)
torch.manual_seed(0)
u = plan.uniforms(lens.sampler)
ub = u.data_ptr()
dep, pts = plan.geometry(fds, dbar)
st = _abi.stream_ptr(torch.device(DEV))
_abi.call("aadff_refocus", _abi.ptr(dep), S, C.c_void_p(ub), GEO_SPP, plan.per, _abi.ptr(plan.tab_green), plan.lc, _abi.ptr(plan.states), st)
w = torch.full((S, 3, 2, K), float("nan"), device=DEV)
_abi.call("aadff_chief_fit_weights", C.c_void_p(ub + 4 * plan.o_chief), S, 3, GEO_SPP, plan.per, plan.per_l, None, _abi.ptr(w), st)
torch.cuda.synchronize()
wh = w.cpu().numpy().astype(np.float64)

# numpy float64 weights on the same uniforms
uh = u.cpu().numpy().reshape(S, plan.per)
xy, fd, fd2 = gen.tables()
worst = 0.0
for s in range(S):
    for l in range(3):
        o = plan.o_chief + l * plan.per_l
        ut, ur = uh[s, o:o + GEO_SPP].astype(np.float64), uh[s, o + GEO_SPP:o + 2 * GEO_SPP].astype(np.float64)
        x, y = np.sqrt(ur) * np.cos(2 * np.pi * ut), np.sqrt(ur) * np.sin(2 * np.pi * ut)
        m = gen.vandermonde(np.stack([x, y], 1), gen.DEGREE).mean(0)
        worst = max(worst, np.abs(fd @ m - wh[s, l, 0]).max(), np.abs(fd2 @ m[:fd2.shape[1]] - wh[s, l, 1]).max())
print(f"weights kernel vs numpy float64: max |d| {worst:.3e}; sum|w| {np.abs(wh[:, :, 0]).sum(-1).max():.3f}", flush=True)


fitc = torch.empty(S * 3 * N * 4, device=DEV)


def launch(weights):
    psf = torch.full((S, N, 3, KS, KS), float("nan"), device=DEV)
    cen = torch.full((S, 3, N, 2), float("nan"), device=DEV)
    _abi.call("aadff_psf_points_fit", _abi.ptr(pts), S, N, 3, _abi.ptr(plan.tab_rgb), _abi.ptr(plan.tab_green),
              plan.lc, _abi.ptr(plan.states), C.c_void_p(ub + 4 * plan.o_main), SPP, plan.per, plan.per_l,
              C.c_void_p(ub + 4 * plan.o_chief), GEO_SPP, plan.per, plan.per_l, KS, 1, 0, _abi.ptr(psf), _abi.ptr(cen), _abi.ptr(plan.flags),
              None if weights is None else _abi.ptr(weights), _abi.ptr(fitc), st)
    plan.check_flags()
    return psf.cpu().numpy().astype(np.float64), cen.cpu().numpy()


psf_full, c_full = launch(None)
psf_fit, c_fit = launch(w)
hi = w[:, :, :1].repeat(1, 1, 2, 1).contiguous()
lo = w[:, :, 1:].repeat(1, 1, 2, 1).contiguous()
_, c_hi = launch(hi)
_, c_lo = launch(lo)
wg_a = (c_hi != c_full).any(-1)                           # guard (a) passed (guard (b) is trivially true with twice the same vector)
wg_fit = (c_fit != c_full).any(-1)
d_trunc = np.abs(c_hi.astype(np.float64) - c_lo)[wg_a]
print(f"guard (a) passed: {wg_a.sum()} of {wg_a.size} ({wg_a.mean():.3f}); fitted (a and b): {wg_fit.sum()} ({wg_fit.mean():.3f})")
print(f"max |c_d - c_(d-2)| among guard-(a) passers: {d_trunc.max():.3e} mm; 99.9 %: {np.quantile(d_trunc, 0.999):.3e}; median {np.median(d_trunc):.3e}")
print(f"max |c_fit - c_full| among fitted: {np.abs(c_fit.astype(np.float64) - c_full)[wg_fit].max():.3e} mm; among guard-(a) passers with degree d: "
      f"{np.abs(c_hi.astype(np.float64) - c_full)[wg_a].max():.3e} mm")
print(f"PSF rel-L2 fit vs full: {np.linalg.norm(psf_fit - psf_full) / np.linalg.norm(psf_full):.3e}; finite: {np.isfinite(psf_fit).all()}")
# |c_d - c_(d-2)| below the resolution of a stored centre (one ulp of a 15 mm coordinate is 9.5e-7 mm): the kernel's centre is
# h0 + sum w (h - h0), so with w = 0 it is h0 and with w = 1024 (w_d - w_(d-2)) it is h0 + 1024 x the difference the guard compares
zero = torch.zeros_like(w)
dw = (1024.0 * (w[:, :, :1] - w[:, :, 1:])).repeat(1, 1, 2, 1).contiguous()
_, c_zero = launch(zero)
_, c_dw = launch(dw)
fine = np.abs(c_dw.astype(np.float64) - c_zero)[wg_a] / 1024.0
print(f"fine |c_d - c_(d-2)| among guard-(a) passers: max {fine.max():.3e} mm; 99.9 % {np.quantile(fine, 0.999):.3e}; 99 % {np.quantile(fine, 0.99):.3e}; "
      f"median {np.median(fine):.3e}; share > 1e-6: {(fine > 1e-6).mean():.4f}, > 5e-7: {(fine > 5e-7).mean():.4f}, > 2.5e-7: {(fine > 2.5e-7).mean():.4f}")
print("fitted share per state:", np.round(wg_fit.mean((1, 2)), 3))
