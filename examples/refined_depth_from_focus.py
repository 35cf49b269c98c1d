#!/usr/bin/env python3
"""Classical depth from focus, refined by its own confidence, as the starting point of an analysis-by-synthesis fit.

    python examples/refined_depth_from_focus.py [--steps 300] [--size 96 128] [--slices 8] [--window 9] [--radius 4] [--iterations 2]

1. The scene and the classical estimate of examples/depth_from_focus_classic.py: a thin-lens focal stack of a synthetic scene with
   known depth, turned into a depth map, a peak focus measure and an all-in-focus composite by aadff.dfocus.depth_from_stack.
2. aadff.refine.refine_depth(est.depth, confidence_from_peak(est.peak), est.aif): the confidence-weighted joint bilateral filter, in
   1 / depth, guided by the composite.  Printed before and after: mean |depth error| on all pixels, on the confident half (peak above
   its median) and on the unconfident half - the pixels the filter is for.
3. The analysis-by-synthesis fit of the classical example through the differentiable thin-lens renderer, the same number of Adam steps
   from the classical estimate and from the refined one.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.dfocus import depth_from_stack                                   # noqa: E402
from aadff.diffrender import thinlens_render_stack                          # noqa: E402
from aadff.refine import confidence_from_peak, refine_depth                 # noqa: E402
from aadff.synth import synth_depth_mm, synth_rgb                           # noqa: E402
from deeplens.psfnet import ThinLens                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--size", type=int, nargs=2, default=(96, 128))
ap.add_argument("--slices", type=int, default=8)
ap.add_argument("--window", type=int, default=9)
ap.add_argument("--interp", default="gaussian")
ap.add_argument("--radius", type=int, default=4)
ap.add_argument("--sigma-range", type=float, default=0.1)
ap.add_argument("--iterations", type=int, default=2)
a = ap.parse_args()
H, W = a.size
dev = torch.device("cuda:0")

# the scene of examples/depth_from_focus_classic.py
thin = ThinLens(foc_len=50.0, fnum=1.8, kernel_size=11, sensor_size=[0.05 * H, 0.05 * W], sensor_res=(H, W))
near, far = 600.0, 3000.0                              # mm
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(dev)
depth_true = -torch.from_numpy(synth_depth_mm(H, W, seed=4, dmin=near, dmax=far, planes=6))[None, None].to(dev)
fds = -1.0 / torch.linspace(1.0 / near, 1.0 / far, a.slices, device=dev)[None]           # uniform in 1 / distance
target = thin.render_stack(img, depth_true, fds)

est = depth_from_stack(target, fds, window=a.window, interp=a.interp)
confident = est.peak > est.peak.median()
ref = refine_depth(est.depth, confidence_from_peak(est.peak), est.aif, radius=a.radius, sigma_range=a.sigma_range, iterations=a.iterations)


def errors(depth):
    e = (depth.detach() - depth_true).abs()
    return e.mean().item(), e[confident].mean().item(), e[~confident].mean().item()


for name, depth in ((f"classical estimate (window {a.window}, {a.interp})", est.depth),
                    (f"refined (radius {a.radius}, sigma_range {a.sigma_range}, {a.iterations} iterations)", ref.depth)):
    print("%-62s |depth error| mean %7.1f mm, confident half %7.1f mm, unconfident half %7.1f mm" % ((name + ":",) + errors(depth)))

u_lo, u_hi = 1.0 / far, 1.0 / near                     # the depth map is the unknown: 1 / |depth| = u_lo + (u_hi - u_lo) sigmoid(logit)


def depth_of(logit):
    return -1.0 / (u_lo + (u_hi - u_lo) * torch.sigmoid(logit))


def fit(depth0):
    frac = ((1.0 / depth0.abs() - u_lo) / (u_hi - u_lo)).clamp(0.02, 0.98)
    logit = torch.logit(frac).clone().requires_grad_(True)
    opt = torch.optim.Adam([logit], lr=0.05)
    for step in range(a.steps + 1):
        depth = depth_of(logit)
        loss = torch.mean((thinlens_render_stack(thin, img, depth, fds) - target) ** 2)
        if step == a.steps:
            return (loss.item(),) + errors(depth)
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()


for name, start in (("classical start", est.depth), ("refined start", ref.depth)):
    print("fit, %d Adam steps from the %-15s: stack MSE %.3e   |depth error| mean %7.1f mm, confident half %7.1f mm, "
          "unconfident half %7.1f mm" % ((a.steps, name) + fit(start)))
