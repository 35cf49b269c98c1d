#!/usr/bin/env python3
"""Depth from focus through the cost-volume head of the reference's second network, DFVNet, on costs made without a network.

    python examples/cost_volume_depth_from_focus.py [--steps 100] [--size 96 128] [--slices 8] [--window 9]

1. A thin-lens focal stack of a synthetic scene with known depth (aadff.diffrender.thinlens_render_stack): the "camera".
2. aadff.dfocus.depth_from_stack(return_volume=True) gives the focus volume F.  The costs DFVNet's decoders would produce are replaced
   by beta * log(F + eps), average-pooled to 1/4 and 1/8 of the image: two decoder levels.
3. aadff.dfv_head.cost_volume_depth_levels upsamples each level to the image, takes the softmax over the slices and regresses the
   focus distance (in dioptres) and its standard deviation, as DFVNet.forward does in training.
4. aadff.focus_head.dff_losses(task="D_FS") per level, summed with DFVNet's level weights 8/15 and 4/15; a few Adam steps on one
   scale beta per level.
Printed: mean |depth error| of the finest level before and after the fit, and how std, the confidence map, sorts the error: the mean
error over the most and over the least confident half of the pixels.
"""
import argparse
import os
import sys

import torch
import torch.nn.functional as F

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.dfocus import depth_from_stack                                   # noqa: E402
from aadff.dfv_head import cost_volume_depth_levels                         # noqa: E402
from aadff.diffrender import thinlens_render_stack                          # noqa: E402
from aadff.focus_head import dff_losses                                     # noqa: E402
from aadff.synth import synth_depth_mm, synth_rgb                           # noqa: E402
from deeplens.psfnet import ThinLens                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=100)
ap.add_argument("--size", type=int, nargs=2, default=(96, 128))
ap.add_argument("--slices", type=int, default=8)
ap.add_argument("--window", type=int, default=9)
a = ap.parse_args()
H, W = a.size
dev = torch.device("cuda:0")
LEVEL_WEIGHTS = (8.0 / 15.0, 4.0 / 15.0)                # DFVNet's weights of its two finest levels

thin = ThinLens(foc_len=50.0, fnum=1.8, kernel_size=11, sensor_size=[0.05 * H, 0.05 * W], sensor_res=(H, W))
near, far = 600.0, 3000.0                              # mm
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(dev)
depth_true = -torch.from_numpy(synth_depth_mm(H, W, seed=4, dmin=near, dmax=far, planes=6))[None, None].to(dev)
fds = -1.0 / torch.linspace(1.0 / near, 1.0 / far, a.slices, device=dev)[None]           # uniform in 1 / distance
with torch.no_grad():
    stack = thinlens_render_stack(thin, img, depth_true, fds)
    volume = depth_from_stack(stack, fds, window=a.window, return_volume=True).volume      # [N,S,H,W]
    log_f = torch.log(volume + 1e-8)
    levels = [F.avg_pool2d(log_f, 4), F.avg_pool2d(log_f, 8)]                               # costs at 1/4 and 1/8 of the image

u = 1000.0 / fds.abs()                                 # dioptres: the slices are uniform there, and gt > 0 is the mask
gt = 1000.0 / depth_true.abs()
betas = torch.ones(len(levels), device=dev, requires_grad=True)


def heads():
    return cost_volume_depth_levels([b * c for b, c in zip(betas, levels)], u, (H, W))


def report(name):
    with torch.no_grad():
        preds, stds = heads()
        err = (-1000.0 / preds[0] - depth_true).abs().flatten()
        order = stds[0].flatten().argsort()                                                 # small std = confident
        half = err.numel() // 2
    print(f"{name:26s} |depth error| mean {err.mean().item():7.1f} mm; confident half {err[order[:half]].mean().item():7.1f} mm, "
          f"other half {err[order[half:]].mean().item():7.1f} mm   (beta {', '.join(f'{b:.2f}' for b in betas.tolist())})")


report("before the fit:")
opt = torch.optim.Adam([betas], lr=0.05)
for step in range(a.steps):
    preds, stds = heads()
    total = sum(wl * dff_losses(p, None, gt_depth=gt, task="D_FS")["total"] for wl, p in zip(LEVEL_WEIGHTS, preds))
    opt.zero_grad(set_to_none=True)
    total.backward()
    opt.step()
report(f"after {a.steps} Adam steps:")
