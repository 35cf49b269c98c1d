#!/usr/bin/env python3
"""Soft depth from focus: the differentiable head on top of the classical focus measure, fitted with the reference's loss.

    python examples/soft_depth_from_focus.py [--steps 200] [--size 96 128] [--slices 8] [--window 9] [--conv]

1. A thin-lens focal stack of a synthetic scene with known depth (aadff.diffrender.thinlens_render_stack): the "camera".
2. aadff.dfocus.depth_from_stack gives the hard estimate (argmax over the slices plus a three-point fit) and the focus volume F.
3. scores = beta * log(F + eps) go through aadff.focus_head.attention_depth: a soft-argmax over the slices in 1 / focus distance, that is
   depth = 1 / sum_s softmax(scores)_s u_s, with gradients.  beta (and with --conv a one-layer plain-torch Conv3d on the scores) is fitted
   with aadff.focus_head.dff_losses(task="D_FS") against the true inverse depth.
Printed: mean |depth error| of the hard estimator and of the soft one before and after the fit.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.dfocus import depth_from_stack                                   # noqa: E402
from aadff.diffrender import thinlens_render_stack                          # noqa: E402
from aadff.focus_head import AttentionHead, dff_losses                      # noqa: E402
from aadff.synth import synth_depth_mm, synth_rgb                           # noqa: E402
from deeplens.psfnet import ThinLens                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--steps", type=int, default=200)
ap.add_argument("--size", type=int, nargs=2, default=(96, 128))
ap.add_argument("--slices", type=int, default=8)
ap.add_argument("--window", type=int, default=9)
ap.add_argument("--conv", action="store_true", help="also fit a Conv3d(1, 1, 3) on the scores")
a = ap.parse_args()
H, W = a.size
dev = torch.device("cuda:0")

thin = ThinLens(foc_len=50.0, fnum=1.8, kernel_size=11, sensor_size=[0.05 * H, 0.05 * W], sensor_res=(H, W))
near, far = 600.0, 3000.0                              # mm
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(dev)
depth_true = -torch.from_numpy(synth_depth_mm(H, W, seed=4, dmin=near, dmax=far, planes=6))[None, None].to(dev)
fds = -1.0 / torch.linspace(1.0 / near, 1.0 / far, a.slices, device=dev)[None]           # uniform in 1 / distance
with torch.no_grad():
    stack = thinlens_render_stack(thin, img, depth_true, fds)

hard = depth_from_stack(stack, fds, window=a.window, return_volume=True)
print(f"hard estimate (argmax + fit, window {a.window}):        |depth error| mean {(hard.depth - depth_true).abs().mean().item():7.1f} mm")

u = 1000.0 / fds.abs()                                 # the head works in dioptres: the slices are uniform there, and gt > 0 is the mask
gt = 1000.0 / depth_true.abs()
log_f = torch.log(hard.volume + 1e-8)[:, None]         # [N,1,S,H,W]
head = AttentionHead()
beta = torch.ones((), device=dev, requires_grad=True)
conv = torch.nn.Conv3d(1, 1, 3, padding=1).to(dev) if a.conv else None
if conv is not None:
    with torch.no_grad():                              # start as the identity
        conv.weight.zero_()
        conv.weight[0, 0, 1, 1, 1] = 1.0
        conv.bias.zero_()


def soft():
    scores = beta * log_f
    return head(conv(scores) if conv is not None else scores, stack, u)


def report(name):
    with torch.no_grad():
        inv, _ = soft()
        err = (-1000.0 / inv - depth_true).abs().mean().item()
    print(f"soft estimate, {name:30s} |depth error| mean {err:7.1f} mm   (beta {beta.item():.2f})")


report("before the fit:")
opt = torch.optim.Adam([beta] + (list(conv.parameters()) if conv is not None else []), lr=0.05)
for step in range(a.steps):
    inv, aif = soft()
    losses = dff_losses(inv, aif, gt_depth=gt, task="D_FS")
    opt.zero_grad(set_to_none=True)
    losses["total"].backward()
    opt.step()
report(f"after {a.steps} Adam steps:")
