#!/usr/bin/env python3
"""A validation loop on the GPU: render, estimate, score - one read-back at the end.

    python examples/evaluate_depth_from_focus.py [--scenes 8] [--size 96 128] [--slices 8] [--window 9]

The shape of `validate()` in the reference's training script, on synthetic scenes with known depth: per scene
1. a thin-lens focal stack of the scene (aadff.diffrender.thinlens_render_stack): the "camera";
2. aadff.dfocus.depth_from_stack: depth from the stack and the all-in-focus composite, in place of the network;
3. aadff.metrics.Evaluator.update: the nine depth scores, PSNR and SSIM of the scene are added to running sums on the device.
Nothing is copied to the host inside the loop; Evaluator.result() reads the averages back once and the table is printed.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.dfocus import depth_from_stack                                   # noqa: E402
from aadff.diffrender import thinlens_render_stack                          # noqa: E402
from aadff.metrics import Evaluator                                         # noqa: E402
from aadff.synth import synth_depth_mm, synth_rgb                           # noqa: E402
from deeplens.psfnet import ThinLens                                        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--scenes", type=int, default=8)
ap.add_argument("--size", type=int, nargs=2, default=(96, 128))
ap.add_argument("--slices", type=int, default=8)
ap.add_argument("--window", type=int, default=9)
a = ap.parse_args()
H, W = a.size
dev = torch.device("cuda:0")

thin = ThinLens(foc_len=50.0, fnum=1.8, kernel_size=11, sensor_size=[0.05 * H, 0.05 * W], sensor_res=(H, W))
near, far = 600.0, 3000.0                              # mm
fds = -1.0 / torch.linspace(1.0 / near, 1.0 / far, a.slices, device=dev)[None]           # uniform in 1 / distance
ev = Evaluator()
with torch.no_grad():
    for i in range(a.scenes):
        img = torch.from_numpy(synth_rgb(H, W, seed=100 + i))[None].to(dev)
        depth_true = -torch.from_numpy(synth_depth_mm(H, W, seed=200 + i, dmin=near, dmax=far, planes=6))[None, None].to(dev)
        stack = thinlens_render_stack(thin, img, depth_true, fds)
        est = depth_from_stack(stack, fds, window=a.window)
        gt_m, est_m = depth_true.abs() / 1000.0, est.depth.abs() / 1000.0                # metres, positive, as the reference scores them
        ev.update(est_m, gt_m, gt_m > 0, est.aif, img)                                   # stays on the device
scores = ev.result()                                                                    # the one read-back
print(f"{a.scenes} scenes of {H} x {W}, {a.slices} slices, window {a.window}")
for k, v in scores.items():
    print(f"  Avg_{k:<12s} {v:10.5f}")
