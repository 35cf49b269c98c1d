#!/usr/bin/env python3
"""Depth from focus by analysis-by-synthesis: recover a depth map from a focal stack by gradient descent THROUGH the aberration-aware
renderer (aadff.diffrender.psfnet_render_stack: fused HIP forward, fused HIP backward to the depth map).

    python examples/depth_from_focus_fit.py [--ckpt PSFNet_rf50mm.pkl] [--fit-iters 2000] [--steps 300] [--size 96 128] [--slices 8]

1. A PSF network for lenses/rf50mm: loaded from --ckpt (a state_dict as PSFNet.train_psfnet / the reference saves it), or fitted here
   to ray-traced PSFs for --fit-iters iterations (a short fit: enough for PSFs that widen away from the focus distance).
2. A synthetic scene with known depth (aadff.synth): all-in-focus image, piecewise-planar depth map; its focal stack is rendered once.
3. The depth map is the unknown: z = sigmoid(logit) per pixel, depth = z2depth(z), flat start at the middle of the focus range;
   Adam on the re-rendering MSE of the whole stack.
Prints the stack MSE and the mean absolute depth error before and after (all pixels, and the pixels where the image has texture:
without texture a blur leaves no trace in the stack and the depth there is not observable)."""
import argparse
import os
import sys
import tempfile

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.diffrender import psfnet_render_stack      # noqa: E402
from aadff.synth import synth_depth_mm, synth_rgb     # noqa: E402
from deeplens.psfnet import PSFNet                    # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--ckpt", default=None)
ap.add_argument("--fit-iters", type=int, default=2000)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--size", type=int, nargs=2, default=(96, 128))
ap.add_argument("--slices", type=int, default=8)
a = ap.parse_args()
H, W = a.size
dev = torch.device("cuda:0")

lens = PSFNet(os.path.join(REPO, "lenses", "rf50mm", "lens.json"), sensor_res=(H, W), kernel_size=11, device=dev)
if a.ckpt:
    lens.load_net(a.ckpt)
else:
    torch.manual_seed(0)
    with tempfile.TemporaryDirectory() as tmp:
        lens.train_psfnet(iters=a.fit_iters, bs=128, lr=1e-3, spp=2048, evaluate_every=10 ** 9, result_dir=tmp)
for p in lens.psfnet.parameters():
    p.requires_grad_(False)

near, far = 600.0, 3000.0                              # mm
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(dev)
depth_true = -torch.from_numpy(synth_depth_mm(H, W, seed=4, dmin=near, dmax=far, planes=6))[None, None].to(dev)
fds = -torch.linspace(near, far, a.slices, device=dev)[None]
with torch.no_grad():
    target = lens.render_stack(img, depth_true, fds)

z0 = 0.5 * (lens.depth2z(torch.tensor(-near)) + lens.depth2z(torch.tensor(-far)))
logit = torch.full_like(depth_true, float(torch.logit(z0)), requires_grad=True)
gx = (img[..., :, 1:] - img[..., :, :-1]).abs().mean(1, keepdim=True)
textured = torch.nn.functional.pad(gx, (0, 1)) > 0.02


def report(tag, depth, loss):
    err = (depth - depth_true).abs()
    print(f"{tag}: stack MSE {loss:.3e}   |depth error| mean {err.mean().item():7.1f} mm, on textured pixels {err[textured].mean().item():7.1f} mm")


opt = torch.optim.Adam([logit], lr=0.05)
for step in range(a.steps + 1):
    depth = lens.z2depth(torch.sigmoid(logit))
    loss = torch.mean((psfnet_render_stack(lens, img, depth, fds) - target) ** 2)
    if step == 0:
        report("start (flat depth)", depth.detach(), loss.item())
    if step == a.steps:
        report(f"after {a.steps} Adam steps", depth.detach(), loss.item())
        break
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
