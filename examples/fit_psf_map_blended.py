#!/usr/bin/env python3
"""Recover a 7 x 7-grid PSF map from a (sharp image, blurred image) pair by gradient descent through the BLENDED HIP renderer:
examples/fit_psf_map.py on the seam-free forward model, where every pixel's PSF is the bilinear blend of the four grid PSFs around it.

    python examples/fit_psf_map_blended.py [steps] [size]

Synthetic data (aadff.synth, no files): a sharp image and a "true" PSF map of Gaussian blobs whose width grows with the field radius,
sampled at the nodes where `psf_map` traces its PSFs; the blurred image is rendered once with the blended forward kernel.  The unknown
map starts as a flat box blur and is fitted with Adam on the re-rendering loss; the gradient to the PSF map comes from
aadff.diffrender.render_psf_map_blend (csrc/conv_blend_bwd.hip).  The parametrisation is a softmax per PSF, so every PSF stays positive
and normalised.  A fit through the patch renderer of the same blurred image would have to explain the smooth field with piecewise
constant PSFs; here the forward model is the one that made the data."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.diffrender import render_psf_map_blend    # noqa: E402
from aadff.synth import synth_rgb                    # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
size = int(sys.argv[2]) if len(sys.argv) > 2 else 512
dev = torch.device("cuda:0")
grid, ks = 7, 11


def to_map(p):
    """[3, grid, grid, ks, ks] PSFs -> the [3, grid*ks, grid*ks] map layout of render_psf_map_blend."""
    return p.permute(0, 1, 3, 2, 4).reshape(3, grid * ks, grid * ks)


# the "true" map: Gaussians, sigma 0.6 px on the axis to 2.2 px in the corners, a little wider in red than in blue, at the psf_map nodes
ax = torch.arange(ks, dtype=torch.float32) - ks // 2
r2 = (ax[:, None] ** 2 + ax[None, :] ** 2)[None, None, None]
c = torch.linspace(-0.98, 0.98, grid)
field = torch.sqrt(c[:, None] ** 2 + c[None, :] ** 2)[None, :, :, None, None] / 2 ** 0.5
sigma = (0.6 + 1.6 * field) * torch.tensor([1.15, 1.0, 0.9])[:, None, None, None, None]
true = torch.exp(-r2 / (2 * sigma ** 2))
true = to_map(true / true.sum((-1, -2), keepdim=True)).contiguous().to(dev)

sharp = torch.from_numpy(synth_rgb(size, size))[None].to(dev)
with torch.no_grad():
    blurred = render_psf_map_blend(sharp, true, grid)

logits = torch.zeros(3, grid, grid, ks * ks, device=dev, requires_grad=True)       # flat start: a box blur
opt = torch.optim.Adam([logits], lr=0.1)
for step in range(steps + 1):
    est = to_map(torch.softmax(logits, -1).reshape(3, grid, grid, ks, ks))
    loss = torch.mean((render_psf_map_blend(sharp, est, grid) - blurred) ** 2)
    if step % 25 == 0 or step == steps:
        with torch.no_grad():
            err = (est - true).norm() / true.norm()
        print(f"step {step:4d}  re-rendering MSE {loss.item():.3e}  PSF map rel-L2 error {err.item():.3f}")
    if step < steps:
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
