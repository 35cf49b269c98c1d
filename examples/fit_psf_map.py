#!/usr/bin/env python3
"""Recover an 11 x 11-grid PSF map from a (sharp image, blurred image) pair by gradient descent through the HIP renderer.

    python examples/fit_psf_map.py [steps] [size]

Synthetic data (aadff.synth, no files): a sharp image and a "true" PSF map of Gaussian blobs whose width grows with the field
radius; the blurred image is rendered once with the forward kernel.  The unknown map starts as a flat box blur and is fitted with
Adam on the re-rendering loss; the gradient to the PSF map comes from aadff.diffrender.render_psf_map (csrc/conv_bwd.hip).  The
parametrisation is a softmax per PSF, so every PSF stays positive and normalised."""
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.diffrender import render_psf_map          # noqa: E402
from aadff.synth import synth_rgb                    # noqa: E402

steps = int(sys.argv[1]) if len(sys.argv) > 1 else 300
size = int(sys.argv[2]) if len(sys.argv) > 2 else 512
dev = torch.device("cuda:0")
grid, ks = 11, 11


def to_map(p):
    """[3, grid, grid, ks, ks] PSFs -> the [3, grid*ks, grid*ks] map layout of render_psf_map."""
    return p.permute(0, 1, 3, 2, 4).reshape(3, grid * ks, grid * ks)


# the "true" map: Gaussians, sigma 0.6 px on the axis to 2.2 px in the corners, a little wider in red than in blue
ax = torch.arange(ks, dtype=torch.float32) - ks // 2
r2 = (ax[:, None] ** 2 + ax[None, :] ** 2)[None, None, None]
c = (torch.arange(grid, dtype=torch.float32) + 0.5) / grid * 2 - 1
field = torch.sqrt(c[:, None] ** 2 + c[None, :] ** 2)[None, :, :, None, None] / 2 ** 0.5
sigma = (0.6 + 1.6 * field) * torch.tensor([1.15, 1.0, 0.9])[:, None, None, None, None]
true = torch.exp(-r2 / (2 * sigma ** 2))
true = to_map(true / true.sum((-1, -2), keepdim=True)).contiguous().to(dev)

sharp = torch.from_numpy(synth_rgb(size, size))[None].to(dev)
with torch.no_grad():
    blurred = render_psf_map(sharp, true, grid)

logits = torch.zeros(3, grid, grid, ks * ks, device=dev, requires_grad=True)       # flat start: a box blur
opt = torch.optim.Adam([logits], lr=0.1)
for step in range(steps + 1):
    est = to_map(torch.softmax(logits, -1).reshape(3, grid, grid, ks, ks))
    loss = torch.mean((render_psf_map(sharp, est, grid) - blurred) ** 2)
    if step % 25 == 0 or step == steps:
        with torch.no_grad():
            err = (est - true).norm() / true.norm()
        print(f"step {step:4d}  re-rendering MSE {loss.item():.3e}  PSF map rel-L2 error {err.item():.3f}")
    if step < steps:
        opt.zero_grad(set_to_none=True)
        loss.backward()
        opt.step()
