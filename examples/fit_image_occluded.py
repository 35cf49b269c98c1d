#!/usr/bin/env python3
"""Recover the all-in-focus image from an occlusion-aware focal stack with known depth layers (deconvolution through the layered
composite), by Adam through aadff.diffrender.render_psf_map_occluded_stack (HIP forward and backward).

The stack is rendered from a test image with the occlusion-aware renderer: a disc over a slanted background, L depth layers, one
Gaussian PSF map per (slice, layer) whose width grows with the layer's distance from the slice's focus.  Two fits from the same start:
  occluded   the forward model that made the stack;
  selection  the per-pixel layer selection (every pixel takes the render of ITS layer, `render_psf_map_stack` per layer and a gather):
             the fast model without occlusion, whose error at the depth edges the fit absorbs into the image.
Printed: the relative L2 error of either recovered image against the true one, overall and within `--edge` pixels of a layer boundary.

    python examples/fit_image_occluded.py [--size 192] [--layers 4] [--slices 5] [--steps 300]
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff import diffrender                                                # noqa: E402
from aadff.focal_stack import depth_layers                                  # noqa: E402
from aadff.occlusion import render_psf_map_occluded_stack                   # noqa: E402
from aadff.synth import synth_disc_depth_mm, synth_rgb                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=192)
ap.add_argument("--layers", type=int, default=4)
ap.add_argument("--slices", type=int, default=5)
ap.add_argument("--grid", type=int, default=3)
ap.add_argument("--ks", type=int, default=11)
ap.add_argument("--steps", type=int, default=300)
ap.add_argument("--lr", type=float, default=0.03)
ap.add_argument("--edge", type=int, default=6)
a = ap.parse_args()
dev = torch.device("cuda:0")
H = W = a.size
L, S, grid, ks = a.layers, a.slices, a.grid, a.ks


def gaussian_maps():
    """[S L,3,grid ks,grid ks]: slice s is focused on layer s (L - 1) / (S - 1); sigma grows with the distance in layers."""
    r = torch.arange(ks, dtype=torch.float32) - ks // 2
    rr = r[:, None] ** 2 + r[None, :] ** 2
    tiles = []
    for s in range(S):
        focus = s * (L - 1) / max(S - 1, 1)
        for l in range(L):
            sigma = 0.35 + 1.1 * abs(l - focus)
            k = torch.exp(-rr / (2 * sigma * sigma))
            tiles.append((k / k.sum()).repeat(grid, grid)[None].expand(3, -1, -1))
    return torch.stack(tiles).contiguous().to(dev)


def selection_stack(x, maps, lay):
    """The per-pixel layer selection, differentiable: [1,3,S,H,W]."""
    out = 0.0
    for l in range(L):
        out = out + torch.where((lay == l)[:, None, None], diffrender.render_psf_map_stack(x, maps[l::L], grid), 0.0)
    return out


def fit(model, target):
    x = torch.full((1, 3, H, W), 0.5, device=dev, requires_grad=True)
    opt = torch.optim.Adam([x], lr=a.lr)
    for _ in range(a.steps):
        opt.zero_grad()
        loss = (model(x) - target).square().mean()
        loss.backward()
        opt.step()
    return x.detach(), float(loss.detach())


truth = torch.from_numpy(synth_rgb(H, W))[None].to(dev)
depth = torch.from_numpy(synth_disc_depth_mm(H, W)[0])[None].to(dev)
lay = depth_layers(depth, L)[0].reshape(1, H, W).to(torch.uint8).contiguous()
maps = gaussian_maps()
with torch.no_grad():
    target = render_psf_map_occluded_stack(truth, maps, lay, L, grid)

li = lay[0].long()
edge = torch.zeros((H, W), dtype=torch.bool, device=dev)
edge[:, 1:] |= li[:, 1:] != li[:, :-1]
edge[1:, :] |= li[1:, :] != li[:-1, :]
near = torch.nn.functional.max_pool2d(edge[None, None].float(), 2 * a.edge + 1, 1, a.edge)[0, 0] > 0


def err(x, mask=None):
    d, t = x - truth, truth
    if mask is not None:
        d, t = d[..., mask], t[..., mask]
    return float(d.norm() / t.norm())


for name, model in (("occluded", lambda x: diffrender.render_psf_map_occluded_stack(x, maps, lay, L, grid)),
                    ("selection", lambda x: selection_stack(x, maps, lay))):
    x, loss = fit(model, target)
    print(f"{name:>9}: final stack loss {loss:.3e}; image rel-L2 {err(x):.4f} overall, {err(x, near):.4f} within {a.edge} px of a layer "
          f"boundary ({100 * float(near.float().mean()):.1f} % of the pixels)")
