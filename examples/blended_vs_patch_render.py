#!/usr/bin/env python3
"""One image through the lens three ways: PSF patches, blended PSFs, and rays traced for every pixel.

    python examples/blended_vs_patch_render.py [--lens rf50mm] [--size 512 512] [--depth -2000] [--focus -1000] [--grid 7] [--ks 21] [--spp 64]

1. `lens.psf_map(depth, grid, ks)`: one grid x grid map of ray-traced PSFs (the lens is focused at --focus, so the plane at --depth
   is blurred and the blur changes over the field).
2. `render_psf_map(img, psf_map, grid)`: every patch convolved with its own PSF - the picture jumps at the patch borders.
3. `render_psf_map_blend(img, psf_map, grid)`: every pixel's PSF interpolated bilinearly between the four grid PSFs around it
   (aadff/blend.py, one fused HIP launch) - continuous.
4. `lens.render_raytraced(img, depth)`: the picture both approximate (it also carries the distortion, which PSFs centred on their
   chief rays drop).
Printed for both PSF routes: the relative L2 distance to the ray-traced picture, and the seam measure - the mean |second difference|
of the picture ACROSS the patch lines (rows and columns int(i / grid * n)), beside the same measure over all other rows and columns:
a ratio near 1 means the patch lines cannot be told from the rest of the picture.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.synth import synth_rgb                                           # noqa: E402
from deeplens.optics import Lensgroup                                       # noqa: E402
from deeplens.render_psf import render_psf_map, render_psf_map_blend        # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lens", default="rf50mm")
ap.add_argument("--size", type=int, nargs=2, default=(512, 512))
ap.add_argument("--depth", type=float, default=-2000.0)
ap.add_argument("--focus", type=float, default=-1000.0)
ap.add_argument("--grid", type=int, default=7)
ap.add_argument("--ks", type=int, default=21)
ap.add_argument("--spp", type=int, default=64)
a = ap.parse_args()
H, W = a.size

torch.manual_seed(0)
lens = Lensgroup(os.path.join(REPO, "lenses", a.lens, "lens.json"), sensor_res=(H, W), device="cuda:0")
lens.refocus(a.focus)
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to("cuda:0")

psf_map = lens.psf_map(depth=a.depth, grid=a.grid, ks=a.ks)
patches = render_psf_map(img, psf_map, a.grid)
blended = render_psf_map_blend(img, psf_map, a.grid)
traced = lens.render_raytraced(img, depth=a.depth, spp=a.spp)


def rel_l2(x, ref):
    return float((x.double() - ref.double()).norm() / ref.double().norm())


def seam(x, n, dim):
    """(mean |second difference| across the patch lines of axis `dim`, the same over every other line)."""
    x = x.double().movedim(dim, -1)
    # d2[q]: the step q+1 -> q+2 against the mean of its two neighbours (zero where the picture is locally a parabola)
    d2 = (x[..., 2:-1] - x[..., 1:-2] - 0.5 * ((x[..., 1:-2] - x[..., :-3]) + (x[..., 3:] - x[..., 2:-1]))).abs()
    lines = torch.tensor([int(i / a.grid * n) for i in range(1, a.grid)], device=x.device) - 2     # the step b-1 -> b
    lines = lines[(lines >= 0) & (lines < d2.shape[-1])]
    on = torch.zeros(d2.shape[-1], dtype=torch.bool, device=x.device)
    on[lines] = True
    return float(d2[..., on].mean()), float(d2[..., ~on].mean())


print(f"{a.lens} at {H} x {W}, focused at {a.focus:g} mm, plane at {a.depth:g} mm, grid {a.grid}, ks {a.ks}; ray-traced picture: {a.spp} rays per pixel")
for name, pic in (("patches", patches), ("blended", blended)):
    (ry, oy), (rx, ox) = seam(pic, H, 2), seam(pic, W, 3)
    on, off = 0.5 * (ry + rx), 0.5 * (oy + ox)
    print(f"  {name:8s} rel L2 to ray-traced {rel_l2(pic, traced):.4f}   across patch lines {on:.5f}, elsewhere {off:.5f}: ratio {on / off:.2f}")
(ry, oy), (rx, ox) = seam(traced, H, 2), seam(traced, W, 3)
print(f"  ray-traced itself: across the same lines {0.5 * (ry + rx):.5f}, elsewhere {0.5 * (oy + ox):.5f}: ratio {(ry + rx) / (oy + ox):.2f}")
print(f"  blended vs patches rel L2 {rel_l2(blended, patches):.4f}")
