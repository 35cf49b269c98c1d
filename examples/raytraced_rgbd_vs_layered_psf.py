#!/usr/bin/env python3
"""One RGB-D scene through the lens three times: ray traced with occlusion, by the layered PSF-grid approximation with a per-pixel
layer selection, and by the same PSF grids composited front to back (occlusion-aware).

    python examples/raytraced_rgbd_vs_layered_psf.py [--lens rf50mm] [--size 256 256] [--layers 8] [--spp 64] [--band 8] [--out .]

The scene is a disc at -600 mm in front of a background that slants from -1500 mm (left) to -3000 mm (right).  Both routes quantise
the depth map with the same `aadff.focal_stack.depth_layers`:

1. `lens.render_raytraced_rgbd(img, depth, layers)`: every ray walks the planes nearest first and composites what it meets with a
   transmittance (aadff.raytrace).  A blurred background cannot bleed through the sharp disc, and the blurred disc
   covers the background only in proportion to the rays it stops.
2. `render_focal_stack_m1_layered(lens, img, depth, focus, layers)`: per layer one 11 x 11 grid of PSFs, each pixel takes the
   render of its own layer.  No occlusion: next to the edge, a pixel's PSF gathers texels of the other surface as if they lay at its
   own depth.
3. `render_focal_stack_m1_layered(..., occlusion=True)`: the same refocus and PSF-grid launches; per layer the premultiplied image and
   the mask are blurred with the layer's PSFs and the layers are composited front to back with a transmittance
   (aadff.occlusion) - the pixel-level form of route 1's per-ray rule.
The lens is focused once on the disc and once on the background behind it.  Printed: mean |difference| (green) to the ray-traced picture
inside a band of `--band` pixels around the disc's edge and outside it, per focus, for both PSF routes.  The ray-traced renders are
saved as PNG.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.focal_stack import render_focal_stack_m1_layered                # noqa: E402
from aadff.synth import synth_disc_depth_mm, synth_rgb                     # noqa: E402
from deeplens.optics import Lensgroup                                      # noqa: E402
from deeplens.utils import save_image                                      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lens", default="rf50mm")
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--layers", type=int, default=8)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--band", type=int, default=8)
ap.add_argument("--out", default=".")
a = ap.parse_args()
H, W = a.size
DEV = "cuda:0"

torch.manual_seed(0)
lens = Lensgroup(os.path.join(REPO, "lenses", a.lens, "lens.json"), sensor_res=(H, W), device=DEV)
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(DEV)
depth_np, disc = synth_disc_depth_mm(H, W)
depth = torch.from_numpy(depth_np)[None, None].to(DEV)
focus = [float(depth_np[disc].mean()), float(depth_np[H // 2, :][~disc[H // 2, :]].mean())]          # the disc, the background beside it

torch.manual_seed(0)
by_psf = render_focal_stack_m1_layered(lens, img, depth, focus, layers=a.layers)                      # [1,3,2,H,W]
torch.manual_seed(0)                                                                                  # the same draws: the same PSF grids
by_occl = render_focal_stack_m1_layered(lens, img, depth, focus, layers=a.layers, occlusion=True)
traced = []
for k, fd in enumerate(focus):
    lens.refocus(fd)
    out, zs = lens.render_raytraced_rgbd(img, depth, layers=a.layers, spp=a.spp, seed=7)              # scales: calc_scale_ray per plane
    traced.append(out)
traced = torch.stack(traced, dim=2)

# distance (pixels) of every pixel from the disc's edge
yy, xx = np.mgrid[0:H, 0:W]
rad = np.sqrt((yy - (H - 1) / 2) ** 2 + (xx - (W - 1) / 2) ** 2)
edge = torch.from_numpy(np.abs(rad - rad[disc].max()) <= a.band).to(DEV)
diffs = {"select": (traced - by_psf).abs()[0, 1], "occlusion-aware": (traced - by_occl).abs()[0, 1]}          # green, [2,H,W]
print(f"{a.lens} at {H} x {W}, {a.layers} layers at {[round(float(z)) for z in zs[0]]} mm, {a.spp} rays per pixel and channel")
print(f"mean |ray-traced - layered PSF grid| (green, image range 0..1), band = {a.band} px around the disc's edge")
for k, (fd, what) in enumerate(zip(focus, ("disc", "background"))):
    for route, diff in diffs.items():
        print(f"  focus {fd:8.1f} mm ({what:10s})  {route:15s}  inside the band {float(diff[k][edge].mean()):.4f}   outside {float(diff[k][~edge].mean()):.4f}")
    path = os.path.join(a.out, f"render_raytraced_rgbd_{what}.png")
    save_image(traced[0, :, k].clamp(0, 1), path)
    print("  wrote", path)
