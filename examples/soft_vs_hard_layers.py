#!/usr/bin/env python3
"""Hard against soft depth layers in the occlusion-aware layered PSF render, at the same number of PSF maps.

    python examples/soft_vs_hard_layers.py [--lens rf50mm] [--size 256 256] [--layers 2 4 8] [--planes 32] [--spp 64] [--band 8]

The scene is the disc at -600 mm in front of a background that slants from -1500 mm (left) to -3000 mm (right)
(`aadff.synth.synth_disc_depth_mm`).  The truth is the ray-traced layered render with `--planes` planes and `--spp` rays per pixel and
channel (`lens.render_raytraced_rgbd`).  Against it, for every L of `--layers` and with the lens focused once on the disc
and once on the background beside it:

  hard  `render_focal_stack_m1_layered(..., layers=L, occlusion=True)`: every texel on one of L layers, blurred with that layer's PSF
        (DESIGN.md 4.20): a slanted surface becomes L stair steps of blur;
  soft  `render_focal_stack_m1_layered(..., layers=L, occlusion="soft")`: L nodes in depth, every texel blurred with the PSF
        interpolated between the two nodes around its own depth.

Both trace L PSF maps per slice on the same draws.  Printed: mean |difference| (green) to the truth inside a band of `--band` pixels
around the disc's edge and outside it (the slanted background and the disc's inside).
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

ap = argparse.ArgumentParser()
ap.add_argument("--lens", default="rf50mm")
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--layers", type=int, nargs="+", default=[2, 4, 8])
ap.add_argument("--planes", type=int, default=32)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--band", type=int, default=8)
a = ap.parse_args()
H, W = a.size
DEV = "cuda:0"

torch.manual_seed(0)
lens = Lensgroup(os.path.join(REPO, "lenses", a.lens, "lens.json"), sensor_res=(H, W), device=DEV)
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(DEV)
depth_np, disc = synth_disc_depth_mm(H, W)
depth = torch.from_numpy(depth_np)[None, None].to(DEV)
focus = [float(depth_np[disc].mean()), float(depth_np[H // 2, :][~disc[H // 2, :]].mean())]          # the disc, the background beside it

traced = []
for fd in focus:
    lens.refocus(fd)
    traced.append(lens.render_raytraced_rgbd(img, depth, layers=a.planes, spp=a.spp, seed=7)[0])
traced = torch.stack(traced, dim=2)                                                                   # [1,3,2,H,W]

yy, xx = np.mgrid[0:H, 0:W]
rad = np.sqrt((yy - (H - 1) / 2) ** 2 + (xx - (W - 1) / 2) ** 2)
edge = torch.from_numpy(np.abs(rad - rad[disc].max()) <= a.band).to(DEV)
print(f"{a.lens} at {H} x {W}; truth: ray traced, {a.planes} planes, {a.spp} rays per pixel and channel")
print(f"mean |truth - layered PSF render| (green, image range 0..1), band = {a.band} px around the disc's edge")
for L in a.layers:
    for route, occlusion in (("hard", True), ("soft", "soft")):
        torch.manual_seed(0)                                                                          # the same draws for both routes
        out = render_focal_stack_m1_layered(lens, img, depth, focus, layers=L, occlusion=occlusion)
        diff = (traced - out).abs()[0, 1]                                                             # green, [2,H,W]
        print(f"  L = {L:2d}  {route}   " + "   ".join(
            f"focus on the {what}: inside the band {float(diff[k][edge].mean()):.4f}  outside {float(diff[k][~edge].mean()):.4f}"
            for k, what in enumerate(("disc", "background"))), flush=True)
