#!/usr/bin/env python3
"""The same image through the lens twice: by tracing rays for every pixel, and by the 7 x 7 PSF-grid approximation.

    python examples/raytraced_vs_psf_render.py [--lens rf50mm] [--size 256 256] [--depth -2000] [--spp 64] [--out .]

1. `lens.refocus(depth)`: the scene plane is in focus.
2. `lens.render_raytraced(img, depth)`: sensor pixel -> exit pupil -> backwards through the lens -> object plane -> sample the
   scene (aadff.raytrace, one fused HIP launch).  It carries the lens's distortion and lateral colour and has no patch seams.
3. `lens.render_single_img(img, depth, method="psf")`: a 7 x 7 grid of 21 x 21 PSFs, each convolved with its patch.  The PSFs
   are centred on their chief rays, so this route keeps the blur and drops the distortion.
Printed: mean |difference| per colour channel in three field zones (image radius / half diagonal below 1/3, 1/3 - 2/3, above), and
the share of valid rays per zone (the lens's vignetting).  Both renders are saved as PNG.
"""
import argparse
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.synth import synth_rgb                                           # noqa: E402
from deeplens.optics import Lensgroup                                       # noqa: E402
from deeplens.utils import save_image                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--lens", default="rf50mm")
ap.add_argument("--size", type=int, nargs=2, default=(256, 256))
ap.add_argument("--depth", type=float, default=-2000.0)
ap.add_argument("--spp", type=int, default=64)
ap.add_argument("--out", default=".")
a = ap.parse_args()
H, W = a.size

torch.manual_seed(0)
lens = Lensgroup(os.path.join(REPO, "lenses", a.lens, "lens.json"), sensor_res=(H, W), device="cuda:0")
lens.refocus(a.depth)
img8 = (synth_rgb(H, W, seed=3).transpose(1, 2, 0) * 255).round().astype(np.uint8)       # what render_single_img takes
img = torch.from_numpy(img8.astype(np.float32) / 255).permute(2, 0, 1)[None].to("cuda:0")

traced, aux = lens.render_raytraced(img, depth=a.depth, spp=a.spp, return_aux=True)      # scale: lens.calc_scale_ray(depth)
by_psf = lens.render_single_img(img8, depth=a.depth, method="psf", return_tensor=True)

yy, xx = torch.meshgrid(torch.arange(H, device="cuda:0") - (H - 1) / 2, torch.arange(W, device="cuda:0") - (W - 1) / 2, indexing="ij")
rad = torch.sqrt(xx ** 2 + yy ** 2) / (0.5 * (H ** 2 + W ** 2) ** 0.5)
diff = (traced - by_psf).abs()[0]
print(f"{a.lens} at {H} x {W}, plane at {a.depth:g} mm, {a.spp} rays per pixel and channel; mean |ray-traced - PSF grid| (image range 0..1)")
for name, lo, hi in (("centre", 0.0, 1 / 3), ("mid field", 1 / 3, 2 / 3), ("edge", 2 / 3, 2.0)):
    zone = (rad >= lo) & (rad < hi)
    r, g, b = (float(diff[c][zone].mean()) for c in range(3))
    print(f"  {name:9s}  R {r:.4f}  G {g:.4f}  B {b:.4f}   valid rays {float(aux['count'][:, zone].mean()) / a.spp:6.1%}")
for name, t in (("raytraced", traced), ("psf_grid", by_psf)):
    path = os.path.join(a.out, f"render_{name}.png")
    save_image(t[0].clamp(0, 1), path)
    print("wrote", path)
