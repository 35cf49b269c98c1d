#!/usr/bin/env python3
"""Why depth from focus is sure in the centre and unsure in a corner: the lens's through-focus MTF beside the estimator's confidence.

    python examples/through_focus_mtf.py [--size 96 128] [--freq 20] [--span 0.6] [--steps 13] [--slices 9] [--spp 64]

1. rf50mm focused at 2 m.  Lensgroup.mtf gives, in one fused launch, the MTF at `--freq` cycles/mm of a 3 x 3 grid of field points on
   `--steps` sensor planes around focus (tangential and sagittal, three colours).  Printed per field point: the MTF in focus, the sensor
   shift of its through-focus peak (over the field: the field-curvature map) and the width of the curve at half its peak - the depth
   of focus the estimator can resolve there.
2. A plane scene at 2 m rendered through the same lens as a ray-traced focal stack (aadff.raytrace.render_raytraced_stack), and
   aadff.dfocus.depth_from_stack on it.  Printed for the same 3 x 3 regions of the image: the estimator's peak confidence and its
   depth error.  Where the through-focus curve is low and wide, the confidence is low and the error large.
"""
import argparse
import os
import sys

import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff.dfocus import depth_from_stack                                   # noqa: E402
from aadff.raytrace import render_raytraced_stack                           # noqa: E402
from aadff.synth import synth_rgb                                           # noqa: E402
from deeplens.optics import Lensgroup                                       # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, nargs=2, default=(96, 128))
ap.add_argument("--freq", type=float, default=20.0)
ap.add_argument("--span", type=float, default=0.6)
ap.add_argument("--steps", type=int, default=13)
ap.add_argument("--slices", type=int, default=9)
ap.add_argument("--spp", type=int, default=64)
a = ap.parse_args()
H, W = a.size
depth = -2000.0
dev = torch.device("cuda:0")

lens = Lensgroup(os.path.join(REPO, "lenses", "rf50mm", "lens.json"), sensor_res=(H, W), device=dev)
torch.manual_seed(0)
lens.refocus(depth)

# 1. field x through-focus MTF, one launch
field = (-0.9, 0.0, 0.9)
points = torch.tensor([[x, y, depth] for y in reversed(field) for x in field])
delta = torch.linspace(-a.span / 2, a.span / 2, a.steps)
res = lens.mtf(points, [a.freq], defocus=delta.tolist())
curve = res.mtf[..., 0].mean(1)                                             # [P,Z,2]: mean over the three colours
print(f"rf50mm at {-depth:.0f} mm, MTF at {a.freq:g} cycles/mm, {a.steps} sensor planes over +-{a.span / 2:g} mm (T / S)")
step = float(delta[1] - delta[0])
for p in range(points.shape[0]):
    row = []
    for k in range(2):
        c = curve[p, :, k]
        i = int(c.argmax())
        width = float((c >= 0.5 * c.max()).sum()) * step
        row.append(f"in focus {float(c[a.steps // 2]):.2f}  peak {float(c.max()):.2f} at {float(delta[i]):+.3f} mm  half-width {width:.2f} mm")
    print(f"  field ({float(points[p, 0]):+.1f}, {float(points[p, 1]):+.1f}):  T {row[0]}   S {row[1]}")

# 2. the estimator on a rendered stack of a plane at the same depth
img = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(dev)
fds = -1.0 / torch.linspace(1.0 / 1200.0, 1.0 / 6000.0, a.slices)
stack = render_raytraced_stack(lens, img, depth, fds, spp=a.spp, seed=1)
est = depth_from_stack(stack, fds.to(dev)[None])
err = (1.0 / est.depth - 1.0 / depth).abs() * 1e3                           # in 1/m: what the stack samples uniformly
print(f"depth_from_stack on a ray-traced stack of {a.slices} slices: peak confidence and |1/depth error| [1/m] per image region")
hs, ws = [0, H // 3, 2 * H // 3, H], [0, W // 3, 2 * W // 3, W]
for i in range(3):
    cells = []
    for j in range(3):
        sl = (0, 0, slice(hs[i], hs[i + 1]), slice(ws[j], ws[j + 1]))
        cells.append(f"peak {float(est.peak[sl].mean()):8.4f} err {float(err[sl].mean()):.3f}")
    print("  " + "   |   ".join(cells))
