#!/usr/bin/env python3
"""Time the occlusion-aware layered PSF-map render (aadff_render_psf_map_stack_occluded, csrc/conv_occl.hip) at 1024 x 1024, 3 channels,
10 slices, ks 11, grid 7 and 11, L = 1, 4, 8, through the C ABI, on two scenes:
  disc    the scene of examples/raytraced_rgbd_vs_layered_psf.py (a disc over a slanted background) through depth_layers: most tiles hold
          one or two layers;
  random  a random layer per texel: every tile holds all L layers, the worst case.
In the same run the per-pixel layer selection aadff_render_psf_map_stack_layered is timed at the same shapes on the same inputs.

    python tools/occlusion_bench.py [--size 1024] [--slices 10] [--ks 11] [--grids 7 11] [--layers 1 4 8] [--reps 5] [--inner 20]

Each figure is the median over --reps of the mean of --inner back-to-back launches between two stream events (microseconds per call),
after warm-up calls; inputs stay resident.  Per line: the ratio to the selection entry's time, the mean number of layers present per
staged tile (what the kernel's layer loop visits, counted on the host from the layer map), and the share of the packed-FMA rate
(157.3 TFLOP/s fp32 vector peak = 78.65e12 FMA/s) for 2 ks^2 FMAs per output pixel, slice and layer present in its tile.  One JSON line
per (grid, L, scene)."""
import argparse
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff import _abi                                                      # noqa: E402
from aadff.focal_stack import depth_layers                                  # noqa: E402
from aadff.occlusion import render_psf_map_occluded_stack                   # noqa: E402
from aadff.synth import synth_disc_depth_mm                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--slices", type=int, default=10)
ap.add_argument("--ks", type=int, default=11)
ap.add_argument("--grids", type=int, nargs="+", default=[7, 11])
ap.add_argument("--layers", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=20)
a = ap.parse_args()
dev = torch.device("cuda:0")
H = W = a.size
S, ks, Cn = a.slices, a.ks, 3
PEAK_FMA = 157.3e12 / 2
TILE = 32


def timed(f, inner):
    for _ in range(3):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(a.reps):
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner * 1e3)
    return float(np.median(ts))


def reflect(i, n):
    i = np.abs(i)
    return np.where(i >= n, 2 * n - 2 - i, i)


def layer_visits(lay, L, g):
    """(sum over tiles of pixels x layers present in the staged tile, mean layers present per tile) of one [H,W] layer map."""
    lay, p = lay.cpu().numpy(), ks // 2
    hb, wb = [int(i / g * H) for i in range(g + 1)], [int(j / g * W) for j in range(g + 1)]
    work, tiles, present = 0, 0, 0
    for i in range(g):
        for y0 in range(hb[i], hb[i + 1], TILE):
            rows = reflect(np.arange(y0 - p, y0 + TILE + p), H)
            for j in range(g):
                for x0 in range(wb[j], wb[j + 1], TILE):
                    cols = reflect(np.arange(x0 - p, x0 + TILE + p), W)
                    seen = np.unique(lay[np.ix_(rows, cols)])
                    n = int((seen < L).sum())
                    work += n * (min(y0 + TILE, hb[i + 1]) - y0) * (min(x0 + TILE, wb[j + 1]) - x0)
                    tiles, present = tiles + 1, present + n
    return work, present / tiles


gen = torch.Generator().manual_seed(0)
img = torch.rand((1, Cn, H, W), generator=gen).to(dev)
depth = torch.from_numpy(synth_disc_depth_mm(H, W)[0])[None].to(dev)
out, st = torch.empty((1, Cn, S, H, W), device=dev), _abi.stream_ptr(dev)
with torch.no_grad():
    for g in a.grids:
        for L in a.layers:
            maps = (torch.rand((S * L, Cn, g * ks, g * ks), generator=gen) / (ks * ks)).to(dev)
            scenes = {"disc": depth_layers(depth, L)[0].reshape(1, H, W).to(torch.uint8).contiguous(),
                      "random": torch.randint(0, L, (1, H, W), generator=gen).to(torch.uint8).to(dev)}
            for name, lay in scenes.items():
                t_occl = timed(lambda: _abi.call("aadff_render_psf_map_stack_occluded", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(lay), _abi.ptr(out), None,
                                                 1, Cn, S, L, H, W, g, ks, 1, st), a.inner)
                assert torch.equal(out, render_psf_map_occluded_stack(img, maps, lay, L, g))
                t_sel = timed(lambda: _abi.call("aadff_render_psf_map_stack_layered", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(lay), _abi.ptr(out),
                                                1, Cn, S, L, H, W, g, ks, st), a.inner)
                work, per_tile = layer_visits(lay[0], L, g)
                fma = 2.0 * ks * ks * work * Cn * S
                print(json.dumps({"tool": "occlusion_bench", "H": H, "W": W, "C": Cn, "S": S, "ks": ks, "grid": g, "L": L, "scene": name,
                                  "occluded_stack_us": round(t_occl, 1), "select_stack_us": round(t_sel, 1), "occluded_over_select": round(t_occl / t_sel, 2),
                                  "layers_present_per_tile": round(per_tile, 2), "gfma": round(fma / 1e9, 2),
                                  "share_of_packed_fma_rate": round(fma / (t_occl * 1e-6) / PEAK_FMA, 3)}), flush=True)
