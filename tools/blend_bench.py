#!/usr/bin/env python3
"""Time the blended PSF-map render (aadff_render_psf_map_blend_stack, csrc/conv_blend.hip) at 1024 x 1024, 3 channels, 10 slices, ks 11,
grid 7 and 11, in one run against
  (a) the patch stack render_psf_map_stack on the same maps, and
  (b) the composition the blend replaces: per-pixel PSFs [1,H,W,ks,ks] interpolated in torch from the map and fed to local_psf_render -
      ONE slice, one channel's PSFs for all three channels (the cheapest form of it; a stack costs S x that, RGB PSFs 3 x).

    python tools/blend_bench.py [--size 1024] [--slices 10] [--ks 11] [--grids 7 11] [--reps 5] [--inner 20]

Each figure is the median over --reps of the mean of --inner back-to-back launches between two stream events (microseconds per call),
after warm-up calls; inputs stay resident, so L2 is as warm as back-to-back calls leave it.  One JSON line per grid."""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np
import torch

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]
from aadff import _abi                                                      # noqa: E402
from aadff.blend import blend_nodes, render_psf_map_blend_stack             # noqa: E402
from deeplens.render_psf import local_psf_render, render_psf_map_stack      # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--slices", type=int, default=10)
ap.add_argument("--ks", type=int, default=11)
ap.add_argument("--grids", type=int, nargs="+", default=[7, 11])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=20)
a = ap.parse_args()
dev = torch.device("cuda:0")
H = W = a.size
S, ks = a.slices, a.ks


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


def interpolated(map_c, g):
    """[1,H,W,ks,ks]: the per-pixel PSFs of one [g ks, g ks] map, flipped for local_psf_render (which does not flip)."""
    t = map_c.reshape(g, ks, g, ks).permute(0, 2, 1, 3)
    out = []
    for n in (H, W):
        node = blend_nodes(n, g).to(dev)
        p = torch.arange(n, device=dev, dtype=torch.float32)
        k = ((node[None, :] <= p[:, None]).sum(1) - 1).clamp(0, g - 2)
        out.append((k, ((p - node[k]) / (node[k + 1] - node[k])).clamp(0, 1)))
    (ky, fy), (kx, fx) = out
    fy, fx = fy[:, None, None, None], fx[None, :, None, None]
    top = torch.lerp(t[ky][:, kx], t[ky][:, kx + 1], fx)
    bot = torch.lerp(t[ky + 1][:, kx], t[ky + 1][:, kx + 1], fx)
    return torch.lerp(top, bot, fy).flip(-1, -2)[None].contiguous()


gen = torch.Generator().manual_seed(0)
img = torch.rand((1, 3, H, W), generator=gen).to(dev)
for g in a.grids:
    maps = torch.rand((S, 3, g * ks, g * ks), generator=gen).to(dev) / (ks * ks)
    with torch.no_grad():
        # the two stack entries through the C ABI directly: the custom-op dispatcher's ~35 us of Python per call is the patch kernel's own time
        out, st = torch.empty((1, 3, S, H, W), device=dev), _abi.stream_ptr(dev)
        ny, nx = blend_nodes(H, g), blend_nodes(W, g)
        hp = lambda t: C.c_void_p(t.data_ptr())                                                    # noqa: E731
        t_blend = timed(lambda: _abi.call("aadff_render_psf_map_blend_stack", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(out), hp(ny), hp(nx),
                                          1, 3, S, H, W, g, ks, st), a.inner)
        assert torch.equal(out, render_psf_map_blend_stack(img, maps, g))
        t_patch = timed(lambda: _abi.call("aadff_render_psf_map_stack", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(out), 1, 3, S, H, W, g, ks, st), a.inner)
        assert torch.equal(out, render_psf_map_stack(img, maps, g))
        t_interp = timed(lambda: interpolated(maps[0, 0], g), 2)
        psfs = interpolated(maps[0, 0], g)
        t_gather = timed(lambda: local_psf_render(img, psfs, kernel_size=ks), 5)
        # the two routes give one picture (channel 0 of slice 0, away from the border where the paddings differ)
        p = ks // 2
        x, y = render_psf_map_blend_stack(img, maps[:1], g)[0, 0, 0, p:-p, p:-p], local_psf_render(img, psfs, kernel_size=ks)[0, 0, p:-p, p:-p]
        agree = float((x - y).norm() / y.norm())
        del psfs
    print(json.dumps({"tool": "blend_bench", "H": H, "W": W, "C": 3, "S": S, "ks": ks, "grid": g,
                      "blend_stack_us": round(t_blend, 1), "patch_stack_us": round(t_patch, 1), "blend_over_patch": round(t_blend / t_patch, 2),
                      "composed_one_slice_us": round(t_interp + t_gather, 1), "composed_interpolate_us": round(t_interp, 1),
                      "composed_gather_us": round(t_gather, 1), "composed_stack_over_blend_stack": round(S * (t_interp + t_gather) / t_blend, 1),
                      "blend_vs_composed_rel_l2": agree}), flush=True)
