#!/usr/bin/env python3
"""Time the gradients of the blended PSF-map render (aadff_render_psf_map_blend_stack_bwd, csrc/conv_blend_bwd.hip) at 1024 x 1024,
3 channels, 10 slices, ks 11, grid 7 and 11, all in one run:
  forward_us            aadff_render_psf_map_blend_stack through the C ABI: conv_blend_kernel<11>
  d_img_us              the backward entry with d_maps = NULL: blend_dimg_kernel<11>
  d_maps_us             the backward entry with d_img = NULL: blend_dmaps_partial_kernel<11> + blend_dmaps_sum_kernel
  bwd_both_us           the backward entry with both gradients
  fwd_bwd_public_us     aadff.diffrender.render_psf_map_blend_stack + backward() of both inputs (autograd, allocations, Python included)
  composed_autograd_us  torch autograd through the composition tools/blend_bench.py times: per-pixel PSFs [1,H,W,ks,ks] interpolated in
                        torch from ONE map of ONE channel, fed to aadff.diffrender.local_psf_render for all three channels, forward +
                        backward to the image and the map - ONE slice at the full size (507 MB per PSF tensor; the graph keeps several)

    python tools/blend_grad_bench.py [--size 1024] [--slices 10] [--ks 11] [--grids 7 11] [--reps 5] [--inner 20]

Each figure is the median over --reps of the mean of --inner back-to-back calls between two stream events (microseconds per call), after
three warm-up calls; inputs stay resident.  FMA counts: every kernel issues the forward's 4 FMAs per tap and output element,
4 ks^2 B C S H W; the fractions are of the 141 TFLOP/s packed fp32 FMA rate profiles/blend_bench.txt uses.  One JSON line per grid."""
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
from aadff import diffrender                                                # noqa: E402
from aadff.blend import blend_nodes                                         # noqa: E402

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
PEAK = 141e12


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
    """[1,H,W,ks,ks]: the per-pixel PSFs of one [g ks, g ks] map, flipped for local_psf_render (which does not flip); differentiable."""
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
dy = torch.randn((1, 3, S, H, W), generator=gen).to(dev)
hp = lambda t: C.c_void_p(t.data_ptr())                                     # noqa: E731
for g in a.grids:
    maps = torch.rand((S, 3, g * ks, g * ks), generator=gen).to(dev) / (ks * ks)
    out, st = torch.empty((1, 3, S, H, W), device=dev), _abi.stream_ptr(dev)
    ny, nx = blend_nodes(H, g), blend_nodes(W, g)
    nbytes = _abi.load_library().aadff_render_psf_map_blend_stack_bwd_workspace(1, 3, S, H, W, g, ks)
    ws = torch.empty((nbytes // 4,), device=dev)
    d_img, d_maps = torch.empty_like(img), torch.empty_like(maps)

    def bwd(gi, gm):
        _abi.call("aadff_render_psf_map_blend_stack_bwd", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(dy), _abi.ptr(gi), _abi.ptr(gm),
                  _abi.ptr(ws) if gm is not None else None, C.c_size_t(nbytes if gm is not None else 0), hp(ny), hp(nx), 1, 3, S, H, W, g, ks, st)

    t_fwd = timed(lambda: _abi.call("aadff_render_psf_map_blend_stack", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(out), hp(ny), hp(nx),
                                    1, 3, S, H, W, g, ks, st), a.inner)
    t_dimg = timed(lambda: bwd(d_img, None), a.inner)
    t_dmaps = timed(lambda: bwd(None, d_maps), a.inner)
    t_both = timed(lambda: bwd(d_img, d_maps), a.inner)

    x, m = img.clone().requires_grad_(), maps.clone().requires_grad_()

    def public():
        x.grad = m.grad = None
        diffrender.render_psf_map_blend_stack(x, m, g).backward(dy)

    t_public = timed(public, a.inner)
    assert torch.equal(x.grad, d_img) and torch.equal(m.grad, d_maps)

    m1 = maps[0, 0].clone().requires_grad_()

    def composed():
        x.grad = m1.grad = None
        diffrender.local_psf_render(x, interpolated(m1, g), kernel_size=ks).backward(dy[:, :, 0])

    t_comp = timed(composed, 2)
    # the two routes give one gradient (d_maps of channel 0 with the other channels' dy set to zero is not what `composed` computes - it
    # sums the three channels under one PSF - so the routes are compared on d_img of channel 0, away from the border)
    one = maps.clone()
    one[0, 1:] = one[0, :1]
    xa = img.clone().requires_grad_()
    diffrender.render_psf_map_blend_stack(xa, one[:1], g).backward(dy[:, :, :1])
    p = ks
    agree = float((xa.grad[0, :, p:-p, p:-p] - x.grad[0, :, p:-p, p:-p]).norm() / x.grad[0, :, p:-p, p:-p].norm())
    x.grad = m1.grad = None
    torch.cuda.empty_cache()

    flop = 2.0 * 4 * ks * ks * 3 * S * H * W
    print(json.dumps({"tool": "blend_grad_bench", "H": H, "W": W, "C": 3, "S": S, "ks": ks, "grid": g, "workspace_MB": round(nbytes / 2 ** 20, 1),
                      "forward_us": round(t_fwd, 1), "d_img_us": round(t_dimg, 1), "d_maps_us": round(t_dmaps, 1), "bwd_both_us": round(t_both, 1),
                      "d_img_over_forward": round(t_dimg / t_fwd, 2), "d_maps_over_forward": round(t_dmaps / t_fwd, 2),
                      "forward_frac_of_packed_fma": round(flop / (t_fwd * 1e-6) / PEAK, 3),
                      "d_img_frac_of_packed_fma": round(flop / (t_dimg * 1e-6) / PEAK, 3),
                      "d_maps_frac_of_packed_fma": round(flop / (t_dmaps * 1e-6) / PEAK, 3),
                      "fwd_bwd_public_us": round(t_public, 1), "composed_autograd_one_slice_us": round(t_comp, 1),
                      "composed_stack_over_public": round(S * t_comp / t_public, 1), "d_img_blend_vs_composed_rel_l2": agree}), flush=True)
