#!/usr/bin/env python3
"""Forward + backward of the differentiable image-space operators (aadff.diffrender, csrc/conv_bwd.hip and csrc/gather.hip) against the reference's
formulation on the same GPU: oracle.conv.render_psf_map / local_psf_render (F.pad + F.conv2d per patch, unfold / fold) on
device tensors with torch.autograd.  Same inputs, warmed up, the two legs alternating, HIP events around >= --seconds of work
per leg and repeat.  Shapes: 1x3x1024^2 grid 11 ks 11 single slice, the same as a 10-slice stack (oracle: the slice loop),
2x3x480x640 ks 11 per-pixel PSFs.

Prints ONE JSON line: per shape the two times (ms per forward + backward, every repeat), their ratio, the forward kernel's time,
each backward kernel's own time (HIP events around back-to-back calls of the C ABI entry with one gradient asked for, outputs and
workspace allocated once: no torch dispatcher, no allocation in the timed region; "d_psf_kernels" of the patch convolution is its
partial pass plus its sum pass), the bytes and FLOPs that kernel must move / do (from the shapes) and the fraction of the bound that applies: the packed fp32 FMA peak
(157.3 TFLOP/s) for the patch convolution's gradients - ~138 MB against 7.6 GFLOP for the 10-slice stack: FMA-bound on paper - and
the HBM peak (8 TB/s) for the per-pixel gather's, whose d_psf writes ks^2 floats per pixel.

    python tools/diffrender_bench.py [--seconds 0.5] [--repeats 2] [--out profiles/diffrender_bench.json]"""
import argparse
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

import ctypes as C                              # noqa: E402

import torch                                    # noqa: E402

import aadff.diffrender as dr                   # noqa: E402
from aadff import _abi                          # noqa: E402
from aadff import ops as _ops                   # noqa: E402,F401
from oracle import conv as oconv                # noqa: E402

DEV = "cuda:0"
FMA_PEAK, HBM_PEAK = 157.3e12, 8.0e12


def timed(fn, seconds, min_iters=3):
    """ms per call: HIP events around batches of calls until `seconds` of device work have been timed."""
    fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    total, n, batch = 0.0, 0, 1
    while total < seconds * 1e3 or n < min_iters:
        e0.record()
        for _ in range(batch):
            fn()
        e1.record()
        e1.synchronize()
        dt = e0.elapsed_time(e1)
        total, n = total + dt, n + batch
        batch = max(1, min(1000, int(batch * 0.2 * seconds * 1e3 / max(dt, 1e-3))))
    return total / n


def fwd_bwd(fn, inputs, dy):
    def run():
        for t in inputs:
            t.grad = None
        fn(*inputs).backward(dy)
    return run


def map_case(S, seconds, repeats):
    B, C_, H, W, grid, ks = 1, 3, 1024, 1024, 11, 11
    g = torch.Generator().manual_seed(1)
    img = torch.rand((B, C_, H, W), generator=g).to(DEV)
    p = torch.rand((S, C_, grid, grid, ks, ks), generator=g)
    maps = (p / p.sum((-1, -2), keepdim=True)).permute(0, 1, 2, 4, 3, 5).reshape(S, C_, grid * ks, grid * ks).contiguous().to(DEV)
    dy = torch.randn((B, C_, S, H, W), generator=g).to(DEV)
    x, m = img.clone().requires_grad_(True), maps.clone().requires_grad_(True)
    new = fwd_bwd(lambda a, b: dr.render_psf_map_stack(a, b, grid), (x, m), dy)
    ref = fwd_bwd(lambda a, b: torch.stack([oconv.render_psf_map(a, b[s], grid) for s in range(S)], dim=2), (x, m), dy)
    t_new, t_ref = [], []
    for _ in range(repeats):                      # alternating legs
        t_ref.append(timed(ref, seconds))
        t_new.append(timed(new, seconds))
    with torch.no_grad():
        t_fwd = timed(lambda: dr.render_psf_map_stack(img, maps, grid), min(seconds, 0.2))
    nb = C.c_size_t(0)
    _abi.call("aadff_render_psf_map_stack_bwd_workspace", B, C_, S, H, W, grid, ks, C.byref(nb))
    ws, d_img, d_psf = torch.empty(nb.value // 4, device=DEV), torch.empty_like(img), torch.empty_like(maps)
    st = _abi.stream_ptr(img.device)

    def bwd(gi, gp):
        return lambda: _abi.call("aadff_render_psf_map_stack_bwd", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(dy), _abi.ptr(gi), _abi.ptr(gp), _abi.ptr(ws),
                                 C.c_size_t(nb.value), B, C_, S, H, W, grid, ks, st)
    t_dimg = timed(bwd(d_img, None), min(seconds, 0.2))
    t_dpsf = timed(bwd(None, d_psf), min(seconds, 0.2))
    px = B * C_ * H * W
    flop = 2.0 * px * S * ks * ks                                   # per gradient: one FMA per (output pixel, slice, tap)
    by_dimg = 4.0 * (px * S + px + maps.numel())                   # read dy and the PSF maps, write d_img
    by_dpsf = 4.0 * (px * S + px + maps.numel())                   # read dy and the image, write d_psf (partials not counted)
    return {"shape": f"{B}x{C_}x{H}x{W} grid {grid} ks {ks} S {S}", "oracle_fwd_bwd_ms": t_ref, "diffrender_fwd_bwd_ms": t_new,
            "speedup": min(t_ref) / max(t_new), "forward_kernel_ms": t_fwd,
            "d_img_kernel": {"ms": t_dimg, "bytes": by_dimg, "flop": flop, "bound": "fp32 FMA", "fraction_of_bound": flop / (t_dimg * 1e-3) / FMA_PEAK},
            "d_psf_kernels": {"ms": t_dpsf, "bytes": by_dpsf, "flop": flop, "bound": "fp32 FMA", "fraction_of_bound": flop / (t_dpsf * 1e-3) / FMA_PEAK}}


def local_case(seconds, repeats):
    B, C_, H, W, ks = 2, 3, 480, 640, 11
    g = torch.Generator().manual_seed(2)
    img = torch.rand((B, C_, H, W), generator=g).to(DEV)
    p = torch.rand((B, H, W, ks, ks), generator=g)
    psf = (p / p.sum((-1, -2), keepdim=True)).to(DEV)
    dy = torch.randn((B, C_, H, W), generator=g).to(DEV)
    x, m = img.clone().requires_grad_(True), psf.clone().requires_grad_(True)
    new = fwd_bwd(lambda a, b: dr.local_psf_render(a, b, kernel_size=ks), (x, m), dy)
    ref = fwd_bwd(lambda a, b: oconv.local_psf_render(a, b, ks), (x, m), dy)
    t_new, t_ref = [], []
    for _ in range(repeats):
        t_ref.append(timed(ref, seconds))
        t_new.append(timed(new, seconds))
    with torch.no_grad():
        t_fwd = timed(lambda: dr.local_psf_render(img, psf, kernel_size=ks), min(seconds, 0.2))
    d_img, d_psf, st = torch.empty_like(img), torch.empty_like(psf), _abi.stream_ptr(img.device)

    def bwd(gi, gp):
        return lambda: _abi.call("aadff_local_psf_render_bwd", _abi.ptr(img), _abi.ptr(psf), _abi.ptr(dy), _abi.ptr(gi), _abi.ptr(gp), B, C_, H, W, ks, st)
    t_dimg = timed(bwd(d_img, None), min(seconds, 0.2))
    t_dpsf = timed(bwd(None, d_psf), min(seconds, 0.2))
    px = B * H * W
    by_dimg = 4.0 * (psf.numel() + 2 * px * C_)                      # read the PSFs and dy, write d_img
    by_dpsf = 4.0 * (psf.numel() + 2 * px * C_)                      # write d_psf, read dy and the image
    flop = 2.0 * px * C_ * ks * ks
    return {"shape": f"{B}x{C_}x{H}x{W} ks {ks} per-pixel PSFs", "oracle_fwd_bwd_ms": t_ref, "diffrender_fwd_bwd_ms": t_new,
            "speedup": min(t_ref) / max(t_new), "forward_kernel_ms": t_fwd,
            "d_img_kernel": {"ms": t_dimg, "bytes": by_dimg, "flop": flop, "bound": "HBM", "fraction_of_bound": by_dimg / (t_dimg * 1e-3) / HBM_PEAK},
            "d_psf_kernel": {"ms": t_dpsf, "bytes": by_dpsf, "flop": flop, "bound": "HBM (the write)", "fraction_of_bound": by_dpsf / (t_dpsf * 1e-3) / HBM_PEAK}}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=0.5)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    res = {"tool": "diffrender_bench", "device": torch.cuda.get_device_name(0), "seconds_per_leg": a.seconds,
           "map_single": map_case(1, a.seconds, a.repeats), "map_stack10": map_case(10, a.seconds, a.repeats),
           "local": local_case(a.seconds, a.repeats)}
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)


if __name__ == "__main__":
    main()
