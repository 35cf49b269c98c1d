#!/usr/bin/env python3
"""Time the backward of the occlusion-aware layered PSF-map render (aadff_render_psf_map_stack_occluded_bwd, csrc/conv_occl_bwd.hip) at
1024 x 1024, 3 channels, 10 slices, ks 11, grid 7, L = 1, 4, 8, on the two scenes of tools/occlusion_bench.py (disc: most tiles hold one
or two layers; random: every tile holds all L layers), and write profiles/occlusion_grad_bench.txt.

    python tools/occlusion_grad_bench.py [--size 1024] [--slices 10] [--ks 11] [--grid 7] [--layers 1 4 8] [--reps 5] [--inner 20]
                                         [--out profiles/occlusion_grad_bench.txt]

Through the C ABI, median over --reps of the mean of --inner back-to-back calls between two stream events (microseconds per call), after
warm-up calls, inputs and a full (one-pass) workspace resident: the forward; the backward for d_img alone (stages 1 + 2), for d_maps
alone (stages 1 + 3) and for both (1 + 2 + 3).  The entry does not expose its stages, so the three stage times are the differences
    layers = img_only + maps_only - both,    dimg = both - maps_only,    dmaps = both - img_only.
Then forward + backward through aadff.diffrender.render_psf_map_occluded_stack (loss = sum(out * g)), and in the same run the only
alternative a user has without the fused backward: torch autograd through 2 L calls of aadff.diffrender.render_psf_map_stack on the
masked image and the masks plus the composite in torch (--alt-reps x --alt-inner calls), with its peak memory beside the workspace size
of the fused entry.  The two are also compared: the rel-L2 of the alternative's gradients to the fused ones.  One JSON line per (L, scene)."""
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
from aadff.focal_stack import depth_layers                                  # noqa: E402
from aadff.synth import synth_disc_depth_mm                                 # noqa: E402

ap = argparse.ArgumentParser()
ap.add_argument("--size", type=int, default=1024)
ap.add_argument("--slices", type=int, default=10)
ap.add_argument("--ks", type=int, default=11)
ap.add_argument("--grid", type=int, default=7)
ap.add_argument("--layers", type=int, nargs="+", default=[1, 4, 8])
ap.add_argument("--reps", type=int, default=5)
ap.add_argument("--inner", type=int, default=20)
ap.add_argument("--alt-reps", type=int, default=3)
ap.add_argument("--alt-inner", type=int, default=2)
ap.add_argument("--out", default=os.path.join(REPO, "profiles", "occlusion_grad_bench.txt"))
a = ap.parse_args()
dev = torch.device("cuda:0")
H = W = a.size
S, ks, Cn, grid = a.slices, a.ks, 3, a.grid


def timed(f, reps, inner, warm=2):
    for _ in range(warm):
        f()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    ts = []
    for _ in range(reps):
        e0.record()
        for _ in range(inner):
            f()
        e1.record()
        torch.cuda.synchronize()
        ts.append(e0.elapsed_time(e1) / inner * 1e3)
    return float(np.median(ts))


def composite_alternative(x, m, lay, L):
    """The occluded stack from 2 L differentiable patch renders on masked inputs and a torch composite: [1,C,S,H,W]."""
    T = V = A = None
    for l in range(L):
        on = (lay == l)[:, None]
        q = diffrender.render_psf_map_stack(torch.where(on, x, 0.0), m[l::L], grid)
        c = diffrender.render_psf_map_stack(on.expand_as(x).float(), m[l::L], grid)
        if T is None:
            V, A, T = q, c, torch.clamp(1.0 - c, min=0.0)
        else:
            V, A, T = V + T * q, A + T * c, T * torch.clamp(1.0 - c, min=0.0)
    return torch.where(A > 0, V / torch.where(A > 0, A, 1.0), 0.0)


def rel(x, y):
    return float((x.double() - y.double()).norm() / y.double().norm())


gen = torch.Generator().manual_seed(0)
img = torch.rand((1, Cn, H, W), generator=gen).to(dev)
g = torch.randn((1, Cn, S, H, W), generator=gen).to(dev)
depth = torch.from_numpy(synth_disc_depth_mm(H, W)[0])[None].to(dev)
out, st = torch.empty((1, Cn, S, H, W), device=dev), _abi.stream_ptr(dev)
d_img = torch.empty_like(img)
lines = ["# tools/occlusion_grad_bench.py: microseconds per call, median of %d x %d back-to-back calls through the C ABI; the stage times are" % (a.reps, a.inner),
         "# differences of the entry's three forms (see the tool's docstring); alt_*: torch autograd through 2 L patch renders + a torch composite"]
query = _abi.load_library().aadff_render_psf_map_stack_occluded_bwd_workspace
for L in a.layers:
    w = torch.rand((S * L, Cn, grid, ks, grid, ks), generator=gen) + 0.05
    maps = (w / w.sum((3, 5), keepdim=True)).reshape(S * L, Cn, grid * ks, grid * ks).to(dev).contiguous()
    d_maps = torch.empty_like(maps)
    nbytes = query(1, Cn, S, L, H, W, grid, ks, 1)
    ws = torch.empty((nbytes // 4,), device=dev)
    scenes = {"disc": depth_layers(depth, L)[0].reshape(1, H, W).to(torch.uint8).contiguous(),
              "random": torch.randint(0, L, (1, H, W), generator=gen).to(torch.uint8).to(dev)}
    for name, lay in scenes.items():
        def fwd():
            _abi.call("aadff_render_psf_map_stack_occluded", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(lay), _abi.ptr(out), None, 1, Cn, S, L, H, W,
                      grid, ks, 1, st)

        def bwd(gi, gm):
            _abi.call("aadff_render_psf_map_stack_occluded_bwd", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(lay), _abi.ptr(g), None, _abi.ptr(gi),
                      _abi.ptr(gm), _abi.ptr(ws), C.c_size_t(nbytes), 1, Cn, S, L, H, W, grid, ks, 1, st)

        t_fwd = timed(fwd, a.reps, a.inner)
        t_img = timed(lambda: bwd(d_img, None), a.reps, a.inner)
        t_maps = timed(lambda: bwd(None, d_maps), a.reps, a.inner)
        t_both = timed(lambda: bwd(d_img, d_maps), a.reps, a.inner)
        fused_i, fused_m = d_img.clone(), d_maps.clone()

        x, m = img.clone().requires_grad_(), maps.clone().requires_grad_()

        def step():
            x.grad = m.grad = None
            (diffrender.render_psf_map_occluded_stack(x, m, lay, L, grid) * g).sum().backward()

        t_step = timed(step, a.reps, a.inner)
        assert torch.equal(x.grad, fused_i) and torch.equal(m.grad, fused_m)
        torch.cuda.synchronize()
        torch.cuda.reset_peak_memory_stats()
        base = torch.cuda.memory_allocated()

        def alt():
            x.grad = m.grad = None
            (composite_alternative(x, m, lay, L) * g).sum().backward()

        t_alt = timed(alt, a.alt_reps, a.alt_inner, warm=1)
        peak = torch.cuda.max_memory_allocated() - base
        rec = {"tool": "occlusion_grad_bench", "H": H, "W": W, "C": Cn, "S": S, "ks": ks, "grid": grid, "L": L, "scene": name,
               "forward_us": round(t_fwd, 1), "bwd_img_only_us": round(t_img, 1), "bwd_maps_only_us": round(t_maps, 1),
               "bwd_both_us": round(t_both, 1), "stage_layers_us": round(t_img + t_maps - t_both, 1), "stage_dimg_us": round(t_both - t_maps, 1),
               "stage_dmaps_us": round(t_both - t_img, 1), "diffrender_fwd_bwd_us": round(t_step, 1), "alt_fwd_bwd_us": round(t_alt, 1),
               "alt_over_fused": round(t_alt / t_step, 2), "workspace_mb": round(nbytes / 2 ** 20, 1), "alt_peak_mb": round(peak / 2 ** 20, 1),
               "alt_d_img_rel_l2": float("%.2e" % rel(x.grad, fused_i)), "alt_d_maps_rel_l2": float("%.2e" % rel(m.grad, fused_m))}
        lines.append(json.dumps(rec))
        print(lines[-1], flush=True)
        del x, m
    del ws
os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
with open(a.out, "w") as f:
    f.write("\n".join(lines) + "\n")
