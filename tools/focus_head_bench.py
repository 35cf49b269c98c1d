#!/usr/bin/env python3
"""The fused depth head (csrc/focus_head.hip: aadff_attention_depth and aadff_attention_depth_bwd) at the reference's own training
configuration (N 2, K 1, C 3, S 8, 480 x 640) and at 1 x 10 slices x 1024^2, against

  (a) the same operation as a float32 torch composition on the same GPU: the oracle of tests/focus_head_common.py (softmax over the
      slices, broadcast products, sums), forward under no_grad and forward + backward through autograd;
  (b) the bytes that must move - forward 4 N H W ((K + Ca) S + Ca + 1): scores and stack once, depth and aif once; backward
      4 N H W ((K + Ca) S + Ca + 1 + (K + Ct) S): scores, stack and the two cotangents once, d_scores and d_stack once - over the kernel
      time, as a share of the 8 TB/s of HBM.

The kernel legs call the C ABI with every buffer allocated once (no allocator, no Python op dispatch inside the timed window: --launches
launches between two device events); the torch legs are timed the same way.  The legs alternate --rounds times; the median round is
reported with the spread.  The results of both are also compared.

Prints ONE JSON line.    python tools/focus_head_bench.py [--launches 100] [--rounds 5] [--out profiles/focus_head_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12
SHAPES = [(2, 1, 3, 8, 480, 640), (1, 1, 3, 10, 1024, 1024)]     # N, K, Ct (= Ca), S, H, W


def bench_shape(shape, a):
    import torch

    import focus_head_common as fc
    from aadff import _abi, ops
    N, K, Ct, S, H, W = shape
    Ca = min(Ct, 3)
    g = torch.Generator().manual_seed(5)
    z = (4.0 * torch.randn(N, K, S, H, W, generator=g)).to(DEV)
    x = torch.rand(N, Ct, S, H, W, generator=g).to(DEV)
    u = (0.3 + 2.7 * torch.rand(N, S, generator=g)).to(DEV)
    gd, ga = torch.randn(N, 1, H, W, generator=g).to(DEV), torch.randn(N, Ca, H, W, generator=g).to(DEV)
    depth, aif = torch.empty_like(gd), torch.empty_like(ga)
    dz, dx, du = torch.empty_like(z), torch.empty_like(x), torch.empty_like(u)
    nws = ops.attention_bwd_workspace_bytes(N, S, H, W)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=DEV)
    st = _abi.stream_ptr(torch.device(DEV))
    dims = (N, K, Ct, Ca, S, H, W, 0, st)

    def k_fwd():
        _abi.call("aadff_attention_depth", _abi.ptr(z), _abi.ptr(x), _abi.ptr(u), _abi.ptr(depth), _abi.ptr(aif), *dims)

    def k_bwd():
        _abi.call("aadff_attention_depth_bwd", _abi.ptr(z), _abi.ptr(x), _abi.ptr(u), _abi.ptr(gd), _abi.ptr(ga), _abi.ptr(dz), _abi.ptr(dx), _abi.ptr(du),
                  _abi.ptr(ws), C.c_size_t(nws), *dims)

    def k_both():
        k_fwd()
        k_bwd()

    def t_fwd():
        with torch.no_grad():
            return fc.head(z, x, u)

    zr, xr, ur = (t.clone().requires_grad_(True) for t in (z, x, u))

    def t_both():
        zr.grad = xr.grad = ur.grad = None
        d, i = fc.head(zr, xr, ur)
        torch.autograd.backward([d, i], [gd, ga])
        return d, i

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n                        # ms per call

    for _ in range(10):
        k_both()
    for _ in range(3):
        ref_d, ref_a = t_both()
    torch.cuda.synchronize()
    rel = lambda p, q: float((p.detach().double() - q.detach().double()).norm() / q.detach().double().norm())      # noqa: E731
    agree = {"depth": rel(depth, ref_d), "aif": rel(aif, ref_a), "d_scores": rel(dz, zr.grad), "d_stack": rel(dx, xr.grad), "d_foc_dists": rel(du, ur.grad)}
    legs = {"kernel_fwd": (k_fwd, a.launches), "torch_fwd": (t_fwd, a.torch_launches), "kernel_bwd": (k_bwd, a.launches),
            "kernel_fwd_bwd": (k_both, a.launches), "torch_fwd_bwd": (t_both, a.torch_launches)}
    times = {k: [] for k in legs}
    for _ in range(a.rounds):                                 # alternate the legs
        for k, (fn, n) in legs.items():
            times[k].append(timed(fn, n))
    med = {k: statistics.median(v) for k, v in times.items()}
    px = 4 * N * H * W
    b_fwd, b_bwd = px * ((K + Ca) * S + Ca + 1), px * ((K + Ca) * S + Ca + 1 + (K + Ct) * S)
    tbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12      # noqa: E731
    out = {"shape": list(shape), "ms": {k: round(v, 5) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
           "speedup_fwd": round(med["torch_fwd"] / med["kernel_fwd"], 2), "speedup_fwd_bwd": round(med["torch_fwd_bwd"] / med["kernel_fwd_bwd"], 2),
           "bytes_that_must_move": {"fwd": b_fwd, "bwd": b_bwd},
           "achieved_TB_per_s": {"fwd": round(tbs(b_fwd, med["kernel_fwd"]), 3), "bwd": round(tbs(b_bwd, med["kernel_bwd"]), 3),
                                 "fwd_bwd": round(tbs(b_fwd + b_bwd, med["kernel_fwd_bwd"]), 3)},
           "relative_L2_vs_composition": {k: float(f"{v:.3e}") for k, v in agree.items()}}
    out["share_of_8TBps_byte_roofline"] = {k: round(v * 1e12 / HBM_BYTES_PER_S, 3) for k, v in out["achieved_TB_per_s"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--torch-launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from aadff import _abi
    _abi.require_gpu()
    res = {"tool": "focus_head_bench", "device": torch.cuda.get_device_name(0), "launches_per_round": a.launches, "torch_launches_per_round": a.torch_launches,
           "rounds": a.rounds, "normalize_attention": False, "shapes": [bench_shape(s, a) for s in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
