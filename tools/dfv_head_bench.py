#!/usr/bin/env python3
"""The fused cost-volume depth head (csrc/dfv_head.hip: aadff_dfv_head_fwd and aadff_dfv_head_bwd) at the size of the reference's
training configuration (B 2, S 10, 480 x 640) from costs at 1/4 (120 x 160) and 1/8 (60 x 80) of the image, against

  (a) the same operation as a float32 torch composition on the same GPU: the oracle of tests/dfv_head_common.py (F.interpolate
      bilinear, softmax over the slices, broadcast products, sums), forward under no_grad and forward + backward through autograd;
  (b) the bytes that must move - forward 4 (B S h w + 2 B H W): the cost once, pred and std once; backward 4 (2 B S h w + B H W): the
      cost and g_pred once, d_cost once - over the kernel time, as a share of the 8 TB/s of HBM.  The kernels are far from that bound
      by construction: per output pixel they evaluate S interpolations from four cached cells and S exponentials (three times
      over beyond 16 slices, where the terms no longer stay in registers).

The kernel legs call the C ABI with every buffer allocated once (no allocator, no Python op dispatch inside the timed window: --launches
launches between two device events, 0.09 s for the shortest leg at the default); the torch legs are timed the same way.  The legs alternate --rounds times; the median round is
reported with the spread.  The results of both are also compared, and the backward is run twice and compared bit for bit.

Prints ONE JSON line.    python tools/dfv_head_bench.py [--launches 5000] [--rounds 5] [--out profiles/dfv_head_bench.json]"""
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
SHAPES = [(2, 10, 120, 160, 480, 640), (2, 10, 60, 80, 480, 640)]     # B, S, h, w, H, W


def bench_shape(shape, a):
    import torch

    import dfv_head_common as dc
    from aadff import _abi, ops
    B, S, h, w, H, W = shape
    g = torch.Generator().manual_seed(5)
    c = (2.0 * torch.randn(B, S, h, w, generator=g)).to(DEV)
    u = (0.3 + 2.7 * torch.rand(B, S, generator=g)).to(DEV)
    gp = torch.randn(B, 1, H, W, generator=g).to(DEV)
    pred, std = torch.empty_like(gp), torch.empty_like(gp)
    dcost, du = torch.empty_like(c), torch.empty_like(u)
    nws = ops.dfv_bwd_workspace_bytes(B, S, h, w, H, W)
    ws = torch.empty(nws // 4, dtype=torch.float32, device=DEV)
    st = _abi.stream_ptr(torch.device(DEV))
    dims = (B, S, h, w, H, W, st)

    def k_fwd():
        _abi.call("aadff_dfv_head_fwd", _abi.ptr(c), _abi.ptr(u), _abi.ptr(pred), _abi.ptr(std), None, *dims)

    def k_bwd():
        _abi.call("aadff_dfv_head_bwd", _abi.ptr(c), _abi.ptr(u), _abi.ptr(gp), _abi.ptr(dcost), _abi.ptr(du), _abi.ptr(ws), C.c_size_t(nws), *dims)

    def k_both():
        k_fwd()
        k_bwd()

    def t_fwd():
        with torch.no_grad():
            return dc.head(c, u, (H, W))

    cr, ur = (t.clone().requires_grad_(True) for t in (c, u))

    def t_both():
        cr.grad = ur.grad = None
        p, s, _ = dc.head(cr, ur, (H, W))
        p.backward(gp)
        return p, s

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
    torch.cuda.synchronize()
    first = (dcost.clone(), du.clone())
    k_bwd()
    torch.cuda.synchronize()
    repeat = torch.equal(first[0], dcost) and torch.equal(first[1], du)
    for _ in range(3):
        ref_p, ref_s = t_both()
    torch.cuda.synchronize()
    rel = lambda p, q: float((p.detach().double() - q.detach().double()).norm() / q.detach().double().norm())      # noqa: E731
    agree = {"pred": rel(pred, ref_p), "std": rel(std, ref_s), "d_cost": rel(dcost, cr.grad), "d_foc_dists": rel(du, ur.grad)}
    legs = {"kernel_fwd": (k_fwd, a.launches), "torch_fwd": (t_fwd, a.torch_launches), "kernel_bwd": (k_bwd, a.launches),
            "kernel_fwd_bwd": (k_both, a.launches), "torch_fwd_bwd": (t_both, a.torch_launches)}
    times = {k: [] for k in legs}
    for _ in range(a.rounds):                                 # alternate the legs
        for k, (fn, n) in legs.items():
            times[k].append(timed(fn, n))
    med = {k: statistics.median(v) for k, v in times.items()}
    b_fwd, b_bwd = 4 * (B * S * h * w + 2 * B * H * W), 4 * (2 * B * S * h * w + B * H * W)
    tbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12      # noqa: E731
    out = {"shape": list(shape), "ms": {k: round(v, 5) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
           "speedup_fwd": round(med["torch_fwd"] / med["kernel_fwd"], 2), "speedup_fwd_bwd": round(med["torch_fwd_bwd"] / med["kernel_fwd_bwd"], 2),
           "bytes_that_must_move": {"fwd": b_fwd, "bwd": b_bwd}, "bwd_workspace_bytes": nws, "bwd_repeats_bit_for_bit": repeat,
           "achieved_TB_per_s": {"fwd": round(tbs(b_fwd, med["kernel_fwd"]), 4), "bwd": round(tbs(b_bwd, med["kernel_bwd"]), 4),
                                 "fwd_bwd": round(tbs(b_fwd + b_bwd, med["kernel_fwd_bwd"]), 4)},
           "relative_L2_vs_composition": {k: float(f"{v:.3e}") for k, v in agree.items()}}
    out["share_of_8TBps_byte_roofline"] = {k: round(v * 1e12 / HBM_BYTES_PER_S, 4) for k, v in out["achieved_TB_per_s"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=5000)
    ap.add_argument("--torch-launches", type=int, default=500)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from aadff import _abi
    _abi.require_gpu()
    res = {"tool": "dfv_head_bench", "device": torch.cuda.get_device_name(0), "launches_per_round": a.launches, "torch_launches_per_round": a.torch_launches,
           "rounds": a.rounds, "shapes": [bench_shape(s, a) for s in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
