#!/usr/bin/env python3
"""Forward + backward of the differentiable thin-lens renderer (aadff.diffrender.thinlens_render_stack, csrc/thinlens.hip) against
the reference's tensor form under torch autograd on the same GPU (lens.coc -> [N,H,W,ks,ks] Gaussian PSFs -> the HIP gather with its
HIP backward, aadff.diffrender._thinlens_tensor_form), at 2x3x480x640 x 8 slices and at 1x3x1024^2 x 10, ks 11.  Gradients to the
image, the depth map and the focus distances in both legs.  The tensor leg runs one slice at a time (forward + backward per slice,
gradients accumulated), as the reference's slice loop does.

Every leg of every shape is a child process of its own under its own time limit (a leg that hangs or fails is reported as such and
does not stop the others).  A leg warms up, then times with HIP events until --seconds of device work have passed, --repeats times;
it also reports the peak of torch's allocator above what was allocated before the call (inputs, cotangent).  The fused leg
additionally times the kernels alone through the C ABI (outputs and workspace allocated once): the stack forward against S launches
of the per-slice forward kernel, the input-gradient kernel with its sum pass (d_depth + d_foc), and the pre-pass + d_img kernel.

Prints ONE JSON line.    python tools/thinlens_grad_bench.py [--seconds 1.0] [--repeats 2] [--out profiles/thinlens_grad_bench.json]"""
import argparse
import json
import os
import subprocess
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

SHAPES = {"2x3x480x640_S8": (2, 3, 8, 480, 640), "1x3x1024x1024_S10": (1, 3, 10, 1024, 1024)}
DEV = "cuda:0"
KS = 11


def timed(fn, seconds, min_iters=2):
    import torch
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


def leg(shape, mode, seconds, repeats):
    import ctypes as C

    import numpy as np
    import torch

    import aadff.diffrender as dr
    from aadff import _abi, ops
    from aadff.synth import synth_depth_mm, synth_rgb
    from deeplens.psfnet import ThinLens
    N, Cn, S, H, W = SHAPES[shape]
    lens = ThinLens(foc_len=50.0, fnum=2.8, kernel_size=KS, sensor_size=[24.0, 24.0 * W / H], sensor_res=(H, W))
    img = torch.stack([torch.from_numpy(synth_rgb(H, W, seed=11 + n)) for n in range(N)]).to(DEV)
    depth = torch.stack([-torch.from_numpy(synth_depth_mm(H, W, seed=12 + n))[None] for n in range(N)]).to(DEV)
    fds = torch.tensor(np.linspace(-500.0, -5000.0, S, dtype=np.float32)).repeat(N, 1).to(DEV)
    dy = torch.randn((N, Cn, S, H, W), generator=torch.Generator().manual_seed(31)).to(DEV)
    x, d, f = img.clone().requires_grad_(True), depth.clone().requires_grad_(True), fds.clone().requires_grad_(True)

    def run_fused():
        x.grad = d.grad = f.grad = None
        dr.thinlens_render_stack(lens, x, d, f).backward(dy)

    def run_tensor():
        x.grad = d.grad = f.grad = None
        for s in range(S):
            dr._thinlens_tensor_form(lens, x, d, f[:, s]).backward(dy[:, :, s])

    run = run_tensor if mode == "tensor" else run_fused
    run()
    torch.cuda.synchronize()
    base = torch.cuda.memory_allocated()
    torch.cuda.reset_peak_memory_stats()
    run()
    torch.cuda.synchronize()
    peak_extra = torch.cuda.max_memory_allocated() - base
    res = {"shape": shape, "mode": mode, "fwd_bwd_ms": [timed(run, seconds) for _ in range(repeats)], "peak_extra_bytes": int(peak_extra)}
    if mode == "fused":
        rows = N * S * H * W
        nb = ops.thinlens_bwd_workspace_bytes(N, Cn, S, H, W, KS, True, True)
        res["expected_extra_bytes"] = {"output": 4 * Cn * rows, "workspace": nb}
        out = torch.empty((N, Cn, S, H, W), device=DEV)
        out1 = torch.empty((N, Cn, H, W), device=DEV)
        ws = torch.empty(nb // 4, device=DEV)
        g_img, g_dep, g_foc = torch.empty_like(img), torch.empty_like(depth), torch.empty_like(fds)
        neg = (depth < 0).any().to(torch.int32).reshape(1)
        cols = [fds[:, s].contiguous() for s in range(S)]
        consts = (C.c_float(lens.foc_len / lens.fnum), C.c_float(lens.foc_len), C.c_float(1.0 / lens.ps), C.c_float(lens.d_min), C.c_float(lens.d_max))
        st = _abi.stream_ptr(torch.device(DEV))

        def fwd_stack():
            _abi.call("aadff_thinlens_render_stack", _abi.ptr(img), _abi.ptr(depth), _abi.ptr(fds), _abi.ptr(neg), _abi.ptr(out), N, Cn, S, H, W, KS, *consts, st)

        def fwd_loop():
            for s in range(S):
                _abi.call("aadff_thinlens_render", _abi.ptr(img), _abi.ptr(depth), _abi.ptr(cols[s]), _abi.ptr(neg), _abi.ptr(out1), N, Cn, H, W, KS, *consts, st)

        def bwd(gi, gd, gf):
            return lambda: _abi.call("aadff_thinlens_render_stack_bwd", _abi.ptr(img), _abi.ptr(depth), _abi.ptr(fds), _abi.ptr(neg), _abi.ptr(dy),
                                     _abi.ptr(gi), _abi.ptr(gd), _abi.ptr(gf), _abi.ptr(ws), C.c_size_t(nb), N, Cn, S, H, W, KS, *consts, st)
        res["stack_forward_kernel_ms"] = timed(fwd_stack, min(seconds, 0.5))
        res["per_slice_forward_kernels_ms"] = timed(fwd_loop, min(seconds, 0.5))
        res["input_grad_kernels_ms"] = timed(bwd(None, g_dep, g_foc), min(seconds, 0.5))
        res["d_img_kernels_ms"] = timed(bwd(g_img, None, None), min(seconds, 0.5))
        res["stack_forward_speedup_over_slice_loop"] = res["per_slice_forward_kernels_ms"] / res["stack_forward_kernel_ms"]
    print("LEG " + json.dumps(res), flush=True)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seconds", type=float, default=1.0)
    ap.add_argument("--repeats", type=int, default=2)
    ap.add_argument("--leg-timeout", type=float, default=240.0, help="time limit of one child process (one leg of one shape), seconds")
    ap.add_argument("--out", default=None)
    ap.add_argument("--leg", nargs=2, metavar=("SHAPE", "MODE"), help="internal: run one leg in this process")
    a = ap.parse_args()
    if a.leg:
        return leg(a.leg[0], a.leg[1], a.seconds, a.repeats)
    res = {"tool": "thinlens_grad_bench", "seconds_per_leg": a.seconds, "shapes": {}}
    for shape in SHAPES:
        entry = {}
        for mode in ("fused", "tensor"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", shape, mode, "--seconds", str(a.seconds), "--repeats", str(a.repeats)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.leg_timeout, text=True)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
                entry[mode] = json.loads(lines[-1][4:]) if p.returncode == 0 and lines else {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            except subprocess.TimeoutExpired:
                entry[mode] = {"error": f"no result within {a.leg_timeout:.0f} s"}
            if "error" in entry[mode]:
                break                                 # a leg that failed or hung: start nothing more on this GPU for this shape
        if all("fwd_bwd_ms" in entry.get(m, {}) for m in ("fused", "tensor")):
            entry["speedup_over_tensor_form"] = min(entry["tensor"]["fwd_bwd_ms"]) / max(entry["fused"]["fwd_bwd_ms"])
            entry["memory_ratio_tensor_form_over_fused"] = entry["tensor"]["peak_extra_bytes"] / max(1, entry["fused"]["peak_extra_bytes"])
        res["shapes"][shape] = entry
        if any("error" in v for v in entry.values() if isinstance(v, dict)):
            break
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if all("speedup_over_tensor_form" in e for e in res["shapes"].values()) and len(res["shapes"]) == len(SHAPES) else 1


if __name__ == "__main__":
    sys.exit(main())
