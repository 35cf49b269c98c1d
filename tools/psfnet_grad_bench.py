#!/usr/bin/env python3
"""Forward + backward of the differentiable PSF-network renderer (aadff.diffrender.psfnet_render_stack, csrc/psfnet_bwd.hip)
against `mlp_precision="torch"` (lens.psfnet under torch autograd + the HIP gather) on the same GPU, at configuration 5's
2x3x480x640 x 8 slices and at 1x3x1024^2 x 10.  Gradients to the image, the depth map and the focus distances in both legs.  The
torch leg runs one slice at a time (forward + backward per slice, gradients accumulated): a whole stack of its activations is
2.9 GB per (image, slice) at 480x640.

Every leg of every shape is a child process of its own under its own time limit (a leg that hangs or fails is reported as such and
does not stop the others).  A leg warms up, then times with HIP events until --seconds of device work have passed, --repeats times;
it also reports the peak of torch's allocator above what was allocated before the call (inputs, weights, cotangent).  The fused leg
additionally times the kernels alone through the C ABI (outputs and workspace allocated once): the forward kernel, the input-gradient
kernel with its two sum passes (d_depth + d_foc_z), and the d_img composition.

Prints ONE JSON line.    python tools/psfnet_grad_bench.py [--seconds 1.0] [--repeats 2] [--out profiles/psfnet_grad_bench.json]"""
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

SHAPES = {"cfg5_2x3x480x640_S8": (2, 3, 8, 480, 640), "1x3x1024x1024_S10": (1, 3, 10, 1024, 1024)}
DEV = "cuda:0"


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
    from aadff import _abi, ops, psfnet_pack
    from aadff.synth import mlp_state_dict, synth_depth_mm, synth_rgb
    from deeplens.psfnet import PSFNet
    N, Cn, S, H, W = SHAPES[shape]
    lens = PSFNet(os.path.join(REPO, "lenses", "rf50mm", "lens.json"), sensor_res=(H, W), kernel_size=11, device=DEV)
    lens.psfnet.load_state_dict({k: torch.from_numpy(v) for k, v in mlp_state_dict(seed=4321).items()})
    lens.mlp_precision = "torch" if mode == "torch" else "fp32"
    for p in lens.psfnet.parameters():
        p.requires_grad_(False)                   # both legs: gradients of the inputs only
    img = torch.stack([torch.from_numpy(synth_rgb(H, W, seed=11 + n)) for n in range(N)]).to(DEV)
    depth = torch.stack([-torch.from_numpy(synth_depth_mm(H, W, seed=12 + n))[None] for n in range(N)]).to(DEV)
    fds = torch.tensor(np.linspace(-500.0, -5000.0, S, dtype=np.float32)).repeat(N, 1).to(DEV)
    dy = torch.randn((N, Cn, S, H, W), generator=torch.Generator().manual_seed(31)).to(DEV)
    x, d, f = img.clone().requires_grad_(True), depth.clone().requires_grad_(True), fds.clone().requires_grad_(True)

    def run_fused():
        x.grad = d.grad = f.grad = None
        dr.psfnet_render_stack(lens, x, d, f).backward(dy)

    def run_torch():
        x.grad = d.grad = f.grad = None
        for s in range(S):
            dr.psfnet_render_stack(lens, x, d, f[:, s:s + 1]).backward(dy[:, :, s:s + 1])

    run = run_torch if mode == "torch" else run_fused
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
        res["expected_extra_bytes"] = {"output": 4 * Cn * rows, "workspace_rows": ops.psfnet_bwd_workspace_bytes(N, S, Cn, H, W, 11, True, False),
                                       "workspace_one_slice_of_psfs": ops.psfnet_bwd_workspace_bytes(N, S, Cn, H, W, 11, False, True)}
        packed = lens._fused(torch.device(DEV))
        wt, wt_exp = psfnet_pack.transposed(packed, lens.psfnet)
        xs, ys = lens._field_axes(H, W, torch.device(DEV))
        fz = lens.depth2z(fds).contiguous()
        inv_range = float(np.float32(1.0) / np.float32(lens.d_max - lens.d_min))
        dep = depth.reshape(N, H, W).contiguous()
        out = torch.empty((N, Cn, S, H, W), device=DEV)
        nb = ops.psfnet_bwd_workspace_bytes(N, S, Cn, H, W, 11, True, True)
        ws = torch.empty(nb // 4, device=DEV)
        g_img, g_dep, g_foc = torch.empty_like(img), torch.empty_like(dep), torch.empty_like(fz)
        st = _abi.stream_ptr(torch.device(DEV))
        ints = lambda v: (C.c_int * len(v))(*v)          # noqa: E731

        def fwd():
            _abi.call("aadff_psfnet_render_rgbd", _abi.ptr(dep), _abi.ptr(xs), _abi.ptr(ys), _abi.ptr(fz), C.c_float(lens.d_min), C.c_float(inv_range), N, S,
                      _abi.ptr(packed.wpack), _abi.ptr(packed.bias), packed.n, packed.ins, packed.outs, _abi.ptr(img), _abi.ptr(out), Cn, H, W, 11, 0,
                      _abi.ptr(packed.flags), st)

        def bwd(gi, gd, gf):
            return lambda: _abi.call("aadff_psfnet_render_rgbd_bwd", _abi.ptr(dep), _abi.ptr(xs), _abi.ptr(ys), _abi.ptr(fz), C.c_float(lens.d_min),
                                     C.c_float(inv_range), N, S, _abi.ptr(packed.wpack), _abi.ptr(packed.bias), _abi.ptr(wt), ints(wt_exp), packed.n,
                                     packed.ins, packed.outs, _abi.ptr(img), _abi.ptr(dy), Cn, H, W, 11, _abi.ptr(gi), _abi.ptr(gd), _abi.ptr(gf),
                                     _abi.ptr(ws), C.c_size_t(nb), st)
        res["forward_kernel_ms"] = timed(fwd, min(seconds, 0.5))
        res["input_grad_kernels_ms"] = timed(bwd(None, g_dep, g_foc), min(seconds, 0.5))
        res["d_img_composition_ms"] = timed(bwd(g_img, None, None), min(seconds, 0.5))
        res["input_grad_over_forward"] = res["input_grad_kernels_ms"] / res["forward_kernel_ms"]
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
    res = {"tool": "psfnet_grad_bench", "seconds_per_leg": a.seconds, "shapes": {}}
    for shape in SHAPES:
        entry = {}
        for mode in ("fused", "torch"):
            cmd = [sys.executable, os.path.abspath(__file__), "--leg", shape, mode, "--seconds", str(a.seconds), "--repeats", str(a.repeats)]
            try:
                p = subprocess.run(cmd, stdout=subprocess.PIPE, stderr=subprocess.PIPE, timeout=a.leg_timeout, text=True)
                lines = [ln for ln in p.stdout.splitlines() if ln.startswith("LEG ")]
                entry[mode] = json.loads(lines[-1][4:]) if p.returncode == 0 and lines else {"error": f"exit status {p.returncode}", "stderr": p.stderr[-2000:]}
            except subprocess.TimeoutExpired:
                entry[mode] = {"error": f"no result within {a.leg_timeout:.0f} s"}
            if "error" in entry[mode]:
                break                                 # a leg that failed or hung: start nothing more on this GPU for this shape
        if all("fwd_bwd_ms" in entry.get(m, {}) for m in ("fused", "torch")):
            entry["speedup_over_torch"] = min(entry["torch"]["fwd_bwd_ms"]) / max(entry["fused"]["fwd_bwd_ms"])
            entry["memory_ratio_torch_over_fused"] = entry["torch"]["peak_extra_bytes"] / max(1, entry["fused"]["peak_extra_bytes"])
        res["shapes"][shape] = entry
        if any("error" in v for v in entry.values() if isinstance(v, dict)):
            break
    line = json.dumps(res)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")
    print(line)
    return 0 if all("speedup_over_torch" in e for e in res["shapes"].values()) and len(res["shapes"]) == len(SHAPES) else 1


if __name__ == "__main__":
    sys.exit(main())
