#!/usr/bin/env python3
"""The ray-traced render (csrc/render_rt.hip, aadff_render_raytraced) at 1024 x 1024, spp 64, B = 1 and B = 4: ms per render and
ray-surface steps per second (3 channels x H x W x spp rays x the lens's surfaces, every ray counted as if it lived to the object
plane - the figure the PSF-grid kernel's ~590 G steps/s is quoted in).

The timed window holds C ABI calls only (outputs allocated once, the in-kernel generator: no uniforms are read), --launches of them
between two device events, --rounds times; the median round is reported with the spread.

Prints ONE JSON line.    python tools/raytrace_bench.py [--lens rf50mm] [--size 1024 1024] [--spp 64] [--launches 10] [--rounds 5]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--lens", default="rf50mm")
    ap.add_argument("--size", type=int, nargs=2, default=(1024, 1024))
    ap.add_argument("--spp", type=int, default=64)
    ap.add_argument("--depth", type=float, default=-2000.0)
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from aadff import _abi
    from aadff.synth import synth_rgb
    from deeplens.basics import WAVE_RGB
    from deeplens.optics import Lensgroup
    _abi.require_gpu()
    H, W = a.size
    lens = Lensgroup(os.path.join(REPO, "lenses", a.lens, "lens.json"), sensor_res=(H, W), device=DEV)
    scale = float(lens.calc_scale_pinhole(a.depth))
    pz, pr = lens.exit_pupil()
    n_surf = len(lens.surfaces)
    base = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(DEV)
    st = _abi.stream_ptr(torch.device(DEV))
    res = {"tool": "raytrace_bench", "device": torch.cuda.get_device_name(0), "lens": a.lens, "n_surf": n_surf, "size": [H, W], "spp": a.spp,
           "depth": a.depth, "launches_per_round": a.launches, "rounds": a.rounds}
    for B in (1, 4):
        img = base.repeat(B, 1, 1, 1).contiguous()
        out = torch.empty_like(img)
        count = torch.empty((3, H, W), dtype=torch.float32, device=DEV)
        args = (_abi.ptr(img), B, H, W, None, C.c_ulonglong(7), a.spp, _abi.ptr(lens._table(WAVE_RGB)), n_surf, float(pz), float(pr),
                float(lens.sensor_size[1]), float(lens.sensor_size[0]), float(lens.pixel_size), a.depth, scale, 0, _abi.ptr(lens._state_device()),
                _abi.ptr(out), _abi.ptr(count), None, _abi.ptr(lens._flags_device()), st)

        def kernel():
            _abi.call("aadff_render_raytraced", *args)

        def timed(n):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            for _ in range(n):
                kernel()
            e1.record()
            e1.synchronize()
            return e0.elapsed_time(e1) / n

        for _ in range(3):
            kernel()
        torch.cuda.synchronize()
        ms = [timed(a.launches) for _ in range(a.rounds)]
        med = statistics.median(ms)
        steps = 3.0 * H * W * a.spp * n_surf
        res[f"B{B}"] = {"ms": round(med, 4), "ms_min_max": [round(min(ms), 4), round(max(ms), 4)],
                        "ray_surface_steps_per_s_G": round(steps / (med * 1e-3) / 1e9, 1), "rays_per_s_G": round(steps / n_surf / (med * 1e-3) / 1e9, 2),
                        "valid_share": round(float(count.mean()) / a.spp, 4), "finite": bool(torch.isfinite(out).all())}
    lens.check_flags()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
