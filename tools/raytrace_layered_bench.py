#!/usr/bin/env python3
"""The layered ray-traced render (csrc/render_rt.hip, aadff_render_raytraced_layered) at 1024 x 1024, spp 64, for L = 1, 4, 8 planes
and B = 1, 4 images per launch, against the plane render (aadff_render_raytraced) timed IN THE SAME RUN at the same size: ms per
render and the ratio layered / plane for the same B.  The scene is examples/raytraced_rgbd_vs_layered_psf.py's - a disc at -600 mm
over a background slanting from -1500 to -3000 mm - quantised by depth_layers into L planes; the plane render sees the same image at
-2000 mm.

The timed window holds C ABI calls only (outputs allocated once, the in-kernel generator: no uniforms are read), --launches of them
between two device events, --rounds times; the median round is reported with the spread (tools/raytrace_bench.py's convention).

Prints ONE JSON line.    python tools/raytrace_layered_bench.py [--lens rf50mm] [--size 1024 1024] [--spp 64] [--launches 10] [--rounds 5]"""
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
    ap.add_argument("--depth", type=float, default=-2000.0, help="object plane of the plane render")
    ap.add_argument("--launches", type=int, default=10)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from aadff import _abi
    from aadff.focal_stack import depth_layers
    from aadff.synth import synth_disc_depth_mm, synth_rgb
    from deeplens.basics import WAVE_RGB
    from deeplens.optics import Lensgroup
    _abi.require_gpu()
    H, W = a.size
    lens = Lensgroup(os.path.join(REPO, "lenses", a.lens, "lens.json"), sensor_res=(H, W), device=DEV)
    pz, pr = lens.exit_pupil()
    n_surf = len(lens.surfaces)
    base = torch.from_numpy(synth_rgb(H, W, seed=3))[None].to(DEV)
    depth = torch.from_numpy(synth_disc_depth_mm(H, W)[0]).to(DEV)
    st = _abi.stream_ptr(torch.device(DEV))
    lens_args = (_abi.ptr(lens._table(WAVE_RGB)), n_surf, float(pz), float(pr), float(lens.sensor_size[1]), float(lens.sensor_size[0]),
                 float(lens.pixel_size))
    res = {"tool": "raytrace_layered_bench", "device": torch.cuda.get_device_name(0), "lens": a.lens, "n_surf": n_surf, "size": [H, W],
           "spp": a.spp, "plane_depth": a.depth, "launches_per_round": a.launches, "rounds": a.rounds}

    def measure(kernel):
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
        return statistics.median(ms), [round(min(ms), 4), round(max(ms), 4)]

    plane = {}
    for B in (1, 4):
        img = base.repeat(B, 1, 1, 1).contiguous()
        out = torch.empty_like(img)
        count = torch.empty((3, H, W), dtype=torch.float32, device=DEV)
        args = (_abi.ptr(img), B, H, W, None, C.c_ulonglong(7), a.spp) + lens_args + (
            a.depth, float(lens.calc_scale_pinhole(a.depth)), 0, _abi.ptr(lens._state_device()), _abi.ptr(out), _abi.ptr(count), None,
            _abi.ptr(lens._flags_device()), st)
        plane[B], spread = measure(lambda: _abi.call("aadff_render_raytraced", *args))
        res[f"plane_B{B}"] = {"ms": round(plane[B], 4), "ms_min_max": spread, "valid_share": round(float(count.mean()) / a.spp, 4)}
        for L in (1, 4, 8):
            idx, centres = depth_layers(depth, L)
            zs = [float(z) for z in centres.cpu()]
            layer = idx.to(torch.uint8)[None].repeat(B, 1, 1).contiguous()
            cov = torch.empty_like(img)
            alive = torch.empty((3, H, W), dtype=torch.float32, device=DEV)
            z_arr, s_arr = (C.c_float * L)(*zs), (C.c_float * L)(*[float(lens.calc_scale_pinhole(z)) for z in zs])
            largs = (_abi.ptr(img), _abi.ptr(layer), B, H, W, None, C.c_ulonglong(7), a.spp) + lens_args + (
                L, C.cast(z_arr, C.c_void_p), C.cast(s_arr, C.c_void_p), 0, _abi.ptr(lens._state_device()), _abi.ptr(out), _abi.ptr(cov),
                _abi.ptr(alive), None, _abi.ptr(lens._flags_device()), st)
            med, spread = measure(lambda: _abi.call("aadff_render_raytraced_layered", *largs))
            res[f"L{L}_B{B}"] = {"ms": round(med, 4), "ms_min_max": spread, "ratio_to_plane": round(med / plane[B], 3),
                                 "layer_depths": [round(z, 1) for z in zs], "coverage_share": round(float(cov.mean()) / a.spp, 4),
                                 "alive_share": round(float(alive.mean()) / a.spp, 4), "finite": bool(torch.isfinite(out).all())}
    lens.check_flags()
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
