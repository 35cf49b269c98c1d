#!/usr/bin/env python3
"""Bit comparison of two builds of the library on the ray-traced lens analysis and the ray-traced renders, for a change that moves
or restates their kernels' text without meaning to change a number (the split of trace.hip).

    split_trace_compare.py hash OUT.json                   the library named by AADFF_LIB (or the tree's own): run every case below,
                                                           write {case: {output: sha256}}
    split_trace_compare.py compare OLD.so NEW.so OUT.json  `hash` in a fresh process per library, then {case: {output: [old, new]}},
                                                           "all_equal"; exit status 1 unless every pair is equal

Cases, at the shapes of the GPU tests (inputs of tests/mtf_common.py, tests/raytrace_common.py, tests/raytrace_layered_common.py):
    spot, mtf   both lenses, spp 64 and 520, the 3 x 3 field grid, the draws of mtf_common.uniforms; aadff_spot_moments with
                ref_mode 0 and 1 (second moments on), aadff_mtf_points with the tests' five frequencies and three sensor planes
    render      both lenses, 24 x 32 (the tests' size) and 21 x 29 (no multiple of the 8-pixel wave block), B = 1 .. 5, draws
                given and generated; the plane render at -2000 and -500 mm, the layered render with L = 1 and L = 4
"""
import ctypes as C
import hashlib
import json
import os
import subprocess
import sys

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd"), os.path.join(REPO, "tests")]

DEPTHS4 = (-500.0, -1000.0, -2000.0, -4000.0)


def sha(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def make_lens(name, res):
    """the sensor by its size, as the GPU tests make it (tests/test_gpu_raytrace.py)"""
    import numpy as np
    from deeplens.optics import Lensgroup
    import raytrace_common as rc
    h, w = res
    lens = Lensgroup(rc.lens_file(name), device="cuda:0", post_computation=False)
    ws = 2 * lens.r_last * w / np.sqrt(h ** 2 + w ** 2)
    while (ws * h / w) / ws != h / w:           # prepare_sensor's exact test for square pixels: the next width that passes it
        ws = float(np.nextafter(ws, np.inf))
    lens.prepare_sensor(res, sensor_size=[ws * h / w, ws])
    lens.post_computation()
    return lens


def analysis_cases(out):
    import numpy as np
    import torch
    import mtf_common as mc
    from aadff import _abi
    from deeplens.basics import WAVE_RGB
    dev = torch.device("cuda:0")
    for name in mc.LENSES:
        lens = make_lens(name, mc.RES)
        torch.manual_seed(mc.SEED)
        lens.refocus(mc.DEPTH)
        pobj = lens._point_grid(lens.sensor_size[0] / 2 * lens.calc_scale_pinhole(mc.DEPTH), mc.DEPTH, 3).reshape(-1, 3)
        P, L = pobj.shape[0], len(WAVE_RGB)
        pupilz, pupilr = lens.entrance_pupil()
        st, flags, table = lens._state_device(), lens._flags_device(), lens._table(WAVE_RGB)
        pts = pobj.to(dev).float().contiguous()
        freqs = mc.FREQS + (float(np.float32(0.5 / lens.pixel_size)),)
        F, Z = len(freqs), len(mc.DEFOCUS)
        fr, df = (C.c_float * F)(*freqs), (C.c_float * Z)(*mc.DEFOCUS)
        for spp in (64, 520):
            u = torch.as_tensor(mc.uniforms(L, spp, P)).reshape(-1).to(dev)
            for ref_mode in (0, 1):
                mom = torch.empty((L, P, 4), dtype=torch.float32, device=dev)
                _abi.call("aadff_spot_moments", _abi.ptr(pts), P, _abi.ptr(u), spp, 8, L, _abi.ptr(table), len(lens.surfaces), float(pupilz),
                          float(pupilr), _abi.ptr(st), ref_mode, 1, _abi.ptr(mom), _abi.ptr(flags), _abi.stream_ptr(dev))
                out[f"spot {name} spp{spp} ref_mode{ref_mode}"] = {"moments": sha(mom)}
            otf = torch.empty((L, P, Z, 2, F, 2), dtype=torch.float32, device=dev)
            mom = torch.empty((L, P, 8), dtype=torch.float32, device=dev)
            _abi.call("aadff_mtf_points", _abi.ptr(pts), P, _abi.ptr(u), spp, 8, L, _abi.ptr(table), len(lens.surfaces), float(pupilz),
                      float(pupilr), _abi.ptr(st), C.cast(fr, C.c_void_p), F, C.cast(df, C.c_void_p), Z, 0, _abi.ptr(otf), _abi.ptr(mom),
                      _abi.ptr(flags), _abi.stream_ptr(dev))
            out[f"mtf {name} spp{spp}"] = {"otf": sha(otf), "moments": sha(mom)}
        lens.check_flags()


def render_cases(out):
    import torch
    import raytrace_common as rc
    dev = "cuda:0"
    for name in rc.LENSES:
        for res in ((rc.H, rc.W), (21, 29)):
            h, w = res
            lens = make_lens(name, res)
            g = torch.Generator().manual_seed(2)
            img = torch.rand((5, 3, h, w), generator=g).to(dev)
            maps = torch.randint(0, 5, (5, h, w), generator=g).to(torch.uint8).to(dev)          # index 4: holes
            u = torch.rand((3, rc.SPP, 2, h, w), generator=g).to(dev)
            scales = tuple(float(lens.calc_scale_pinhole(z)) for z in DEPTHS4)
            for B in range(1, 6):
                for draws, kw in (("u", dict(u=u)), ("seed", dict(seed=11))):
                    for depth in rc.DEPTHS:
                        o, aux = lens.render_raytraced(img[:B], depth=depth, spp=rc.SPP, scale=float(lens.calc_scale_pinhole(depth)),
                                                       return_aux="valid", **kw)
                        out[f"plane {name} {h}x{w} B{B} {draws} depth{depth:g}"] = {"out": sha(o), **{k: sha(v) for k, v in sorted(aux.items())}}
                    for nl in (1, 4):
                        lay = maps[:B] if nl == 4 else torch.zeros_like(maps[:B])
                        o, aux = lens.render_raytraced_layered(img[:B], lay, DEPTHS4[:nl], scales=scales[:nl], spp=rc.SPP,
                                                               return_aux="valid", **kw)
                        out[f"layered {name} {h}x{w} B{B} {draws} L{nl}"] = {"out": sha(o), **{k: sha(v) for k, v in sorted(aux.items())}}
            lens.check_flags()


def hash_all(path):
    from aadff import _abi
    out = {}
    analysis_cases(out)
    render_cases(out)
    with open(path, "w") as f:
        json.dump({"library": os.path.basename(os.path.dirname(os.path.abspath(_abi.LIB_PATH))) + "/" + os.path.basename(_abi.LIB_PATH),
                   "cases": out}, f, indent=0, sort_keys=True)
    print(f"{len(out)} cases -> {path}")


def compare(old_lib, new_lib, path):
    got = []
    for lib in (old_lib, new_lib):
        tmp = path + "." + str(len(got)) + ".tmp"
        subprocess.check_call([sys.executable, os.path.abspath(__file__), "hash", tmp], env=dict(os.environ, AADFF_LIB=os.path.abspath(lib)))
        with open(tmp) as f:
            got.append(json.load(f)["cases"])
        os.remove(tmp)
    old, new = got
    assert sorted(old) == sorted(new)
    pairs = {c: {k: [old[c][k], new[c][k]] for k in old[c]} for c in old}
    differ = sorted(f"{c}: {k}" for c in pairs for k, (a, b) in pairs[c].items() if a != b)
    with open(path, "w") as f:
        json.dump({"cases": len(pairs), "outputs": sum(len(v) for v in pairs.values()), "all_equal": not differ, "differ": differ, "sha256": pairs},
                  f, indent=0, sort_keys=True)
    print(f"{len(pairs)} cases, {sum(len(v) for v in pairs.values())} outputs: " + ("every pair equal" if not differ else f"{len(differ)} DIFFER: {differ[:8]}"))
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "hash":
        hash_all(sys.argv[2])
    elif len(sys.argv) == 5 and sys.argv[1] == "compare":
        sys.exit(compare(*sys.argv[2:]))
    else:
        sys.exit(__doc__)
