#!/usr/bin/env python3
"""Wall time of the ray-traced lens analysis on one GPU: analysis_rms() (calc_scale_ray + four passes of 31 x 31 fields x 2048
rays, one aadff_spot_moments launch each call) and calc_magnification3(), rf50mm at 480 x 640.  Prints one JSON line; run it
under `rocprofv3 --kernel-trace --stats -- python tools/spot_profile.py` for the kernel times.

    PYTHONPATH=aberration-aware-depth-from-focus_amd python tools/spot_profile.py [reps]
"""
import json
import os
import sys
import time

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd")]

import torch  # noqa: E402
from deeplens.optics import Lensgroup  # noqa: E402


def timed(fn, reps):
    out = []
    for _ in range(reps):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        fn()
        torch.cuda.synchronize()
        out.append(time.perf_counter() - t0)
    return out


if __name__ == "__main__":
    reps = int(sys.argv[1]) if len(sys.argv) > 1 else 5
    lens = Lensgroup(os.path.join(REPO, "lenses", "rf50mm", "lens.json"), sensor_res=(480, 640), device="cuda:0")
    torch.manual_seed(2)
    rms = lens.analysis_rms()                                   # warm-up (pinned block, tables, pupil cache)
    lens.calc_magnification3(-20000)
    t_rms = timed(lambda: lens.analysis_rms(), reps)
    t_mag = timed(lambda: lens.calc_magnification3(-20000), reps)
    t_draw = timed(lambda: torch.rand(4 * 2 * 2048 * 961 + 2 * 512 * 441), reps)
    print(json.dumps({"analysis_rms_s": sorted(t_rms), "calc_magnification3_s": sorted(t_mag),
                      "torch_rand_same_count_s": sorted(t_draw), "rms_mm": [float(v) for v in rms],
                      "device": torch.cuda.get_device_name(0)}))
