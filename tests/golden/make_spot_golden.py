#!/usr/bin/env python3
"""Generate fixture G17 (tests/golden/g17_spot.npz + g17_spot.json) by IMPORTING the reference: its ray-traced lens
analysis - pupil sampling (deeplens/optics.py:539-591), magnification (:1221-1256, :1294-1307), RMS spot radii
(:1975-2012), spot-diagram centroids (:1832-1862) and the line `analysis()` prints (:1552-1563).

Every call runs after its own `torch.manual_seed`; the next `torch.rand(8)` is stored beside its result, so a test can
check that the same number of draws was consumed.  Runs only where the reference checkout is (CPU, ~2 minutes), with the
import stubs of make_golden.py.

Usage:  PYTHONDONTWRITEBYTECODE=1 python tests/golden/make_spot_golden.py
"""
import contextlib
import io
import json
import os
import sys
import tempfile

sys.dont_write_bytecode = True
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import make_golden as mg  # noqa: E402  (installs the import stubs and imports the reference)

import numpy as np  # noqa: E402
import torch  # noqa: E402

ref_optics = sys.modules["deeplens.optics"]
Lensgroup, REF, HERE, CPU = mg.Lensgroup, mg.REF, mg.HERE, mg.CPU

CONFIGS = (("rf50mm", (480, 640)), ("50mm_f2.8", (480, 640)), ("rf50mm", (1024, 1024)))
ANALYSIS_CONFIGS = (("rf50mm", (480, 640)), ("50mm_f2.8", (480, 640)))


class _Axis:
    def __init__(self, rec, i, j):
        self.rec, self.i, self.j = rec, i, j

    def scatter(self, x, y, *a, **k):
        if len(x) == 1:                                   # the second scatter of each panel is the centroid (optics.py:1849)
            self.rec[self.i, self.j] = (float(x[0]), float(y[0]))

    def set_aspect(self, *a, **k):
        pass


class _SpotPlot:
    """Stands in for matplotlib.pyplot inside draw_spot_diagram: records the centroid of every panel, writes no file."""

    def __init__(self):
        self.rec = None

    def subplots(self, M, N, **k):
        self.rec = np.full((M, N, 2), np.nan)
        axs = np.empty((M, N), dtype=object)
        for i in range(M):
            for j in range(N):
                axs[i, j] = _Axis(self.rec, i, j)
        return None, axs

    def savefig(self, *a, **k):
        pass

    def close(self, *a, **k):
        pass


def seeded(seed, fn):
    torch.manual_seed(seed)
    out = fn()
    return out, torch.rand(8).numpy()


def main():
    arrays, meta = {}, {}
    # sample_pupil, both branches, explicit pupil (no trace needed)
    lens = Lensgroup(filename=f"{REF}/lenses/rf50mm/lens.json", sensor_res=(480, 640), device=CPU)
    for tag, spp, res in (("strat", 16, (3, 4)), ("naive", 12, (3, 4))):
        o, r8 = seeded(7, lambda: lens.sample_pupil(res=res, spp=spp, num_angle=8, pupilr=3.1, pupilz=1.7))
        arrays[f"pupil_{tag}"], arrays[f"pupil_{tag}_rand8"] = o.numpy(), r8
        meta[f"pupil_{tag}"] = {"seed": 7, "spp": spp, "res": list(res), "num_angle": 8, "pupilr": 3.1, "pupilz": 1.7}

    for name, res in CONFIGS:
        key = f"{name}@{res[0]}x{res[1]}"
        lens = Lensgroup(filename=f"{REF}/lenses/{name}/lens.json", sensor_res=res, device=CPU)
        rec = {"entrance_pupil": [float(v) for v in lens.entrance_pupil()], "hfov": float(lens.hfov)}
        mag, r8 = seeded(1, lambda: lens.calc_magnification3(-20000))
        rec["mag_-20000"], arrays[f"{key}/mag_rand8"] = float(mag), r8
        s, r8 = seeded(3, lambda: lens.calc_scale_ray(-1500.0))
        rec["scale_-1500"], arrays[f"{key}/scale_rand8"] = float(s), r8
        s, r8 = seeded(4, lambda: lens.calc_scale_ray(torch.tensor([-1500.0, -20000.0])))
        arrays[f"{key}/scale_vec"], arrays[f"{key}/scale_vec_rand8"] = s.numpy(), r8
        for seed, ref in ((2, True), (5, False)):
            out, r8 = seeded(seed, lambda: lens.analysis_rms(ref=ref))
            rec[f"rms_ref{int(ref)}"] = [float(v) for v in out]           # (rms_avg, on-axis, off-axis) in mm
            arrays[f"{key}/rms_ref{int(ref)}_rand8"] = r8
        plot, real = _SpotPlot(), ref_optics.plt
        ref_optics.plt = plot
        try:
            _, r8 = seeded(6, lambda: lens.draw_spot_diagram(M=7, save_name="unused"))
        finally:
            ref_optics.plt = real
        arrays[f"{key}/spot_centroids"], arrays[f"{key}/spot_rand8"] = plot.rec, r8
        meta[key] = rec
        print(key, rec, flush=True)

    for name, res in ANALYSIS_CONFIGS:
        key = f"{name}@{res[0]}x{res[1]}"
        with tempfile.TemporaryDirectory() as tmp:
            torch.manual_seed(0)
            lens = Lensgroup(filename=f"{REF}/lenses/{name}/lens.json", sensor_res=res, device=CPU)
            buf = io.StringIO()
            with contextlib.redirect_stdout(buf):
                lens.analysis(save_name=os.path.join(tmp, "lens"))
            arrays[f"{key}/analysis_rand8"] = torch.rand(8).numpy()
        meta[key]["analysis_line"] = [ln for ln in buf.getvalue().splitlines() if ln.startswith("On-axis RMS radius")][0]
        print(key, meta[key]["analysis_line"], flush=True)

    np.savez_compressed(f"{HERE}/g17_spot.npz", **arrays)
    with open(f"{HERE}/g17_spot.json", "w") as f:
        json.dump(meta, f, indent=1)


if __name__ == "__main__":
    main()
