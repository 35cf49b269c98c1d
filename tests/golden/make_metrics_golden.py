#!/usr/bin/env python3
"""Writes tests/golden/g19_metrics.npz: what the numpy-only functions of the reference's dff/metrics.py return on seeded float32 inputs,
recorded as data, plus the signatures of all its public functions.  Run once, on the CPU, where a checkout of the reference is at hand;
the tests only read the file.

    python tests/golden/make_metrics_golden.py --reference /path/to/reference [--out tests/golden/g19_metrics.npz]

The reference's file imports scikit-image, which is stubbed here the way make_golden.py stubs it: batch_PSNR, batch_SSIM (and mask_psnr,
mask_ssim on top of them) and the two bumpiness functions need the real library and are NOT recorded; only their signatures are.

Per shape (3 x 5, 37 x 70, 37 x 76): gt uniform in [0.3, 3.2] with about 20 % exact zeros, mask = gt > 0, est = gt * exp(N(0, 0.25)) + 0.01
(so the unmasked functions meet real infinities and no nan), conf uniform in [0.1, 1].  The seed is advanced until no valid pixel's ratio
max(e / g, g / e) lies within 1e-5 relative of 1.25, 1.5625 or 1.953125; float32 and float64 then give the same accuracy counts, which is
asserted.  Every function is fed float32 arrays, as the reference's script feeds it."""
import argparse
import importlib.util
import inspect
import os
import sys
import types

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
SHAPES = [(3, 5), (37, 70), (37, 76)]
THRESHOLDS = (1.25, 1.5625, 1.953125)
NOT_RECORDED = ("get_bumpiness", "get_bumpiness_non_mask", "batch_PSNR", "batch_SSIM", "mask_psnr", "mask_ssim")


def load_reference(root):
    sk, skf, skm = types.ModuleType("skimage"), types.ModuleType("skimage.filters"), types.ModuleType("skimage.metrics")
    skm.peak_signal_noise_ratio = skm.structural_similarity = None
    sk.filters, sk.metrics = skf, skm
    for name, mod in (("skimage", sk), ("skimage.filters", skf), ("skimage.metrics", skm)):
        sys.modules.setdefault(name, mod)
    keep = sys.dont_write_bytecode
    sys.dont_write_bytecode = True
    try:
        spec = importlib.util.spec_from_file_location("ref_metrics", os.path.join(root, "dff", "metrics.py"))
        ref = importlib.util.module_from_spec(spec)
        spec.loader.exec_module(ref)
    finally:
        sys.dont_write_bytecode = keep
    return ref


def inputs(shape, seed):
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.3, 3.2, shape).astype(np.float32)
    gt[rng.uniform(size=shape) < 0.2] = 0.0
    est = (gt * np.exp(rng.normal(0.0, 0.25, shape)).astype(np.float32) + np.float32(0.01)).astype(np.float32)
    conf = rng.uniform(0.1, 1.0, shape).astype(np.float32)
    return est, gt, gt > 0, conf


def ratio(est, gt, dtype):
    e, g = est.astype(dtype), gt.astype(dtype)
    with np.errstate(all="ignore"):
        return np.maximum(e / g, g / e)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--reference", required=True, help="root of a checkout of the reference project")
    ap.add_argument("--out", default=os.path.join(HERE, "g19_metrics.npz"))
    a = ap.parse_args()
    ref = load_reference(a.reference)
    funcs = {k: v for k, v in vars(ref).items() if inspect.isfunction(v) and v.__module__ == ref.__name__}
    data = {"shapes": np.array(SHAPES, np.int32), "thresholds": np.array(THRESHOLDS),
            "signatures": np.array([f"{k}{inspect.signature(v)}" for k, v in funcs.items()])}
    seed = 1900
    for i, shape in enumerate(SHAPES):
        while True:
            est, gt, mask, conf = inputs(shape, seed)
            seed += 1
            q64 = ratio(est, gt, np.float64)
            near = min(float(np.min(np.abs(q64[mask] / t - 1.0))) for t in THRESHOLDS)
            if near > 1e-5 and mask.any() and not mask.all() and not np.isnan(q64).any():
                break
        q32 = ratio(est, gt, np.float32)
        for t in THRESHOLDS:
            assert np.array_equal(q32 < np.float32(t), q64 < t), "float32 and float64 disagree on a threshold"
        tag = f"s{i}_"
        data.update({tag + "est": est, tag + "gt": gt, tag + "mask": mask, tag + "conf": conf, tag + "nearest": np.float64(near)})
        with np.errstate(all="ignore"):
            for name, f in funcs.items():
                if name in NOT_RECORDED:
                    continue
                pars = list(inspect.signature(f).parameters)
                args = {"est_depth": est, "est": est, "gt_depth": gt, "gt": gt, "mask": mask, "conf": conf}
                for k in ((1, 2, 3) if "k" in pars else (None,)):
                    val = f(*[(k if p == "k" else args[p].copy()) for p in pars])
                    data[tag + name + (f"_{k}" if k else "")] = np.float64(val)
        print(f"{shape}: seed {seed - 1}, {int(mask.sum())} of {mask.size} valid, nearest threshold {near:.2e}, "
              f"mask_abs_rel {float(data[tag + 'mask_abs_rel']):.6f}, abs_rel {float(data[tag + 'abs_rel']):.6f}")
    np.savez_compressed(a.out, **data)
    print(f"{a.out}: {os.path.getsize(a.out)} bytes, {len(data)} entries")


if __name__ == "__main__":
    main()
