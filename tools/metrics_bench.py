#!/usr/bin/env python3
"""The fused evaluation metrics (csrc/metrics.hip: aadff_depth_metric_sums and aadff_image_metric_sums) at the validation size of the
reference's script (1 x 480 x 640, 3-channel images) and at 1024^2, against

  (a) the same arithmetic as a torch composition on the same GPU: float64 terms and masked sums for the depth scores; quantisation,
      7 x 7 box sums of the integer-valued float64 images (avg_pool2d) and the SSIM map for the images;
  (b) the reference's route: device -> host copies of depth, prediction, mask and both images, nine numpy passes in float32 for the depth
      scores, PSNR in numpy and SSIM through the scipy-based filter oracle of the tests (scikit-image itself is not required here);
  (c) the bytes that must move - depth 9 H W (est, gt, mask once), images 8 C H W (both once) - over the kernel time, as a share of the
      8 TB/s of HBM.

The kernel legs call the C ABI with every buffer allocated once (--launches launches between two device events); the torch leg is timed
the same way, the host route with a wall clock around synchronised copies.  The legs alternate --rounds times; the median round is
reported with the spread.  The results of all three are also compared.

Prints ONE JSON line.    python tools/metrics_bench.py [--launches 100] [--rounds 5] [--out profiles/metrics_bench.json]"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

HERE = os.path.dirname(os.path.abspath(__file__))
REPO = os.path.dirname(HERE)
for p in (REPO, os.path.join(REPO, "aberration-aware-depth-from-focus_amd"), os.path.join(REPO, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

DEV = "cuda:0"
HBM_BYTES_PER_S = 8.0e12
SHAPES = [(1, 3, 480, 640), (1, 3, 1024, 1024)]              # N, C of the images, H, W


def torch_depth(e, g, m):
    """the nine scores of one image as float64 torch operations on the device"""
    import torch
    e, g = e.double()[m], g.double()[m]
    d = g - e
    n = e.numel()
    q = torch.maximum(e / g, g / e)
    return torch.stack([(d.abs() / g).sum() / n, (d * d / g).sum() / n, (d * d).sum() / n, d.abs().sum() / n, ((d * d).sum() / n).sqrt(),
                        ((g.log() - e.log()) ** 2).sum().div(n).sqrt(), (q < 1.25).sum() / n, (q < 1.5625).sum() / n, (q < 1.953125).sum() / n])


def torch_image(x, y):
    """(psnr, ssim) of one batch as torch operations on the device; the box sums of integer-valued float64 images are exact"""
    import torch
    import torch.nn.functional as F
    qx, qy = (t.mul(255).add(0.5).clamp(0, 255).to(torch.uint8).double() for t in (x, y))
    mse = ((qx - qy) ** 2).mean(dim=(1, 2, 3))
    box = lambda t: F.avg_pool2d(t, 7, stride=1)                                   # noqa: E731
    ux, uy, uxx, uyy, uxy = box(qx), box(qy), box(qx * qx), box(qy * qy), box(qx * qy)
    k, c1, c2 = 49.0 / 48.0, (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
    vx, vy, vxy = k * (uxx - ux * ux), k * (uyy - uy * uy), k * (uxy - ux * uy)
    s = ((2 * ux * uy + c1) * (2 * vxy + c2)) / ((ux * ux + uy * uy + c1) * (vx + vy + c2))
    return 10.0 * torch.log10(65025.0 / mse), s.mean(dim=(1, 2, 3))


def host_route(e, g, m, x, y):
    """what validate() does per sample: copies to the host, nine float32 numpy passes, quantised copies of the images, PSNR and SSIM"""
    import numpy as np
    import torch

    import metrics_common as mc
    e, g, m = np.squeeze(e.cpu().numpy()), np.squeeze(g.cpu().numpy()), np.squeeze(m.cpu().numpy())
    with np.errstate(all="ignore"):
        out = [np.mean(np.abs(g[m] - e[m]) / g[m]), np.mean((g[m] - e[m]) ** 2 / g[m]), np.mean((g[m] - e[m]) ** 2), np.mean(np.abs(g[m] - e[m])),
               np.sqrt(np.mean((e[m] - g[m]) ** 2)), np.sqrt(np.mean((np.log(g[m]) - np.log(e[m])) ** 2))]
        for k in (1, 2, 3):
            out.append(np.sum(np.maximum(e[m] / g[m], g[m] / e[m]) < 1.25 ** k) / np.sum(m))
    qx, qy = (t.cpu().mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8).numpy() for t in (x, y))
    mse = np.mean((qx.astype(np.float64) - qy.astype(np.float64)) ** 2, axis=(1, 2, 3))
    return np.array(out, np.float64), 10.0 * np.log10(65025.0 / mse), mc.ssim_filter(qx, qy)


def bench_shape(shape, a):
    import numpy as np
    import torch

    import metrics_common as mc
    from aadff import _abi, metrics, ops
    N, Cn, H, W = shape
    est, gt, mask, _ = mc.depth_inputs(N, H, W, seed=7)
    e, g, m = (torch.from_numpy(t).to(DEV) for t in (est, gt, mask))
    pred, target = (t.to(DEV) for t in mc.image_inputs(N, Cn, H, W, seed=8))
    dsums = torch.empty((N, 16), dtype=torch.float64, device=DEV)
    isums = torch.empty((N, 2), dtype=torch.float64, device=DEV)
    nd, ni = ops.depth_metric_workspace_bytes(N, H, W), ops.image_metric_workspace_bytes(N, Cn, H, W, True)
    wd, wi = torch.empty(nd // 8, dtype=torch.float64, device=DEV), torch.empty(ni // 8, dtype=torch.float64, device=DEV)
    st = _abi.stream_ptr(torch.device(DEV))

    def k_depth():
        _abi.call("aadff_depth_metric_sums", _abi.ptr(e), _abi.ptr(g), _abi.ptr(m), None, _abi.ptr(dsums), _abi.ptr(wd), C.c_size_t(nd), N, H, W, 0, st)

    def k_image():
        _abi.call("aadff_image_metric_sums", _abi.ptr(pred), _abi.ptr(target), _abi.ptr(isums), _abi.ptr(wi), C.c_size_t(ni), N, Cn, H, W, 1, st)

    def k_both():
        k_depth()
        k_image()

    def t_both():
        return torch_depth(e[0, 0], g[0, 0], m[0, 0]), torch_image(pred, target)

    def api_both():                                           # the public calls: op dispatch, allocation of outputs and workspaces included
        return metrics.depth_metrics(e, g, m), metrics.image_metrics(pred, target)

    def timed(fn, n):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(n):
            fn()
        e1.record()
        e1.synchronize()
        return e0.elapsed_time(e1) / n                        # ms per call

    def host_timed(fn, n):
        torch.cuda.synchronize()
        t0 = time.perf_counter()
        for _ in range(n):
            fn()
        return (time.perf_counter() - t0) * 1e3 / n

    for _ in range(10):
        k_both()
    for _ in range(3):
        t_d, (t_p, t_s) = t_both()
    torch.cuda.synchronize()
    h_d, h_p, h_s = host_route(e, g, m, pred, target)
    d, im = api_both()
    k_d = np.array([float(d[k][0]) for k in ("abs_rel", "sq_rel", "mse", "mae", "rmse", "rmse_log", "accuracy_1", "accuracy_2", "accuracy_3")])
    agree = {"depth_vs_torch_max_rel": float(np.max(np.abs(k_d - t_d.cpu().numpy()) / np.abs(k_d))),
             "depth_vs_host_float32_max_rel": float(np.max(np.abs(k_d - h_d) / np.abs(k_d))),
             "psnr_vs_torch_abs": float((im["psnr"] - t_p).abs().max()), "ssim_vs_torch_abs": float((im["ssim"] - t_s).abs().max()),
             "psnr_vs_host_abs": float(np.max(np.abs(im["psnr"].cpu().numpy() - h_p))), "ssim_vs_host_abs": float(np.max(np.abs(im["ssim"].cpu().numpy() - h_s)))}
    legs = {"kernel_depth": (k_depth, a.launches, timed), "kernel_image": (k_image, a.launches, timed), "kernel_both": (k_both, a.launches, timed),
            "api_both": (api_both, a.launches, timed), "torch_both": (t_both, a.torch_launches, timed),
            "host_route": (lambda: host_route(e, g, m, pred, target), a.host_launches, host_timed)}
    times = {k: [] for k in legs}
    for _ in range(a.rounds):                                 # alternate the legs
        for k, (fn, n, how) in legs.items():
            times[k].append(how(fn, n))
    med = {k: statistics.median(v) for k, v in times.items()}
    b_depth, b_image = 9 * N * H * W, 8 * N * Cn * H * W
    tbs = lambda nbytes, ms: nbytes / (ms * 1e-3) / 1e12      # noqa: E731
    out = {"shape": list(shape), "ms": {k: round(v, 5) for k, v in med.items()},
           "ms_min_max": {k: [round(min(v), 5), round(max(v), 5)] for k, v in times.items()},
           "kernel_vs_torch": round(med["torch_both"] / med["kernel_both"], 2), "api_vs_torch": round(med["torch_both"] / med["api_both"], 2),
           "kernel_vs_host_route": round(med["host_route"] / med["kernel_both"], 1),
           "bytes_that_must_move": {"depth": b_depth, "image": b_image},
           "achieved_TB_per_s": {"depth": round(tbs(b_depth, med["kernel_depth"]), 4), "image": round(tbs(b_image, med["kernel_image"]), 4)},
           "agreement": {k: float(f"{v:.3e}") for k, v in agree.items()}}
    out["share_of_8TBps_byte_roofline"] = {k: round(v * 1e12 / HBM_BYTES_PER_S, 4) for k, v in out["achieved_TB_per_s"].items()}
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--launches", type=int, default=100)
    ap.add_argument("--torch-launches", type=int, default=10)
    ap.add_argument("--host-launches", type=int, default=2)
    ap.add_argument("--rounds", type=int, default=5)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch

    from aadff import _abi
    _abi.require_gpu()
    res = {"tool": "metrics_bench", "device": torch.cuda.get_device_name(0), "launches_per_round": a.launches, "torch_launches_per_round": a.torch_launches,
           "host_launches_per_round": a.host_launches, "rounds": a.rounds, "shapes": [bench_shape(s, a) for s in SHAPES]}
    line = json.dumps(res)
    print(line)
    if a.out:
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
