"""The evaluation metrics (aadff/metrics.py, csrc/metrics.hip) restated from their specification (include/aadff.h) in numpy
and torch on the CPU, and the seeded inputs of their tests.

  depth_sums / depth_scores     the sixteen float64 sums per image and the scores formed from them
  log_sum_bound                 how far two float64 evaluations of column 5 may differ when each log is within one ulp
  DEPTH_FUNCS / oracle_scores   which score, mode and arguments each function of the reference's dff/metrics.py stands for
  f32_bound                     what the reference's float32 arithmetic may differ by from float64
  quantise                      the reference's literal torch expression
  ssim_integer                  SSIM from exact integer box sums (cumulative sums in int64), integer numerators, S in float64
  ssim_filter                   SSIM the way scikit-image computes it: scipy.ndimage.uniform_filter in float64
"""
import math

import numpy as np
import torch

COLS = 16
THRESHOLDS = (1.25, 1.5625, 1.953125)
C1, C2 = (0.01 * 255.0) ** 2, (0.03 * 255.0) ** 2
U53, U24 = 2.0 ** -53, 2.0 ** -24


# ---------------------------------------------------------------- depth
def depth_sums(est, gt, mask=None, conf=None, mode="mask"):
    """est, gt [N,1,H,W] float32 arrays (mask bool, conf float32, or None) -> [N,16] float64, column numbering of include/aadff.h"""
    est, gt = np.asarray(est, np.float32), np.asarray(gt, np.float32)
    N = est.shape[0]
    out = np.zeros((N, COLS))
    with np.errstate(all="ignore"):
        for n in range(N):
            e, g = est[n].astype(np.float64).ravel(), gt[n].astype(np.float64).ravel()
            c = np.zeros_like(e) if conf is None else np.asarray(conf, np.float32)[n].astype(np.float64).ravel()
            d = g - e
            ad, d2 = np.abs(d), d * d
            rel, sq = ad / g, d2 / g
            lg, le = np.log(g), np.log(e)
            l2 = (lg - le) ** 2
            q = np.maximum(e / g, g / e)
            if mode == "finite":
                v = np.ones(e.shape, bool)
                row = [v.sum(), ad.sum(), d2.sum(), np.where(np.isinf(rel), 0.0, rel).sum(), np.where(np.isinf(sq), 0.0, sq).sum(),
                       np.where(np.isinf(l2), 0.0, l2).sum()]
                tail = [(~np.isinf(rel)).sum(), (~np.isinf(sq)).sum(), (~np.isinf(le) & ~np.isinf(lg)).sum(), (~np.isinf(q)).sum()]
            else:
                v = np.ones(e.shape, bool) if mask is None else np.asarray(mask)[n].ravel() != 0
                row = [v.sum(), ad[v].sum(), d2[v].sum(), rel[v].sum(), sq[v].sum(), l2[v].sum()]
                tail = [0, 0, 0, 0]
            row += [(q[v] < t).sum() for t in THRESHOLDS] + [c[v].sum(), (c * ad)[v].sum(), (c * d2)[v].sum()]
            out[n] = np.array(row + tail, np.float64)
    return out


def depth_scores(s, mode="mask", conf=False):
    """the scores of one row of sums, as aadff.metrics.depth_metrics forms them"""
    s = np.asarray(s, np.float64)
    fin = mode == "finite"
    with np.errstate(all="ignore"):
        n = s[0]
        out = {"abs_rel": s[3] / (s[12] if fin else n), "sq_rel": s[4] / (s[13] if fin else n), "mae": s[1] / n, "mse": s[2] / n,
               "rmse": np.sqrt(s[2] / n), "rmse_log": np.sqrt(s[5] / (s[14] if fin else n)), "count": n}
        for k in (1, 2, 3):
            out[f"accuracy_{k}"] = s[5 + k] / (s[15] if fin else n)
        if conf:
            out["mae_w_conf"], out["mse_w_conf"] = s[10] / s[9], s[11] / s[9]
    return out


def log_sum_bound(est, gt, valid, n_terms):
    """Absolute bound on the difference between two float64 evaluations of sum (log g - log e)^2 over `valid` whose logs are each within
    one ulp of the true value (what the device's float64 log promises; numpy's is at least as good).  A log in error by
    |log| * 2^-52 moves dl = log g - log e by at most (|log g| + |log e|) * 2^-52, so dl^2 by 2 |dl| times that (the square of the error
    is below the last bit), per side; two sides double it.  The subtraction, the square and the order of the sum add the
    (n + 8) * 2^-53 relative of every other column."""
    e, g = np.asarray(est, np.float64).ravel()[valid], np.asarray(gt, np.float64).ravel()[valid]
    with np.errstate(all="ignore"):
        lg, le = np.log(g), np.log(e)
        dl = lg - le
        ok = np.isfinite(dl)
        per_log = 2.0 * (2.0 * np.abs(dl[ok]) * (np.abs(lg[ok]) + np.abs(le[ok])) * 2.0 ** -52).sum()
        return per_log + (n_terms + 8) * U53 * (dl[ok] ** 2).sum()


def depth_inputs(N, H, W, seed, zeros=0.2):
    """different images per row: gt in [0.3, 3.2] with exact zeros, est = gt * exp(N(0, 0.25)) + 0.01, mask = gt > 0, conf in [0.1, 1]"""
    rng = np.random.default_rng(seed)
    gt = rng.uniform(0.3, 3.2, (N, 1, H, W)).astype(np.float32)
    gt[rng.uniform(size=gt.shape) < zeros] = 0.0
    est = (gt * np.exp(rng.normal(0.0, 0.25, gt.shape)).astype(np.float32) + np.float32(0.01)).astype(np.float32)
    conf = rng.uniform(0.1, 1.0, gt.shape).astype(np.float32)
    return est, gt, gt > 0, conf


# ---------------------------------------------------------------- the reference's functions on the golden inputs (g19_metrics.npz)
# reference function -> (score, mode, takes mask, takes conf)
DEPTH_FUNCS = {
    "abs_rel": ("abs_rel", "finite", 0, 0), "sq_rel": ("sq_rel", "finite", 0, 0), "rmse_log": ("rmse_log", "finite", 0, 0),
    "mae": ("mae", "mask", 0, 0), "mse": ("mse", "mask", 0, 0), "rmse": ("rmse", "mask", 0, 0),
    "AIF_DepthNEt_abs_rel": ("abs_rel", "mask", 1, 0), "AIF_DepthNEt_sq_rel": ("sq_rel", "mask", 1, 0),
    "mask_abs_rel": ("abs_rel", "mask", 1, 0), "mask_sq_rel": ("sq_rel", "mask", 1, 0), "mask_mse": ("mse", "mask", 1, 0),
    "mask_mae": ("mae", "mask", 1, 0), "mask_rmse": ("rmse", "mask", 1, 0), "mask_rmse_log": ("rmse_log", "mask", 1, 0),
    "mask_mse_w_conf": ("mse_w_conf", "mask", 1, 1), "mask_mae_w_conf": ("mae_w_conf", "mask", 1, 1),
    "mask_mse_w_conf_wo_mask": ("mse_w_conf", "mask", 0, 1), "mask_mae_w_conf_wo_mask": ("mae_w_conf", "mask", 0, 1),
}
for _k in (1, 2, 3):
    DEPTH_FUNCS[f"accuracy_k_{_k}"] = (f"accuracy_{_k}", "finite", 0, 0)
    DEPTH_FUNCS[f"mask_accuracy_k_{_k}"] = (f"accuracy_{_k}", "mask", 1, 0)


def f32_bound(n):
    return (8 + math.ceil(math.log2(max(n, 1)))) * U24


def golden_case(gold, i):
    e, g, m, c = (gold[f"s{i}_{k}"][None, None] for k in ("est", "gt", "mask", "conf"))
    return e, g, m, c


def oracle_scores(gold, i):
    """name of a recorded reference function -> (the float64 oracle's value, the number of pixels behind it)"""
    e, g, m, c = golden_case(gold, i)
    rows = {("finite", 0, 0): depth_sums(e, g, None, None, "finite")[0], ("mask", 0, 0): depth_sums(e, g, None, None)[0],
            ("mask", 1, 0): depth_sums(e, g, m, None)[0], ("mask", 1, 1): depth_sums(e, g, m, c)[0], ("mask", 0, 1): depth_sums(e, g, None, c)[0]}
    out = {}
    for name, (key, mode, use_m, use_c) in DEPTH_FUNCS.items():
        s = rows[(mode, use_m, use_c)]
        n = {"abs_rel": s[12], "sq_rel": s[13], "rmse_log": s[14]}.get(key, s[15]) if mode == "finite" else s[0]
        out[name] = (depth_scores(s, mode, bool(use_c))[key], int(n))
    return out


# ---------------------------------------------------------------- images
def quantise(img):
    """the reference's expression (dff/metrics.py batch_PSNR), out of place"""
    return img.mul(255).add(0.5).clamp(0, 255).to(torch.uint8)


def adversarial_values():
    """float32 values where the rule can go wrong: the neighbours (0, +-1, +-2 ulp) of every (k + 0.5) / 255, k = 0..254, of 0 and 1,
    negative values, values above 1 and -0.0"""
    ties = np.concatenate([(np.arange(255, dtype=np.float64) + 0.5) / 255.0, [0.0, 1.0, 1.0 / 255.0, 254.5 / 255.0]]).astype(np.float32)
    vals = [ties]
    up, down = ties.copy(), ties.copy()
    for _ in range(2):
        up, down = np.nextafter(up, np.float32(np.inf)), np.nextafter(down, np.float32(-np.inf))
        vals += [up.copy(), down.copy()]
    vals.append(np.array([-0.0, -1e-8, -0.001, -0.0019607844, -0.5, -3.0, 1.0000001, 1.001, 1.0019608, 1.5, 2.0, 300.0, 1e-45, -1e-45, 0.99999994],
                         np.float32))
    return np.concatenate(vals)


def _box(a):
    """sums over every full 7 x 7 window of the last two axes, exact in int64: [...,H,W] -> [...,H-6,W-6]"""
    c = np.cumsum(np.cumsum(a.astype(np.int64), axis=-2), axis=-1)
    c = np.pad(c, [(0, 0)] * (a.ndim - 2) + [(1, 0), (1, 0)])
    return c[..., 7:, 7:] - c[..., :-7, 7:] - c[..., 7:, :-7] + c[..., :-7, :-7]


def ssim_integer(x, y):
    """x, y [N,C,H,W] uint8 -> (sse [N] int64, sum of S over windows and channels [N] float64, number of windows per image)"""
    x, y = np.asarray(x).astype(np.int64), np.asarray(y).astype(np.int64)
    sse = ((x - y) ** 2).sum(axis=(1, 2, 3))
    if x.shape[2] < 7 or x.shape[3] < 7:
        return sse, np.zeros(x.shape[0]), 0
    sx, sy, sxx, syy, sxy = _box(x), _box(y), _box(x * x), _box(y * y), _box(x * y)
    nx, ny, nxy = 49 * sxx - sx * sx, 49 * syy - sy * sy, 49 * sxy - sx * sy            # exact
    ux, uy = sx / 49.0, sy / 49.0
    vx, vy, vxy = nx / 2352.0, ny / 2352.0, nxy / 2352.0                                # / (49 * 48): sample covariance
    S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux * ux + uy * uy + C1) * (vx + vy + C2))
    return sse, S.sum(axis=(1, 2, 3)), int(np.prod(S.shape[1:]))


def ssim_filter(x, y):
    """x, y [N,C,H,W] uint8 -> mean SSIM [N] float64 as skimage.metrics.structural_similarity(channel_axis=0) computes it on uint8
    images: uniform_filter in float64, sample covariance, crop by 3, mean over pixels and then over channels"""
    from scipy.ndimage import uniform_filter
    x, y = np.asarray(x).astype(np.float64), np.asarray(y).astype(np.float64)
    out = np.zeros(x.shape[0])
    for n in range(x.shape[0]):
        per = []
        for c in range(x.shape[1]):
            X, Y = x[n, c], y[n, c]
            ux, uy = uniform_filter(X, size=7), uniform_filter(Y, size=7)
            uxx, uyy, uxy = uniform_filter(X * X, size=7), uniform_filter(Y * Y, size=7), uniform_filter(X * Y, size=7)
            k = 49.0 / 48.0
            vx, vy, vxy = k * (uxx - ux * ux), k * (uyy - uy * uy), k * (uxy - ux * uy)
            S = ((2 * ux * uy + C1) * (2 * vxy + C2)) / ((ux ** 2 + uy ** 2 + C1) * (vx + vy + C2))
            per.append(S[3:-3, 3:-3].mean(dtype=np.float64))
        out[n] = np.mean(per)
    return out


def psnr_of(sse, count):
    with np.errstate(divide="ignore"):
        return 10.0 * np.log10(65025.0 / (np.asarray(sse, np.float64) / count))


def image_inputs(N, Cn, H, W, seed):
    """different images per row: a smooth pattern plus noise as target, target plus smaller noise as pred, both a little outside [0,1]"""
    g = torch.Generator().manual_seed(seed)
    yy, xx = torch.meshgrid(torch.arange(H, dtype=torch.float32), torch.arange(W, dtype=torch.float32), indexing="ij")
    base = torch.stack([0.5 + 0.45 * torch.sin(0.37 * (n + 1) * xx + 0.1 * c) * torch.cos(0.23 * yy + 0.5 * n) for n in range(N) for c in range(Cn)])
    target = base.reshape(N, Cn, H, W) + 0.08 * torch.randn(N, Cn, H, W, generator=g)
    pred = target + 0.05 * (1 + torch.arange(N, dtype=torch.float32).reshape(N, 1, 1, 1)) * torch.randn(N, Cn, H, W, generator=g)
    return pred.contiguous(), target.contiguous()


def adversarial_images(H, W, Cn=1):
    """one pair [1,Cn,H,W] filled with the adversarial quantisation values, in two different orders"""
    v = torch.from_numpy(adversarial_values())
    n = Cn * H * W
    reps = (n + v.numel() - 1) // v.numel()
    a = v.repeat(reps)[:n].reshape(1, Cn, H, W)
    b = v.flip(0).roll(7).repeat(reps)[:n].reshape(1, Cn, H, W)
    return a.contiguous(), b.contiguous()
