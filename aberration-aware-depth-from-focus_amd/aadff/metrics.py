"""Evaluation metrics on the GPU: what `validate()` of the reference's training script computes around its network
(2_aber_aware_dff_aif.py:189-214 with dff/metrics.py) - nine depth scores by nine numpy passes over host copies, PSNR and SSIM by
scikit-image on quantised host copies - as two fused HIP calls whose results stay on the device.

    scores = depth_metrics(est, gt, mask)                  # dict of [N] float64 tensors: abs_rel, sq_rel, mae, mse, rmse, rmse_log, ...
    scores = image_metrics(pred_aif, gt_aif)               # {'psnr': [N], 'ssim': [N]}
    ev = Evaluator(); ev.update(est, gt, mask, pred_aif, gt_aif); ...; ev.result()      # one read-back at the end of a validation loop

plus every public function of the reference's dff/metrics.py except the two bumpiness ones, under its own name and signature (numpy arrays
or tensors in, a float out): thin wrappers over the two calls, and the one place here that synchronises.  The kernels are
csrc/metrics.hip (`torch.ops.aadff.depth_metric_sums`, `torch.ops.aadff.image_metric_sums`): float64 terms from the exactly converted
float32 inputs, exact integer window sums for SSIM, no atomics, bit-reproducible.  There is no CPU fallback: without the HIP library or
a GPU the functions raise like the renderers.  scikit-image is not needed.
"""
import numpy as np
import torch

from . import _abi, ops  # noqa: F401  (registers torch.ops.aadff.depth_metric_sums / image_metric_sums)

VALID = ("mask", "finite")
DEPTH_KEYS = ("abs_rel", "sq_rel", "mae", "mse", "rmse", "rmse_log", "accuracy_1", "accuracy_2", "accuracy_3")
# the columns of torch.ops.aadff.depth_metric_sums (include/aadff.h)
COUNT, S_ABS, S_SQ, S_REL, S_SQREL, S_LOG, N_LT1, N_LT2, N_LT3, S_CONF, S_CONF_ABS, S_CONF_SQ, N_REL, N_SQREL, N_LOG, N_Q = range(16)


def _device_of(t):
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _tensor(who, name, t):
    if isinstance(t, np.ndarray):
        t = torch.from_numpy(np.ascontiguousarray(t))
    if not torch.is_tensor(t):
        raise TypeError(f"{who}: {name} must be a tensor or a numpy array, not {type(t).__name__}")
    return t


def _depth_map(who, name, t, floating=True):
    """[H,W], [N,H,W] or [N,1,H,W] -> [N,1,H,W]"""
    t = _tensor(who, name, t)
    if floating and not t.is_floating_point():
        raise TypeError(f"{who}: {name} must have a floating dtype, not {t.dtype}")
    if t.dim() == 2:
        return t[None, None]
    if t.dim() == 3:
        return t[:, None]
    if t.dim() == 4 and t.shape[1] == 1:
        return t
    raise ValueError(f"{who}: {name} must be [N,1,H,W], [N,H,W] or [H,W], not {tuple(t.shape)}")


def depth_metrics(est, gt, mask=None, conf=None, valid="mask"):
    """Per-image depth scores of est against gt ([N,1,H,W], [N,H,W] or [H,W], any floating dtype, any device; the arithmetic reads them
    as float32) -> dict of [N] float64 tensors on the GPU, without synchronising.

    valid "mask": over the pixels where mask (bool, or numeric: non-zero) holds, all pixels without a mask - the reference's mask_*,
    AIF_DepthNEt_*, mae, mse and rmse.  valid "finite" (no mask): over all pixels, an infinite term left out of its sum and of its
    count, a nan kept - the reference's unmasked abs_rel, sq_rel, rmse_log and accuracy_k, each with its own idea of "infinite".
    Keys: abs_rel = mean |g - e| / g, sq_rel = mean (g - e)^2 / g, mae, mse, rmse, rmse_log = sqrt(mean (log g - log e)^2), accuracy_k =
    share of max(e / g, g / e) < 1.25^k, count = valid pixels, and with conf ([N,1,H,W] weights) mae_w_conf = sum conf |g - e| / sum conf
    and mse_w_conf.  An image without valid pixels has count 0 and nan scores, like numpy's mean of nothing."""
    who = "depth_metrics"
    if valid not in VALID:
        raise ValueError(f"{who}: valid {valid!r} is not one of {VALID}")
    e, g = _depth_map(who, "est", est), _depth_map(who, "gt", gt)
    if e.shape != g.shape:
        raise ValueError(f"{who}: est {tuple(e.shape)} and gt {tuple(g.shape)} differ in shape")
    m = c = None
    if mask is not None:
        if valid == "finite":
            raise ValueError(f"{who}: valid 'finite' takes every pixel, a mask cannot be given with it")
        m = _depth_map(who, "mask", mask, floating=False)
        if m.shape != e.shape:
            raise ValueError(f"{who}: mask {tuple(m.shape)} does not match est {tuple(e.shape)}")
    if conf is not None:
        c = _depth_map(who, "conf", conf)
        if c.shape != e.shape:
            raise ValueError(f"{who}: conf {tuple(c.shape)} does not match est {tuple(e.shape)}")
    N, _, H, W = e.shape
    if H * W == 0:
        raise ValueError(f"{who}: the maps are {H} x {W}, at least one pixel is needed")
    if N == 0:
        s = torch.zeros((0, _abi.DEPTH_METRIC_COLS), dtype=torch.float64, device=e.device)
    else:
        _abi.require_gpu()
        dev = _device_of(e)
        none = torch.empty((0,), dtype=torch.float32, device=dev)
        if m is not None:
            m = m.to(dev)
            m = m if m.dtype == torch.bool else m != 0
        s = torch.ops.aadff.depth_metric_sums(_abi.f32c(e.detach(), dev), _abi.f32c(g.detach(), dev), none if m is None else m.contiguous(),
                                              none if c is None else _abi.f32c(c.detach(), dev), valid)
    n = s[:, COUNT]
    finite = valid == "finite"
    mse = s[:, S_SQ] / n
    out = {"abs_rel": s[:, S_REL] / (s[:, N_REL] if finite else n), "sq_rel": s[:, S_SQREL] / (s[:, N_SQREL] if finite else n),
           "mae": s[:, S_ABS] / n, "mse": mse, "rmse": torch.sqrt(mse), "rmse_log": torch.sqrt(s[:, S_LOG] / (s[:, N_LOG] if finite else n))}
    for k in (1, 2, 3):
        out[f"accuracy_{k}"] = s[:, N_LT1 + k - 1] / (s[:, N_Q] if finite else n)
    out["count"] = n
    if c is not None:
        out["mae_w_conf"], out["mse_w_conf"] = s[:, S_CONF_ABS] / s[:, S_CONF], s[:, S_CONF_SQ] / s[:, S_CONF]
    return out


def image_metrics(pred, target, ssim=True):
    """PSNR and SSIM of pred against target ([N,C,H,W] or [C,H,W], C in 1..4, values nominally in [0,1], any floating dtype, any device)
    -> {'psnr': [N], 'ssim': [N]} float64 on the GPU ('ssim' only when asked for), without synchronising.

    Both images are quantised to bytes as the reference's batch_PSNR / batch_SSIM do (img * 255 + 0.5, clamped, truncated).  psnr =
    10 log10(255^2 / mean (x - y)^2), inf for equal images; ssim = scikit-image's structural_similarity with its defaults and
    channel_axis=0: uniform 7 x 7 window, sample covariance, K1 0.01, K2 0.03, data range 255, the mean over the image cropped by 3 on
    every side and over the channels.  Like scikit-image, SSIM refuses an image smaller than the window."""
    who = "image_metrics"
    x, y = _tensor(who, "pred", pred), _tensor(who, "target", target)
    if not (x.is_floating_point() and y.is_floating_point()):
        raise TypeError(f"{who}: pred and target must have floating dtypes, not {x.dtype} and {y.dtype}")
    if x.dim() == 3:
        x = x[None]
    if y.dim() == 3:
        y = y[None]
    if x.dim() != 4 or x.shape != y.shape:
        raise ValueError(f"{who}: pred {tuple(x.shape)} and target {tuple(y.shape)} must both be [N,C,H,W]")
    N, Cn, H, W = x.shape
    if not 1 <= Cn <= 4:
        raise ValueError(f"{who}: the images have C = {Cn} channels, expected 1..4")
    if H * W == 0:
        raise ValueError(f"{who}: the images are {H} x {W}, at least one pixel is needed")
    if ssim and min(H, W) < 7:
        raise ValueError(f"{who}: SSIM needs images of at least 7 x 7 (its window), got H = {H}, W = {W}")
    if N == 0:
        s = torch.zeros((0, 2), dtype=torch.float64, device=x.device)
    else:
        _abi.require_gpu()
        dev = _device_of(x)
        s = torch.ops.aadff.image_metric_sums(_abi.f32c(x.detach(), dev), _abi.f32c(y.detach(), dev), bool(ssim))
    out = {"psnr": 10.0 * torch.log10(65025.0 / (s[:, 0] / float(Cn * H * W)))}
    if ssim:
        out["ssim"] = s[:, 1] / float(Cn * (H - 6) * (W - 6))
    return out


class Evaluator:
    """The running averages of a validation loop, kept on the GPU:

        update(est, gt, mask, pred_aif=None, gt_aif=None)   adds the per-image scores of a batch, without synchronising
        result(num=None)                                    one read-back -> dict of floats: the nine depth scores (DEPTH_KEYS) and
                                                            'psnr', 'ssim', each a sum over the images divided by `num` when given
                                                            (validate() divides by its own num_val), else by the images counted
        reset()

    An image whose mask is empty is left out of every sum and of the count, as validate() skips such a sample."""
    KEYS = DEPTH_KEYS + ("psnr", "ssim")

    def __init__(self):
        self.reset()

    def reset(self):
        self._sum = None                                      # [13]: the eleven sums, depth images counted, image pairs counted

    def update(self, est, gt, mask, pred_aif=None, gt_aif=None):
        d = depth_metrics(est, gt, mask)
        keep = d["count"] > 0
        zero = torch.zeros((), dtype=torch.float64, device=keep.device)
        rows = [torch.where(keep, d[k], zero).sum() for k in DEPTH_KEYS]
        n_img = zero
        if (pred_aif is None) != (gt_aif is None):
            raise ValueError("Evaluator.update: pred_aif and gt_aif go together")
        if pred_aif is not None:
            a = image_metrics(pred_aif, gt_aif)
            if a["psnr"].shape != keep.shape:
                raise ValueError(f"Evaluator.update: {a['psnr'].shape[0]} image pairs for {keep.shape[0]} depth maps")
            a = {k: v.to(keep.device) for k, v in a.items()}
            rows += [torch.where(keep, a["psnr"], zero).sum(), torch.where(keep, a["ssim"], zero).sum()]
            n_img = keep.sum().to(torch.float64)
        else:
            rows += [zero, zero]
        add = torch.stack(rows + [keep.sum().to(torch.float64), n_img])
        self._sum = add if self._sum is None else self._sum.to(add.device) + add

    def result(self, num=None):
        if self._sum is None:
            return {k: float("nan") for k in self.KEYS}
        s = self._sum.cpu().tolist()                          # the one synchronisation
        with np.errstate(all="ignore"):
            out = {k: float(np.float64(s[i]) / np.float64(s[11] if num is None else num)) for i, k in enumerate(DEPTH_KEYS)}
            for i, k in ((9, "psnr"), (10, "ssim")):
                out[k] = float(np.float64(s[i]) / np.float64(s[12] if num is None else num))
        return out


# ---------------------------------------------------------------- the reference's functions (dff/metrics.py), names and signatures kept
def _one(who, name, t):
    """any array -> one image [1,1,R,C]: the reference's functions treat their arguments as one set of pixels"""
    t = _tensor(who, name, t)
    if t.numel() == 0:
        return t.reshape(1, 1, 1, 0)
    return t.reshape(1, 1, -1, t.shape[-1]) if t.dim() >= 1 else t.reshape(1, 1, 1, 1)


def _score(who, key, est_depth, gt_depth, mask=None, conf=None, valid="mask"):
    e, g = _one(who, "est_depth", est_depth), _one(who, "gt_depth", gt_depth)
    if e.numel() == 0:
        return float("nan")
    m = None if mask is None else _one(who, "mask", mask)
    c = None if conf is None else _one(who, "conf", conf)
    try:
        d = depth_metrics(e, g, m, c, valid)
    except ValueError as err:
        raise ValueError(str(err).replace("depth_metrics", who)) from None
    return float(d[key].cpu()[0])


def abs_rel(est_depth, gt_depth):
    return _score("abs_rel", "abs_rel", est_depth, gt_depth, valid="finite")


def sq_rel(est_depth, gt_depth):
    return _score("sq_rel", "sq_rel", est_depth, gt_depth, valid="finite")


def mae(est_depth, gt_depth):
    return _score("mae", "mae", est_depth, gt_depth)


def mse(est_depth, gt_depth):
    return _score("mse", "mse", est_depth, gt_depth)


def rmse(est_depth, gt_depth):
    return _score("rmse", "rmse", est_depth, gt_depth)


def rmse_log(est_depth, gt_depth):
    return _score("rmse_log", "rmse_log", est_depth, gt_depth, valid="finite")


def _k(who, k):
    if k not in (1, 2, 3):
        raise ValueError(f"{who}: k = {k!r}, the thresholds 1.25^k are computed for k in 1, 2, 3")
    return f"accuracy_{int(k)}"


def accuracy_k(est_depth, gt_depth, k):
    return _score("accuracy_k", _k("accuracy_k", k), est_depth, gt_depth, valid="finite")


def AIF_DepthNEt_abs_rel(est, gt, mask):
    return _score("AIF_DepthNEt_abs_rel", "abs_rel", est, gt, mask)


def AIF_DepthNEt_sq_rel(est, gt, mask):
    return _score("AIF_DepthNEt_sq_rel", "sq_rel", est, gt, mask)


def mask_abs_rel(est_depth, gt_depth, mask):
    return _score("mask_abs_rel", "abs_rel", est_depth, gt_depth, mask)


def mask_sq_rel(est_depth, gt_depth, mask):
    return _score("mask_sq_rel", "sq_rel", est_depth, gt_depth, mask)


def mask_mse(est_depth, gt_depth, mask):
    return _score("mask_mse", "mse", est_depth, gt_depth, mask)


def mask_mae(est_depth, gt_depth, mask):
    return _score("mask_mae", "mae", est_depth, gt_depth, mask)


def mask_rmse(est_depth, gt_depth, mask):
    return _score("mask_rmse", "rmse", est_depth, gt_depth, mask)


def mask_rmse_log(est_depth, gt_depth, mask):
    return _score("mask_rmse_log", "rmse_log", est_depth, gt_depth, mask)


def mask_accuracy_k(est_depth, gt_depth, k, mask):
    return _score("mask_accuracy_k", _k("mask_accuracy_k", k), est_depth, gt_depth, mask)


def mask_mse_w_conf(est_depth, gt_depth, conf, mask):
    return _score("mask_mse_w_conf", "mse_w_conf", est_depth, gt_depth, mask, conf)


def mask_mae_w_conf(est_depth, gt_depth, conf, mask):
    return _score("mask_mae_w_conf", "mae_w_conf", est_depth, gt_depth, mask, conf)


def mask_mse_w_conf_wo_mask(est_depth, gt_depth, conf):
    return _score("mask_mse_w_conf_wo_mask", "mse_w_conf", est_depth, gt_depth, None, conf)


def mask_mae_w_conf_wo_mask(est_depth, gt_depth, conf):
    return _score("mask_mae_w_conf_wo_mask", "mae_w_conf", est_depth, gt_depth, None, conf)


def _batch_mean(who, key, img, img_clean):
    try:
        v = image_metrics(img, img_clean, ssim=key == "ssim")[key]
    except ValueError as err:
        raise ValueError(str(err).replace("image_metrics", who)) from None
    if v.numel() == 0:
        raise ZeroDivisionError(f"{who}: the batch is empty")
    v = v.cpu().tolist()
    return round(sum(v) / len(v), 4)                          # the reference's rounding of the batch mean


def batch_PSNR(img, img_clean):
    """ Compute PSNR for image batch.
    """
    return _batch_mean("batch_PSNR", "psnr", img, img_clean)


def batch_SSIM(img, img_clean):
    """ Compute SSIM for image batch.
    """
    return _batch_mean("batch_SSIM", "ssim", img, img_clean)


def mask_psnr(est_aif, gt_aif):
    return batch_PSNR(est_aif, gt_aif)


def mask_ssim(est_aif, gt_aif):
    return batch_SSIM(est_aif, gt_aif)


__all__ = ["depth_metrics", "image_metrics", "Evaluator", "abs_rel", "sq_rel", "mae", "mse", "rmse", "rmse_log", "accuracy_k",
           "AIF_DepthNEt_abs_rel", "AIF_DepthNEt_sq_rel", "mask_abs_rel", "mask_sq_rel", "mask_mse", "mask_mae", "mask_rmse", "mask_rmse_log",
           "mask_accuracy_k", "mask_mse_w_conf", "mask_mae_w_conf", "mask_mse_w_conf_wo_mask", "mask_mae_w_conf_wo_mask", "batch_PSNR",
           "batch_SSIM", "mask_psnr", "mask_ssim"]
