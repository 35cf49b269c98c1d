"""GPU tests (run with `-m gpu` on an MI355X) of the fused evaluation metrics (csrc/metrics.hip) through torch.ops.aadff.* and
aadff.metrics, against the numpy oracles of tests/metrics_common.py.  Every row of a batch holds a different image and is compared on
its own, so a batch-stride error cannot cancel.

Depth sums.  Kernel and oracle form every term in float64 from the same float32 inputs with IEEE operations, so the
terms agree bit for bit except where a log enters; only the order of the sums differs.
  * the count, the three threshold counts and the four counts of "finite" mode are integers: exact.
  * every other sum but column 5 adds n non-negative terms: within (n + 8) * 2^-53 relative of the oracle in any order, n the number
    of terms of that sum.  Where a zero of gt is inside the valid set (no mask) the oracle's sum is inf or nan and the kernel's is the same.
  * column 5, sum (log g - log e)^2: the device's float64 log is within one ulp, not correctly rounded.  A log off by |log| 2^-52 moves
    dl = log g - log e by at most (|log g| + |log e|) 2^-52 and dl^2 by 2 |dl| times that; both sides may be off, so the bound is
    sum 4 |dl| (|log g| + |log e|) 2^-52 + (n + 8) 2^-53 sum dl^2, absolute, evaluated on the oracle's own values
    (metrics_common.log_sum_bound).  The largest share of either bound that a row of a case uses goes through the `margin` fixture.
Shapes (N, H, W): a thread owns four pixels of the flattened image and a workgroup 1024, so 37 x 70 (2590 pixels, scalar path, a ragged
last group) and 37 x 76 (2812 pixels, 16-byte path) span three workgroups per image; 1 x 1, 1 x 7 and 5 x 1 are the degenerate extents.

Image sums.  Column 0 (squared error of the quantised images) is an integer: exact.  Column 1 adds one S <= 1 per window, each about ten
float64 roundings away from exact integers, then the sum: within 64 * 2^-53 * n_windows absolute of the integer oracle.  Extents around
the 32 x 64 tile of windows: exactly one tile (38 x 70), one row and one column spilled into new tiles (39 x 71), W % 4 != 0 with two
tiles in a row (37 x 73), and the smallest images.
"""
import inspect
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import metrics_common as mc                                   # noqa: E402
from aadff import _abi, metrics, ops  # noqa: E402,F401
from metrics_common import DEPTH_FUNCS, f32_bound, oracle_scores      # noqa: E402

DEV = "cuda:0"
TH, TW = _abi.SSIM_TILE_H, _abi.SSIM_TILE_W
DEPTH_SHAPES = [(2, 1, 1), (2, 1, 7), (2, 5, 1), (3, 37, 70), (2, 37, 76)]
# (mode, with mask, with conf); the mask of the last image of a batch is all false
DEPTH_VARIANTS = [("mask", False, False), ("mask", True, False), ("mask", True, True), ("mask", False, True), ("finite", False, False),
                  ("finite", False, True)]
IMAGE_SHAPES = [(7, 7), (7, 9), (13, 8), (TH + 6, TW + 6), (TH + 7, TW + 7), (TH + 5, TW + 9)]
INT_COLS, SUM_TERMS = (0, 6, 7, 8, 12, 13, 14, 15), {1: 0, 2: 0, 3: 12, 4: 13, 9: 0, 10: 0, 11: 0}      # sum column -> the column counting its terms

_DEPTH, _IMAGE = {}, {}


def _depth_case(shape):
    """seeded inputs of a shape (cached, never written to): est, gt, mask (last image all false), conf"""
    if shape not in _DEPTH:
        est, gt, mask, conf = mc.depth_inputs(*shape, seed=40 + DEPTH_SHAPES.index(shape))
        mask = mask.copy()
        mask[-1] = False
        _DEPTH[shape] = (est, gt, mask, conf, {})
    return _DEPTH[shape]


def _depth_oracle(shape, mode, use_mask, use_conf):
    est, gt, mask, conf, cache = _depth_case(shape)
    key = (mode, use_mask, use_conf)
    if key not in cache:
        cache[key] = mc.depth_sums(est, gt, mask if use_mask else None, conf if use_conf else None, mode)
    return cache[key]


def _gpu_depth_sums(shape, mode, use_mask, use_conf):
    est, gt, mask, conf, _ = _depth_case(shape)
    t = lambda a: torch.from_numpy(a).to(DEV)                                      # noqa: E731
    none = torch.empty(0, device=DEV)
    out = torch.ops.aadff.depth_metric_sums(t(est), t(gt), t(mask) if use_mask else none, t(conf) if use_conf else none, mode)
    torch.cuda.synchronize()
    return out


def _same(a, b):
    """equal, or both nan: what an infinite or undefined term of the oracle asks of the kernel"""
    return (np.isnan(a) and np.isnan(b)) or a == b


@pytest.mark.parametrize("variant", DEPTH_VARIANTS, ids=["%s_m%d_c%d" % v for v in DEPTH_VARIANTS])
@pytest.mark.parametrize("shape", DEPTH_SHAPES, ids=["%dx%dx%d" % s for s in DEPTH_SHAPES])
def test_depth_sums_match_the_float64_oracle(margin, shape, variant):
    mode, use_mask, use_conf = variant
    est, gt, mask, conf, _ = _depth_case(shape)
    want = _depth_oracle(shape, *variant)
    got_t = _gpu_depth_sums(shape, *variant)
    assert got_t.shape == (shape[0], 16) and got_t.dtype == torch.float64 and got_t.device.type == "cuda"
    got = got_t.cpu().numpy()
    tag = "depth sums %dx%dx%d %s m%d c%d" % (*shape, mode, use_mask, use_conf)
    worst_sum = worst_log = 0.0                                                     # largest share of a bound that any row uses
    for n in range(shape[0]):
        for k in INT_COLS:
            assert got[n, k] == want[n, k], f"{tag}: row {n} column {k}: {got[n, k]} != {want[n, k]}"
        if want[n, 0] == 0:
            assert not got[n].any(), f"{tag}: row {n} has no valid pixel and must be zeros"
            continue
        for k, count_col in SUM_TERMS.items():
            if want[n, k] == 0 or not np.isfinite(want[n, k]):                    # nothing to add, or a zero of gt inside the valid set
                assert _same(got[n, k], want[n, k]), f"{tag}: row {n} column {k}: {got[n, k]} for {want[n, k]}"
                continue
            err, tol = abs(got[n, k] - want[n, k]) / want[n, k], (want[n, count_col] + 8) * mc.U53
            assert err <= tol, f"{tag}: row {n} column {k}: {got[n, k]!r} for {want[n, k]!r}, {err:.3e} relative exceeds {tol:.1e}"
            worst_sum = max(worst_sum, err / tol)
        valid = np.ones(est[n].size, bool) if (mode == "finite" or not use_mask) else mask[n].ravel()
        tol = mc.log_sum_bound(est[n], gt[n], valid, want[n, 14] if mode == "finite" else want[n, 0])
        if np.isfinite(want[n, 5]) and tol > 0:
            err = abs(got[n, 5] - want[n, 5])
            assert err <= tol, f"{tag}: row {n} column 5: {got[n, 5]!r} for {want[n, 5]!r}, {err:.3e} exceeds {tol:.1e}"
            worst_log = max(worst_log, err / tol)
        else:                                                                       # no finite term, or an infinite one that MASK mode keeps
            assert _same(got[n, 5], want[n, 5]), f"{tag}: row {n} column 5: {got[n, 5]} for {want[n, 5]}"
    margin(f"{tag}: float sums, share of (n + 8) 2^-53", worst_sum, 1.0)
    margin(f"{tag}: log sum, share of its bound", worst_log, 1.0)
    if use_mask:                                                                    # the masked-out image: zeros, and nan means
        assert want[-1, 0] == 0 and not got[-1].any()
    again = _gpu_depth_sums(shape, *variant)
    assert torch.equal(again, got_t), f"{tag}: a second run differs"


def test_depth_metrics_of_an_empty_mask_are_nan_and_rows_are_independent():
    shape = (3, 37, 70)
    est, gt, mask, conf, _ = _depth_case(shape)
    d = metrics.depth_metrics(torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask), torch.from_numpy(conf))
    assert all(v.device.type == "cuda" and v.dtype == torch.float64 and v.shape == (3,) for v in d.values())
    want = _depth_oracle(shape, "mask", True, True)
    for n in range(3):
        sc = mc.depth_scores(want[n], "mask", True)
        for k, v in d.items():
            g, w = float(v[n]), float(sc[k])
            if n == 2:
                assert (g == 0.0) if k == "count" else np.isnan(g), (k, g)
            else:
                assert abs(g - w) <= 1e-12 * abs(w), (n, k, g, w)
    assert float(d["mae"][0]) != float(d["mae"][1])
    one = metrics.depth_metrics(torch.from_numpy(est[1]), torch.from_numpy(gt[1]), torch.from_numpy(mask[1]))      # [1,H,W] -> N = 1
    assert float(one["mae"][0]) == float(d["mae"][1])


def test_depth_metrics_accept_other_devices_dtypes_and_shapes():
    est, gt, mask, conf, _ = _depth_case((2, 37, 76))
    e, g, m = torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask)
    base = metrics.depth_metrics(e.to(DEV), g.to(DEV), m.to(DEV))
    for args in ((e.double(), g.double(), m), (e[:, 0], g[:, 0], m[:, 0].to(torch.uint8)), (e.to(DEV), g, m.float() * 3.0),
                 (e.requires_grad_(True), g, m)):
        d = metrics.depth_metrics(*args)
        for k in base:
            assert torch.equal(torch.nan_to_num(d[k], nan=-1.0), torch.nan_to_num(base[k], nan=-1.0)), k
            assert not d[k].requires_grad
    h = metrics.depth_metrics(e.detach().half(), g.half(), m)                       # float16 values, read as float32
    w = mc.depth_sums(e.detach().half().float().numpy(), g.half().float().numpy(), mask)
    assert abs(float(h["mae"][0]) - w[0, 1] / w[0, 0]) <= 1e-12 * w[0, 1] / w[0, 0]
    hw = metrics.depth_metrics(e.detach()[0, 0], g[0, 0], m[0, 0])                 # [H,W]
    assert hw["mae"].shape == (1,) and float(hw["mae"][0]) == float(base["mae"][0])


# ---------------------------------------------------------------- images
def _image_case(key):
    """(pred, target) float32 on the CPU with the integer oracle of their quantised bytes (cached, read-only)"""
    if key not in _IMAGE:
        if key[0] == "adversarial":
            pred, target = mc.adversarial_images(*key[1:])
        else:
            N, Cn, H, W = key
            pred, target = mc.image_inputs(N, Cn, H, W, seed=1000 * Cn + 10 * H + W)
        x, y = mc.quantise(pred).numpy(), mc.quantise(target).numpy()
        _IMAGE[key] = (pred, target, mc.ssim_integer(x, y))
    return _IMAGE[key]


def _check_image_sums(margin, tag, key, ssim=True):
    pred, target, (sse, ssum, nwin) = _image_case(key)
    N = pred.shape[0]
    got_t = torch.ops.aadff.image_metric_sums(pred.to(DEV), target.to(DEV), ssim)
    torch.cuda.synchronize()
    assert got_t.shape == (N, 2) and got_t.dtype == torch.float64
    got = got_t.cpu().numpy()
    for n in range(N):
        assert got[n, 0] == float(sse[n]), f"{tag}: row {n}: squared error {got[n, 0]} != {sse[n]}"
        if ssim:
            margin(f"{tag} row {n} SSIM sum over {nwin} windows", abs(got[n, 1] - ssum[n]), 64 * mc.U53 * nwin)
        else:
            assert got[n, 1] == 0.0
    assert sse.min() > 0 and (N == 1 or sse[0] != sse[1])
    again = torch.ops.aadff.image_metric_sums(pred.to(DEV), target.to(DEV), ssim)
    assert torch.equal(again, got_t), f"{tag}: a second run differs"


@pytest.mark.parametrize("Cn", [1, 3, 4])
@pytest.mark.parametrize("hw", IMAGE_SHAPES, ids=["%dx%d" % s for s in IMAGE_SHAPES])
def test_image_sums_match_the_integer_oracle(margin, hw, Cn):
    _check_image_sums(margin, "image sums %dx%d C%d" % (*hw, Cn), (2, Cn, *hw))


def test_image_sums_of_the_adversarial_quantisation_values(margin):
    _check_image_sums(margin, "image sums adversarial 39x71", ("adversarial", TH + 7, TW + 7, 1))
    _check_image_sums(margin, "image sums adversarial 13x8 C3", ("adversarial", 13, 8, 3))


@pytest.mark.parametrize("hw", [(1, 1), (3, 5), (37, 76)], ids=["1x1", "3x5", "37x76"])
def test_squared_error_alone_needs_no_window(margin, hw):
    _check_image_sums(margin, "image sums %dx%d without SSIM" % hw, (2, 3, *hw), ssim=False)
    pred, target, (sse, _, _) = _image_case((2, 3, *hw))
    a = metrics.image_metrics(pred, target, ssim=False)
    assert list(a) == ["psnr"] and np.allclose(a["psnr"].cpu().numpy(), mc.psnr_of(sse, 3 * hw[0] * hw[1]), rtol=1e-14, atol=0)


def test_image_metrics_and_batch_functions():
    key = (2, 3, TH + 7, TW + 7)
    pred, target, (sse, ssum, nwin) = _image_case(key)
    a = metrics.image_metrics(pred.to(DEV), target.to(DEV))
    assert all(v.device.type == "cuda" and v.dtype == torch.float64 and v.shape == (2,) for v in a.values())
    psnr, ssim = mc.psnr_of(sse, pred[0].numel()), ssum / nwin
    assert np.allclose(a["psnr"].cpu().numpy(), psnr, rtol=1e-14, atol=0) and np.allclose(a["ssim"].cpu().numpy(), ssim, rtol=0, atol=1e-14)
    filt = mc.ssim_filter(mc.quantise(pred).numpy(), mc.quantise(target).numpy())          # the way scikit-image computes it
    assert np.abs(a["ssim"].cpu().numpy() - filt).max() <= 1e-12
    assert metrics.batch_PSNR(pred, target) == round(float(psnr.mean()), 4) == metrics.mask_psnr(pred, target)
    assert metrics.batch_SSIM(pred, target) == round(float(filt.mean()), 4) == metrics.mask_ssim(pred, target)
    same = metrics.image_metrics(pred, pred.clone())
    assert torch.isposinf(same["psnr"]).all() and (same["ssim"] == 1.0).all()
    b = metrics.image_metrics(pred.double(), target.double().requires_grad_(True))
    assert torch.equal(b["psnr"], a["psnr"]) and torch.equal(b["ssim"], a["ssim"]) and not b["ssim"].requires_grad
    c = metrics.image_metrics(pred[0], target[0])                                    # [C,H,W] -> N = 1
    assert c["psnr"].shape == (1,) and float(c["psnr"][0]) == float(a["psnr"][0])


# ---------------------------------------------------------------- the reference's functions and the evaluator
@pytest.mark.parametrize("i", range(3))
def test_wrappers_return_the_recorded_reference_values(golden_dir, margin, i):
    """The recorded values are the reference's float32 results; the GPU's float64 sums are the more exact side, held to the float32
    bound of the host test ((8 + ceil(log2 n)) * 2^-24 relative) and, far inside it, to the float64 oracle."""
    z = np.load(os.path.join(golden_dir, "g19_metrics.npz"))
    gold = {k: z[k] for k in z.files}
    e, g, m, c = (gold[f"s{i}_{k}"] for k in ("est", "gt", "mask", "conf"))
    oracle = oracle_scores(gold, i)
    for name, (key, mode, use_m, use_c) in DEPTH_FUNCS.items():
        f, k = (getattr(metrics, name[:-2]), int(name[-1])) if "accuracy_k" in name else (getattr(metrics, name), None)
        args = {"est_depth": e, "est": e, "gt_depth": g, "gt": g, "mask": m, "conf": c, "k": k}
        got = f(*[args[p] for p in inspect.signature(f).parameters])
        ref, (want, n) = float(gold[f"s{i}_{name}"]), oracle[name]
        assert isinstance(got, float)
        if "accuracy" in name:
            assert got == ref == want, name
        else:
            margin(f"metrics wrapper vs reference: {name} at shape {i}", abs(got - ref) / abs(ref), f32_bound(n))
            assert abs(got - want) <= 1e-11 * abs(want), (name, got, want)
    t = metrics.mask_mae(torch.from_numpy(e).to(DEV), torch.from_numpy(g), torch.from_numpy(m))      # tensors, mixed devices
    assert t == metrics.mask_mae(e, g, m)


def test_evaluator_averages_on_the_device():
    ev = metrics.Evaluator()
    per, n_img = {k: [] for k in ev.KEYS}, 0
    for j in range(3):
        est, gt, mask, _ = mc.depth_inputs(2, 37, 70, seed=70 + j)
        if j == 1:
            mask[1] = False                                                        # left out, as validate() skips such a sample
        pred, target = mc.image_inputs(2, 3, 20, 30, seed=80 + j)
        e, g, m = torch.from_numpy(est).to(DEV), torch.from_numpy(gt).to(DEV), torch.from_numpy(mask).to(DEV)
        ev.update(e, g, m, pred.to(DEV), target.to(DEV))
        d, a = metrics.depth_metrics(e, g, m), metrics.image_metrics(pred.to(DEV), target.to(DEV))
        for n in range(2):
            if j == 1 and n == 1:
                continue
            n_img += 1
            for k in ev.KEYS:
                per[k].append(float((d[k] if k in d else a[k])[n]))
    res = ev.result()
    assert n_img == 5 and list(res) == list(ev.KEYS)
    for k in ev.KEYS:
        want = float(np.mean(per[k]))
        assert abs(res[k] - want) <= 1e-13 * abs(want), (k, res[k], want)
    by_num = ev.result(num=10)
    assert abs(by_num["mae"] - res["mae"] / 2) <= 1e-15
    ev.reset()
    assert all(np.isnan(v) for v in ev.result().values())
    est, gt, mask, _ = mc.depth_inputs(1, 5, 7, seed=3)
    ev.update(torch.from_numpy(est), torch.from_numpy(gt), torch.from_numpy(mask))  # depth only, from the CPU
    r = ev.result()
    assert np.isnan(r["psnr"]) and abs(r["mae"] - float(metrics.depth_metrics(est, gt, mask)["mae"][0])) <= 1e-15
