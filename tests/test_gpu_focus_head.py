"""GPU tests (run with `-m gpu` on an MI355X) of the fused depth head and its loss (csrc/focus_head.hip) through torch.ops.aadff.* and
aadff.focus_head, against the torch CPU oracle of tests/focus_head_common.py evaluated in float64 on the same float32 inputs.

Budget of every parity comparison: relative L2 per tensor <= 4 x d32, where d32 is the distance of the SAME oracle
evaluated in float32 on the CPU from its float64 evaluation, computed here for the very inputs of the case - the project's standing
allowance for another summation order of the same float32 terms (tests/test_gpu_diffrender.py).  Nothing is measured against the code
under test and no pixel is excluded.  Where d32 is exactly 0 (a tensor that float32 represents exactly) the kernel must be exact too.
Every (error, 4 x d32) pair goes through the `margin` fixture.

Bounds this file derives itself:
  * the count of the mask is an integer: exact.  The sums of |e|, e^2 and |aif - gt| add float32 terms in float64, so they carry only the
    roundings of their terms: one (the subtraction), three (the subtraction twice, the product) and one - relative bounds 1, 3 and 1 x 2^-24.
  * the loss dict is float32 made from the float64 sums by one rounding: its budget is that of the oracle's dict plus 2^-24.
Shapes of the head (N, K, Ct, S, H, W): a thread owns four pixels of a row and a workgroup 1024, so 37 x 76 (16-byte path) and 37 x 70
(scalar path, ragged groups) span three workgroups per image; 33 x 68 is N = 1 with [S] focus distances' shape; the others are the
degenerate extents 1 x 1, 1 x 7, 5 x 1, 3 x 3 and S = 1.  One case has 2.2e9 elements per tensor: offsets past 2^31 show only there.
"""
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import focus_head_common as fc                               # noqa: E402
from aadff import ops  # noqa: E402,F401
from aadff.focus_head import AttentionHead, attention_depth, dff_losses      # noqa: E402

DEV = "cuda:0"
U24 = 2.0 ** -24
HEAD_SHAPES = [(2, 1, 3, 1, 1, 1), (2, 2, 4, 3, 1, 7), (2, 1, 1, 2, 5, 1), (2, 2, 3, 3, 3, 3), (2, 1, 3, 10, 37, 76), (2, 2, 4, 17, 37, 70),
               (1, 1, 4, 8, 33, 68), (2, 2, 3, 8, 37, 76)]
HEAD_IDS = ["%dx%dx%dx%dx%dx%d" % s for s in HEAD_SHAPES]
HEAD_KEYS = ("depth", "aif", "d_scores", "d_stack", "d_foc_dists")
LOSS_SHAPES = [(1, 1, 1, 1), (1, 7, 1, 7), (5, 1, 5, 1), (3, 3, 3, 3), (37, 70, 37, 70), (37, 76, 37, 76), (37, 76, 35, 70)]      # H, W, gt H, gt W
LOSS_IDS = ["%dx%d_gt%dx%d" % s for s in LOSS_SHAPES]
WEIGHTS = dict(disp_w=1.0, aif_w=0.7, smooth_w=0.3)

_HEAD = {}


def _head_case(shape, norm):
    """Seeded inputs of a case with the oracle in float64 and float32 (cached, read-only)."""
    if (shape, norm) not in _HEAD:
        t = fc.head_inputs(*shape, seed=10 + HEAD_SHAPES.index(shape))
        args = (t["scores"], t["stack"], t["foc_dists"], t["g_depth"], t["g_aif"], norm)
        _HEAD[(shape, norm)] = (t, fc.head_grads(*args, dtype=torch.float64), fc.head_grads(*args, dtype=torch.float32))
    return _HEAD[(shape, norm)]


def _gpu_head(t, norm, need=(True, True, True), aif_channels=None):
    """The op and its backward for the cotangents of `t`; a gradient that is not needed comes back as None."""
    z, x, u = (t[k].to(DEV).requires_grad_(n) for k, n in zip(("scores", "stack", "foc_dists"), need))
    Ca = min(x.shape[1], 3) if aif_channels is None else aif_channels
    depth, aif = torch.ops.aadff.attention_depth(z, x, u, norm, Ca)
    if any(need):
        torch.autograd.backward([depth, aif], [t["g_depth"].to(DEV), t["g_aif"][:, :Ca].to(DEV)])
    torch.cuda.synchronize()
    cpu = lambda v: None if v is None else v.detach().cpu()                        # noqa: E731
    return {"depth": cpu(depth), "aif": cpu(aif), "d_scores": cpu(z.grad), "d_stack": cpu(x.grad), "d_foc_dists": cpu(u.grad)}


def _budget(margin, name, got, f64, f32):
    err, d32 = fc.rel_l2(got, f64), fc.rel_l2(f32, f64)
    print(f"{name}: error {err:.3e}, d32 {d32:.3e}")
    if d32 == 0.0:
        assert err == 0.0, f"{name}: the float32 oracle is exact, the kernel is {err:.3e} off"
    else:
        margin(name, err, 4.0 * d32)


@pytest.mark.parametrize("norm", [False, True], ids=["softmax", "softplus"])
@pytest.mark.parametrize("shape", HEAD_SHAPES, ids=HEAD_IDS)
def test_head_against_the_oracle(shape, norm, margin):
    t, f64, f32 = _head_case(shape, norm)
    got = _gpu_head(t, norm)
    N, K, Ct, S, H, W = shape
    Ca = min(Ct, 3)
    assert got["depth"].shape == (N, 1, H, W) and got["aif"].shape == (N, Ca, H, W) and got["d_scores"].shape == (N, K, S, H, W)
    assert got["d_stack"].shape == (N, Ct, S, H, W) and got["d_foc_dists"].shape == (N, S)
    tag = f"focus head {HEAD_IDS[HEAD_SHAPES.index(shape)]} {'softplus' if norm else 'softmax'}"
    for k in HEAD_KEYS:
        assert got[k].dtype == torch.float32 and bool(torch.isfinite(got[k]).all()), k       # also with scores of +-80 and +-1e4
        _budget(margin, f"{tag} {k}", got[k], f64[k], f32[k])
    assert bool((got["d_stack"][:, Ca:] == 0).all())


@pytest.fixture(scope="module")
def gold(golden_dir):
    z = np.load(os.path.join(golden_dir, "g18_focus_head.npz"))
    return {k: (torch.from_numpy(z[k]) if z[k].dtype.kind == "f" else z[k]) for k in z.files}


@pytest.mark.parametrize("i", range(4))
def test_head_against_the_reference_golden(gold, i, margin):
    K, norm = (int(v) for v in gold["nets"][i])
    t = {"scores": gold[f"net{i}_logits"], "stack": gold["stack"], "foc_dists": gold["foc_dists"], "g_depth": gold["g_depth"], "g_aif": gold["g_aif"]}
    args = (t["scores"], t["stack"], t["foc_dists"], t["g_depth"], t["g_aif"], bool(norm))
    f64, f32 = fc.head_grads(*args, dtype=torch.float64), fc.head_grads(*args, dtype=torch.float32)
    got = _gpu_head(t, bool(norm))
    for key, name in (("depth", "depth"), ("aif", "aif"), ("d_scores", "d_logits")):
        err, d32 = fc.rel_l2(got[key], gold[f"net{i}_{name}"]), fc.rel_l2(f32[key], f64[key])
        print(f"golden net {i} {name}: kernel vs reference {err:.3e}, d32 {d32:.3e}")
        margin(f"focus head golden net{i} K{K} {'softplus' if norm else 'softmax'} {name}", err, 4.0 * d32)


@pytest.mark.parametrize("norm", [False, True], ids=["softmax", "softplus"])
@pytest.mark.parametrize("shape", [(2, 1, 3, 1, 1, 1), (2, 2, 4, 1, 37, 70), (2, 1, 3, 1, 37, 76)], ids=["1x1", "K2_37x70", "37x76"])
def test_head_one_slice_is_exact(shape, norm):
    t = fc.head_inputs(*shape, seed=3)
    N, K, Ct, S, H, W = shape
    got = _gpu_head(t, norm)
    assert torch.equal(got["depth"], t["foc_dists"].reshape(N, 1, 1, 1).expand(N, 1, H, W))
    assert torch.equal(got["aif"], t["stack"][:, :3, 0])
    assert bool((got["d_scores"] == 0).all())
    assert torch.equal(got["d_stack"][:, :3, 0], t["g_aif"]) and bool((got["d_stack"][:, 3:] == 0).all())


@pytest.mark.parametrize("norm", [False, True], ids=["softmax", "softplus"])
@pytest.mark.parametrize("shape", [HEAD_SHAPES[1], HEAD_SHAPES[4], HEAD_SHAPES[5]], ids=[HEAD_IDS[1], HEAD_IDS[4], HEAD_IDS[5]])
def test_head_runs_repeat_and_gradients_do_not_depend_on_each_other(shape, norm):
    t, _, _ = _head_case(shape, norm)
    full = _gpu_head(t, norm)
    again = _gpu_head(t, norm)
    assert all(torch.equal(full[k], again[k]) for k in HEAD_KEYS)
    for need in ((True, False, False), (False, True, False), (False, False, True), (True, True, False), (True, False, True), (False, True, True)):
        got = _gpu_head(t, norm, need)
        assert torch.equal(got["depth"], full["depth"]) and torch.equal(got["aif"], full["aif"])
        for k, n in zip(("d_scores", "d_stack", "d_foc_dists"), need):
            assert torch.equal(got[k], full[k]) if n else got[k] is None, (k, need)
    none = _gpu_head(t, norm, (False, False, False))
    assert torch.equal(none["depth"], full["depth"]) and torch.equal(none["aif"], full["aif"])


@pytest.mark.parametrize("shape", [(2, 1, 3, 3, 3, 3), (2, 1, 4, 10, 37, 76), (2, 1, 3, 17, 37, 70)], ids=["3x3", "37x76", "37x70"])
def test_head_two_equal_score_channels_are_one_channel(shape):
    one = fc.head_inputs(*shape, seed=5)
    two = dict(one, scores=one["scores"].repeat(1, 2, 1, 1, 1))
    a, b = _gpu_head(one, False), _gpu_head(two, False)
    for k in ("depth", "aif", "d_stack", "d_foc_dists"):
        assert torch.equal(a[k], b[k]), k
    assert torch.equal(a["d_scores"][:, 0], b["d_scores"][:, 0] + b["d_scores"][:, 1])


def test_head_aif_channels_are_read_in_place():
    t = fc.head_inputs(2, 2, 4, 5, 37, 76, seed=8)
    for Ca in (1, 2, 4):
        cut = dict(t, stack=t["stack"][:, :Ca].contiguous(), g_aif=torch.cat([t["g_aif"], t["g_depth"]], 1)[:, :Ca].contiguous())
        whole = _gpu_head(dict(t, g_aif=cut["g_aif"]), True, aif_channels=Ca)
        part = _gpu_head(cut, True, aif_channels=Ca)
        assert whole["aif"].shape == (2, Ca, 37, 76)
        for k in ("depth", "aif", "d_scores", "d_foc_dists"):
            assert torch.equal(whole[k], part[k]), (k, Ca)
        assert torch.equal(whole["d_stack"][:, :Ca], part["d_stack"]) and bool((whole["d_stack"][:, Ca:] == 0).all())


def test_head_offsets_past_2_to_the_31_elements():
    """scores and stack of 33 x 16 slices x 2048^2 = 2.2e9 elements each (8.9 GB): the last batch item starts at element 2^31, where a
    32-bit offset wraps.  Inputs are drawn on the device; the first and the last item must equal, bit for bit, what the same op
    gives for that item alone (whose offsets are small)."""
    N, S, H, W = 33, 16, 2048, 2048
    assert (N - 1) * S * H * W >= 2 ** 31 > (N - 2) * S * H * W
    g = torch.Generator(device=DEV).manual_seed(9)
    z = torch.randn(N, 1, S, H, W, device=DEV, generator=g).mul_(4.0).requires_grad_(True)
    x = torch.rand(N, 1, S, H, W, device=DEV, generator=g)
    u = torch.rand(N, S, device=DEV, generator=g).add_(0.5).requires_grad_(True)
    gd, ga = torch.randn(N, 1, H, W, device=DEV, generator=g), torch.randn(N, 1, H, W, device=DEV, generator=g)
    depth, aif = torch.ops.aadff.attention_depth(z, x, u, False, 1)
    torch.autograd.backward([depth, aif], [gd, ga])
    for n in (0, N - 1):
        z1, u1 = z[n:n + 1].detach().clone().requires_grad_(True), u[n:n + 1].detach().clone().requires_grad_(True)
        d1, a1 = torch.ops.aadff.attention_depth(z1, x[n:n + 1].clone(), u1, False, 1)
        torch.autograd.backward([d1, a1], [gd[n:n + 1].clone(), ga[n:n + 1].clone()])
        assert torch.equal(d1, depth[n:n + 1]) and torch.equal(a1, aif[n:n + 1]), n
        assert torch.equal(z1.grad, z.grad[n:n + 1]) and torch.equal(u1.grad, u.grad[n:n + 1]), n
    assert bool(torch.isfinite(depth).all()) and float(depth.min()) >= 0.5 - 1e-6 and float(depth.max()) <= 1.5 + 1e-6
    del z, x, depth, aif
    torch.cuda.empty_cache()


def test_head_public_function_devices_dtypes_and_module():
    shape = (2, 2, 4, 6, 37, 70)
    t = fc.head_inputs(*shape, seed=21)
    want = _gpu_head(t, True)
    # float64, non-contiguous inputs on the CPU: converted, results and gradients on the CPU, in the inputs' dtypes and layouts
    z = t["scores"].double().permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3).requires_grad_(True)
    x = t["stack"].double().permute(0, 1, 2, 4, 3).contiguous().permute(0, 1, 2, 4, 3).requires_grad_(True)
    u = t["foc_dists"].double().requires_grad_(True)
    assert not z.is_contiguous() and not x.is_contiguous()
    depth, aif = attention_depth(z, x, u, normalize_attention=True)
    assert depth.device.type == aif.device.type == "cpu" and depth.dtype == aif.dtype == torch.float32
    torch.autograd.backward([depth, aif], [t["g_depth"], t["g_aif"]])
    assert torch.equal(depth, want["depth"]) and torch.equal(aif, want["aif"])
    assert z.grad.dtype == torch.float64 and torch.equal(z.grad.float(), want["d_scores"]) and torch.equal(x.grad.float(), want["d_stack"])
    assert torch.equal(u.grad.float(), want["d_foc_dists"])
    # on the device, through the module, with [S] focus distances for N == 1
    head = AttentionHead(normalize_attention=True)
    d1, a1 = head(t["scores"][:1].to(DEV), t["stack"][:1].to(DEV), t["foc_dists"][0].to(DEV))
    assert d1.device == torch.device(DEV) and torch.equal(d1.cpu(), want["depth"][:1]) and torch.equal(a1.cpu(), want["aif"][:1])
    d4, a4 = attention_depth(t["scores"], t["stack"], t["foc_dists"], True, aif_channels=4)
    assert a4.shape == (2, 4, 37, 70) and torch.equal(a4[:, :3], want["aif"]) and torch.equal(d4, want["depth"])


# ------------------------------------------------------------------ the loss
_LOSS = {}


def _loss_case(shape, zero_gt=False):
    if (shape, zero_gt) not in _LOSS:
        H, W, gh, gw = shape
        _LOSS[(shape, zero_gt)] = fc.loss_inputs(2, 3, H, W, gh, gw, seed=40 + LOSS_SHAPES.index(shape), zero_gt=zero_gt)
    return _LOSS[(shape, zero_gt)]


def _gpu_sums(t, task, mask_range, cot):
    """The sums op on the tensors a task uses and the gradients of <cot, sums>."""
    use_d, use_a = task != "A_FS", task != "D_FS"
    none = torch.empty(0, device=DEV)
    d, a = t["depth"].to(DEV).requires_grad_(True), t["aif"].to(DEV).requires_grad_(True)
    rng = torch.stack((t["foc_dists"].min(), t["foc_dists"].max())).to(DEV) if mask_range and use_d else none
    sums = torch.ops.aadff.dff_loss_sums(d, a if use_a else none, t["gt_depth"].to(DEV) if use_d else none, t["gt_aif"].to(DEV) if use_a else none, rng)
    (sums * cot.to(DEV)).sum().backward()
    torch.cuda.synchronize()
    return sums.detach().cpu(), d.grad.cpu(), (torch.zeros_like(t["aif"]) if a.grad is None else a.grad.cpu())


@pytest.mark.parametrize("mask_range", [False, True], ids=["positive", "range"])
@pytest.mark.parametrize("task", ["D_FS", "A_FS", "DA_FS"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=LOSS_IDS)
def test_loss_sums_and_their_gradients(shape, task, mask_range, margin):
    t = _loss_case(shape)
    cot = torch.tensor([0.9, 0.0, 0.0, 0.6, 1.3, 0.8], dtype=torch.float64)        # the count and the mean square carry no gradient
    kw = dict(task=task, foc_dists=t["foc_dists"], mask_range=mask_range, sums_cotangent=cot)
    f64 = fc.loss_grads(t["depth"], t["aif"], t["gt_depth"], t["gt_aif"], dtype=torch.float64, **kw)
    f32 = fc.loss_grads(t["depth"], t["aif"], t["gt_depth"], t["gt_aif"], dtype=torch.float32, **kw)
    sums, d_depth, d_aif = _gpu_sums(t, task, mask_range, cot)
    again = _gpu_sums(t, task, mask_range, cot)
    assert torch.equal(sums, again[0]) and torch.equal(d_depth, again[1]) and torch.equal(d_aif, again[2])       # bit-equal from run to run
    assert sums.dtype == torch.float64 and d_depth.shape == t["depth"].shape and d_aif.shape == t["aif"].shape
    tag = f"dff loss {LOSS_IDS[LOSS_SHAPES.index(shape)]} {task} {'range' if mask_range else 'positive'}"
    _budget(margin, f"{tag} sums", sums, f64["sums"], f32["sums"])
    assert float(sums[1]) == float(f64["sums"][1])
    for k, roundings in ((0, 1), (2, 3), (3, 1)):
        # (1e-12: the float64 additions of both sides, at most 5180 terms of 2^-53 each)
        assert abs(float(sums[k]) - float(f64["sums"][k])) <= (roundings * U24 + 1e-12) * float(f64["sums"][k]), (k, sums, f64["sums"])
    _budget(margin, f"{tag} d_depth", d_depth, f64["d_depth"], f32["d_depth"])
    _budget(margin, f"{tag} d_aif", d_aif, f64["d_aif"], f32["d_aif"])
    gh, gw = shape[2:]
    assert not d_depth[:, :, gh:].any() and not d_depth[:, :, :, gw:].any()         # nothing outside the window
    if task != "D_FS":
        assert not d_aif[:, :, gh:].any() and not d_aif[:, :, :, gw:].any()


def _vector(d, keys):
    return torch.stack([d[k].detach().double().cpu() for k in keys])


def _check_dict(margin, tag, t, task, mask_range, zero_gt=False):
    kw = dict(task=task, foc_dists=t["foc_dists"], mask_range=mask_range, **WEIGHTS)
    f64 = fc.loss_grads(t["depth"], t["aif"], t["gt_depth"], t["gt_aif"], dtype=torch.float64, **kw)
    f32 = fc.loss_grads(t["depth"], t["aif"], t["gt_depth"], t["gt_aif"], dtype=torch.float32, **kw)
    runs = []
    for _ in range(2):
        d, a = t["depth"].to(DEV).requires_grad_(True), t["aif"].to(DEV).requires_grad_(True)
        out = dff_losses(d, a, t["gt_depth"].to(DEV), t["gt_aif"].to(DEV), **kw)
        out["total"].backward()
        torch.cuda.synchronize()
        runs.append((out, d.grad.cpu(), torch.zeros_like(t["aif"]) if a.grad is None else a.grad.cpu()))
    (out, d_depth, d_aif), (out2, d_depth2, d_aif2) = runs
    keys = list(f64["losses"])
    assert list(out) == keys and all(v.dim() == 0 and v.dtype == torch.float32 and v.device == torch.device(DEV) for v in out.values())
    assert "disp_MSE" not in out or not out["disp_MSE"].requires_grad
    got, want, w32 = _vector(out, keys), _vector(f64["losses"], keys), _vector(f32["losses"], keys)
    assert torch.equal(torch.isnan(got), torch.isnan(want)), (tag, out, f64["losses"])         # the oracle's nan pattern
    assert torch.equal(torch.isnan(_vector(out2, keys)), torch.isnan(got)) and torch.equal(d_depth, d_depth2) and torch.equal(d_aif, d_aif2)
    ok = ~torch.isnan(want)
    if bool(ok.any()):
        err, d32 = fc.rel_l2(got[ok], want[ok]), fc.rel_l2(w32[ok], want[ok])
        print(f"{tag} dict: error {err:.3e}, d32 {d32:.3e}")
        margin(f"{tag} dict", err, 4.0 * d32 + U24)
    assert bool(torch.isfinite(d_depth).all()) and bool(torch.isfinite(d_aif).all())
    _budget(margin, f"{tag} d_depth of total", d_depth, f64["d_depth"], f32["d_depth"])
    _budget(margin, f"{tag} d_aif of total", d_aif, f64["d_aif"], f32["d_aif"])
    return out


@pytest.mark.parametrize("mask_range", [False, True], ids=["positive", "range"])
@pytest.mark.parametrize("task", ["D_FS", "A_FS", "DA_FS"])
@pytest.mark.parametrize("shape", LOSS_SHAPES, ids=LOSS_IDS)
def test_loss_dict_and_gradients_of_total(shape, task, mask_range, margin):
    tag = f"dff_losses {LOSS_IDS[LOSS_SHAPES.index(shape)]} {task} {'range' if mask_range else 'positive'}"
    out = _check_dict(margin, tag, _loss_case(shape), task, mask_range)
    H, W, gh, gw = shape
    if task != "D_FS":                                        # an extent of 1 has no neighbour differences: the mean of nothing
        assert bool(torch.isnan(out["smooth"])) == (min(gh, gw) == 1)


@pytest.mark.parametrize("task", ["D_FS", "DA_FS"])
@pytest.mark.parametrize("shape", [LOSS_SHAPES[3], LOSS_SHAPES[5]], ids=[LOSS_IDS[3], LOSS_IDS[5]])
def test_loss_with_an_empty_mask(shape, task, margin):
    out = _check_dict(margin, f"dff_losses {LOSS_IDS[LOSS_SHAPES.index(shape)]} {task} all-zero gt", _loss_case(shape, zero_gt=True), task, False)
    assert bool(torch.isnan(out["depth"])) and bool(torch.isnan(out["total"]))


def test_loss_public_function_devices_dtypes_and_names():
    t = _loss_case(LOSS_SHAPES[6])
    kw = dict(task="DA_FS", foc_dists=t["foc_dists"], mask_range=True, pred_name="disp", **WEIGHTS)
    d, a = t["depth"].to(DEV).requires_grad_(True), t["aif"].to(DEV).requires_grad_(True)
    want = dff_losses(d, a, t["gt_depth"].to(DEV), t["gt_aif"].to(DEV), **kw)
    want["total"].backward()
    assert list(want) == ["disp", "AiF", "smooth", "total"]
    # float64, non-contiguous on the CPU
    dc = t["depth"].double().transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)
    ac = t["aif"].double().transpose(2, 3).contiguous().transpose(2, 3).requires_grad_(True)
    got = dff_losses(dc, ac, t["gt_depth"].double(), t["gt_aif"].double(), **kw)
    got["total"].backward()
    assert all(v.device.type == "cpu" and v.dtype == torch.float32 and torch.equal(v, want[k].cpu()) for k, v in got.items())
    assert dc.grad.dtype == torch.float64 and torch.equal(dc.grad.float(), d.grad.cpu()) and torch.equal(ac.grad.float(), a.grad.cpu())


def test_chain_head_then_loss(margin):
    """attention_depth -> dff_losses(...)['total'].backward() against the same chain of the oracle in float64.  gt_depth is the oracle's
    float64 prediction moved by +-(1e-3 + 0.1 rand), so no |e| is near zero; the stack lies in [0, 0.3) and gt_aif around 0.5 and 0.75, so
    no |aif - gt_aif| is either: no sign can differ between the arithmetics and no pixel is excluded."""
    shape = (2, 1, 3, 8, 37, 76)
    t = fc.head_inputs(*shape, seed=77)
    g = torch.Generator().manual_seed(78)
    stack = 0.3 * t["stack"]
    gt_aif = fc.smooth_image(2, 3, 37, 76, g)
    pred64, _ = fc.head(t["scores"].double(), stack.double(), t["foc_dists"].double())
    move = (1e-3 + 0.1 * torch.rand(pred64.shape, generator=g, dtype=torch.float64)) * torch.where(torch.rand(pred64.shape, generator=g) < 0.5, -1.0, 1.0)
    gt_depth = (pred64 + move).float()
    kw = dict(task="DA_FS", **WEIGHTS)

    def chain(dtype):
        z, x, u = (v.detach().to(dtype).requires_grad_(True) for v in (t["scores"], stack, t["foc_dists"]))
        depth, aif = fc.head(z, x, u)
        out = fc.losses(depth, aif, gt_depth.to(dtype), gt_aif.to(dtype), **kw)
        out["total"].backward()
        return {"total": out["total"].detach(), "d_scores": z.grad, "d_stack": x.grad, "d_foc_dists": u.grad}

    f64, f32 = chain(torch.float64), chain(torch.float32)
    assert float((pred64 - gt_depth.double()).abs().min()) > 5e-4
    z, x, u = (v.to(DEV).requires_grad_(True) for v in (t["scores"], stack, t["foc_dists"]))
    depth, aif = attention_depth(z, x, u)
    out = dff_losses(depth, aif, gt_depth.to(DEV), gt_aif.to(DEV), **kw)
    out["total"].backward()
    torch.cuda.synchronize()
    got = {"total": out["total"].detach().cpu(), "d_scores": z.grad.cpu(), "d_stack": x.grad.cpu(), "d_foc_dists": u.grad.cpu()}
    err, d32 = fc.rel_l2(got["total"], f64["total"]), fc.rel_l2(f32["total"], f64["total"])
    print(f"chain total: error {err:.3e}, d32 {d32:.3e}")
    margin("focus head chain total", err, 4.0 * d32 + U24)
    for k in ("d_scores", "d_stack", "d_foc_dists"):
        _budget(margin, f"focus head chain {k}", got[k], f64[k], f32[k])


def test_opcheck():
    t = fc.head_inputs(2, 2, 4, 3, 9, 12, seed=1)
    z, x, u = t["scores"].to(DEV), t["stack"].to(DEV), t["foc_dists"].to(DEV)
    gd, ga = t["g_depth"].to(DEV), t["g_aif"].to(DEV)
    utils = ("test_schema", "test_faketensor")
    for norm, Ca in ((False, 3), (True, 4), (True, 1)):
        torch.library.opcheck(torch.ops.aadff.attention_depth.default, (z, x, u, norm, Ca), test_utils=utils)
    for need in ((True, True, True), (False, True, False), (True, False, True)):
        torch.library.opcheck(torch.ops.aadff.attention_depth_bwd.default, (z, x, u, gd, ga, True, 3, *need), test_utils=utils)
    L = fc.loss_inputs(2, 3, 9, 12, 8, 10, seed=2)
    d, a, gtd, gta = (L[k].to(DEV) for k in ("depth", "aif", "gt_depth", "gt_aif"))
    none, rng = torch.empty(0, device=DEV), torch.tensor([0.8, 2.2], device=DEV)
    g = torch.ones(6, dtype=torch.float64, device=DEV)
    for args in ((d, a, gtd, gta, rng), (d, none, gtd, none, none), (d, a, none, gta, none)):
        torch.library.opcheck(torch.ops.aadff.dff_loss_sums.default, args, test_utils=utils)
        torch.library.opcheck(torch.ops.aadff.dff_loss_bwd.default, (*args, g, True, args[1].numel() > 0), test_utils=utils)
