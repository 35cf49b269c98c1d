"""The differentiable depth head and its loss (aadff/focus_head.py, csrc/focus_head.hip) restated in torch from their specification
(DESIGN.md 4.11), with the seeded inputs the tests share.  Everything here runs on the CPU in the dtype of its inputs, float64 for
the reference and float32 for its own rounding distance, and is differentiable by autograd.  Not used by the package.

The head:  zd = scores[:, 0], za = scores[:, K-1];  pd = softmax_S(zd) or, normalised, softplus(zd) / sum_S softplus(zd);  pa likewise of
za, except that K == 1 with normalisation keeps pa = softmax_S(za);  depth = sum_s pd_s foc_dists[n, s];  aif = sum_s pa_s stack[n, :Ca, s].
The loss:  over the common top-left window of the tensors a task uses - masked mean |depth - gt|, masked mean square (no gradient),
mean |aif - gt_aif|, smooth = (mean(wx r(d_gx)) + mean(wy r(d_gy))) / 2 with differences along H / W, w = exp(-mean_c (150 g)^2) of gt_aif and
r(x) = sqrt(x^2 + 1e-6)."""
import torch
import torch.nn.functional as F

EXTREMES = (80.0, -80.0, 1e4, -1e4)


def _attention(z, soft):
    if soft:
        sp = F.softplus(z)                                    # beta 1, threshold 20
        return sp / sp.sum(dim=1, keepdim=True)
    return torch.softmax(z, dim=1)


def head(scores, stack, foc_dists, normalize_attention=False, aif_channels=None):
    """scores [N,K,S,H,W], stack [N,Ct,S,H,W], foc_dists [N,S] -> depth [N,1,H,W], aif [N,Ca,H,W]."""
    N, K, S, H, W = scores.shape
    Ca = min(stack.shape[1], 3) if aif_channels is None else aif_channels
    pd = _attention(scores[:, 0], normalize_attention)
    pa = _attention(scores[:, K - 1], normalize_attention and K == 2)
    depth = (pd * foc_dists.reshape(N, S, 1, 1)).sum(dim=1, keepdim=True)
    aif = (pa[:, None] * stack[:, :Ca]).sum(dim=2)
    return depth, aif


def head_grads(scores, stack, foc_dists, g_depth, g_aif, normalize_attention=False, aif_channels=None, dtype=torch.float64):
    """Forward and the gradients of <g_depth, depth> + <g_aif, aif> in `dtype`: depth, aif, d_scores, d_stack, d_foc_dists."""
    z, x, u = (t.detach().to(dtype).requires_grad_(True) for t in (scores, stack, foc_dists))
    depth, aif = head(z, x, u, normalize_attention, aif_channels)
    ((depth * g_depth.to(dtype)).sum() + (aif * g_aif.to(dtype)).sum()).backward()
    return {"depth": depth.detach(), "aif": aif.detach(), "d_scores": z.grad, "d_stack": x.grad, "d_foc_dists": u.grad}


def _window(tensors):
    h, w = min(t.shape[2] for t in tensors), min(t.shape[3] for t in tensors)
    return [t[:, :, :h, :w] for t in tensors]


def _mask(gt, foc_dists, mask_range):
    if mask_range:
        fd = foc_dists.to(gt.dtype)
        return (gt >= fd.min()) & (gt <= fd.max())
    return gt > 0


def _smooth_terms(depth, gt_aif):
    """(wx r(d_gx), wy r(d_gy)): the two weighted maps whose means make the smoothness loss."""
    grads = lambda t: (t[:, :, 1:, :] - t[:, :, :-1, :], t[:, :, :, 1:] - t[:, :, :, :-1])      # noqa: E731
    r = lambda t: torch.sqrt(t * t + 1e-6)                                                        # noqa: E731
    (ix, iy), (dx, dy) = grads(gt_aif), grads(depth)
    wx = torch.exp(-((150.0 * ix) ** 2).mean(dim=1, keepdim=True))
    wy = torch.exp(-((150.0 * iy) ** 2).mean(dim=1, keepdim=True))
    return wx * r(dx), wy * r(dy)


def losses(depth, aif, gt_depth=None, gt_aif=None, task="D_FS", foc_dists=None, mask_range=False, disp_w=1.0, aif_w=0.0, smooth_w=0.0,
           pred_name="depth"):
    """The loss dict as a torch composition."""
    out = {}
    if task == "D_FS":
        depth, gt_depth = _window([depth, gt_depth])
        m = _mask(gt_depth, foc_dists, mask_range)
        out[pred_name] = (depth[m] - gt_depth[m]).abs().mean()
        out["disp_MSE"] = ((depth[m] - gt_depth[m]) ** 2).mean().detach()
        out["total"] = disp_w * out[pred_name]
    elif task == "A_FS":
        depth, aif, gt_aif = _window([depth, aif, gt_aif])
        out["AiF"] = (aif - gt_aif).abs().mean()
        tx, ty = _smooth_terms(depth, gt_aif)
        out["smooth"] = (tx.mean() + ty.mean()) / 2.0
        out["total"] = aif_w * out["AiF"] + smooth_w * out["smooth"]
    elif task == "DA_FS":
        depth, aif, gt_depth, gt_aif = _window([depth, aif, gt_depth, gt_aif])
        m = _mask(gt_depth, foc_dists, mask_range)
        out[pred_name] = (depth[m] - gt_depth[m]).abs().mean()
        out["AiF"] = (aif - gt_aif).abs().mean()
        tx, ty = _smooth_terms(depth, gt_aif)
        out["smooth"] = (tx.mean() + ty.mean()) / 2.0
        out["total"] = aif_w * out["AiF"] + disp_w * out[pred_name] + smooth_w * out["smooth"]
    else:
        raise NotImplementedError(task)
    return out


def loss_sums(depth, aif, gt_depth, gt_aif, task, foc_dists=None, mask_range=False):
    """The six sums the kernel reports, in the dtype of the inputs: sum_mask |e|, |mask|, sum_mask e^2, sum |aif - gt_aif|, sum wx r(d_gx),
    sum wy r(d_gy); zero where the task has no such term."""
    use_d, use_a = task in ("D_FS", "DA_FS"), task in ("A_FS", "DA_FS")
    used = _window([depth] + ([gt_depth] if use_d else []) + ([aif, gt_aif] if use_a else []))
    depth = used[0]
    s = [depth.new_zeros(()) for _ in range(6)]
    if use_d:
        gt = used[1]
        m = _mask(gt, foc_dists, mask_range)
        e = depth[m] - gt[m]
        s[0], s[1], s[2] = e.abs().sum(), m.sum().to(depth.dtype), (e * e).sum()
    if use_a:
        a, ga = used[-2], used[-1]
        tx, ty = _smooth_terms(depth, ga)
        s[3], s[4], s[5] = (a - ga).abs().sum(), tx.sum(), ty.sum()
    return torch.stack(s)


def loss_grads(depth, aif, gt_depth, gt_aif, dtype=torch.float64, sums_cotangent=None, **kw):
    """The dict, the sums and the gradients in `dtype`: d_depth and d_aif of 'total', or with `sums_cotangent` [6] of <cotangent, sums>."""
    d, a = (t.detach().to(dtype).requires_grad_(True) for t in (depth, aif))
    gd = None if gt_depth is None else gt_depth.to(dtype)
    ga = None if gt_aif is None else gt_aif.to(dtype)
    out = losses(d, a, gd, ga, **kw)
    sums = loss_sums(d, a, gd, ga, kw.get("task", "D_FS"), kw.get("foc_dists"), kw.get("mask_range", False))
    target = out["total"] if sums_cotangent is None else (sums * sums_cotangent.to(dtype)).sum()
    if target.requires_grad:
        target.backward()
    zero = lambda t: torch.zeros_like(t) if t.grad is None else t.grad      # noqa: E731
    return {"losses": {k: v.detach() for k, v in out.items()}, "sums": sums.detach(), "d_depth": zero(d), "d_aif": zero(a)}


def rel_l2(got, want):
    """|got - want| / |want| in float64 (0 for two zero tensors)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = float(want.norm())
    num = float((got - want).norm())
    return num / den if den > 0 else num


# ------------------------------------------------------------------ seeded inputs
def head_inputs(N, K, Ct, S, H, W, seed=0, extremes=True):
    """scores 4 * randn with a few entries at +-80 and +-1e4 (each on a pixel of its own, and only with S >= 2, so that no pixel's scores
    are all hugely negative: the normalised softplus of such a pixel is 0 / 0 in any arithmetic), stack uniform in [0, 1), focus distances
    unordered with both signs, and the two cotangents.  float32."""
    g = torch.Generator().manual_seed(seed)
    scores = 4.0 * torch.randn(N, K, S, H, W, generator=g)
    if extremes and S >= 2:
        pix = torch.randperm(N * H * W, generator=g)[:len(EXTREMES)]
        for i, p in enumerate(pix.tolist()):
            n, y, x = p // (H * W), (p // W) % H, p % W
            scores[n, int(torch.randint(K, (1,), generator=g)), int(torch.randint(S, (1,), generator=g)), y, x] = EXTREMES[i]
    stack = torch.rand(N, Ct, S, H, W, generator=g)
    foc = (0.3 + 2.7 * torch.rand(N, S, generator=g)) * torch.where(torch.rand(N, S, generator=g) < 0.25, -1.0, 1.0)
    Ca = min(Ct, 3)
    return {"scores": scores, "stack": stack, "foc_dists": foc, "g_depth": torch.randn(N, 1, H, W, generator=g),
            "g_aif": torch.randn(N, Ca, H, W, generator=g)}


def smooth_image(N, C, H, W, g):
    """An image whose neighbour differences are around 1 / 150, so that the edge weights spread over (0, 1), with one sharp step."""
    img = 0.5 + 0.004 * torch.randn(N, C, H, W, generator=g)
    img[:, :, H // 2:, W // 3:] += 0.25
    return img


def loss_inputs(N, Ca, H, W, gh=None, gw=None, seed=0, zero_gt=False):
    """depth and aif [N,.,H,W], gt_depth (about 10 % zeros, or all zeros) and gt_aif [N,.,gh,gw], and focus distances whose range holds about
    two thirds of gt_depth.  float32."""
    g = torch.Generator().manual_seed(seed)
    gh, gw = gh or H, gw or W
    depth = 0.5 + 2.0 * torch.rand(N, 1, H, W, generator=g)
    aif = torch.rand(N, Ca, H, W, generator=g)
    gt_depth = 0.5 + 2.0 * torch.rand(N, 1, gh, gw, generator=g)
    gt_depth[torch.rand(N, 1, gh, gw, generator=g) < 0.1] = 0.0
    if zero_gt:
        gt_depth.zero_()
    return {"depth": depth, "aif": aif, "gt_depth": gt_depth, "gt_aif": smooth_image(N, Ca, gh, gw, g),
            "foc_dists": torch.tensor([[0.9, 2.2, 1.4], [1.1, 0.8, 2.0]])[:N]}
