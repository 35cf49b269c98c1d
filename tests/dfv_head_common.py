"""The cost-volume depth head (aadff/dfv_head.py, csrc/dfv_head.hip) restated in torch from its specification, with the
seeded inputs the tests share.  Everything here runs on the CPU in the dtype of its inputs, float64 for the reference and float32 for
its own rounding distance, and is differentiable by autograd.  Not used by the package.

    up = F.interpolate(cost, [H, W], mode='bilinear');  p = softmax(up, 1);  pred = sum_s p_s foc_dists[b, s];
    std = sqrt(sum_s p_s (pred - foc_dists[b, s])^2) under no_grad

which is DFV_models/DFFNet.py:94-95 with disparityregression(1) of DFV_models/submodule.py:63-77 of the reference."""
import torch
import torch.nn.functional as F

EXTREMES = (80.0, -80.0, 1e4, -1e4)


def head(cost, foc_dists, size):
    """cost [B,S,h,w], foc_dists [B,S], size (H, W) -> pred [B,1,H,W], std [B,1,H,W] (detached), prob [B,S,H,W]."""
    B, S = cost.shape[:2]
    up = F.interpolate(cost, list(size), mode="bilinear")
    p = F.softmax(up, 1)
    disp = foc_dists.reshape(B, S, 1, 1)
    pred = torch.sum(p * disp, 1, keepdim=True)
    with torch.no_grad():
        std = torch.sqrt(torch.sum(p * (pred - disp) ** 2, 1, keepdim=True))
    return pred, std.detach(), p


def head_grads(cost, foc_dists, g_pred, size, dtype=torch.float64):
    """Forward and the gradients of <g_pred, pred> in `dtype`: pred, std, prob, d_cost, d_foc_dists."""
    c, u = (t.detach().to(dtype).requires_grad_(True) for t in (cost, foc_dists))
    pred, std, prob = head(c, u, size)
    (pred * g_pred.to(dtype)).sum().backward()
    return {"pred": pred.detach(), "std": std, "prob": prob.detach(), "d_cost": c.grad, "d_foc_dists": u.grad}


def rel_l2(got, want):
    """|got - want| / |want| in float64 (0 for two zero tensors)."""
    got, want = got.detach().double().cpu(), want.detach().double().cpu()
    den = float(want.norm())
    num = float((got - want).norm())
    return num / den if den > 0 else num


# ------------------------------------------------------------------ seeded inputs
def head_inputs(B, S, h, w, H, W, seed=0, extremes=False):
    """cost 2 * randn (spanning about +-6), with `extremes` four cells of different slices at +-80 and +-1e4 (only with S >= 2 and at
    least four cells), focus distances unordered with both signs, and the cotangent of pred.  float32."""
    g = torch.Generator().manual_seed(seed)
    cost = 2.0 * torch.randn(B, S, h, w, generator=g)
    if extremes and S >= 2 and B * h * w >= len(EXTREMES):
        cells = torch.randperm(B * h * w, generator=g)[:len(EXTREMES)]
        for i, p in enumerate(cells.tolist()):
            cost[p // (h * w), int(torch.randint(S, (1,), generator=g)), (p // w) % h, p % w] = EXTREMES[i]
    foc = (0.3 + 2.7 * torch.rand(B, S, generator=g)) * torch.where(torch.rand(B, S, generator=g) < 0.25, -1.0, 1.0)
    return {"cost": cost, "foc_dists": foc, "g_pred": torch.randn(B, 1, H, W, generator=g), "size": (H, W)}
