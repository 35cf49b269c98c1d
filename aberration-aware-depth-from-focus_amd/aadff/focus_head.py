"""Differentiable depth head over a focal stack and its loss: what the reference's training script puts between a
stack and its loss - stage 2 ("attention") of AiFDepthNet.fit and AiFDepthNet.compute_loss (dff/AiFNet.py:376-434, 450-584).

    depth, aif = attention_depth(scores, stack, foc_dists)             # soft-argmax over the slices, attention-weighted composite
    losses = dff_losses(depth, aif, gt_depth, gt_aif, task="DA_FS")    # the reference's dict: masked L1, MSE, AiF L1, smoothness

Both are fused HIP kernels with HIP backward passes (csrc/focus_head.hip, `torch.ops.aadff.attention_depth`,
`torch.ops.aadff.dff_loss_sums`), so the chain render -> estimate -> loss -> gradient stays on the GPU: scores may come from a network or,
for instance, as beta * log(focus volume) from aadff.dfocus.depth_from_stack(return_volume=True) (examples/soft_depth_from_focus.py).
The 3-D network of the reference itself is not part of this package.  There is no CPU fallback: without the HIP library
or a GPU the functions raise like the renderers.
"""
import torch

from . import _abi, ops  # noqa: F401  (registers torch.ops.aadff.attention_depth / dff_loss_sums)

TASKS = ("D_FS", "A_FS", "DA_FS")


def _device_of(t):
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def attention_depth(scores, stack, foc_dists, normalize_attention=False, aif_channels=None):
    """scores [N,K,S,H,W] (K 1 or 2), stack [N,Ct,S,H,W] (Ct in 1..4), foc_dists [N,S] ([S] when N == 1), on any device and of any
    floating dtype -> (depth [N,1,H,W], aif [N,Ca,H,W]) in float32 on the device of `scores`, with gradients to all three inputs.

    zd = scores[:, 0], za = scores[:, K-1].  normalize_attention False: pd = softmax_S(zd), pa = softmax_S(za).  True:
    pd = softplus(zd) / sum_S softplus(zd), and pa likewise of za for K == 2 but softmax_S(za) for K == 1 (as the reference has it).
    depth = sum_s pd_s foc_dists[n,s]; aif = sum_s pa_s stack[n,c,s] over the first Ca = aif_channels channels (default min(Ct, 3), the
    reference's x[:, :3]), read in place.  The focus distances may have any values in any order."""
    if not torch.is_tensor(scores) or scores.dim() != 5:
        raise ValueError("attention_depth: scores must be [N,K,S,H,W]")
    if not torch.is_tensor(stack) or stack.dim() != 5:
        raise ValueError("attention_depth: stack must be [N,Ct,S,H,W]")
    N, K, S, H, W = scores.shape
    if K not in (1, 2):
        raise ValueError(f"attention_depth: scores has K = {K} channels, expected 1 or 2")
    Ct = stack.shape[1]
    if not 1 <= Ct <= 4:
        raise ValueError(f"attention_depth: stack has Ct = {Ct} channels, expected 1..4")
    if (stack.shape[0], *stack.shape[2:]) != (N, S, H, W):
        raise ValueError(f"attention_depth: stack {tuple(stack.shape)} does not match scores {tuple(scores.shape)} in N, S, H, W")
    Ca = min(Ct, 3) if aif_channels is None else aif_channels
    if not isinstance(Ca, int) or not 1 <= Ca <= Ct:
        raise ValueError(f"attention_depth: aif_channels {aif_channels!r} is outside 1..Ct = {Ct}")
    if S == 0:
        raise ValueError("attention_depth: the stack has no slices")
    fd = foc_dists if torch.is_tensor(foc_dists) else torch.as_tensor(foc_dists, dtype=torch.float32)
    if fd.dim() == 1 and N == 1:
        fd = fd.reshape(1, -1)
    if fd.dim() != 2 or tuple(fd.shape) != (N, S):
        raise ValueError(f"attention_depth: foc_dists has shape {tuple(fd.shape)}, expected [{N},{S}]" + (f" or [{S}]" if N == 1 else ""))
    src = scores.device
    if N == 0 or H * W == 0:
        zero = (scores.sum() + stack.sum() + fd.sum()).to(torch.float32) * 0                 # keeps the graph connected
        return zero.expand(N, 1, H, W).clone(), zero.expand(N, Ca, H, W).clone()
    _abi.require_gpu()
    dev = _device_of(scores)
    depth, aif = torch.ops.aadff.attention_depth(_abi.f32c(scores, dev), _abi.f32c(stack, dev), _abi.f32c(fd, dev), bool(normalize_attention), Ca)
    return depth.to(src), aif.to(src)


class AttentionHead(torch.nn.Module):
    """attention_depth as a module: forward(scores, stack, foc_dists) -> (depth, aif)."""

    def __init__(self, normalize_attention=False, aif_channels=None):
        super().__init__()
        self.normalize_attention = bool(normalize_attention)
        self.aif_channels = aif_channels

    def forward(self, scores, stack, foc_dists):
        return attention_depth(scores, stack, foc_dists, self.normalize_attention, self.aif_channels)

    def extra_repr(self):
        return f"normalize_attention={self.normalize_attention}, aif_channels={self.aif_channels}"


def _map4(name, t, channels=None):
    if not torch.is_tensor(t) or t.dim() != 4 or (channels is not None and t.shape[1] != channels):
        raise ValueError(f"dff_losses: {name} must be [N,{'C' if channels is None else channels},H,W]")
    return t


def dff_losses(depth, aif, gt_depth=None, gt_aif=None, task="D_FS", foc_dists=None, mask_range=False, disp_w=1.0, aif_w=0.0, smooth_w=0.0,
               pred_name="depth"):
    """The reference's loss dict of 0-dim float32 tensors on the device of `depth`, with gradients to depth [N,1,H,W] and aif [N,Ca,H,W].

    task "D_FS":  {pred_name: mean_mask |depth - gt_depth|, 'disp_MSE': mean_mask (depth - gt_depth)^2 (no gradient), 'total'}
         "A_FS":  {'AiF': mean |aif - gt_aif|, 'smooth', 'total'}        "DA_FS": {pred_name, 'AiF', 'smooth', 'total'}
    mask = gt_depth > 0, or min(foc_dists) <= gt_depth <= max(foc_dists) with mask_range.  smooth = (mean(wx r(d_gx)) + mean(wy r(d_gy))) / 2
    with gx / gy the stride-1 differences along H / W, w = exp(-mean_c (150 g)^2) of gt_aif and r(x) = sqrt(x^2 + 1e-6).  total =
    disp_w * depth term + aif_w * AiF + smooth_w * smooth, as far as the task has them.  The tensors a task uses are cropped to their
    common top-left window; gradients outside it are zero.  An empty mask or an extent of 1 gives nan in the means concerned, as
    the torch composition does, and no gradient from them."""
    if task not in TASKS:
        raise NotImplementedError(f"dff_losses: task {task!r} is not one of {TASKS}")
    use_d, use_a = task in ("D_FS", "DA_FS"), task in ("A_FS", "DA_FS")
    _map4("depth", depth, 1)
    N = depth.shape[0]
    if use_d:
        if gt_depth is None:
            raise ValueError(f"dff_losses: task {task} needs gt_depth")
        _map4("gt_depth", gt_depth, 1)
    if use_a:
        if gt_aif is None:
            raise ValueError(f"dff_losses: task {task} needs gt_aif")
        _map4("aif", aif)
        _map4("gt_aif", gt_aif, aif.shape[1])
        if not 1 <= aif.shape[1] <= 4:
            raise ValueError(f"dff_losses: aif has {aif.shape[1]} channels, expected 1..4")
    used = [depth] + ([gt_depth] if use_d else []) + ([aif, gt_aif] if use_a else [])
    if any(t.shape[0] != N for t in used):
        raise ValueError("dff_losses: the batch sizes differ")
    if mask_range and use_d and foc_dists is None:
        raise ValueError("dff_losses: mask_range needs foc_dists")
    src = depth.device
    h, w = min(t.shape[2] for t in used), min(t.shape[3] for t in used)
    if N * h * w == 0:                                        # every mean is over nothing
        nan = (depth.sum() + (aif.sum() if use_a else 0)).to(torch.float32) * float("nan")
        keys = {"D_FS": (pred_name, "disp_MSE", "total"), "A_FS": ("AiF", "smooth", "total"), "DA_FS": (pred_name, "AiF", "smooth", "total")}[task]
        return {k: (nan.detach() if k == "disp_MSE" else nan) for k in keys}
    _abi.require_gpu()
    dev = _device_of(depth)
    none = torch.empty((0,), dtype=torch.float32, device=dev)
    rng = none
    if mask_range and use_d:
        fd = torch.as_tensor(foc_dists).detach().to(device=dev, dtype=torch.float32)
        rng = torch.stack((fd.min(), fd.max()))
    sums = torch.ops.aadff.dff_loss_sums(_abi.f32c(depth, dev), _abi.f32c(aif, dev) if use_a else none,
                                         _abi.f32c(gt_depth.detach(), dev) if use_d else none, _abi.f32c(gt_aif.detach(), dev) if use_a else none, rng)
    out, total = {}, 0.0
    if use_d:
        out[pred_name] = sums[0] / sums[1]
        total = total + disp_w * out[pred_name]
        if task == "D_FS":
            out["disp_MSE"] = (sums[2] / sums[1]).detach()
    if use_a:
        Ca = aif.shape[1]
        out["AiF"] = sums[3] / float(N * Ca * h * w)
        nx, ny = float(N * (h - 1) * w), float(N * h * (w - 1))                # 0 for an extent of 1: 0 / 0 = nan, like the mean of nothing
        out["smooth"] = (sums[4] / nx + sums[5] / ny) / 2.0
        total = aif_w * out["AiF"] + total + smooth_w * out["smooth"]
    out["total"] = total
    return {k: v.to(device=src, dtype=torch.float32) for k, v in out.items()}
