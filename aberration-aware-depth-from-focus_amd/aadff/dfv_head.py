"""Cost-volume depth head: what the reference's second network, DFVNet, puts between a decoder level's cost volume and
its loss (DFV_models/DFFNet.py:94-95, 102-115 with disparityregression of DFV_models/submodule.py:63-77).

    pred, std = cost_volume_depth(cost, foc_dists, size=(H, W))         # cost [B,S,h,w] at 1/4 ... 1/32 of the image
    preds, stds = cost_volume_depth_levels([cost3, cost4], foc_dists, (H, W))      # the training branch: one call per level

    up = F.interpolate(cost, [H, W], mode='bilinear');  p = softmax(up, 1);  pred = sum_s p_s foc_dists[b,s];
    std = sqrt(sum_s p_s (pred - foc_dists[b,s])^2), detached

as one fused HIP kernel with a HIP backward (csrc/dfv_head.hip, `torch.ops.aadff.dfv_regress`): the upsampled cost and the softmax
never exist at full resolution, and the gradient to the cost is gathered without atomics, so it is the same from run to run.  The
reference's trilinear call of levels 3 and 4 keeps the depth and is the same operation slice by slice.  The 3-D networks that produce
the costs are not part of this package.  There is no CPU fallback: without the HIP library or a GPU the functions raise
like the renderers.
"""
import operator

import numpy as np
import torch

from . import _abi, ops  # noqa: F401  (registers torch.ops.aadff.dfv_regress)


def _device_of(t):
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def cost_volume_depth(cost, foc_dists, size=None, return_prob=False):
    """cost [B,S,h,w] (or [B,1,S,h,w], the shape the reference gives its trilinear call), foc_dists [B,S] ([S] when B == 1), on any
    device and of any floating dtype -> (pred [B,1,H,W], std [B,1,H,W]) and with return_prob also prob [B,S,H,W], in float32 on the
    device of `cost`.  size = (H, W) with H >= h and W >= w, any ratio; None means (h, w).  Gradients flow through pred to cost and
    foc_dists; std and prob carry none, as in the reference.  The focus distances may have any values in any order."""
    if not torch.is_tensor(cost) or cost.dim() not in (4, 5):
        raise ValueError("cost_volume_depth: cost must be [B,S,h,w] or [B,1,S,h,w]")
    if cost.dim() == 5:
        if cost.shape[1] != 1:
            raise ValueError(f"cost_volume_depth: a 5-D cost must be [B,1,S,h,w], got {tuple(cost.shape)}")
        cost = cost.squeeze(1)
    B, S, h, w = cost.shape
    if S == 0:
        raise ValueError("cost_volume_depth: the cost has no slices")
    fd = foc_dists if torch.is_tensor(foc_dists) else torch.as_tensor(foc_dists, dtype=torch.float32)
    if fd.dim() == 1 and B == 1:
        fd = fd.reshape(1, -1)
    if fd.dim() != 2 or tuple(fd.shape) != (B, S):            # a cost depth other than S would need resampling along S: out of scope
        raise ValueError(f"cost_volume_depth: foc_dists has shape {tuple(fd.shape)}, expected [{B},{S}]" + (f" or [{S}]" if B == 1 else ""))
    if size is None:
        H, W = h, w
    else:
        try:                                                  # any integer type (numpy's too); floats and bools are refused
            if isinstance(size, (str, bytes)) or any(isinstance(v, (bool, np.bool_)) for v in size):
                raise TypeError
            H, W = (operator.index(v) for v in size)
        except (TypeError, ValueError):
            raise ValueError(f"cost_volume_depth: size {size!r} is not a pair of integers (H, W)") from None
    if H < h or W < w:
        raise ValueError(f"cost_volume_depth: size {H} x {W} is smaller than the cost {h} x {w}: shrinking is not supported")
    if h * w == 0 and H * W != 0:
        raise ValueError(f"cost_volume_depth: a cost of {h} x {w} cannot be upsampled to {H} x {W}")
    src = cost.device
    if B == 0 or H * W == 0:
        zero = (cost.sum() + fd.sum()).to(torch.float32) * 0                                 # keeps the graph connected
        out = (zero.expand(B, 1, H, W).clone(), zero.detach().expand(B, 1, H, W).clone())
        return out + (zero.detach().expand(B, S, H, W).clone(),) if return_prob else out
    _abi.require_gpu()
    dev = _device_of(cost)
    pred, std, prob = torch.ops.aadff.dfv_regress(_abi.f32c(cost, dev), _abi.f32c(fd, dev), H, W, bool(return_prob))
    return (pred.to(src), std.to(src), prob.to(src)) if return_prob else (pred.to(src), std.to(src))


class CostVolumeHead(torch.nn.Module):
    """cost_volume_depth as a module: forward(cost, foc_dists) -> (pred, std[, prob])."""

    def __init__(self, size=None, return_prob=False):
        super().__init__()
        self.size = size
        self.return_prob = bool(return_prob)

    def forward(self, cost, foc_dists):
        return cost_volume_depth(cost, foc_dists, self.size, self.return_prob)

    def extra_repr(self):
        return f"size={self.size}, return_prob={self.return_prob}"


def cost_volume_depth_levels(costs, foc_dists, size):
    """One cost_volume_depth per level of `costs` (a list of [B,S,h_l,w_l], finest first) at the same `size` -> (preds, stds), two lists,
    as the training branch of the reference's DFVNet.forward returns them."""
    if not isinstance(costs, (list, tuple)) or len(costs) == 0:
        raise ValueError("cost_volume_depth_levels: costs must be a non-empty list of cost volumes")
    preds, stds = [], []
    for c in costs:
        p, s = cost_volume_depth(c, foc_dists, size)
        preds.append(p)
        stds.append(s)
    return preds, stds
