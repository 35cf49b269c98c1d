"""Confidence-guided depth refinement: the step after the estimator.  Every depth head of this package returns a depth
map and a per-pixel confidence (depth_from_stack its `peak`, cost_volume_depth its `std`); this module uses the confidence: textureless
pixels, where the focus measure is flat and the argmax is noise, are filled from confident neighbours, and the guide (the all-in-focus
image) keeps depth from being smeared across object edges.

    est = depth_from_stack(stack, foc_dists)
    ref = refine_depth(est.depth, confidence_from_peak(est.peak), est.aif)       # RefinedDepth(depth, confidence)

One iteration is a confidence-weighted joint (cross) bilateral filter,

    w(p,q) = exp(-(|p - q|^2 / (2 sigma_space^2) + |g(p) - g(q)|^2 / (2 sigma_range^2 C))) over the (2 radius + 1)^2 window, clipped,
    u'(p) = sum w c(q) u(q) / sum w c(q)   (u(p) itself where every confidence of the window is zero),   c'(p) = sum w c(q) / sum w,

as one fused HIP kernel with a two-pass gather backward to u and c (csrc/depth_refine.hip, `torch.ops.aadff.depth_refine`): no shifted
temporaries, no atomics, the same bits from run to run.  The confidence diffuses with the depth, so a later iteration reaches what an
earlier one could not.  The guide is a constant.  There is no CPU fallback: without the HIP library or a GPU the functions raise like
the renderers.
"""
import math
import operator
from collections import namedtuple

import torch

from . import _abi, ops  # noqa: F401  (registers torch.ops.aadff.depth_refine)

RefinedDepth = namedtuple("RefinedDepth", ["depth", "confidence"])
SPACES = ("inverse", "linear")
MAX_RADIUS, MAX_CHANNELS = 8, 4


def _device_of(t):
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _positive(who, name, v):
    try:
        v = float(v)
    except (TypeError, ValueError):
        raise ValueError(f"{who}: {name} = {v!r} is not a number") from None
    if not (v > 0.0 and math.isfinite(v)):
        raise ValueError(f"{who}: {name} = {v!r} must be a positive number")
    return v


def _parameters(who, radius, sigma_space, sigma_range, iterations, space):
    try:
        if isinstance(radius, bool) or isinstance(iterations, bool):
            raise TypeError
        radius, iterations = operator.index(radius), operator.index(iterations)
    except TypeError:
        raise ValueError(f"{who}: radius {radius!r} and iterations {iterations!r} must be integers") from None
    if not 1 <= radius <= MAX_RADIUS:
        raise ValueError(f"{who}: radius = {radius} is not in 1..{MAX_RADIUS}")
    if iterations < 0:
        raise ValueError(f"{who}: iterations = {iterations} is negative")
    if space not in SPACES:
        raise ValueError(f"{who}: space {space!r} is not one of {SPACES}")
    sigma_space = radius / 2.0 if sigma_space is None else _positive(who, "sigma_space", sigma_space)
    return radius, sigma_space, _positive(who, "sigma_range", sigma_range), iterations


def refine_depth(depth, confidence, guide, radius=4, sigma_space=None, sigma_range=0.1, iterations=2, space="inverse"):
    """depth, confidence [N,1,H,W], guide [N,C,H,W] with C in 1..4, on any device and of any floating dtype -> RefinedDepth(depth,
    confidence), float32 on the device of `depth`.  confidence >= 0 (a value below 2^-30 counts as 0); where it is 0 the depth may be
    anything, nan included.  radius in 1..8, sigma_space defaults to radius / 2; sigma_range is in the guide's units.  space "inverse"
    filters 1 / depth and returns 1 / u' (depth_from_stack fits there; depths of either sign), "linear" filters depth itself.
    `iterations` passes, each differentiable with respect to depth and confidence; the guide is detached."""
    who = "refine_depth"
    radius, sigma_space, sigma_range, iterations = _parameters(who, radius, sigma_space, sigma_range, iterations, space)
    for name, t in (("depth", depth), ("confidence", confidence), ("guide", guide)):
        if not torch.is_tensor(t) or t.dim() != 4 or not t.is_floating_point():
            raise ValueError(f"{who}: {name} must be a floating-point tensor [N,{'C' if name == 'guide' else '1'},H,W]")
    N, Cn, H, W = guide.shape
    if not 1 <= Cn <= MAX_CHANNELS:
        raise ValueError(f"{who}: the guide has {Cn} channels, 1 to {MAX_CHANNELS} are supported")
    if tuple(depth.shape) != (N, 1, H, W) or tuple(confidence.shape) != (N, 1, H, W):
        raise ValueError(f"{who}: depth {tuple(depth.shape)} and confidence {tuple(confidence.shape)} must both be {(N, 1, H, W)}, "
                         f"the guide is {tuple(guide.shape)}")
    src = depth.device
    if N * H * W == 0:
        zero = ((depth.sum() + confidence.sum()) * 0).to(torch.float32)                         # keeps the graph connected
        return RefinedDepth(zero.expand(N, 1, H, W).clone(), zero.expand(N, 1, H, W).clone())
    conf_d = confidence.detach()
    if bool((conf_d < 0).any()) or bool(torch.isnan(conf_d).any()):
        raise ValueError(f"{who}: the confidence must be >= 0 everywhere")
    if space == "inverse" and bool(((depth.detach() == 0) & (conf_d > 0)).any()):
        raise ValueError(f"{who}: a depth of 0 at a pixel with non-zero confidence has no inverse")
    _abi.require_gpu()
    dev = _device_of(depth)
    u, c, g = _abi.f32c(depth, dev), _abi.f32c(confidence, dev), _abi.f32c(guide.detach(), dev)
    if space == "inverse":
        u = 1.0 / u                                           # (1 / 0 under a zero confidence is an inf no pixel reads)
    for _ in range(iterations):
        u, c = torch.ops.aadff.depth_refine(u, c, g, radius, sigma_space, sigma_range)
    if space == "inverse":
        u = 1.0 / u
    return RefinedDepth(u.to(src), c.to(src))


def _per_image(who, name, value, like):
    """A scalar or one value per image as [N,1,1,1] on the device of `like`; None when the caller did not give one."""
    if value is None:
        return None
    v = torch.as_tensor(value, dtype=like.dtype, device=like.device)
    if v.dim() > 1 or (v.dim() == 1 and v.shape[0] != like.shape[0]):
        raise ValueError(f"{who}: {name} must be a scalar or one value per image, got shape {tuple(v.shape)}")
    if bool((v < 0).any()) or not bool(torch.isfinite(v).all()):
        raise ValueError(f"{who}: {name} must be finite and >= 0")
    return v.reshape(-1, 1, 1, 1)


def _median(t):
    return t.detach().flatten(1).median(1).values.reshape(-1, 1, 1, 1)


def confidence_from_peak(peak, tau=None):
    """peak [N,1,H,W] >= 0 (depth_from_stack's peak focus measure) -> peak / (peak + tau) in [0, 1).  tau: a scalar or one value per
    image, by default the median of each image; where it is 0 the result is (peak > 0) as 0 / 1."""
    who = "confidence_from_peak"
    if not torch.is_tensor(peak) or peak.dim() != 4 or not peak.is_floating_point():
        raise ValueError(f"{who}: peak must be a floating-point tensor [N,1,H,W]")
    if peak.numel() == 0:
        return peak.clone()
    if bool((peak.detach() < 0).any()):
        raise ValueError(f"{who}: the peak must be >= 0 everywhere")
    tau = _per_image(who, "tau", tau, peak)
    tau = _median(peak) if tau is None else tau
    return torch.where(tau > 0, peak / (peak + tau).clamp_min(torch.finfo(peak.dtype).tiny), (peak > 0).to(peak.dtype))


def confidence_from_std(std, scale=None):
    """std [N,1,H,W] >= 0 (cost_volume_depth's standard deviation) -> 1 / (1 + (std / scale)^2) in (0, 1].  scale: a positive scalar or
    one value per image, by default the median of each image."""
    who = "confidence_from_std"
    if not torch.is_tensor(std) or std.dim() != 4 or not std.is_floating_point():
        raise ValueError(f"{who}: std must be a floating-point tensor [N,1,H,W]")
    if std.numel() == 0:
        return std.clone()
    if bool((std.detach() < 0).any()):
        raise ValueError(f"{who}: the std must be >= 0 everywhere")
    scale = _per_image(who, "scale", scale, std)
    scale = _median(std) if scale is None else scale
    if bool((scale == 0).any()):
        raise ValueError(f"{who}: a scale of 0 (the median of an image whose std is 0 on half of its pixels?) - give a positive scale")
    return 1.0 / (1.0 + (std / scale) ** 2)


class DepthRefiner(torch.nn.Module):
    """refine_depth as a module, for use behind AttentionHead / CostVolumeHead: forward(depth, confidence, guide) -> RefinedDepth."""

    def __init__(self, radius=4, sigma_space=None, sigma_range=0.1, iterations=2, space="inverse"):
        super().__init__()
        _parameters("DepthRefiner", radius, sigma_space, sigma_range, iterations, space)
        self.radius, self.sigma_space, self.sigma_range, self.iterations, self.space = radius, sigma_space, sigma_range, iterations, space

    def forward(self, depth, confidence, guide):
        return refine_depth(depth, confidence, guide, self.radius, self.sigma_space, self.sigma_range, self.iterations, self.space)

    def extra_repr(self):
        return (f"radius={self.radius}, sigma_space={self.sigma_space}, sigma_range={self.sigma_range}, iterations={self.iterations}, "
                f"space={self.space!r}")
