"""Depth from a focal stack, the classical estimator: the counterpart of the stack renderers.

    depth, index, peak, aif, volume = depth_from_stack(stack, foc_dists)

Per slice the modified Laplacian of the gray image summed over a window, the first argmax over the slices and a three-point peak fit
on the slice abscissae - one fused HIP launch that reads the stack once (csrc/dfocus.hip, `torch.ops.aadff.depth_from_stack`).  It needs
no network and no lens model, so it serves as a baseline and as the initialiser of an analysis-by-synthesis fit through
aadff.diffrender (examples/depth_from_focus_classic.py).  No gradients: the argmax has none (aadff.focus_head is the soft, differentiable
counterpart).  There is no CPU fallback: without the HIP
library or a GPU it raises like the renderers.
"""
from collections import namedtuple

import torch

from . import _abi, ops  # noqa: F401  (registers torch.ops.aadff.depth_from_stack)

DepthFromStack = namedtuple("DepthFromStack", ["depth", "index", "peak", "aif", "volume"])

WINDOWS = (1, 3, 5, 7, 9)
INTERPS = tuple(_abi.DFOCUS_INTERP)
SPACES = ("inverse", "linear")


def slice_coords(foc_dists, N, S, space):
    """Focus distances -> the float32 abscissae [N,S] of the fit on the CPU (`inverse`: 1 / foc_dist), checked."""
    fd = torch.as_tensor(foc_dists).detach().to(device="cpu", dtype=torch.float32)
    if fd.dim() == 1 and N == 1:
        fd = fd.reshape(1, -1)
    if fd.dim() != 2 or tuple(fd.shape) != (N, S):
        raise ValueError(f"depth_from_stack: foc_dists has shape {tuple(fd.shape)}, expected [{N},{S}]" + (f" or [{S}]" if N == 1 else ""))
    if space == "inverse":
        if bool((fd == 0).any()):
            raise ValueError("depth_from_stack: a focus distance is zero (space='inverse' fits in 1 / foc_dist)")
        fd = 1.0 / fd
    step = fd[:, 1:] - fd[:, :-1]
    if not bool(((step > 0).all(dim=1) | (step < 0).all(dim=1)).all()):
        raise ValueError("depth_from_stack: the slice coordinates of a row are not strictly monotone")
    return fd.contiguous()


@torch.no_grad()
def depth_from_stack(stack, foc_dists, window=9, interp="gaussian", space="inverse", eps=1e-8, return_volume=False):
    """stack [N,C,S,H,W] (C in 1..4) and its focus distances foc_dists [N,S] ([S] when N == 1), on any device ->
    DepthFromStack(depth [N,1,H,W], index [N,1,H,W] int32, peak [N,1,H,W], aif [N,C,H,W], volume [N,S,H,W] or empty).

    window  side of the square over which the modified Laplacian is summed: 1, 3, 5, 7 or 9
    interp  "none": depth of the sharpest slice; "parabola" / "gaussian": vertex of the parabola through the focus measure (its
            logarithm) at the sharpest slice and its two neighbours; the sharpest slice itself at either end of the stack
    space   "inverse": the fit runs in 1 / foc_dist, where defocus blur is nearly symmetric, and depth = 1 / u* keeps the sign
            convention of foc_dists; "linear": in foc_dists themselves
    peak    the focus measure at the sharpest slice: a confidence (low on textureless pixels)
    aif     every pixel copied from its sharpest slice: an all-in-focus composite
    The rows of foc_dists must be strictly monotone (either direction, any spacing)."""
    if not torch.is_tensor(stack) or stack.dim() != 5:
        raise ValueError("depth_from_stack: stack must be [N,C,S,H,W]")
    if window not in WINDOWS:
        raise ValueError(f"depth_from_stack: window {window!r} is not one of {WINDOWS}")
    if interp not in INTERPS:
        raise ValueError(f"depth_from_stack: interp {interp!r} is not one of {INTERPS}")
    if space not in SPACES:
        raise ValueError(f"depth_from_stack: space {space!r} is not one of {SPACES}")
    if not eps > 0:
        raise ValueError(f"depth_from_stack: eps {eps!r} is not positive")
    N, Cn, S, H, W = stack.shape
    if S == 0:
        raise ValueError("depth_from_stack: the stack has no slices")
    coords = slice_coords(foc_dists, N, S, space)
    src = stack.device
    if N == 0 or H * W == 0:
        new = lambda shape, dt=torch.float32: torch.empty(shape, dtype=dt, device=src)      # noqa: E731
        return DepthFromStack(new((N, 1, H, W)), new((N, 1, H, W), torch.int32), new((N, 1, H, W)), new((N, Cn, H, W)),
                              new((N, S, H, W) if return_volume else (0,)))
    _abi.require_gpu()
    dev = src if stack.is_cuda else torch.device("cuda", torch.cuda.current_device())
    u, index, peak, aif, volume = torch.ops.aadff.depth_from_stack(_abi.f32c(stack, dev), coords.to(dev), int(window), interp, float(eps),
                                                                  True, bool(return_volume))
    depth = 1.0 / u if space == "inverse" else u
    return DepthFromStack(*(t.to(src) for t in (depth, index, peak, aif, volume)))
