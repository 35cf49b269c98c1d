"""Differentiable image-space PSF rendering on MI355X.

The reference's deeplens/render_psf.py is plain torch (F.pad + F.conv2d :12-73, unfold / fold :76-107), so its functions
are differentiable with respect to the image and the PSF.  `deeplens.render_psf` of this package is forward-only; this
module has the same five functions - signatures, assertions and return conventions of the reference - with gradients
to the image AND the PSF from hand-written HIP kernels (csrc/conv_bwd.hip through torch.ops.aadff.*_diff, aadff/ops.py):

    from aadff.diffrender import render_psf_map          # instead of: from deeplens.render_psf import render_psf_map

The forward is the existing kernel: under torch.no_grad(), or when no input requires grad, every function returns exactly
what the forward-only function returns.  `grid` / `kernel_size` get no gradient, integer inputs are converted as in the
forward, double backward is not supported (it raises).  Not covered: gradients through the ray tracer, the fused
PSF-network renderers, thinlens_render and the M1-layered stack.
"""
import importlib

import numpy as np
import torch

from . import _abi
from . import ops as _ops      # noqa: F401  (registers torch.ops.aadff.*)


def _fwd():
    return importlib.import_module("deeplens.render_psf")       # (the package re-exports a same-named function)


def _wants_grad(*ts):
    return torch.is_grad_enabled() and any(torch.is_tensor(t) and t.requires_grad for t in ts)


def _dev(t):
    _abi.require_gpu()
    return t.device if t.is_cuda else torch.device("cuda", torch.cuda.current_device())


def _empty(img, psf, shape):
    """An empty result that stays in the autograd graph: backward() gives zero gradients of the inputs' shapes, as the reference's
    conv2d / unfold over an empty batch (or an empty slice loop) does."""
    zero = img.to(torch.float32).sum() * 0 + psf.to(device=img.device, dtype=torch.float32).sum() * 0
    return zero.expand(tuple(shape)) * 1


def render_psf(img, psf):
    """One PSF [C,ks,ks] for the whole image [B,C,H,W]: flip + reflect pad + depthwise conv (render_psf.py:12-28)."""
    if not _wants_grad(img, psf):
        return _fwd().render_psf(img, psf)
    C_, ks, ks2 = psf.shape
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    B, C, H, W = img.shape
    assert C == C_, "PSF map should have the same channel as image"
    assert ks == ks2 and ks % 2 == 1, "PSF kernel size should be odd"
    if img.numel() == 0:
        return _empty(img, psf, img.shape)
    dev = _dev(img)
    out = torch.ops.aadff.render_psf_map_stack_diff(_abi.f32c(img, dev), _abi.f32c(psf, dev).unsqueeze(0), 1)
    return out.squeeze(2).to(img.device)


def render_psf_map(img, psf_map, grid):
    """Different PSF per image patch: img [B,3,H,W], psf_map [3,grid*ks,grid*ks] (render_psf.py:31-73)."""
    if not _wants_grad(img, psf_map):
        return _fwd().render_psf_map(img, psf_map, grid)
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    Cpsf, Hpsf, Wpsf = psf_map.shape
    assert Hpsf % grid == 0 and Wpsf % grid == 0, "PSF map size should be divisible by grid"
    ks = int(Hpsf / grid)
    assert ks % 2 == 1, "PSF kernel size should be odd"
    B, C, H, W = img.shape
    assert C == Cpsf, "PSF map should have the same channel as image"
    if img.numel() == 0:
        return _empty(img, psf_map, img.shape)
    dev = _dev(img)
    out = torch.ops.aadff.render_psf_map_stack_diff(_abi.f32c(img, dev), _abi.f32c(psf_map, dev).unsqueeze(0), grid)
    return out.squeeze(2).to(img.device)


def render_psf_map_stack(img, psf_maps, grid):
    """Stack-fused form: img [B,C,H,W], psf_maps [S,C,grid*ks,grid*ks] -> [B,C,S,H,W]; d_img is the sum over the slices."""
    if not _wants_grad(img, psf_maps):
        return _fwd().render_psf_map_stack(img, psf_maps, grid)
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    S, Cpsf, Hpsf, Wpsf = psf_maps.shape
    assert Hpsf % grid == 0 and Wpsf % grid == 0, "PSF map size should be divisible by grid"
    ks = int(Hpsf / grid)
    assert ks % 2 == 1, "PSF kernel size should be odd"
    B, C, H, W = img.shape
    assert C == Cpsf, "PSF map should have the same channel as image"
    if img.numel() == 0 or S == 0:
        return _empty(img, psf_maps, (B, C, S, H, W))
    dev = _dev(img)
    return torch.ops.aadff.render_psf_map_stack_diff(_abi.f32c(img, dev), _abi.f32c(psf_maps, dev), grid).to(img.device)


def local_psf_render(input, psf, kernel_size=11):
    """Per-pixel PSF [B,H,W,ks,ks] (same for every channel), replicate padding, no flip (render_psf.py:76-107)."""
    if not _wants_grad(input, psf):
        return _fwd().local_psf_render(input, psf, kernel_size=kernel_size)
    if len(input.shape) < 4:
        input = input.unsqueeze(0)
    b, c, h, w = input.shape
    if input.numel() == 0:
        return _empty(input, psf, input.shape)
    dev = _dev(input)
    x = _abi.f32c(input, dev)
    p = _abi.f32c(psf, dev).reshape(-1, h, w, kernel_size, kernel_size)
    assert p.shape[0] == b, "psf should be [B, H, W, ks, ks]"
    return torch.ops.aadff.local_psf_render_diff(x, p, kernel_size).to(input.device)


def local_psf_render_high_res(input, psf, patch_size=[320, 480], kernel_size=11):
    """Tiled variant WITHOUT halo (render_psf.py:110-127): every tile replicate-pads itself, so the seams of the reference are
    in the output and in the gradients alike."""
    if not _wants_grad(input, psf):
        return _fwd().local_psf_render_high_res(input, psf, patch_size=patch_size, kernel_size=kernel_size)
    B, C, H, W = input.shape
    out = torch.zeros_like(input, dtype=torch.float32)
    for pi in range(int(np.ceil(H / patch_size[0]))):
        for pj in range(int(np.ceil(W / patch_size[1]))):
            i0, i1 = pi * patch_size[0], min((pi + 1) * patch_size[0], H)
            j0, j1 = pj * patch_size[1], min((pj + 1) * patch_size[1], W)
            out[:, :, i0:i1, j0:j1] = local_psf_render(input[:, :, i0:i1, j0:j1], psf[:, i0:i1, j0:j1, :, :], kernel_size=kernel_size)
    return out
