"""Seam-free PSF-map rendering (csrc/conv_blend.hip): every pixel's PSF is the bilinear interpolation of the four
grid PSFs whose nodes surround it, computed in one launch straight from the [S,C,grid*ks,grid*ks] maps of `Lensgroup.psf_map` /
`render_focal_stack_m1(..., return_maps=True)`.  The patch route (`render_psf_map[_stack]`) holds the PSF constant over each patch
and jumps at every patch border; this one is continuous, at four FMAs per tap instead of one.

    render_psf_map_blend(img, psf_map, grid, nodes="psf_map")          -> [B,C,H,W]
    render_psf_map_blend_stack(img, psf_maps, grid, nodes="psf_map")   -> [B,C,S,H,W]
    blend_nodes(n, grid, mode)                                         -> float32 [grid]

`nodes` says where the grid PSFs sit, in pixel-index units (pixel centres at integers):
    "psf_map"  where `psf_map` traces them: linspace(-0.98, 0.98, grid) of the field, (u + 1) / 2 * n - 0.5     (default)
    "patch"    the centres of the patches of `render_psf_map`: (i + 0.5) / grid * n - 0.5
    (node_y, node_x)   two explicit 1-D tensors of `grid` strictly increasing values
Pixels beyond the outer nodes take the outer PSF.  Forward only: tensors that require grad are refused here; the differentiable twins
(gradients to the image and the maps, csrc/conv_blend_bwd.hip) are `aadff.diffrender.render_psf_map_blend[_stack]`.
The functions call the C entry (aadff_render_psf_map_blend_stack) directly, as the planners of aadff/focal_stack.py do; there is no
torch custom op for it: the set of `torch.ops.aadff` ops is a recorded one (tests/golden/ops_schemas.json).
"""
import ctypes as C

import numpy as np
import torch

from . import _abi

NODE_MODES = ("psf_map", "patch")


def blend_nodes(n, grid, mode="psf_map"):
    """float32 [grid]: the pixel-index positions of the grid PSFs along an axis of n pixels, computed in float64 and rounded once."""
    n, grid = int(n), int(grid)
    assert grid >= 1, "grid should be at least 1"
    j = np.arange(grid, dtype=np.float64)
    if mode == "psf_map":
        pos = np.array([(n - 1) / 2.0]) if grid == 1 else ((-0.98 + 1.96 * j / (grid - 1)) + 1.0) / 2.0 * n - 0.5
    elif mode == "patch":
        pos = (j + 0.5) / grid * n - 0.5
    else:
        raise ValueError(f"blend_nodes: mode {mode!r} is not one of {NODE_MODES}")
    return torch.from_numpy(pos.astype(np.float32))


def _nodes(nodes, H, W, grid):
    if isinstance(nodes, str):
        return blend_nodes(H, grid, nodes), blend_nodes(W, grid, nodes)
    node_y, node_x = nodes
    node_y = torch.as_tensor(node_y).detach().to("cpu", torch.float32).contiguous()
    node_x = torch.as_tensor(node_x).detach().to("cpu", torch.float32).contiguous()
    assert node_y.shape == (grid,) and node_x.shape == (grid,), "nodes should be two 1-D tensors of grid values"
    return node_y, node_x


def _prep(img, psf_maps, what):
    if (img.requires_grad or psf_maps.requires_grad) and torch.is_grad_enabled():
        raise RuntimeError(f"{what}: forward-only HIP op, call it under torch.no_grad() or detach the input (the differentiable twin is aadff.diffrender.{what})")
    _abi.require_gpu()
    return img.device if img.is_cuda else torch.device("cuda", torch.cuda.current_device())


def render_psf_map_blend_stack(img, psf_maps, grid, nodes="psf_map"):
    """img [B,C,H,W], psf_maps [S,C,grid*ks,grid*ks] -> [B,C,S,H,W]: slice s is img rendered with the bilinearly interpolated PSFs of
    map s; equal to torch.stack([render_psf_map_blend(img, m, grid, nodes) for m in psf_maps], dim=2) bit for bit, with the image
    tile staged once for all S slices."""
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    S, Cpsf, Hpsf, Wpsf = psf_maps.shape
    assert Hpsf % grid == 0 and Wpsf % grid == 0, "PSF map size should be divisible by grid"
    ks = int(Hpsf / grid)
    assert ks % 2 == 1, "PSF kernel size should be odd"
    B, C_, H, W = img.shape
    assert C_ == Cpsf, "PSF map should have the same channel as image"
    node_y, node_x = _nodes(nodes, H, W, grid)
    if img.numel() == 0 or S == 0:
        return torch.empty((B, C_, S, H, W), dtype=torch.float32, device=img.device)
    dev = _prep(img, psf_maps, "render_psf_map_blend_stack")
    x, p = _abi.f32c(img, dev), _abi.f32c(psf_maps, dev)
    out = x.new_empty((B, C_, S, H, W))
    with _abi.on_device(dev):
        _abi.call("aadff_render_psf_map_blend_stack", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), C.c_void_p(node_y.data_ptr()),
                  C.c_void_p(node_x.data_ptr()), B, C_, S, H, W, grid, ks, _abi.stream_ptr(dev))
    return out.to(img.device)


def render_psf_map_blend(img, psf_map, grid, nodes="psf_map"):
    """img [B,C,H,W], psf_map [C,grid*ks,grid*ks] -> [B,C,H,W]: the seam-free sibling of render_psf_map."""
    assert len(psf_map.shape) == 3, "PSF map should be [C, grid*ks, grid*ks]"
    return render_psf_map_blend_stack(img, psf_map[None], grid, nodes)[:, :, 0]
