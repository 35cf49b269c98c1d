"""Occlusion-aware layered PSF-map rendering (csrc/conv_occl.hip): every depth layer's premultiplied image and its
mask are blurred with that layer's grid PSFs and the layers are composited front to back with a transmittance, in one launch per
stack.  The per-pixel layer selection of `render_focal_stack_m1_layered` lets a blurred background bleed through a sharp foreground
edge and the reverse; this is the pixel-level form of the per-ray rule of `render_raytraced_layered`.

    render_psf_map_occluded(img, maps, layer, grid, normalize=True, return_coverage=False)            -> [B,C,H,W]
    render_psf_map_occluded_stack(img, maps, layer, L, grid, normalize=True, return_coverage=False)   -> [B,C,S,H,W]

`maps` holds one PSF map per layer ([L,C,grid*ks,grid*ks]) or, for a stack, per (slice, layer) pair ([S*L,...], pair s*L + l), as
`render_focal_stack_m1_layered(..., return_parts=True)` returns them.  `layer` [B,H,W] is uint8, or int64 as `depth_layers` returns it;
layer 0 is the nearest and an index >= L lies on no layer (a hole: it covers nothing and shows nothing).  With `normalize` the
composite V is divided by the accumulated coverage A where A > 0 (0 elsewhere); `return_coverage` adds A as a second result.  The rule,
tap order included, is the arithmetic contract of `aadff_render_psf_map_stack_occluded` in include/aadff.h.

    render_psf_map_soft_occluded(img, maps, pos, grid, normalize=True, return_coverage=False)         -> [B,C,H,W]
    render_psf_map_soft_occluded_stack(img, maps, pos, L, grid, normalize=True, return_coverage=False) -> [B,C,S,H,W]
    layer_coordinate(depth_mm, centres) -> pos          depth_nodes(depth_mm, layers) -> (pos, centres)

The soft pair (csrc/conv_occl_soft.hip) takes the maps as NODES in depth and a float layer coordinate `pos` [B,H,W]
in place of the index map: a texel with coordinate k + f lies in slab k and is blurred with (1 - f) PSF_k + f PSF_{k+1}; the slabs are
composited front to back as the layers are.  !(pos >= 0) is a hole, pos above L - 1 counts as L - 1, integral coordinates give the
hard render bit for bit.  The rule is the contract of `aadff_render_psf_map_stack_soft_occluded`.  `layer_coordinate` (pure torch,
differentiable) maps depths to coordinates over given node depths and `depth_nodes` places the nodes of a depth map.

Forward only: tensors that require grad are refused (the differentiable twins of the same names are in aadff.diffrender, DESIGN.md
4.21).  The functions call the C entry directly; there is no torch custom op for it: the
set of `torch.ops.aadff` ops is a recorded one (tests/golden/ops_schemas.json).
"""
import torch

from . import _abi

MAX_LAYERS = 32                     # AADFF_RENDER_MAX_LAYERS: the presence mask of a tile is one 32-bit word


def _layer_u8(layer, B, H, W, L):
    """The layer map as uint8 [B,H,W]; int64 values outside 0 .. 255 are refused (they would wrap into a layer)."""
    assert tuple(layer.shape) == (B, H, W), "layer should be [B, H, W]"
    assert layer.dtype in (torch.uint8, torch.int64), "layer should be uint8 or int64"
    if layer.dtype == torch.int64 and layer.numel():
        lo, hi = int(layer.min()), int(layer.max())
        assert 0 <= lo and hi <= 255, f"layer values should be in 0..255 (an index >= L = {L} is a hole), got {lo}..{hi}"
        layer = layer.to(torch.uint8)
    return layer


def render_psf_map_occluded_stack(img, maps, layer, L, grid, normalize=True, return_coverage=False):
    """img [B,C,H,W], maps [S*L,C,grid*ks,grid*ks], layer [B,H,W] -> [B,C,S,H,W] (and the coverage A [B,C,S,H,W]): slice s is the
    front-to-back composite of the L layers blurred with maps s*L .. s*L + L-1; equal to the slices rendered one by one bit for bit,
    with the image and layer tiles staged once for all S slices."""
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    assert len(maps.shape) == 4, "PSF maps should be [S*L, C, grid*ks, grid*ks]"
    L, grid = int(L), int(grid)
    assert 1 <= L <= MAX_LAYERS, f"L should be in 1..{MAX_LAYERS}"
    SL, Cpsf, Hpsf, Wpsf = maps.shape
    assert SL % L == 0, "PSF maps should hold L maps per slice"
    assert grid >= 1 and Hpsf % grid == 0 and Wpsf % grid == 0 and Hpsf == Wpsf, "PSF map size should be divisible by grid"
    ks = Hpsf // grid
    assert ks % 2 == 1, "PSF kernel size should be odd"
    assert 3 <= ks <= _abi.MAX_KS, f"PSF kernel size should be in 3..{_abi.MAX_KS}"
    B, C_, H, W = img.shape
    assert C_ == Cpsf, "PSF map should have the same channel as image"
    S = SL // L
    lay = _layer_u8(layer, B, H, W, L)
    if (img.requires_grad or maps.requires_grad) and torch.is_grad_enabled():
        raise RuntimeError("render_psf_map_occluded_stack: forward-only HIP op, call it under torch.no_grad() or detach the input")
    if img.numel() == 0 or S == 0:
        out = torch.empty((B, C_, S, H, W), dtype=torch.float32, device=img.device)
        return (out, torch.empty_like(out)) if return_coverage else out
    _abi.require_gpu()
    dev = img.device if img.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x, p, li = _abi.f32c(img, dev), _abi.f32c(maps, dev), lay.to(dev).contiguous()
    out = x.new_empty((B, C_, S, H, W))
    cov = x.new_empty((B, C_, S, H, W)) if return_coverage else None
    with _abi.on_device(dev):
        _abi.call("aadff_render_psf_map_stack_occluded", _abi.ptr(x), _abi.ptr(p), _abi.ptr(li), _abi.ptr(out), _abi.ptr(cov), B, C_, S, L, H, W,
                  grid, ks, 1 if normalize else 0, _abi.stream_ptr(dev))
    if return_coverage:
        return out.to(img.device), cov.to(img.device)
    return out.to(img.device)


def render_psf_map_occluded(img, maps, layer, grid, normalize=True, return_coverage=False):
    """img [B,C,H,W], maps [L,C,grid*ks,grid*ks] (one map per layer), layer [B,H,W] -> [B,C,H,W]: the occlusion-aware sibling of the
    per-pixel layer selection."""
    assert len(maps.shape) == 4, "PSF maps should be [L, C, grid*ks, grid*ks]"
    res = render_psf_map_occluded_stack(img, maps, layer, maps.shape[0], grid, normalize, return_coverage)
    if return_coverage:
        return res[0][:, :, 0], res[1][:, :, 0]
    return res[:, :, 0]


# ------------------------------------------------------------------------------------------------------------- soft depth layers
def _coordinate(d, c):
    """Positive distances d (any shape) over increasing node distances c [L]: sum_i clamp((d - c_i) / (c_{i+1} - c_i), 0, 1)."""
    if c.numel() == 1:
        return torch.zeros_like(d)
    lo, step = c[:-1], c[1:] - c[:-1]
    return torch.clamp((d.unsqueeze(-1) - lo) / step, 0.0, 1.0).sum(-1)


def layer_coordinate(depth_mm, centres):
    """The layer coordinate of every depth (mm, < 0 = in front of the lens; >= 0 = invalid) over the node depths `centres` [L] (mm, < 0,
    nearest first, strictly monotone): piecewise linear between nodes (a depth at node l gives l), clamped to [0, L-1]; an invalid depth
    goes to L-1, as `depth_layers` sends it to the farthest layer.  Pure torch and differentiable in both arguments; same shape and
    dtype as `depth_mm`."""
    centres = torch.as_tensor(centres, dtype=depth_mm.dtype, device=depth_mm.device).reshape(-1)
    L = centres.numel()
    assert L >= 1, "centres should hold at least one node depth"
    c = -centres
    assert bool((c > 0).all()) and (L == 1 or bool((c[1:] > c[:-1]).all())), \
        "centres should be negative depths (mm), nearest first and strictly monotone"
    pos = _coordinate(-depth_mm, c)
    return torch.where(depth_mm < 0, pos, torch.full_like(pos, float(L - 1)))


def depth_nodes(depth_mm, layers):
    """Node depths for a depth map (mm, < 0; >= 0 = invalid) and its layer coordinate: `layers` nodes spaced uniformly from the nearest to
    the farthest valid depth (layers = 1: the single node at the mid depth, pos = 0).  Returns (pos like depth_mm, centres [layers], mm
    < 0, nearest first).  Invalid pixels go to the farthest node.  No host read-back."""
    L = int(layers)
    assert L >= 1, "layers should be >= 1"
    d = -depth_mm
    valid = d > 0
    dmin = torch.where(valid, d, torch.full_like(d, float("inf"))).amin()
    dmax = d.amax()
    if L == 1:
        return torch.zeros_like(depth_mm), -((dmin + dmax) * 0.5).reshape(1)
    gap = torch.clamp(dmin * 1e-4, min=1e-6) * (L - 1)
    far = torch.where(dmax - dmin >= gap, dmax, dmin + gap)                      # a flat scene still gets distinct nodes
    t = torch.arange(L, device=d.device, dtype=d.dtype) / (L - 1)
    c = dmin * (1 - t) + far * t                         # the end nodes are the extreme depths exactly: they get 0 and L - 1 exactly
    pos = torch.where(valid, _coordinate(d, c), torch.full_like(d, float(L - 1)))
    return pos, -c


def render_psf_map_soft_occluded_stack(img, maps, pos, L, grid, normalize=True, return_coverage=False):
    """img [B,C,H,W], maps [S*L,C,grid*ks,grid*ks] (node l of slice s is map s*L + l, node 0 the nearest), pos [B,H,W] float, the layer
    coordinate -> [B,C,S,H,W] (and the coverage A [B,C,S,H,W]): slice s is the front-to-back composite of the slabs between the nodes,
    every texel blurred with the PSF interpolated between the two nodes around its coordinate."""
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    assert len(maps.shape) == 4, "PSF maps should be [S*L, C, grid*ks, grid*ks]"
    L, grid = int(L), int(grid)
    assert 1 <= L <= MAX_LAYERS, f"L should be in 1..{MAX_LAYERS}"
    SL, Cpsf, Hpsf, Wpsf = maps.shape
    assert SL % L == 0, "PSF maps should hold L maps per slice"
    assert grid >= 1 and Hpsf % grid == 0 and Wpsf % grid == 0 and Hpsf == Wpsf, "PSF map size should be divisible by grid"
    ks = Hpsf // grid
    assert ks % 2 == 1, "PSF kernel size should be odd"
    assert 3 <= ks <= _abi.MAX_KS, f"PSF kernel size should be in 3..{_abi.MAX_KS}"
    B, C_, H, W = img.shape
    assert C_ == Cpsf, "PSF map should have the same channel as image"
    S = SL // L
    assert tuple(pos.shape) == (B, H, W), "pos should be [B, H, W]"
    assert pos.is_floating_point(), "pos should be a float tensor (the layer coordinate; an index map goes to render_psf_map_occluded)"
    if (img.requires_grad or maps.requires_grad or pos.requires_grad) and torch.is_grad_enabled():
        raise RuntimeError("render_psf_map_soft_occluded_stack: forward-only HIP op, its backward is not built: call it under "
                           "torch.no_grad() or detach the input")
    if img.numel() == 0 or S == 0:
        out = torch.empty((B, C_, S, H, W), dtype=torch.float32, device=img.device)
        return (out, torch.empty_like(out)) if return_coverage else out
    _abi.require_gpu()
    dev = img.device if img.is_cuda else torch.device("cuda", torch.cuda.current_device())
    x, p, c = _abi.f32c(img, dev), _abi.f32c(maps, dev), _abi.f32c(pos, dev)
    out = x.new_empty((B, C_, S, H, W))
    cov = x.new_empty((B, C_, S, H, W)) if return_coverage else None
    with _abi.on_device(dev):
        _abi.call("aadff_render_psf_map_stack_soft_occluded", _abi.ptr(x), _abi.ptr(p), _abi.ptr(c), _abi.ptr(out), _abi.ptr(cov), B, C_, S, L,
                  H, W, grid, ks, 1 if normalize else 0, _abi.stream_ptr(dev))
    if return_coverage:
        return out.to(img.device), cov.to(img.device)
    return out.to(img.device)


def render_psf_map_soft_occluded(img, maps, pos, grid, normalize=True, return_coverage=False):
    """img [B,C,H,W], maps [L,C,grid*ks,grid*ks] (one map per node), pos [B,H,W] float -> [B,C,H,W]: the soft-layer sibling of
    `render_psf_map_occluded`."""
    assert len(maps.shape) == 4, "PSF maps should be [L, C, grid*ks, grid*ks]"
    res = render_psf_map_soft_occluded_stack(img, maps, pos, maps.shape[0], grid, normalize, return_coverage)
    if return_coverage:
        return res[0][:, :, 0], res[1][:, :, 0]
    return res[:, :, 0]
