"""Differentiable image-space PSF rendering on MI355X.

The reference's deeplens/render_psf.py is plain torch (F.pad + F.conv2d :12-73, unfold / fold :76-107), so its functions
are differentiable with respect to the image and the PSF.  `deeplens.render_psf` of this package is forward-only; this
module has the same five functions - signatures, assertions and return conventions of the reference - with gradients
to the image AND the PSF from hand-written HIP kernels (csrc/conv_bwd.hip, csrc/gather.hip through torch.ops.aadff.*_diff, aadff/ops.py):

    from aadff.diffrender import render_psf_map          # instead of: from deeplens.render_psf import render_psf_map

The forward is the existing kernel: under torch.no_grad(), or when no input requires grad, every function returns exactly
what the forward-only function returns.  `grid` / `kernel_size` get no gradient, integer inputs are converted as in the
forward, double backward is not supported (it raises).

`psfnet_render` / `psfnet_render_stack` are PSFNet.render / PSFNet.render_stack (deeplens/psfnet.py:393-450, the path the
reference's training scripts render their stacks with) differentiable to the image, the DEPTH map and the focus distances: the
fused kernel's forward, and a fused backward that recomputes it and runs the transposed network on the matrix cores
(csrc/psfnet_bwd.hip, torch.ops.aadff.psfnet_render_rgbd_diff) - nothing is stored between forward and backward.

`thinlens_render` / `thinlens_render_stack` are ThinLens.render (deeplens/psfnet.py:549-570, the baseline lens of
dff.factory.get_lens) and its stack form with the same three gradients: the fused forward kernels, and a fused backward that
re-evaluates every pixel's Gaussian PSF in the kernel (csrc/thinlens.hip, torch.ops.aadff.thinlens_render_stack_diff) - no
[N,H,W,ks,ks] tensor in either direction.  With them both lens models of dff.factory.get_lens have a differentiable renderer.

`render_psf_map_blend` / `render_psf_map_blend_stack` are the seam-free renders of aadff/blend.py (every pixel's PSF the bilinear blend of
the four grid PSFs around it) with gradients to the image and the PSF maps from csrc/conv_blend_bwd.hip: the forward is
the forward-only kernel, bit for bit, the backward calls aadff_render_psf_map_blend_stack_bwd through the C ABI (no torch custom op),
computes only the gradients autograd asks for and keeps nothing but the two inputs in between.  `grid` and `nodes` get no gradient.

`render_psf_map_occluded` / `render_psf_map_occluded_stack` are the occlusion-aware layered renders of aadff/occlusion.py (every layer's
premultiplied image and mask blurred with that layer's PSFs, composited front to back) with gradients to the image and the PSF maps from
csrc/conv_occl_bwd.hip: the forward is the forward-only kernel, bit for bit; the backward calls
aadff_render_psf_map_stack_occluded_bwd through the C ABI, recomputes the per-layer sums, computes only the gradients autograd asks for
and keeps nothing but the inputs in between.  With `return_coverage` both results are differentiable.  The layer map gets no gradient.

Not covered: gradients through the ray tracer and the M1-layered stack; gradients to the nodes of the blended render and to a depth map
behind the layer map of the occluded render.
"""
import ctypes as C
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


# ---------------------------------------------------------------- blended PSF-map render (aadff/blend.py, csrc/conv_blend_bwd.hip)
def _host_ptr(t):
    return C.c_void_p(t.data_ptr())


class _BlendStack(torch.autograd.Function):
    """x [B,C,H,W], p [S,C,g ks,g ks] float32 contiguous on the GPU -> [B,C,S,H,W]; node_y, node_x float32 [g] on the CPU."""

    @staticmethod
    def forward(ctx, x, p, node_y, node_x, grid):
        B, C_, H, W = x.shape
        S, ks = p.shape[0], p.shape[-1] // grid
        out = x.new_empty((B, C_, S, H, W))
        with _abi.on_device(x.device):
            _abi.call("aadff_render_psf_map_blend_stack", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), _host_ptr(node_y), _host_ptr(node_x),
                      B, C_, S, H, W, grid, ks, _abi.stream_ptr(x.device))
        ctx.save_for_backward(x, p)
        ctx.nodes, ctx.grid = (node_y, node_x), grid
        return out

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, dy):
        x, p = ctx.saved_tensors
        node_y, node_x = ctx.nodes
        grid = ctx.grid
        B, C_, H, W = x.shape
        S, ks = p.shape[0], p.shape[-1] // grid
        want_img, want_maps = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        dy = _abi.f32c(dy, x.device)
        d_img = torch.empty_like(x) if want_img else None
        d_maps = torch.empty_like(p) if want_maps else None
        ws, nbytes = None, 0
        if want_maps:
            nbytes = _abi.load_library().aadff_render_psf_map_blend_stack_bwd_workspace(B, C_, S, H, W, grid, ks)
            ws = _abi.workspace(x, nbytes)
        with _abi.on_device(x.device):
            _abi.call("aadff_render_psf_map_blend_stack_bwd", _abi.ptr(x), _abi.ptr(p), _abi.ptr(dy), _abi.ptr(d_img), _abi.ptr(d_maps),
                      _abi.ptr(ws), C.c_size_t(nbytes), _host_ptr(node_y), _host_ptr(node_x), B, C_, S, H, W, grid, ks,
                      _abi.stream_ptr(x.device))
        return d_img, d_maps, None, None, None


def render_psf_map_blend_stack(img, psf_maps, grid, nodes="psf_map"):
    """aadff.blend.render_psf_map_blend_stack with gradients: img [B,C,H,W], psf_maps [S,C,grid*ks,grid*ks] -> [B,C,S,H,W]; d_img is the sum
    over the slices, d_maps the sum over the batch.  Under torch.no_grad(), or when neither input requires grad, this IS the forward-only
    function.  Double backward raises."""
    from . import blend
    if not _wants_grad(img, psf_maps):
        return blend.render_psf_map_blend_stack(img, psf_maps, grid, nodes)
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    S, Cpsf, Hpsf, Wpsf = psf_maps.shape
    assert Hpsf % grid == 0 and Wpsf % grid == 0, "PSF map size should be divisible by grid"
    ks = int(Hpsf / grid)
    assert ks % 2 == 1, "PSF kernel size should be odd"
    B, C_, H, W = img.shape
    assert C_ == Cpsf, "PSF map should have the same channel as image"
    node_y, node_x = blend._nodes(nodes, H, W, grid)
    if img.numel() == 0 or S == 0:
        return _empty(img, psf_maps, (B, C_, S, H, W))
    dev = _dev(img)
    return _BlendStack.apply(_abi.f32c(img, dev), _abi.f32c(psf_maps, dev), node_y, node_x, int(grid)).to(img.device)


def render_psf_map_blend(img, psf_map, grid, nodes="psf_map"):
    """aadff.blend.render_psf_map_blend with gradients: img [B,C,H,W], psf_map [C,grid*ks,grid*ks] -> [B,C,H,W]."""
    assert len(psf_map.shape) == 3, "PSF map should be [C, grid*ks, grid*ks]"
    return render_psf_map_blend_stack(img, psf_map[None], grid, nodes)[:, :, 0]


# ---------------------------------------------------------------- occlusion-aware layered render (aadff/occlusion.py, csrc/conv_occl_bwd.hip)
OCCL_WORKSPACE_CAP = 1 << 30          # bytes of backward workspace above which a stack is taken in several passes


class _OcclStack(torch.autograd.Function):
    """x [B,C,H,W], p [S L,C,g ks,g ks] float32 and lay [B,H,W] uint8, contiguous on the GPU -> (out, coverage) [B,C,S,H,W]."""

    @staticmethod
    def forward(ctx, x, p, lay, L, grid, normalize):
        B, C_, H, W = x.shape
        S, ks = p.shape[0] // L, p.shape[-1] // grid
        out, cov = x.new_empty((B, C_, S, H, W)), x.new_empty((B, C_, S, H, W))
        with _abi.on_device(x.device):
            _abi.call("aadff_render_psf_map_stack_occluded", _abi.ptr(x), _abi.ptr(p), _abi.ptr(lay), _abi.ptr(out), _abi.ptr(cov), B, C_, S, L, H, W,
                      grid, ks, normalize, _abi.stream_ptr(x.device))
        ctx.save_for_backward(x, p, lay)
        ctx.set_materialize_grads(False)         # an unused result's gradient arrives as None and goes to the entry as NULL
        ctx.args = (L, grid, normalize)
        return out, cov

    @staticmethod
    @torch.autograd.function.once_differentiable
    def backward(ctx, g, h):
        x, p, lay = ctx.saved_tensors
        L, grid, normalize = ctx.args
        B, C_, H, W = x.shape
        S, ks = p.shape[0] // L, p.shape[-1] // grid
        want_img, want_maps = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
        g = None if g is None else _abi.f32c(g, x.device)
        h = None if h is None else _abi.f32c(h, x.device)
        if g is None and h is None:
            return (torch.zeros_like(x) if want_img else None), (torch.zeros_like(p) if want_maps else None), None, None, None, None
        d_img = torch.empty_like(x) if want_img else None
        d_maps = torch.empty_like(p) if want_maps else None
        query = _abi.load_library().aadff_render_psf_map_stack_occluded_bwd_workspace
        nbytes = query(B, C_, S, L, H, W, grid, ks, 1 if want_maps else 0)
        if nbytes > OCCL_WORKSPACE_CAP:          # fewer slices per pass, never below one: the gradients are bit-equal for every size
            one = query(B, C_, 1, L, H, W, grid, ks, 1 if want_maps else 0)
            nbytes = max(one, OCCL_WORKSPACE_CAP // one * one)
        ws = _abi.workspace(x, nbytes)
        with _abi.on_device(x.device):
            _abi.call("aadff_render_psf_map_stack_occluded_bwd", _abi.ptr(x), _abi.ptr(p), _abi.ptr(lay), _abi.ptr(g), _abi.ptr(h), _abi.ptr(d_img),
                      _abi.ptr(d_maps), _abi.ptr(ws), C.c_size_t(nbytes), B, C_, S, L, H, W, grid, ks, normalize, _abi.stream_ptr(x.device))
        return d_img, d_maps, None, None, None, None


def render_psf_map_occluded_stack(img, maps, layer, L, grid, normalize=True, return_coverage=False):
    """aadff.occlusion.render_psf_map_occluded_stack with gradients: img [B,C,H,W], maps [S*L,C,grid*ks,grid*ks], layer [B,H,W] (uint8 or
    int64, an index >= L a hole) -> [B,C,S,H,W], and the coverage with `return_coverage`; both are differentiable.  d_img is the sum over
    the slices, d_maps the sum over the batch; the layer map gets no gradient.  Under torch.no_grad(), or when neither input requires
    grad, this IS the forward-only function.  Double backward raises."""
    from . import occlusion
    if not _wants_grad(img, maps):
        return occlusion.render_psf_map_occluded_stack(img, maps, layer, L, grid, normalize, return_coverage)
    assert len(img.shape) == 4, "Input image should be [B, C, H, W]"
    assert len(maps.shape) == 4, "PSF maps should be [S*L, C, grid*ks, grid*ks]"
    L, grid = int(L), int(grid)
    assert 1 <= L <= occlusion.MAX_LAYERS, f"L should be in 1..{occlusion.MAX_LAYERS}"
    SL, Cpsf, Hpsf, Wpsf = maps.shape
    assert SL % L == 0, "PSF maps should hold L maps per slice"
    assert grid >= 1 and Hpsf % grid == 0 and Wpsf % grid == 0 and Hpsf == Wpsf, "PSF map size should be divisible by grid"
    ks = Hpsf // grid
    assert ks % 2 == 1, "PSF kernel size should be odd"
    assert 3 <= ks <= _abi.MAX_KS, f"PSF kernel size should be in 3..{_abi.MAX_KS}"
    B, C_, H, W = img.shape
    assert C_ == Cpsf, "PSF map should have the same channel as image"
    S = SL // L
    lay = occlusion._layer_u8(layer, B, H, W, L)
    if img.numel() == 0 or S == 0:
        out = _empty(img, maps, (B, C_, S, H, W))
        return (out, out * 1) if return_coverage else out
    dev = _dev(img)
    out, cov = _OcclStack.apply(_abi.f32c(img, dev), _abi.f32c(maps, dev), lay.to(dev).contiguous(), L, grid, 1 if normalize else 0)
    return (out.to(img.device), cov.to(img.device)) if return_coverage else out.to(img.device)


def render_psf_map_occluded(img, maps, layer, grid, normalize=True, return_coverage=False):
    """aadff.occlusion.render_psf_map_occluded with gradients: img [B,C,H,W], maps [L,C,grid*ks,grid*ks] (one map per layer),
    layer [B,H,W] -> [B,C,H,W] (and the coverage)."""
    assert len(maps.shape) == 4, "PSF maps should be [L, C, grid*ks, grid*ks]"
    res = render_psf_map_occluded_stack(img, maps, layer, maps.shape[0], grid, normalize, return_coverage)
    if return_coverage:
        return res[0][:, :, 0], res[1][:, :, 0]
    return res[:, :, 0]


# ---------------------------------------------------------------- PSF-network renderers (deeplens/psfnet.py:393-450)
_DIFF_MODES = ("fp32", "torch")


def _psfnet_stack(lens, img, depth, foc_dists):
    """img [N,C,H,W], depth [N,H,W], foc_dists [N,S] on any device -> [N,C,S,H,W] with gradients."""
    from . import psfnet_pack
    mode = lens.mlp_precision
    if mode not in _DIFF_MODES:
        raise ValueError(f"aadff.diffrender: mlp_precision={mode!r} has no differentiable renderer; supported modes are 'fp32' (fused HIP "
                         "backward) and 'torch' (torch autograd over the network)")
    dev = next(lens.psfnet.parameters()).device
    N, C, H, W = img.shape
    ks = lens.kernel_size
    x, d = _abi.f32c(img, dev), _abi.f32c(depth, dev)
    foc_z = lens.depth2z(foc_dists.to(device=dev, dtype=torch.float32).reshape(N, -1))          # torch autograd: the clamp's chain rule
    if mode == "torch":
        z = lens.depth2z(d)
        gx, gy = lens._field_grid(H, W, dev)
        gx, gy = gx.unsqueeze(0).expand(N, H, W), gy.unsqueeze(0).expand(N, H, W)
        slices = []
        for i in range(foc_z.shape[1]):
            o = torch.stack((gx, gy, z, foc_z[:, i].reshape(N, 1, 1).expand(N, H, W)), -1).float()
            psf = lens.psfnet(o)
            slices.append(local_psf_render(x, psf.reshape(N, H, W, ks, ks), ks))
        return torch.stack(slices, dim=2)
    _abi.require_gpu()
    if dev.type != "cuda" or not psfnet_pack.supported(lens.psfnet):
        raise ValueError("aadff.diffrender: this PSF network is outside what the fused kernel supports (psfnet_pack.supported) or not on "
                         "the GPU; supported modes are 'fp32' for such a network on the GPU and 'torch'")
    packed = lens._fused(dev)
    wt, wt_exp = psfnet_pack.transposed(packed, lens.psfnet)
    xs, ys = lens._field_axes(H, W, dev)
    inv_range = float(np.float32(1.0) / np.float32(lens.d_max - lens.d_min))      # as psfnet_pack.render_rgbd
    out, flags = torch.ops.aadff.psfnet_render_rgbd_diff(x, d, xs, ys, foc_z, float(lens.d_min), inv_range, packed.wpack, packed.bias, wt,
                                                         list(wt_exp), list(packed.ins), list(packed.outs), ks)
    if int(flags.item()) & 16:
        raise psfnet_pack.ActivationOverflow("aadff: a hidden activation of the PSF network exceeded 65504, the range of the fp16 hi/lo "
                                             "operand split of the fused kernel; use mlp_precision='torch' for this network")
    return out


def _psfnet_wants_grad(lens, *ts):
    return _wants_grad(*ts) or (lens.mlp_precision == "torch" and _wants_grad(*lens.psfnet.parameters()))


def psfnet_render_stack(lens, img, depth, foc_dists):
    """PSFNet.render_stack with gradients: img [N,C,H,W], depth [N,1,H,W] (mm, < 0), foc_dists [N,S] (mm, < 0) -> [N,C,S,H,W].

    Gradients go to `img`, `depth` and `foc_dists` (through depth2z = torch.clamp: exactly 0 for a depth or a focus distance outside
    [d_max, d_min]); only those that are required are computed.  `lens.mlp_precision`:
      "fp32"  (default) the fused forward kernel (bit-equal to lens.render_stack) and the fused HIP backward.  The network WEIGHTS get
              no gradient on this path.
      "torch" lens.psfnet under torch autograd + `local_psf_render` of this module: keeps every activation, also gives parameter gradients.
      "fp16" / "bf16" raise ValueError, as does a network the fused kernel does not support in "fp32" mode: no silent fallback.
    Under torch.no_grad(), or when nothing requires grad, this IS lens.render_stack.  Double backward raises."""
    if not _psfnet_wants_grad(lens, img, depth, foc_dists):
        return lens.render_stack(img, depth, foc_dists)
    N, C, H, W = img.shape
    return _psfnet_stack(lens, img, depth.reshape(N, H, W), foc_dists.reshape(N, -1)).to(img.device)


def psfnet_render(lens, img, depth, foc_dist):
    """PSFNet.render with gradients (see psfnet_render_stack): img [N,C,H,W], depth [N,1,H,W], foc_dist [N] -> [N,C,H,W], or the 3-D
    branch img [C,H,W], depth [H,W], scalar foc_dist (a float, or a 0-d tensor that may require grad) -> [C,H,W]."""
    if not _psfnet_wants_grad(lens, img, depth, foc_dist):
        return lens.render(img, depth, foc_dist)
    if len(img.shape) == 3:
        H, W = depth.shape
        fd = torch.as_tensor(foc_dist, dtype=torch.float32).reshape(1, 1)
        return _psfnet_stack(lens, img.unsqueeze(0), depth.reshape(1, H, W), fd)[0, :, 0].to(img.device)
    if len(img.shape) != 4:
        raise ValueError("img should be [C,H,W] or [N,C,H,W]")
    N, C, H, W = img.shape
    return _psfnet_stack(lens, img, depth.reshape(N, H, W), foc_dist.reshape(N, 1))[:, :, 0].to(img.device)


# ---------------------------------------------------------------- thin-lens baseline (deeplens/psfnet.py:489-570)
_THIN_KS = (3, 5, 7, 9, 11, 13)


def _thinlens_tensor_form(lens, img, depth, fd):
    """The reference's tensor form (psfnet.py:549-570) under torch autograd: lens.coc -> [N,H,W,ks,ks] Gaussian PSFs -> `local_psf_render`
    of this module.  The path of shapes outside the fused kernels' domain."""
    ks, dev = lens.kernel_size, img.device
    N, C, H, W = img.shape
    fdm = fd.reshape(N, 1, 1, 1).expand(N, 1, H, W)
    x, y = torch.meshgrid(torch.linspace(-ks / 2 + 1 / 2, ks / 2 - 1 / 2, ks), torch.linspace(ks / 2 - 1 / 2, -ks / 2 + 1 / 2, ks), indexing="xy")
    x, y = x.to(dev), y.to(dev)
    rad = lens.coc(depth, fdm).squeeze(1).unsqueeze(-1).unsqueeze(-1) / 2
    psf = torch.exp(-(x ** 2 + y ** 2) / 2 / rad ** 2) / (2 * np.pi * rad ** 2)
    psf = psf * (x ** 2 + y ** 2 < rad ** 2)
    psf = psf / psf.sum((-1, -2)).unsqueeze(-1).unsqueeze(-1)
    return local_psf_render(img, psf, ks)


def _thinlens_stack(lens, img, depth, foc_dists):
    """img [N,C,H,W], depth [N,1,H,W], foc_dists [N,S] on any device -> [N,C,S,H,W] on the GPU, with gradients."""
    N, C, H, W = img.shape
    S = foc_dists.shape[1]
    if img.numel() == 0 or S == 0:
        zero = img.to(torch.float32).sum() * 0 + depth.to(device=img.device, dtype=torch.float32).sum() * 0 \
            + foc_dists.to(device=img.device, dtype=torch.float32).sum() * 0
        return zero.expand((N, C, S, H, W)) * 1
    dev = _dev(img)
    x, d, f = _abi.f32c(img, dev), _abi.f32c(depth, dev), _abi.f32c(foc_dists, dev)
    ks = lens.kernel_size
    if C > 4 or ks not in _THIN_KS:
        return torch.stack([_thinlens_tensor_form(lens, x, d, f[:, i]) for i in range(S)], dim=2)
    return torch.ops.aadff.thinlens_render_stack_diff(x, d, f, ks, float(lens.foc_len), float(lens.fnum), float(lens.ps), float(lens.d_min),
                                                      float(lens.d_max))


def thinlens_render_stack(lens, img, depth, foc_dists):
    """ThinLens.render_stack with gradients: img [N,C,H,W], depth [N,1,H,W] (mm, either sign convention), foc_dists [N,S] -> [N,C,S,H,W].

    Gradients go to `img`, `depth` and `foc_dists`; only those that are required are computed.  They are the autograd of the reference's
    tensor form with the disc mask as a constant: exactly 0 for a depth outside [d_min, d_max] and where the 0.1 px floor of the circle of
    confusion is active, and bit-identical from run to run.  C <= 4 and kernel_size in {3, 5, ..., 13}: the fused HIP forward (bit-equal
    to lens.render_stack) and the fused HIP backward; any other shape: the reference's tensor form under torch autograd with
    `local_psf_render` of this module, one slice at a time.  Under torch.no_grad(), or when nothing requires grad, this IS
    lens.render_stack.  Double backward raises."""
    if len(img.shape) != 4:
        raise ValueError("ThinLens.render_stack needs [N,C,H,W] (the reference's 3-D branch calls methods ThinLens lacks)")
    N, C, H, W = img.shape
    if not _wants_grad(img, depth, foc_dists):
        return lens.render_stack(img, depth, foc_dists)
    S = foc_dists.shape[-1] if foc_dists.dim() == 2 else foc_dists.numel() // max(N, 1)
    return _thinlens_stack(lens, img, depth.reshape(N, 1, H, W), foc_dists.reshape(N, S)).to(img.device)


def thinlens_render(lens, img, depth, foc_dist):
    """ThinLens.render with gradients (see thinlens_render_stack): img [N,C,H,W], depth [N,1,H,W], foc_dist [N] -> [N,C,H,W].  The 3-D
    branch raises the ValueError of ThinLens.render."""
    if not _wants_grad(img, depth, foc_dist):
        return lens.render(img, depth, foc_dist)
    if len(img.shape) != 4:
        raise ValueError("ThinLens.render needs [N,C,H,W] (the reference's 3-D branch calls methods ThinLens lacks)")
    N, C, H, W = img.shape
    return _thinlens_stack(lens, img, depth.reshape(N, 1, H, W), foc_dist.reshape(N, 1))[:, :, 0].to(img.device)
