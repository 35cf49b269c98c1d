"""torch custom ops (`torch.ops.aadff.*`) over the C ABI of include/aadff.h.

Each op is a `torch.library.custom_op` whose implementation packs pointers and calls libaadff.so on the current HIP stream.  Its outputs
are declared ONCE, in a function of the op's own arguments (`_..._out`, or one shared by a family) that allocates them from a reference
tensor: the implementation calls it, and the same function is the op's fake implementation (the `@_fake(...)` line above the op) -
on a device tensor it allocates, on a fake or meta tensor it infers - so the two cannot disagree.  An op without an autograd formula
raises torch's "not differentiable" error in a backward; the reference never back-propagates through those functions.
A `_diff` op is its plain twin - one shared forward, the same ABI call - with a formula whose backward is the `_bwd` op beside it.

ops                                                   C entry points (aadff_...)                  csrc/             public module
----------------------------------------------------  ------------------------------------------  ----------------  ------------------------
render_psf_map(_stack), render_psf                    the same names                              conv.hip          deeplens/render_psf.py
local_psf_render                                      local_psf_render                            gather.hip        deeplens/render_psf.py
thinlens_render                                       thinlens_render                             thinlens.hip      deeplens/psfnet.py
render_psf_map_stack_diff / _bwd                      render_psf_map_stack, ..._bwd(_workspace)   conv_bwd.hip      aadff/diffrender.py
local_psf_render_diff / _bwd                          local_psf_render, ..._bwd                   gather.hip        aadff/diffrender.py
psfnet_forward, psfnet_render_rgbd                    the same names                              psfnet.hip        deeplens/psfnet.py
psfnet_render_rgbd_diff / _bwd                        psfnet_render_rgbd, ..._bwd(_workspace)     psfnet_bwd.hip    aadff/diffrender.py
thinlens_render_stack, ..._diff / _bwd                thinlens_render_stack, ..._bwd(_workspace)  thinlens.hip      psfnet.py, diffrender.py
depth_from_stack                                      depth_from_stack                            dfocus.hip        aadff/dfocus.py
attention_depth / _bwd, dff_loss_sums, dff_loss_bwd   the same names                              focus_head.hip    aadff/focus_head.py
dfv_regress / _bwd                                    dfv_head_fwd, dfv_head_bwd                  dfv_head.hip      aadff/dfv_head.py
depth_refine / _bwd                                   depth_refine_fwd, depth_refine_bwd          depth_refine.hip  aadff/refine.py
depth_metric_sums, image_metric_sums                  the same names                              metrics.hip       aadff/metrics.py
psf_points, psf_points_block                          psf_points                                  trace.hip         deeplens/optics.py

The deeplens mirror (deeplens/render_psf.py, deeplens/psfnet.py) calls these ops; the multi-launch planners
(aadff/focal_stack.py, aadff/training.py) keep calling the ABI directly because they pass raw offsets into pinned rings.
"""
import ctypes as C
from typing import List, Tuple

import torch
from torch.library import custom_op

from . import _abi
from ._abi import f32 as _f32, opt as _opt, ptr as _ptr, workspace as _workspace


def _st(t):
    return _abi.stream_ptr(t.device)


def _new(ref, shape, want=True, dtype=torch.float32):
    """An output of `shape` on the device of `ref`; one that is not wanted is an empty tensor of its own (outputs must not alias)."""
    return ref.new_empty(shape if want else (0,), dtype=dtype)


def _like(t, want=True):
    """`_new` in the shape of `t`, which is float32 and contiguous (see `_fake`): the plain empty_like, the cheapest allocation per call."""
    return torch.empty_like(t) if want else t.new_empty((0,))


def _fake(outputs):
    """Decorator of an op: its fake implementation is `outputs`, the function that declares its outputs.  The implementation calls
    `outputs` with its tensor arguments converted (`_f32`); here they are converted too, so `outputs` sees float32 contiguous tensors
    either way."""
    def fake(*args):
        return outputs(*[_f32(a) if isinstance(a, torch.Tensor) else a for a in args])

    def register(op):
        op.register_fake(fake)
        return op
    return register


def _image_like(img, *_):
    return torch.empty_like(img)


def _grad_pair(a, b, need_a, need_b):
    """(d_a, d_b) in the shapes of a and b."""
    return _like(a, need_a), _like(b, need_b)


def _grads(ctx, needs, grads, inputs, at=(0, 1, 2)):
    """The return tuple of a backward: grads[i] in the shape of inputs[i] at argument at[i] where needs[i], None everywhere else."""
    out = [None] * len(ctx.needs_input_grad)
    for i, need, d, t in zip(at, needs, grads, inputs):
        if need:
            out[i] = d.reshape(t.shape)
    return tuple(out)


def _no_grads(ctx, *_):
    return (None,) * len(ctx.needs_input_grad)


def _save_first(n):
    """A setup_context that saves the first n arguments (the tensors) for the backward and keeps the others in ctx.consts."""
    def setup(ctx, inputs, output):
        ctx.save_for_backward(*inputs[:n])
        ctx.consts = tuple(inputs[n:])
    return setup


# ---------------------------------------------------------------- image space (deeplens/render_psf.py:12-107)
@_fake(_image_like)
@custom_op("aadff::render_psf_map", mutates_args=(), device_types="cuda")
def render_psf_map(img: torch.Tensor, psf_map: torch.Tensor, grid: int) -> torch.Tensor:
    B, Cn, H, W = img.shape
    ks = psf_map.shape[1] // grid
    x, p = _f32(img), _f32(psf_map)
    out = _image_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_render_psf_map", _ptr(x), _ptr(p), _ptr(out), B, Cn, H, W, grid, ks, _st(x))
    return out


def _map_stack_out(img, psf_maps, grid):
    B, Cn, H, W = img.shape
    return img.new_empty((B, Cn, psf_maps.shape[0], H, W), dtype=torch.float32)


def _map_stack_forward(img, psf_maps, grid):
    B, Cn, H, W = img.shape
    S, ks = psf_maps.shape[0], psf_maps.shape[2] // grid
    x, p = _f32(img), _f32(psf_maps)
    out = _map_stack_out(x, p, grid)
    with torch.cuda.device(x.device):
        _abi.call("aadff_render_psf_map_stack", _ptr(x), _ptr(p), _ptr(out), B, Cn, S, H, W, grid, ks, _st(x))
    return out


@_fake(_map_stack_out)
@custom_op("aadff::render_psf_map_stack", mutates_args=(), device_types="cuda")
def render_psf_map_stack(img: torch.Tensor, psf_maps: torch.Tensor, grid: int) -> torch.Tensor:
    return _map_stack_forward(img, psf_maps, grid)


@_fake(_image_like)
@custom_op("aadff::render_psf", mutates_args=(), device_types="cuda")
def render_psf(img: torch.Tensor, psf: torch.Tensor) -> torch.Tensor:
    B, Cn, H, W = img.shape
    x, p = _f32(img), _f32(psf)
    out = _image_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_render_psf", _ptr(x), _ptr(p), _ptr(out), B, Cn, H, W, psf.shape[-1], _st(x))
    return out


def _local_forward(img, psf, ks):
    B, Cn, H, W = img.shape
    x, p = _f32(img), _f32(psf)
    out = _image_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_local_psf_render", _ptr(x), _ptr(p), _ptr(out), B, Cn, H, W, ks, _st(x))
    return out


@_fake(_image_like)
@custom_op("aadff::local_psf_render", mutates_args=(), device_types="cuda")
def local_psf_render(img: torch.Tensor, psf: torch.Tensor, ks: int) -> torch.Tensor:
    return _local_forward(img, psf, ks)


def _thin_inputs(img, depth, foc, *foc_shape):
    """(img, depth [N,1,H,W], foc [foc_shape], neg): neg is the reference's whole-tensor sign test of the depth, kept on the device."""
    N, Cn, H, W = img.shape
    d = _f32(depth).reshape(N, 1, H, W)
    return _f32(img), d, _f32(foc).reshape(foc_shape), (d < 0).any().to(torch.int32).reshape(1)


def _thin_args(foc_len, fnum, pixel_size, d_min, d_max):
    return (C.c_float(foc_len / fnum), C.c_float(foc_len), C.c_float(1.0 / pixel_size), C.c_float(d_min), C.c_float(d_max))


@_fake(_image_like)
@custom_op("aadff::thinlens_render", mutates_args=(), device_types="cuda")
def thinlens_render(img: torch.Tensor, depth: torch.Tensor, foc_dist: torch.Tensor, ks: int, foc_len: float, fnum: float,
                    pixel_size: float, d_min: float, d_max: float) -> torch.Tensor:
    N, Cn, H, W = img.shape
    x, d, fd, neg = _thin_inputs(img, depth, foc_dist, N)
    out = _image_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_thinlens_render", _ptr(x), _ptr(d), _ptr(fd), _ptr(neg), _ptr(out), N, Cn, H, W, ks,
                  *_thin_args(foc_len, fnum, pixel_size, d_min, d_max), _st(x))
    return out


# ---------------------------------------------------------------- differentiable image space (csrc/conv_bwd.hip, csrc/gather.hip)
# Plain (non-differentiable) ops over the backward ABI, and front ops whose forward is the EXISTING kernel and whose autograd
# formula calls them.  A gradient that is not needed is not computed (NULL pointer) and comes back as an empty tensor.
@_fake(lambda img, psf_maps, dy, grid, need_img, need_psf: _grad_pair(img, psf_maps, need_img, need_psf))
@custom_op("aadff::render_psf_map_stack_bwd", mutates_args=(), device_types="cuda")
def render_psf_map_stack_bwd(img: torch.Tensor, psf_maps: torch.Tensor, dy: torch.Tensor, grid: int, need_img: bool,
                             need_psf: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    B, Cn, H, W = img.shape
    S, ks = psf_maps.shape[0], psf_maps.shape[2] // grid
    x, p, g = _f32(img), _f32(psf_maps), _f32(dy)
    d_img, d_psf = _grad_pair(x, p, need_img, need_psf)
    with torch.cuda.device(x.device):
        nbytes = _abi.query_bytes("aadff_render_psf_map_stack_bwd_workspace", B, Cn, S, H, W, grid, ks) if need_psf else 0
        ws = _workspace(x, nbytes) if need_psf else None
        _abi.call("aadff_render_psf_map_stack_bwd", _ptr(x), _ptr(p), _ptr(g), _opt(d_img), _opt(d_psf), _ptr(ws), C.c_size_t(nbytes),
                  B, Cn, S, H, W, grid, ks, _st(x))
    return d_img, d_psf


@_fake(lambda img, psf, dy, ks, need_img, need_psf: _grad_pair(img, psf, need_img, need_psf))
@custom_op("aadff::local_psf_render_bwd", mutates_args=(), device_types="cuda")
def local_psf_render_bwd(img: torch.Tensor, psf: torch.Tensor, dy: torch.Tensor, ks: int, need_img: bool,
                         need_psf: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    B, Cn, H, W = img.shape
    x, p, g = _f32(img), _f32(psf), _f32(dy)
    d_img, d_psf = _grad_pair(x, p, need_img, need_psf)
    with torch.cuda.device(x.device):
        _abi.call("aadff_local_psf_render_bwd", _ptr(x), _ptr(p), _ptr(g), _opt(d_img), _opt(d_psf), B, Cn, H, W, ks, _st(x))
    return d_img, d_psf


@_fake(_map_stack_out)
@custom_op("aadff::render_psf_map_stack_diff", mutates_args=(), device_types="cuda")
def render_psf_map_stack_diff(img: torch.Tensor, psf_maps: torch.Tensor, grid: int) -> torch.Tensor:
    """render_psf_map_stack with an autograd formula (image and PSF maps); the forward is the same ABI call."""
    return _map_stack_forward(img, psf_maps, grid)


@_fake(_image_like)
@custom_op("aadff::local_psf_render_diff", mutates_args=(), device_types="cuda")
def local_psf_render_diff(img: torch.Tensor, psf: torch.Tensor, ks: int) -> torch.Tensor:
    """local_psf_render with an autograd formula (image and per-pixel PSFs); the forward is the same ABI call."""
    return _local_forward(img, psf, ks)


def _conv_backward(bwd_op):
    def backward(ctx, dy):
        need = ctx.needs_input_grad[:2]
        return _grads(ctx, need, bwd_op(*ctx.saved_tensors, dy, *ctx.consts, *need), ctx.saved_tensors)
    return backward


render_psf_map_stack_diff.register_autograd(_conv_backward(torch.ops.aadff.render_psf_map_stack_bwd), setup_context=_save_first(2))
local_psf_render_diff.register_autograd(_conv_backward(torch.ops.aadff.local_psf_render_bwd), setup_context=_save_first(2))


# ---------------------------------------------------------------- PSF network (deeplens/psfnet.py:375-441)
def _ints(v):
    return (C.c_int * len(v))(*v)


def _psfnet_out(inp, wpack, bias, in_features, out_features, *_):
    return inp.new_empty((inp.numel() // 4, out_features[-1]), dtype=torch.float32)


@_fake(_psfnet_out)
@custom_op("aadff::psfnet_forward", mutates_args=("flags",), device_types="cuda")
def psfnet_forward(inp: torch.Tensor, wpack: torch.Tensor, bias: torch.Tensor, in_features: List[int], out_features: List[int],
                   flags: torch.Tensor, precision: int = 0) -> torch.Tensor:
    x = _f32(inp).reshape(-1, 4)
    out = _psfnet_out(x, wpack, bias, in_features, out_features)
    with torch.cuda.device(x.device):
        _abi.call("aadff_psfnet_forward", _ptr(x), x.shape[0], _ptr(wpack), _ptr(bias), len(in_features), _ints(in_features),
                  _ints(out_features), 0, _ptr(out), None, None, 0, 0, 0, 0, 0, int(precision), _ptr(flags), _st(x))
    return out


def _rgbd_out(img, depth, xs, ys, foc_z, *_):
    N, Cn, H, W = img.shape
    return img.new_empty((N, Cn, foc_z.numel() // N, H, W), dtype=torch.float32)


def _rgbd_forward(out, img, depth, xs, ys, foc_z, d_min, inv_range, wpack, bias, in_features, out_features, ks, flags, precision):
    N, Cn, H, W = img.shape
    S = foc_z.numel() // N
    x, d, fz = _f32(img), _f32(depth), _f32(foc_z)
    with torch.cuda.device(x.device):
        _abi.call("aadff_psfnet_render_rgbd", _ptr(d), _ptr(_f32(xs)), _ptr(_f32(ys)), _ptr(fz), C.c_float(d_min), C.c_float(inv_range), N, S,
                  _ptr(wpack), _ptr(bias), len(in_features), _ints(in_features), _ints(out_features), _ptr(x), _ptr(out), Cn, H, W, ks,
                  int(precision), _ptr(flags), _st(x))
    return out


@_fake(_rgbd_out)
@custom_op("aadff::psfnet_render_rgbd", mutates_args=("flags",), device_types="cuda")
def psfnet_render_rgbd(img: torch.Tensor, depth: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, foc_z: torch.Tensor, d_min: float,
                       inv_range: float, wpack: torch.Tensor, bias: torch.Tensor, in_features: List[int], out_features: List[int],
                       ks: int, flags: torch.Tensor, precision: int = 0) -> torch.Tensor:
    return _rgbd_forward(_rgbd_out(img, depth, xs, ys, foc_z), img, depth, xs, ys, foc_z, d_min, inv_range, wpack, bias, in_features,
                         out_features, ks, flags, precision)


# ---------------------------------------------------------------- differentiable RGB-D render (csrc/psfnet_bwd.hip)
def psfnet_bwd_workspace_bytes(N, S, Cn, H, W, ks, need_input, need_img):
    """Bytes of device workspace aadff_psfnet_render_rgbd_bwd needs (host arithmetic, no GPU)."""
    return _abi.query_bytes("aadff_psfnet_render_rgbd_bwd_workspace", N, S, Cn, H, W, ks, int(need_input), int(need_img))


def _rgbd_bwd_out(img, depth, xs, ys, foc_z, dy, d_min, inv_range, wpack, bias, wtpack, wt_exp, in_features, out_features, ks, need_img,
                  need_depth, need_foc):
    N, Cn, H, W = img.shape
    return _like(img, need_img), _new(img, (N, H, W), need_depth), _new(img, (N, foc_z.numel() // N), need_foc)


@_fake(_rgbd_bwd_out)
@custom_op("aadff::psfnet_render_rgbd_bwd", mutates_args=(), device_types="cuda")
def psfnet_render_rgbd_bwd(img: torch.Tensor, depth: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, foc_z: torch.Tensor, dy: torch.Tensor,
                           d_min: float, inv_range: float, wpack: torch.Tensor, bias: torch.Tensor, wtpack: torch.Tensor, wt_exp: List[int],
                           in_features: List[int], out_features: List[int], ks: int, need_img: bool, need_depth: bool,
                           need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d_img [N,C,H,W], d_depth [N,H,W], d_foc_z [N,S]) of psfnet_render_rgbd; a gradient that is not needed is not computed and comes
    back empty.  Workspace: 4 bytes per (n, slice, pixel) for d_depth / d_foc_z, the PSFs of ONE slice for d_img."""
    N, Cn, H, W = img.shape
    S = foc_z.numel() // N
    x, d, fz, g = _f32(img), _f32(depth), _f32(foc_z), _f32(dy)
    d_img, d_depth, d_foc = _rgbd_bwd_out(x, d, xs, ys, fz, g, d_min, inv_range, wpack, bias, wtpack, wt_exp, in_features, out_features, ks,
                                          need_img, need_depth, need_foc)
    with torch.cuda.device(x.device):
        nbytes = psfnet_bwd_workspace_bytes(N, S, Cn, H, W, ks, need_depth or need_foc, need_img)
        ws = _workspace(x, nbytes)
        _abi.call("aadff_psfnet_render_rgbd_bwd", _ptr(d), _ptr(_f32(xs)), _ptr(_f32(ys)), _ptr(fz), C.c_float(d_min), C.c_float(inv_range), N, S,
                  _ptr(wpack), _ptr(bias), _ptr(wtpack), _ints(wt_exp), len(in_features), _ints(in_features), _ints(out_features), _ptr(x),
                  _ptr(g), Cn, H, W, ks, _opt(d_img), _opt(d_depth), _opt(d_foc), _ptr(ws), C.c_size_t(nbytes), _st(x))
    return d_img, d_depth, d_foc


def _rgbd_diff_out(img, depth, xs, ys, foc_z, *_):
    return _rgbd_out(img, depth, xs, ys, foc_z), img.new_zeros((1,), dtype=torch.int32)


@_fake(_rgbd_diff_out)
@custom_op("aadff::psfnet_render_rgbd_diff", mutates_args=(), device_types="cuda")
def psfnet_render_rgbd_diff(img: torch.Tensor, depth: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, foc_z: torch.Tensor, d_min: float,
                            inv_range: float, wpack: torch.Tensor, bias: torch.Tensor, wtpack: torch.Tensor, wt_exp: List[int],
                            in_features: List[int], out_features: List[int], ks: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """psfnet_render_rgbd (fp32-equivalent mode) with an autograd formula for img [N,C,H,W], depth [N,H,W] and foc_z [N,S]; the forward
    is the same ABI call.  The network weights (wpack, bias, wtpack) get no gradient.  Returns (out [N,C,S,H,W], flags int32[1]): an op
    with an autograd formula cannot write into an argument, so the kernel's saturation flag (bit 4) comes back as a second result."""
    out, flags = _rgbd_diff_out(img, depth, xs, ys, foc_z)
    return _rgbd_forward(out, img, depth, xs, ys, foc_z, d_min, inv_range, wpack, bias, in_features, out_features, ks, flags, 0), flags


def _rgbd_setup(ctx, inputs, output):
    img, depth, xs, ys, foc_z, d_min, inv_range, wpack, bias, wtpack, wt_exp, in_features, out_features, ks = inputs
    ctx.save_for_backward(img, depth, xs, ys, foc_z, wpack, bias, wtpack)
    ctx.consts = (d_min, inv_range, list(wt_exp), list(in_features), list(out_features), ks)


def _rgbd_backward(ctx, dy, _dflags):
    img, depth, xs, ys, foc_z, wpack, bias, wtpack = ctx.saved_tensors
    d_min, inv_range, wt_exp, ins, outs, ks = ctx.consts
    need = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[4]
    grads = torch.ops.aadff.psfnet_render_rgbd_bwd(img, depth, xs, ys, foc_z, dy, d_min, inv_range, wpack, bias, wtpack, wt_exp, ins, outs, ks, *need)
    return _grads(ctx, need, grads, (img, depth, foc_z), at=(0, 1, 4))


psfnet_render_rgbd_diff.register_autograd(_rgbd_backward, setup_context=_rgbd_setup)


# ---------------------------------------------------------------- differentiable thin-lens baseline (csrc/thinlens.hip)
def _thin_stack_out(img, depth, foc_dists, *_):
    N, Cn, H, W = img.shape
    return img.new_empty((N, Cn, foc_dists.numel() // N, H, W), dtype=torch.float32)


def _thin_stack_forward(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max):
    N, Cn, H, W = img.shape
    S = foc_dists.numel() // N
    x, d, fd, neg = _thin_inputs(img, depth, foc_dists, N, S)
    out = _thin_stack_out(x, d, fd)
    with torch.cuda.device(x.device):
        _abi.call("aadff_thinlens_render_stack", _ptr(x), _ptr(d), _ptr(fd), _ptr(neg), _ptr(out), N, Cn, S, H, W, ks,
                  *_thin_args(foc_len, fnum, pixel_size, d_min, d_max), _st(x))
    return out


@_fake(_thin_stack_out)
@custom_op("aadff::thinlens_render_stack", mutates_args=(), device_types="cuda")
def thinlens_render_stack(img: torch.Tensor, depth: torch.Tensor, foc_dists: torch.Tensor, ks: int, foc_len: float, fnum: float,
                          pixel_size: float, d_min: float, d_max: float) -> torch.Tensor:
    """thinlens_render for foc_dists [N,S] -> [N,C,S,H,W]; slice s is bit-equal to thinlens_render(..., foc_dists[:, s])."""
    return _thin_stack_forward(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max)


def thinlens_bwd_workspace_bytes(N, Cn, S, H, W, ks, need_img, need_foc):
    """Bytes of device workspace aadff_thinlens_render_stack_bwd needs (host arithmetic, no GPU):
    4 * ((2 * N*S*H*W if need_img) + (N*S*H*ceil(W/64) if need_foc))."""
    return _abi.query_bytes("aadff_thinlens_render_stack_bwd_workspace", N, Cn, S, H, W, ks, int(need_img), int(need_foc))


def _thin_bwd_out(img, depth, foc_dists, dy, ks, foc_len, fnum, pixel_size, d_min, d_max, need_img, need_depth, need_foc):
    N, Cn, H, W = img.shape
    return _like(img, need_img), _new(img, (N, 1, H, W), need_depth), _new(img, (N, foc_dists.numel() // N), need_foc)


@_fake(_thin_bwd_out)
@custom_op("aadff::thinlens_render_stack_bwd", mutates_args=(), device_types="cuda")
def thinlens_render_stack_bwd(img: torch.Tensor, depth: torch.Tensor, foc_dists: torch.Tensor, dy: torch.Tensor, ks: int, foc_len: float,
                              fnum: float, pixel_size: float, d_min: float, d_max: float, need_img: bool, need_depth: bool,
                              need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d_img [N,C,H,W], d_depth [N,1,H,W], d_foc [N,S]) of thinlens_render_stack; a gradient that is not needed is not computed and
    comes back empty.  Workspace: 8 bytes per (n, slice, pixel) for d_img, 4 bytes per 64-pixel run and slice for d_foc."""
    N, Cn, H, W = img.shape
    S = foc_dists.numel() // N
    x, d, fd, neg = _thin_inputs(img, depth, foc_dists, N, S)
    g = _f32(dy)
    d_img, d_depth, d_foc = _thin_bwd_out(x, d, fd, g, ks, foc_len, fnum, pixel_size, d_min, d_max, need_img, need_depth, need_foc)
    with torch.cuda.device(x.device):
        nbytes = thinlens_bwd_workspace_bytes(N, Cn, S, H, W, ks, need_img, need_foc)
        ws = _workspace(x, nbytes)
        _abi.call("aadff_thinlens_render_stack_bwd", _ptr(x), _ptr(d), _ptr(fd), _ptr(neg), _ptr(g), _opt(d_img), _opt(d_depth), _opt(d_foc),
                  _ptr(ws), C.c_size_t(nbytes), N, Cn, S, H, W, ks, *_thin_args(foc_len, fnum, pixel_size, d_min, d_max), _st(x))
    return d_img, d_depth, d_foc


@_fake(_thin_stack_out)
@custom_op("aadff::thinlens_render_stack_diff", mutates_args=(), device_types="cuda")
def thinlens_render_stack_diff(img: torch.Tensor, depth: torch.Tensor, foc_dists: torch.Tensor, ks: int, foc_len: float, fnum: float,
                               pixel_size: float, d_min: float, d_max: float) -> torch.Tensor:
    """thinlens_render_stack with an autograd formula for img [N,C,H,W], depth [N,1,H,W] and foc_dists [N,S]; the forward is the same
    ABI call."""
    return _thin_stack_forward(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max)


def _thin_backward(ctx, dy):
    need = ctx.needs_input_grad[:3]
    return _grads(ctx, need, torch.ops.aadff.thinlens_render_stack_bwd(*ctx.saved_tensors, dy, *ctx.consts, *need), ctx.saved_tensors)


thinlens_render_stack_diff.register_autograd(_thin_backward, setup_context=_save_first(3))


# ---------------------------------------------------------------- depth from a focal stack (csrc/dfocus.hip)
def _dfocus_out(stack, coords, window, interp, eps, want_aif, want_volume):
    N, Cn, S, H, W = stack.shape
    return (_new(stack, (N, 1, H, W)), _new(stack, (N, 1, H, W), dtype=torch.int32), _new(stack, (N, 1, H, W)),
            _new(stack, (N, Cn, H, W), want_aif), _new(stack, (N, S, H, W), want_volume))


@_fake(_dfocus_out)
@custom_op("aadff::depth_from_stack", mutates_args=(), device_types="cuda")
def depth_from_stack(stack: torch.Tensor, coords: torch.Tensor, window: int, interp: str, eps: float, want_aif: bool,
                     want_volume: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor, torch.Tensor]:
    """(depth [N,1,H,W], index [N,1,H,W] int32, peak [N,1,H,W], aif [N,C,H,W], volume [N,S,H,W]) of stack [N,C,S,H,W] over the slice
    abscissae coords [N,S]: window-summed modified Laplacian, first argmax over the slices, three-point fit (`interp` none / parabola /
    gaussian) in one launch.  An output that is not wanted is not written and comes back empty.  No autograd formula:
    the argmax has no gradient."""
    N, Cn, S, H, W = stack.shape
    if interp not in _abi.DFOCUS_INTERP:
        raise ValueError(f"depth_from_stack: interp {interp!r} is not one of {sorted(_abi.DFOCUS_INTERP)}")
    x, u = _f32(stack), _f32(coords).reshape(N, S)
    depth, index, peak, aif, volume = _dfocus_out(x, u, window, interp, eps, want_aif, want_volume)
    with torch.cuda.device(x.device):
        _abi.call("aadff_depth_from_stack", _ptr(x), _ptr(u), _ptr(depth), _ptr(index), _ptr(peak), _opt(aif), _opt(volume), N, Cn, S, H, W,
                  window, _abi.DFOCUS_INTERP[interp], C.c_float(eps), _st(x))
    return depth, index, peak, aif, volume


# ---------------------------------------------------------------- differentiable depth head and loss (csrc/focus_head.hip)
def _head_dims(scores, stack, aif_channels):
    N, K, S, H, W = scores.shape
    return N, K, stack.shape[1], aif_channels, S, H, W


def attention_bwd_workspace_bytes(N, S, H, W):
    """Bytes of device workspace aadff_attention_depth_bwd needs for d_foc: one float per wave and slice (include/aadff.h)."""
    return 4 * N * S * 4 * ((H * ((W + 3) // 4) + 255) // 256)


def _head_out(scores, stack, foc_dists, normalize_attention, aif_channels):
    N, K, S, H, W = scores.shape
    return _new(scores, (N, 1, H, W)), _new(scores, (N, aif_channels, H, W))


@_fake(_head_out)
@custom_op("aadff::attention_depth", mutates_args=(), device_types="cuda")
def attention_depth(scores: torch.Tensor, stack: torch.Tensor, foc_dists: torch.Tensor, normalize_attention: bool,
                    aif_channels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(depth [N,1,H,W], aif [N,Ca,H,W]) of scores [N,K,S,H,W] (K 1 or 2), stack [N,Ct,S,H,W] and foc_dists [N,S]: softmax or
    normalised-softplus attention over the slices, expectation of the focus distances and attention-weighted composite of the first
    Ca = aif_channels channels of the stack, in one launch.  Autograd formula for scores, stack and foc_dists."""
    N, K, Ct, Ca, S, H, W = _head_dims(scores, stack, aif_channels)
    z, x, fd = _f32(scores), _f32(stack), _f32(foc_dists).reshape(N, S)
    depth, aif = _head_out(z, x, fd, normalize_attention, aif_channels)
    with torch.cuda.device(z.device):
        _abi.call("aadff_attention_depth", _ptr(z), _ptr(x), _ptr(fd), _ptr(depth), _ptr(aif), N, K, Ct, Ca, S, H, W,
                  int(normalize_attention), _st(z))
    return depth, aif


def _head_bwd_out(scores, stack, foc_dists, g_depth, g_aif, normalize_attention, aif_channels, need_scores, need_stack, need_foc):
    return (_like(scores, need_scores), _like(stack, need_stack),
            _new(scores, (scores.shape[0], scores.shape[2]), need_foc))


@_fake(_head_bwd_out)
@custom_op("aadff::attention_depth_bwd", mutates_args=(), device_types="cuda")
def attention_depth_bwd(scores: torch.Tensor, stack: torch.Tensor, foc_dists: torch.Tensor, g_depth: torch.Tensor, g_aif: torch.Tensor,
                        normalize_attention: bool, aif_channels: int, need_scores: bool, need_stack: bool,
                        need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d_scores [N,K,S,H,W], d_stack [N,Ct,S,H,W], d_foc [N,S]) of attention_depth; the attention is recomputed from the scores.  A
    gradient that is not needed is not computed and comes back empty; the others do not depend on that."""
    N, K, Ct, Ca, S, H, W = _head_dims(scores, stack, aif_channels)
    z, x, fd = _f32(scores), _f32(stack), _f32(foc_dists).reshape(N, S)
    gd, ga = _f32(g_depth), _f32(g_aif)
    d_z, d_x, d_fd = _head_bwd_out(z, x, fd, gd, ga, normalize_attention, aif_channels, need_scores, need_stack, need_foc)
    nbytes = attention_bwd_workspace_bytes(N, S, H, W) if need_foc else 0
    ws = _workspace(z, nbytes) if need_foc else None
    with torch.cuda.device(z.device):
        _abi.call("aadff_attention_depth_bwd", _ptr(z), _ptr(x), _ptr(fd), _ptr(gd), _ptr(ga), _opt(d_z), _opt(d_x), _opt(d_fd),
                  _ptr(ws), C.c_size_t(nbytes), N, K, Ct, Ca, S, H, W, int(normalize_attention), _st(z))
    return d_z, d_x, d_fd


def _head_backward(ctx, g_depth, g_aif):
    need = ctx.needs_input_grad[:3]
    return _grads(ctx, need, torch.ops.aadff.attention_depth_bwd(*ctx.saved_tensors, g_depth, g_aif, *ctx.consts, *need), ctx.saved_tensors)


attention_depth.register_autograd(_head_backward, setup_context=_save_first(3))


def _loss_dims(depth, aif, gt_depth, gt_aif):
    hw = lambda t: (t.shape[-2], t.shape[-1]) if t.numel() else (0, 0)      # noqa: E731
    Ca = aif.shape[1] if aif.numel() else (gt_aif.shape[1] if gt_aif.numel() else 0)
    return (depth.shape[0], Ca, *hw(depth), *hw(aif), *hw(gt_depth), *hw(gt_aif))


def _loss_out(depth, *_):
    return _new(depth, (6,), dtype=torch.float64)


@_fake(_loss_out)
@custom_op("aadff::dff_loss_sums", mutates_args=(), device_types="cuda")
def dff_loss_sums(depth: torch.Tensor, aif: torch.Tensor, gt_depth: torch.Tensor, gt_aif: torch.Tensor, mask_range: torch.Tensor) -> torch.Tensor:
    """The six float64 sums of the depth-from-focus loss over the common top-left window of depth [N,1,Hd,Wd], aif [N,Ca,Ha,Wa],
    gt_depth [N,1,Hg,Wg] and gt_aif [N,Ca,Hi,Wi]: (sum_mask |e|, |mask|, sum_mask e^2, sum |aif - gt_aif|, sum wx r(d_gx), sum wy r(d_gy)).
    An empty tensor stands for one that is absent (aif and gt_aif go together); mask_range: the two floats {lo, hi} of the range mask or
    empty for gt_depth > 0.  Autograd formula for depth and aif (include/aadff.h)."""
    d, a, gd, ga, rng = _f32(depth), _f32(aif), _f32(gt_depth), _f32(gt_aif), _f32(mask_range)
    dims = _loss_dims(d, a, gd, ga)
    sums = _loss_out(d)
    nbytes = 48 * ((dims[0] * dims[2] * dims[3] + 1023) // 1024)
    ws = _workspace(d, nbytes, torch.float64)
    with torch.cuda.device(d.device):
        _abi.call("aadff_dff_loss_sums", _ptr(d), _opt(a), _opt(gd), _opt(ga), _opt(rng), _ptr(sums), _ptr(ws), C.c_size_t(nbytes), *dims, _st(d))
    return sums


@_fake(lambda depth, aif, gt_depth, gt_aif, mask_range, g_sums, need_depth, need_aif: _grad_pair(depth, aif, need_depth, need_aif))
@custom_op("aadff::dff_loss_bwd", mutates_args=(), device_types="cuda")
def dff_loss_bwd(depth: torch.Tensor, aif: torch.Tensor, gt_depth: torch.Tensor, gt_aif: torch.Tensor, mask_range: torch.Tensor,
                 g_sums: torch.Tensor, need_depth: bool, need_aif: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_depth, d_aif) of dff_loss_sums for the cotangents g_sums [6] of its sums, in the shapes of depth and aif, zero outside the
    window.  A gradient that is not needed is not computed and comes back empty."""
    d, a, gd, ga, rng = _f32(depth), _f32(aif), _f32(gt_depth), _f32(gt_aif), _f32(mask_range)
    g = g_sums.contiguous().double()
    d_d, d_a = _grad_pair(d, a, need_depth, need_aif)
    with torch.cuda.device(d.device):
        _abi.call("aadff_dff_loss_bwd", _ptr(d), _opt(a), _opt(gd), _opt(ga), _opt(rng), _ptr(g), _opt(d_d), _opt(d_a),
                  *_loss_dims(d, a, gd, ga), _st(d))
    return d_d, d_a


def _loss_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _loss_backward(ctx, g_sums):
    depth, aif = ctx.saved_tensors[:2]
    need = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and aif.numel() > 0
    if not any(need):
        return _no_grads(ctx)
    return _grads(ctx, need, torch.ops.aadff.dff_loss_bwd(*ctx.saved_tensors, g_sums, *need), (depth, aif))


dff_loss_sums.register_autograd(_loss_backward, setup_context=_loss_setup)


# ---------------------------------------------------------------- cost-volume depth head (csrc/dfv_head.hip)
def dfv_bwd_tiling(w, W):
    """(TC, R): the cells of a cost row and the output rows one workgroup of the backward's first stage owns (include/aadff.h)."""
    ratio = -(-W // w)
    tc = min(max(240 // ratio - 1, 1), 8)
    return tc, min(max(256 // ((tc + 1) * ratio + 1), 1), 8)


def dfv_bwd_workspace_bytes(B, S, h, w, H, W, need_cost=True, need_foc=True):
    """Bytes of device workspace aadff_dfv_head_bwd needs: the row sums [B,S,H,w] for d_cost and one partial per slice and workgroup
    for d_foc (include/aadff.h)."""
    tc, r = dfv_bwd_tiling(w, W)
    return 4 * B * S * ((H * w if need_cost else 0) + (-(-H // r) * -(-w // tc) if need_foc else 0))


def _dfv_out(cost, foc_dists, height, width, want_prob):
    B, S = cost.shape[0], cost.shape[1]
    return _new(cost, (B, 1, height, width)), _new(cost, (B, 1, height, width)), _new(cost, (B, S, height, width), want_prob)


@_fake(_dfv_out)
@custom_op("aadff::dfv_regress", mutates_args=(), device_types="cuda")
def dfv_regress(cost: torch.Tensor, foc_dists: torch.Tensor, height: int, width: int,
                want_prob: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pred [B,1,H,W], std [B,1,H,W], prob [B,S,H,W] or empty) of cost [B,S,h,w] and foc_dists [B,S]: bilinear upsampling to
    height x width (ATen's align_corners = False), softmax over the slices, expectation of the focus distances and its standard
    deviation in one launch.  Autograd formula for cost and foc_dists through pred; std and prob carry no graph."""
    B, S, h, w = cost.shape
    c, fd = _f32(cost), _f32(foc_dists).reshape(B, S)
    pred, std, prob = _dfv_out(c, fd, height, width, want_prob)
    with torch.cuda.device(c.device):
        _abi.call("aadff_dfv_head_fwd", _ptr(c), _ptr(fd), _ptr(pred), _ptr(std), _opt(prob), B, S, h, w, height, width, _st(c))
    return pred, std, prob


def _dfv_bwd_out(cost, foc_dists, g_pred, need_cost, need_foc):
    return _like(cost, need_cost), _new(cost, (cost.shape[0], cost.shape[1]), need_foc)


@_fake(_dfv_bwd_out)
@custom_op("aadff::dfv_regress_bwd", mutates_args=(), device_types="cuda")
def dfv_regress_bwd(cost: torch.Tensor, foc_dists: torch.Tensor, g_pred: torch.Tensor, need_cost: bool,
                    need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_cost [B,S,h,w], d_foc [B,S]) of dfv_regress for the cotangent g_pred [B,1,H,W]; the softmax is recomputed from the cost.  A
    gradient that is not needed is not computed and comes back empty; the other does not depend on that."""
    B, S, h, w = cost.shape
    H, W = g_pred.shape[-2], g_pred.shape[-1]
    c, fd, g = _f32(cost), _f32(foc_dists).reshape(B, S), _f32(g_pred)
    d_c, d_fd = _dfv_bwd_out(c, fd, g, need_cost, need_foc)
    nbytes = dfv_bwd_workspace_bytes(B, S, h, w, H, W, need_cost, need_foc)
    ws = _workspace(c, nbytes)
    with torch.cuda.device(c.device):
        _abi.call("aadff_dfv_head_bwd", _ptr(c), _ptr(fd), _ptr(g), _opt(d_c), _opt(d_fd), _ptr(ws), C.c_size_t(nbytes), B, S, h, w, H, W, _st(c))
    return d_c, d_fd


def _dfv_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs[:2])
    ctx.mark_non_differentiable(output[1], output[2])          # std is computed under no_grad in the reference; prob is its eval output


def _dfv_backward(ctx, g_pred, g_std, g_prob):
    need = ctx.needs_input_grad[:2]
    if not any(need):
        return _no_grads(ctx)
    return _grads(ctx, need, torch.ops.aadff.dfv_regress_bwd(*ctx.saved_tensors, g_pred, *need), ctx.saved_tensors)


dfv_regress.register_autograd(_dfv_backward, setup_context=_dfv_setup)


# ---------------------------------------------------------------- confidence-guided depth refinement (csrc/depth_refine.hip)
def depth_refine_constants(channels, sigma_space, sigma_range):
    """(ks, kr) = (1 / (2 sigma_space^2), 1 / (2 sigma_range^2 C)), formed in float64 and rounded to the float32 values the kernels get."""
    return (C.c_float(1.0 / (2.0 * float(sigma_space) ** 2)).value, C.c_float(1.0 / (2.0 * float(sigma_range) ** 2 * channels)).value)


def depth_refine_bwd_workspace_bytes(N, H, W):
    """Bytes of device workspace aadff_depth_refine_bwd needs: alpha, u', beta and the pass-through term, [N,H,W] each."""
    return 16 * N * H * W


def _refine_out(u, c, *_):
    return torch.empty_like(u), torch.empty_like(c)


@_fake(_refine_out)
@custom_op("aadff::depth_refine", mutates_args=(), device_types="cuda")
def depth_refine(u: torch.Tensor, c: torch.Tensor, g: torch.Tensor, radius: int, sigma_space: float,
                 sigma_range: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u' [N,1,H,W], c' [N,1,H,W]): one iteration of the confidence-weighted joint bilateral filter of u [N,1,H,W] with confidence
    c [N,1,H,W] and guide g [N,C,H,W], C in 1..4, over the clipped (2 radius + 1)^2 window.  Autograd formula for u and
    c; the guide is a constant."""
    N, Cn, H, W = g.shape
    x, cc, gg = _f32(u), _f32(c), _f32(g)
    ks, kr = depth_refine_constants(Cn, sigma_space, sigma_range)
    u_out, c_out = _refine_out(x, cc)
    with torch.cuda.device(x.device):
        _abi.call("aadff_depth_refine_fwd", _ptr(x), _ptr(cc), _ptr(gg), _ptr(u_out), _ptr(c_out), N, Cn, H, W, radius, ks, kr, _st(x))
    return u_out, c_out


@_fake(lambda u, c, g, g_u, g_c, radius, sigma_space, sigma_range, need_u, need_c: _grad_pair(u, c, need_u, need_c))
@custom_op("aadff::depth_refine_bwd", mutates_args=(), device_types="cuda")
def depth_refine_bwd(u: torch.Tensor, c: torch.Tensor, g: torch.Tensor, g_u: torch.Tensor, g_c: torch.Tensor, radius: int,
                     sigma_space: float, sigma_range: float, need_u: bool, need_c: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_u, d_c) [N,1,H,W] of depth_refine for the cotangents g_u, g_c of its two outputs; the sums of the forward are recomputed.  A
    gradient that is not needed is not written and comes back empty; the other does not depend on that."""
    N, Cn, H, W = g.shape
    x, cc, gg, gu, gc = _f32(u), _f32(c), _f32(g), _f32(g_u), _f32(g_c)
    ks, kr = depth_refine_constants(Cn, sigma_space, sigma_range)
    d_u, d_c = _grad_pair(x, cc, need_u, need_c)
    nbytes = depth_refine_bwd_workspace_bytes(N, H, W)
    ws = _workspace(x, nbytes)
    with torch.cuda.device(x.device):
        _abi.call("aadff_depth_refine_bwd", _ptr(x), _ptr(cc), _ptr(gg), _ptr(gu), _ptr(gc), _opt(d_u), _opt(d_c), _ptr(ws), C.c_size_t(nbytes),
                  N, Cn, H, W, radius, ks, kr, _st(x))
    return d_u, d_c


def _refine_backward(ctx, g_u, g_c):
    need = ctx.needs_input_grad[:2]
    if not any(need):
        return _no_grads(ctx)
    return _grads(ctx, need, torch.ops.aadff.depth_refine_bwd(*ctx.saved_tensors, g_u, g_c, *ctx.consts, *need), ctx.saved_tensors)


depth_refine.register_autograd(_refine_backward, setup_context=_save_first(3))


# ---------------------------------------------------------------- evaluation metrics (csrc/metrics.hip)
def depth_metric_workspace_bytes(N, H, W):
    """Bytes of device workspace aadff_depth_metric_sums needs: one row of 16 doubles per workgroup of 1024 pixels (include/aadff.h)."""
    return 128 * N * (((H * W + 3) // 4 + 255) // 256)


def image_metric_workspace_bytes(N, Cn, H, W, ssim):
    """Bytes of device workspace aadff_image_metric_sums needs: an int64 and a double per workgroup - per channel and 32 x 64 tile of
    windows with SSIM, per 1024 values without (include/aadff.h)."""
    if ssim:
        return 16 * N * Cn * ((H - 6 + _abi.SSIM_TILE_H - 1) // _abi.SSIM_TILE_H) * ((W - 6 + _abi.SSIM_TILE_W - 1) // _abi.SSIM_TILE_W)
    return 16 * N * (((Cn * H * W + 3) // 4 + 255) // 256)


def _depth_metric_out(est, *_):
    return _new(est, (est.shape[0], _abi.DEPTH_METRIC_COLS), dtype=torch.float64)


@_fake(_depth_metric_out)
@custom_op("aadff::depth_metric_sums", mutates_args=(), device_types="cuda")
def depth_metric_sums(est: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, conf: torch.Tensor, valid_mode: str) -> torch.Tensor:
    """sums [N,16] float64 of est, gt [N,1,H,W] in one pass: count, the error sums, the three threshold counts, the confidence-weighted
    sums and the counts of "finite" mode, one row per image (column numbering: include/aadff.h).  mask [N,1,H,W] bool
    and conf [N,1,H,W]: an empty tensor stands for one that is absent.  valid_mode "mask" or "finite".  No autograd formula: the output
    carries no graph."""
    if valid_mode not in _abi.VALID_MODES:
        raise ValueError(f"depth_metric_sums: valid_mode {valid_mode!r} is not one of {sorted(_abi.VALID_MODES)}")
    e, g = _f32(est.detach()), _f32(gt.detach())
    N, H, W = e.shape[0], e.shape[-2], e.shape[-1]
    m = mask.contiguous() if mask.numel() else None
    if m is not None and m.dtype != torch.bool:
        m = m != 0
    c = _f32(conf.detach())
    sums = _depth_metric_out(e)
    nbytes = depth_metric_workspace_bytes(N, H, W)
    ws = _workspace(e, nbytes, torch.float64)
    with torch.cuda.device(e.device):
        _abi.call("aadff_depth_metric_sums", _ptr(e), _ptr(g), _ptr(m), _opt(c), _ptr(sums), _ptr(ws), C.c_size_t(nbytes),
                  N, H, W, _abi.VALID_MODES[valid_mode], _st(e))
    return sums


def _image_metric_out(pred, *_):
    return _new(pred, (pred.shape[0], 2), dtype=torch.float64)


@_fake(_image_metric_out)
@custom_op("aadff::image_metric_sums", mutates_args=(), device_types="cuda")
def image_metric_sums(pred: torch.Tensor, target: torch.Tensor, ssim: bool) -> torch.Tensor:
    """sums [N,2] float64 of pred, target [N,C,H,W] (C in 1..4) quantised to bytes as the reference's batch_PSNR does: the exact sum of
    squared differences and, with `ssim`, the sum of the SSIM index over all full 7 x 7 windows and channels (else 0).  No autograd
    formula: the output carries no graph."""
    x, y = _f32(pred.detach()), _f32(target.detach())
    N, Cn, H, W = x.shape
    sums = _image_metric_out(x)
    nbytes = image_metric_workspace_bytes(N, Cn, H, W, ssim) if (not ssim or (H >= 7 and W >= 7)) else 16
    ws = _workspace(x, nbytes, torch.float64)
    with torch.cuda.device(x.device):
        _abi.call("aadff_image_metric_sums", _ptr(x), _ptr(y), _ptr(sums), _ptr(ws), C.c_size_t(nbytes), N, Cn, H, W, int(ssim), _st(x))
    return sums


# scores, not losses: an input that requires a gradient is accepted and the sums carry no graph
def _metric_setup(ctx, inputs, output):
    ctx.mark_non_differentiable(output)


depth_metric_sums.register_autograd(_no_grads, setup_context=_metric_setup)
image_metric_sums.register_autograd(_no_grads, setup_context=_metric_setup)


# ---------------------------------------------------------------- ray trace -> PSFs (deeplens/optics.py:888-1026)
_LC_FIELDS = [f for f, _ in _abi.LensConst._fields_]


def lens_const_to_list(lc):
    return [float(getattr(lc, f)) for f in _LC_FIELDS]


def lens_const_from_list(v):
    lc = _abi.LensConst()
    for f, x in zip(_LC_FIELDS, v):
        setattr(lc, f, int(x) if f == "n_surf" else float(x))
    return lc


def _psf_grid_out(points, lead, N, L, ks, map_layout):
    """PSFs of N field points and L wavelengths behind the leading dimensions `lead`: [N,L,ks,ks] or, with map_layout, [L,g*ks,g*ks]."""
    g = int(round(N ** 0.5))
    return points.new_empty((*lead, L, g * ks, g * ks) if map_layout else (*lead, N, L, ks, ks), dtype=torch.float32)


def _psf_points_out(points, surf_main, surf_chief, lens_const, states, u_main, u_chief, ks, centre, map_layout, flags):
    return _psf_grid_out(points, (points.shape[0],), points.shape[1], u_main.shape[1], ks, map_layout)


@_fake(_psf_points_out)
@custom_op("aadff::psf_points", mutates_args=("flags",), device_types="cuda")
def psf_points(points: torch.Tensor, surf_main: torch.Tensor, surf_chief: torch.Tensor, lens_const: List[float], states: torch.Tensor,
               u_main: torch.Tensor, u_chief: torch.Tensor, ks: int, centre: bool, map_layout: bool, flags: torch.Tensor) -> torch.Tensor:
    """points [S,N,3] normalised field points; surf_* / states: the packed byte tensors of deeplens.optics
    (aadff_surface_t tables per wavelength, aadff_lens_state_t[S]); lens_const: the fields of aadff_lens_const_t in
    declaration order (n_surf first); u_main [S,L,2,spp], u_chief [S,L,2,spp_chief] raw uniforms (u_chief may be empty
    when centre is False) -> [S,N,L,ks,ks] or, with map_layout, [S,L,g*ks,g*ks]."""
    S, N = points.shape[0], points.shape[1]
    L, spp, spc = u_main.shape[1], u_main.shape[3], (u_chief.shape[3] if u_chief.numel() else 0)
    lc = lens_const_from_list(lens_const)
    out = _psf_points_out(points, surf_main, surf_chief, lens_const, states, u_main, u_chief, ks, centre, map_layout, flags)
    pts, um, uc = _f32(points), _f32(u_main), _f32(u_chief)
    with torch.cuda.device(pts.device):
        _abi.call("aadff_psf_points", _ptr(pts), S, N, L, _ptr(surf_main), _ptr(surf_chief), lc, _ptr(states),
                  _ptr(um), spp, 2 * L * spp, 2 * spp, _opt(uc), spc, 2 * L * spc, 2 * spc, ks, int(centre), int(map_layout),
                  _ptr(out), None, _ptr(flags), _st(pts))
    return out


def _psf_block_out(points, surf_main, surf_chief, lens_const, states, u_block, n_wave, spp, spp_chief, ks, map_layout, flags):
    return _psf_grid_out(points, (), points.shape[0], n_wave, ks, map_layout)


@_fake(_psf_block_out)
@custom_op("aadff::psf_points_block", mutates_args=("flags",), device_types="cuda")
def psf_points_block(points: torch.Tensor, surf_main: torch.Tensor, surf_chief: torch.Tensor, lens_const: List[float], states: torch.Tensor,
                     u_block: torch.Tensor, n_wave: int, spp: int, spp_chief: int, ks: int, map_layout: bool, flags: torch.Tensor) -> torch.Tensor:
    """psf_points for ONE focus state with the uniforms as the flat block the host generator produced, in the reference's draw order
    (SURVEY.md Appendix B): per wavelength [main theta spp | main r spp | chief theta spp_chief | chief r spp_chief]; spp_chief = 0:
    no chief rays (center=False).  points [N,3] -> [N,L,ks,ks] or, with map_layout, [L,g*ks,g*ks].  No re-layout copy: the kernel
    takes the rows through strides."""
    N, L = points.shape[0], n_wave
    per_l = 2 * spp + 2 * spp_chief
    lc = lens_const_from_list(lens_const)
    out = _psf_block_out(points, surf_main, surf_chief, lens_const, states, u_block, n_wave, spp, spp_chief, ks, map_layout, flags)
    base = u_block.data_ptr()
    with torch.cuda.device(points.device):
        _abi.call("aadff_psf_points", _ptr(points), 1, N, L, _ptr(surf_main), _ptr(surf_chief), lc, _ptr(states),
                  C.c_void_p(base), spp, L * per_l, per_l, C.c_void_p(base + 8 * spp) if spp_chief else None, spp_chief, L * per_l, per_l, ks,
                  int(spp_chief > 0), int(map_layout), _ptr(out), None, _ptr(flags), _st(points))
    return out
