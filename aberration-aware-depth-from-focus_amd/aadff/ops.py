"""torch custom ops (`torch.ops.aadff.*`) over the C ABI of include/aadff.h.

`north_star` asks for the HIP kernels "through PyTorch-ROCm custom ops": each op below is a thin
`torch.library.custom_op` wrapper (schema + fake/meta shape function) whose implementation packs pointers and calls
libaadff.so on the current HIP stream.  With them the path is visible to FakeTensor / `torch.compile` tracing and
`torch.library.opcheck`; no autograd formula is registered for them — the reference never back-propagates through these
functions, so a backward through them raises torch's "not differentiable" error.  The differentiable
forms of the image-space operators are separate ops (`render_psf_map_stack_diff`, `local_psf_render_diff`, at the end of
the image-space section; public functions in aadff/diffrender.py): same forward kernels, backward in csrc/conv_bwd.hip.
`psfnet_render_rgbd_diff` is the fused RGB-D renderer with gradients to the image, the depth map and foc_z (csrc/psfnet_bwd.hip);
`thinlens_render_stack_diff` is the thin-lens baseline with gradients to the image, the depth map and the focus distances
(csrc/thinlens_bwd.hip).  `depth_from_stack` goes the other way: focal stack -> depth map, the classical estimator (csrc/dfocus.hip;
public function in aadff/dfocus.py).  `attention_depth` and `dff_loss_sums` are the differentiable way back: the attention head over a
stack's scores and the sums of its loss, each with a backward op of its own (csrc/focus_head.hip; public functions in aadff/focus_head.py).
`dfv_regress` is the head of the reference's second network: a low-resolution cost volume upsampled, softmaxed and regressed to depth and
its standard deviation in one kernel, with a gather-form backward (csrc/dfv_head.hip; public functions in aadff/dfv_head.py).
`depth_refine` is the step after any of these estimators: one iteration of a confidence-weighted joint bilateral filter guided by the
all-in-focus image, with a two-pass gather backward to the filtered quantity and its confidence (csrc/depth_refine.hip; public functions
in aadff/refine.py).
`depth_metric_sums` and `image_metric_sums` score the result: the per-image sums behind the reference's depth metrics and PSNR / SSIM
(csrc/metrics.hip; public functions in aadff/metrics.py); their outputs carry no graph.

The deeplens mirror (deeplens/render_psf.py, deeplens/psfnet.py) calls these ops; the multi-launch planners
(aadff/focal_stack.py, aadff/training.py) keep calling the ABI directly because they pass raw offsets into pinned rings.
"""
import ctypes as C
from typing import List, Tuple

import torch
from torch.library import custom_op

from . import _abi


def _st(t):
    return _abi.stream_ptr(t.device)


# ---------------------------------------------------------------- image space (deeplens/render_psf.py:12-107)
@custom_op("aadff::render_psf_map", mutates_args=(), device_types="cuda")
def render_psf_map(img: torch.Tensor, psf_map: torch.Tensor, grid: int) -> torch.Tensor:
    B, Cn, H, W = img.shape
    ks = psf_map.shape[1] // grid
    x, p = img.contiguous().float(), psf_map.contiguous().float()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_render_psf_map", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), B, Cn, H, W, grid, ks, _st(x))
    return out


@render_psf_map.register_fake
def _(img, psf_map, grid):
    return torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format)


@custom_op("aadff::render_psf_map_stack", mutates_args=(), device_types="cuda")
def render_psf_map_stack(img: torch.Tensor, psf_maps: torch.Tensor, grid: int) -> torch.Tensor:
    B, Cn, H, W = img.shape
    S, ks = psf_maps.shape[0], psf_maps.shape[2] // grid
    x, p = img.contiguous().float(), psf_maps.contiguous().float()
    out = torch.empty((B, Cn, S, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_render_psf_map_stack", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), B, Cn, S, H, W, grid, ks, _st(x))
    return out


@render_psf_map_stack.register_fake
def _(img, psf_maps, grid):
    B, Cn, H, W = img.shape
    return img.new_empty((B, Cn, psf_maps.shape[0], H, W), dtype=torch.float32)


@custom_op("aadff::render_psf", mutates_args=(), device_types="cuda")
def render_psf(img: torch.Tensor, psf: torch.Tensor) -> torch.Tensor:
    B, Cn, H, W = img.shape
    x, p = img.contiguous().float(), psf.contiguous().float()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_render_psf", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), B, Cn, H, W, psf.shape[-1], _st(x))
    return out


@render_psf.register_fake
def _(img, psf):
    return torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format)


@custom_op("aadff::local_psf_render", mutates_args=(), device_types="cuda")
def local_psf_render(img: torch.Tensor, psf: torch.Tensor, ks: int) -> torch.Tensor:
    B, Cn, H, W = img.shape
    x, p = img.contiguous().float(), psf.contiguous().float()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_local_psf_render", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), B, Cn, H, W, ks, _st(x))
    return out


@local_psf_render.register_fake
def _(img, psf, ks):
    return torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format)


@custom_op("aadff::thinlens_render", mutates_args=(), device_types="cuda")
def thinlens_render(img: torch.Tensor, depth: torch.Tensor, foc_dist: torch.Tensor, ks: int, foc_len: float, fnum: float,
                    pixel_size: float, d_min: float, d_max: float) -> torch.Tensor:
    N, Cn, H, W = img.shape
    x, d, fd = img.contiguous().float(), depth.contiguous().float().reshape(N, 1, H, W), foc_dist.contiguous().float().reshape(N)
    neg = (d < 0).any().to(torch.int32).reshape(1)              # the reference's whole-tensor sign test, kept on the device
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_thinlens_render", _abi.ptr(x), _abi.ptr(d), _abi.ptr(fd), _abi.ptr(neg), _abi.ptr(out), N, Cn, H, W, ks,
                  C.c_float(foc_len / fnum), C.c_float(foc_len), C.c_float(1.0 / pixel_size), C.c_float(d_min), C.c_float(d_max), _st(x))
    return out


@thinlens_render.register_fake
def _(img, depth, foc_dist, ks, foc_len, fnum, pixel_size, d_min, d_max):
    return torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format)


# ---------------------------------------------------------------- differentiable image space (csrc/conv_bwd.hip)
# Plain (non-differentiable) ops over the backward ABI, and front ops whose forward is the EXISTING kernel and whose autograd
# formula calls them.  A gradient that is not needed is not computed (NULL pointer) and comes back as an empty tensor.
@custom_op("aadff::render_psf_map_stack_bwd", mutates_args=(), device_types="cuda")
def render_psf_map_stack_bwd(img: torch.Tensor, psf_maps: torch.Tensor, dy: torch.Tensor, grid: int, need_img: bool,
                             need_psf: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    B, Cn, H, W = img.shape
    S, ks = psf_maps.shape[0], psf_maps.shape[2] // grid
    x, p, g = img.contiguous().float(), psf_maps.contiguous().float(), dy.contiguous().float()
    d_img = torch.empty_like(x) if need_img else x.new_empty((0,))
    d_psf = torch.empty_like(p) if need_psf else x.new_empty((0,))
    with torch.cuda.device(x.device):
        ws, nbytes = None, C.c_size_t(0)
        if need_psf:
            _abi.call("aadff_render_psf_map_stack_bwd_workspace", B, Cn, S, H, W, grid, ks, C.byref(nbytes))
            ws = torch.empty((max(1, (nbytes.value + 3) // 4),), dtype=torch.float32, device=x.device)
        _abi.call("aadff_render_psf_map_stack_bwd", _abi.ptr(x), _abi.ptr(p), _abi.ptr(g), _abi.ptr(d_img) if need_img else None,
                  _abi.ptr(d_psf) if need_psf else None, _abi.ptr(ws), C.c_size_t(nbytes.value), B, Cn, S, H, W, grid, ks, _st(x))
    return d_img, d_psf


@render_psf_map_stack_bwd.register_fake
def _(img, psf_maps, dy, grid, need_img, need_psf):
    return (torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format) if need_img else img.new_empty((0,), dtype=torch.float32),
            torch.empty_like(psf_maps, dtype=torch.float32, memory_format=torch.contiguous_format) if need_psf else img.new_empty((0,), dtype=torch.float32))


@custom_op("aadff::local_psf_render_bwd", mutates_args=(), device_types="cuda")
def local_psf_render_bwd(img: torch.Tensor, psf: torch.Tensor, dy: torch.Tensor, ks: int, need_img: bool,
                         need_psf: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    B, Cn, H, W = img.shape
    x, p, g = img.contiguous().float(), psf.contiguous().float(), dy.contiguous().float()
    d_img = torch.empty_like(x) if need_img else x.new_empty((0,))
    d_psf = torch.empty_like(p) if need_psf else x.new_empty((0,))
    with torch.cuda.device(x.device):
        _abi.call("aadff_local_psf_render_bwd", _abi.ptr(x), _abi.ptr(p), _abi.ptr(g), _abi.ptr(d_img) if need_img else None,
                  _abi.ptr(d_psf) if need_psf else None, B, Cn, H, W, ks, _st(x))
    return d_img, d_psf


@local_psf_render_bwd.register_fake
def _(img, psf, dy, ks, need_img, need_psf):
    return (torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format) if need_img else img.new_empty((0,), dtype=torch.float32),
            torch.empty_like(psf, dtype=torch.float32, memory_format=torch.contiguous_format) if need_psf else img.new_empty((0,), dtype=torch.float32))


@custom_op("aadff::render_psf_map_stack_diff", mutates_args=(), device_types="cuda")
def render_psf_map_stack_diff(img: torch.Tensor, psf_maps: torch.Tensor, grid: int) -> torch.Tensor:
    """render_psf_map_stack with an autograd formula (image and PSF maps); the forward is the same ABI call."""
    B, Cn, H, W = img.shape
    S, ks = psf_maps.shape[0], psf_maps.shape[2] // grid
    x, p = img.contiguous().float(), psf_maps.contiguous().float()
    out = torch.empty((B, Cn, S, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_render_psf_map_stack", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), B, Cn, S, H, W, grid, ks, _st(x))
    return out


@render_psf_map_stack_diff.register_fake
def _(img, psf_maps, grid):
    B, Cn, H, W = img.shape
    return img.new_empty((B, Cn, psf_maps.shape[0], H, W), dtype=torch.float32)


def _map_setup(ctx, inputs, output):
    img, psf_maps, grid = inputs
    ctx.save_for_backward(img, psf_maps)
    ctx.grid = grid


def _map_backward(ctx, dy):
    img, psf_maps = ctx.saved_tensors
    need_img, need_psf = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    d_img, d_psf = torch.ops.aadff.render_psf_map_stack_bwd(img, psf_maps, dy, ctx.grid, need_img, need_psf)
    return (d_img if need_img else None), (d_psf if need_psf else None), None


render_psf_map_stack_diff.register_autograd(_map_backward, setup_context=_map_setup)


@custom_op("aadff::local_psf_render_diff", mutates_args=(), device_types="cuda")
def local_psf_render_diff(img: torch.Tensor, psf: torch.Tensor, ks: int) -> torch.Tensor:
    """local_psf_render with an autograd formula (image and per-pixel PSFs); the forward is the same ABI call."""
    B, Cn, H, W = img.shape
    x, p = img.contiguous().float(), psf.contiguous().float()
    out = torch.empty_like(x)
    with torch.cuda.device(x.device):
        _abi.call("aadff_local_psf_render", _abi.ptr(x), _abi.ptr(p), _abi.ptr(out), B, Cn, H, W, ks, _st(x))
    return out


@local_psf_render_diff.register_fake
def _(img, psf, ks):
    return torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format)


def _local_setup(ctx, inputs, output):
    img, psf, ks = inputs
    ctx.save_for_backward(img, psf)
    ctx.ks = ks


def _local_backward(ctx, dy):
    img, psf = ctx.saved_tensors
    need_img, need_psf = ctx.needs_input_grad[0], ctx.needs_input_grad[1]
    d_img, d_psf = torch.ops.aadff.local_psf_render_bwd(img, psf, dy, ctx.ks, need_img, need_psf)
    return (d_img if need_img else None), (d_psf if need_psf else None), None


local_psf_render_diff.register_autograd(_local_backward, setup_context=_local_setup)


# ---------------------------------------------------------------- PSF network (deeplens/psfnet.py:375-441)
def _ints(v):
    return (C.c_int * len(v))(*v)


@custom_op("aadff::psfnet_forward", mutates_args=("flags",), device_types="cuda")
def psfnet_forward(inp: torch.Tensor, wpack: torch.Tensor, bias: torch.Tensor, in_features: List[int], out_features: List[int],
                   flags: torch.Tensor, precision: int = 0) -> torch.Tensor:
    x = inp.contiguous().float().reshape(-1, 4)
    out = torch.empty((x.shape[0], out_features[-1]), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_psfnet_forward", _abi.ptr(x), x.shape[0], _abi.ptr(wpack), _abi.ptr(bias), len(in_features), _ints(in_features),
                  _ints(out_features), 0, _abi.ptr(out), None, None, 0, 0, 0, 0, 0, int(precision), _abi.ptr(flags), _st(x))
    return out


@psfnet_forward.register_fake
def _(inp, wpack, bias, in_features, out_features, flags, precision=0):
    return inp.new_empty((inp.numel() // 4, out_features[-1]), dtype=torch.float32)


@custom_op("aadff::psfnet_render_rgbd", mutates_args=("flags",), device_types="cuda")
def psfnet_render_rgbd(img: torch.Tensor, depth: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, foc_z: torch.Tensor, d_min: float,
                       inv_range: float, wpack: torch.Tensor, bias: torch.Tensor, in_features: List[int], out_features: List[int],
                       ks: int, flags: torch.Tensor, precision: int = 0) -> torch.Tensor:
    N, Cn, H, W = img.shape
    S = foc_z.numel() // N
    x, d, fz = img.contiguous().float(), depth.contiguous().float(), foc_z.contiguous().float()
    out = torch.empty((N, Cn, S, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_psfnet_render_rgbd", _abi.ptr(d), _abi.ptr(xs.contiguous().float()), _abi.ptr(ys.contiguous().float()), _abi.ptr(fz),
                  C.c_float(d_min), C.c_float(inv_range), N, S, _abi.ptr(wpack), _abi.ptr(bias), len(in_features), _ints(in_features),
                  _ints(out_features), _abi.ptr(x), _abi.ptr(out), Cn, H, W, ks, int(precision), _abi.ptr(flags), _st(x))
    return out


@psfnet_render_rgbd.register_fake
def _(img, depth, xs, ys, foc_z, d_min, inv_range, wpack, bias, in_features, out_features, ks, flags, precision=0):
    N, Cn, H, W = img.shape
    return img.new_empty((N, Cn, foc_z.numel() // N, H, W), dtype=torch.float32)


# ---------------------------------------------------------------- differentiable RGB-D render (csrc/psfnet_bwd.hip)
def psfnet_bwd_workspace_bytes(N, S, Cn, H, W, ks, need_input, need_img):
    """Bytes of device workspace aadff_psfnet_render_rgbd_bwd needs (host arithmetic, no GPU)."""
    nbytes = C.c_size_t(0)
    lib = _abi.load_library()
    if lib.aadff_psfnet_render_rgbd_bwd_workspace(N, S, Cn, H, W, ks, int(need_input), int(need_img), C.byref(nbytes)) != 0:
        raise RuntimeError("aadff_psfnet_render_rgbd_bwd_workspace failed: " + lib.aadff_last_error().decode(errors="replace"))
    return nbytes.value


@custom_op("aadff::psfnet_render_rgbd_bwd", mutates_args=(), device_types="cuda")
def psfnet_render_rgbd_bwd(img: torch.Tensor, depth: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, foc_z: torch.Tensor, dy: torch.Tensor,
                           d_min: float, inv_range: float, wpack: torch.Tensor, bias: torch.Tensor, wtpack: torch.Tensor, wt_exp: List[int],
                           in_features: List[int], out_features: List[int], ks: int, need_img: bool, need_depth: bool,
                           need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d_img [N,C,H,W], d_depth [N,H,W], d_foc_z [N,S]) of psfnet_render_rgbd; a gradient that is not needed is not computed and comes
    back empty.  Workspace: 4 bytes per (n, slice, pixel) for d_depth / d_foc_z, the PSFs of ONE slice for d_img."""
    N, Cn, H, W = img.shape
    S = foc_z.numel() // N
    x, d, fz, g = img.contiguous().float(), depth.contiguous().float(), foc_z.contiguous().float(), dy.contiguous().float()
    d_img = torch.empty_like(x) if need_img else x.new_empty((0,))
    d_depth = torch.empty((N, H, W), dtype=torch.float32, device=x.device) if need_depth else x.new_empty((0,))
    d_foc = torch.empty((N, S), dtype=torch.float32, device=x.device) if need_foc else x.new_empty((0,))
    with torch.cuda.device(x.device):
        nbytes = psfnet_bwd_workspace_bytes(N, S, Cn, H, W, ks, need_depth or need_foc, need_img)
        ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
        _abi.call("aadff_psfnet_render_rgbd_bwd", _abi.ptr(d), _abi.ptr(xs.contiguous().float()), _abi.ptr(ys.contiguous().float()), _abi.ptr(fz),
                  C.c_float(d_min), C.c_float(inv_range), N, S, _abi.ptr(wpack), _abi.ptr(bias), _abi.ptr(wtpack), _ints(wt_exp), len(in_features),
                  _ints(in_features), _ints(out_features), _abi.ptr(x), _abi.ptr(g), Cn, H, W, ks, _abi.ptr(d_img) if need_img else None,
                  _abi.ptr(d_depth) if need_depth else None, _abi.ptr(d_foc) if need_foc else None, _abi.ptr(ws), C.c_size_t(nbytes), _st(x))
    return d_img, d_depth, d_foc


@psfnet_render_rgbd_bwd.register_fake
def _(img, depth, xs, ys, foc_z, dy, d_min, inv_range, wpack, bias, wtpack, wt_exp, in_features, out_features, ks, need_img, need_depth, need_foc):
    N, Cn, H, W = img.shape
    e = img.new_empty((0,), dtype=torch.float32)
    return (torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format) if need_img else e,
            img.new_empty((N, H, W), dtype=torch.float32) if need_depth else e,
            img.new_empty((N, foc_z.numel() // N), dtype=torch.float32) if need_foc else e)


@custom_op("aadff::psfnet_render_rgbd_diff", mutates_args=(), device_types="cuda")
def psfnet_render_rgbd_diff(img: torch.Tensor, depth: torch.Tensor, xs: torch.Tensor, ys: torch.Tensor, foc_z: torch.Tensor, d_min: float,
                            inv_range: float, wpack: torch.Tensor, bias: torch.Tensor, wtpack: torch.Tensor, wt_exp: List[int],
                            in_features: List[int], out_features: List[int], ks: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """psfnet_render_rgbd (fp32-equivalent mode) with an autograd formula for img [N,C,H,W], depth [N,H,W] and foc_z [N,S]; the forward
    is the same ABI call.  The network weights (wpack, bias, wtpack) get no gradient.  Returns (out [N,C,S,H,W], flags int32[1]): an op
    with an autograd formula cannot write into an argument, so the kernel's saturation flag (bit 4) comes back as a second result."""
    N, Cn, H, W = img.shape
    S = foc_z.numel() // N
    x, d, fz = img.contiguous().float(), depth.contiguous().float(), foc_z.contiguous().float()
    out = torch.empty((N, Cn, S, H, W), dtype=torch.float32, device=x.device)
    flags = torch.zeros(1, dtype=torch.int32, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_psfnet_render_rgbd", _abi.ptr(d), _abi.ptr(xs.contiguous().float()), _abi.ptr(ys.contiguous().float()), _abi.ptr(fz),
                  C.c_float(d_min), C.c_float(inv_range), N, S, _abi.ptr(wpack), _abi.ptr(bias), len(in_features), _ints(in_features),
                  _ints(out_features), _abi.ptr(x), _abi.ptr(out), Cn, H, W, ks, 0, _abi.ptr(flags), _st(x))
    return out, flags


@psfnet_render_rgbd_diff.register_fake
def _(img, depth, xs, ys, foc_z, d_min, inv_range, wpack, bias, wtpack, wt_exp, in_features, out_features, ks):
    N, Cn, H, W = img.shape
    return img.new_empty((N, Cn, foc_z.numel() // N, H, W), dtype=torch.float32), img.new_empty((1,), dtype=torch.int32)


def _rgbd_setup(ctx, inputs, output):
    img, depth, xs, ys, foc_z, d_min, inv_range, wpack, bias, wtpack, wt_exp, in_features, out_features, ks = inputs
    ctx.save_for_backward(img, depth, xs, ys, foc_z, wpack, bias, wtpack)
    ctx.consts = (d_min, inv_range, list(wt_exp), list(in_features), list(out_features), ks)


def _rgbd_backward(ctx, dy, _dflags):
    img, depth, xs, ys, foc_z, wpack, bias, wtpack = ctx.saved_tensors
    d_min, inv_range, wt_exp, ins, outs, ks = ctx.consts
    need_img, need_depth, need_foc = ctx.needs_input_grad[0], ctx.needs_input_grad[1], ctx.needs_input_grad[4]
    d_img, d_depth, d_foc = torch.ops.aadff.psfnet_render_rgbd_bwd(img, depth, xs, ys, foc_z, dy, d_min, inv_range, wpack, bias, wtpack, wt_exp, ins, outs,
                                                                   ks, need_img, need_depth, need_foc)
    return ((d_img.reshape(img.shape) if need_img else None), (d_depth.reshape(depth.shape) if need_depth else None), None, None,
            (d_foc.reshape(foc_z.shape) if need_foc else None), None, None, None, None, None, None, None, None, None)


psfnet_render_rgbd_diff.register_autograd(_rgbd_backward, setup_context=_rgbd_setup)


# ---------------------------------------------------------------- differentiable thin-lens baseline (csrc/thinlens_bwd.hip)
def _thin_args(foc_len, fnum, pixel_size, d_min, d_max):
    return (C.c_float(foc_len / fnum), C.c_float(foc_len), C.c_float(1.0 / pixel_size), C.c_float(d_min), C.c_float(d_max))


def _thin_stack_forward(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max):
    N, Cn, H, W = img.shape
    S = foc_dists.numel() // N
    x, d, fd = img.contiguous().float(), depth.contiguous().float().reshape(N, 1, H, W), foc_dists.contiguous().float().reshape(N, S)
    neg = (d < 0).any().to(torch.int32).reshape(1)              # the reference's whole-tensor sign test, kept on the device
    out = torch.empty((N, Cn, S, H, W), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_thinlens_render_stack", _abi.ptr(x), _abi.ptr(d), _abi.ptr(fd), _abi.ptr(neg), _abi.ptr(out), N, Cn, S, H, W, ks,
                  *_thin_args(foc_len, fnum, pixel_size, d_min, d_max), _st(x))
    return out


@custom_op("aadff::thinlens_render_stack", mutates_args=(), device_types="cuda")
def thinlens_render_stack(img: torch.Tensor, depth: torch.Tensor, foc_dists: torch.Tensor, ks: int, foc_len: float, fnum: float,
                          pixel_size: float, d_min: float, d_max: float) -> torch.Tensor:
    """thinlens_render for foc_dists [N,S] -> [N,C,S,H,W]; slice s is bit-equal to thinlens_render(..., foc_dists[:, s])."""
    return _thin_stack_forward(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max)


@thinlens_render_stack.register_fake
def _(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max):
    N, Cn, H, W = img.shape
    return img.new_empty((N, Cn, foc_dists.numel() // N, H, W), dtype=torch.float32)


def thinlens_bwd_workspace_bytes(N, Cn, S, H, W, ks, need_img, need_foc):
    """Bytes of device workspace aadff_thinlens_render_stack_bwd needs (host arithmetic, no GPU):
    4 * ((2 * N*S*H*W if need_img) + (N*S*H*ceil(W/64) if need_foc))."""
    nbytes = C.c_size_t(0)
    lib = _abi.load_library()
    if lib.aadff_thinlens_render_stack_bwd_workspace(N, Cn, S, H, W, ks, int(need_img), int(need_foc), C.byref(nbytes)) != 0:
        raise RuntimeError("aadff_thinlens_render_stack_bwd_workspace failed: " + lib.aadff_last_error().decode(errors="replace"))
    return nbytes.value


@custom_op("aadff::thinlens_render_stack_bwd", mutates_args=(), device_types="cuda")
def thinlens_render_stack_bwd(img: torch.Tensor, depth: torch.Tensor, foc_dists: torch.Tensor, dy: torch.Tensor, ks: int, foc_len: float,
                              fnum: float, pixel_size: float, d_min: float, d_max: float, need_img: bool, need_depth: bool,
                              need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d_img [N,C,H,W], d_depth [N,1,H,W], d_foc [N,S]) of thinlens_render_stack; a gradient that is not needed is not computed and
    comes back empty.  Workspace: 8 bytes per (n, slice, pixel) for d_img, 4 bytes per 64-pixel run and slice for d_foc."""
    N, Cn, H, W = img.shape
    S = foc_dists.numel() // N
    x, d, fd = img.contiguous().float(), depth.contiguous().float().reshape(N, 1, H, W), foc_dists.contiguous().float().reshape(N, S)
    g = dy.contiguous().float()
    neg = (d < 0).any().to(torch.int32).reshape(1)
    d_img = torch.empty_like(x) if need_img else x.new_empty((0,))
    d_depth = torch.empty_like(d) if need_depth else x.new_empty((0,))
    d_foc = torch.empty_like(fd) if need_foc else x.new_empty((0,))
    with torch.cuda.device(x.device):
        nbytes = thinlens_bwd_workspace_bytes(N, Cn, S, H, W, ks, need_img, need_foc)
        ws = torch.empty((max(1, (nbytes + 3) // 4),), dtype=torch.float32, device=x.device)
        _abi.call("aadff_thinlens_render_stack_bwd", _abi.ptr(x), _abi.ptr(d), _abi.ptr(fd), _abi.ptr(neg), _abi.ptr(g),
                  _abi.ptr(d_img) if need_img else None, _abi.ptr(d_depth) if need_depth else None, _abi.ptr(d_foc) if need_foc else None,
                  _abi.ptr(ws), C.c_size_t(nbytes), N, Cn, S, H, W, ks, *_thin_args(foc_len, fnum, pixel_size, d_min, d_max), _st(x))
    return d_img, d_depth, d_foc


@thinlens_render_stack_bwd.register_fake
def _(img, depth, foc_dists, dy, ks, foc_len, fnum, pixel_size, d_min, d_max, need_img, need_depth, need_foc):
    N, Cn, H, W = img.shape
    return (torch.empty_like(img, dtype=torch.float32, memory_format=torch.contiguous_format) if need_img else img.new_empty((0,), dtype=torch.float32),
            img.new_empty((N, 1, H, W) if need_depth else (0,), dtype=torch.float32),
            img.new_empty((N, foc_dists.numel() // N) if need_foc else (0,), dtype=torch.float32))


@custom_op("aadff::thinlens_render_stack_diff", mutates_args=(), device_types="cuda")
def thinlens_render_stack_diff(img: torch.Tensor, depth: torch.Tensor, foc_dists: torch.Tensor, ks: int, foc_len: float, fnum: float,
                               pixel_size: float, d_min: float, d_max: float) -> torch.Tensor:
    """thinlens_render_stack with an autograd formula for img [N,C,H,W], depth [N,1,H,W] and foc_dists [N,S]; the forward is the same
    ABI call."""
    return _thin_stack_forward(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max)


@thinlens_render_stack_diff.register_fake
def _(img, depth, foc_dists, ks, foc_len, fnum, pixel_size, d_min, d_max):
    N, Cn, H, W = img.shape
    return img.new_empty((N, Cn, foc_dists.numel() // N, H, W), dtype=torch.float32)


def _thin_setup(ctx, inputs, output):
    img, depth, foc_dists = inputs[:3]
    ctx.save_for_backward(img, depth, foc_dists)
    ctx.consts = tuple(inputs[3:])


def _thin_backward(ctx, dy):
    img, depth, foc_dists = ctx.saved_tensors
    need_img, need_depth, need_foc = ctx.needs_input_grad[:3]
    d_img, d_depth, d_foc = torch.ops.aadff.thinlens_render_stack_bwd(img, depth, foc_dists, dy, *ctx.consts, need_img, need_depth, need_foc)
    return ((d_img.reshape(img.shape) if need_img else None), (d_depth.reshape(depth.shape) if need_depth else None),
            (d_foc.reshape(foc_dists.shape) if need_foc else None), None, None, None, None, None, None)


thinlens_render_stack_diff.register_autograd(_thin_backward, setup_context=_thin_setup)


# ---------------------------------------------------------------- depth from a focal stack (csrc/dfocus.hip)
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
    x, u = stack.contiguous().float(), coords.contiguous().float().reshape(N, S)
    depth = torch.empty((N, 1, H, W), dtype=torch.float32, device=x.device)
    index = torch.empty((N, 1, H, W), dtype=torch.int32, device=x.device)
    peak = torch.empty_like(depth)
    aif = torch.empty((N, Cn, H, W), dtype=torch.float32, device=x.device) if want_aif else x.new_empty((0,))
    volume = torch.empty((N, S, H, W), dtype=torch.float32, device=x.device) if want_volume else x.new_empty((0,))
    with torch.cuda.device(x.device):
        _abi.call("aadff_depth_from_stack", _abi.ptr(x), _abi.ptr(u), _abi.ptr(depth), _abi.ptr(index), _abi.ptr(peak),
                  _abi.ptr(aif) if want_aif else None, _abi.ptr(volume) if want_volume else None, N, Cn, S, H, W, window,
                  _abi.DFOCUS_INTERP[interp], C.c_float(eps), _st(x))
    return depth, index, peak, aif, volume


@depth_from_stack.register_fake
def _(stack, coords, window, interp, eps, want_aif, want_volume):
    N, Cn, S, H, W = stack.shape
    return (stack.new_empty((N, 1, H, W), dtype=torch.float32), stack.new_empty((N, 1, H, W), dtype=torch.int32),
            stack.new_empty((N, 1, H, W), dtype=torch.float32),
            stack.new_empty((N, Cn, H, W) if want_aif else (0,), dtype=torch.float32),
            stack.new_empty((N, S, H, W) if want_volume else (0,), dtype=torch.float32))


# ---------------------------------------------------------------- differentiable depth head and loss (csrc/focus_head.hip)
def _head_dims(scores, stack, aif_channels):
    N, K, S, H, W = scores.shape
    return N, K, stack.shape[1], aif_channels, S, H, W


def attention_bwd_workspace_bytes(N, S, H, W):
    """Bytes of device workspace aadff_attention_depth_bwd needs for d_foc: one float per wave and slice (include/aadff.h)."""
    return 4 * N * S * 4 * ((H * ((W + 3) // 4) + 255) // 256)


@custom_op("aadff::attention_depth", mutates_args=(), device_types="cuda")
def attention_depth(scores: torch.Tensor, stack: torch.Tensor, foc_dists: torch.Tensor, normalize_attention: bool,
                    aif_channels: int) -> Tuple[torch.Tensor, torch.Tensor]:
    """(depth [N,1,H,W], aif [N,Ca,H,W]) of scores [N,K,S,H,W] (K 1 or 2), stack [N,Ct,S,H,W] and foc_dists [N,S]: softmax or
    normalised-softplus attention over the slices, expectation of the focus distances and attention-weighted composite of the first
    Ca = aif_channels channels of the stack, in one launch.  Autograd formula for scores, stack and foc_dists."""
    N, K, Ct, Ca, S, H, W = _head_dims(scores, stack, aif_channels)
    z, x, fd = scores.contiguous().float(), stack.contiguous().float(), foc_dists.contiguous().float().reshape(N, S)
    depth = torch.empty((N, 1, H, W), dtype=torch.float32, device=z.device)
    aif = torch.empty((N, Ca, H, W), dtype=torch.float32, device=z.device)
    with torch.cuda.device(z.device):
        _abi.call("aadff_attention_depth", _abi.ptr(z), _abi.ptr(x), _abi.ptr(fd), _abi.ptr(depth), _abi.ptr(aif), N, K, Ct, Ca, S, H, W,
                  int(normalize_attention), _st(z))
    return depth, aif


@attention_depth.register_fake
def _(scores, stack, foc_dists, normalize_attention, aif_channels):
    N, K, S, H, W = scores.shape
    return scores.new_empty((N, 1, H, W), dtype=torch.float32), scores.new_empty((N, aif_channels, H, W), dtype=torch.float32)


@custom_op("aadff::attention_depth_bwd", mutates_args=(), device_types="cuda")
def attention_depth_bwd(scores: torch.Tensor, stack: torch.Tensor, foc_dists: torch.Tensor, g_depth: torch.Tensor, g_aif: torch.Tensor,
                        normalize_attention: bool, aif_channels: int, need_scores: bool, need_stack: bool,
                        need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(d_scores [N,K,S,H,W], d_stack [N,Ct,S,H,W], d_foc [N,S]) of attention_depth; the attention is recomputed from the scores.  A
    gradient that is not needed is not computed and comes back empty; the others do not depend on that."""
    N, K, Ct, Ca, S, H, W = _head_dims(scores, stack, aif_channels)
    z, x, fd = scores.contiguous().float(), stack.contiguous().float(), foc_dists.contiguous().float().reshape(N, S)
    gd, ga = g_depth.contiguous().float(), g_aif.contiguous().float()
    d_z = torch.empty_like(z) if need_scores else z.new_empty((0,))
    d_x = torch.empty_like(x) if need_stack else z.new_empty((0,))
    d_fd = torch.empty_like(fd) if need_foc else z.new_empty((0,))
    nbytes = attention_bwd_workspace_bytes(N, S, H, W) if need_foc else 0
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=z.device) if need_foc else None
    with torch.cuda.device(z.device):
        _abi.call("aadff_attention_depth_bwd", _abi.ptr(z), _abi.ptr(x), _abi.ptr(fd), _abi.ptr(gd), _abi.ptr(ga),
                  _abi.ptr(d_z) if need_scores else None, _abi.ptr(d_x) if need_stack else None, _abi.ptr(d_fd) if need_foc else None,
                  _abi.ptr(ws), C.c_size_t(nbytes), N, K, Ct, Ca, S, H, W, int(normalize_attention), _st(z))
    return d_z, d_x, d_fd


@attention_depth_bwd.register_fake
def _(scores, stack, foc_dists, g_depth, g_aif, normalize_attention, aif_channels, need_scores, need_stack, need_foc):
    N, K, S, H, W = scores.shape
    e = lambda: scores.new_empty((0,), dtype=torch.float32)      # noqa: E731  (one each: outputs must not alias)
    return (torch.empty_like(scores, dtype=torch.float32, memory_format=torch.contiguous_format) if need_scores else e(),
            torch.empty_like(stack, dtype=torch.float32, memory_format=torch.contiguous_format) if need_stack else e(),
            scores.new_empty((N, S), dtype=torch.float32) if need_foc else e())


def _head_setup(ctx, inputs, output):
    scores, stack, foc_dists, normalize_attention, aif_channels = inputs
    ctx.save_for_backward(scores, stack, foc_dists)
    ctx.consts = (normalize_attention, aif_channels)


def _head_backward(ctx, g_depth, g_aif):
    scores, stack, foc_dists = ctx.saved_tensors
    need = ctx.needs_input_grad[:3]
    d_z, d_x, d_fd = torch.ops.aadff.attention_depth_bwd(scores, stack, foc_dists, g_depth, g_aif, *ctx.consts, *need)
    return ((d_z.reshape(scores.shape) if need[0] else None), (d_x.reshape(stack.shape) if need[1] else None),
            (d_fd.reshape(foc_dists.shape) if need[2] else None), None, None)


attention_depth.register_autograd(_head_backward, setup_context=_head_setup)


def _loss_dims(depth, aif, gt_depth, gt_aif):
    hw = lambda t: (t.shape[-2], t.shape[-1]) if t.numel() else (0, 0)      # noqa: E731
    Ca = aif.shape[1] if aif.numel() else (gt_aif.shape[1] if gt_aif.numel() else 0)
    return (depth.shape[0], Ca, *hw(depth), *hw(aif), *hw(gt_depth), *hw(gt_aif))


def _opt(t):
    return _abi.ptr(t) if t.numel() else None


@custom_op("aadff::dff_loss_sums", mutates_args=(), device_types="cuda")
def dff_loss_sums(depth: torch.Tensor, aif: torch.Tensor, gt_depth: torch.Tensor, gt_aif: torch.Tensor, mask_range: torch.Tensor) -> torch.Tensor:
    """The six float64 sums of the depth-from-focus loss over the common top-left window of depth [N,1,Hd,Wd], aif [N,Ca,Ha,Wa],
    gt_depth [N,1,Hg,Wg] and gt_aif [N,Ca,Hi,Wi]: (sum_mask |e|, |mask|, sum_mask e^2, sum |aif - gt_aif|, sum wx r(d_gx), sum wy r(d_gy)).
    An empty tensor stands for one that is absent (aif and gt_aif go together); mask_range: the two floats {lo, hi} of the range mask or
    empty for gt_depth > 0.  Autograd formula for depth and aif (include/aadff.h)."""
    d, a, gd, ga = (t.contiguous().float() for t in (depth, aif, gt_depth, gt_aif))
    rng = mask_range.contiguous().float()
    dims = _loss_dims(d, a, gd, ga)
    sums = torch.empty((6,), dtype=torch.float64, device=d.device)
    nbytes = 48 * ((dims[0] * dims[2] * dims[3] + 1023) // 1024)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=d.device)
    with torch.cuda.device(d.device):
        _abi.call("aadff_dff_loss_sums", _abi.ptr(d), _opt(a), _opt(gd), _opt(ga), _opt(rng), _abi.ptr(sums), _abi.ptr(ws), C.c_size_t(nbytes), *dims, _st(d))
    return sums


@dff_loss_sums.register_fake
def _(depth, aif, gt_depth, gt_aif, mask_range):
    return depth.new_empty((6,), dtype=torch.float64)


@custom_op("aadff::dff_loss_bwd", mutates_args=(), device_types="cuda")
def dff_loss_bwd(depth: torch.Tensor, aif: torch.Tensor, gt_depth: torch.Tensor, gt_aif: torch.Tensor, mask_range: torch.Tensor,
                 g_sums: torch.Tensor, need_depth: bool, need_aif: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_depth, d_aif) of dff_loss_sums for the cotangents g_sums [6] of its sums, in the shapes of depth and aif, zero outside the
    window.  A gradient that is not needed is not computed and comes back empty."""
    d, a, gd, ga = (t.contiguous().float() for t in (depth, aif, gt_depth, gt_aif))
    rng, g = mask_range.contiguous().float(), g_sums.contiguous().double()
    d_d = torch.empty_like(d) if need_depth else d.new_empty((0,))
    d_a = torch.empty_like(a) if need_aif else d.new_empty((0,))
    with torch.cuda.device(d.device):
        _abi.call("aadff_dff_loss_bwd", _abi.ptr(d), _opt(a), _opt(gd), _opt(ga), _opt(rng), _abi.ptr(g), _abi.ptr(d_d) if need_depth else None,
                  _abi.ptr(d_a) if need_aif else None, *_loss_dims(d, a, gd, ga), _st(d))
    return d_d, d_a


@dff_loss_bwd.register_fake
def _(depth, aif, gt_depth, gt_aif, mask_range, g_sums, need_depth, need_aif):
    return (torch.empty_like(depth, dtype=torch.float32, memory_format=torch.contiguous_format) if need_depth else depth.new_empty((0,), dtype=torch.float32),
            torch.empty_like(aif, dtype=torch.float32, memory_format=torch.contiguous_format) if need_aif else depth.new_empty((0,), dtype=torch.float32))


def _loss_setup(ctx, inputs, output):
    ctx.save_for_backward(*inputs)


def _loss_backward(ctx, g_sums):
    depth, aif, gt_depth, gt_aif, mask_range = ctx.saved_tensors
    need_depth, need_aif = ctx.needs_input_grad[0], ctx.needs_input_grad[1] and aif.numel() > 0
    if not (need_depth or need_aif):
        return None, None, None, None, None
    d_d, d_a = torch.ops.aadff.dff_loss_bwd(depth, aif, gt_depth, gt_aif, mask_range, g_sums, need_depth, need_aif)
    return ((d_d.reshape(depth.shape) if need_depth else None), (d_a.reshape(aif.shape) if need_aif else None), None, None, None)


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


@custom_op("aadff::dfv_regress", mutates_args=(), device_types="cuda")
def dfv_regress(cost: torch.Tensor, foc_dists: torch.Tensor, height: int, width: int,
                want_prob: bool) -> Tuple[torch.Tensor, torch.Tensor, torch.Tensor]:
    """(pred [B,1,H,W], std [B,1,H,W], prob [B,S,H,W] or empty) of cost [B,S,h,w] and foc_dists [B,S]: bilinear upsampling to
    height x width (ATen's align_corners = False), softmax over the slices, expectation of the focus distances and its standard
    deviation in one launch.  Autograd formula for cost and foc_dists through pred; std and prob carry no graph."""
    B, S, h, w = cost.shape
    c, fd = cost.contiguous().float(), foc_dists.contiguous().float().reshape(B, S)
    pred = torch.empty((B, 1, height, width), dtype=torch.float32, device=c.device)
    std = torch.empty_like(pred)
    prob = torch.empty((B, S, height, width) if want_prob else (0,), dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        _abi.call("aadff_dfv_head_fwd", _abi.ptr(c), _abi.ptr(fd), _abi.ptr(pred), _abi.ptr(std), _abi.ptr(prob) if want_prob else None,
                  B, S, h, w, height, width, _st(c))
    return pred, std, prob


@dfv_regress.register_fake
def _(cost, foc_dists, height, width, want_prob):
    B, S = cost.shape[0], cost.shape[1]
    return (cost.new_empty((B, 1, height, width), dtype=torch.float32), cost.new_empty((B, 1, height, width), dtype=torch.float32),
            cost.new_empty((B, S, height, width) if want_prob else (0,), dtype=torch.float32))


@custom_op("aadff::dfv_regress_bwd", mutates_args=(), device_types="cuda")
def dfv_regress_bwd(cost: torch.Tensor, foc_dists: torch.Tensor, g_pred: torch.Tensor, need_cost: bool,
                    need_foc: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_cost [B,S,h,w], d_foc [B,S]) of dfv_regress for the cotangent g_pred [B,1,H,W]; the softmax is recomputed from the cost.  A
    gradient that is not needed is not computed and comes back empty; the other does not depend on that."""
    B, S, h, w = cost.shape
    H, W = g_pred.shape[-2], g_pred.shape[-1]
    c, fd, g = cost.contiguous().float(), foc_dists.contiguous().float().reshape(B, S), g_pred.contiguous().float()
    d_c = torch.empty_like(c) if need_cost else c.new_empty((0,))
    d_fd = torch.empty_like(fd) if need_foc else c.new_empty((0,))
    nbytes = dfv_bwd_workspace_bytes(B, S, h, w, H, W, need_cost, need_foc)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=c.device)
    with torch.cuda.device(c.device):
        _abi.call("aadff_dfv_head_bwd", _abi.ptr(c), _abi.ptr(fd), _abi.ptr(g), _abi.ptr(d_c) if need_cost else None,
                  _abi.ptr(d_fd) if need_foc else None, _abi.ptr(ws), C.c_size_t(nbytes), B, S, h, w, H, W, _st(c))
    return d_c, d_fd


@dfv_regress_bwd.register_fake
def _(cost, foc_dists, g_pred, need_cost, need_foc):
    e = lambda: cost.new_empty((0,), dtype=torch.float32)      # noqa: E731  (one each: outputs must not alias)
    return (torch.empty_like(cost, dtype=torch.float32, memory_format=torch.contiguous_format) if need_cost else e(),
            cost.new_empty((cost.shape[0], cost.shape[1]), dtype=torch.float32) if need_foc else e())


def _dfv_setup(ctx, inputs, output):
    cost, foc_dists = inputs[:2]
    ctx.save_for_backward(cost, foc_dists)
    ctx.mark_non_differentiable(output[1], output[2])          # std is computed under no_grad in the reference; prob is its eval output


def _dfv_backward(ctx, g_pred, g_std, g_prob):
    cost, foc_dists = ctx.saved_tensors
    need = ctx.needs_input_grad[:2]
    if not any(need):
        return None, None, None, None, None
    d_c, d_fd = torch.ops.aadff.dfv_regress_bwd(cost, foc_dists, g_pred, *need)
    return ((d_c.reshape(cost.shape) if need[0] else None), (d_fd.reshape(foc_dists.shape) if need[1] else None), None, None, None)


dfv_regress.register_autograd(_dfv_backward, setup_context=_dfv_setup)


# ---------------------------------------------------------------- confidence-guided depth refinement (csrc/depth_refine.hip)
def depth_refine_constants(channels, sigma_space, sigma_range):
    """(ks, kr) = (1 / (2 sigma_space^2), 1 / (2 sigma_range^2 C)), formed in float64 and rounded to the float32 values the kernels get."""
    return (C.c_float(1.0 / (2.0 * float(sigma_space) ** 2)).value, C.c_float(1.0 / (2.0 * float(sigma_range) ** 2 * channels)).value)


def depth_refine_bwd_workspace_bytes(N, H, W):
    """Bytes of device workspace aadff_depth_refine_bwd needs: alpha, u', beta and the pass-through term, [N,H,W] each."""
    return 16 * N * H * W


@custom_op("aadff::depth_refine", mutates_args=(), device_types="cuda")
def depth_refine(u: torch.Tensor, c: torch.Tensor, g: torch.Tensor, radius: int, sigma_space: float,
                 sigma_range: float) -> Tuple[torch.Tensor, torch.Tensor]:
    """(u' [N,1,H,W], c' [N,1,H,W]): one iteration of the confidence-weighted joint bilateral filter of u [N,1,H,W] with confidence
    c [N,1,H,W] and guide g [N,C,H,W], C in 1..4, over the clipped (2 radius + 1)^2 window.  Autograd formula for u and
    c; the guide is a constant."""
    N, Cn, H, W = g.shape
    x, cc, gg = u.contiguous().float(), c.contiguous().float(), g.contiguous().float()
    ks, kr = depth_refine_constants(Cn, sigma_space, sigma_range)
    u_out, c_out = torch.empty_like(x), torch.empty_like(cc)
    with torch.cuda.device(x.device):
        _abi.call("aadff_depth_refine_fwd", _abi.ptr(x), _abi.ptr(cc), _abi.ptr(gg), _abi.ptr(u_out), _abi.ptr(c_out), N, Cn, H, W,
                  radius, ks, kr, _st(x))
    return u_out, c_out


@depth_refine.register_fake
def _(u, c, g, radius, sigma_space, sigma_range):
    return (torch.empty_like(u, dtype=torch.float32, memory_format=torch.contiguous_format),
            torch.empty_like(c, dtype=torch.float32, memory_format=torch.contiguous_format))


@custom_op("aadff::depth_refine_bwd", mutates_args=(), device_types="cuda")
def depth_refine_bwd(u: torch.Tensor, c: torch.Tensor, g: torch.Tensor, g_u: torch.Tensor, g_c: torch.Tensor, radius: int,
                     sigma_space: float, sigma_range: float, need_u: bool, need_c: bool) -> Tuple[torch.Tensor, torch.Tensor]:
    """(d_u, d_c) [N,1,H,W] of depth_refine for the cotangents g_u, g_c of its two outputs; the sums of the forward are recomputed.  A
    gradient that is not needed is not written and comes back empty; the other does not depend on that."""
    N, Cn, H, W = g.shape
    x, cc, gg = u.contiguous().float(), c.contiguous().float(), g.contiguous().float()
    gu, gc = g_u.contiguous().float(), g_c.contiguous().float()
    ks, kr = depth_refine_constants(Cn, sigma_space, sigma_range)
    d_u = torch.empty_like(x) if need_u else x.new_empty((0,))
    d_c = torch.empty_like(cc) if need_c else x.new_empty((0,))
    nbytes = depth_refine_bwd_workspace_bytes(N, H, W)
    ws = torch.empty((nbytes // 4,), dtype=torch.float32, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_depth_refine_bwd", _abi.ptr(x), _abi.ptr(cc), _abi.ptr(gg), _abi.ptr(gu), _abi.ptr(gc),
                  _abi.ptr(d_u) if need_u else None, _abi.ptr(d_c) if need_c else None, _abi.ptr(ws), C.c_size_t(nbytes), N, Cn, H, W,
                  radius, ks, kr, _st(x))
    return d_u, d_c


@depth_refine_bwd.register_fake
def _(u, c, g, g_u, g_c, radius, sigma_space, sigma_range, need_u, need_c):
    e = lambda: u.new_empty((0,), dtype=torch.float32)         # noqa: E731  (one each: outputs must not alias)
    return (torch.empty_like(u, dtype=torch.float32, memory_format=torch.contiguous_format) if need_u else e(),
            torch.empty_like(c, dtype=torch.float32, memory_format=torch.contiguous_format) if need_c else e())


def _refine_setup(ctx, inputs, output):
    u, c, g, ctx.radius, ctx.sigma_space, ctx.sigma_range = inputs
    ctx.save_for_backward(u, c, g)


def _refine_backward(ctx, g_u, g_c):
    u, c, g = ctx.saved_tensors
    need = ctx.needs_input_grad[:2]
    if not any(need):
        return None, None, None, None, None, None
    d_u, d_c = torch.ops.aadff.depth_refine_bwd(u, c, g, g_u, g_c, ctx.radius, ctx.sigma_space, ctx.sigma_range, *need)
    return ((d_u.reshape(u.shape) if need[0] else None), (d_c.reshape(c.shape) if need[1] else None), None, None, None, None)


depth_refine.register_autograd(_refine_backward, setup_context=_refine_setup)


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


@custom_op("aadff::depth_metric_sums", mutates_args=(), device_types="cuda")
def depth_metric_sums(est: torch.Tensor, gt: torch.Tensor, mask: torch.Tensor, conf: torch.Tensor, valid_mode: str) -> torch.Tensor:
    """sums [N,16] float64 of est, gt [N,1,H,W] in one pass: count, the error sums, the three threshold counts, the confidence-weighted
    sums and the counts of "finite" mode, one row per image (column numbering: include/aadff.h).  mask [N,1,H,W] bool
    and conf [N,1,H,W]: an empty tensor stands for one that is absent.  valid_mode "mask" or "finite".  No autograd formula: the output
    carries no graph."""
    if valid_mode not in _abi.VALID_MODES:
        raise ValueError(f"depth_metric_sums: valid_mode {valid_mode!r} is not one of {sorted(_abi.VALID_MODES)}")
    e, g = est.detach().contiguous().float(), gt.detach().contiguous().float()
    N, H, W = e.shape[0], e.shape[-2], e.shape[-1]
    m = mask.contiguous() if mask.numel() else None
    if m is not None and m.dtype != torch.bool:
        m = m != 0
    c = conf.detach().contiguous().float() if conf.numel() else None
    sums = torch.empty((N, _abi.DEPTH_METRIC_COLS), dtype=torch.float64, device=e.device)
    nbytes = depth_metric_workspace_bytes(N, H, W)
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=e.device)
    with torch.cuda.device(e.device):
        _abi.call("aadff_depth_metric_sums", _abi.ptr(e), _abi.ptr(g), _abi.ptr(m), _abi.ptr(c), _abi.ptr(sums), _abi.ptr(ws), C.c_size_t(nbytes),
                  N, H, W, _abi.VALID_MODES[valid_mode], _st(e))
    return sums


@depth_metric_sums.register_fake
def _(est, gt, mask, conf, valid_mode):
    return est.new_empty((est.shape[0], _abi.DEPTH_METRIC_COLS), dtype=torch.float64)


@custom_op("aadff::image_metric_sums", mutates_args=(), device_types="cuda")
def image_metric_sums(pred: torch.Tensor, target: torch.Tensor, ssim: bool) -> torch.Tensor:
    """sums [N,2] float64 of pred, target [N,C,H,W] (C in 1..4) quantised to bytes as the reference's batch_PSNR does: the exact sum of
    squared differences and, with `ssim`, the sum of the SSIM index over all full 7 x 7 windows and channels (else 0).  No autograd
    formula: the output carries no graph."""
    x, y = pred.detach().contiguous().float(), target.detach().contiguous().float()
    N, Cn, H, W = x.shape
    sums = torch.empty((N, 2), dtype=torch.float64, device=x.device)
    nbytes = image_metric_workspace_bytes(N, Cn, H, W, ssim) if (not ssim or (H >= 7 and W >= 7)) else 16
    ws = torch.empty((nbytes // 8,), dtype=torch.float64, device=x.device)
    with torch.cuda.device(x.device):
        _abi.call("aadff_image_metric_sums", _abi.ptr(x), _abi.ptr(y), _abi.ptr(sums), _abi.ptr(ws), C.c_size_t(nbytes), N, Cn, H, W, int(ssim),
                  _st(x))
    return sums


@image_metric_sums.register_fake
def _(pred, target, ssim):
    return pred.new_empty((pred.shape[0], 2), dtype=torch.float64)


# scores, not losses: an input that requires a gradient is accepted and the sums carry no graph
def _metric_setup(ctx, inputs, output):
    ctx.mark_non_differentiable(output)


def _depth_metric_backward(ctx, g):
    return None, None, None, None, None


def _image_metric_backward(ctx, g):
    return None, None, None


depth_metric_sums.register_autograd(_depth_metric_backward, setup_context=_metric_setup)
image_metric_sums.register_autograd(_image_metric_backward, setup_context=_metric_setup)


# ---------------------------------------------------------------- ray trace -> PSFs (deeplens/optics.py:888-1026)
_LC_FIELDS = [f for f, _ in _abi.LensConst._fields_]


def lens_const_to_list(lc):
    return [float(getattr(lc, f)) for f in _LC_FIELDS]


def lens_const_from_list(v):
    lc = _abi.LensConst()
    for f, x in zip(_LC_FIELDS, v):
        setattr(lc, f, int(x) if f == "n_surf" else float(x))
    return lc


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
    g = int(round(N ** 0.5))
    out = torch.empty((S, L, g * ks, g * ks) if map_layout else (S, N, L, ks, ks), dtype=torch.float32, device=points.device)
    pts, um, uc = points.contiguous().float(), u_main.contiguous().float(), u_chief.contiguous().float()
    with torch.cuda.device(pts.device):
        _abi.call("aadff_psf_points", _abi.ptr(pts), S, N, L, _abi.ptr(surf_main), _abi.ptr(surf_chief), lc, _abi.ptr(states),
                  _abi.ptr(um), spp, 2 * L * spp, 2 * spp, _abi.ptr(uc) if spc else None, spc, 2 * L * spc, 2 * spc, ks, int(centre), int(map_layout),
                  _abi.ptr(out), None, _abi.ptr(flags), _st(pts))
    return out


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
    g = int(round(N ** 0.5))
    out = torch.empty((L, g * ks, g * ks) if map_layout else (N, L, ks, ks), dtype=torch.float32, device=points.device)
    base = u_block.data_ptr()
    with torch.cuda.device(points.device):
        _abi.call("aadff_psf_points", _abi.ptr(points), 1, N, L, _abi.ptr(surf_main), _abi.ptr(surf_chief), lc, _abi.ptr(states),
                  C.c_void_p(base), spp, L * per_l, per_l, C.c_void_p(base + 8 * spp) if spp_chief else None, spp_chief, L * per_l, per_l, ks,
                  int(spp_chief > 0), int(map_layout), _abi.ptr(out), None, _abi.ptr(flags), _st(points))
    return out


@psf_points_block.register_fake
def _(points, surf_main, surf_chief, lens_const, states, u_block, n_wave, spp, spp_chief, ks, map_layout, flags):
    N = points.shape[0]
    g = int(round(N ** 0.5))
    return points.new_empty((n_wave, g * ks, g * ks) if map_layout else (N, n_wave, ks, ks), dtype=torch.float32)


@psf_points.register_fake
def _(points, surf_main, surf_chief, lens_const, states, u_main, u_chief, ks, centre, map_layout, flags):
    S, N, L = points.shape[0], points.shape[1], u_main.shape[1]
    g = int(round(N ** 0.5))
    return points.new_empty((S, L, g * ks, g * ks) if map_layout else (S, N, L, ks, ks), dtype=torch.float32)
