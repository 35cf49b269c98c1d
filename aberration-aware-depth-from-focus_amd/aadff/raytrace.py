"""Ray-traced image rendering through the lens: the picture the PSF routes approximate.

    out = render_raytraced(lens, img, depth=-2000.0, spp=64)                  # [B,3,H,W]
    out, aux = render_raytraced(lens, img, depth, return_aux=True)            # aux["count"] [3,H,W]: valid rays per pixel
    stack = render_raytraced_stack(lens, img, depth, foc_dists)               # [B,3,S,H,W]
    out = render_raytraced_layered(lens, img, layer, layer_depths)            # a layered RGB-D scene, front to back
    out, depths = render_raytraced_rgbd(lens, img, depth_mm, layers=8)        # depth_layers per image, then the above
    stack = render_raytraced_layered_stack(lens, img, layer, layer_depths, foc_dists)

Every pixel of the sensor sends `spp` rays per colour channel through stratified points of the exit pupil, backwards through
all surfaces to the object plane z = depth, and averages the bilinear samples of the scene where they land - one fused HIP
launch (csrc/render_rt.hip, `aadff_render_raytraced`) that shares the trace core of the PSF kernels.  No patch seams, no kernel-size
cut-off; distortion, lateral colour and (with `vignetting=True`) the lens's fall-off are in the picture.  The scene is sampled
so that an ideal lens of magnification -1 / scale renders the identity: nothing is left for the caller to flip.

No gradients (the validity of a ray has none), `parity="fast"` lenses only, and no CPU fallback: without the HIP library or a
GPU it raises like the other renderers.
"""
import ctypes as C

import torch

from . import _abi
from deeplens.basics import DEPTH, WAVE_RGB

NUM_ANGLE = 8                       # sectors of the stratified pupil samples (sample_pupil's default, deeplens/optics.py:539)


def _check_spp(fn, spp):
    if not isinstance(spp, int) or isinstance(spp, bool) or spp <= 0 or spp % NUM_ANGLE != 0:
        raise ValueError(f"{fn}: spp {spp!r} is not a positive multiple of {NUM_ANGLE} (stratified pupil samples: {NUM_ANGLE} sectors)")


def _draw_seed():
    """one 63-bit seed from torch's global generator, so torch.manual_seed governs the render"""
    return int(torch.randint(0, 2 ** 63 - 1, (1,), dtype=torch.int64).item())


def _check_seed(fn, seed):
    if not isinstance(seed, int) or isinstance(seed, bool) or not 0 <= seed < 2 ** 64:
        raise ValueError(f"{fn}: seed {seed!r} is not an integer in [0, 2^64)")
    return seed


def _check_scene(fn, lens, img, u):
    """the checks every render makes of its lens, image and uniforms before anything else; returns (B, H, W)"""
    if getattr(lens, "parity", "fast") != "fast":
        raise NotImplementedError(f"{fn}: parity={lens.parity!r} lenses trace in the reference's float32 operation order on a different "
                                  "kernel, which has no fused render; use a parity='fast' lens")
    if not torch.is_tensor(img) or img.dim() != 4 or img.shape[1] != 3:
        raise ValueError(f"{fn}: img must be [B,3,H,W], got {tuple(img.shape) if torch.is_tensor(img) else type(img).__name__}")
    if img.dtype != torch.float32:
        raise ValueError(f"{fn}: img must be float32, got {img.dtype}")
    B, _, H, W = img.shape
    if B < 1 or H < 1 or W < 1:
        raise ValueError(f"{fn}: img has an empty dimension {tuple(img.shape)}")
    if tuple(lens.sensor_res) != (H, W):
        raise ValueError(f"{fn}: the lens's sensor_res {tuple(lens.sensor_res)} is not the image's (H, W) = {(H, W)}; call "
                         "lens.prepare_sensor((H, W)) first")
    if img.requires_grad or (torch.is_tensor(u) and u.requires_grad):
        raise RuntimeError(f"{fn}: no autograd - a tensor that requires grad was passed (detach it; the ray-traced render has no "
                           "backward, aadff.diffrender has the differentiable routes)")
    return B, H, W


def _check_uniforms(fn, u, seed, spp, H, W):
    if seed is not None:
        raise ValueError(f"{fn}: pass u or seed, not both")
    if not torch.is_tensor(u) or tuple(u.shape) != (3, spp, 2, H, W):
        raise ValueError(f"{fn}: u must be [3,{spp},2,{H},{W}], got {tuple(u.shape) if torch.is_tensor(u) else type(u).__name__}")
    if u.dtype != torch.float32:
        raise ValueError(f"{fn}: u must be float32, got {u.dtype}")


@torch.no_grad()
def sensor_uniforms(seed, spp, H, W, device=None):
    """[3, spp, 2, H, W] float32 in [0, 1): the jitter uniforms `render_raytraced(seed=seed)` draws inside its kernel - element
    idx (flat) is output idx of the SplitMix64 sequence seeded with `seed`, top 24 bits.  u[c, s, 0] jitters the angle and
    u[c, s, 1] the squared radius of sample s of channel c; u[c] is the flat block `lens.sample_pupil((H, W), spp)` consumes."""
    _check_spp("sensor_uniforms", spp)
    _check_seed("sensor_uniforms", seed)
    if H < 1 or W < 1:
        raise ValueError(f"sensor_uniforms: H={H}, W={W} must be positive")
    _abi.require_gpu()
    dev = torch.device("cuda", torch.cuda.current_device()) if device is None else torch.device(device)
    if dev.type != "cuda":
        raise ValueError(f"sensor_uniforms: device {dev} is not a GPU (the values are generated by the render's own device function)")
    out = torch.empty((3, spp, 2, H, W), dtype=torch.float32, device=dev)
    with _abi.on_device(out.device):
        _abi.call("aadff_sensor_uniforms", C.c_ulonglong(seed), spp, H, W, _abi.ptr(out), _abi.stream_ptr(out.device))
    return out


@torch.no_grad()
def render_raytraced(lens, img, depth=DEPTH, spp=64, scale=None, u=None, seed=None, vignetting=False, return_aux=False):
    """img [B,3,H,W] float32 (any device) seen through `lens` (sensor_res == (H, W)) as a plane scene at z = depth (mm < 0)
    -> [B,3,H,W] on img's device.

    scale        object mm per sensor mm; None: lens.calc_scale_ray(depth) (one traced magnification, synchronises)
    spp          rays per pixel and channel, a multiple of 8 (8 sectors x spp/8 rings of the exit pupil)
    u            [3,spp,2,H,W] uniforms in [0, 1) for the pupil jitter (see `sensor_uniforms`), or None: the kernel draws them
                 from `seed`; seed None: one 63-bit seed from torch's generator (torch.manual_seed governs it)
    vignetting   False: each pixel is the mean over its valid rays; True: the sum over valid rays / spp (fall-off stays in)
    return_aux   True: also a dict with "count" [3,H,W], the valid rays per pixel; "valid": additionally "valid"
                 [3,spp,H,W] bool, the validity of every ray (diagnostics: spp bytes per pixel and channel)
    The sensor position is read from the lens's device state inside the kernel: a `lens.refocus()` queued before the call is
    honoured without a host round trip.  A NaN Newton residual raises FloatingPointError at the lens's next flag check."""
    fn = "render_raytraced"
    B, H, W = _check_scene(fn, lens, img, u)
    _check_spp(fn, spp)
    depth = float(depth)
    if not depth < 0:
        raise ValueError(f"{fn}: depth {depth} must be negative (the object plane lies in front of the lens)")
    if return_aux not in (False, True, "valid"):
        raise ValueError(f"{fn}: return_aux {return_aux!r} is not False, True or 'valid'")
    if scale is None:
        scale = lens.calc_scale_ray(depth)
    scale = float(scale)
    if not scale * lens.pixel_size > 0:
        raise ValueError(f"{fn}: scale {scale} x pixel_size {lens.pixel_size} must be positive")
    dev = lens._gpu()
    if u is not None:
        _check_uniforms(fn, u, seed, spp, H, W)
        u = _abi.f32c(u, dev)
        seed = 0
    else:
        seed = _draw_seed() if seed is None else _check_seed(fn, seed)
    pupil_z, pupil_r = lens.exit_pupil()
    src = img.device
    x = _abi.f32c(img, dev)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    count = torch.empty((3, H, W), dtype=torch.float32, device=dev) if return_aux else None
    valid = torch.empty((3, spp, H, W), dtype=torch.uint8, device=dev) if return_aux == "valid" else None
    lens._poll_flags()
    st, flags = lens._state_device(), lens._flags_device()
    with _abi.on_device(dev):
        _abi.call("aadff_render_raytraced", _abi.ptr(x), B, H, W, _abi.ptr(u), C.c_ulonglong(seed), spp, _abi.ptr(lens._table(WAVE_RGB)),
                  len(lens.surfaces), float(pupil_z), float(pupil_r), float(lens.sensor_size[1]), float(lens.sensor_size[0]),
                  float(lens.pixel_size), depth, scale, int(bool(vignetting)), _abi.ptr(st), _abi.ptr(out), _abi.ptr(count), _abi.ptr(valid),
                  _abi.ptr(flags), _abi.stream_ptr(dev))
    lens._psf_calls += 1                      # kernels on record: the flags word is checked at exit if nobody reads it earlier
    if lens.sync_flags:
        lens.check_flags()
    out = out.to(src)
    if not return_aux:
        return out
    aux = {"count": count.to(src)}
    if valid is not None:
        aux["valid"] = valid.bool().to(src)
    return out, aux


@torch.no_grad()
def render_raytraced_stack(lens, img, depth, foc_dists, spp=64, scale=None, u=None, seed=None, vignetting=False):
    """A focal stack of ray-traced renders: per focus distance `lens.refocus(fd)` and one `render_raytraced` -> [B,3,S,H,W] on
    img's device.  foc_dists: S object distances (mm < 0, list or 1-D tensor).  The scene geometry (`scale`; None:
    lens.calc_scale_ray(depth) at the lens's current focus) and the pupil samples (`u`, or one `seed`) are the same for every
    slice, so slices differ by focus alone - focus breathing included.  The refocus and the render of a slice are queued back to
    back (the kernel reads the sensor position on the device); the lens's sensor position and the first-order numbers that follow
    it are put back afterwards."""
    fn = "render_raytraced_stack"
    fds = [float(f) for f in (foc_dists.reshape(-1).tolist() if torch.is_tensor(foc_dists) else list(foc_dists))]
    if not fds:
        raise ValueError(f"{fn}: foc_dists is empty")
    if any(not f < 0 for f in fds):
        raise ValueError(f"{fn}: focus distances must be negative (object side), got {fds}")
    if getattr(lens, "parity", "fast") != "fast":
        raise NotImplementedError(f"{fn}: parity={lens.parity!r} lenses have no fused render; use a parity='fast' lens")
    if scale is None:
        scale = lens.calc_scale_ray(float(depth))
    if u is None and seed is None:
        seed = _draw_seed()
    saved = (lens.d_sensor, lens.hfov, lens.foclen, lens.fnum)
    try:
        slices = []
        for fd in fds:
            lens.refocus(fd)
            slices.append(render_raytraced(lens, img, depth=depth, spp=spp, scale=scale, u=u, seed=seed, vignetting=vignetting))
        return torch.stack(slices, dim=2)
    finally:
        lens.d_sensor, lens.hfov, lens.foclen, lens.fnum = saved


MAX_LAYERS = 32                     # AADFF_RENDER_MAX_LAYERS: the plane table travels in the kernel arguments


def _check_layers(fn, layer, layer_depths, scales, B, H, W):
    """-> (depths, scales or None) as lists of floats; the layer map is checked, not converted"""
    depths = [float(z) for z in (layer_depths.reshape(-1).tolist() if torch.is_tensor(layer_depths) else list(layer_depths))]
    L = len(depths)
    if not 1 <= L <= MAX_LAYERS:
        raise ValueError(f"{fn}: {L} layer depths, the number of layers must be in [1, {MAX_LAYERS}]")
    if any(not z < 0 for z in depths):
        raise ValueError(f"{fn}: layer depths must be negative (planes in front of the lens), got {depths}")
    if any(not b < a for a, b in zip(depths, depths[1:])):
        raise ValueError(f"{fn}: layer depths must be strictly decreasing, nearest first, got {depths}")
    if not torch.is_tensor(layer) or tuple(layer.shape) != (B, H, W):
        raise ValueError(f"{fn}: layer must be [{B},{H},{W}] (one index map per image), got "
                         f"{tuple(layer.shape) if torch.is_tensor(layer) else type(layer).__name__}")
    if layer.dtype not in (torch.uint8, torch.int64):
        raise ValueError(f"{fn}: layer must be uint8 or int64 (as depth_layers returns it), got {layer.dtype}")
    if scales is not None:
        scales = [float(s) for s in (scales.reshape(-1).tolist() if torch.is_tensor(scales) else list(scales))]
        if len(scales) != L:
            raise ValueError(f"{fn}: {len(scales)} scales for {L} layers")
    return depths, scales


@torch.no_grad()
def render_raytraced_layered(lens, img, layer, layer_depths, scales=None, spp=64, u=None, seed=None, vignetting=False, return_aux=False):
    """img [B,3,H,W] float32 with a layer map, seen through `lens` as a scene of L fronto-parallel planes composited front to back
     -> [B,3,H,W] on img's device.  Occlusion is in the picture: a ray that meets a texel of a near plane is stopped
    there in proportion to the bilinear coverage `a` of that plane's texels, and only T = prod (1 - a) of it goes on.

    layer         [B,H,W] uint8, or int64 as `aadff.focal_stack.depth_layers` returns it: the plane each texel lies on; an index >= L
                  (or outside 0..255) lies on no plane - a hole, which lets every ray through
    layer_depths  L values (1 <= L <= 32), mm < 0, strictly decreasing: nearest plane first
    scales        L values, object mm per sensor mm at each plane; None: lens.calc_scale_ray(z_l) per plane (L traced
                  magnifications: synchronises L times)
    spp, u, seed, vignetting   as in `render_raytraced`; the pixel is sum V / sum A over its rays (vignetting: sum V / spp)
    return_aux    True: also a dict with "coverage" [B,3,H,W] = sum A and "alive" [3,H,W], the rays that survived the lens;
                  "valid": additionally "alive_rays" [3,spp,H,W] bool
    With L = 1 and layer == 0 the result is `render_raytraced`'s bit for bit and coverage its count."""
    fn = "render_raytraced_layered"
    B, H, W = _check_scene(fn, lens, img, u)
    _check_spp(fn, spp)
    depths, scales = _check_layers(fn, layer, layer_depths, scales, B, H, W)
    if return_aux not in (False, True, "valid"):
        raise ValueError(f"{fn}: return_aux {return_aux!r} is not False, True or 'valid'")
    if u is not None:
        _check_uniforms(fn, u, seed, spp, H, W)
    elif seed is not None:
        _check_seed(fn, seed)
    if scales is None:
        scales = [float(lens.calc_scale_ray(z)) for z in depths]
    if any(not s * lens.pixel_size > 0 for s in scales):
        raise ValueError(f"{fn}: every scale x pixel_size {lens.pixel_size} must be positive, got scales {scales}")
    dev = lens._gpu()
    if u is not None:
        u = _abi.f32c(u, dev)
        seed = 0
    elif seed is None:
        seed = _draw_seed()
    L = len(depths)
    lay = layer.to(dev)
    if lay.dtype != torch.uint8:
        lay = torch.where((lay < 0) | (lay > 255), torch.full_like(lay, 255), lay).to(torch.uint8)
    lay = lay.contiguous()
    pupil_z, pupil_r = lens.exit_pupil()
    src = img.device
    x = _abi.f32c(img, dev)
    out = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev)
    coverage = torch.empty((B, 3, H, W), dtype=torch.float32, device=dev) if return_aux else None
    alive = torch.empty((3, H, W), dtype=torch.float32, device=dev) if return_aux else None
    rays = torch.empty((3, spp, H, W), dtype=torch.uint8, device=dev) if return_aux == "valid" else None
    zs, sc = (C.c_float * L)(*depths), (C.c_float * L)(*scales)
    lens._poll_flags()
    st, flags = lens._state_device(), lens._flags_device()
    with _abi.on_device(dev):
        _abi.call("aadff_render_raytraced_layered", _abi.ptr(x), _abi.ptr(lay), B, H, W, _abi.ptr(u), C.c_ulonglong(seed), spp,
                  _abi.ptr(lens._table(WAVE_RGB)), len(lens.surfaces), float(pupil_z), float(pupil_r), float(lens.sensor_size[1]),
                  float(lens.sensor_size[0]), float(lens.pixel_size), L, C.cast(zs, C.c_void_p), C.cast(sc, C.c_void_p), int(bool(vignetting)),
                  _abi.ptr(st), _abi.ptr(out), _abi.ptr(coverage), _abi.ptr(alive), _abi.ptr(rays), _abi.ptr(flags), _abi.stream_ptr(dev))
    lens._psf_calls += 1                      # kernels on record: the flags word is checked at exit if nobody reads it earlier
    if lens.sync_flags:
        lens.check_flags()
    out = out.to(src)
    if not return_aux:
        return out
    aux = {"coverage": coverage.to(src), "alive": alive.to(src)}
    if rays is not None:
        aux["alive_rays"] = rays.bool().to(src)
    return out, aux


@torch.no_grad()
def render_raytraced_rgbd(lens, img, depth_mm, layers=8, scales=None, spp=64, u=None, seed=None, vignetting=False, return_aux=False):
    """An RGB-D image through the lens: `depth_layers(depth_mm[b], layers)` per image, then `render_raytraced_layered` with that
    image's planes.  img [B,3,H,W], depth_mm [B,1,H,W] or [B,H,W] (mm < 0; 0 = invalid: farthest layer) -> (out [B,3,H,W],
    layer_depths [B,layers] float32 nearest first, on the host) and, with return_aux, the aux dict (coverage [B,3,H,W]; alive and
    alive_rays of the first image's call: the rays do not depend on the image).  Reads each image's layer depths back (they go into
    the kernel arguments): it synchronises once per image, and with scales=None `layers` times more.  One seed (or `u`) serves every
    image."""
    from .focal_stack import depth_layers
    fn = "render_raytraced_rgbd"
    B, H, W = _check_scene(fn, lens, img, u)
    _check_spp(fn, spp)
    layers = int(layers)
    if not 1 <= layers <= MAX_LAYERS:
        raise ValueError(f"{fn}: layers={layers} must be in [1, {MAX_LAYERS}]")
    if not torch.is_tensor(depth_mm) or tuple(depth_mm.shape) not in ((B, 1, H, W), (B, H, W)):
        raise ValueError(f"{fn}: depth_mm must be [{B},1,{H},{W}] or [{B},{H},{W}], got "
                         f"{tuple(depth_mm.shape) if torch.is_tensor(depth_mm) else type(depth_mm).__name__}")
    if u is not None:
        _check_uniforms(fn, u, seed, spp, H, W)
    elif seed is None:
        seed = _draw_seed()
    dmap = depth_mm.reshape(B, H, W).float()
    outs, zs, auxs = [], [], []
    for b in range(B):
        idx, centres = depth_layers(dmap[b], layers)
        centres = centres.float().cpu()
        r = render_raytraced_layered(lens, img[b:b + 1], idx[None], centres, scales=scales, spp=spp, u=u, seed=seed, vignetting=vignetting,
                                     return_aux=return_aux)
        outs.append(r[0] if return_aux else r)
        auxs.append(r[1] if return_aux else None)
        zs.append(centres)
    out, zs = torch.cat(outs), torch.stack(zs)
    if not return_aux:
        return out, zs
    aux = dict(auxs[0], coverage=torch.cat([a["coverage"] for a in auxs]))
    return out, zs, aux


@torch.no_grad()
def render_raytraced_layered_stack(lens, img, layer, layer_depths, foc_dists, scales=None, spp=64, u=None, seed=None, vignetting=False):
    """A focal stack of layered renders: per focus distance `lens.refocus(fd)` and one `render_raytraced_layered` -> [B,3,S,H,W].
    The planes' scales (None: lens.calc_scale_ray(z_l) at the lens's current focus) and the pupil samples (`u`, or one `seed`) are
    the same for every slice; the lens's sensor position and the first-order numbers that follow it are put back afterwards, as
    `render_raytraced_stack` does."""
    fn = "render_raytraced_layered_stack"
    fds = [float(f) for f in (foc_dists.reshape(-1).tolist() if torch.is_tensor(foc_dists) else list(foc_dists))]
    if not fds:
        raise ValueError(f"{fn}: foc_dists is empty")
    if any(not f < 0 for f in fds):
        raise ValueError(f"{fn}: focus distances must be negative (object side), got {fds}")
    B, H, W = _check_scene(fn, lens, img, u)
    depths, scales = _check_layers(fn, layer, layer_depths, scales, B, H, W)
    if scales is None:
        scales = [float(lens.calc_scale_ray(z)) for z in depths]
    if u is None and seed is None:
        seed = _draw_seed()
    saved = (lens.d_sensor, lens.hfov, lens.foclen, lens.fnum)
    try:
        slices = []
        for fd in fds:
            lens.refocus(fd)
            slices.append(render_raytraced_layered(lens, img, layer, depths, scales=scales, spp=spp, u=u, seed=seed, vignetting=vignetting))
        return torch.stack(slices, dim=2)
    finally:
        lens.d_sensor, lens.hfov, lens.foclen, lens.fnum = saved
