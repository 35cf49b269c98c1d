"""The ray-traced rendering rule restated on the CPU oracle (oracle.lens: OracleLens, Rays, trace, propagate_to),
shared by tests/test_raytrace_host.py and tests/test_gpu_raytrace.py.  It runs in whatever dtype it is asked for (the oracle
follows torch's default dtype), takes the sensor position, the exit pupil, the scale, the uniforms and the images as INPUTS - so
the kernel and the restatement see the same numbers - and returns the image, the valid count per pixel, the validity of every
ray and a mask of the rays whose validity is robust.

    sensor point of pixel (i, j)   x = -Ws/2 + (j+1) ps, y = Hs/2 - (i+1) ps, z = d_sensor
    pupil point of sample s        sector s // (spp/8), ring s % (spp/8): theta = (u[c,s,0] + sector) 2 pi / 8,
                                   r^2 = (u[c,s,1] + ring) pr^2 8 / spp, at z = pz
    scene coordinates              uj = W/2 - 1 - px / (scale ps), vi = H/2 - 1 + py / (scale ps) of the landing point (px, py)
    valid                          survived every surface and -1 <= uj <= W, -1 <= vi <= H
    value                          bilinear in img[b, c] at (vi, uj), indices clamped; pixel = sum value / count (0 if count = 0)
"""
import contextlib
import functools
import os

import numpy as np
import torch

from oracle.lens import WAVE_RGB, OracleLens, Rays

REPO = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NUM_ANGLE = 8
LENSES = ("rf50mm", "50mm_f2.8")
H, W, SPP, B = 24, 32, 16, 2          # the smallest shapes with several rings and sectors, rows != columns, border texels, vignetted corners
DEPTHS = (-2000.0, -500.0)
RADIUS_EPS = 1e-5                     # a ray is robust when its validity survives every clear radius scaled by 1 -+ this
WINDOW_EPS = 1e-3                     # ... and, valid, it lies further than this (texels) from the four window bounds


def lens_file(name):
    return os.path.join(REPO, "lenses", name, "lens.json")


@contextlib.contextmanager
def default_dtype(dt):
    old = torch.get_default_dtype()
    torch.set_default_dtype(dt)
    try:
        yield
    finally:
        torch.set_default_dtype(old)


@functools.lru_cache(maxsize=None)
def fixed_inputs():
    """(u [3,SPP,2,H,W], img [B,3,H,W]) as float32 arrays: what the kernel is given, and - widened - the restatement"""
    rng = np.random.default_rng(3)
    u = rng.random((3, SPP, 2, H, W)).astype(np.float32)
    img = rng.random((3, H, W))
    assert float(u.max()) < 1.0
    return u, np.stack((img, 1 - img)).astype(np.float32)


def sensor_points(res, geom):
    """x [1,W], y [H,1] of the pixels' sensor points; geom = (Ws, Hs, ps)"""
    h, w = res
    Ws, Hs, ps = geom
    x = -Ws / 2 + (torch.arange(w, dtype=torch.get_default_dtype()) + 1) * ps
    y = Hs / 2 - (torch.arange(h, dtype=torch.get_default_dtype()) + 1) * ps
    return x.reshape(1, w), y.reshape(h, 1)


def sensor_rays(u_c, res, geom, d_sensor, pupil, wvln):
    """Rays [spp,H,W] of one channel: sensor points towards the stratified pupil points of u_c [spp,2,H,W]"""
    h, w = res
    spp = u_c.shape[0]
    pz, pr = pupil
    rings = spp // NUM_ANGLE
    s = torch.arange(spp)
    sector = (s // rings).to(u_c.dtype).reshape(spp, 1, 1)
    ring = (s % rings).to(u_c.dtype).reshape(spp, 1, 1)
    theta = (u_c[:, 0] + sector) * (2 * np.pi / NUM_ANGLE)
    r = torch.sqrt((u_c[:, 1] + ring) * (pr ** 2 / spp * NUM_ANGLE))
    o2 = torch.stack((r * torch.cos(theta), r * torch.sin(theta), torch.full_like(r, pz)), -1)
    x, y = sensor_points(res, geom)
    o = torch.stack((x.expand(h, w), y.expand(h, w), torch.full((h, w), float(d_sensor), dtype=u_c.dtype)), -1)
    o = o.unsqueeze(0).expand(spp, h, w, 3)
    return Rays(o, o2 - o, wvln=wvln)


def scene_coords(px, py, res, scale, ps):
    h, w = res
    return w / 2 - 1 - px / (scale * ps), h / 2 - 1 + py / (scale * ps)


def window_valid(alive, uj, vi, res):
    h, w = res
    return alive & (uj >= -1) & (uj <= w) & (vi >= -1) & (vi <= h)


def bilinear_mean(img, uj, vi, valid, vignetting=False):
    """img [B,3,H,W]; uj, vi, valid [3,spp,H,W] (any device, any float dtype) -> (out [B,3,H,W], count [3,H,W])"""
    h, w = img.shape[-2:]
    uj = torch.where(valid, uj, torch.zeros_like(uj))          # a dead ray's coordinates never become an index
    vi = torch.where(valid, vi, torch.zeros_like(vi))
    fu, fv = torch.floor(uj), torch.floor(vi)
    ax, ay = uj - fu, vi - fv
    xa, xb = fu.long().clamp(0, w - 1), (fu.long() + 1).clamp(0, w - 1)
    ya, yb = fv.long().clamp(0, h - 1), (fv.long() + 1).clamp(0, h - 1)
    out = []
    for b in range(img.shape[0]):
        val = []
        for c in range(3):
            p = img[b, c]
            top = (1 - ax[c]) * p[ya[c], xa[c]] + ax[c] * p[ya[c], xb[c]]
            bot = (1 - ax[c]) * p[yb[c], xa[c]] + ax[c] * p[yb[c], xb[c]]
            val.append((1 - ay[c]) * top + ay[c] * bot)
        out.append(torch.stack(val))
    val = torch.stack(out) * valid.unsqueeze(0)                # [B,3,spp,H,W]
    count = valid.sum(1).to(val.dtype)
    den = torch.full_like(count, valid.shape[1]) if vignetting else count
    img_out = torch.where(count > 0, val.sum(2) / den.clamp(min=1), torch.zeros_like(count))
    return img_out, count


def render_rule(trace_fn, wvlns, res, geom, d_sensor, pupil, scale, u, img, vignetting=False):
    """The rule with the trace left open: trace_fn(rays, c) -> (px, py, alive) of channel c's rays at the object plane.
    u [3,spp,2,H,W], img [B,3,H,W] tensors of the working dtype.  Returns dict(img, count, valid, uj, vi)."""
    px, py, alive = [], [], []
    for c, w in enumerate(wvlns):
        a, b, m = trace_fn(sensor_rays(u[c], res, geom, d_sensor, pupil, w), c)
        px.append(a), py.append(b), alive.append(m)
    uj, vi = scene_coords(torch.stack(px), torch.stack(py), res, scale, geom[2])
    valid = window_valid(torch.stack(alive), uj, vi, res)
    out, count = bilinear_mean(img, uj, vi, valid, vignetting)
    return dict(img=out, count=count, valid=valid, uj=uj, vi=vi)


def render_oracle(name, depth, d_sensor, pupil, scale, dtype, r_scale=1.0, res=(H, W), u=None, img=None, vignetting=False, geom=None):
    """The rule on OracleLens(lenses/<name>) in `dtype`, every clear radius scaled by r_scale; u / img default to the fixed
    inputs.  d_sensor, pupil = (pz, pr) and scale are the caller's, and so is geom = (Ws, Hs, ps) when given (None: the oracle lens's own)."""
    fu, fi = fixed_inputs()
    with default_dtype(dtype):
        lens = OracleLens(lens_file(name), sensor_res=res)
        for s in lens.surfaces:
            s.r = s.r * r_scale

        def trace_fn(rays, c):
            out = OracleLens.propagate_to(lens.trace(rays), depth)
            return out.o[..., 0], out.o[..., 1], out.ra > 0

        if geom is None:
            geom = (lens.sensor_size[1], lens.sensor_size[0], lens.pixel_size)
        return render_rule(trace_fn, WAVE_RGB, res, geom, d_sensor, pupil, scale, torch.as_tensor(fu if u is None else u).to(dtype),
                           torch.as_tensor(fi if img is None else img).to(dtype), vignetting)


@functools.lru_cache(maxsize=None)
def reference_case(name, depth, d_sensor, pupil, scale, geom=None):
    """Everything the tests compare against, for the fixed inputs, computed once per (lens, depth, sensor position, pupil, scale):
    ref    the float64 restatement (img, count, valid, uj, vi)
    robust [3,spp,H,W]: the ray's validity is the same in three float64 runs with every clear radius scaled by 1 - 1e-5, 1 and
           1 + 1e-5 (1e-5 relative is ~1e-4 mm at these apertures, the order of the edge mode's 2e-4 mm band), and a valid ray
           lies more than 1e-3 texel from the four window bounds
    pix    [3,H,W]: every ray of the pixel is robust
    f32    the float32 restatement"""
    ref = render_oracle(name, depth, d_sensor, pupil, scale, torch.float64, geom=geom)
    lo = render_oracle(name, depth, d_sensor, pupil, scale, torch.float64, r_scale=1 - RADIUS_EPS, geom=geom)
    hi = render_oracle(name, depth, d_sensor, pupil, scale, torch.float64, r_scale=1 + RADIUS_EPS, geom=geom)
    h, w = ref["img"].shape[-2:]
    inner = torch.minimum(torch.minimum(ref["uj"] + 1, w - ref["uj"]), torch.minimum(ref["vi"] + 1, h - ref["vi"])) > WINDOW_EPS
    robust = (ref["valid"] == lo["valid"]) & (ref["valid"] == hi["valid"]) & (~ref["valid"] | inner)
    f32 = render_oracle(name, depth, d_sensor, pupil, scale, torch.float32, geom=geom)
    return dict(ref=ref, robust=robust, pix=robust.all(1), f32=f32)


def floor_distance(case):
    """max |float32 restatement - float64 restatement| per batch image over the pixels whose rays are all robust"""
    m = case["pix"].unsqueeze(0)
    d = (case["f32"]["img"].double() - case["ref"]["img"]).abs() * m
    return d.amax(dim=(1, 2, 3))


def oracle_inputs(name, depth, res=(H, W)):
    """(d_sensor, (pz, pr), scale) of the float64 oracle lens itself: what the host tests feed the restatement"""
    with default_dtype(torch.float64):
        lens = OracleLens(lens_file(name), sensor_res=res)
        pz, pr = lens.exit_pupil()
        return float(lens.d_sensor), (float(pz), float(pr)), float(lens.calc_scale_pinhole(depth))
