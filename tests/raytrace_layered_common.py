"""The layered ray-traced rendering rule restated on the CPU oracle, shared by tests/test_raytrace_layered_host.py
and tests/test_gpu_raytrace_layered.py.  Built from tests/raytrace_common.py (sensor_rays, scene_coords, window_valid) and the
oracle's trace / propagate_to: every channel is traced once, the traced rays are propagated from their last surface to every plane.
Runs in whatever dtype it is asked for; the sensor position, the pupil, the scales, the uniforms, the images and the layer maps are
INPUTS.

    per ray and image b: T = 1, A = 0, V = 0; for l = 0 .. L-1 (nearest plane first):
        (uj, vi) at z_l with scale_l; the ray meets plane l if it survived the lens and -1 <= uj <= W, -1 <= vi <= H
        a = bilinear form of m_t = (layer[b, t] == l), q = the same form of (m_t ? img[b, c, t] : 0)   (four texels t, clamped)
        V += T q;  A += T a;  T = T (1 - a)
    pixel = sum V / sum A over its rays (0 where sum A = 0); vignetting: sum V / spp
"""
import functools

import numpy as np
import torch

import raytrace_common as rc
from oracle.lens import WAVE_RGB, OracleLens

LAYER_DEPTHS = (-500.0, -1000.0, -2000.0)
HOLE = 255


@functools.lru_cache(maxsize=None)
def fixed_layers():
    """[B,H,W] uint8.  Image 0: columns < 12 on plane 0, an 8 x 8 block on plane 1, the rest on plane 2, one 2 x 2 hole.  Image 1: an
    independent random plane per texel - the worst case for the bilinear masks."""
    a = np.full((rc.H, rc.W), 2, dtype=np.uint8)
    a[:, :12] = 0
    a[8:16, 16:24] = 1
    a[4:6, 26:28] = HOLE
    b = np.random.default_rng(5).integers(0, 3, (rc.H, rc.W)).astype(np.uint8)
    return np.stack((a, b))


def _bilinear(t00, t01, t10, t11, ax, ay):
    top = (1 - ax) * t00 + ax * t01
    bot = (1 - ax) * t10 + ax * t11
    return (1 - ay) * top + ay * bot


def layered_rule(trace_fn, wvlns, res, geom, d_sensor, pupil, depths, scales, u, img, layer, vignetting=False):
    """trace_fn(rays, c) -> the traced Rays of channel c (at their last surface).  u [3,spp,2,H,W], img [B,3,H,W] of the working
    dtype, layer [B,H,W] integer.  Returns dict(img, coverage [B,3,H,W], alive [3,spp,H,W] bool, uj, vi [L,3,spp,H,W])."""
    h, w = res
    traced = [trace_fn(rc.sensor_rays(u[c], res, geom, d_sensor, pupil, wv), c) for c, wv in enumerate(wvlns)]
    alive = torch.stack([t.ra > 0 for t in traced])
    layer = layer.long()
    nb = img.shape[0]
    T = torch.ones((nb,) + tuple(alive.shape), dtype=img.dtype)
    V, A = torch.zeros_like(T), torch.zeros_like(T)
    ujs, vis = [], []
    for l, (z, scale) in enumerate(zip(depths, scales)):
        at = [OracleLens.propagate_to(t, z) for t in traced]
        uj, vi = rc.scene_coords(torch.stack([p.o[..., 0] for p in at]), torch.stack([p.o[..., 1] for p in at]), res, scale, geom[2])
        ujs.append(uj), vis.append(vi)
        meets = rc.window_valid(alive, uj, vi, res)
        uj0 = torch.where(meets, uj, torch.zeros_like(uj))         # coordinates outside the window never become an index
        vi0 = torch.where(meets, vi, torch.zeros_like(vi))
        fu, fv = torch.floor(uj0), torch.floor(vi0)
        ax, ay = uj0 - fu, vi0 - fv
        xa, xb = fu.long().clamp(0, w - 1), (fu.long() + 1).clamp(0, w - 1)
        ya, yb = fv.long().clamp(0, h - 1), (fv.long() + 1).clamp(0, h - 1)
        zero = torch.zeros((), dtype=img.dtype)
        for b in range(nb):
            m = [layer[b][y, x] == l for y, x in ((ya, xa), (ya, xb), (yb, xa), (yb, xb))]            # each [3,spp,H,W]
            a = _bilinear(*(t.to(img.dtype) for t in m), ax, ay)
            q = []
            for c in range(3):
                p = img[b, c]
                tex = [torch.where(mt[c], p[y[c], x[c]], zero) for mt, (y, x) in zip(m, ((ya, xa), (ya, xb), (yb, xa), (yb, xb)))]
                q.append(_bilinear(*tex, ax[c], ay[c]))
            a = torch.where(meets, a, torch.zeros_like(a))
            q = torch.where(meets, torch.stack(q), torch.zeros_like(a))
            V[b] = V[b] + T[b] * q
            A[b] = A[b] + T[b] * a
            T[b] = T[b] * (1 - a)
    sum_v, cov = V.sum(2), A.sum(2)
    den = torch.full_like(cov, alive.shape[1]) if vignetting else torch.where(cov > 0, cov, torch.ones_like(cov))
    out = torch.where(cov > 0, sum_v / den, torch.zeros_like(cov))
    return dict(img=out, coverage=cov, alive=alive, uj=torch.stack(ujs), vi=torch.stack(vis))


def layered_oracle(name, depths, scales, d_sensor, pupil, dtype, r_scale=1.0, res=(rc.H, rc.W), u=None, img=None, layer=None, vignetting=False,
                   geom=None):
    """The rule on OracleLens(lenses/<name>) in `dtype`, every clear radius scaled by r_scale; u / img / layer default to the fixed
    inputs; geom = (Ws, Hs, ps), None: the oracle lens's own."""
    fu, fi = rc.fixed_inputs()
    with rc.default_dtype(dtype):
        lens = OracleLens(rc.lens_file(name), sensor_res=res)
        for s in lens.surfaces:
            s.r = s.r * r_scale
        if geom is None:
            geom = (lens.sensor_size[1], lens.sensor_size[0], lens.pixel_size)
        return layered_rule(lambda rays, c: lens.trace(rays), WAVE_RGB, res, geom, d_sensor, pupil, depths, scales,
                            torch.as_tensor(fu if u is None else u).to(dtype), torch.as_tensor(fi if img is None else img).to(dtype),
                            torch.as_tensor(fixed_layers() if layer is None else layer), vignetting)


def survival(name, d_sensor, pupil, r_scale, res=(rc.H, rc.W), geom=None):
    """[3,spp,H,W] bool: the rays of the fixed uniforms that survive the float64 oracle lens with its clear radii scaled"""
    fu, _ = rc.fixed_inputs()
    with rc.default_dtype(torch.float64):
        lens = OracleLens(rc.lens_file(name), sensor_res=res)
        for s in lens.surfaces:
            s.r = s.r * r_scale
        if geom is None:
            geom = (lens.sensor_size[1], lens.sensor_size[0], lens.pixel_size)
        u = torch.as_tensor(fu).double()
        return torch.stack([lens.trace(rc.sensor_rays(u[c], res, geom, d_sensor, pupil, wv)).ra > 0 for c, wv in enumerate(WAVE_RGB)])


@functools.lru_cache(maxsize=None)
def reference_case(name, d_sensor, pupil, scales, geom=None):
    """For the fixed inputs and the three planes, computed once per (lens, sensor position, pupil, scales):
    ref    the float64 restatement
    robust [3,spp,H,W]: the ray's survival is the same in three float64 runs with every clear radius scaled by 1 - 1e-5, 1 and
           1 + 1e-5 and, alive, its coordinates at EVERY plane lie more than 1e-3 texel from the four window bounds
    pix    [3,H,W]: every ray of the pixel is robust
    f32    the float32 restatement"""
    ref = layered_oracle(name, LAYER_DEPTHS, scales, d_sensor, pupil, torch.float64, geom=geom)
    lo = survival(name, d_sensor, pupil, 1 - rc.RADIUS_EPS, geom=geom)
    hi = survival(name, d_sensor, pupil, 1 + rc.RADIUS_EPS, geom=geom)
    h, w = ref["img"].shape[-2:]
    uj, vi = ref["uj"], ref["vi"]
    dist = torch.minimum(torch.minimum((uj + 1).abs(), (w - uj).abs()), torch.minimum((vi + 1).abs(), (h - vi).abs()))     # [L,3,spp,H,W]
    clear = (dist > rc.WINDOW_EPS).all(0)
    robust = (ref["alive"] == lo) & (ref["alive"] == hi) & (~ref["alive"] | clear)
    f32 = layered_oracle(name, LAYER_DEPTHS, scales, d_sensor, pupil, torch.float32, geom=geom)
    return dict(ref=ref, robust=robust, pix=robust.all(1), f32=f32)


def floor_distance(case, key):
    """max |float32 restatement - float64 restatement| of `key` per batch image over the pixels whose rays are all robust"""
    d = (case["f32"][key].double() - case["ref"][key]).abs() * case["pix"].unsqueeze(0)
    return d.amax(dim=(1, 2, 3))


def oracle_inputs(name):
    """(d_sensor, (pz, pr), scales) of the float64 oracle lens itself for the three planes"""
    d_sensor, pupil, _ = rc.oracle_inputs(name, LAYER_DEPTHS[0])
    return d_sensor, pupil, tuple(rc.oracle_inputs(name, z)[2] for z in LAYER_DEPTHS)
