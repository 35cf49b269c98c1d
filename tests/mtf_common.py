"""The ray-traced MTF rule restated on the CPU oracle (oracle.lens: OracleLens, Rays, trace, propagate_to), shared by
tests/test_mtf_host.py and tests/test_gpu_mtf.py, in the pattern of tests/raytrace_common.py.  It runs in whatever dtype it is asked
for, and takes the sensor position, the entrance pupil, the object points, the uniforms, the frequencies and the sensor shifts as
INPUTS - so the kernel and the restatement see the same numbers.

    pupil point of sample s     sector s // (spp/8), ring s % (spp/8): theta = (u[q,s,0,p] + sector) 2 pi / 8,
                                r^2 = (u[q,s,1,p] + ring) pr^2 8 / spp, at z = pz
    ray                         from object point p towards it, through every surface (table of wavelength q), to z = d_sensor:
                                hit (x, y), slopes a = dx/dz, b = dy/dz; valid when it survived every surface
    on the plane d_sensor + dl  h = (x + a dl, y + b dl), centre c = (mean x + mean a dl, mean y + mean b dl), plain means over valid rays
    axes                        radial: e_T = (p_x, p_y) / hypot(p_x, p_y) ((1, 0) when both are 0), e_S = (-e_T.y, e_T.x); xy: (1, 0), (0, 1)
    OTF(nu, e)                  (1/n) sum over valid rays of exp(-2 pi i nu e.(h - c)); zeros when n = 0
"""
import functools

import numpy as np
import torch

from oracle.lens import WAVE_RGB, OracleLens, Rays
from raytrace_common import default_dtype, lens_file

NUM_ANGLE = 8
LENSES = ("rf50mm", "50mm_f2.8")
RES = (24, 32)
DEPTH = -2000.0
DEFOCUS = (-0.1, 0.0, 0.1)
FREQS = (0.0, 5.0, 20.0, 80.0)        # cycles/mm; the tests append the sensor's Nyquist frequency
RADIUS_EPS = 1e-5                     # a ray is robust when its validity survives every clear radius scaled by 1 -+ this
SEED = 5


def uniforms(n_pass, spp, P):
    """[n_pass, spp, 2, P] float32 in [0, 1): the kernel's layout (per pass and sample a theta block of P, then an r^2 block)"""
    u = np.random.default_rng(SEED).random((n_pass, spp, 2, P)).astype(np.float32)
    assert float(u.max()) < 1.0
    return u


def axes_of(points, axes):
    x, y = points[:, 0], points[:, 1]
    if axes == "xy":
        e_t = torch.stack((torch.ones_like(x), torch.zeros_like(x)), -1)
    else:
        zero = (x == 0) & (y == 0)
        h = torch.where(zero, torch.ones_like(x), torch.hypot(x, y))
        e_t = torch.stack((torch.where(zero, torch.ones_like(x), x / h), torch.where(zero, torch.zeros_like(y), y / h)), -1)
    return e_t, torch.stack((-e_t[:, 1], e_t[:, 0]), -1)


def otf_rule(x, y, a, b, valid, e_t, e_s, freqs, defocus):
    """The rule on given rays, in the dtype of x.  x, y, a, b [spp,P], valid [spp,P] bool, e_t, e_s [P,2] ->
    dict(otf [P,Z,2,F] complex, n [P], mean [P,4] = means of x, y, a, b over the valid rays)"""
    dt = x.dtype
    w = valid.to(dt)
    n = w.sum(0)
    den = torch.where(n > 0, n, torch.ones_like(n))
    z0 = torch.zeros((), dtype=dt)
    x, y, a, b = (torch.where(valid, v, z0) for v in (x, y, a, b))
    mean = torch.stack([v.sum(0) / den for v in (x, y, a, b)], -1)
    nu = torch.as_tensor(freqs, dtype=dt).reshape(-1, 1, 1)
    out = []
    for dl in defocus:
        hx = (x + a * dl) - (mean[:, 0] + mean[:, 2] * dl)
        hy = (y + b * dl) - (mean[:, 1] + mean[:, 3] * dl)
        per_axis = []
        for e in (e_t, e_s):
            ph = (2 * np.pi) * (nu * (e[:, 0] * hx + e[:, 1] * hy))                       # [F,spp,P]
            re = (torch.cos(ph) * w).sum(1) / den
            im = -(torch.sin(ph) * w).sum(1) / den
            per_axis.append(torch.complex(re, im).transpose(0, 1))                        # [P,F]
        out.append(torch.stack(per_axis, 1))
    otf = torch.stack(out, 1)
    otf[n == 0] = 0
    return dict(otf=otf, n=n, mean=mean)


def trace_rule(name, d_sensor, pupil, points, u, wvlns, dtype, r_scale=1.0):
    """(x, y, a, b, valid), each [n_pass, spp, P], on OracleLens(lenses/<name>) in `dtype` with every clear radius scaled by r_scale"""
    with default_dtype(dtype):
        lens = OracleLens(lens_file(name), sensor_res=RES)
        for s in lens.surfaces:
            s.r = s.r * r_scale
        pz, pr = pupil
        pts = torch.as_tensor(points).to(dtype)
        u = torch.as_tensor(u).to(dtype)
        n_pass, spp, _, P = u.shape
        rings = spp // NUM_ANGLE
        s = torch.arange(spp)
        sector = (s // rings).to(dtype).reshape(spp, 1)
        ring = (s % rings).to(dtype).reshape(spp, 1)
        out = []
        for q, w in enumerate(wvlns):
            theta = (u[q, :, 0] + sector) * (2 * np.pi / NUM_ANGLE)
            r = torch.sqrt((u[q, :, 1] + ring) * (pr ** 2 / spp * NUM_ANGLE))
            o2 = torch.stack((r * torch.cos(theta), r * torch.sin(theta), torch.full_like(r, pz)), -1)
            o = pts.unsqueeze(0).expand(spp, P, 3)
            ray = OracleLens.propagate_to(lens.trace(Rays(o, o2 - o, wvln=w)), d_sensor)
            out.append((ray.o[..., 0], ray.o[..., 1], ray.d[..., 0] / ray.d[..., 2], ray.d[..., 1] / ray.d[..., 2], ray.ra > 0))
        return tuple(torch.stack([c[i] for c in out]) for i in range(5))


def mtf_oracle(name, d_sensor, pupil, points, u, freqs, defocus, wvlns, axes, dtype, r_scale=1.0):
    """The whole rule in `dtype`: dict(otf [L,P,Z,2,F] complex, n [L,P], mean [L,P,4], valid [L,spp,P])"""
    x, y, a, b, valid = trace_rule(name, d_sensor, pupil, points, u, wvlns, dtype, r_scale)
    e_t, e_s = axes_of(torch.as_tensor(points).to(dtype), axes)
    per = [otf_rule(x[q], y[q], a[q], b[q], valid[q], e_t, e_s, freqs, defocus) for q in range(len(wvlns))]
    return dict(otf=torch.stack([p["otf"] for p in per]), n=torch.stack([p["n"] for p in per]), mean=torch.stack([p["mean"] for p in per]),
                valid=valid)


@functools.lru_cache(maxsize=None)
def reference_case(name, d_sensor, pupil, points_key, spp, freqs, defocus, axes="radial"):
    """Everything the tests compare against, computed once per case.  points_key: the [P,3] float32 object points as nested tuples.
    ref     the float64 restatement
    f32     the float32 restatement
    robust  [L,spp,P]: the ray's validity is the same in three float64 runs with every clear radius scaled by 1 - 1e-5, 1, 1 + 1e-5
    usable  [L,P]: every ray of the field is robust and the float32 restatement's validity equals float64's on all of them"""
    points = np.asarray(points_key, dtype=np.float32)
    u = uniforms(len(WAVE_RGB), spp, points.shape[0])
    args = (name, d_sensor, pupil, points, u)
    ref = mtf_oracle(*args, freqs, defocus, WAVE_RGB, axes, torch.float64)
    robust = ref["valid"].clone()
    robust[:] = True
    for rs in (1 - RADIUS_EPS, 1 + RADIUS_EPS):
        robust &= trace_rule(*args, WAVE_RGB, torch.float64, r_scale=rs)[4] == ref["valid"]
    f32 = mtf_oracle(*args, freqs, defocus, WAVE_RGB, axes, torch.float32)
    usable = robust.all(1) & (f32["valid"] == ref["valid"]).all(1)
    return dict(ref=ref, f32=f32, robust=robust, usable=usable, u=u, points=points)


def otf_floor(case):
    """[F]: max over the usable fields, sensor planes and axes of the float32 restatement's distance from float64, the larger of
    the real part's and the imaginary part's (|d MTF| <= |d OTF|, so the MTF is held to the same number)"""
    d = case["f32"]["otf"].to(torch.complex128) - case["ref"]["otf"]
    d = torch.maximum(d.real.abs(), d.imag.abs()) * case["usable"][:, :, None, None, None]
    return d.amax(dim=(0, 1, 2, 3))


def mean_floor(case):
    """[4]: the same for the means of x, y (mm) and a, b"""
    d = (case["f32"]["mean"].double() - case["ref"]["mean"]).abs() * case["usable"][:, :, None]
    return d.amax(dim=(0, 1))


def oracle_inputs(name):
    """(d_sensor, (pz, pr), points [9,3] float32, nyquist) of the float64 oracle lens itself, refocused to DEPTH with seed-5 draws: what
    a host run feeds the restatement"""
    with default_dtype(torch.float64):
        lens = OracleLens(lens_file(name), sensor_res=RES)
        torch.manual_seed(SEED)
        lens.refocus(DEPTH)
        pz, pr = lens.entrance_pupil()
        scale = lens.calc_scale_pinhole(DEPTH)
        R = lens.sensor_size[0] / 2 * scale
        gx, gy = torch.meshgrid(torch.linspace(-1, 1, 3), torch.linspace(1, -1, 3), indexing="xy")
        pts = torch.stack((gx * R * RES[1] / RES[0], gy * R, torch.full_like(gx, DEPTH)), -1).reshape(-1, 3)
        return float(lens.d_sensor), (float(pz), float(pr)), pts.float().numpy(), 0.5 / lens.pixel_size


def points_key(points):
    return tuple(tuple(float(v) for v in row) for row in np.asarray(points, dtype=np.float32))
