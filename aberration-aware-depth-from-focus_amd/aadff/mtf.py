"""Ray-traced MTF and distortion of a lens.

    res = mtf(lens, points, freqs)                                   # res.mtf [P,L,Z,2,F]: field x colour x sensor plane x (T, S) x frequency
    delta, curve, peak = mtf_through_focus(lens, point, 20.0, span=0.4, steps=9)
    freq, tan, sag = psf2mtf(lens, psf)                              # the reference's FFT of a PSF the caller already has
    draw_mtf(lens, [0.0, 0.7, 1.0], "./mtf.png")
    ideal, traced = distortion_grid(lens, depth)

The geometric OTF of an object point is the Fourier transform of its spot: with n valid rays landing at h_k around their mean c,

    OTF(nu, e) = (1/n) sum_k exp(-2 pi i nu e.(h_k - c)),        MTF = |OTF|,

for a frequency nu (cycles/mm) along a unit vector e.  It is computed here from the traced rays themselves, in one fused HIP launch
(csrc/lens_analysis.hip, `aadff_mtf_points`): no histogram, so no bin width and no window cut-off.  Behind the last surface a ray is a straight
line, so the same rays give the OTF on every sensor plane d_sensor + delta at one multiply-add each - the through-focus curve whose
peak `aadff.dfocus.depth_from_stack` looks for.  The centre c is subtracted before the multiplication by nu: the hits sit at up to
+-20 mm and nu reaches hundreds of cycles/mm, float32 phases of the raw positions would be useless.

Axes: "radial" - tangential e_T along the object point's own direction (p_x, p_y) / hypot(p_x, p_y) ((1, 0) on the axis), sagittal
e_S = (-e_T.y, e_T.x); "xy" - e_T = (1, 0), e_S = (0, 1).  The direction is an input, never a computed centroid (noise near the axis).

The rays are those of `Lensgroup.analysis_rms` on the same seed: stratified pupil samples, draws from `lens.sampler` in the same
order.  parity="fast" lenses take the fused launch; strict / edge lenses the composed route (`sample_pupil` -> their trace -> the
same sums in torch float64).  No gradients, no custom op, and no CPU fallback.
"""
import collections
import ctypes as C
import logging

import numpy as np
import torch

from . import _abi
from deeplens.basics import DEFAULT_WAVE, DEPTH, GEO_SPP, WAVE_RGB, Ray

NUM_ANGLE = 8                       # sectors of the stratified pupil samples (sample_pupil's default, deeplens/optics.py:539)
MAX_SPP, MAX_F, MAX_Z = 2048, 128, 16
AXES = {"radial": 0, "xy": 1}

MTFResult = collections.namedtuple("MTFResult", "mtf otf centroid count")


def _floats(fn, name, values, limit):
    v = values.reshape(-1).tolist() if torch.is_tensor(values) else [float(x) for x in np.atleast_1d(np.asarray(values, dtype=np.float64)).reshape(-1)]
    if not 1 <= len(v) <= limit:
        raise ValueError(f"{fn}: {len(v)} {name} values, the kernel takes 1 to {limit} per launch")
    if not all(np.isfinite(x) for x in v):
        raise ValueError(f"{fn}: {name} holds a non-finite value")
    return [float(x) for x in v]


def _check(fn, lens, freqs, defocus, spp, axes):
    if any(getattr(s, "is_square", False) for s in lens.surfaces):
        raise NotImplementedError(f"{fn}: square apertures are outside the focal-stack hot path")
    if axes not in AXES:
        raise ValueError(f"{fn}: axes {axes!r} is not 'radial' or 'xy'")
    if not isinstance(spp, int) or isinstance(spp, bool) or spp <= 0 or spp % NUM_ANGLE != 0:
        raise ValueError(f"{fn}: spp {spp!r} is not a positive multiple of {NUM_ANGLE} (stratified pupil samples: {NUM_ANGLE} sectors)")
    if spp > MAX_SPP:
        raise ValueError(f"{fn}: spp {spp} exceeds {MAX_SPP} (the rays of a field point stay in LDS)")
    freqs = _floats(fn, "frequency", freqs, MAX_F)
    if any(f < 0 for f in freqs):
        raise ValueError(f"{fn}: a frequency is negative (cycles/mm >= 0)")
    return freqs, _floats(fn, "defocus", defocus, MAX_Z)


def _object_points(fn, pobj):
    pobj = torch.as_tensor(pobj, dtype=torch.float32).detach().cpu()
    if pobj.dim() != 2 or pobj.shape[1] != 3 or pobj.shape[0] < 1:
        raise ValueError(f"{fn}: points must be [P,3], got {tuple(pobj.shape)}")
    if not bool((pobj[:, 2] < 0).all()):
        raise ValueError(f"{fn}: every point's depth must be negative (object side)")
    return pobj.contiguous()


def axes_of(pobj, axes):
    """(e_T [P,2], e_S [P,2]) of object points [P,3] in their dtype: the rule's axes"""
    x, y = pobj[:, 0], pobj[:, 1]
    if axes == "xy":
        e_t = torch.stack((torch.ones_like(x), torch.zeros_like(x)), -1)
    else:
        h = torch.hypot(x, y)
        on_axis = (x == 0) & (y == 0)
        h = torch.where(on_axis, torch.ones_like(h), h)
        e_t = torch.stack((torch.where(on_axis, torch.ones_like(x), x / h), torch.where(on_axis, torch.zeros_like(y), y / h)), -1)
    return e_t, torch.stack((-e_t[:, 1], e_t[:, 0]), -1)


def otf_of_hits(x, y, a, b, valid, e_t, e_s, freqs, defocus):
    """The rule on stored rays, in the dtype of x: x, y, a, b, valid [spp,P] (hits at d_sensor, slopes, validity), axes [P,2] ->
    (otf [P,Z,2,F] complex, moments [P,5] = (n, sum x, sum y, sum a, sum b)).  n = 0 gives zeros."""
    w = valid.to(x.dtype)
    n = w.sum(0)
    den = n.clamp(min=1)
    sums = [(v * w).sum(0) for v in (x, y, a, b)]
    mx, my, ma, mb = [s / den for s in sums]
    P = x.shape[1]
    out = torch.zeros((P, len(defocus), 2, len(freqs)), dtype=torch.complex128 if x.dtype == torch.float64 else torch.complex64)
    for z, dl in enumerate(defocus):
        hx = (x + a * dl) - (mx + ma * dl)
        hy = (y + b * dl) - (my + mb * dl)
        for k, e in enumerate((e_t, e_s)):
            t = e[:, 0] * hx + e[:, 1] * hy
            for f, nu in enumerate(freqs):
                ph = (2 * np.pi * nu) * t
                out[:, z, k, f] = torch.complex((torch.cos(ph) * w).sum(0) / den, -(torch.sin(ph) * w).sum(0) / den)
    out[n == 0] = 0
    return out, torch.stack([n, *sums], -1)


def _launch(lens, pobj, u, wvlns, freqs, defocus, spp, axes):
    """one aadff_mtf_points launch -> (otf [L,P,Z,2,F,2], moments [L,P,8]) float32 on the host; u: the L * 2 * spp * P draws"""
    dev = lens._gpu()
    P, L, F, Z = pobj.shape[0], len(wvlns), len(freqs), len(defocus)
    pupilz, pupilr = lens.entrance_pupil()
    st = lens._state_device()
    pts = _abi.f32c(pobj, dev)
    u = _abi.f32c(u, dev)
    assert u.numel() == L * 2 * spp * P
    otf = torch.empty((L, P, Z, 2, F, 2), dtype=torch.float32, device=dev)
    mom = torch.empty((L, P, 8), dtype=torch.float32, device=dev)
    fr, df = (C.c_float * F)(*freqs), (C.c_float * Z)(*defocus)
    with _abi.on_device(dev):
        _abi.call("aadff_mtf_points", _abi.ptr(pts), P, _abi.ptr(u), spp, NUM_ANGLE, L, _abi.ptr(lens._table(wvlns)), len(lens.surfaces),
                  float(pupilz), float(pupilr), _abi.ptr(st), C.cast(fr, C.c_void_p), F, C.cast(df, C.c_void_p), Z, AXES[axes],
                  _abi.ptr(otf), _abi.ptr(mom), _abi.ptr(lens._flags_device()), _abi.stream_ptr(dev))
    otf, mom = otf.cpu(), mom.cpu()
    lens.check_flags()
    return otf, mom


def _composed(lens, pobj, wvlns, freqs, defocus, spp, axes):
    """The composed route: per colour `sample_pupil((1, P), spp)` (the draws of one sample_point_source call) -> rays from the object
    points -> lens.trace -> project_to(d_sensor), then the rule in torch float64 -> (otf [L,P,Z,2,F] complex128, moments [L,P,5])"""
    P = pobj.shape[0]
    dev = lens._ray_device()
    e_t, e_s = axes_of(pobj.double(), axes)
    d_sensor = lens.d_sensor
    otf, mom = [], []
    for w in wvlns:
        o = pobj.to(dev).reshape(1, 1, P, 3).repeat(spp, 1, 1, 1)
        d = lens.sample_pupil(res=(1, P), spp=spp) - o
        d = d / torch.linalg.vector_norm(d, ord=2, dim=-1, keepdim=True)
        ray, _, _ = lens.trace(Ray(o, d, w, device=dev))
        hit = ray.project_to(d_sensor).reshape(spp, P, 2).double().cpu()
        dd = ray.d.reshape(spp, P, 3).double().cpu()
        valid = (ray.ra.reshape(spp, P) > 0).cpu()
        ok = valid & (dd[..., 2] != 0)
        a = torch.where(ok, dd[..., 0] / dd[..., 2], torch.zeros_like(dd[..., 0]))
        b = torch.where(ok, dd[..., 1] / dd[..., 2], torch.zeros_like(dd[..., 1]))
        x = torch.where(valid, hit[..., 0], torch.zeros_like(a))
        y = torch.where(valid, hit[..., 1], torch.zeros_like(a))
        o_w, m_w = otf_of_hits(x, y, a, b, valid, e_t, e_s, freqs, defocus)
        otf.append(o_w), mom.append(m_w)
    return torch.stack(otf), torch.stack(mom)


@torch.no_grad()
def mtf_points(lens, pobj, freqs, wvlns=WAVE_RGB, defocus=(0.0,), spp=GEO_SPP, axes="radial", u=None):
    """`mtf` for object points in mm ([P,3], z = depth < 0), as the kernel takes them.  u: the L * 2 * spp * P uniforms (per colour,
    per sample a theta block of P then an r^2 block of P), or None: drawn from `lens.sampler` as `analysis_rms` draws them."""
    fn = "mtf_points"
    freqs, defocus = _check(fn, lens, freqs, defocus, spp, axes)
    pobj = _object_points(fn, pobj)
    wvlns = [float(w) for w in ([wvlns] if isinstance(wvlns, (int, float)) else wvlns)]
    if not 1 <= len(wvlns) <= 16:
        raise ValueError(f"{fn}: {len(wvlns)} wavelengths, the kernel takes 1 to 16 passes per launch")
    P, L = pobj.shape[0], len(wvlns)
    if lens.parity != "fast":
        if u is not None:
            raise ValueError(f"{fn}: parity={lens.parity!r} lenses draw from lens.sampler (the composed route), u cannot be given")
        otf, mom = _composed(lens, pobj, wvlns, freqs, defocus, spp, axes)
    else:
        if u is None:
            u = lens._uniform_block(L * 2 * spp * P)
        elif not torch.is_tensor(u) or u.numel() != L * 2 * spp * P or u.dtype != torch.float32:
            raise ValueError(f"{fn}: u must hold {L} x 2 x {spp} x {P} float32 uniforms")
        raw, mom = _launch(lens, pobj, u, wvlns, freqs, defocus, spp, axes)
        otf = torch.view_as_complex(raw.contiguous())
    n = mom[..., 0]
    den = n.clamp(min=1).unsqueeze(-1)
    dl = torch.tensor(defocus, dtype=mom.dtype).reshape(1, 1, -1, 1)
    centroid = (mom[..., 1:3] / den).unsqueeze(2) + (mom[..., 3:5] / den).unsqueeze(2) * dl             # [L,P,Z,2]
    return MTFResult(otf.abs().transpose(0, 1), otf.transpose(0, 1), centroid.transpose(0, 1), n.transpose(0, 1))


@torch.no_grad()
def mtf(lens, points, freqs, wvlns=WAVE_RGB, defocus=(0.0,), spp=GEO_SPP, axes="radial"):
    """MTF of `lens` at normalised field points [P,3] (x, y in [-1, 1] of the half sensor, z = object depth in mm < 0, as for
    `lens.psf`; an MTF against object depth at a fixed focus is therefore just more points).

    freqs    F <= 128 frequencies, cycles/mm, >= 0
    wvlns    L <= 16 wavelengths (um)
    defocus  Z <= 16 sensor shifts delta along the axis (mm): the OTF on the plane d_sensor + delta
    spp      rays per point and colour, a multiple of 8 and <= 2048
    axes     "radial" (tangential / sagittal by the object point's direction) or "xy"
    -> MTFResult(mtf [P,L,Z,2,F], otf complex [P,L,Z,2,F], centroid [P,L,Z,2] (mm, the centre c on each plane), count [P,L] (valid rays)),
    index 0 of the axis dimension tangential (x), 1 sagittal (y).  Synchronises; raises the reference's Newton error."""
    _check("mtf", lens, freqs, defocus, spp, axes)                  # before anything touches the device
    points = torch.as_tensor(points, dtype=torch.float32)
    if points.dim() == 1:
        points = points.unsqueeze(0)
    if points.dim() != 2 or points.shape[1] != 3:
        raise ValueError(f"mtf: points must be [P,3] normalised field points, got {tuple(points.shape)}")
    return mtf_points(lens, lens._object_points(points.detach().cpu()), freqs, wvlns=wvlns, defocus=defocus, spp=spp, axes=axes)


def parabola_peak(delta, curve):
    """delta [S] evenly spaced, curve [S]: the abscissa of the maximum by the parabola through the largest sample and its two
    neighbours (the sample itself at either end)"""
    i = int(torch.argmax(curve))
    if i == 0 or i == len(delta) - 1:
        return float(delta[i])
    ym, y0, yp = float(curve[i - 1]), float(curve[i]), float(curve[i + 1])
    den = ym - 2 * y0 + yp
    if den == 0:
        return float(delta[i])
    return float(delta[i]) + 0.5 * float(delta[i + 1] - delta[i]) * (ym - yp) / den


@torch.no_grad()
def mtf_through_focus(lens, point, freq, span, steps, wvln=DEFAULT_WAVE, spp=GEO_SPP, axes="radial"):
    """The MTF at `freq` cycles/mm of one normalised field point on `steps` sensor planes evenly spaced over [-span/2, +span/2] mm
    around d_sensor -> (delta [steps], curve [steps,2] (T, S), peak [2]): peak is the delta of each axis's maximum by the three-point
    parabola, the sensor shift at which this field point is sharpest - over the field, the field-curvature map.  All planes see the
    same rays (one block of draws; more than 16 planes run as several launches on it)."""
    fn = "mtf_through_focus"
    if not isinstance(steps, int) or steps < 3:
        raise ValueError(f"{fn}: steps {steps!r} must be an integer >= 3 (the peak is a three-point fit)")
    if not float(span) > 0:
        raise ValueError(f"{fn}: span {span} must be positive (mm)")
    delta = torch.linspace(-float(span) / 2, float(span) / 2, steps, dtype=torch.float64)
    point = torch.as_tensor(point, dtype=torch.float32).reshape(1, 3)
    pobj = lens._object_points(point)
    if lens.parity != "fast":
        if steps > MAX_Z:
            raise ValueError(f"{fn}: parity={lens.parity!r} lenses take at most {MAX_Z} planes (one block of draws per call)")
        curve = mtf_points(lens, pobj, [freq], [wvln], delta.tolist(), spp, axes).mtf[0, 0, :, :, 0]
    else:
        _check(fn, lens, [freq], [0.0], spp, axes)
        u = lens._uniform_block(2 * spp)
        curve = torch.cat([mtf_points(lens, pobj, [freq], [wvln], delta[i:i + MAX_Z].tolist(), spp, axes, u=u).mtf[0, 0, :, :, 0]
                           for i in range(0, steps, MAX_Z)])
    peak = torch.tensor([parabola_peak(delta, curve[:, k].double()) for k in range(2)], dtype=torch.float64)
    return delta, curve, peak


def psf2mtf(lens, psf, diag=False):
    """Convert a 2-D PSF kernel to MTF curves by FFT: the reference's function (deeplens/optics.py:1028-1065), host numpy, for PSFs
    the caller already has -> (freq, tangential_mtf, sagittal_mtf) on the positive frequencies of fftfreq(psf.shape[0], pixel_size).
    The 'tangential' curve is the column through the centre bin, the 'sagittal' one the row; `diag` is accepted and unused, as there."""
    psf = psf.cpu().numpy()
    center_x = psf.shape[1] // 2
    center_y = psf.shape[0] // 2
    sagittal_psf = psf[center_y, :]
    tangential_psf = psf[:, center_x]
    sagittal_mtf = np.abs(np.fft.fft(sagittal_psf))
    tangential_mtf = np.abs(np.fft.fft(tangential_psf))
    sagittal_mtf /= sagittal_mtf.max()
    tangential_mtf /= tangential_mtf.max()
    freq = np.fft.fftfreq(psf.shape[0], lens.pixel_size)
    positive_freq_idx = freq > 0
    return freq[positive_freq_idx], tangential_mtf[positive_freq_idx], sagittal_mtf[positive_freq_idx]


def draw_mtf_axis(lens):
    """draw_mtf's frequency axis: the positive part of fftfreq(256, pixel_size) (the reference's ks = 256 histogram), 127 values up to
    one step below Nyquist"""
    freq = np.fft.fftfreq(256, lens.pixel_size)
    return freq[freq > 0]


@torch.no_grad()
def draw_mtf(lens, relative_fov=[0.0, 0.7, 1.0], save_name="./mtf.png", wvlns=DEFAULT_WAVE, depth=DEPTH):
    """Draw the MTF curves of the lens at the diagonal field points (fov, fov, depth): the reference's signature, figure and file
    name (deeplens/optics.py:1914-1941).  The curves are the ray-traced MTF of `mtf()` on the reference's frequency axis, not the
    reference's cut: it FFTs one row and one column, one bin wide, of a 256 x 256 `psf_diff` histogram, which is no line spread (a
    line spread integrates across the cut) and whose 256 bins the PSF kernels here do not reach (AADFF_MAX_KS = 51).  The OTF of the
    hits has no bins and no window, and 'tangential' / 'sagittal' are taken along and across the field direction.
    Returns the file name (None without matplotlib, as draw_spot_diagram)."""
    from deeplens import optics
    if save_name[-4:] != ".png":
        save_name += ".png"
    relative_fov = [relative_fov] if isinstance(relative_fov, float) else relative_fov
    wvlns = [wvlns] if isinstance(wvlns, float) else wvlns
    color_list = "rgb"
    freq = draw_mtf_axis(lens)
    points = torch.tensor([[fov, fov, depth] for fov in relative_fov], dtype=torch.float32)
    res = mtf(lens, points, freq.tolist(), wvlns=wvlns)
    if optics.plt is None:
        logging.getLogger().info("draw_mtf: matplotlib is not installed, %s not written", save_name)
        return None
    plt = optics.plt
    plt.figure(figsize=(6, 6))
    for wvln_idx, wvln in enumerate(wvlns):
        for fov_idx, fov in enumerate(relative_fov):
            fov_deg = round(fov * lens.hfov * 57.3, 1)
            plt.plot(freq, res.mtf[fov_idx, wvln_idx, 0, 0].numpy(), color_list[fov_idx % 3], label=f"{fov_deg}(deg)-Tangential")
            plt.plot(freq, res.mtf[fov_idx, wvln_idx, 0, 1].numpy(), color_list[fov_idx % 3], label=f"{fov_deg}(deg)-Sagittal", linestyle="--")
    plt.legend()
    plt.xlabel("Spatial Frequency [cycles/mm]")
    plt.ylabel("MTF")
    plt.savefig(f"{save_name}", bbox_inches="tight", format="png", dpi=300)
    plt.close()
    return save_name


@torch.no_grad()
def distortion_grid(lens, depth=DEPTH, M=16):
    """(ideal [M,M,2], traced [M,M,2]) in mm on the sensor: the object grid of `sample_point_source(M, spp=GEO_SPP, R = sensor_size[0]
    / 2 * scale)` over the pinhole scale, and the centroids sum o2 ra / sum ra of its traced rays (deeplens/optics.py:1944-1959).
    Fast lenses: one aadff_spot_moments launch; strict / edge: the composed trace.  torch's generator is left where that
    `sample_point_source` call leaves it."""
    scale = lens.calc_scale_pinhole(depth)
    R = lens.sensor_size[0] / 2 * scale
    if lens.parity != "fast":
        ray = lens.sample_point_source(M=M, spp=GEO_SPP, depth=depth, R=R, pupil=True)
        ideal = ray.o.detach().cpu()[0, :, :, :2] / scale
        ray, _, _ = lens.trace(ray)
        o2, ra = ray.project_to(lens.d_sensor).clone().cpu(), ray.ra.cpu()
        return ideal, torch.stack((torch.sum(o2[..., 0] * ra, 0) / torch.sum(ra, 0), torch.sum(o2[..., 1] * ra, 0) / torch.sum(ra, 0)), -1)
    o = lens._point_grid(R, depth, M)
    mom = lens._spot_moments(o.reshape(-1, 3), [DEFAULT_WAVE], GEO_SPP, 0, False)[0].reshape(M, M, 4)
    return o[..., :2] / scale, mom[..., 1:3] / mom[..., 0:1]


@torch.no_grad()
def draw_distortion(lens, depth=DEPTH, save_name=None):
    """Scatter of the ideal grid and the traced centroids of `distortion_grid`, the reference's figure and file name
    (deeplens/optics.py:1944-1972).  Returns the file name (None without matplotlib, as draw_spot_diagram)."""
    from deeplens import optics
    ideal, traced = distortion_grid(lens, depth, M=16)
    name = f"./distortion{-depth}mm.png" if save_name is None else f"{save_name}_distortion{-depth}mm.png"
    if optics.plt is None:
        logging.getLogger().info("draw_distortion: matplotlib is not installed, %s not written", name)
        return None
    plt = optics.plt
    fig, ax = plt.subplots()
    ax.set_title("Lens distortion")
    ax.scatter(ideal[..., 0], ideal[..., 1], s=2)
    ax.scatter(traced[..., 0], traced[..., 1], s=2)
    ax.legend(["ref", "distortion"])
    ax.axis("scaled")
    plt.savefig(name, bbox_inches="tight", format="png", dpi=300)
    plt.close()
    return name
