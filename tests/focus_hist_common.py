"""The stages that open and close the ray-traced PSF pipeline - `refocus_kernel` (aadff_refocus, aadff_refocus_staged,
aadff_post_computation), `splat_hit` (aadff_psf_splat) and `normalise_and_write` (aadff_psf_normalise), csrc/trace.hip - restated on
the CPU in float64, with the inputs and the bounds of tests/test_focus_hist_host.py (CPU), tests/test_gpu_focus_stage.py and
tests/test_gpu_histogram.py (GPU).  No bound in this file comes from a kernel's output.

A. FOCUS STAGE.  The reference is oracle/lens.py under torch.float64 on explicit draws: `refocus_rays` / `focus_distances` restate
deeplens/optics.py:1155-1180 as OracleLens.refocus does (oracle/lens.py:296-312), taking (u_theta, u_r); calc_fov is the oracle's own.
The packed fp32 trace is not asked to agree with float64 ray by ray: the tests compare a COUNT (n_focus_rays, exactly) and a MEAN
(d_sensor, within a tolerance), on draws for which the count is decidable:

  * `react_clear` walks the oracle's own Surf.react and reads, beside it, how far every ray clears each validity decision of the
    reference: the aperture radius (and the conic's domain radius) on each surface [mm], the sign of the intersection parameter and of
    the focus distance [mm], Newton's |residual| < 1e-5 and the two refraction tests (cos^2 i > 0.1, total internal reflection)
    [relative to the threshold].  A draw that clears one of them by less than CLEAR_MM = 1e-3 mm (the recorded fp32-vs-float64 hit
    floor is 4.1e-5 mm) or CLEAR_REL = 1e-3 is replaced by a fresh one.  A spherical hit inside the aperture whose Newton iteration did
    not converge is replaced too: the reference discards Newton's mask there (surfaces.py:456-487) and keeps an arbitrary point.
    The condition is on the INPUTS: no ray is excluded from any comparison.
  * 15-50 % of the rays of every draw set (three states) are invalid in float64; natural draws give 25-34 %, a set outside the range
    (the small ones) has draws exchanged for clear ones of the other kind.  spp = 1 cannot take part in that: the one ray of each
    state has to be valid for flags == 0.  A launch with S = 1 runs the first state of its set.
  * valid rays with the largest |focus_d - mean| sit at `tail_positions`: the last rays of the launch (of each quarter for the staged
    entry) and the last lane that carries a second ray, so that a mishandled tail lane moves the value as well as the count.
  * per state the theta row is at s * stride and the r row spp floats behind it, stride = 2 spp + GAP; the gap holds valid draws
    (0.25 and 0.04 alternately), not NaN, which the kernel's `fd == fd` test would silently drop.

The tolerance of d_sensor and of hfov / tan_hfov / foclen / fnum is 4 x the largest distance of the float32 oracle (same code, default
dtype float32) from the float64 oracle over every state of every draw set, and never above the project's 1e-5 (`tolerances`).

B. HISTOGRAM.  `splat_reference` is deeplens/monte_carlo.py:9-121 (as oracle/splat.py states it) in float64 numpy on the fp32 inputs
promoted exactly.  Bound of a raw bin, from the arithmetic of splat_hit with U = 2^-24 = EPS32 / 2 (round to nearest) and K = ks - 1:
    X = -ox - cx                     one rounding, <= U |X| <= U K/2 pixels
    (a weight != 1 scales X first    U K/2 pixels)
    fma(X, scale, K/2)               scale = fl(K / (hi - lo)): U |X scale| <= U K/2 pixels; the fma rounds once: U K; K/2 is a float
                                     (and a hit at X = 0 is at K/2 exactly, as in the reference, whose quotient is then 0.5)
  so a bin coordinate carries at most (0.5 + 0.5 + 0.5 + 1) K U = 2.5 K U <= COORD_ULPS K U = 1.5 K EPS32 pixels.  A tap
  weight (1-wb)(1-wr) ra moves by at most ra per unit of either coordinate, and its own four roundings add 4 U ra; n taps added to a
  bin in any order differ from their exact sum by at most n U times the bin (all terms >= 0).  With A = the summed ra and n = the number
  of the rays within one pixel (inclusive) of the bin in both coordinates:
    |raw - ref| <= U (2 COORD_ULPS K + 4) A + n U ref.
  This needs every ray clear of the discontinuities (`clear_hits`): 1e-4 ps from the window limit, and a non-integer bin coordinate
  1e-4 from an integer (the coordinate error above is 9e-6 at ks = 51).  The normalised PSF divides by the total, summed by 256
  threads: ceil(ks^2 / 256) - 1 strided adds, six wave steps, three adds over the waves; the division is IEEE:
    |psf - ref| <= bound / T + ref (sum(bound) / T + (depth + 1) U),   T = sum(ref).
C. NORMALISE.  relative (depth + 2) EPS32 per element against raw / sum(raw) in float64, depth = the adds on the longest path of
normalise_and_write's tree: ceil(ks^2 / 512) - 1 strided, six wave steps, seven over the eight waves.
"""
import functools
import json
import math

import numpy as np
import torch

from oracle.lens import DEFAULT_WAVE, EPSILON, MAXT, NEWTON_MAXITER, STEP_BOUND, TOL_LOOSE, TOL_TIGHT, OracleLens, Rays
from raytrace_common import default_dtype, lens_file

LENSES = ("rf50mm", "50mm_f2.8")
EPS32 = float(np.finfo(np.float32).eps)
U = EPS32 / 2

# ------------------------------------------------------------------------------------------------------------------ A. focus stage
DEPTHS = (-2000.0, -700.0, -300.0)
PLAIN_SPP = (1, 2, 63, 1023, 1025, 2047, 2049, 3000)
STAGED_SPP = (1, 3, 5, 511, 513, 1023, 1025, 2049)
STAGED_S = (1, 3)
NT = {"plain": 1024, "staged": 256}                  # kRefocusThreads; NT of aadff_refocus_staged
SPLIT = {"plain": 1, "staged": 4}                    # kRefocusSplit
GAP = 24
GAP_FILL = (0.25, 0.04)
CLEAR_MM, CLEAR_REL = 1e-3, 1e-3
INVALID_MIN, INVALID_MAX = 0.15, 0.50
PROJECT_TOL = 1e-5
FIELDS = ("hfov", "tan_hfov", "foclen", "fnum")
UPLOAD_N = (0, 1, 3, 4, 5, 1023, 4 * 256 * 7 + 2)
SEED = 11
INF = float("inf")


def stride_of(spp):
    return 2 * spp + GAP


def parts(spp, entry):
    """[begin, end) of the rays of each workgroup of a focus state (refocus_kernel: chunk = ceil(spp / SPLIT))"""
    split = SPLIT[entry]
    chunk = (spp + split - 1) // split
    return [(p * chunk, min(spp, p * chunk + chunk)) for p in range(split)]


def last_second_ray(begin, end, nt):
    """the last ray of [begin, end) that is the second ray of a lane (i1 = i + NT of a pass of 2 NT rays), or None"""
    for i in range(end - 1, begin - 1, -1):
        if (i - begin) % (2 * nt) >= nt:
            return i
    return None


def tail_positions(spp, entry):
    """where the outliers go, the last ray first: up to four at the end of every part, and the last second-ray lane of every part"""
    pos = []
    for begin, end in parts(spp, entry):
        if begin >= end:
            continue
        pos += [end - 1 - k for k in range(min(4, end - begin))]
        sec = last_second_ray(begin, end, NT[entry])
        if sec is not None:
            pos.append(sec)
    return sorted(set(pos), reverse=True)


def _newton(surf, o, d, ra):
    """Surf.newton (oracle/lens.py:100-130) returning, beside t, the residual that its validity test reads"""
    dx, dy, dz = d[..., 0], d[..., 1], d[..., 2]
    t0 = (surf.d - o[..., 2]) / dz
    t = t0
    ft = MAXT * torch.ones_like(o[..., 2])
    it = 0

    def residual(t, mask_fn):
        p = o + d * t.unsqueeze(-1)
        px, py = p[..., 0], p[..., 1]
        m = mask_fn(px, py) & (ra > 0)
        xm, ym = px * m, py * m
        ft = surf.sag_r2(xm ** 2 + ym ** 2) + surf.d - p[..., 2]
        dr2dt = 2 * ((dx ** 2 + dy ** 2) * t + (dx * o[..., 0] + dy * o[..., 1]))
        return ft, surf.dsag_dr2(xm ** 2 + ym ** 2) * dr2dt - dz

    while (torch.abs(ft) > TOL_LOOSE).any() and it < NEWTON_MAXITER:
        it += 1
        ft, dfdt = residual(t, surf.valid_loose)
        t = t - torch.clamp(ft / (dfdt + EPSILON), -STEP_BOUND, STEP_BOUND)
    t = t0 + (t - t0)
    ft, dfdt = residual(t, surf.valid_strict)
    t = t - torch.clamp(ft / (dfdt + EPSILON), -STEP_BOUND, STEP_BOUND)
    return t, ft


def react_clear(surf, rays):
    """(Surf.react(rays), clear_mm, clear_rel): the oracle's own step, and by how much each ray that reaches the surface alive clears the
    decisions of that step (inf for a ray that is dead already, and for a decision the ray does not reach)"""
    o, d, ra, w = rays.o, rays.d, rays.ra, rays.wvln
    out = surf.react(Rays(o.clone(), d.clone(), ra.clone(), w, normalize=False))
    alive = ra > 0
    inf = torch.full_like(ra, INF)
    forward = (d * ra.unsqueeze(-1))[..., 2].sum() > 0
    eta = surf.mat1.ior(w) / surf.mat2.ior(w) if forward else surf.mat2.ior(w) / surf.mat1.ior(w)
    rel = inf.clone()
    if surf.c.item() == 0:
        t = (surf.d - o[..., 2]) / d[..., 2]
        p = o + t.unsqueeze(-1) * d
        rad = torch.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2)
        mm = (rad - surf.r).abs()
        valid = (rad <= surf.r) & alive
        refracts = eta != 1
    else:
        t, ft = _newton(surf, o, d, ra)
        p = o + t.unsqueeze(-1) * d
        rad = torch.sqrt(p[..., 0] ** 2 + p[..., 1] ** 2)
        mm = torch.minimum((rad - surf.r).abs(), t.abs())
        if surf.ai is None and surf.k == 0:
            valid = (p[..., 0] ** 2 + p[..., 1] ** 2 <= surf.r ** 2) & (t >= 0) & alive
            rel = torch.where(valid & ~(ft.abs() < TOL_TIGHT), torch.zeros_like(ra), inf)      # an arbitrary point that counts
        else:
            if surf.k > -1:
                mm = torch.minimum(mm, (rad - math.sqrt((1 - EPSILON) / float(surf.c) ** 2 / (1 + float(surf.k)))).abs())
            valid = surf.valid_strict(p[..., 0], p[..., 1]) & (ft.abs() < TOL_TIGHT) & alive & (t > 0)
            rel = (ft.abs() - TOL_TIGHT).abs() / TOL_TIGHT
        refracts = True
    if refracts:
        p = torch.where(valid.unsqueeze(-1), p, o)
        n = surf.normal(p, ra * valid)
        if (d * (ra * valid).unsqueeze(-1))[..., 2].sum() > 0:
            n = -n
        c2 = torch.sum(d * n, axis=-1) ** 2
        rel = torch.minimum(rel, torch.where(valid, torch.minimum((c2 - 0.1).abs() / 0.1, (eta ** 2 * (1 - c2) - 1).abs()), inf))
    return out, torch.where(alive, mm, inf), torch.where(alive, rel, inf)


def refocus_rays(lens, depth, u_theta, u_r):
    """deeplens/optics.py:1166-1170 on given draws; depth a float or one value per ray"""
    s0 = lens.surfaces[0]
    dt = torch.get_default_dtype()
    theta = torch.as_tensor(u_theta).to(dt) * 2 * np.pi
    r = torch.sqrt(torch.as_tensor(u_r).to(dt) * s0.r ** 2)
    x2, y2 = r * torch.cos(theta), r * torch.sin(theta)
    o = torch.stack((x2, y2, torch.full_like(x2, s0.d.item())), 1)
    src = torch.stack((torch.zeros_like(x2), torch.zeros_like(x2), torch.as_tensor(depth).to(dt).expand_as(x2)), 1)
    return Rays(o, o - src, wvln=DEFAULT_WAVE)


def focus_distances(ray):
    """deeplens/optics.py:1171-1175: (focus_d, counted) of every ray"""
    t = (ray.d[..., 0] * ray.o[..., 0] + ray.d[..., 1] * ray.o[..., 1]) / (ray.d[..., 0] ** 2 + ray.d[..., 1] ** 2)
    t = t * ray.ra
    fd = ray.o[..., 2] - ray.d[..., 2] * t
    return fd, (ray.ra > 0) & ~torch.isnan(fd) & (fd > 0)


def trace_focus(lens, depth, u_theta, u_r, clear=False):
    """(focus_d, counted[, clear]) as numpy: the oracle in the default dtype; clear [n] bool: every decision cleared by the margins"""
    rays = refocus_rays(lens, depth, u_theta, u_r)
    if not clear:
        fd, ok = focus_distances(lens.trace(rays))
        return fd.numpy(), ok.numpy()
    mm = torch.full_like(rays.ra, INF)
    rel = mm.clone()
    for s in lens.surfaces:
        rays, m, r = react_clear(s, rays)
        mm, rel = torch.minimum(mm, m), torch.minimum(rel, r)
    fd, ok = focus_distances(rays)
    mm = torch.minimum(mm, torch.where(rays.ra > 0, fd.abs(), torch.full_like(fd, INF)))
    return fd.numpy(), ok.numpy(), ((mm >= CLEAR_MM) & (rel >= CLEAR_REL)).numpy()


class DrawSet:
    """One block of draws [3 states][stride] for an entry and an spp, and everything the tests hold the kernel to."""

    def __init__(self, name, entry, spp):
        self.name, self.entry, self.spp, self.stride = name, entry, spp, stride_of(spp)
        self.ut = np.zeros((len(DEPTHS), spp), np.float32)
        self.ur = np.zeros((len(DEPTHS), spp), np.float32)

    @property
    def key(self):
        return (self.entry, self.spp)

    def block(self, pad=0):
        """the flat float32 block the kernel reads, `pad` floats of gap fill behind it"""
        S, spp = len(DEPTHS), self.spp
        u = np.empty(S * self.stride + pad, np.float32)
        u[0::2], u[1::2] = GAP_FILL[0], GAP_FILL[1]
        for s in range(S):
            u[s * self.stride:s * self.stride + spp] = self.ut[s]
            u[s * self.stride + spp:s * self.stride + 2 * spp] = self.ur[s]
        return u


def _flat(sets):
    ut = np.concatenate([d.ut.reshape(-1) for d in sets])
    ur = np.concatenate([d.ur.reshape(-1) for d in sets])
    dep = np.concatenate([np.repeat(np.asarray(DEPTHS), d.spp) for d in sets])
    return ut, ur, dep


def _split(sets, *arrays):
    out, at = [], 0
    for d in sets:
        n = len(DEPTHS) * d.spp
        out.append(tuple(a[at:at + n].reshape(len(DEPTHS), d.spp) for a in arrays))
        at += n
    return out


def oracle_lens(name, dtype):
    """the oracle lens in `dtype`; its exit pupil does not depend on d_sensor and is computed once"""
    with default_dtype(dtype):
        lens = OracleLens(lens_file(name), sensor_res=(64, 64))
        pupil = lens.exit_pupil(shrink_pupil=True)
        full, lens.enp_r = lens.exit_pupil(), lens.entrance_pupil()[1]
        lens.exit_pupil = lambda shrink_pupil=False: pupil if shrink_pupil else full
    return lens


def lens_state_at(lens, d_sensor):
    """float64 post_computation at a given d_sensor: dict of FIELDS (optics.py:178-187, :1097-1102, :1187-1217)"""
    lens.d_sensor = d_sensor
    hfov = lens.calc_fov()
    tan = float(np.tan(hfov))
    foclen = lens.r_last / tan
    return dict(hfov=hfov, tan_hfov=tan, foclen=foclen, fnum=foclen / lens.enp_r / 2)


def _place_tail(d, s, fd, ok):
    """permute the draws of state s so that the valid rays furthest from the mean sit at tail_positions, the furthest last"""
    pos = tail_positions(d.spp, d.entry)
    valid = np.flatnonzero(ok)
    far = valid[np.argsort(-np.abs(fd[valid] - fd[valid].mean()), kind="stable")][:len(pos)]
    pos = pos[:len(far)]
    perm = np.empty(d.spp, np.int64)
    perm[pos] = far
    perm[np.setdiff1d(np.arange(d.spp), pos)] = np.setdiff1d(np.arange(d.spp), far)
    # a read of the r row at +2048 of a launch with spp = 2048 - k skips the first k radii and takes the gap's (valid) fill for the
    # last k: the rays it skips are invalid ones, so that the count moves
    for j in range(2048 - d.spp if 0 < 2048 - d.spp <= GAP else 0):
        if ok[perm[j]]:
            i = next(i for i in range(2048 - d.spp, d.spp) if not ok[perm[i]])
            perm[j], perm[i] = perm[i], perm[j]
    d.ut[s], d.ur[s] = d.ut[s][perm], d.ur[s][perm]


@functools.lru_cache(maxsize=None)
def draw_sets(name):
    """{(entry, spp): DrawSet} of one lens, with the float64 reference and the float32 oracle's distance from it per state:
    fd, ok [3, spp], count [3], d_sensor [3], state [3] (dict of FIELDS), ok32 [3, spp], floor_d [3], floor[field] [3]"""
    rng = np.random.default_rng(SEED + LENSES.index(name))
    sets = [DrawSet(name, e, spp) for e, spps in (("plain", PLAIN_SPP), ("staged", STAGED_SPP)) for spp in spps]
    for d in sets:
        d.ut[:], d.ur[:] = rng.random(d.ut.shape, dtype=np.float32), rng.random(d.ur.shape, dtype=np.float32)
    with default_dtype(torch.float64):
        lens = oracle_lens(name, torch.float64)
        # clear draws of either kind per depth, for the sets whose share of invalid rays is out of range
        pool = {}
        for k, dep in enumerate(DEPTHS):
            pt, pr = rng.random(512, dtype=np.float32), rng.random(512, dtype=np.float32)
            _, ok, clear = trace_focus(lens, dep, pt, pr, clear=True)
            pool[k] = {kind: [(pt[i], pr[i]) for i in np.flatnonzero(clear & (ok == kind))] for kind in (True, False)}
        for _ in range(40):
            _, ok, clear = trace_focus(lens, torch.from_numpy(_flat(sets)[2]), *_flat(sets)[:2], clear=True)
            done = bool(clear.all())
            for d, (ok_d, clear_d) in zip(sets, _split(sets, ok, clear)):
                for s, i in zip(*np.nonzero(~clear_d)):
                    d.ut[s, i], d.ur[s, i] = rng.random(dtype=np.float32), rng.random(dtype=np.float32)
                n, bad = ok_d.size, int((~ok_d).sum())
                want = 0 if d.spp == 1 else min(max(bad, math.ceil(INVALID_MIN * n)), math.floor(INVALID_MAX * n))
                for k in range(abs(want - bad)):
                    s = k % len(DEPTHS)
                    to_valid = bad > want
                    cand = np.flatnonzero(~ok_d[s] if to_valid else ok_d[s])
                    if len(cand) == 0 or (not to_valid and len(cand) == 1):          # a state keeps a valid ray
                        s = int(np.argmax(ok_d.sum(1))) if not to_valid else int(np.argmin(ok_d.sum(1)))
                        cand = np.flatnonzero(~ok_d[s] if to_valid else ok_d[s])
                    i = int(cand[0])
                    d.ut[s, i], d.ur[s, i] = pool[s][to_valid].pop()
                    ok_d[s, i] = to_valid
                    done = False
                for s in range(len(DEPTHS)):                                         # no state without a valid ray (flags == 0)
                    if not ok_d[s].any():
                        d.ut[s, 0], d.ur[s, 0] = pool[s][True].pop()
                        ok_d[s, 0] = True
                        done = False
            if done:
                break
        else:
            raise AssertionError("the draws did not settle")
        fd, ok = trace_focus(lens, torch.from_numpy(_flat(sets)[2]), *_flat(sets)[:2])
        for d, (fd_d, ok_d) in zip(sets, _split(sets, fd, ok)):
            for s in range(len(DEPTHS)):
                _place_tail(d, s, fd_d[s], ok_d[s])
            # focus_d does not depend on theta (the object point is on the axis), so a kernel that read the r row 2048 floats behind the
            # theta row would, at spp = 2049, trace the same radii but one - ut[2048] in place of ur[2048] - and move the mean of 1500
            # rays by less than any tolerance.  The theta draws that such a read takes for radii are therefore in [0.9, 1): rim rays,
            # which the stop removes, where the true last ray is valid - the count decides
            d.ut[:, 2048:] = np.float32(0.9) + np.float32(0.1) * d.ut[:, 2048:]
        fd, ok, clear = trace_focus(lens, torch.from_numpy(_flat(sets)[2]), *_flat(sets)[:2], clear=True)
        for d, (fd_d, ok_d, clear_d) in zip(sets, _split(sets, fd, ok, clear)):
            d.fd, d.ok, d.clear = fd_d, ok_d, clear_d
            d.count = ok_d.sum(1)
            d.d_sensor = np.array([fd_d[s][ok_d[s]].mean() for s in range(len(DEPTHS))])
            d.state = [lens_state_at(lens, float(z)) for z in d.d_sensor]
    with default_dtype(torch.float32):
        lens32 = oracle_lens(name, torch.float32)
        ut, ur, dep = _flat(sets)
        fd, ok = trace_focus(lens32, torch.from_numpy(dep.astype(np.float32)), ut, ur)
        for d, (fd_d, ok_d) in zip(sets, _split(sets, fd, ok)):
            d.ok32 = ok_d
            d32 = np.array([float(np.mean(fd_d[s][ok_d[s]])) for s in range(len(DEPTHS))])          # np.mean of float32, as the reference
            d.floor_d = np.abs(d32 - d.d_sensor) / d.d_sensor
            st32 = [lens_state_at(lens32, float(z)) for z in d32]
            d.floor = {f: np.array([abs(st32[s][f] - d.state[s][f]) / abs(d.state[s][f]) for s in range(len(DEPTHS))]) for f in FIELDS}
    return {d.key: d for d in sets}


@functools.lru_cache(maxsize=None)
def tolerances():
    """{'d_sensor' and FIELDS: 4 x the largest float32-oracle distance over every state of every draw set of both lenses, <= 1e-5}"""
    sets = [d for name in LENSES for d in draw_sets(name).values()]
    tol = {"d_sensor": max(float(d.floor_d.max()) for d in sets)}
    tol.update({f: max(float(d.floor[f].max()) for d in sets) for f in FIELDS})
    return {k: min(PROJECT_TOL, 4 * v) for k, v in tol.items()}


def focus_check(count, d_sensor, ref_count, ref_d_sensor, tol):
    """the check the GPU test applies to a state: the count exactly, d_sensor within tol (relative)"""
    return int(count) == int(ref_count) and abs(d_sensor - ref_d_sensor) <= tol * abs(ref_d_sensor)


MUTATIONS = ("drop_last", "last_twice", "drop_second_of_last_pair", "u_r_at_2048")


def mutated_reference(d, s, what, lens):
    """(count, d_sensor) of a float64 reference with one of the tail bugs, or None where the launch has no such ray"""
    fd, ok = d.fd[s], d.ok[s]
    w = ok.astype(np.float64)
    if what == "drop_last":
        w[-1] = 0
    elif what == "last_twice":
        w[-1] *= 2
    elif what == "drop_second_of_last_pair":
        sec = [last_second_ray(b, e, NT[d.entry]) for b, e in parts(d.spp, d.entry) if b < e]
        sec = [i for i in sec if i is not None]
        if not sec:
            return None
        w[max(sec)] = 0
    elif what == "u_r_at_2048":
        u = d.block(pad=2048 + d.spp)
        with default_dtype(torch.float64):
            fd, ok = trace_focus(lens, DEPTHS[s], d.ut[s], u[s * d.stride + 2048:s * d.stride + 2048 + d.spp])
        w = ok.astype(np.float64)
    n = w.sum()
    return int(n), float((np.where(w > 0, fd, 0.0) * w).sum() / n) if n else float("nan")


# ------------------------------------------------------------------------------------------------------------------ B. histogram
SPLAT_KS = (2, 3, 11, 12, 31, 51)
SPLAT_SPP = (1, 255, 257, 1000)
SPLAT_N = (1, 3)
FRACTIONAL_CASE = (11, 257, 3)                       # (ks, spp, N): the one case with weights other than 0 and 1
CENTRES = np.array([[0.75, -1.25], [-2.5, 0.375], [1.875, 2.625]], np.float32)      # mm; few mantissa bits: -centre is a hit at X = 0
EMPTY_POINT = 1                                      # of N = 3: no ray inside
COORD_ULPS = 3
HIT_CLEAR = 1e-4
SPLAT_THREADS, NORMALISE_THREADS = 256, 512
SPLAT_MUTATIONS = ("swap_xy", "no_flip", "window_at_hi", "ra0_counted", "drop_last", "previous_centre", "centre_shifted")


def pixel_size(name, res=1024):
    """float32 pixel size of a shipped lens on a res x res sensor (deeplens/optics.py:153-175)"""
    with open(lens_file(name)) as f:
        r_last = json.load(f)["r_last"]
    return float(np.float32(2 * r_last * res / np.sqrt(2 * res * res) / res))


def window(ps, ks):
    lo, hi = (-ks / 2 + 0.5) * ps, (ks / 2 - 0.5) * ps
    return lo, hi, hi - 0.01 * ps


def bin_coordinates(o_xy, ra, centre, ps, ks, mutate=None):
    """monte_carlo.py:24-38 and :60-70 in float64: (rowf, colf, weight) [spp, N] of every ray, and the unscaled shift [spp, N, 2]"""
    o_xy, ra, centre = (np.asarray(a, np.float64) for a in (o_xy, ra, centre))
    lo, hi, lim = window(ps, ks)
    if mutate == "window_at_hi":
        lim = hi
    if mutate == "previous_centre":
        centre = np.roll(centre, 1, axis=0)
    if mutate == "centre_shifted":
        centre = centre + 1e-3 * ps
    if mutate == "ra0_counted":
        ra = np.where(ra == 0, 1.0, ra)
    if mutate == "drop_last":
        ra = ra.copy()
        ra[-1] = 0
    shift = (o_xy if mutate == "no_flip" else -o_xy) - centre[None]
    if mutate == "swap_xy":
        shift = shift[..., ::-1]
    w = ra * (np.abs(shift[..., 0]) < lim) * (np.abs(shift[..., 1]) < lim)
    scaled = shift * w[..., None]
    if ks == 1:
        raise ValueError("ks = 1: the reference's window is empty and its bin coordinate is 0 / 0")
    rowf = (scaled[..., 1] - hi) / (lo - hi) * (ks - 1)
    colf = (scaled[..., 0] - lo) / (hi - lo) * (ks - 1)
    return rowf, colf, w, shift


def splat_reference(o_xy, ra, centre, ps, ks, mutate=None):
    """(raw [N,ks,ks], A [N,ks,ks], n [N,ks,ks]) in float64: the histogram of monte_carlo.py:60-121, and per bin the summed weight and the
    number of the counted rays within one pixel of it"""
    rowf, colf, w, _ = bin_coordinates(o_xy, ra, centre, ps, ks, mutate)
    N = w.shape[1]
    raw, A, cnt = (np.zeros((N, ks, ks)) for _ in range(3))
    fr, fc = np.floor(rowf), np.floor(colf)
    wb, wr = rowf - fr, colf - fc
    taps = ((fr, fc, (1 - wb) * (1 - wr)), (fr, np.floor(colf + 1), (1 - wb) * wr), (np.floor(rowf + 1), fc, wb * (1 - wr)), (fr + 1, fc + 1, wb * wr))
    rr, cc = np.arange(ks)[:, None, None], np.arange(ks)[None, :, None]
    for n in range(N):
        for r, c, v in taps:
            np.add.at(raw[n], (r[:, n].astype(np.int64), c[:, n].astype(np.int64)), v[:, n] * w[:, n])
        k = w[:, n] > 0
        near = (np.abs(rowf[k, n][None, None] - rr) <= 1) & (np.abs(colf[k, n][None, None] - cc) <= 1)
        A[n], cnt[n] = (near * w[k, n]).sum(-1), near.sum(-1)
    return raw, A, cnt


def splat_bounds(raw, A, cnt, ks):
    """(bound of raw, bound of the normalised PSF) per element; module docstring B"""
    b = U * (2 * COORD_ULPS * (ks - 1) + 4) * A + cnt * U * raw
    T = raw.sum((1, 2), keepdims=True)
    depth = -(-ks * ks // SPLAT_THREADS) - 1 + 6 + 3
    with np.errstate(invalid="ignore", divide="ignore"):
        bp = b / T + raw / T * (b.sum((1, 2), keepdims=True) / T + (depth + 1) * U)
    return b, bp


def splat_check(got_raw, got_psf, ref):
    """(worst |raw - ref| / bound, worst |psf - ref| / bound, NaN positions equal); a bin with bound 0 must be equal"""
    raw, A, cnt, ks = ref
    b, bp = splat_bounds(raw, A, cnt, ks)
    T = raw.sum((1, 2), keepdims=True)
    with np.errstate(invalid="ignore", divide="ignore"):
        psf = raw / T

    def worst(err, bound):
        bad = err > bound
        with np.errstate(invalid="ignore", divide="ignore"):
            ratio = np.where(bound > 0, err / bound, np.where(bad, INF, 0.0))
        return float(ratio.max())
    r_raw = worst(np.abs(np.asarray(got_raw, np.float64) - raw), b) if got_raw is not None else 0.0
    nan_ref = np.isnan(psf)
    nan_ok = got_psf is None or bool(np.array_equal(np.isnan(got_psf), nan_ref))
    r_psf = 0.0
    if got_psf is not None and nan_ok:
        r_psf = worst(np.abs(np.asarray(got_psf, np.float64) - psf)[~nan_ref], bp[~nan_ref]) if (~nan_ref).any() else 0.0
    return r_raw, r_psf, nan_ok


@functools.lru_cache(maxsize=None)
def splat_case(name, ks, spp, N):
    """(o [spp,N,3], ra [spp,N], centre [N,2], ps) float32: synthetic hits of every kind, mixed; the last ray of a point is well inside
    (but for EMPTY_POINT of N = 3, which has no ray inside at all)"""
    ps = pixel_size(name)
    lo, hi, lim = window(ps, ks)
    rng = np.random.default_rng(1000 * ks + 10 * spp + N + LENSES.index(name))
    centre = CENTRES[:N]
    i, n = np.meshgrid(np.arange(spp), np.arange(N), indexing="ij")
    kind = (i + 3 * n) % 9                               # 0, 1, 2, 8: well inside; 3 ... 7 below
    kind[-1] = 0
    if N == 3:
        kind[:, EMPTY_POINT] = 3 + i[:, EMPTY_POINT] % 3
    if ks % 2 == 0:
        kind[kind == 6] = 0
    if (ks, spp, N) != FRACTIONAL_CASE:
        kind[kind == 7] = 0
    o = np.zeros((spp, N, 3), np.float32)
    ra = np.ones((spp, N), np.float32)
    todo = np.ones((spp, N), bool)
    for _ in range(200):
        m = int(todo.sum())
        k, ii = kind[todo], i[todo]
        sign = lambda: np.where(rng.random(m) < 0.5, 1.0, -1.0)
        X, Y, w = rng.uniform(-lim, lim, m), rng.uniform(-lim, lim, m), np.ones(m)
        X = np.where(k == 3, sign() * rng.uniform(lim + 2 * HIT_CLEAR * ps, hi - 2 * HIT_CLEAR * ps, m), X)     # the ring: contributes nothing
        far = sign() * rng.uniform(hi + 0.1 * ps, hi + 3 * ps, m)                                                # outside in one coordinate only
        X, Y = np.where((k == 4) & (ii % 2 == 1), far, X), np.where((k == 4) & (ii % 2 == 0), far, Y)
        w = np.where(k == 5, 0.0, w)                                                                             # a dead ray inside the window
        X, Y = np.where((k == 6) & (ii // 9 % 3 != 1), 0.0, X), np.where((k == 6) & (ii // 9 % 3 != 0), 0.0, Y)            # exactly on the centre tap
        w = np.where(k == 7, rng.choice([0.25, 0.5, 0.75], m), w)                                                # a weight other than 0 and 1
        c = np.broadcast_to(centre[None].astype(np.float64), (spp, N, 2))[todo]
        o[todo, 0], o[todo, 1], ra[todo] = -(c[:, 0] + X), -(c[:, 1] + Y), w
        todo = ~clear_hits(o[..., :2], ra, centre, ps, ks)
        if not todo.any():
            break
    else:
        raise AssertionError("no clear hits found")
    o[..., 2] = rng.uniform(50, 60, (spp, N)).astype(np.float32)          # the sensor plane's z: not read
    return o, ra, centre, ps, kind


def clear_hits(o_xy, ra, centre, ps, ks):
    """[spp,N] bool: the hit is >= 1e-4 ps from the window limit in both coordinates, and - where the ray counts - a bin coordinate that
    is not an integer is >= 1e-4 from one (the kernel keeps the reference's floor(f + 1), which one ulp below 1, 3, 7, 15, 31 differs from
    floor(f) + 1 in fp32 by design)"""
    rowf, colf, w, shift = bin_coordinates(o_xy, ra, centre, ps, ks)
    lim = window(ps, ks)[2]
    ok = (np.abs(np.abs(shift) - lim) >= HIT_CLEAR * ps).all(-1)
    frac = np.stack([np.abs(f - np.round(f)) for f in (rowf, colf)])
    return ok & ((w == 0) | ((frac == 0) | (frac >= HIT_CLEAR)).all(0))


# ------------------------------------------------------------------------------------------------------------------ C. normalise
NORM_S, NORM_L = 2, 3
NORM_N = (1, 4, 9)
NORM_KS = (3, 12, 51)


def normalise_depth(ks):
    return -(-ks * ks // NORMALISE_THREADS) - 1 + 6 + (NORMALISE_THREADS // 64 - 1)


@functools.lru_cache(maxsize=None)
def normalise_case(N, ks):
    """raw [S*L][N][ks*ks] float32 >= 0, every tile on a scale of its own (a mis-tiled element is off by a factor), one tile all zero"""
    rng = np.random.default_rng(100 * N + ks)
    raw = rng.random((NORM_S * NORM_L, N, ks * ks)).astype(np.float32)
    raw *= np.float32(3.0) ** np.arange(NORM_S * NORM_L * N, dtype=np.float32).reshape(NORM_S * NORM_L, N, 1)
    zero = (NORM_S * NORM_L - 2, N - 1)
    raw[zero] = 0
    return raw, zero


def normalise_reference(raw, N, ks, layout):
    """float64 raw / sum(raw) in the layout of aadff_psf_points: 0 = [S,N,L,ks,ks], 1 = psf_map tiling [S,L,g*ks,g*ks]"""
    with np.errstate(invalid="ignore", divide="ignore"):
        p = (raw.astype(np.float64) / raw.astype(np.float64).sum(-1, keepdims=True)).reshape(NORM_S, NORM_L, N, ks, ks)
    if layout == 0:
        return p.transpose(0, 2, 1, 3, 4)
    g = int(round(N ** 0.5))
    return p.reshape(NORM_S, NORM_L, g, g, ks, ks).transpose(0, 1, 2, 4, 3, 5).reshape(NORM_S, NORM_L, g * ks, g * ks)
