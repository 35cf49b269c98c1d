"""GPU: the ray-traced MTF (aadff_mtf_points behind aadff.mtf / Lensgroup.mtf) against the float64 restatement of its
rule on the CPU oracle (tests/mtf_common.py): counts per field, the OTF element by element against a float32 floor computed in the
run and taken per frequency, exactness at zero frequency, the centroids, the composed route (sample_pupil -> trace -> torch float64
sums) on the same draws, reproducibility, the through-focus peak, the distortion grid and the refusals."""
import functools
import os

import numpy as np
import pytest
import torch

import mtf_common as mc
from aadff import _abi, mtf
from deeplens.basics import DEFAULT_WAVE, DEPTH, GEO_SPP, WAVE_RGB
from deeplens.optics import Lensgroup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"
# (lens, spp, frequencies): spp 64 = 8 sectors x 8 rings, fewer rays than lanes (the second ray of every pair is inactive); spp 520 =
# several iterations per lane, the last one partly active; F = 48 x Z = 3 x 2 axes = 288 entries, more than the 256 lanes
CASES = [("rf50mm", 64, "five"), ("50mm_f2.8", 64, "five"), ("rf50mm", 520, "five"), ("50mm_f2.8", 64, "many")]
IDS = [f"{n}-spp{s}-{k}" for n, s, k in CASES]


def make_lens(name, parity="fast"):
    """the sensor by its size, so that the reference's exact float test for square pixels holds (see tests/test_gpu_raytrace.py)"""
    h, w = mc.RES
    lens = Lensgroup(mc.lens_file(name), device=DEV, post_computation=False, parity=parity)
    ws = 2 * lens.r_last * w / np.sqrt(h ** 2 + w ** 2)
    lens.prepare_sensor(mc.RES, sensor_size=[ws * h / w, ws])
    lens.post_computation()
    return lens


@functools.lru_cache(maxsize=None)
def shared_lens(name):
    lens = make_lens(name)
    torch.manual_seed(mc.SEED)
    lens.refocus(mc.DEPTH)
    return lens


def grid_points(lens):
    """3 x 3 object points over the full field at DEPTH: the axis, the edges, the vignetted corners"""
    return lens._point_grid(lens.sensor_size[0] / 2 * lens.calc_scale_pinhole(mc.DEPTH), mc.DEPTH, 3).reshape(-1, 3)


def freqs_of(lens, kind):
    if kind == "five":
        return mc.FREQS + (float(np.float32(0.5 / lens.pixel_size)),)
    return tuple(float(v) for v in np.linspace(0, 80, 48, dtype=np.float32))


class _Replay:
    """a sampler that hands the lens the given block, in one draw or in consecutive ones (the stream a host generator would give)"""
    on_device = False

    def __init__(self, block):
        self.block, self.at = torch.as_tensor(block).reshape(-1).clone(), 0

    def rand_block(self, sizes):
        n = int(sum(sizes))
        assert self.at + n <= self.block.numel()
        self.at += n
        return self.block[self.at - n:self.at].clone()

    def rand_into(self, out):
        return out.copy_(self.rand_block([out.numel()]))


@functools.lru_cache(maxsize=None)
def kernel_case(name, spp, kind):
    """(reference case fed the GPU lens's own d_sensor, entrance pupil and object points; kernel otf [L,P,Z,2,F] complex; moments [L,P,8])"""
    lens = shared_lens(name)
    pz, pr = lens.entrance_pupil()
    pts = grid_points(lens)
    freqs = freqs_of(lens, kind)
    case = mc.reference_case(name, float(lens.d_sensor), (float(pz), float(pr)), mc.points_key(pts), spp, freqs, mc.DEFOCUS)
    raw, mom = mtf._launch(lens, pts, torch.as_tensor(case["u"]).reshape(-1), list(WAVE_RGB), list(freqs), list(mc.DEFOCUS), spp, "radial")
    return case, torch.view_as_complex(raw.contiguous()), mom, freqs


def bound_check(margin, tag, got, want, usable, floor, freqs):
    """per frequency, on the usable fields: |got - want| <= 4 x floor for the real part, the imaginary part and the modulus"""
    d = got.to(torch.complex128) - want.to(torch.complex128)
    dm = (got.abs().double() - want.abs().double()).abs()
    m = usable[:, :, None, None, None]
    worst = torch.stack([(d.real.abs() * m).amax(dim=(0, 1, 2, 3)), (d.imag.abs() * m).amax(dim=(0, 1, 2, 3)), (dm * m).amax(dim=(0, 1, 2, 3))])
    top = 0.0
    for f, nu in enumerate(freqs):
        w, fl = float(worst[:, f].max()), float(floor[f])
        if nu == 0:
            assert fl == 0 and w == 0, f"{tag}: nu = 0 must be exact, got {w:.3e} (floor {fl:.3e})"
            continue
        assert fl > 0
        print(f"{tag} nu={nu:g}: re {float(worst[0, f]):.3e} im {float(worst[1, f]):.3e} mtf {float(worst[2, f]):.3e}, float32 floor {fl:.3e}, "
              f"ratio {w / fl:.2f}")
        top = max(top, w / (4 * fl))
        assert w <= 4 * fl, f"{tag} nu={nu:g}: {w:.3e} exceeds 4 x float32 floor {fl:.3e} (ratio {w / fl:.2f})"
    margin(f"{tag}: worst |d| / (4 x f32 floor) over frequencies", top, 1.0)


@pytest.mark.parametrize("name,spp,kind", CASES, ids=IDS)
def test_counts_per_field(name, spp, kind):
    """The inputs are fit for the comparison (robust rays are nearly all rays), and on every usable field - all rays robust, float32
    validity equal to float64's - the kernel counts the rays float64 counts"""
    case, _, mom, _ = kernel_case(name, spp, kind)
    assert float(case["robust"].double().mean()) >= 0.999
    assert float(case["usable"].double().mean()) >= 0.9
    assert float(case["ref"]["n"].min()) >= 1
    assert torch.equal(mom[..., 0][case["usable"]].double(), case["ref"]["n"][case["usable"]])
    assert bool((mom[..., 5:] == 0).all())


@pytest.mark.parametrize("name,spp,kind", CASES, ids=IDS)
def test_otf_elementwise_against_float64(name, spp, kind, margin):
    """|kernel - float64| <= 4 F(nu) elementwise on the usable fields, F(nu) = the float32 restatement's own distance from float64 at
    that frequency in this run.  The factor 4 is the one tests/test_gpu_raytrace.py grants the same trace arithmetic (one-ulp rcp / rsq /
    sin / cos hardware forms, FMA contraction).  Measured on one MI355X: DESIGN.md 4.17."""
    case, otf, _, freqs = kernel_case(name, spp, kind)
    assert otf.shape == case["ref"]["otf"].shape and bool(torch.isfinite(torch.view_as_real(otf)).all())
    bound_check(margin, f"mtf {name} spp {spp} {kind}", otf, case["ref"]["otf"], case["usable"], mc.otf_floor(case), freqs)


@pytest.mark.parametrize("name,spp,kind", CASES[:3], ids=IDS[:3])
def test_zero_frequency_is_exact(name, spp, kind):
    case, otf, mom, freqs = kernel_case(name, spp, kind)
    assert freqs[0] == 0
    seen = mom[..., 0] > 0
    assert bool(seen.all())
    assert bool((otf[..., 0].abs() == 1.0).all()) and bool((otf[..., 0].real == 1.0).all()) and bool((otf[..., 0].imag == 0.0).all())


@pytest.mark.parametrize("name,spp,kind", CASES[:3], ids=IDS[:3])
def test_centroids(name, spp, kind, margin):
    """sum x / n, sum y / n, sum a / n, sum b / n under the same 4 x floor rule, per quantity"""
    case, _, mom, _ = kernel_case(name, spp, kind)
    got = mom[..., 1:5].double() / mom[..., 0:1].double()
    floor = mc.mean_floor(case)
    d = ((got - case["ref"]["mean"]).abs() * case["usable"][:, :, None]).amax(dim=(0, 1))
    for i, q in enumerate(("x [mm]", "y [mm]", "a", "b")):
        assert float(floor[i]) > 0
        print(f"mtf {name} spp {spp} mean {q}: kernel {float(d[i]):.3e}, float32 floor {float(floor[i]):.3e}, ratio {float(d[i] / floor[i]):.2f}")
        margin(f"mtf {name} spp {spp}: mean {q} |kernel - f64| / (4 x f32 floor)", float(d[i] / (4 * floor[i])), 1.0)


@pytest.mark.parametrize("name", mc.LENSES)
def test_composed_route_like_with_like(name, margin):
    """The same draws through sample_pupil -> lens.trace (the generic kernel) -> project_to -> torch float64 sums: fields of equal count
    within the bound of the OTF test"""
    case, otf, mom, freqs = kernel_case(name, 64, "five")
    lens = make_lens(name)
    lens.d_sensor = shared_lens(name).d_sensor
    lens.sampler = _Replay(case["u"][0])
    comp, cmom = [], []
    for q, w in enumerate(WAVE_RGB):
        lens.sampler = _Replay(case["u"][q])
        o, m = mtf._composed(lens, torch.as_tensor(case["points"]), [w], list(freqs), list(mc.DEFOCUS), 64, "radial")
        comp.append(o[0]), cmom.append(m[0])
    comp, cmom = torch.stack(comp), torch.stack(cmom)
    margin(f"mtf {name} fused vs composed: valid count per field", float((cmom[..., 0] - mom[..., 0].double()).abs().max()), 2)
    same = cmom[..., 0] == mom[..., 0].double()
    assert float(same.double().mean()) >= 0.9
    bound_check(margin, f"mtf {name} fused vs composed", otf, comp, same & case["usable"], mc.otf_floor(case), freqs)


def test_strict_lens_composed_route_against_float64(margin):
    """A strict lens takes the composed route through the public call; on rf50mm it meets the float64 fixture of the OTF test"""
    name = "rf50mm"
    case, _, _, freqs = kernel_case(name, 64, "five")
    lens = make_lens(name, parity="strict")
    lens.d_sensor = shared_lens(name).d_sensor
    lens.sampler = _Replay(case["u"])
    launched = []
    orig = mtf._launch
    mtf._launch = lambda *a, **k: launched.append(1) or orig(*a, **k)
    try:
        res = mtf.mtf_points(lens, torch.as_tensor(case["points"]), list(freqs), WAVE_RGB, mc.DEFOCUS, 64, "radial")
    finally:
        mtf._launch = orig
    assert not launched and res.otf.dtype == torch.complex128
    got = res.otf.transpose(0, 1)
    same = (res.count.transpose(0, 1).double() == case["ref"]["n"]) & case["usable"]
    assert float(same.double().mean()) >= 0.9
    bound_check(margin, f"mtf {name} strict composed vs f64", got, case["ref"]["otf"], same, mc.otf_floor(case), freqs)


def test_reproducible_and_same_rays_as_spot_moments():
    """Two launches are bit-equal; the public call returns the launch's numbers; count, sum x and sum y equal aadff_spot_moments' on the
    same draws bit for bit (the same rays, summed in the same order)"""
    name, spp = "50mm_f2.8", 520
    lens = shared_lens(name)
    pts = grid_points(lens)
    freqs = freqs_of(lens, "five")
    u = torch.as_tensor(mc.uniforms(3, spp, pts.shape[0])).reshape(-1)
    a = mtf._launch(lens, pts, u, list(WAVE_RGB), list(freqs), list(mc.DEFOCUS), spp, "radial")
    b = mtf._launch(lens, pts, u, list(WAVE_RGB), list(freqs), list(mc.DEFOCUS), spp, "radial")
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    res = mtf.mtf_points(lens, pts, freqs, WAVE_RGB, mc.DEFOCUS, spp, "radial", u=u)
    assert tuple(res.mtf.shape) == (9, 3, 3, 2, 5) and tuple(res.centroid.shape) == (9, 3, 3, 2) and tuple(res.count.shape) == (9, 3)
    assert torch.equal(torch.view_as_real(res.otf.transpose(0, 1).contiguous()), a[0])
    saved = lens.sampler
    lens.sampler = _Replay(u)
    try:
        spot = lens._spot_moments(pts, list(WAVE_RGB), spp, 0, False)
    finally:
        lens.sampler = saved
    assert torch.equal(spot[..., :3], a[1][..., :3])


def test_through_focus_peak(margin):
    """rf50mm's axis point at 20 cycles/mm: the peak of mtf_through_focus lies within one step of the float64 restatement's"""
    name, steps, span = "rf50mm", 9, 0.4
    lens = shared_lens(name)
    pz, pr = lens.entrance_pupil()
    u = mc.uniforms(1, GEO_SPP, 1)
    saved = lens.sampler
    lens.sampler = _Replay(u)
    try:
        delta, curve, peak = lens.mtf_through_focus([0.0, 0.0, mc.DEPTH], 20.0, span, steps)
    finally:
        lens.sampler = saved
    assert tuple(curve.shape) == (steps, 2) and torch.equal(delta, torch.linspace(-span / 2, span / 2, steps, dtype=torch.float64))
    ref = mc.mtf_oracle(name, float(lens.d_sensor), (float(pz), float(pr)), np.array([[0.0, 0.0, mc.DEPTH]], dtype=np.float32), u, [20.0],
                        delta.tolist(), [DEFAULT_WAVE], "radial", torch.float64)["otf"].abs()[0, 0, :, :, 0]
    step = span / (steps - 1)
    for k, ax in enumerate("TS"):
        want = mtf.parabola_peak(delta, ref[:, k])
        i = int(torch.argmax(ref[:, k]))
        assert 0 < i < steps - 1, "the float64 curve peaks inside the span"
        print(f"through focus {ax}: peak {float(peak[k]):+.4f} mm, float64 {want:+.4f} mm, curve max {float(curve[:, k].max()):.3f}")
        margin(f"mtf through focus {ax}: |peak - f64 peak| / step", abs(float(peak[k]) - want) / step, 1.0)


def test_distortion_grid(repo_root, margin):
    """distortion_grid == the composed reference computation (optics.py:1944-1959) on the same seed, under test_gpu_spot.py's centroid
    rule (test_fused_against_composed: counts within 2 per field, centroids within 5e-5 mm on the fields of equal count, which are at
    least 0.9 of all - a ray that changes validity moves a centroid by its distance from it over 2048); torch's generator is left where
    sample_point_source leaves it"""
    lens = Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(480, 640), device=DEV)
    scale = lens.calc_scale_pinhole(DEPTH)
    R = lens.sensor_size[0] / 2 * scale
    torch.manual_seed(31)
    ray = lens.sample_point_source(M=16, spp=GEO_SPP, depth=DEPTH, R=R, pupil=True)
    o1 = ray.o.detach().cpu()
    ray, _, _ = lens.trace(ray)
    o2, ra = ray.project_to(lens.d_sensor).clone().cpu(), ray.ra.cpu()
    want = torch.stack((torch.sum(o2[..., 0] * ra, 0) / torch.sum(ra, 0), torch.sum(o2[..., 1] * ra, 0) / torch.sum(ra, 0)), -1)
    tail = torch.rand(8)
    torch.manual_seed(31)
    ideal, traced = lens.distortion_grid(DEPTH)
    assert torch.equal(torch.rand(8), tail)
    assert tuple(ideal.shape) == (16, 16, 2) and tuple(traced.shape) == (16, 16, 2)
    assert torch.equal(ideal, o1[0, :, :, :2] / scale)
    torch.manual_seed(31)                        # the launch distortion_grid made, for its counts
    mom = lens._spot_moments(lens._point_grid(R, DEPTH, 16).reshape(-1, 3), [DEFAULT_WAVE], GEO_SPP, 0, False)[0].reshape(16, 16, 4)
    assert torch.equal(traced, mom[..., 1:3] / mom[..., 0:1])
    margin("distortion_grid rf50mm vs composed: valid count per field", float((mom[..., 0] - ra.sum(0)).abs().max()), 2)
    same = mom[..., 0] == ra.sum(0)
    assert float(same.double().mean()) >= 0.9
    margin("distortion_grid rf50mm vs composed: centroid [mm] (fields of equal count)", float((traced - want)[same].abs().max()), 5e-5)


def test_draw_mtf_and_distortion(repo_root, tmp_path):
    pytest.importorskip("matplotlib")
    lens = Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(480, 640), device=DEV)
    name = lens.draw_mtf(save_name=str(tmp_path / "mtf"))
    assert name == str(tmp_path / "mtf") + ".png" and os.path.getsize(name) > 10_000
    name = lens.draw_distortion(save_name=str(tmp_path / "lens"))
    assert name == str(tmp_path / "lens") + f"_distortion{-DEPTH}mm.png" and os.path.getsize(name) > 5_000


def test_refusals_launch_nothing(monkeypatch):
    lens = shared_lens("rf50mm")
    pts = [[0.0, 0.0, mc.DEPTH], [0.5, 0.5, mc.DEPTH]]
    calls = []
    real = _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: calls.append(name) or real(name, *a))
    for kw, exc, reason in ((dict(freqs=[10.0], spp=60), ValueError, "multiple of 8"),
                            (dict(freqs=[10.0], spp=2056), ValueError, "exceeds 2048"),
                            (dict(freqs=[]), ValueError, "0 frequency values"),
                            (dict(freqs=list(range(129))), ValueError, "129 frequency values"),
                            (dict(freqs=[10.0], defocus=[0.01 * i for i in range(17)]), ValueError, "17 defocus values"),
                            (dict(freqs=[10.0, -1.0]), ValueError, "negative"),
                            (dict(freqs=[float("nan")]), ValueError, "non-finite"),
                            (dict(freqs=[float("inf")]), ValueError, "non-finite"),
                            (dict(freqs=[10.0], defocus=[float("inf")]), ValueError, "non-finite"),
                            (dict(freqs=[10.0], axes="diagonal"), ValueError, "radial")):
        with pytest.raises(exc, match=reason):
            lens.mtf(pts, **{"spp": 64, **kw})
    assert calls == []
    square = make_lens("rf50mm")
    calls.clear()
    square.surfaces[0].is_square = True
    with pytest.raises(NotImplementedError, match="square apertures"):
        square.mtf(pts, [10.0], spp=64)
    assert calls == []
