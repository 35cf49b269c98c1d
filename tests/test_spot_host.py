"""CPU: the host side of the ray-traced lens analysis (sample_pupil, the RMS / magnification formulas on per-field moments,
the aadff_spot_moments ABI entry) against fixture G17 (tests/golden/make_spot_golden.py) and against direct restatements of
the reference's formulas (deeplens/optics.py:539-591, 1221-1256, 1975-2012).  No GPU."""
import ctypes as C
import inspect
import json
import os
import re

import numpy as np
import pytest
import torch

from aadff import _abi
from aadff.sampling import HostSampler
from deeplens.basics import DEPTH, EPSILON
from deeplens.optics import Lensgroup

SIX = ("sample_pupil", "sample_point_source", "calc_magnification3", "calc_scale_ray", "analysis_rms", "draw_spot_diagram")


@pytest.fixture(scope="module")
def g17(golden_dir):
    return np.load(os.path.join(golden_dir, "g17_spot.npz")), json.load(open(os.path.join(golden_dir, "g17_spot.json")))


@pytest.fixture(scope="module")
def host_lens(repo_root):
    """a lens without its device state: sample_pupil with an explicit pupil needs no trace"""
    return Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(480, 640), post_computation=False, device="cpu")


def _per_call_pupil(res, spp, num_angle, pupilr, pupilz):
    """sample_pupil as the reference computes it (deeplens/optics.py:563-589): one torch.rand per reference call, float32
    torch operations on the reference's tensor shapes - evaluated on the CPU that runs the test"""
    H, W = res
    if spp % num_angle != 0 or spp >= 10000:
        theta = torch.rand((spp, H, W)) * 2 * np.pi
        r = torch.sqrt(torch.rand((spp, H, W)) * pupilr ** 2)
        x, y = r * torch.cos(theta), r * torch.sin(theta)
    else:
        xs, ys = [], []
        for i in range(num_angle):
            for j in range(spp // num_angle):
                theta = torch.rand((1, H, W)) * 2 * np.pi / num_angle + i * 2 * np.pi / num_angle
                r = torch.sqrt(torch.rand((1, H, W)) * pupilr ** 2 / spp * num_angle + j * pupilr ** 2 / spp * num_angle)
                xs.append(r * torch.cos(theta))
                ys.append(r * torch.sin(theta))
        x, y = torch.cat(xs), torch.cat(ys)
    return torch.stack((x, y, torch.full_like(x, pupilz)), -1)


@pytest.mark.parametrize("spp,res", [(16, (3, 4)), (12, (3, 4)), (2048, (31, 31)), (1024, (7, 7)), (20, (21, 21))])
def test_sample_pupil_bits_equal_the_per_call_computation(host_lens, spp, res):
    """Bit-equal to the reference's per-call computation on this CPU, both branches (spp 12 and 20: naive), and the
    generator is left where the reference leaves it"""
    torch.manual_seed(9)
    want = _per_call_pupil(res, spp, 8, 13.35, 19.81)
    tail_want = torch.rand(8)
    torch.manual_seed(9)
    got = host_lens.sample_pupil(res=res, spp=spp, num_angle=8, pupilr=13.35, pupilz=19.81)
    assert got.shape == (spp, *res, 3) and got.dtype == torch.float32
    assert torch.equal(got, want) and torch.equal(torch.rand(8), tail_want)


@pytest.mark.parametrize("tag", ["strat", "naive"])
def test_sample_pupil_against_reference_fixture(g17, host_lens, margin, tag):
    """Against the reference's own output (fixture G17) and its draw count.  The draws, r^2 and the square root are the same
    bits on every CPU; torch's float32 cos / sin are not (they dispatch to CPU-specific vector code), so x and y are held to
    the fixture within 4 ulp of the pupil radius - bit equality with the reference's operations is the test above."""
    arrays, meta = g17
    m = meta[f"pupil_{tag}"]
    torch.manual_seed(m["seed"])
    got = host_lens.sample_pupil(res=tuple(m["res"]), spp=m["spp"], num_angle=m["num_angle"], pupilr=m["pupilr"], pupilz=m["pupilz"])
    after = torch.rand(8).numpy()
    want = arrays[f"pupil_{tag}"]
    assert got.shape == want.shape and got.dtype == torch.float32
    assert np.array_equal(after, arrays[f"pupil_{tag}_rand8"])
    assert np.array_equal(got[..., 2].numpy(), want[..., 2])
    ulp = float(np.spacing(np.float32(m["pupilr"])))
    margin(f"G17 sample_pupil ({tag}) x / y [ulp of the pupil radius]", float(np.abs(got[..., :2].numpy() - want[..., :2]).max()) / ulp, 4)
    r_got, r_want = np.hypot(got[..., 0].numpy(), got[..., 1].numpy()), np.hypot(want[..., 0], want[..., 1])
    assert np.abs(r_got - r_want).max() <= 4 * ulp


@pytest.mark.parametrize("hw", [961, 441, 49, 12])
def test_one_flat_block_is_the_per_call_stream(hw):
    """sample_pupil draws 2 * spp blocks of H*W in one flat call: the same numbers as the reference's per-call torch.rand((1,H,W))"""
    spp = 16
    torch.manual_seed(5)
    want = torch.cat([torch.rand((1, hw)).reshape(-1) for _ in range(2 * spp)])
    tail_want = torch.rand(8)
    torch.manual_seed(5)
    got = HostSampler().rand_block([2 * spp * hw])
    assert torch.equal(got, want) and torch.equal(torch.rand(8), tail_want)


def test_six_methods_have_the_reference_signatures(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "g16_signatures.json")))["deeplens.optics"]
    import deeplens.basics as basics
    for name in SIX:
        want = ref[f"Lensgroup.{name}"]
        got = list(inspect.signature(getattr(Lensgroup, name)).parameters.values())
        assert [p.name for p in got] == [w[0] for w in want], name
        for p, (_, dflt) in zip(got, want):
            if dflt is None:
                assert p.default is inspect.Parameter.empty, (name, p.name)
                continue
            d = getattr(basics, dflt) if dflt.isupper() else eval(dflt)
            mine = p.default
            assert (list(mine) if isinstance(mine, tuple) else mine) == (list(d) if isinstance(d, tuple) else d), (name, p.name)


def test_spot_symbol_declared_exported_bound(repo_root):
    header = open(os.path.join(repo_root, "include", "aadff.h")).read()
    assert re.search(r"^int aadff_spot_moments\(", header, flags=re.M)
    assert "aadff_spot_moments" in _abi.PROTOTYPES and len(_abi.PROTOTYPES["aadff_spot_moments"]) == 16
    assert hasattr(C.CDLL(_abi.LIB_PATH), "aadff_spot_moments")
    assert _abi.ABI_VERSION == 9


def test_spot_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_spot_moments
    p = C.c_void_p(16)
    assert f(None, 9, p, 16, 8, 1, p, 12, 1.0, 2.0, p, 0, 1, p, None, None) == -1 and b"NULL" in lib.aadff_last_error()
    assert f(p, 9, p, 12, 8, 1, p, 12, 1.0, 2.0, p, 0, 1, p, None, None) == -1 and b"multiple of num_angle" in lib.aadff_last_error()
    assert f(p, 9, p, 4096, 8, 1, p, 12, 1.0, 2.0, p, 0, 1, p, None, None) == -1 and b"at most 2048" in lib.aadff_last_error()
    assert f(p, 0, p, 16, 8, 1, p, 12, 1.0, 2.0, p, 0, 1, p, None, None) == -1 and b"bad sizes" in lib.aadff_last_error()
    assert f(p, 9, p, 16, 8, 17, p, 12, 1.0, 2.0, p, 0, 1, p, None, None) == -1 and b"bad sizes" in lib.aadff_last_error()
    assert f(p, 9, p, 16, 8, 1, p, 0, 1.0, 2.0, p, 0, 1, p, None, None) == -1 and b"n_surf" in lib.aadff_last_error()
    assert f(p, 9, p, 16, 8, 1, p, 12, 1.0, 2.0, p, 2, 1, p, None, None) == -1 and b"ref_mode" in lib.aadff_last_error()
    assert f(p, 9, p, 16, 8, 1, p, 12, float("nan"), 2.0, p, 0, 1, p, None, None) == -1 and b"pupil" in lib.aadff_last_error()


def _kernel_moments(p, ra, ref):
    """What aadff_spot_moments returns, restated: per pass and field (count, sum x, sum y, S2 about the centroid of pass 0
    (ref) or of the pass itself, centroid = sum / (count + 1e-4))"""
    n = ra.sum(1)
    sx, sy = (p[..., 0] * ra).sum(1), (p[..., 1] * ra).sum(1)
    c = torch.stack((sx, sy), -1) / (n + 1e-4).unsqueeze(-1)
    if ref:
        c = c[0:1].expand_as(c)
    s2 = (((p - c.unsqueeze(1)) ** 2).sum(-1) * ra).sum(1)
    return torch.stack((n, sx, sy, s2), -1)


@pytest.mark.parametrize("ref", [True, False])
def test_rms_combination_equals_the_reference_formulas(ref):
    """Lensgroup._rms_from_moments on per-field moments == the reference's analysis_rms reductions (optics.py:1994-2011)
    written out on the rays: the on-axis index wart ([H//2+1]^2 over the count at [H//2]^2), the +0.0001 centroid"""
    H, S = 31, 256
    g = torch.Generator().manual_seed(0)
    passes = 4 if ref else 3
    p = torch.randn((passes, S, H, H, 2), generator=g, dtype=torch.float64) * 0.02 + torch.linspace(-5, 5, H, dtype=torch.float64).view(1, 1, 1, H, 1)
    ra = (torch.rand((passes, S, H, H), generator=g, dtype=torch.float64) > 0.3).double()
    ra[1:, :, H // 2 + 1, H // 2 + 1] *= (torch.rand((passes - 1, S), generator=g, dtype=torch.float64) > 0.5).double()
    mom = _kernel_moments(p.reshape(passes, S, H * H, 2), ra.reshape(passes, S, H * H), ref)
    got = Lensgroup._rms_from_moments(mom, H, ref)
    # the reference's reductions
    rms, on, off = [], [], []
    if ref:
        p_ref = (p[0] * ra[0].unsqueeze(-1)).sum(0) / ra[0].sum(0).add(0.0001).unsqueeze(-1)
    for w in range(1 if ref else 0, passes):
        o2, r = p[w], ra[w]
        c = p_ref if ref else (o2 * r.unsqueeze(-1)).sum(0) / r.sum(0).add(0.0001).unsqueeze(-1)
        o2n = (o2 - c) * r.unsqueeze(-1)
        rms.append(torch.sqrt(torch.sum(o2n ** 2 * r.unsqueeze(-1)) / torch.sum(r)))
        on.append(torch.sqrt(torch.sum(o2n[:, H // 2 + 1, H // 2 + 1, :] ** 2 * r[:, H // 2 + 1, H // 2 + 1].unsqueeze(-1)) / torch.sum(r[:, H // 2, H // 2])))
        off.append(torch.sqrt(torch.sum(o2n[:, 0, 0, :] ** 2 * r[:, 0, 0].unsqueeze(-1)) / torch.sum(r[:, 0, 0])))
    want = (sum(rms) / len(rms), sum(on) / len(on), sum(off) / len(off))
    for a, b in zip(got, want):
        assert a.dim() == 0 and a.dtype == torch.float32
        assert abs(float(a) - float(b)) <= 2e-6 * float(b)
    # the wart matters: the on-axis term differs from a same-field ratio
    same = np.sqrt(float(mom[1 if ref else 0, (H // 2 + 1) * H + H // 2 + 1, 3] / mom[1 if ref else 0, (H // 2 + 1) * H + H // 2 + 1, 0]))
    assert abs(float(on[0]) - same) > 1e-4 * same


def test_magnification_formula(host_lens):
    """calc_magnification3's host part (optics.py:1240-1256): NaN-free mean of the top-left 10 x 10 quadrant, pinhole scale
    when the mean is infinite"""
    host_lens.hfov = 0.41
    M = 21
    o = host_lens._point_grid(-DEPTH * np.tan(host_lens.hfov) * 0.5, DEPTH, M)
    x1 = torch.flip(o[..., :2], [0, 1])[..., 0]
    g = torch.Generator().manual_seed(1)
    x2 = x1 * (0.0025 * (1 + 1e-3 * torch.randn((M, M), generator=g)))
    x2[3, 4] = float("nan")
    n = torch.full((M, M), 512.0)
    x2s = x2 * n
    got = host_lens._mag_from_x(x1, x2s / n.add(EPSILON), DEPTH)
    tmp = (x1 / x2)[:10, :10]
    assert got == pytest.approx(1 / torch.mean(tmp[~tmp.isnan()]).item(), rel=1e-6)
    assert abs(got - 0.0025) < 1e-5
    zero = torch.zeros((M, M))
    assert host_lens._mag_from_x(x1, zero, DEPTH) == pytest.approx(1 / (-DEPTH * np.tan(0.41) / host_lens.r_last))
