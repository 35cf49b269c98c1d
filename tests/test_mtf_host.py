"""CPU: the host side of the ray-traced MTF: the rule's restatement (tests/mtf_common.py) and the package's own torch
form of it on synthetic hits with closed forms, psf2mtf against a direct DFT, the three-point peak, and the aadff_mtf_points ABI entry
(declared, bound, exported; its argument refusals return before any device is touched).  No GPU."""
import ctypes as C
import inspect
import json
import os
import re
import types

import numpy as np
import pytest
import torch

import mtf_common as mc
from aadff import _abi, mtf
from deeplens.optics import Lensgroup

RULES = [("restatement", lambda *a: mc.otf_rule(*a)["otf"]), ("package", lambda *a: mtf.otf_of_hits(*a)[0])]


def _one_field(x, a=None, y=None, b=None, valid=None):
    """[n] hit coordinates of one field -> the rule's arguments for axes xy"""
    x = torch.as_tensor(x, dtype=torch.float64).reshape(-1, 1)
    zero = torch.zeros_like(x)
    cols = [x, zero if y is None else torch.as_tensor(y, dtype=torch.float64).reshape(-1, 1),
            zero if a is None else torch.as_tensor(a, dtype=torch.float64).reshape(-1, 1),
            zero if b is None else torch.as_tensor(b, dtype=torch.float64).reshape(-1, 1)]
    valid = torch.ones_like(x, dtype=torch.bool) if valid is None else torch.as_tensor(valid).reshape(-1, 1)
    e_t, e_s = mc.axes_of(torch.tensor([[1.0, 0.0, -1.0]], dtype=torch.float64), "xy")
    return (*cols, valid, e_t, e_s)


def _comb(nu, w, n):
    """|sum of n unit phasors spaced w / n apart| / n"""
    return np.abs(np.sin(np.pi * nu * w) / (n * np.sin(np.pi * nu * w / n)))


@pytest.mark.parametrize("which,rule", RULES)
def test_equally_spaced_hits(which, rule):
    """n hits spaced w / n apart, anywhere on the sensor: |sin(pi nu w) / (n sin(pi nu w / n))| along x, 1 along y"""
    n, w = 12, 0.03
    freqs = [0.0, 3.0, 17.0, 41.5, 100.0]
    x = 11.7 + np.arange(n) * (w / n)
    otf = rule(*_one_field(x), freqs, [0.0])
    assert tuple(otf.shape) == (1, 1, 2, len(freqs))
    want = np.array([1.0 if f == 0 else _comb(f, w, n) for f in freqs])
    assert np.abs(otf[0, 0, 0].abs().numpy() - want).max() <= 1e-12
    assert np.abs(otf[0, 0, 0].imag.numpy()).max() <= 1e-12               # symmetric about its mean: real
    assert np.abs(otf[0, 0, 1].abs().numpy() - 1.0).max() <= 1e-12


@pytest.mark.parametrize("which,rule", RULES)
def test_two_points_and_dead_rays(which, rule):
    """two hits d apart: |cos(pi nu d)|; a dead ray between them, with any coordinates, changes nothing; no valid ray: zeros"""
    d = 0.02
    freqs = [0.0, 10.0, 25.0, 60.0]
    want = np.abs(np.cos(np.pi * np.array(freqs) * d))
    otf = rule(*_one_field([-3.0, 55.0, -3.0 + d], valid=[True, False, True]), freqs, [0.0])
    assert np.abs(otf[0, 0, 0].abs().numpy() - want).max() <= 1e-12
    assert float(otf[0, 0, 0, 2].abs()) <= 1e-12                            # nu d = 1/2: the first zero
    none = rule(*_one_field([1.0, 2.0], valid=[False, False]), freqs, [0.0])
    assert bool((none == 0).all())


@pytest.mark.parametrize("which,rule", RULES)
def test_slope_spread_grows_linearly_with_defocus(which, rule):
    """all rays through one point of the sensor with equally spaced slopes: on the plane delta the spot is the comb of width
    n da |delta| - the MTF is 1 in focus, even in delta, and depends on nu and delta through their product alone"""
    n, da, nu = 16, 0.01, 30.0
    a = (np.arange(n) - 3.3) * da
    defocus = [-0.2, -0.1, 0.0, 0.1, 0.2]
    otf = rule(*_one_field(np.full(n, 2.5), a=a), [nu, 2 * nu], defocus)
    got = otf[0, :, 0, :].abs().numpy()
    want = np.array([[1.0 if dl == 0 else _comb(f, n * da * abs(dl), n) for f in (nu, 2 * nu)] for dl in defocus])
    assert np.abs(got - want).max() <= 1e-12
    assert abs(got[3, 1] - got[4, 0]) <= 1e-12                              # (2 nu, delta) == (nu, 2 delta)
    # and the RMS width of the spot is linear in |delta|: the second moment the OTF's curvature at nu -> 0 measures
    small = rule(*_one_field(np.full(n, 2.5), a=a), [1e-3], defocus)[0, :, 0, 0].abs().numpy()
    width = np.sqrt(np.maximum(2 * (1 - small), 0)) / (2 * np.pi * 1e-3)
    assert np.abs(width - np.std(a) * np.abs(defocus)).max() <= 1e-6


def test_radial_axes_follow_the_object_point():
    pts = torch.tensor([[0.0, 0.0, -1.0], [3.0, 4.0, -1.0], [0.0, -2.0, -1.0], [-5.0, 0.0, -1.0]], dtype=torch.float64)
    for fn in (mc.axes_of, mtf.axes_of):
        e_t, e_s = fn(pts, "radial")
        assert torch.equal(e_t[0], torch.tensor([1.0, 0.0], dtype=torch.float64)) and torch.equal(e_s[0], torch.tensor([0.0, 1.0], dtype=torch.float64))
        assert torch.allclose(e_t[1], torch.tensor([0.6, 0.8], dtype=torch.float64)) and torch.allclose(e_s[1], torch.tensor([-0.8, 0.6], dtype=torch.float64))
        assert torch.equal(e_t[2], torch.tensor([0.0, -1.0], dtype=torch.float64)) and torch.equal(e_t[3], torch.tensor([-1.0, 0.0], dtype=torch.float64))
        e_t, e_s = fn(pts, "xy")
        assert bool((e_t == torch.tensor([1.0, 0.0], dtype=torch.float64)).all()) and bool((e_s == torch.tensor([0.0, 1.0], dtype=torch.float64)).all())


def test_parabola_peak():
    delta = torch.linspace(-0.2, 0.2, 9, dtype=torch.float64)
    assert mtf.parabola_peak(delta, 1 - (delta - 0.013) ** 2) == pytest.approx(0.013, abs=1e-12)
    assert mtf.parabola_peak(delta, delta) == 0.2 and mtf.parabola_peak(delta, -delta) == -0.2


def test_psf2mtf_against_a_direct_dft(repo_root):
    """the reference's psf2mtf (optics.py:1028-1065) restated without an FFT: the centre column ('tangential') and row ('sagittal'),
    |DFT| over its maximum, on the positive frequencies k / (N pixel_size)"""
    rng = np.random.default_rng(0)
    psf = rng.random((31, 31))
    psf /= psf.sum()
    ps = 0.0043
    N = 31
    k = np.arange(N)
    dft = np.exp(-2j * np.pi * np.outer(k, k) / N)
    tan, sag = np.abs(dft @ psf[:, N // 2]), np.abs(dft @ psf[N // 2, :])
    pos = np.arange(1, (N - 1) // 2 + 1)
    want = (pos / (N * ps), (tan / tan.max())[pos], (sag / sag.max())[pos])
    lens = Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(480, 640), post_computation=False, device="cpu")
    lens.pixel_size = ps
    for got in (mtf.psf2mtf(types.SimpleNamespace(pixel_size=ps), torch.from_numpy(psf)), lens.psf2mtf(torch.from_numpy(psf))):
        assert len(got) == 3
        for g, w in zip(got, want):
            assert g.shape == (15,) and np.abs(g - w).max() <= 1e-12


def test_draw_mtf_axis():
    ax = mtf.draw_mtf_axis(types.SimpleNamespace(pixel_size=0.005))
    assert ax.shape == (127,) and ax[0] == pytest.approx(1 / (256 * 0.005)) and ax[-1] < 0.5 / 0.005 and len(ax) <= mtf.MAX_F


def test_reference_signatures(golden_dir):
    ref = json.load(open(os.path.join(golden_dir, "g16_signatures.json")))["deeplens.optics"]
    for name in ("psf2mtf", "draw_mtf", "draw_distortion"):
        got = list(inspect.signature(getattr(Lensgroup, name)).parameters)
        assert got == [w[0] for w in ref[f"Lensgroup.{name}"]], name
    assert list(inspect.signature(Lensgroup.mtf).parameters) == ["self", "points", "freqs", "wvlns", "defocus", "spp", "axes"]


def test_mtf_symbol_declared_exported_bound(repo_root):
    header = open(os.path.join(repo_root, "include", "aadff.h")).read()
    m = re.search(r"^int aadff_mtf_points\(([^;]*)\);", header, flags=re.M)
    assert m and len(m.group(1).split(",")) == 20
    assert "optics.py:1028-1065" in header
    assert "aadff_mtf_points" in _abi.PROTOTYPES and len(_abi.PROTOTYPES["aadff_mtf_points"]) == 20
    assert hasattr(C.CDLL(_abi.LIB_PATH), "aadff_mtf_points")
    assert _abi.ABI_VERSION == 9 and _abi.load_library().aadff_abi_version() == 9


def test_mtf_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_mtf_points
    p = C.c_void_p(16)
    fr = (C.c_float * 129)(*[float(i) for i in range(129)])
    df = (C.c_float * 17)(*[0.01 * i for i in range(17)])
    frp, dfp = C.cast(fr, C.c_void_p), C.cast(df, C.c_void_p)

    def call(points=p, P=9, spp=64, num_angle=8, n_pass=3, n_surf=12, pz=1.0, pr=2.0, freqs=frp, F=5, defocus=dfp, Z=3, axes=0):
        rc = f(points, P, p, spp, num_angle, n_pass, p, n_surf, pz, pr, p, freqs, F, defocus, Z, axes, p, p, None, None)
        return rc, lib.aadff_last_error()

    for kw, reason in ((dict(points=None), b"NULL"), (dict(freqs=None), b"NULL"), (dict(spp=60), b"multiple of num_angle"),
                       (dict(spp=2056), b"at most 2048"), (dict(spp=0), b"positive multiple"), (dict(P=0), b"bad sizes"),
                       (dict(n_pass=17), b"bad sizes"), (dict(n_surf=0), b"n_surf"), (dict(F=0), b"F=0"), (dict(F=129), b"F=129"),
                       (dict(Z=0), b"Z=0"), (dict(Z=17), b"Z=17"), (dict(axes=2), b"axes_mode"), (dict(pz=float("nan")), b"pupil")):
        rc, msg = call(**kw)
        assert rc == -1 and reason in msg, (kw, msg)
    for i, bad in ((2, -1.0), (0, float("nan")), (4, float("inf"))):
        arr = (C.c_float * 5)(0.0, 5.0, 20.0, 80.0, 100.0)
        arr[i] = bad
        rc, msg = call(freqs=C.cast(arr, C.c_void_p))
        assert rc == -1 and b"frequency %d" % i in msg, msg
    arr = (C.c_float * 3)(-0.1, float("nan"), 0.1)
    rc, msg = call(defocus=C.cast(arr, C.c_void_p))
    assert rc == -1 and b"defocus 1" in msg, msg
