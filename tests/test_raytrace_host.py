"""CPU: the ray-traced rendering rule as restated in tests/raytrace_common.py - its coordinate convention, the
conditions the GPU tests rely on, the float32 floor of the path - and the host side of the two ABI entries.  No GPU."""
import ctypes as C
import inspect
import os
import re

import numpy as np
import pytest
import torch

import raytrace_common as rc
from aadff import _abi, raytrace
from deeplens.optics import Lensgroup

CASES = [(name, depth) for name in rc.LENSES for depth in rc.DEPTHS]


def host_case(name, depth):
    return rc.reference_case(name, depth, *rc.oracle_inputs(name, depth))


def test_ideal_lens_renders_the_identity():
    """The trace replaced by an ideal lens of magnification -1 / scale (p = -scale x sensor point): (vi, uj) = (i, j) and the
    rule returns the image itself, bit for bit in float64.  Pixel size, scale and the image are dyadic (0.5 mm, 64, k / 256) so
    that every step of the rule is exact: a sum of 16 equal 53-bit values is not, in general."""
    res, ps, scale = (rc.H, rc.W), 0.5, 64.0
    geom = (rc.W * ps, rc.H * ps, ps)
    rng = np.random.default_rng(5)
    with rc.default_dtype(torch.float64):
        img = torch.as_tensor(rng.integers(0, 256, (rc.B, 3, rc.H, rc.W)) / 256.0)
        u = torch.as_tensor(rc.fixed_inputs()[0]).double()
        ideal = lambda rays, c: (-scale * rays.o[..., 0], -scale * rays.o[..., 1], torch.ones(rays.o.shape[:-1], dtype=torch.bool))  # noqa: E731
        got = rc.render_rule(ideal, rc.WAVE_RGB, res, geom, 60.0, (20.0, 8.0), scale, u, img)
    ii, jj = torch.meshgrid(torch.arange(rc.H), torch.arange(rc.W), indexing="ij")
    assert torch.equal(got["vi"], ii.double().expand_as(got["vi"])) and torch.equal(got["uj"], jj.double().expand_as(got["uj"]))
    assert torch.equal(got["img"], img) and bool((got["count"] == rc.SPP).all())
    # vignetting with every ray valid changes nothing
    with rc.default_dtype(torch.float64):
        assert torch.equal(rc.render_rule(ideal, rc.WAVE_RGB, res, geom, 60.0, (20.0, 8.0), scale, u, img, vignetting=True)["img"], img)


def test_constant_image_returns_the_constant():
    """Through the real lens in float64: 0.5 (exact under every pair of bilinear weights) comes back exactly wherever a ray is
    valid, 0 elsewhere; a generic constant within a few ulp (weights (1-f) + f sum to 1 only up to rounding)."""
    name, depth = "rf50mm", -2000.0
    d_sensor, pupil, scale = rc.oracle_inputs(name, depth)
    for const, ulps in ((0.5, 0), (0.7, 12)):          # 0.7: 3 ulp from the two lerp levels, 7.5 from 15 additions, 0.5 from the division
        img = np.full((1, 3, rc.H, rc.W), const)
        got = rc.render_oracle(name, depth, d_sensor, pupil, scale, torch.float64, img=img)
        lit = got["count"] > 0
        assert bool(lit.any())
        assert float((got["img"][0][lit] - const).abs().max()) <= ulps * np.spacing(const)
        assert bool((got["img"][0][~lit] == 0).all())


@pytest.mark.parametrize("name,depth", CASES)
def test_caps_the_gpu_tests_rely_on(name, depth):
    """With the fixed inputs, the float64 restatement alone: few non-robust rays, nearly every pixel with all rays robust, at least
    one valid ray in every pixel"""
    case = host_case(name, depth)
    assert float((~case["robust"]).double().mean()) <= 1e-3
    assert float(case["pix"].double().mean()) >= 0.99
    assert float(case["ref"]["count"].min()) >= 1
    assert tuple(case["ref"]["img"].shape) == (rc.B, 3, rc.H, rc.W) and tuple(case["robust"].shape) == (3, rc.SPP, rc.H, rc.W)


@pytest.mark.parametrize("name,depth", CASES)
def test_float32_floor(name, depth, margin):
    """The float32 restatement against the float64 one on the pixels whose rays are all robust: finite and below 1e-4 (a sanity
    bound; the GPU test computes the floor it uses from the GPU lens's own numbers).  On robust rays float32 decides alike."""
    case = host_case(name, depth)
    F = rc.floor_distance(case)
    assert bool(torch.isfinite(F).all())
    margin(f"raytrace {name} {depth:g}: float32 oracle vs float64, image (robust pixels)", float(F.max()), 1e-4)
    assert torch.equal(case["f32"]["valid"][case["robust"]], case["ref"]["valid"][case["robust"]])


def test_symbols_declared_exported_bound(repo_root):
    header = open(os.path.join(repo_root, "include", "aadff.h")).read()
    lib = C.CDLL(_abi.LIB_PATH)
    for name, nargs in (("aadff_render_raytraced", 23), ("aadff_sensor_uniforms", 6)):
        assert re.search(rf"^int {name}\(", header, flags=re.M)
        assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name]) == nargs
        assert hasattr(lib, name)
    assert _abi.ABI_VERSION == 9 and _abi.load_library().aadff_abi_version() == 9


def test_argument_errors_need_no_gpu():
    """Each argument error returns -1 with its message before any HIP call"""
    lib = _abi.load_library()
    p = C.c_void_p(16)

    def call(img=p, B=2, H=24, W=32, spp=16, surf=p, n_surf=12, ps=1.0, depth=-2000.0, scale=40.0, state=p, out=p):
        rc_ = lib.aadff_render_raytraced(img, B, H, W, None, 7, spp, surf, n_surf, 20.0, 8.0, 32.0, 24.0, ps, depth, scale, 0, state, out,
                                         None, None, None, None)
        return rc_, lib.aadff_last_error()

    for kw in (dict(img=None), dict(surf=None), dict(state=None), dict(out=None)):
        r, msg = call(**kw)
        assert r == -1 and b"NULL pointer" in msg, kw
    for kw, text in ((dict(spp=12), b"multiple of 8"), (dict(spp=0), b"multiple of 8"), (dict(B=0), b"bad sizes"), (dict(H=0), b"bad sizes"),
                     (dict(W=0), b"bad sizes"), (dict(scale=0.0), b"scale * pixel_size must be positive"),
                     (dict(scale=-40.0), b"scale * pixel_size must be positive"), (dict(ps=0.0), b"scale * pixel_size must be positive"),
                     (dict(depth=0.0), b"must be negative"), (dict(depth=10.0), b"must be negative"), (dict(n_surf=0), b"n_surf"),
                     (dict(n_surf=33), b"n_surf")):
        r, msg = call(**kw)
        assert r == -1 and text in msg, (kw, msg)
    f = lib.aadff_sensor_uniforms
    assert f(7, 16, 24, 32, None, None) == -1 and b"NULL pointer" in lib.aadff_last_error()
    assert f(7, 12, 24, 32, p, None) == -1 and b"multiple of 8" in lib.aadff_last_error()
    assert f(7, 16, 0, 32, p, None) == -1 and b"bad sizes" in lib.aadff_last_error()


@pytest.fixture(scope="module")
def host_lens(repo_root):
    return Lensgroup(rc.lens_file("rf50mm"), sensor_res=(rc.H, rc.W), post_computation=False, device="cpu")


def test_python_layer_refuses_before_it_needs_a_gpu(host_lens):
    img = torch.zeros((1, 3, rc.H, rc.W))
    with pytest.raises(ValueError, match="multiple of 8"):
        raytrace.render_raytraced(host_lens, img, depth=-2000.0, spp=12, scale=40.0)
    with pytest.raises(ValueError, match="multiple of 8"):
        host_lens.render_raytraced(img, depth=-2000.0, spp=12, scale=40.0)
    with pytest.raises(ValueError, match="multiple of 8"):
        raytrace.sensor_uniforms(1, 12, rc.H, rc.W)
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        raytrace.render_raytraced(host_lens, img[0], depth=-2000.0, scale=40.0)
    with pytest.raises(ValueError, match="float32"):
        raytrace.render_raytraced(host_lens, img.double(), depth=-2000.0, scale=40.0)
    with pytest.raises(ValueError, match="sensor_res"):
        raytrace.render_raytraced(host_lens, torch.zeros((1, 3, 8, 8)), depth=-2000.0, scale=40.0)
    with pytest.raises(ValueError, match="must be negative"):
        raytrace.render_raytraced(host_lens, img, depth=2000.0, scale=40.0)
    with pytest.raises(ValueError, match="must be positive"):
        raytrace.render_raytraced(host_lens, img, depth=-2000.0, scale=-1.0)
    with pytest.raises(RuntimeError, match="no autograd"):
        raytrace.render_raytraced(host_lens, img.clone().requires_grad_(), depth=-2000.0, scale=40.0)
    for parity in ("strict", "edge"):
        lens = Lensgroup(rc.lens_file("rf50mm"), sensor_res=(rc.H, rc.W), post_computation=False, device="cpu", parity=parity)
        with pytest.raises(NotImplementedError, match="parity"):
            raytrace.render_raytraced(lens, img, depth=-2000.0, scale=40.0)
        with pytest.raises(NotImplementedError, match="parity"):
            raytrace.render_raytraced_stack(lens, img, -2000.0, [-1500.0], scale=40.0)
    with pytest.raises(ValueError, match="empty"):
        raytrace.render_raytraced_stack(host_lens, img, -2000.0, [], scale=40.0)


def test_sample_sensor_signature_and_refusals(host_lens):
    """The reference's signature (optics.py:494) and its two exceptions; render_single_img's refusal now names the way out"""
    sig = inspect.signature(Lensgroup.sample_sensor)
    assert [(p.name, p.default) for p in list(sig.parameters.values())[1:]] == [("spp", 64), ("pupil", True), ("wvln", 0.589), ("sub_pixel", False)]
    with pytest.raises(Exception, match="This feature has been abandoned."):
        host_lens.sample_sensor(pupil=False)
    with pytest.raises(Warning, match="This feature is not finished yet."):
        host_lens.sample_sensor(sub_pixel=True)
    with pytest.raises(NotImplementedError, match="render_raytraced"):
        host_lens.render_single_img(np.zeros((8, 8, 3), dtype=np.uint8))
