"""CPU: the layered ray-traced rendering rule as restated in tests/raytrace_layered_common.py - that it reduces
to the plane rule of 4.15, its ordering, the conditions the GPU tests rely on - and the host side of the ABI entry and of the Python
entry points.  No GPU."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import raytrace_common as rc
import raytrace_layered_common as rl
from aadff import _abi, raytrace
from deeplens.optics import Lensgroup

Z0, Z1, Z2 = rl.LAYER_DEPTHS


def uniform_map(index):
    return np.full((rc.B, rc.H, rc.W), index, dtype=np.uint8)


@pytest.mark.parametrize("name", rc.LENSES)
def test_one_layer_is_the_plane_rule(name):
    """L = 1 with layer == 0: a = 1 and T -> 0 exactly, V = q: the image and the count of raytrace_common.render_rule, bit for bit"""
    for depth in rc.DEPTHS:
        d_sensor, pupil, scale = rc.oracle_inputs(name, depth)
        plane = rc.render_oracle(name, depth, d_sensor, pupil, scale, torch.float64)
        got = rl.layered_oracle(name, (depth,), (scale,), d_sensor, pupil, torch.float64, layer=uniform_map(0))
        assert torch.equal(got["img"], plane["img"])
        for b in range(rc.B):
            assert torch.equal(got["coverage"][b], plane["count"])
        assert torch.equal(got["alive"] & rc.window_valid(got["alive"], got["uj"][0], got["vi"][0], (rc.H, rc.W)), plane["valid"])


def test_ordering_through_empty_and_opaque_planes():
    """Three planes: a map that is all 0 stops every ray at z_0 (T = 0 behind it), a map that is all 2 lets it through two empty
    planes with T exactly 1 - either way the L = 1 result at that plane, bit for bit.  An all-hole map renders nothing."""
    name = "rf50mm"
    d_sensor, pupil, scales = rl.oracle_inputs(name)
    for index in (0, 2):
        got = rl.layered_oracle(name, rl.LAYER_DEPTHS, scales, d_sensor, pupil, torch.float64, layer=uniform_map(index))
        one = rl.layered_oracle(name, (rl.LAYER_DEPTHS[index],), (scales[index],), d_sensor, pupil, torch.float64, layer=uniform_map(0))
        assert torch.equal(got["img"], one["img"]) and torch.equal(got["coverage"], one["coverage"])
    got = rl.layered_oracle(name, rl.LAYER_DEPTHS, scales, d_sensor, pupil, torch.float64, layer=uniform_map(rl.HOLE))
    assert bool((got["img"] == 0).all()) and bool((got["coverage"] == 0).all())


def test_constant_image_and_coverage():
    """0.5 comes back exactly wherever coverage > 0 (q = 0.5 a and V = 0.5 A term by term: a scaling by a power of two), 0 elsewhere;
    the coverage of a pixel never exceeds the number of its rays that survived the lens; the hole lets rays through"""
    name = "50mm_f2.8"
    d_sensor, pupil, scales = rl.oracle_inputs(name)
    got = rl.layered_oracle(name, rl.LAYER_DEPTHS, scales, d_sensor, pupil, torch.float64, img=np.full((rc.B, 3, rc.H, rc.W), 0.5))
    lit = got["coverage"] > 0
    assert bool(lit.any()) and bool((got["img"][lit] == 0.5).all()) and bool((got["img"][~lit] == 0).all())
    count = got["alive"].sum(1).double()
    assert bool((got["coverage"] <= count.unsqueeze(0)).all())
    assert float((count.unsqueeze(0) - got["coverage"]).max()) > 0.5


@pytest.mark.parametrize("name", rc.LENSES)
def test_caps_the_gpu_tests_rely_on(name):
    """With the fixed inputs, the float64 restatement alone: few non-robust rays (union over the three planes), nearly every pixel
    with all rays robust; on robust rays float32 decides survival alike"""
    d_sensor, pupil, scales = rl.oracle_inputs(name)
    case = rl.reference_case(name, d_sensor, pupil, scales)
    print(f"layered {name}: rays not robust {float((~case['robust']).double().mean()):.2e}, robust pixels {float(case['pix'].double().mean()):.4f}")
    assert float((~case["robust"]).double().mean()) <= 1e-3
    assert float(case["pix"].double().mean()) >= 0.99
    assert tuple(case["robust"].shape) == (3, rc.SPP, rc.H, rc.W) and tuple(case["ref"]["img"].shape) == (rc.B, 3, rc.H, rc.W)
    assert torch.equal(case["f32"]["alive"][case["robust"]], case["ref"]["alive"][case["robust"]])
    for key in ("img", "coverage"):
        F = rl.floor_distance(case, key)
        assert bool(torch.isfinite(F).all()) and float(F.min()) > 0


def test_symbol_declared_exported_bound(repo_root):
    header = open(os.path.join(repo_root, "include", "aadff.h")).read()
    name = "aadff_render_raytraced_layered"
    assert re.search(rf"^int {name}\(", header, flags=re.M)
    assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name]) == 26
    assert hasattr(C.CDLL(_abi.LIB_PATH), name)
    assert re.search(r"^#define AADFF_RENDER_MAX_LAYERS 32$", header, flags=re.M) and raytrace.MAX_LAYERS == 32
    assert _abi.ABI_VERSION == 9 and _abi.load_library().aadff_abi_version() == 9


def test_argument_errors_need_no_gpu():
    """Each argument error returns -1 with its message before any HIP call"""
    lib = _abi.load_library()
    p = C.c_void_p(16)

    def call(img=p, layer=p, spp=16, surf=p, ps=1.0, depths=(Z0, Z1, Z2), scales=(10.0, 20.0, 40.0), L=None, state=p, out=p):
        zs = (C.c_float * max(len(depths), 1))(*depths) if depths is not None else None
        sc = (C.c_float * max(len(scales), 1))(*scales) if scales is not None else None
        r = lib.aadff_render_raytraced_layered(img, layer, 2, 24, 32, None, 7, spp, surf, 12, 20.0, 8.0, 32.0, 24.0, ps,
                                               len(depths) if L is None else L, zs, sc, 0, state, out, None, None, None, None, None)
        return r, lib.aadff_last_error()

    for kw in (dict(img=None), dict(layer=None), dict(surf=None), dict(state=None), dict(out=None), dict(depths=None, L=3), dict(scales=None)):
        r, msg = call(**kw)
        assert r == -1 and b"NULL pointer" in msg, kw
    many = tuple(-100.0 * (k + 1) for k in range(33))
    for kw, text in ((dict(L=0), b"outside [1,32]"), (dict(depths=many, scales=(1.0,) * 33), b"outside [1,32]"), (dict(L=-1), b"outside [1,32]"),
                     (dict(depths=(Z0, Z2, Z1)), b"strictly decreasing"), (dict(depths=(Z0, Z0, Z2)), b"strictly decreasing"),
                     (dict(depths=(Z2, Z1, Z0)), b"strictly decreasing"), (dict(depths=(500.0, Z1, Z2)), b"must be negative"),
                     (dict(depths=(0.0, Z1, Z2)), b"must be negative"), (dict(scales=(10.0, 0.0, 40.0)), b"scale * pixel_size must be positive"),
                     (dict(scales=(10.0, 20.0, -40.0)), b"scale * pixel_size must be positive"), (dict(ps=0.0), b"scale * pixel_size must be positive"),
                     (dict(spp=12), b"multiple of 8"), (dict(spp=0), b"multiple of 8")):
        r, msg = call(**kw)
        assert r == -1 and text in msg, (kw, msg)


@pytest.fixture(scope="module")
def host_lens(repo_root):
    return Lensgroup(rc.lens_file("rf50mm"), sensor_res=(rc.H, rc.W), post_computation=False, device="cpu")


def test_python_layer_refuses_before_it_needs_a_gpu(host_lens):
    img = torch.zeros((rc.B, 3, rc.H, rc.W))
    layer = torch.zeros((rc.B, rc.H, rc.W), dtype=torch.uint8)
    ok = dict(layer_depths=rl.LAYER_DEPTHS, scales=(10.0, 20.0, 40.0))
    for fn, args in ((raytrace.render_raytraced_layered, (host_lens, img, layer)), (host_lens.render_raytraced_layered, (img, layer))):
        with pytest.raises(ValueError, match=r"in \[1, 32\]"):
            fn(*args, layer_depths=(), scales=())
        with pytest.raises(ValueError, match=r"in \[1, 32\]"):
            fn(*args, layer_depths=[-100.0 * (k + 1) for k in range(33)], scales=[1.0] * 33)
        with pytest.raises(ValueError, match="strictly decreasing"):
            fn(*args, layer_depths=(Z0, Z2, Z1), scales=ok["scales"])
        with pytest.raises(ValueError, match="must be negative"):
            fn(*args, layer_depths=(500.0, Z1, Z2), scales=ok["scales"])
        with pytest.raises(ValueError, match="must be negative"):
            fn(*args, layer_depths=(0.0, Z1, Z2), scales=ok["scales"])
        with pytest.raises(ValueError, match="multiple of 8"):
            fn(*args, spp=12, **ok)
        with pytest.raises(ValueError, match="u or seed, not both"):
            fn(*args, spp=rc.SPP, u=torch.zeros((3, rc.SPP, 2, rc.H, rc.W)), seed=1, **ok)
        with pytest.raises(ValueError, match="must be positive"):
            fn(*args, layer_depths=rl.LAYER_DEPTHS, scales=(10.0, -20.0, 40.0))
        with pytest.raises(ValueError, match="3 layers"):
            fn(*args, layer_depths=rl.LAYER_DEPTHS, scales=(10.0, 20.0))
    lay = raytrace.render_raytraced_layered
    with pytest.raises(ValueError, match=r"layer must be \[2,24,32\]"):
        lay(host_lens, img, layer[0], **ok)
    with pytest.raises(ValueError, match=r"layer must be \[2,24,32\]"):
        lay(host_lens, img, layer[:, None], **ok)
    with pytest.raises(ValueError, match="uint8 or int64"):
        lay(host_lens, img, layer.float(), **ok)
    with pytest.raises(ValueError, match="uint8 or int64"):
        lay(host_lens, img, layer.int(), **ok)
    with pytest.raises(ValueError, match=r"\[B,3,H,W\]"):
        lay(host_lens, img[0], layer, **ok)
    with pytest.raises(ValueError, match="return_aux"):
        lay(host_lens, img, layer, return_aux="all", **ok)
    with pytest.raises(RuntimeError, match="no autograd"):
        lay(host_lens, img.clone().requires_grad_(), layer, **ok)
    with pytest.raises(ValueError, match="empty"):
        raytrace.render_raytraced_layered_stack(host_lens, img, layer, rl.LAYER_DEPTHS, [], scales=ok["scales"])
    with pytest.raises(ValueError, match="strictly decreasing"):
        raytrace.render_raytraced_layered_stack(host_lens, img, layer, (Z0, Z2, Z1), [-1500.0], scales=ok["scales"])
    with pytest.raises(ValueError, match=r"layers=33"):
        raytrace.render_raytraced_rgbd(host_lens, img, torch.full((rc.B, 1, rc.H, rc.W), -1000.0), layers=33)
    with pytest.raises(ValueError, match="depth_mm must be"):
        raytrace.render_raytraced_rgbd(host_lens, img, torch.full((rc.B, 1, 8, 8), -1000.0))
    with pytest.raises(ValueError, match="multiple of 8"):
        host_lens.render_raytraced_rgbd(img, torch.full((rc.B, 1, rc.H, rc.W), -1000.0), spp=12)
    for parity in ("strict", "edge"):
        lens = Lensgroup(rc.lens_file("rf50mm"), sensor_res=(rc.H, rc.W), post_computation=False, device="cpu", parity=parity)
        with pytest.raises(NotImplementedError, match="parity"):
            lay(lens, img, layer, **ok)
        with pytest.raises(NotImplementedError, match="parity"):
            raytrace.render_raytraced_layered_stack(lens, img, layer, rl.LAYER_DEPTHS, [-1500.0], scales=ok["scales"])
        with pytest.raises(NotImplementedError, match="parity"):
            raytrace.render_raytraced_rgbd(lens, img, torch.full((rc.B, 1, rc.H, rc.W), -1000.0))
