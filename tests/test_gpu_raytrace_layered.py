"""GPU: the layered ray-traced render (aadff_render_raytraced_layered behind aadff.raytrace / Lensgroup.render_raytraced_layered,
DESIGN.md 4.16) against the float64 restatement of its rule on the CPU oracle (tests/raytrace_layered_common.py): survival ray by
ray, image and coverage element by element against a float32 floor computed in the run; and bit for bit against the plane render of
4.15 where the rule reduces to it, across chunks of a batch, through a focal stack and from the in-kernel generator."""
import functools

import numpy as np
import pytest
import torch

import raytrace_common as rc
import raytrace_layered_common as rl
from aadff import raytrace
from deeplens.optics import Lensgroup

pytestmark = pytest.mark.gpu

DEV = "cuda:0"


def make_lens(name, res=(rc.H, rc.W)):
    """The sensor given by its size - the width the lens would derive, the height as width x H / W - so that prepare_sensor's exact
    float test for square pixels holds at 24 x 32 for both lenses (as in tests/test_gpu_raytrace.py)."""
    h, w = res
    lens = Lensgroup(rc.lens_file(name), device=DEV, post_computation=False)
    ws = 2 * lens.r_last * w / np.sqrt(h ** 2 + w ** 2)
    lens.prepare_sensor(res, sensor_size=[ws * h / w, ws])
    lens.post_computation()
    return lens


@functools.lru_cache(maxsize=None)
def shared_lens(name):
    """never refocused: the test that moves the sensor makes its own"""
    return make_lens(name)


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    u, img = rc.fixed_inputs()
    return torch.as_tensor(u).to(DEV), torch.as_tensor(img).to(DEV), torch.as_tensor(rl.fixed_layers()).to(DEV)


def scales_of(lens, depths=rl.LAYER_DEPTHS):
    return tuple(float(lens.calc_scale_pinhole(z)) for z in depths)             # host arithmetic: no synchronisation


@functools.lru_cache(maxsize=None)
def kernel_case(name):
    """(reference case fed the GPU lens's own d_sensor, exit pupil, geometry and the test's scales, kernel output, kernel aux)"""
    lens = shared_lens(name)
    scales = scales_of(lens)
    pz, pr = lens.exit_pupil()
    geom = (float(lens.sensor_size[1]), float(lens.sensor_size[0]), float(lens.pixel_size))
    case = rl.reference_case(name, float(lens.d_sensor), (float(pz), float(pr)), scales, geom)
    u, img, layer = gpu_inputs()
    out, aux = lens.render_raytraced_layered(img, layer, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u, return_aux="valid")
    lens.check_flags()
    return case, out.cpu(), {k: v.cpu() for k, v in aux.items()}


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("name", rc.LENSES)
def test_survival_ray_by_ray(name):
    """On every robust ray the kernel's ray survives exactly when the float64 one does; robust rays are nearly all rays (conditions
    of the test, not measurements)"""
    case, _, aux = kernel_case(name)
    assert aux["alive_rays"].shape == case["robust"].shape and aux["alive_rays"].dtype == torch.bool
    assert float((~case["robust"]).double().mean()) <= 1e-3
    assert float(case["pix"].double().mean()) >= 0.99
    differ = (aux["alive_rays"] != case["ref"]["alive"]) & case["robust"]
    assert int(differ.sum()) == 0
    assert torch.equal(aux["alive"], aux["alive_rays"].sum(1).float())
    shared_lens(name).check_flags()


@pytest.mark.parametrize("name", rc.LENSES)
def test_image_and_coverage_elementwise_against_float64(name, margin):
    """On the pixels whose rays are all robust, both images (the banded map and the per-texel random one): |kernel - float64| <= 4 F
    for the image and for the coverage, F = the float32 restatement's own distance from float64 on the same pixels, measured in this
    run.  The factor 4 is 4.15's: the kernel's one-ulp rcp / rsq / sin / cos hardware forms and its FMA contraction against the
    oracle's IEEE operations.  Measured on one MI355X (kernel / F): see DESIGN.md 4.16."""
    case, out, aux = kernel_case(name)
    pix = case["pix"].unsqueeze(0)
    for key, got in (("img", out), ("coverage", aux["coverage"])):
        F = rl.floor_distance(case, key)
        assert bool(torch.isfinite(F).all()) and float(F.min()) > 0
        d = ((got.double() - case["ref"][key]).abs() * pix).amax(dim=(1, 2, 3))
        for b in range(rc.B):
            print(f"layered {name} {key} {b}: kernel {float(d[b]):.3e}, float32 floor {float(F[b]):.3e}, ratio {float(d[b] / F[b]):.2f}")
            margin(f"layered {name} {key} {b}: |kernel - f64| / (4 x f32 floor {float(F[b]):.1e})", float(d[b] / (4 * F[b])), 1.0)
    shared_lens(name).check_flags()


@pytest.mark.parametrize("name", rc.LENSES)
def test_one_layer_is_the_plane_render_bit_for_bit(name):
    lens = shared_lens(name)
    u, img, _ = gpu_inputs()
    zeros = torch.zeros((rc.B, rc.H, rc.W), dtype=torch.uint8, device=DEV)
    for depth in rc.DEPTHS:
        scale = float(lens.calc_scale_pinhole(depth))
        want, waux = lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, u=u, return_aux=True)
        got, aux = lens.render_raytraced_layered(img, zeros, (depth,), scales=(scale,), spp=rc.SPP, u=u, return_aux=True)
        assert torch.equal(got, want)
        for b in range(rc.B):
            assert torch.equal(aux["coverage"][b], waux["count"])
        assert bool((aux["alive"] >= waux["count"]).all())
        assert torch.equal(lens.render_raytraced_layered(img, zeros.long(), (depth,), scales=(scale,), spp=rc.SPP, u=u), want)       # int64 map
    lens.check_flags()


def test_ordering_through_empty_and_opaque_planes():
    """Under the three-plane table an all-0 map is the L = 1 render at z_0 (T = 0 behind it) and an all-2 map the L = 1 render at
    z_2 (T exactly 1 through two empty planes), bit for bit; an all-hole map renders nothing"""
    lens = shared_lens("rf50mm")
    u, img, _ = gpu_inputs()
    scales = scales_of(lens)
    for index in (0, 2):
        full = torch.full((rc.B, rc.H, rc.W), index, dtype=torch.uint8, device=DEV)
        got, aux = lens.render_raytraced_layered(img, full, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u, return_aux=True)
        one, oaux = lens.render_raytraced_layered(img, torch.zeros_like(full), (rl.LAYER_DEPTHS[index],), scales=(scales[index],), spp=rc.SPP,
                                                  u=u, return_aux=True)
        assert torch.equal(got, one) and torch.equal(aux["coverage"], oaux["coverage"]) and torch.equal(aux["alive"], oaux["alive"])
        assert torch.equal(got, lens.render_raytraced(img, depth=rl.LAYER_DEPTHS[index], spp=rc.SPP, scale=scales[index], u=u))
    holes = torch.full((rc.B, rc.H, rc.W), rl.HOLE, dtype=torch.uint8, device=DEV)
    got, aux = lens.render_raytraced_layered(img, holes, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u, return_aux=True)
    assert bool((got == 0).all()) and bool((aux["coverage"] == 0).all()) and float(aux["alive"].max()) > 0
    lens.check_flags()


def test_batch_chunks_and_vignetting():
    """B = 5 with five different layer maps (a launch of 4 images and one of 1 over the same rays) equals five B = 1 renders bit for
    bit; vignetting=True is sum V / spp where the default is sum V / sum A: equal to out * coverage / spp within 2 ulp"""
    lens = shared_lens("50mm_f2.8")
    u, img, layer = gpu_inputs()
    scales = scales_of(lens)
    g = torch.Generator().manual_seed(2)
    five = torch.cat((img, torch.rand((3, 3, rc.H, rc.W), generator=g).to(DEV)))
    maps = torch.cat((layer, torch.randint(0, 4, (3, rc.H, rc.W), generator=g).to(torch.uint8).to(DEV)))            # index 3: holes
    out, aux = lens.render_raytraced_layered(five, maps, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u, return_aux=True)
    assert tuple(out.shape) == (5, 3, rc.H, rc.W) and tuple(aux["coverage"].shape) == (5, 3, rc.H, rc.W) and "alive_rays" not in aux
    for b in range(5):
        o1, a1 = lens.render_raytraced_layered(five[b:b + 1], maps[b:b + 1], rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u, return_aux=True)
        assert torch.equal(out[b:b + 1], o1) and torch.equal(aux["coverage"][b:b + 1], a1["coverage"]) and torch.equal(aux["alive"], a1["alive"]), b
    assert not torch.equal(out[0], out[1]) and not torch.equal(aux["coverage"][3], aux["coverage"][4])
    vig, vaux = lens.render_raytraced_layered(five, maps, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u, vignetting=True, return_aux=True)
    assert torch.equal(vaux["coverage"], aux["coverage"]) and float(aux["coverage"].min()) < rc.SPP
    want = out.double().cpu() * aux["coverage"].double().cpu() / rc.SPP
    err = (vig.double().cpu() - want).abs().numpy()
    assert bool((err <= 2 * ulp32(want.numpy())).all())
    lens.check_flags()


def test_large_grid_constant_image():
    """1024 x 1024 (4096 workgroups per channel, pixel indices beyond 2^20), spp 8, four planes in bands of 256 rows with a band
    edge every ray near it straddles: q = 0.5 a and V = 0.5 A term by term (a scaling by a power of two), so the constant 0.5 comes
    back within 2 ulp wherever anything is covered, and 0 elsewhere"""
    lens = make_lens("rf50mm", res=(1024, 1024))
    depths = (-500.0, -1000.0, -2000.0, -4000.0)
    img = torch.full((1, 3, 1024, 1024), 0.5, device=DEV)
    layer = (torch.arange(1024, device=DEV) // 256).to(torch.uint8).reshape(1, 1024, 1).expand(1, 1024, 1024).contiguous()
    out, aux = lens.render_raytraced_layered(img, layer, depths, scales=scales_of(lens, depths), spp=8, seed=11, return_aux=True)
    lit = aux["coverage"] > 0
    assert float(lit.float().mean()) > 0.9
    assert float((out[lit] - 0.5).abs().max()) <= 2 * float(ulp32(0.5))
    assert bool((out[~lit] == 0).all())
    assert float(aux["coverage"].max()) <= 8 and float(aux["alive"].max()) <= 8
    frac = aux["coverage"] - aux["coverage"].floor()
    assert float((frac > 0).float().mean()) > 0.001                  # the band edges are in the picture: partial coverage
    lens.check_flags()


def test_stack():
    """render_raytraced_layered_stack = refocus + render per slice, bit for bit, and puts the lens state back"""
    lens = make_lens("rf50mm")
    u, img, layer = gpu_inputs()
    scales = scales_of(lens)
    fds = [-500.0, -2000.0]
    before = (lens.d_sensor, lens.hfov, lens.foclen, lens.fnum)
    torch.manual_seed(4)
    stack = lens.render_raytraced_layered_stack(img, layer, rl.LAYER_DEPTHS, fds, scales=scales, spp=rc.SPP, u=u)
    assert tuple(stack.shape) == (rc.B, 3, 2, rc.H, rc.W)
    assert (lens.d_sensor, lens.hfov, lens.foclen, lens.fnum) == before
    torch.manual_seed(4)
    singles = []
    for fd in fds:
        lens.refocus(fd)
        singles.append(lens.render_raytraced_layered(img, layer, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u))
    assert torch.equal(stack, torch.stack(singles, dim=2))
    assert not torch.equal(stack[:, :, 0], stack[:, :, 1])
    lens.check_flags()


def test_generator_and_rgbd():
    """seed = s is u = sensor_uniforms(s) bit for bit; render_raytraced_rgbd is depth_layers per image plus the layered render"""
    from aadff.focal_stack import depth_layers
    lens = shared_lens("rf50mm")
    _, img, layer = gpu_inputs()
    scales = scales_of(lens)
    seed = 0x1234_5678_9ABC_DEF1
    u = raytrace.sensor_uniforms(seed, rc.SPP, rc.H, rc.W, device=DEV)
    by_seed = lens.render_raytraced_layered(img, layer, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, seed=seed)
    assert torch.equal(by_seed, lens.render_raytraced_layered(img, layer, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, u=u))
    assert not torch.equal(by_seed, lens.render_raytraced_layered(img, layer, rl.LAYER_DEPTHS, scales=scales, spp=rc.SPP, seed=seed + 1))
    # a slanted depth map per image, quantised into 3 planes by depth_layers
    ramp = torch.linspace(-600.0, -1800.0, rc.W, device=DEV).reshape(1, 1, 1, rc.W).expand(rc.B, 1, rc.H, rc.W).clone()
    ramp[1] *= 1.5
    got, zs, aux = lens.render_raytraced_rgbd(img, ramp, layers=3, scales=scales, spp=rc.SPP, seed=seed, return_aux=True)
    assert tuple(got.shape) == (rc.B, 3, rc.H, rc.W) and tuple(zs.shape) == (rc.B, 3) and tuple(aux["coverage"].shape) == (rc.B, 3, rc.H, rc.W)
    for b in range(rc.B):
        idx, centres = depth_layers(ramp[b, 0], 3)
        assert torch.equal(zs[b], centres.float().cpu()) and bool((zs[b][1:] < zs[b][:-1]).all())
        assert torch.equal(got[b:b + 1], lens.render_raytraced_layered(img[b:b + 1], idx[None], centres.cpu(), scales=scales, spp=rc.SPP, seed=seed))
    lens.check_flags()
