"""GPU: the ray-traced render (aadff_render_raytraced behind aadff.raytrace / Lensgroup.render_raytraced) against
the float64 restatement of its rule on the CPU oracle (tests/raytrace_common.py): validity ray by ray, the image element by element
against a float32 floor computed in the run, the composed route (sample_sensor -> trace -> propagate_to) on the same uniforms, the
in-kernel generator, and the edges of the domain."""
import functools

import numpy as np
import pytest
import torch

import raytrace_common as rc
from aadff import raytrace
from deeplens.basics import WAVE_RGB
from deeplens.optics import Lensgroup

pytestmark = pytest.mark.gpu

CASES = [(name, depth) for name in rc.LENSES for depth in rc.DEPTHS]
DEV = "cuda:0"


def make_lens(name, res=(rc.H, rc.W)):
    """Lensgroup.prepare_sensor keeps the reference's exact float test for square pixels (optics.py:153-175), which the sizes it
    derives itself, 2 r H / diag over 2 r W / diag, fail for some r_last (50mm_f2.8 at 24 x 32).  The sensor is therefore given by
    its size: the width the lens would derive, and the height as width x H / W, so the ratio is exact."""
    h, w = res
    lens = Lensgroup(rc.lens_file(name), device=DEV, post_computation=False)
    ws = 2 * lens.r_last * w / np.sqrt(h ** 2 + w ** 2)
    lens.prepare_sensor(res, sensor_size=[ws * h / w, ws])
    lens.post_computation()
    return lens


def geom_of(lens):
    return (float(lens.sensor_size[1]), float(lens.sensor_size[0]), float(lens.pixel_size))


@functools.lru_cache(maxsize=None)
def shared_lens(name):
    """never refocused: the tests that move the sensor make their own"""
    return make_lens(name)


@functools.lru_cache(maxsize=None)
def gpu_inputs():
    u, img = rc.fixed_inputs()
    return torch.as_tensor(u).to(DEV), torch.as_tensor(img).to(DEV)


@functools.lru_cache(maxsize=None)
def kernel_case(name, depth):
    """(reference case fed the GPU lens's own d_sensor and exit pupil and the test's scale, kernel output, kernel aux, scale)"""
    lens = shared_lens(name)
    scale = float(lens.calc_scale_pinhole(depth))
    pz, pr = lens.exit_pupil()
    case = rc.reference_case(name, depth, float(lens.d_sensor), (float(pz), float(pr)), scale, geom_of(lens))
    u, img = gpu_inputs()
    out, aux = lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, u=u, return_aux="valid")
    lens.check_flags()
    return case, out.cpu(), {k: v.cpu() for k, v in aux.items()}, scale


def ulp32(x):
    return np.spacing(np.abs(np.asarray(x, dtype=np.float32))).astype(np.float64)


@pytest.mark.parametrize("name,depth", CASES)
def test_validity_ray_by_ray(name, depth):
    """On every robust ray the kernel decides as float64 does - exactly; and robust rays are nearly all rays"""
    case, _, aux, _ = kernel_case(name, depth)
    assert aux["valid"].shape == case["robust"].shape and aux["valid"].dtype == torch.bool
    assert float((~case["robust"]).double().mean()) <= 1e-3
    assert float(case["pix"].double().mean()) >= 0.99
    assert float(case["ref"]["count"].min()) >= 1
    differ = (aux["valid"] != case["ref"]["valid"]) & case["robust"]
    assert int(differ.sum()) == 0
    assert torch.equal(aux["count"], aux["valid"].sum(1).float())


@pytest.mark.parametrize("name,depth", CASES)
def test_image_elementwise_against_float64(name, depth, margin):
    """On the pixels whose rays are all robust, both batch images: |kernel - float64| <= 4 F, F = the float32 oracle's own
    distance from float64 on the same pixels (this run).  The factor 4 pays for the kernel's one-ulp rcp / rsq / sin / cos
    hardware forms and FMA contraction where the oracle uses IEEE operations, at a maximum over ~4 600 single values.
    Measured on one MI355X (kernel / F): see DESIGN.md 4.15."""
    case, out, aux, _ = kernel_case(name, depth)
    pix = case["pix"]
    assert torch.equal(aux["count"][pix].double(), case["ref"]["count"][pix])
    F = rc.floor_distance(case)
    assert bool(torch.isfinite(F).all()) and float(F.min()) > 0
    d = ((out.double() - case["ref"]["img"]).abs() * pix.unsqueeze(0)).amax(dim=(1, 2, 3))
    for b in range(rc.B):
        print(f"raytrace {name} {depth:g} image {b}: kernel {float(d[b]):.3e}, float32 floor {float(F[b]):.3e}, ratio {float(d[b] / F[b]):.2f}")
        margin(f"raytrace {name} {depth:g} image {b}: |kernel - f64| / (4 x f32 floor {float(F[b]):.1e})", float(d[b] / (4 * F[b])), 1.0)


class _Replay:
    """a sampler that hands sample_pupil the given block"""
    on_device = False

    def __init__(self, block):
        self.block = block

    def rand_block(self, sizes):
        assert int(sum(sizes)) == self.block.numel()
        return self.block.clone()


@pytest.mark.parametrize("name,depth", CASES)
def test_composed_route_like_with_like(name, depth, margin):
    """The same uniforms through sample_sensor -> lens.trace (the generic kernel, backward) -> propagate_to(depth) -> the
    restatement's bilinear step in torch on the GPU: counts within 1 per pixel, pixels of identical validity within 4 F"""
    case, out, aux, scale = kernel_case(name, depth)
    lens = make_lens(name)
    u, img = gpu_inputs()
    uj, vi, alive = [], [], []
    for c, w in enumerate(WAVE_RGB):
        lens.sampler = _Replay(u[c].reshape(-1).cpu())
        ray = lens.sample_sensor(spp=rc.SPP, wvln=w)
        assert tuple(ray.o.shape) == (rc.SPP, rc.H, rc.W, 3)
        ray, _, _ = lens.trace(ray)
        ray = ray.propagate_to(depth)
        a, b = rc.scene_coords(ray.o[..., 0], ray.o[..., 1], (rc.H, rc.W), scale, lens.pixel_size)
        uj.append(a), vi.append(b), alive.append(ray.ra > 0)
    uj, vi = torch.stack(uj), torch.stack(vi)
    valid = rc.window_valid(torch.stack(alive), uj, vi, (rc.H, rc.W))
    comp, count = rc.bilinear_mean(img, uj, vi, valid)
    comp, count, valid = comp.cpu(), count.cpu(), valid.cpu()
    margin(f"raytrace {name} {depth:g} fused vs composed: valid count per pixel", float((count - aux["count"]).abs().max()), 1)
    same = (valid == aux["valid"]).all(1)
    assert float(same.double().mean()) >= 0.99
    F = rc.floor_distance(case)
    d = ((out.double() - comp.double()).abs() * same.unsqueeze(0)).amax(dim=(1, 2, 3))
    for b in range(rc.B):
        margin(f"raytrace {name} {depth:g} image {b}: |fused - composed| / (4 x f32 floor)", float(d[b] / (4 * F[b])), 1.0)


def test_generator():
    lens = shared_lens("rf50mm")
    _, img = gpu_inputs()
    depth, scale = -2000.0, float(lens.calc_scale_pinhole(-2000.0))
    seed = 0x1234_5678_9ABC_DEF1
    u = raytrace.sensor_uniforms(seed, rc.SPP, rc.H, rc.W, device=DEV)
    assert tuple(u.shape) == (3, rc.SPP, 2, rc.H, rc.W) and u.dtype == torch.float32
    assert float(u.min()) >= 0 and float(u.max()) < 1
    assert not torch.equal(u[0], u[1]) and not torch.equal(u[1], u[2]) and not torch.equal(u[0], u[2])
    by_seed = lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, seed=seed)
    assert torch.equal(by_seed, lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, u=u))
    assert torch.equal(by_seed, lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, seed=seed))
    assert not torch.equal(by_seed, lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, seed=seed + 1))
    # seed=None: one draw from torch's generator
    torch.manual_seed(3)
    a = lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale)
    b = lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale)
    torch.manual_seed(3)
    assert torch.equal(a, lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale)) and not torch.equal(a, b)
    # 3 * 4096 * 2 * 16 = 393 216 values: the mean of n uniforms has standard error sqrt(1 / (12 n))
    big = raytrace.sensor_uniforms(seed, 4096, 4, 4, device=DEV).double()
    assert float(big.min()) >= 0 and float(big.max()) < 1
    assert abs(float(big.mean()) - 0.5) <= 5 * (1 / (12 * big.numel())) ** 0.5
    for c in range(3):
        assert abs(float(big[c].mean()) - 0.5) <= 5 * (1 / (12 * big[c].numel())) ** 0.5
    lens.check_flags()


def test_batch_chunks_and_vignetting():
    """B = 5 (a launch of 4 images and one of 1 over the same rays) equals five B = 1 renders bit for bit; vignetting=True is
    sum / spp where the default is sum / count: equal to out * count / spp within 2 ulp"""
    lens = shared_lens("50mm_f2.8")
    u, img = gpu_inputs()
    depth, scale = -500.0, float(lens.calc_scale_pinhole(-500.0))
    g = torch.Generator().manual_seed(2)
    five = torch.cat((img, torch.rand((3, 3, rc.H, rc.W), generator=g).to(DEV)))
    out = lens.render_raytraced(five, depth=depth, spp=rc.SPP, scale=scale, u=u)
    assert tuple(out.shape) == (5, 3, rc.H, rc.W)
    for b in range(5):
        assert torch.equal(out[b:b + 1], lens.render_raytraced(five[b:b + 1], depth=depth, spp=rc.SPP, scale=scale, u=u)), b
    vig, aux = lens.render_raytraced(five, depth=depth, spp=rc.SPP, scale=scale, u=u, vignetting=True, return_aux=True)
    assert "valid" not in aux and float(aux["count"].min()) < rc.SPP             # the corners of this lens are vignetted
    want = out.double().cpu() * aux["count"].double().cpu() / rc.SPP
    err = (vig.double().cpu() - want).abs().numpy()
    assert bool((err <= 2 * ulp32(want.numpy())).all())
    lens.check_flags()


def test_large_grid_constant_image():
    """1024 x 1024 (4096 workgroups per channel, pixel indices beyond 2^20), spp 8, one launch: the constant 0.5 - exact under any
    pair of bilinear weights (1-f) + f, so the sum of 8 samples and its division are exact too - comes back within 2 ulp
    wherever a ray is valid and 0 elsewhere"""
    lens = make_lens("rf50mm", res=(1024, 1024))
    img = torch.full((1, 3, 1024, 1024), 0.5, device=DEV)
    out, aux = lens.render_raytraced(img, depth=-2000.0, spp=8, scale=float(lens.calc_scale_pinhole(-2000.0)), seed=11, return_aux=True)
    lit = aux["count"] > 0
    assert float(lit.float().mean()) > 0.9
    assert float((out[0][lit] - 0.5).abs().max()) <= 2 * float(ulp32(0.5))
    assert bool((out[0][~lit] == 0).all())
    assert float(aux["count"].max()) <= 8
    lens.check_flags()


def test_rays_that_leave_the_window():
    """A scale off by 4 x in either direction: finite output within the image's range, zeros where no ray counts, no flag.  With the
    scale 4 x too small a texel covers a sixteenth of the object area it should, the scene fills a quarter of the field in each
    direction and most rays land outside the window; 4 x too large, every ray lands in the scene's central texels."""
    lens = shared_lens("rf50mm")
    u, img = gpu_inputs()
    pinhole = float(lens.calc_scale_pinhole(-2000.0))
    for factor in (4.0, 0.25):
        out, aux = lens.render_raytraced(img, depth=-2000.0, spp=rc.SPP, scale=factor * pinhole, u=u, return_aux="valid")
        assert bool(torch.isfinite(out).all())
        share = float(aux["valid"].float().mean())
        assert 0 < share < 0.25 if factor < 1 else share > 0.5
        assert bool((out[:, aux["count"] == 0] == 0).all())
        assert float(out.min()) >= 0 and float(out.max()) <= 1
        assert torch.equal(aux["count"], aux["valid"].sum(1).float())
    lens.check_flags()


def test_stack_and_queued_refocus():
    """render_raytraced_stack = refocus + render per slice, and puts the sensor back; a render queued directly behind a refocus reads
    the sensor position that refocus writes (no host round trip in between)"""
    lens = make_lens("rf50mm")
    u, img = gpu_inputs()
    depth, scale = -2000.0, float(lens.calc_scale_pinhole(-2000.0))
    fds = [-1500.0, -2500.0]
    before = (lens.d_sensor, lens.hfov, lens.foclen, lens.fnum)
    torch.manual_seed(4)
    stack = raytrace.render_raytraced_stack(lens, img, depth, fds, spp=rc.SPP, scale=scale, u=u)
    assert tuple(stack.shape) == (rc.B, 3, 2, rc.H, rc.W)
    assert (lens.d_sensor, lens.hfov, lens.foclen, lens.fnum) == before
    torch.manual_seed(4)
    singles = []
    for fd in fds:
        lens.refocus(fd)                                     # queued; nothing reads the lens state back before the render
        singles.append(lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, u=u))
    assert torch.equal(stack, torch.stack(singles, dim=2))
    assert not torch.equal(stack[:, :, 0], stack[:, :, 1])
    torch.manual_seed(4)
    lens.refocus(fds[0])
    torch.cuda.synchronize()
    assert lens.d_sensor != before[0]                        # host read-back: the refocus has completed
    assert torch.equal(singles[0], lens.render_raytraced(img, depth=depth, spp=rc.SPP, scale=scale, u=u))
    lens.check_flags()
