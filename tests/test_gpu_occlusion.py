"""GPU tests (run with `-m gpu` on an MI355X): the occlusion-aware layered PSF-map render (aadff_render_psf_map_stack_occluded,
csrc/conv_occl.hip; aadff/occlusion.py) against float64 on the CPU, bit for bit against itself, and on the exact consequences of
occlusion.

tests/occlusion_common.py has the case table (one case at least for every kernel instantiation), the comparator (the specification
with oracle.conv.render_psf_map on masked float64 inputs) and the derived elementwise budget; tests/test_occlusion_host.py anchors the
comparator on the CPU.  Every case asserts: every element of V (normalize = 0), of the coverage and of the normalised output written
(the outputs are pre-filled with a sentinel), finite and within the budget, none excluded.  The largest share of the budget used is
printed per case and recorded.  No number here comes from the kernel under test.

Largest shares of the budget measured on an MI355X (V / coverage / out), case by case: see DESIGN.md 4.20.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import occlusion_common as oc                              # noqa: E402
from aadff import _abi                                     # noqa: E402
from aadff import occlusion                                # noqa: E402

DEV = "cuda:0"


def _run(img, maps, layer, L, grid, normalize=1, want_cov=True):
    """The C entry into sentinel-filled outputs: (out, coverage) float32 [B,C,S,H,W] on the CPU, after the every-element-written check."""
    B, Cn, H, W = img.shape
    S, ks = maps.shape[0] // L, maps.shape[-1] // grid
    x, m, li = img.to(DEV).contiguous(), maps.to(DEV).contiguous(), layer.to(DEV).contiguous()
    assert li.dtype == torch.uint8
    out = torch.full((B, Cn, S, H, W), oc.SENTINEL, device=DEV)
    cov = torch.full((B, Cn, S, H, W), oc.SENTINEL, device=DEV) if want_cov else None
    _abi.call("aadff_render_psf_map_stack_occluded", _abi.ptr(x), _abi.ptr(m), _abi.ptr(li), _abi.ptr(out), _abi.ptr(cov), B, Cn, S, L, H, W, grid, ks,
              normalize, _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    res = []
    for t in (out, cov):
        if t is not None:
            t = t.cpu()
            left = int((t == oc.SENTINEL).sum())
            assert left == 0, f"{left} of {t.numel()} elements were never written"
            res.append(t)
    return res if want_cov else res[0]


@pytest.mark.parametrize("c", oc.TABLE, ids=[c.id for c in oc.TABLE])
def test_case_against_float64(c, margin):
    assert oc.dispatch(c.ks) == c.kernel and c.kernel in oc.expected_instantiations()
    img, maps, layer, r = oc.reference(c)
    V, cov0 = _run(img, maps, layer, c.L, c.grid, normalize=0)
    out, cov = _run(img, maps, layer, c.L, c.grid, normalize=1)
    assert torch.equal(cov0, cov)
    assert torch.equal(cov == 0, r.A == 0), "A > 0 is an exact decision"
    uses = {}
    for what, got, want, budget in (("V", V, r.V, r.eV), ("coverage", cov, r.A, r.eA), ("out", out, r.out, r.eOut)):
        uses[what] = oc.share(got, want, budget)
    print(f"\n{c.id} [{c.kernel}; {c.reaches}]: largest use of the elementwise budget " + ", ".join(f"{k} {u:.3f}" for k, (u, _) in uses.items()))
    for what, (use, worst) in uses.items():
        assert use <= 1.0, f"{c.id}: {what} element {worst} of {tuple(out.shape)} is {use:.2f} x its budget from float64"
        margin(f"occlusion {c.id}: {what}, share of the elementwise budget", use, 1.0)


def test_all_k_map_under_an_L_layer_table_equals_the_single_layer_call_bit_for_bit():
    c = oc.DISC
    img, maps, _, _ = oc.reference(c)
    G = c.grid * c.ks
    for k in range(c.L):
        full = _run(img, maps, torch.full((c.B, c.H, c.W), k, dtype=torch.uint8), c.L, c.grid, normalize=0)
        one = _run(img, maps.reshape(c.S, c.L, c.C, G, G)[:, k].contiguous(), torch.zeros((c.B, c.H, c.W), dtype=torch.uint8), 1, c.grid, normalize=0)
        assert torch.equal(full[0], one[0]) and torch.equal(full[1], one[1]), k


def test_stack_equals_its_slices_and_repeats_bit_for_bit():
    for c in (oc.DISC, oc.TABLE[6]):                                            # ks 11, S 3, L 4; the run-time-ks kernel, S 2, L 3
        img, maps, layer, _ = oc.reference(c)
        a = _run(img, maps, layer, c.L, c.grid)
        b = _run(img, maps, layer, c.L, c.grid)
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
        for s in range(c.S):
            one = _run(img, maps[s * c.L:(s + 1) * c.L], layer, c.L, c.grid)
            assert torch.equal(one[0][:, :, 0], a[0][:, :, s]) and torch.equal(one[1][:, :, 0], a[1][:, :, s]), s


def test_batch_equals_its_images_bit_for_bit():
    c = oc.BATCH
    img, maps, layer, _ = oc.reference(c)
    a = _run(img, maps, layer, c.L, c.grid)
    for b in range(c.B):
        one = _run(img[b:b + 1], maps, layer[b:b + 1], c.L, c.grid)
        assert torch.equal(one[0][0], a[0][b]) and torch.equal(one[1][0], a[1][b]), b


def test_wrappers_call_the_entry_and_take_int64_layers():
    c = oc.DISC
    img, maps, layer, _ = oc.reference(c)
    want, wcov = _run(img, maps, layer, c.L, c.grid)
    got, cov = occlusion.render_psf_map_occluded_stack(img.to(DEV), maps.to(DEV), layer.to(DEV).long(), c.L, c.grid, return_coverage=True)
    assert got.is_cuda and torch.equal(got.cpu(), want) and torch.equal(cov.cpu(), wcov)
    got = occlusion.render_psf_map_occluded_stack(img, maps, layer, c.L, c.grid, normalize=False)          # CPU in, CPU out
    assert got.device.type == "cpu" and torch.equal(got, _run(img, maps, layer, c.L, c.grid, normalize=0, want_cov=False))
    one = occlusion.render_psf_map_occluded(img, maps[c.L:2 * c.L], layer, c.grid)
    assert one.shape == (c.B, c.C, c.H, c.W) and torch.equal(one, want[:, :, 1])
    with pytest.raises(RuntimeError, match="reflect padding"):
        occlusion.render_psf_map_occluded_stack(img[:, :, :5].to(DEV), maps.to(DEV), layer[:, :5], c.L, c.grid)


# ------------------------------------------------------------------------------------------------------------ occlusion itself, exact
RECT = (slice(14, 31), slice(20, 45))                       # the rectangle on layer 0 of a 48 x 64 scene, background on layer 1


def _rect_scene(ks, grid=2, seed=77):
    H, W = 48, 64
    gen = torch.Generator().manual_seed(seed + ks)
    img = torch.rand((1, 2, H, W), generator=gen) * 37.5 - 3.0
    maps = oc.positive_maps(2, 2, grid, ks, gen)
    layer = torch.ones((1, H, W), dtype=torch.uint8)
    layer[0][RECT] = 0
    return img, maps, layer, grid


def test_foreground_texels_change_no_pixel_they_do_not_cover():
    img, maps, layer, grid = _rect_scene(7)
    base = _run(img, maps, layer, 2, grid, want_cov=False)
    # a_0 of every pixel: the coverage of an L = 1 call on the mask's own layer (holes elsewhere)
    own = layer.clone()
    own[layer != 0] = oc.HOLE
    a0 = _run(img, maps[:1], own, 1, grid)[1]
    r = oc.occl64(img, maps[:1], own, 1, grid, want_bound=False)
    assert torch.equal(a0 == 0, r.A == 0)
    other = img.clone()
    other[0, :, RECT[0], RECT[1]] = torch.rand((2, 17, 25), generator=torch.Generator().manual_seed(1)) * 1000.0 - 500.0
    moved = _run(other, maps, layer, 2, grid, want_cov=False)
    free = a0 == 0
    assert int(free.sum()) > 0 and int((~free).sum()) > 0
    assert torch.equal(moved[free], base[free])
    assert not torch.equal(moved[~free], base[~free])


def test_delta_psf_on_the_foreground_shows_the_image_exactly_inside_the_rectangle():
    ks, grid = 7, 2
    img, maps, layer, _ = _rect_scene(ks)
    maps = maps.clone().reshape(2, 2, grid, ks, grid, ks)
    maps[0] = 0.0
    maps[0, :, :, ks // 2, :, ks // 2] = 1.0                                      # layer 0: a delta in every tile
    maps = maps.reshape(2, 2, grid * ks, grid * ks)
    p = ks // 2
    inner = (slice(None), slice(None), 0, slice(RECT[0].start + p, RECT[0].stop - p), slice(RECT[1].start + p, RECT[1].stop - p))
    for seed in (0, 1):                                                          # whatever the background's PSF is
        m = maps.clone()
        m[1] = oc.positive_maps(1, 2, grid, ks, torch.Generator().manual_seed(seed))[0]
        out, cov = _run(img, m, layer, 2, grid)
        assert torch.equal(out[inner], img[:, :, inner[3], inner[4]])
        assert bool((cov[inner] == 1).all())


def test_constant_image_without_holes_stays_constant_exactly():
    for c in (oc.TABLE[1], oc.DISC, oc.TABLE[6]):
        _, maps, layer, _ = oc.reference(c)
        assert int((layer >= c.L).sum()) == 0
        out, cov = _run(torch.full((c.B, c.C, c.H, c.W), 0.5), maps, layer, c.L, c.grid)
        assert bool((cov > 0).all()) and bool((out == 0.5).all())


def test_nan_on_hole_texels_leaves_the_output_finite_and_unchanged():
    c = oc.HOLE6
    img, maps, layer, _ = oc.reference(c)
    base = _run(img, maps, layer, c.L, c.grid)
    bad = img.clone()
    bad[:, :, layer[0] == oc.HOLE] = float("nan")
    assert int(torch.isnan(bad).sum()) == 36
    got = _run(bad, maps, layer, c.L, c.grid)
    assert bool(torch.isfinite(got[0]).all()) and torch.equal(got[0], base[0]) and torch.equal(got[1], base[1])
    assert int((got[1] == 0).sum()) == 16 and bool((got[0][got[1] == 0] == 0).all())


def test_power_of_two_image_scale_scales_V_bit_for_bit():
    c = oc.TABLE[0]
    img, maps, layer, _ = oc.reference(c)
    V = _run(img, maps, layer, c.L, c.grid, normalize=0, want_cov=False)
    assert torch.equal(_run(img * 8.0, maps, layer, c.L, c.grid, normalize=0, want_cov=False), V * 8.0)


# ------------------------------------------------------------------------------------------------------------------- the stack renderer
def _lens(repo_root):
    from deeplens.optics import Lensgroup
    return Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(64, 64), device=DEV)


def _scene():
    from aadff.synth import synth_disc_depth_mm
    img = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(3)).to(DEV)
    depth = torch.from_numpy(synth_disc_depth_mm(64, 64)[0])[None, None].to(DEV)
    return img, depth


def _recorded(monkeypatch):
    """Every _abi.call from here on is recorded as (name, its integer arguments): the launches of a render and their shapes."""
    seen, real = [], _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: seen.append((name, tuple(v for v in a if isinstance(v, int)))) or real(name, *a))
    return seen


def _rel(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


FOCUS, KW, SPP = [-700.0, -2000.0], dict(layers=3, grid=3, ks=11, spp=256), 256


def test_stack_renderer_with_occlusion_is_the_primitive_on_its_own_parts(repo_root, monkeypatch):
    from aadff.focal_stack import render_focal_stack_m1_layered
    lens = _lens(repo_root)
    img, depth = _scene()
    render_focal_stack_m1_layered(lens, img, depth, FOCUS, **KW)                 # the lens's one-time tables are built outside the recorded calls
    seen = _recorded(monkeypatch)
    torch.manual_seed(0)
    out, maps, lidx = render_focal_stack_m1_layered(lens, img, depth, FOCUS, occlusion=True, return_parts=True, **KW)
    with_occlusion = list(seen)
    del seen[:]
    assert out.shape == (1, 3, 2, 64, 64) and maps.shape == (6, 3, 33, 33) and lidx.dtype == torch.uint8 and bool(torch.isfinite(out).all())
    assert torch.equal(out, occlusion.render_psf_map_occluded_stack(img, maps, lidx, 3, 3))
    del seen[:]
    torch.manual_seed(0)
    sel = render_focal_stack_m1_layered(lens, img, depth, FOCUS, **KW)
    assert not torch.equal(sel, out)                                             # another last step ...
    assert with_occlusion[:-1] == seen[:-1] and len(seen) >= 3                   # ... behind the same refocus and PSF-grid launches
    assert with_occlusion[-1][0] == "aadff_render_psf_map_stack_occluded" and seen[-1][0] == "aadff_render_psf_map_stack_layered"


def test_stack_renderer_without_occlusion_is_unchanged(repo_root, monkeypatch):
    """occlusion=False against a call that omits the argument, same seed: the same launches with the same arguments, the same index map,
    and each result is the select kernel on ITS OWN maps bit for bit.  The two results themselves are compared bit for bit only through
    these: the PSF histograms are summed with float atomics (tests/test_gpu_parity.py: 'run-to-run 1e-7'), so two traces of the same
    rays differ by the order of at most spp positive terms per bin - each within (spp - 1) U of the exact bin, the normalising sum alike:
    2 (spp + 2) U on the maps in relative L2, twice that on the render of a positive image."""
    from aadff.focal_stack import render_focal_stack_m1_layered
    lens = _lens(repo_root)
    img, depth = _scene()
    render_focal_stack_m1_layered(lens, img, depth, FOCUS, **KW)
    seen = _recorded(monkeypatch)
    res, calls = [], []
    for extra in ({}, {"occlusion": False}):
        del seen[:]
        torch.manual_seed(0)
        res.append(render_focal_stack_m1_layered(lens, img, depth, FOCUS, return_parts=True, **KW, **extra))
        calls.append(list(seen))
    assert calls[0] == calls[1] and calls[0][-1][0] == "aadff_render_psf_map_stack_layered"
    assert torch.equal(res[0][2], res[1][2])
    for out, maps, lidx in res:
        sel = torch.empty_like(out)
        _abi.call("aadff_render_psf_map_stack_layered", _abi.ptr(img), _abi.ptr(maps), _abi.ptr(lidx), _abi.ptr(sel), 1, 3, 2, 3, 64, 64, 3, 11,
                  _abi.stream_ptr(torch.device(DEV)))
        torch.cuda.synchronize()
        assert torch.equal(sel, out)
    assert _rel(res[0][1], res[1][1]) <= 2 * (SPP + 2) * oc.U
    assert _rel(res[0][0], res[1][0]) <= 4 * (SPP + 2) * oc.U
