"""GPU tests (run with `-m gpu` on an MI355X): the soft-depth-layer occluded PSF-map render (aadff_render_psf_map_stack_soft_occluded,
csrc/conv_occl_soft.hip; aadff/occlusion.py) against float64 on the CPU, bit for bit against the hard entry and against itself on the
exact consequences of its contract.

tests/soft_occl_common.py has the case table (the twelve shapes of the hard render's table with coordinate scenes, plus a case of edge
values; one case at least for every kernel instantiation), the comparator (the specification in float64 on the float32 decode of pos) and
the derived elementwise budget; tests/test_soft_occl_host.py anchors them on the CPU.  Every case asserts: every element of V
(normalize = 0), of the coverage and of the normalised output written (the outputs are pre-filled with a sentinel), finite and within the
budget, none excluded.  The largest share of the budget used is printed per case and recorded.  No number here comes from the kernel
under test.

Largest shares of the budget measured on an MI355X (V / coverage / out), case by case: see DESIGN.md 4.22.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import occlusion_common as oc                              # noqa: E402
import soft_occl_common as sc                              # noqa: E402
from aadff import _abi                                     # noqa: E402
from aadff import occlusion                                # noqa: E402

DEV = "cuda:0"
NAME = "aadff_render_psf_map_stack_soft_occluded"


def _entry(name, img, maps, third, L, grid, normalize=1, want_cov=True):
    """A C entry of the occluded family into sentinel-filled outputs: (out, coverage) float32 [B,C,S,H,W] on the CPU, after the
    every-element-written check."""
    B, Cn, H, W = img.shape
    S, ks = maps.shape[0] // L, maps.shape[-1] // grid
    x, m, t = img.to(DEV).contiguous(), maps.to(DEV).contiguous(), third.to(DEV).contiguous()
    out = torch.full((B, Cn, S, H, W), sc.SENTINEL, device=DEV)
    cov = torch.full((B, Cn, S, H, W), sc.SENTINEL, device=DEV) if want_cov else None
    _abi.call(name, _abi.ptr(x), _abi.ptr(m), _abi.ptr(t), _abi.ptr(out), _abi.ptr(cov), B, Cn, S, L, H, W, grid, ks, normalize,
              _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    res = []
    for r in (out, cov):
        if r is not None:
            r = r.cpu()
            left = int((r == sc.SENTINEL).sum())
            assert left == 0, f"{left} of {r.numel()} elements were never written"
            res.append(r)
    return res if want_cov else res[0]


def _run(img, maps, pos, L, grid, normalize=1, want_cov=True):
    assert pos.dtype == torch.float32
    return _entry(NAME, img, maps, pos, L, grid, normalize, want_cov)


def _hard(img, maps, layer, L, grid, normalize=1):
    assert layer.dtype == torch.uint8
    return _entry("aadff_render_psf_map_stack_occluded", img, maps, layer, L, grid, normalize)


def _same(a, b):
    """Bit for bit, NaN payloads and the sign of zero included."""
    return all(torch.equal(p.view(torch.int32), q.view(torch.int32)) for p, q in zip(a, b))


@pytest.mark.parametrize("c", sc.TABLE, ids=[c.id for c in sc.TABLE])
def test_case_against_float64(c, margin):
    assert sc.dispatch(c.ks) == c.kernel and c.kernel in sc.expected_instantiations()
    img, maps, pos, r = sc.reference(c)
    V, cov0 = _run(img, maps, pos, c.L, c.grid, normalize=0)
    out, cov = _run(img, maps, pos, c.L, c.grid, normalize=1)
    assert torch.equal(cov0, cov)
    assert torch.equal(cov == 0, r.A == 0), "A > 0 is an exact decision"
    uses = {}
    for what, got, want, budget in (("V", V, r.V, r.eV), ("coverage", cov, r.A, r.eA), ("out", out, r.out, r.eOut)):
        uses[what] = sc.share(got, want, budget)
    print(f"\n{c.id} [{c.kernel}; {c.scene}]: largest use of the elementwise budget " + ", ".join(f"{k} {u:.3f}" for k, (u, _) in uses.items()))
    for what, (use, worst) in uses.items():
        assert use <= 1.0, f"{c.id}: {what} element {worst} of {tuple(out.shape)} is {use:.2f} x its budget from float64"
        margin(f"soft occlusion {c.id}: {what}, share of the elementwise budget", use, 1.0)


# ------------------------------------------------------------------------------------------------ the exact consequences, bit for bit
@pytest.mark.parametrize("c", sc.HARD, ids=[c.id for c in sc.HARD])
def test_integral_coordinates_are_the_hard_render_bit_for_bit(c):
    img, maps, layer = oc.inputs(c)
    holes = layer >= c.L
    for hole_value in (float("nan"), -1.0):
        pos = layer.float()
        pos[holes] = hole_value
        for normalize in (0, 1):
            assert _same(_run(img, maps, pos, c.L, c.grid, normalize), _hard(img, maps, layer, c.L, c.grid, normalize)), (hole_value, normalize)
        if not bool(holes.any()):
            break


def test_single_node_gives_the_hard_single_layer_render_for_every_coordinate():
    c = sc.HOLE6                                                                 # L = 1, pos in [0, 3) and a hole block of -1
    img, maps, pos, _ = sc.reference(c)
    assert bool((pos > 1).any())
    layer = torch.where(pos >= 0, 0, oc.HOLE).to(torch.uint8)
    assert _same(_run(img, maps, pos, 1, c.grid), _hard(img, maps, layer, 1, c.grid))
    c = sc.GENERIC                                                               # the run-time-ks kernel: its first node alone, S = 2
    img, maps, pos, _ = sc.reference(c)
    one = maps.reshape(c.S, c.L, *maps.shape[1:])[:, 0].contiguous()
    assert _same(_run(img, one, pos, 1, c.grid), _hard(img, one, torch.zeros((c.B, c.H, c.W), dtype=torch.uint8), 1, c.grid))


def test_coordinates_above_the_last_node_count_as_the_last_node():
    for c in (sc.EDGES, sc.GENERIC):
        img, maps, pos, _ = sc.reference(c)
        top = float(c.L - 1)
        far = pos.clone()
        pick = torch.rand(pos.shape, generator=torch.Generator().manual_seed(5)) < 0.3
        far[pick] = top + 0.75
        far[0, 0, :3] = torch.tensor([1e30, float("inf"), top + 2.0 ** -20])
        assert int((far > top).sum()) > 3
        assert _same(_run(img, maps, far, c.L, c.grid), _run(img, maps, torch.where(far > top, top, far), c.L, c.grid))


def test_a_slab_with_no_texel_in_the_window_changes_nothing():
    """Nodes 0, 1 with a block of slab 2 in one corner, against the two-node render of the same coordinates (where the block clamps to
    node 1): outside the windows that see the block nothing differs - in the tiles that never stage slab 2 (the presence skip) and in the
    pixels of the block's own tiles whose window misses it (a slab that is staged but adds fma(T, 0, V))."""
    for ks in (7, 17):                                                           # the templated and the run-time-ks kernel
        H, W, grid, p = 70, 90, 2, ks // 2
        gen = torch.Generator().manual_seed(21 + ks)
        img = torch.rand((1, 2, H, W), generator=gen) * 37.5 - 3.0
        maps = oc.positive_maps(2 * 3, 2, grid, ks, gen)                         # S = 2, L = 3
        pos = torch.rand((1, H, W), generator=gen)                               # slab 0 ...
        pos[:, ::3, ::2] = 1.0                                                   # ... and node 1 itself (slab 1 with f = 0 / the last slab)
        pos[:, 3:9, 4:11] = 2.0
        three = _run(img, maps, pos, 3, grid)
        two = _run(img, maps.reshape(2, 3, *maps.shape[1:])[:, :2].reshape(4, *maps.shape[1:]).contiguous(), pos, 2, grid)
        sees = torch.zeros((H, W), dtype=torch.bool)
        sees[max(3 - p, 0):9 + p, max(4 - p, 0):11 + p] = True
        assert int((~sees[:32, :32]).sum()) > 0 and int(sees.sum()) < H * W // 2
        for a, b in zip(three, two):
            assert _same([a[..., ~sees]], [b[..., ~sees]]) and not torch.equal(a[..., sees], b[..., sees])


def test_power_of_two_image_scale_scales_V_bit_for_bit():
    for c in (sc.TABLE[0], sc.GENERIC):
        img, maps, pos, _ = sc.reference(c)
        V = _run(img, maps, pos, c.L, c.grid, normalize=0, want_cov=False)
        assert torch.equal(_run(img * 8.0, maps, pos, c.L, c.grid, normalize=0, want_cov=False), V * 8.0)
        assert torch.equal(_run(img * 0.25, maps, pos, c.L, c.grid, normalize=0, want_cov=False), V * 0.25)


def test_stack_equals_its_slices_and_repeats_bit_for_bit():
    for c in (sc.DISC, sc.GENERIC):                                              # ks 11, S 3, L 4; the run-time-ks kernel, S 2, L 3
        img, maps, pos, _ = sc.reference(c)
        a = _run(img, maps, pos, c.L, c.grid)
        assert _same(a, _run(img, maps, pos, c.L, c.grid))
        for s in range(c.S):
            one = _run(img, maps[s * c.L:(s + 1) * c.L], pos, c.L, c.grid)
            assert torch.equal(one[0][:, :, 0], a[0][:, :, s]) and torch.equal(one[1][:, :, 0], a[1][:, :, s]), s


def test_batch_equals_its_images_bit_for_bit():
    c = sc.BATCH
    img, maps, pos, _ = sc.reference(c)
    a = _run(img, maps, pos, c.L, c.grid)
    for b in range(c.B):
        one = _run(img[b:b + 1], maps, pos[b:b + 1], c.L, c.grid)
        assert torch.equal(one[0][0], a[0][b]) and torch.equal(one[1][0], a[1][b]), b


def test_nan_on_holes_reaches_nothing():
    for c in (sc.TABLE[0], sc.HOLE6, sc.EDGES):                                  # NaN holes; -1 holes; both
        img, maps, pos, _ = sc.reference(c)
        hole = ~(pos >= 0)
        assert int(hole.sum()) > 0
        base = _run(img, maps, pos, c.L, c.grid)
        bad = img.clone()
        bad[hole[:, None].expand_as(img)] = float("nan")
        got = _run(bad, maps, pos, c.L, c.grid)
        assert bool(torch.isfinite(got[0]).all()) and _same(got, base)


def test_nan_on_another_slab_stays_in_that_slab():
    """NaN on every texel of slab 1 (the right half of the image): the chains of the other slabs select it away, so a pixel whose window
    holds no slab-1 texel keeps its bits, also in the tiles that stage and walk slab 1; a pixel whose window holds one is NaN, as the
    contract says; and the coverage, which no image value enters, keeps every bit everywhere."""
    for c in (sc.TABLE[1], sc.GENERIC):                                          # ks 7, L 2 (slab 1 the last); the run-time-ks kernel, L 3
        img, maps, _, _ = sc.reference(c)
        pos = torch.rand((c.B, c.H, c.W), generator=torch.Generator().manual_seed(9)) * 0.75
        pos[:, :, c.W // 2 + 8:] += 1.0
        k, _f = sc.decode(pos, c.L)
        on1 = (k == 1)
        base = _run(img, maps, pos, c.L, c.grid)
        bad = img.clone()
        bad[on1[:, None].expand_as(img)] = float("nan")
        got = _run(bad, maps, pos, c.L, c.grid)
        p = c.ks // 2
        sees = torch.zeros((c.H, c.W), dtype=torch.bool)
        sees[:, c.W // 2 + 8 - p:] = True                                        # (the reflection at the left edge brings no slab-1 texel: p < W / 2)
        assert p < c.W // 2                                                      # (W 72, patches from 0, 36: the tile from 36 holds both kinds; W 64, ks 17: the tile 21 .. 41)
        assert torch.equal(got[1], base[1])
        assert bool(torch.isfinite(got[0][..., ~sees]).all()) and torch.equal(got[0][..., ~sees], base[0][..., ~sees])
        assert bool(torch.isnan(got[0][..., sees]).all())


def test_wrappers_call_the_entry():
    c = sc.DISC
    img, maps, pos, _ = sc.reference(c)
    want, wcov = _run(img, maps, pos, c.L, c.grid)
    got, cov = occlusion.render_psf_map_soft_occluded_stack(img.to(DEV), maps.to(DEV), pos.to(DEV).double(), c.L, c.grid, return_coverage=True)
    assert got.is_cuda and torch.equal(got.cpu(), want) and torch.equal(cov.cpu(), wcov)
    got = occlusion.render_psf_map_soft_occluded_stack(img, maps, pos, c.L, c.grid, normalize=False)     # CPU in, CPU out
    assert got.device.type == "cpu" and torch.equal(got, _run(img, maps, pos, c.L, c.grid, normalize=0, want_cov=False))
    one = occlusion.render_psf_map_soft_occluded(img, maps[c.L:2 * c.L], pos, c.grid)
    assert one.shape == (c.B, c.C, c.H, c.W) and torch.equal(one, want[:, :, 1])
    with pytest.raises(RuntimeError, match="reflect padding"):
        occlusion.render_psf_map_soft_occluded_stack(img[:, :, :5].to(DEV), maps.to(DEV), pos[:, :5], c.L, c.grid)


# ------------------------------------------------------------------------------------------------------------------- the call sites
def _lens(repo_root):
    from deeplens.optics import Lensgroup
    return Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(64, 64), device=DEV)


def _scene():
    from aadff.synth import synth_disc_depth_mm
    img = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(3)).to(DEV)
    depth = torch.from_numpy(synth_disc_depth_mm(64, 64)[0])[None, None].to(DEV)
    return img, depth


FOCUS, KW = [-700.0, -2000.0], dict(layers=3, grid=3, ks=11, spp=256)


def test_stack_renderer_soft_is_the_primitive_on_its_own_parts(repo_root, monkeypatch):
    """The PSF trace sums with float atomics, so two renders are not compared: the soft stack is compared with the primitive on the maps
    and the coordinate it returns, and its launches with those of occlusion=True."""
    from aadff.focal_stack import render_focal_stack_m1_layered
    lens = _lens(repo_root)
    img, depth = _scene()
    render_focal_stack_m1_layered(lens, img, depth, FOCUS, **KW)                 # the lens's one-time tables are built outside the recorded calls
    seen, real = [], _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: seen.append((name, tuple(v for v in a if isinstance(v, int)))) or real(name, *a))
    torch.manual_seed(0)
    out, maps, pos = render_focal_stack_m1_layered(lens, img, depth, FOCUS, occlusion="soft", return_parts=True, **KW)
    soft_calls = list(seen)
    assert out.shape == (1, 3, 2, 64, 64) and maps.shape == (6, 3, 33, 33) and bool(torch.isfinite(out).all())
    assert pos.dtype == torch.float32 and pos.shape == (1, 64, 64) and float(pos.min()) == 0.0 and float(pos.max()) == 2.0
    want, nodes = occlusion.depth_nodes(depth, 3)
    assert torch.equal(pos, want.reshape(1, 64, 64)) and bool((nodes[1:] < nodes[:-1]).all())
    assert torch.equal(out, occlusion.render_psf_map_soft_occluded_stack(img, maps, pos, 3, 3))
    del seen[:]
    torch.manual_seed(0)
    hard = render_focal_stack_m1_layered(lens, img, depth, FOCUS, occlusion=True, **KW)
    assert not torch.equal(hard, out)                                            # other field depths and another last step ...
    assert [n for n, _ in soft_calls[:-1]] == [n for n, _ in seen[:-1]] and len(seen) >= 3       # ... behind the same launches
    assert soft_calls[:-1] == seen[:-1]                                          # with the same shapes
    assert soft_calls[-1][0] == NAME and seen[-1][0] == "aadff_render_psf_map_stack_occluded" and soft_calls[-1][1] == seen[-1][1]


def test_lensgroup_render_occluded_soft(repo_root, monkeypatch):
    lens = _lens(repo_root)
    img, depth = _scene()
    lens.render_occluded(img, depth, layers=3, grid=3, ks=11, spp=256)
    seen, real = [], _abi.call
    monkeypatch.setattr(_abi, "call", lambda name, *a: seen.append((name, tuple(v for v in a if isinstance(v, int)))) or real(name, *a))
    soft = lens.render_occluded(img, depth, layers=3, grid=3, ks=11, spp=256, soft=True)
    soft_calls = list(seen)
    del seen[:]
    hard = lens.render_occluded(img, depth, layers=3, grid=3, ks=11, spp=256)
    assert soft.shape == hard.shape == (1, 3, 64, 64) and bool(torch.isfinite(soft).all()) and not torch.equal(soft, hard)
    assert soft_calls[-1][0] == NAME and seen[-1][0] == "aadff_render_psf_map_stack_occluded"
    assert soft_calls[-1][1] == seen[-1][1] and soft_calls[-1][1][:8] == (1, 3, 1, 3, 64, 64, 3, 11)
    traces = [n for n, _ in soft_calls if n.startswith("aadff_psf_points")]
    assert len(traces) == 3 == len([n for n, _ in seen if n.startswith("aadff_psf_points")])      # one psf_map per node, as one per layer
