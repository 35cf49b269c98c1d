"""GPU tests (run with `-m gpu` on an MI355X): the blended PSF-map render (aadff_render_psf_map_blend_stack, csrc/conv_blend.hip;
aadff/blend.py) against float64 on the CPU.

tests/blend_common.py has the case table (one case at least for every kernel instantiation, named by `dispatch`), the comparator (the
specification with oracle.conv.render_psf in float64) and the derived elementwise budget; tests/test_blend_host.py anchors the
comparator on the CPU.  Every case asserts: the instantiation it reaches; every element written (the output is pre-filled with a
sentinel), finite and within the budget, none excluded.  The relative L2 is printed and recorded, not gated.  No number here comes
from the kernel under test.
"""
import ctypes as C
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import blend_common as bc                                  # noqa: E402
from aadff import _abi                                     # noqa: E402
from aadff import blend                                    # noqa: E402

DEV = "cuda:0"


def _host_ptr(t):
    assert t.dtype == torch.float32 and t.is_contiguous() and not t.is_cuda
    return C.c_void_p(t.data_ptr())


def _run(img, maps, ny, nx, grid):
    """The C entry into a sentinel-filled output: float32 [B,C,S,H,W] on the CPU, after the every-element-written check."""
    B, Cn, H, W = img.shape
    S, ks = maps.shape[0], maps.shape[-1] // grid
    x, m = img.to(DEV).contiguous(), maps.to(DEV).contiguous()
    out = torch.full((B, Cn, S, H, W), bc.SENTINEL, device=DEV)
    _abi.call("aadff_render_psf_map_blend_stack", _abi.ptr(x), _abi.ptr(m), _abi.ptr(out), _host_ptr(ny), _host_ptr(nx), B, Cn, S, H, W, grid, ks,
              _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    got = out.cpu()
    left = int((got == bc.SENTINEL).sum())
    assert left == 0, f"{left} of {got.numel()} elements were never written"
    assert bool(torch.isfinite(got).all())
    return got


@pytest.mark.parametrize("c", bc.TABLE, ids=[c.id for c in bc.TABLE])
def test_case_against_float64(c, margin):
    assert bc.dispatch(c.ks) == c.kernel and c.kernel in bc.expected_instantiations()
    img, maps, ny, nx, r = bc.reference(c)
    got = _run(img, maps, ny, nx, c.grid)
    use, worst, rel = bc.compare(c.ks, got, r)
    err = float((got.double() - r.out64).abs().flatten()[worst])
    print(f"\n{c.id} [{c.kernel}; {c.reaches}]: largest use of the elementwise budget {use:.3f}; rel_l2 {rel:.3e}")
    assert use <= 1.0, f"{c.id}: element {worst} of {tuple(got.shape)} is {err:.3e} from float64, {use:.2f} x its budget"
    margin(f"blend {c.id}: share of the elementwise budget", use, 1.0)
    margin(f"blend {c.id}: rel_l2 (reported, not gated)", rel, float("inf"))


def test_stack_equals_its_slices_and_repeats_bit_for_bit():
    c = bc.TABLE[2]                                                              # S 3, ks 11
    img, maps, ny, nx, _ = bc.reference(c)
    x, m = img.to(DEV), maps.to(DEV)
    a = blend.render_psf_map_blend_stack(x, m, c.grid)
    b = blend.render_psf_map_blend_stack(x, m, c.grid)
    assert torch.equal(a, b)
    assert torch.equal(a.cpu(), _run(img, maps, ny, nx, c.grid))                 # the wrapper's default nodes are the case's
    for s in range(c.S):
        assert torch.equal(blend.render_psf_map_blend(x, m[s], c.grid), a[:, :, s]), s
    c = bc.TABLE[6]                                                              # the run-time-ks kernel
    img, maps, ny, nx, _ = bc.reference(c)
    a = _run(img, maps, ny, nx, c.grid)
    assert torch.equal(a, _run(img, maps, ny, nx, c.grid))
    for s in range(c.S):
        assert torch.equal(_run(img, maps[s:s + 1], ny, nx, c.grid)[:, :, 0], a[:, :, s]), s


def test_cpu_input_comes_back_on_the_cpu_and_explicit_nodes_are_taken():
    c = bc.TABLE[8]
    img, maps, ny, nx, r = bc.reference(c)
    got = blend.render_psf_map_blend_stack(img, maps, c.grid, nodes=(ny, nx.tolist()))
    assert got.device.type == "cpu" and torch.equal(got, _run(img, maps, ny, nx, c.grid))
    other = blend.render_psf_map_blend_stack(img, maps, c.grid, nodes="patch")
    assert not torch.equal(other, got)


def _plain_patch_stack(img, maps, grid, monkeypatch):
    """render_psf_map_stack on its plain-fp32 kernels (packed FMA / generic), whose budget is tests/conv_paths_common.py's plain one."""
    from deeplens.render_psf import render_psf_map_stack
    monkeypatch.setenv("AADFF_CONV_PATH", "valu")
    out = render_psf_map_stack(img.to(DEV), maps.to(DEV), grid)
    torch.cuda.synchronize()
    monkeypatch.delenv("AADFF_CONV_PATH")
    return out.cpu()


def test_equal_tiles_and_grid_one_agree_with_the_patch_render(monkeypatch):
    g, ks, H, W = 3, 7, 50, 70
    gen = torch.Generator().manual_seed(21)
    img = torch.rand((1, 2, H, W), generator=gen) * 37.5 - 3.0
    tile = torch.rand((2, 2, ks, ks), generator=gen) + 0.05
    tile = tile / tile.sum((2, 3), keepdim=True)
    eq = tile[:, :, None, :, None, :].expand(2, 2, g, ks, g, ks).reshape(2, 2, g * ks, g * ks).contiguous()
    ny, nx = bc.closed_form_nodes(H, g, "psf_map"), bc.closed_form_nodes(W, g, "psf_map")
    for maps, grid, nodes in ((eq, g, (ny, nx)), (tile.contiguous(), 1, (bc.closed_form_nodes(H, 1, "psf_map"), bc.closed_form_nodes(W, 1, "psf_map")))):
        r = bc.blend64(img, maps, grid, *nodes)
        got = _run(img, maps, *nodes, grid)
        patch = _plain_patch_stack(img, maps, grid, monkeypatch)
        room = bc.bound(ks, r) + bc.plain_bound(ks, r)                          # each kernel within its own budget of the one float64 answer
        assert bool(((got.double() - patch.double()).abs() <= room).all())
        assert bool(((patch.double() - r.out64).abs() <= bc.plain_bound(ks, r)).all())


def test_constant_image_gives_the_interpolated_tile_sums():
    c = bc.TABLE[0]
    _, maps, ny, nx, _ = bc.reference(c)
    img = torch.full((1, c.C, c.H, c.W), 2.5)
    got = _run(img, maps, ny, nx, c.grid)
    g, ks = c.grid, c.ks
    sums = maps.double().reshape(c.S, c.C, g, ks, g, ks).sum((3, 5))             # [S,C,g,g]
    ky, fy = bc.axis_weights(ny, c.H)
    kx, fx = bc.axis_weights(nx, c.W)
    fy, fx = torch.from_numpy(fy)[:, None], torch.from_numpy(fx)[None, :]
    want = ((1 - fy) * ((1 - fx) * sums[:, :, ky][:, :, :, kx] + fx * sums[:, :, ky][:, :, :, kx + 1])
            + fy * ((1 - fx) * sums[:, :, ky + 1][:, :, :, kx] + fx * sums[:, :, ky + 1][:, :, :, kx + 1])) * 2.5
    want = want.permute(1, 0, 2, 3)[None]                                        # [1,C,S,H,W]
    r = bc.Ref(want, want.abs(), torch.full_like(want, 2.5 * float(sums.max())))     # positive taps: A = |out|, M <= 2.5 max tile sum
    assert bool(((got.double() - want).abs() <= bc.bound(ks, r)).all())


def test_interior_agrees_with_the_per_pixel_gather():
    """Two independent kernels, one answer: local_psf_render fed the flipped, interpolated per-pixel PSFs (rounded to float32: one more
    U sum|x w|) agrees with the blend further than ks / 2 from the border, where replicate and reflect padding do not matter."""
    from deeplens.render_psf import local_psf_render
    c = bc.TABLE[0]                                                              # 37 x 45, grid 3, ks 5
    img, maps, ny, nx, r = bc.reference(c)
    got = _run(img, maps, ny, nx, c.grid)
    ks, p = c.ks, c.ks // 2
    inner = (slice(None), slice(p, c.H - p), slice(p, c.W - p))
    for ch in range(c.C):
        psfs = bc.interpolated_psfs(maps[0, ch], c.grid, ny, nx, c.H, c.W).flip(-1, -2).float()
        loc = local_psf_render(img[:, ch:ch + 1].to(DEV), psfs[None].expand(c.B, -1, -1, -1, -1).contiguous().to(DEV), kernel_size=ks).cpu()[:, 0]
        A, o64 = r.A[:, ch, 0], r.out64[:, ch, 0]
        room = bc.bound(ks, r)[:, ch, 0] + (ks * ks + 1) * bc.U * A + bc.U * o64.abs()
        diff = (got[:, ch, 0].double() - loc.double()).abs()
        assert bool((diff[inner] <= room[inner]).all()), ch
        assert bool(((loc.double() - o64).abs()[inner] <= ((ks * ks + 1) * bc.U * A + bc.U * o64.abs())[inner]).all()), ch


def test_lens_render_blended_composes_psf_map_and_the_blend(repo_root, monkeypatch):
    """render_blended is psf_map composed with render_psf_map_blend: bit for bit on the map it traced, and on the same seed equal to the
    composition done by hand up to what psf_map itself repeats to - its histogram is summed with float atomics, so two traces of the
    same rays differ by the order of at most spp positive terms per bin: (spp + 2) U relative, bin by bin, hence in L2."""
    from deeplens.optics import Lensgroup
    lens = Lensgroup(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(64, 64), device=DEV)
    img = torch.rand((1, 3, 64, 64), generator=torch.Generator().manual_seed(3)).to(DEV)
    kw = dict(depth=-1500.0, grid=3, ks=11, spp=512)
    trace, seen = lens.psf_map, []
    trace(**kw)                                                                  # the lens's one-time tables are built outside the seeded calls
    monkeypatch.setattr(lens, "psf_map", lambda **k: seen.append((k, trace(**k))) or seen[-1][1])
    torch.manual_seed(0)
    got = lens.render_blended(img, **kw)
    assert len(seen) == 1 and seen[0][0] == kw
    used = seen[0][1]
    assert got.shape == (1, 3, 64, 64) and bool(torch.isfinite(got).all())
    assert torch.equal(got, blend.render_psf_map_blend(img, used, 3))
    torch.manual_seed(0)
    again = trace(**kw)
    tol = (kw["spp"] + 2) * bc.U
    assert bc.rel_l2(again, used) <= tol
    assert bc.rel_l2(blend.render_psf_map_blend(img, again, 3), got) <= tol + 2 * (11 * 11 + bc.C1 + bc.C2 + 1) * bc.U
    assert 0.5 < float(got.mean() / img.mean()) < 1.5


def test_wrapper_refuses_what_the_entry_refuses():
    c = bc.TABLE[0]
    img, maps, ny, nx, _ = bc.reference(c)
    with pytest.raises(RuntimeError, match="node_x is not strictly increasing at index 2"):
        blend.render_psf_map_blend_stack(img.to(DEV), maps.to(DEV), c.grid, nodes=(ny, torch.tensor([0.0, 5.0, 5.0])))
    with pytest.raises(RuntimeError, match="reflect padding"):
        blend.render_psf_map_blend_stack(img[:, :, :2].to(DEV), maps.to(DEV), c.grid)
