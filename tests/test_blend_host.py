"""CPU: the blended PSF-map render (aadff_render_psf_map_blend_stack, csrc/conv_blend.hip; aadff/blend.py) - the symbol and its
binding, every argument error of the C entry before any HIP call, the wrapper's assertions, empty results and
refusals, the node closed forms, and the float64 comparator of tests/blend_common.py against a literal restatement and against the
properties the specification implies."""
import ctypes as C

import numpy as np
import pytest
import torch

import blend_common as bc
from aadff import _abi
from aadff import blend
from oracle import conv as oconv

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first


def _err(lib):
    return lib.aadff_last_error()


def _host(values):
    return (C.c_float * len(values))(*values)


def test_symbol_is_exported_and_bound():
    lib = _abi.load_library()
    assert "aadff_render_psf_map_blend_stack" in _abi.PROTOTYPES and len(_abi.PROTOTYPES["aadff_render_psf_map_blend_stack"]) == 13
    assert lib.aadff_render_psf_map_blend_stack.argtypes == _abi.PROTOTYPES["aadff_render_psf_map_blend_stack"]
    assert lib.aadff_abi_version() == _abi.ABI_VERSION == 9


def test_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = lib.aadff_render_psf_map_blend_stack
    n2, n3 = _host([0.0, 63.0]), _host([0.0, 31.5, 63.0])
    ok = (1, 3, 1, 64, 64, 2, 3, None)
    for hole in range(5):                                                        # every pointer
        ptrs = [P8, P8, P8, n2, n2]
        ptrs[hole] = None
        assert f(*ptrs, *ok) == -1 and b"NULL" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 1, 3, 1, 64, 64, 2, 4, None) == -1 and b"odd" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 1, 3, 1, 64, 64, 2, 53, None) == -1 and b"ks" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 1, 3, 1, 64, 64, 2, -1, None) == -1
    assert f(P8, P8, P8, n2, n2, 1, 3, 1, 64, 64, 65, 3, None) == -1 and b"grid" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 1, 3, 1, 64, 64, 0, 3, None) == -1 and b"grid" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 1, 3, 1, 5, 64, 2, 11, None) == -1 and b"pad" in _err(lib)            # H == ks / 2
    assert f(P8, P8, P8, n2, n2, 1, 3, 1, 64, 5, 2, 11, None) == -1 and b"pad" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 1, 3, 0, 64, 64, 2, 3, None) == -1 and b"empty" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 0, 3, 1, 64, 64, 2, 3, None) == -1 and b"empty" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 300, 300, 1, 64, 64, 2, 3, None) == -1 and b"too large" in _err(lib)
    assert f(P8, P8, P8, n2, n2, 1, 1, 1, 65535 * 32, 64, 2, 3, None) == -1 and b"too large" in _err(lib)
    for bad in (float("nan"), float("inf"), -float("inf")):
        assert f(P8, P8, P8, _host([0.0, bad, 63.0]), n3, 1, 3, 1, 64, 64, 3, 3, None) == -1 and b"node_y[1]" in _err(lib) and b"finite" in _err(lib)
        assert f(P8, P8, P8, n3, _host([0.0, 1.0, bad]), 1, 3, 1, 64, 64, 3, 3, None) == -1 and b"node_x[2]" in _err(lib)
    assert f(P8, P8, P8, _host([0.0, 31.5, 31.5]), n3, 1, 3, 1, 64, 64, 3, 3, None) == -1
    assert b"node_y" in _err(lib) and b"strictly increasing" in _err(lib) and b"index 2" in _err(lib)
    assert f(P8, P8, P8, n3, _host([5.0, 4.0, 63.0]), 1, 3, 1, 64, 64, 3, 3, None) == -1
    assert b"node_x" in _err(lib) and b"strictly increasing" in _err(lib) and b"index 1" in _err(lib)


def test_wrapper_assertions_and_empty_results():
    img, maps = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 10, 10)
    with pytest.raises(AssertionError, match=r"\[B, C, H, W\]"):
        blend.render_psf_map_blend_stack(img[0], maps, 2)
    with pytest.raises(AssertionError, match="divisible by grid"):
        blend.render_psf_map_blend_stack(img, maps, 3)
    with pytest.raises(AssertionError, match="should be odd"):
        blend.render_psf_map_blend_stack(img, torch.zeros(2, 3, 8, 8), 2)
    with pytest.raises(AssertionError, match="same channel"):
        blend.render_psf_map_blend_stack(img[:, :2], maps, 2)
    with pytest.raises(AssertionError, match="grid values"):
        blend.render_psf_map_blend_stack(img, maps, 2, nodes=(torch.zeros(3), torch.zeros(2)))
    with pytest.raises(ValueError, match="mode"):
        blend.render_psf_map_blend_stack(img, maps, 2, nodes="centre")
    with pytest.raises(AssertionError, match="PSF map should be"):
        blend.render_psf_map_blend(img, maps, 2)
    # empty batch / empty stack: an empty result without a GPU
    assert blend.render_psf_map_blend_stack(img[:0], maps, 2).shape == (0, 3, 2, 16, 16)
    assert blend.render_psf_map_blend_stack(img, maps[:0], 2).shape == (2, 3, 0, 16, 16)
    assert blend.render_psf_map_blend(img[:0], maps[0], 2).shape == (0, 3, 16, 16)
    # the same functions beside their patch twins
    import importlib
    rp = importlib.import_module("deeplens.render_psf")
    assert rp.render_psf_map_blend is blend.render_psf_map_blend and rp.render_psf_map_blend_stack is blend.render_psf_map_blend_stack
    from deeplens.optics import Lensgroup
    assert callable(Lensgroup.render_blended)


def test_no_cpu_fallback_and_grad_refused(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    img, maps = torch.zeros(1, 3, 16, 16), torch.zeros(1, 3, 10, 10)
    with pytest.raises(RuntimeError, match="no HIP device"):
        blend.render_psf_map_blend_stack(img, maps, 2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        blend.render_psf_map_blend(img, maps[0], 2, nodes="patch")
    for a, b in ((img.clone().requires_grad_(), maps), (img, maps.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="forward-only HIP op"):
            blend.render_psf_map_blend_stack(a, b, 2)
        with torch.no_grad(), pytest.raises(RuntimeError, match="no HIP device"):
            blend.render_psf_map_blend_stack(a, b, 2)


def test_blend_nodes_closed_forms():
    for n, g in ((45, 3), (1024, 7), (130, 5), (5, 64), (9, 7), (64, 2)):
        got = blend.blend_nodes(n, g, "psf_map")
        want = np.array([((-0.98 + 1.96 * j / (g - 1)) + 1) / 2 * n - 0.5 for j in range(g)]).astype(np.float32)
        assert got.dtype == torch.float32 and got.shape == (g,) and np.array_equal(got.numpy(), want)
        assert abs(float(got[0]) - (0.01 * n - 0.5)) < 1e-4 and abs(float(got[-1]) - (0.99 * n - 0.5)) < 1e-4
        assert bool((got[1:] > got[:-1]).all())
        got = blend.blend_nodes(n, g, "patch")
        assert np.array_equal(got.numpy(), np.array([(i + 0.5) / g * n - 0.5 for i in range(g)]).astype(np.float32))
        assert torch.equal(bc.closed_form_nodes(n, g, "psf_map"), blend.blend_nodes(n, g, "psf_map"))
    assert blend.blend_nodes(40, 1, "psf_map").tolist() == [19.5] and blend.blend_nodes(40, 1, "patch").tolist() == [19.5]
    with pytest.raises(ValueError):
        blend.blend_nodes(40, 3, "corner")


def test_table_reaches_every_instantiation():
    assert {c.kernel for c in bc.TABLE} == bc.expected_instantiations()
    for c in bc.TABLE:
        assert bc.dispatch(c.ks) == c.kernel, c.id
        ny, nx = bc.nodes_of(c)
        assert ny.shape == nx.shape == (c.grid,) and bool((ny[1:] > ny[:-1]).all()) and bool((nx[1:] > nx[:-1]).all())
    ex = next(c for c in bc.TABLE if c.nodes == "explicit")
    for nodes, n in ((bc.EXPLICIT_Y, ex.H), (bc.EXPLICIT_X, ex.W)):
        assert nodes[0] < 0 and nodes[-1] > n - 1 and np.floor(nodes[1]) == np.floor(nodes[2])


TINY = [(1, 2, 2, 7, 9, 3, 3, "psf_map"), (2, 1, 1, 6, 5, 2, 3, "patch"), (1, 1, 1, 5, 6, 1, 3, "psf_map"), (1, 1, 1, 8, 7, 4, 1, "explicit")]


def _tiny(t):
    B, Cn, S, H, W, g, ks, mode = t
    gen = torch.Generator().manual_seed(sum(t[:7]))
    img = torch.rand((B, Cn, H, W), generator=gen) * 37.5 - 3.0
    maps = torch.rand((S, Cn, g * ks, g * ks), generator=gen) - 0.3
    if mode == "explicit":
        ny, nx = torch.tensor([-2.5, 2.25, 2.5, 11.0]), torch.tensor([0.0, 1.0, 3.5, 6.0])
    else:
        ny, nx = bc.closed_form_nodes(H, g, mode), bc.closed_form_nodes(W, g, mode)
    return img, maps, g, ny, nx


@pytest.mark.parametrize("t", TINY, ids=[str(t) for t in TINY])
def test_comparator_is_the_literal_definition(t):
    img, maps, g, ny, nx = _tiny(t)
    want = bc.loop64(img, maps, g, ny, nx)
    got = bc.blend64(img, maps, g, ny, nx)
    assert float((got.out64 - want).abs().max()) <= 1e-13 * float(want.abs().max())
    assert bool((got.out64.abs() <= got.A * (1 + 1e-12)).all()) and bool((got.M >= got.out64.abs() * (1 - 1e-12)).all())


def test_comparator_constant_image_and_equal_tiles():
    g, ks, H, W = 3, 5, 21, 26
    gen = torch.Generator().manual_seed(5)
    maps = torch.rand((2, 2, g * ks, g * ks), generator=gen)
    ny, nx = bc.closed_form_nodes(H, g, "psf_map"), bc.closed_form_nodes(W, g, "psf_map")
    # a constant image: exactly the bilinear interpolation of the tile sums
    got = bc.blend64(torch.full((1, 2, H, W), 2.5), maps, g, ny, nx, want_bound=False).out64
    sums = maps.double().reshape(2, 2, g, ks, g, ks).sum((3, 5))                                   # [S,C,g,g]
    ky, fy = bc.axis_weights(ny, H)
    kx, fx = bc.axis_weights(nx, W)
    fy, fx = torch.from_numpy(fy)[:, None], torch.from_numpy(fx)[None, :]
    want = ((1 - fy) * ((1 - fx) * sums[:, :, ky][:, :, :, kx] + fx * sums[:, :, ky][:, :, :, kx + 1])
            + fy * ((1 - fx) * sums[:, :, ky + 1][:, :, :, kx] + fx * sums[:, :, ky + 1][:, :, :, kx + 1])) * 2.5
    assert float((got[0].permute(1, 0, 2, 3) - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # equal tiles: render_psf with that tile, whatever the weights
    img = torch.rand((2, 2, H, W), generator=gen) * 37.5 - 3.0
    tile = torch.rand((2, ks, ks), generator=gen)
    eq = tile[None, :, None, :, None, :].expand(1, 2, g, ks, g, ks).reshape(1, 2, g * ks, g * ks)
    got = bc.blend64(img, eq, g, ny, nx, want_bound=False).out64[:, :, 0]
    want = oconv.render_psf(img.double(), tile.double())
    assert float((got - want).abs().max()) <= 1e-13 * float(want.abs().max())
    # grid 1: oracle.conv.render_psf_map
    one = torch.rand((1, 2, ks, ks), generator=gen)
    got = bc.blend64(img, one, 1, bc.closed_form_nodes(H, 1, "psf_map"), bc.closed_form_nodes(W, 1, "psf_map"), want_bound=False).out64[:, :, 0]
    assert torch.equal(got, oconv.render_psf_map(img.double(), one[0].double(), 1))


def test_comparator_reproduces_a_bilinear_psf_field_and_patches_do_not():
    """A PSF field that is bilinear in position, sampled at the patch centres: inside the node hull the blend IS the per-pixel render
    (1e-12 relative), and the patch render of the same map misses it by more than 0.1 relative L2 - the test can tell the routes apart."""
    g, ks, H, W = 3, 5, 37, 45
    gen = torch.Generator().manual_seed(11)
    img = torch.rand((1, 2, H, W), generator=gen) * 37.5 - 3.0
    base = torch.rand((4, ks, ks), generator=gen).double()
    base[1:] = (base[1:] - 0.5) * 8.0
    y, x = torch.arange(H, dtype=torch.float64) / (H - 1), torch.arange(W, dtype=torch.float64) / (W - 1)
    field = lambda yy, xx: (base[0] + yy[..., None, None] * base[1] + xx[..., None, None] * base[2] + (yy * xx)[..., None, None] * base[3])      # noqa: E731
    psfs = field(y[:, None].expand(H, W), x[None, :].expand(H, W))                                # [H,W,ks,ks]
    ny, nx = bc.closed_form_nodes(H, g, "patch"), bc.closed_form_nodes(W, g, "patch")
    tiles = field((ny.double() / (H - 1))[:, None].expand(g, g), (nx.double() / (W - 1))[None, :].expand(g, g))       # [g,g,ks,ks]
    one = tiles.permute(0, 2, 1, 3).reshape(g * ks, g * ks)
    maps = torch.stack([one, one])[None]                                                            # [1,2,g ks,g ks], the same for both channels
    want = bc.per_pixel64(img, psfs)
    got = bc.blend64(img.double(), maps, g, ny, nx, want_bound=False).out64[:, :, 0]
    r0, r1 = int(np.ceil(float(ny[0]))), int(np.floor(float(ny[-1])))
    c0, c1 = int(np.ceil(float(nx[0]))), int(np.floor(float(nx[-1])))
    hull = (slice(None), slice(None), slice(r0, r1 + 1), slice(c0, c1 + 1))
    assert float((got[hull] - want[hull]).abs().max()) <= 1e-12 * float(want[hull].abs().max())
    # the interpolated per-pixel PSFs are the field itself there
    interp = bc.interpolated_psfs(one, g, ny, nx, H, W)
    assert float((interp[r0:r1 + 1, c0:c1 + 1] - psfs[r0:r1 + 1, c0:c1 + 1]).abs().max()) <= 1e-12 * float(psfs.abs().max())
    patch = oconv.render_psf_map(img.double(), maps[0], g)
    assert bc.rel_l2(patch[hull], want[hull]) > 0.1
    assert bc.rel_l2(got[hull], want[hull]) < 1e-12
