"""CPU: the occlusion-aware layered PSF-map render (aadff_render_psf_map_stack_occluded, csrc/conv_occl.hip; aadff/occlusion.py) - the
symbol and its binding, every argument error of the C entry before any HIP call, the wrappers' checks before a device is needed, and the
float64 comparator of tests/occlusion_common.py against a literal restatement and against the properties the specification implies."""
import ctypes as C
import inspect

import pytest
import torch

import occlusion_common as oc
from aadff import _abi
from aadff import occlusion
from oracle import conv as oconv

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
NAME = "aadff_render_psf_map_stack_occluded"


def _err(lib):
    return lib.aadff_last_error()


def test_symbol_is_exported_and_bound():
    lib = _abi.load_library()
    assert NAME in _abi.PROTOTYPES and len(_abi.PROTOTYPES[NAME]) == 15
    assert getattr(lib, NAME).argtypes == _abi.PROTOTYPES[NAME]
    assert lib.aadff_abi_version() == _abi.ABI_VERSION == 9


def test_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = getattr(lib, NAME)

    def call(B=1, Cn=3, S=1, L=2, H=64, W=64, grid=2, ks=3, ptrs=(P8, P8, P8, P8, None)):
        return f(*ptrs, B, Cn, S, L, H, W, grid, ks, 1, None)

    for hole in range(4):                                                        # every required pointer; coverage may be NULL
        ptrs = [P8, P8, P8, P8, P8]
        ptrs[hole] = None
        assert call(ptrs=ptrs) == -1 and b"NULL" in _err(lib)
    assert call(ks=4) == -1 and b"odd" in _err(lib)
    for ks in (1, 53, -1):
        assert call(ks=ks) == -1 and b"ks" in _err(lib) and b"outside [3,51]" in _err(lib)
    for L in (0, 33, -2):
        assert call(L=L) == -1 and b"layers outside [1,32]" in _err(lib)
    for grid in (0, 65):
        assert call(grid=grid) == -1 and b"grid" in _err(lib) and b"outside [1,64]" in _err(lib)
    assert call(H=5, W=64, grid=6) == -1 and b"grid 6 above min(H,W) = 5" in _err(lib)
    assert call(H=64, W=7, grid=8) == -1 and b"above min(H,W) = 7" in _err(lib)
    assert call(H=5, ks=11) == -1 and b"pad" in _err(lib)                        # H == ks / 2
    assert call(W=5, ks=11) == -1 and b"pad" in _err(lib)
    assert call(S=0) == -1 and b"empty" in _err(lib)
    assert call(B=0) == -1 and b"empty" in _err(lib)
    assert call(B=300, Cn=300) == -1 and b"too large" in _err(lib)
    assert call(Cn=1, H=65535 * 32) == -1 and b"too large" in _err(lib)


TINY = [(1, 2, 2, 3, 7, 9, 3, 3), (2, 1, 1, 2, 6, 5, 2, 3)]                      # B, C, S, L, H, W, grid, ks


def _tiny(t):
    B, Cn, S, L, H, W, g, ks = t
    gen = torch.Generator().manual_seed(sum(t))
    img = torch.rand((B, Cn, H, W), generator=gen) * 37.5 - 3.0
    maps = oc.positive_maps(S * L, Cn, g, ks, gen)
    lay = torch.randint(0, L + 1, (B, H, W), generator=gen).to(torch.uint8)     # index L: holes
    return img, maps, lay, L, g


@pytest.mark.parametrize("t", TINY, ids=[str(t) for t in TINY])
def test_comparator_is_the_literal_definition(t):
    img, maps, lay, L, g = _tiny(t)
    V, A, out = oc.loop64(img, maps, lay, L, g)
    r = oc.occl64(img, maps, lay, L, g)
    for got, want in ((r.V, V), (r.A, A), (r.out, out)):
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
    assert bool((r.eV >= 0).all()) and bool((r.eA >= 0).all()) and bool((r.eOut >= 0).all())


def test_all_k_map_is_the_plain_render_with_map_k():
    g, ks, L, H, W = 3, 5, 4, 21, 26
    gen = torch.Generator().manual_seed(5)
    img = (torch.rand((2, 2, H, W), generator=gen) * 37.5 - 3.0).double()
    maps = oc.positive_maps(L, 2, g, ks, gen).double()
    for k in range(L):
        r = oc.occl64(img, maps, torch.full((2, H, W), k, dtype=torch.uint8), L, g, want_bound=False)
        q = oconv.render_psf_map(img, maps[k], g)
        a = oconv.render_psf_map(torch.ones_like(img), maps[k], g)
        assert torch.equal(r.V[:, :, 0], q) and torch.equal(r.A[:, :, 0], a)


def test_single_layer_with_a_hole_block_gives_zeros_where_the_window_sees_only_holes():
    c = oc.HOLE6
    img, maps, lay = oc.inputs(c)
    r = oc.occl64(img.double(), maps.double(), lay, 1, c.grid)
    p = c.ks // 2
    blind = torch.zeros((c.H, c.W), dtype=torch.bool)
    blind[11 + p:17 - p, 20 + p:26 - p] = True                                    # the 3 x 3 window lies inside the 6 x 6 hole
    assert int(blind.sum()) == 16
    A, out, V = r.A[0, 0, 0], r.out[0, 0, 0], r.V[0, 0, 0]
    assert torch.equal(A == 0, blind)
    assert bool((out[blind] == 0).all()) and bool((V[blind] == 0).all()) and bool((r.eOut[0, 0, 0][blind] == 0).all())
    assert bool((A[~blind] > 0).all())


def test_wrapper_checks_come_before_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    img, maps, lay = torch.zeros(2, 3, 16, 16), torch.zeros(4, 3, 6, 6), torch.zeros(2, 16, 16, dtype=torch.uint8)
    f = occlusion.render_psf_map_occluded_stack
    with pytest.raises(AssertionError, match=r"\[B, C, H, W\]"):
        f(img[0], maps, lay, 2, 2)
    with pytest.raises(AssertionError, match="L should be in 1..32"):
        f(img, maps, lay, 33, 2)
    with pytest.raises(AssertionError, match="L maps per slice"):
        f(img, maps, lay, 3, 2)
    with pytest.raises(AssertionError, match="divisible by grid"):
        f(img, torch.zeros(4, 3, 7, 7), lay, 2, 2)
    with pytest.raises(AssertionError, match="should be odd"):
        f(img, torch.zeros(4, 3, 8, 8), lay, 2, 2)
    with pytest.raises(AssertionError, match="should be in 3"):
        f(img, torch.zeros(4, 3, 2, 2), lay, 2, 2)
    with pytest.raises(AssertionError, match="same channel"):
        f(img[:, :2], maps, lay, 2, 2)
    with pytest.raises(AssertionError, match=r"layer should be \[B, H, W\]"):
        f(img, maps, lay[:1], 2, 2)
    with pytest.raises(AssertionError, match="uint8 or int64"):
        f(img, maps, lay.float(), 2, 2)
    with pytest.raises(AssertionError, match="in 0..255"):
        f(img, maps, lay.long() - 1, 2, 2)
    with pytest.raises(AssertionError, match="in 0..255"):
        f(img, maps, lay.long() + 256, 2, 2)
    with pytest.raises(AssertionError, match="PSF maps should be"):
        occlusion.render_psf_map_occluded(img, maps[0], lay, 2)
    for a, b in ((img.clone().requires_grad_(), maps), (img, maps.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="forward-only HIP op"):
            f(a, b, lay, 2, 2)
    # empty batch / empty stack: an empty result without a GPU
    assert f(img[:0], maps, lay[:0], 2, 2).shape == (0, 3, 2, 16, 16)
    out, cov = f(img, maps[:0], lay, 2, 2, return_coverage=True)
    assert out.shape == cov.shape == (2, 3, 0, 16, 16)
    # valid arguments: no CPU fallback
    with pytest.raises(RuntimeError, match="no HIP device"):
        f(img, maps, lay.long(), 2, 2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        occlusion.render_psf_map_occluded(img, maps, lay, 2)


def test_public_surface():
    import importlib
    rp = importlib.import_module("deeplens.render_psf")
    assert rp.render_psf_map_occluded is occlusion.render_psf_map_occluded
    assert rp.render_psf_map_occluded_stack is occlusion.render_psf_map_occluded_stack
    from aadff.focal_stack import render_focal_stack_m1_layered
    par = inspect.signature(render_focal_stack_m1_layered).parameters
    assert "occlusion" in par and par["occlusion"].default is False
    from deeplens.optics import Lensgroup
    par = inspect.signature(Lensgroup.render_occluded).parameters
    assert [par[k].default for k in ("layers", "grid", "ks")] == [8, 11, 11]
    assert occlusion.MAX_LAYERS == 32


def test_table_reaches_every_instantiation():
    assert {c.kernel for c in oc.TABLE} == oc.expected_instantiations()
    for c in oc.TABLE:
        _, maps, lay = oc.inputs(c)
        assert lay.dtype == torch.uint8 and tuple(lay.shape) == (c.B, c.H, c.W) and bool((maps > 0).all())
        on = lay[lay != oc.HOLE]
        assert int(on.max()) < c.L
    lay = oc.inputs(oc.TABLE[4])[2]
    assert oc.TABLE[4].L == 32 and bool((lay % 2 == 0).all()) and len(lay.unique()) == 16
    assert len(oc.inputs(oc.DISC)[2].unique()) >= 3
