"""CPU: the soft-depth-layer occluded PSF-map render (aadff_render_psf_map_stack_soft_occluded, csrc/conv_occl_soft.hip;
aadff/occlusion.py) - the symbol and its binding, every argument error of the C entry before any HIP call, the wrappers' checks before a
device is needed, the float64 comparator of tests/soft_occl_common.py against a literal restatement and against the hard comparator at
integral coordinates, a float32 restatement of the kernel's order inside the budget with planted errors outside it, and the coordinate
helpers `layer_coordinate` / `depth_nodes`."""
import ctypes as C
import inspect

import pytest
import torch

import occlusion_common as oc
import soft_occl_common as sc
from aadff import _abi
from aadff import occlusion

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
NAME = "aadff_render_psf_map_stack_soft_occluded"


def _err(lib):
    return lib.aadff_last_error()


def test_symbol_is_exported_and_bound():
    lib = _abi.load_library()
    assert NAME in _abi.PROTOTYPES and _abi.PROTOTYPES[NAME] == _abi.PROTOTYPES["aadff_render_psf_map_stack_occluded"]
    assert getattr(lib, NAME).argtypes == _abi.PROTOTYPES[NAME]
    assert lib.aadff_abi_version() == _abi.ABI_VERSION == 9


def test_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = getattr(lib, NAME)

    def call(B=1, Cn=3, S=1, L=2, H=64, W=64, grid=2, ks=3, ptrs=(P8, P8, P8, P8, None)):
        return f(*ptrs, B, Cn, S, L, H, W, grid, ks, 1, None)

    for hole in range(4):                                                        # every required pointer (pos is one); coverage may be NULL
        ptrs = [P8, P8, P8, P8, P8]
        ptrs[hole] = None
        assert call(ptrs=ptrs) == -1 and b"NULL" in _err(lib) and b"soft_occluded" in _err(lib)
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


# ----------------------------------------------------------------------------------------------------------------- the comparator
TINY = [(1, 2, 2, 3, 7, 9, 3, 3), (2, 1, 1, 2, 6, 5, 2, 3), (1, 1, 1, 1, 5, 6, 1, 3)]     # B, C, S, L, H, W, grid, ks


def _tiny(t):
    B, Cn, S, L, H, W, g, ks = t
    gen = torch.Generator().manual_seed(sum(t))
    img = torch.rand((B, Cn, H, W), generator=gen) * 37.5 - 3.0
    maps = oc.positive_maps(S * L, Cn, g, ks, gen)
    pos = torch.rand((B, H, W), generator=gen) * (L + 0.5) - 0.25               # below 0: holes; above L - 1: clamped
    pos[0, 0, 0], pos[0, 1, 1], pos[0, 2, 2] = float("nan"), float(L - 1), 0.0
    return img, maps, pos, L, g


@pytest.mark.parametrize("t", TINY, ids=[str(t) for t in TINY])
def test_comparator_is_the_literal_definition(t):
    img, maps, pos, L, g = _tiny(t)
    V, A, out = sc.loop64(img, maps, pos, L, g)
    r = sc.soft64(img, maps, pos, L, g)
    for got, want in ((r.V, V), (r.A, A), (r.out, out)):
        assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
    assert bool((r.eV >= 0).all()) and bool((r.eA >= 0).all()) and bool((r.eOut >= 0).all())


@pytest.mark.parametrize("c", sc.HARD[:6], ids=[c.id for c in sc.HARD[:6]])
def test_comparator_at_integral_coordinates_is_the_hard_comparator(c):
    img, maps, layer = oc.inputs(c)
    pos = layer.float()
    pos[layer >= c.L] = float("nan")
    r, h = sc.soft64(img, maps, pos, c.L, c.grid), oc.occl64(img, maps, layer, c.L, c.grid)
    assert torch.equal(r.V, h.V) and torch.equal(r.A, h.A) and torch.equal(r.out, h.out)
    assert bool((r.eV >= h.eV).all()) and bool((r.eA >= h.eA).all())             # the soft budget holds the hard one plus the new roundings
    n = c.ks * c.ks                                                              # ... and little more: (n + 4) U against (n + 1) U per chain
    assert bool((r.eV <= (n + 5) / (n + 1) * h.eV).all()) and bool((r.eA <= (n + 5) / (n + 1) * h.eA).all())


def test_decode_follows_the_contract_on_edge_values():
    L = 3
    k, f = sc.decode(sc.edge_values(L), L)
    t = 2.0 ** -24
    assert k.tolist() == [2, 2, 2, 2, 0, 0, 0, 0, 0, 1, 1, 1, 0, 0, -1, -1, 0, 1]
    assert f.tolist() == [0, 0, 0, 0, t, 2 * t, 3 * t, 5 * t, 1 - t, 0, 2 * t, 1 - 2 * t, 0, 0, 0, 0, 0.5, 0.25]
    assert bool((1 - f[k >= 0] >= t).all())                                      # fl(1 - f) never reaches 0: A > 0 stays an exact decision


def test_hole_windows_are_the_zeros_of_A_exactly():
    c = sc.HOLE6
    img, maps, pos, r = sc.reference(c)
    p = c.ks // 2
    blind = torch.zeros((c.H, c.W), dtype=torch.bool)
    blind[11 + p:17 - p, 20 + p:26 - p] = True
    assert torch.equal(r.A[0, 0, 0] == 0, blind) and bool((r.out[0, 0, 0][blind] == 0).all()) and bool((r.eOut[0, 0, 0][blind] == 0).all())
    # L = 1: every pos >= 0 is the hard L = 1 render
    h = oc.occl64(img, maps, oc.inputs(oc.HOLE6)[2], 1, c.grid)
    assert bool((pos[pos >= 0] > 0).any()) and torch.equal(r.V, h.V) and torch.equal(r.A, h.A)


# ------------------------------------------------------------------------------------------- the kernel's order, in float32 on the CPU
@pytest.mark.parametrize("c", sc.TABLE, ids=[c.id for c in sc.TABLE])
def test_float32_restatement_of_the_kernel_order_is_inside_the_budget(c):
    img, maps, pos, r = sc.reference(c)
    V, A, out = sc.restate32(img, maps, pos, c.L, c.grid)
    assert torch.equal(A == 0, r.A == 0), "A > 0 is an exact decision"
    for what, got, want, budget in (("V", V, r.V, r.eV), ("coverage", A, r.A, r.eA), ("out", out, r.out, r.eOut)):
        use, worst = sc.share(got, want, budget)
        assert use <= 1.0, f"{c.id}: {what} element {worst} is {use:.2f} x its budget"


def _caught(c, plant, img=None, pos=None):
    """The largest share of the budget a planted error uses over V, coverage and out (inf for a non-finite result)."""
    i0, maps, p0, _ = sc.reference(c)
    img, pos = i0 if img is None else img, p0 if pos is None else pos
    r = sc.soft64(torch.nan_to_num(img), maps, pos, c.L, c.grid) if (img is not i0 or pos is not p0) else sc.reference(c)[3]
    worst = 0.0
    for got, want, budget in zip(sc.restate32(img, maps, pos, c.L, c.grid, plant), (r.V, r.A, r.out), (r.eV, r.eA, r.eOut)):
        worst = max(worst, sc.share(got, want, budget)[0] if bool(torch.isfinite(got).all()) else float("inf"))
    return worst


def test_planted_errors_exceed_the_budget():
    c = sc.TABLE[0]                                                              # 2 x 3 x 1 x 3, ks 5, random coordinates plus a NaN hole
    assert _caught(c, None) <= 1.0
    for plant in ("swap", "node", "round", "noflip", "batch"):
        assert _caught(c, plant) > 1.0, plant
    # the product instead of the select, on a NaN image value under a hole: the select hides it, the product does not
    img, _, pos, _ = sc.reference(c)
    bad = img.clone()
    bad[:, :, torch.isnan(pos[0])] = float("nan")
    assert int(torch.isnan(bad).sum()) == 2 * 3 * 4
    assert _caught(c, None, img=bad) <= 1.0 and _caught(c, "product", img=bad) > 1.0
    # the clamp at L - 1 missing: coordinates above L - 1
    assert _caught(sc.HOLE6, None) <= 1.0 and _caught(sc.HOLE6, "noclamp") > 1.0
    assert _caught(sc.EDGES, "noclamp", pos=torch.nan_to_num(sc.reference(sc.EDGES)[2], nan=-1.0, posinf=7.0).clamp(max=7.0)) > 1.0
    # a wrong slice (one of the two is scaled by 1e-3)
    assert _caught(sc.TABLE[1], "slice") > 1.0


def test_table_reaches_every_instantiation_and_every_scene():
    assert {c.kernel for c in sc.TABLE} == sc.expected_instantiations() and len(sc.TABLE) == 13 and len(sc.HARD) == 12
    for c in sc.TABLE:
        img, maps, pos = sc.inputs(c)
        assert pos.dtype == torch.float32 and tuple(pos.shape) == (c.B, c.H, c.W) and bool((maps > 0).all())
        hi, mi, _ = oc.inputs(c._replace(scene="random"))
        assert torch.equal(img, hi) and torch.equal(maps, mi)
    k, f = sc.decode(sc.inputs(sc.TABLE[4])[2], 32)
    assert bool((k % 2 == 0).all()) and len(k.unique()) == 16 and bool((f > 0).any())        # L = 32 with only some slabs occupied
    k, f = sc.decode(sc.inputs(sc.DISC)[2], sc.DISC.L)
    assert sorted(k.unique().tolist()) == list(range(sc.DISC.L)) and bool(((f > 0) & (f < 1)).any())   # the slant crosses every slab
    pos = sc.inputs(sc.EDGES)[2]
    assert int(torch.isnan(pos).sum()) > 0 and int((pos == -1).sum()) > 0 and int((pos > 2).sum()) > 0
    assert int(torch.isnan(sc.inputs(sc.TABLE[0])[2]).sum()) == 2 * 4


# --------------------------------------------------------------------------------------------------------------------- the wrappers
def test_wrapper_checks_come_before_the_device(monkeypatch):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    img, maps, pos = torch.zeros(2, 3, 16, 16), torch.zeros(4, 3, 6, 6), torch.zeros(2, 16, 16)
    f = occlusion.render_psf_map_soft_occluded_stack
    with pytest.raises(AssertionError, match=r"\[B, C, H, W\]"):
        f(img[0], maps, pos, 2, 2)
    with pytest.raises(AssertionError, match="L should be in 1..32"):
        f(img, maps, pos, 33, 2)
    with pytest.raises(AssertionError, match="L should be in 1..32"):
        f(img, maps, pos, 0, 2)
    with pytest.raises(AssertionError, match="L maps per slice"):
        f(img, maps, pos, 3, 2)
    with pytest.raises(AssertionError, match="divisible by grid"):
        f(img, torch.zeros(4, 3, 7, 7), pos, 2, 2)
    with pytest.raises(AssertionError, match="should be odd"):
        f(img, torch.zeros(4, 3, 8, 8), pos, 2, 2)
    with pytest.raises(AssertionError, match="should be in 3"):
        f(img, torch.zeros(4, 3, 2, 2), pos, 2, 2)
    with pytest.raises(AssertionError, match="same channel"):
        f(img[:, :2], maps, pos, 2, 2)
    with pytest.raises(AssertionError, match=r"pos should be \[B, H, W\]"):
        f(img, maps, pos[:1], 2, 2)
    with pytest.raises(AssertionError, match=r"pos should be \[B, H, W\]"):
        f(img, maps, pos[:, None], 2, 2)
    for wrong in (pos.long(), pos.to(torch.uint8)):
        with pytest.raises(AssertionError, match="pos should be a float tensor"):
            f(img, maps, wrong, 2, 2)
    with pytest.raises(AssertionError, match="PSF maps should be"):
        occlusion.render_psf_map_soft_occluded(img, maps[0], pos, 2)
    for a, b, p in ((img.clone().requires_grad_(), maps, pos), (img, maps.clone().requires_grad_(), pos), (img, maps, pos.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="forward-only HIP op, its backward is not built"):
            f(a, b, p, 2, 2)
    # empty batch / empty stack: an empty result without a GPU
    assert f(img[:0], maps, pos[:0], 2, 2).shape == (0, 3, 2, 16, 16)
    out, cov = f(img, maps[:0], pos, 2, 2, return_coverage=True)
    assert out.shape == cov.shape == (2, 3, 0, 16, 16)
    # valid arguments (float64 coordinates too): no CPU fallback
    with pytest.raises(RuntimeError, match="no HIP device"):
        f(img, maps, pos.double(), 2, 2)
    with pytest.raises(RuntimeError, match="no HIP device"):
        occlusion.render_psf_map_soft_occluded(img, maps, pos, 2)


def test_public_surface():
    import importlib
    rp = importlib.import_module("deeplens.render_psf")
    assert rp.render_psf_map_soft_occluded is occlusion.render_psf_map_soft_occluded
    assert rp.render_psf_map_soft_occluded_stack is occlusion.render_psf_map_soft_occluded_stack
    from deeplens.optics import Lensgroup
    par = inspect.signature(Lensgroup.render_occluded).parameters
    assert par["soft"].default is False and [par[k].default for k in ("layers", "grid", "ks")] == [8, 11, 11]
    par = inspect.signature(occlusion.render_psf_map_soft_occluded).parameters
    assert list(par) == ["img", "maps", "pos", "grid", "normalize", "return_coverage"]
    par = inspect.signature(occlusion.render_psf_map_soft_occluded_stack).parameters
    assert list(par) == ["img", "maps", "pos", "L", "grid", "normalize", "return_coverage"]


def test_stack_renderer_occlusion_argument(monkeypatch):
    """As far as it runs without a GPU: the values of `occlusion` and the layer limit are checked before the lens or a device is touched."""
    from aadff.focal_stack import render_focal_stack_m1_layered

    class NoLens:
        sensor_res = (8, 8)

        def _gpu(self):
            raise RuntimeError("reached the device")

    img, depth = torch.zeros(1, 3, 8, 8), -torch.ones(1, 1, 8, 8)
    for bad in ("hard", "Soft", 2, None):
        with pytest.raises(AssertionError, match="occlusion should be False, True or 'soft'"):
            render_focal_stack_m1_layered(NoLens(), img, depth, [-1000.0], occlusion=bad)
    for occl in (True, "soft"):
        with pytest.raises(AssertionError, match="at most 32 depth layers"):
            render_focal_stack_m1_layered(NoLens(), img, depth, [-1000.0], layers=33, occlusion=occl)
    for occl in (False, True, "soft"):                                           # accepted: the next thing it asks for is the device
        with pytest.raises(RuntimeError, match="reached the device"):
            render_focal_stack_m1_layered(NoLens(), img, depth, [-1000.0], layers=4, occlusion=occl)


# ------------------------------------------------------------------------------------------------------------ the layer coordinate
def _coordinate_loop(depth, centres):
    """float64, element by element: the segment of the node table that holds the depth, linear inside it, clamped outside."""
    L, out = len(centres), []
    for z in depth:
        if not z < 0:
            out.append(float(L - 1))
            continue
        d, c = -z, [-v for v in centres]
        if L == 1 or d <= c[0]:
            out.append(0.0)
        elif d >= c[-1]:
            out.append(float(L - 1))
        else:
            k = max(i for i in range(L - 1) if c[i] <= d)
            out.append(k + (d - c[k]) / (c[k + 1] - c[k]))
    return out


def test_layer_coordinate_against_a_float64_loop():
    gen = torch.Generator().manual_seed(11)
    centres = torch.tensor([-400.0, -650.0, -700.0, -1500.0, -4000.0], dtype=torch.float64)     # non-uniform, nearest first
    depth = -(torch.rand(400, generator=gen, dtype=torch.float64) * 4500.0 + 100.0)
    depth[:8] = torch.tensor([0.0, 5.0, float("nan"), -400.0, -700.0, -4000.0, -399.0, -1e6], dtype=torch.float64)
    got = occlusion.layer_coordinate(depth, centres)
    want = torch.tensor(_coordinate_loop(depth.tolist(), centres.tolist()), dtype=torch.float64)
    assert got.dtype == torch.float64 and got.shape == depth.shape and float((got - want).abs().max()) <= 1e-12
    assert got[:8].tolist() == [4.0, 4.0, 4.0, 0.0, 2.0, 4.0, 0.0, 4.0]          # invalid -> L - 1; a depth at node l -> l; clamped outside
    assert float(got.min()) >= 0.0 and float(got.max()) <= 4.0
    one = occlusion.layer_coordinate(depth.reshape(2, 1, 10, 20), centres[:1])   # a single node: 0, invalid depths L - 1 = 0 too
    assert one.shape == (2, 1, 10, 20) and bool((one == 0).all())
    assert occlusion.layer_coordinate(depth.float(), centres.tolist()).dtype == torch.float32
    for bad in ([-400.0, -400.0], [-700.0, -400.0], [-400.0, 10.0], []):
        with pytest.raises(AssertionError, match="centres should"):
            occlusion.layer_coordinate(depth, torch.tensor(bad, dtype=torch.float64))


def test_depth_nodes_against_a_float64_loop():
    gen = torch.Generator().manual_seed(12)
    depth = -(torch.rand((2, 1, 9, 11), generator=gen, dtype=torch.float64) * 3000.0 + 500.0)
    depth[0, 0, 0, :3] = 0.0                                                     # invalid
    valid = depth[depth < 0]
    near, far = float(-valid.max()), float(-valid.min())
    for L in (1, 2, 5, 32):
        pos, centres = occlusion.depth_nodes(depth, L)
        assert pos.shape == depth.shape and centres.shape == (L,) and pos.dtype == torch.float64
        if L == 1:
            assert abs(float(centres[0]) + 0.5 * (near + far)) <= 1e-9 and bool((pos == 0).all())
            continue
        want_c = [-(near + i * (far - near) / (L - 1)) for i in range(L)]
        assert float((centres - torch.tensor(want_c, dtype=torch.float64)).abs().max()) <= 1e-9
        want = torch.tensor(_coordinate_loop(depth.flatten().tolist(), centres.tolist()), dtype=torch.float64).reshape(depth.shape)
        assert float((pos - want).abs().max()) <= 1e-10
        assert bool((pos[0, 0, 0, :3] == L - 1).all()) and float(pos.min()) == 0.0 and float(pos.max()) == L - 1
        assert float((pos - occlusion.layer_coordinate(depth, centres)).abs().max()) <= 1e-12
    flat = torch.full((1, 1, 4, 4), -800.0)                                      # one depth only: distinct nodes all the same
    pos, centres = occlusion.depth_nodes(flat, 3)
    assert bool((pos == 0).all()) and bool((centres[1:] < centres[:-1]).all())


def test_layer_coordinate_gradients():
    gen = torch.Generator().manual_seed(13)
    centres = torch.tensor([-400.0, -650.0, -700.0, -1500.0], dtype=torch.float64, requires_grad=True)
    # depths strictly inside segments (the function has kinks at the nodes), one in front of node 0 and one behind the last
    depth = torch.tensor([-450.0, -600.0, -660.0, -690.0, -900.0, -1400.0, -300.0, -2000.0], dtype=torch.float64, requires_grad=True)
    assert torch.autograd.gradcheck(occlusion.layer_coordinate, (depth, centres), eps=1e-6, atol=1e-7)
    g, = torch.autograd.grad(occlusion.layer_coordinate(depth, centres.detach()).sum(), depth)
    assert g.tolist()[-2:] == [0.0, 0.0] and abs(float(g[0]) + 1.0 / 250.0) <= 1e-15          # clamped: no gradient; inside: -1 / spacing
    d2 = (-(torch.rand((1, 1, 5, 6), generator=gen, dtype=torch.float64) * 2000.0 + 500.0)).requires_grad_()
    lo, hi = int(d2.argmax()), int(d2.argmin())                                  # the extreme depths define the nodes: kinks, left out
    keep = torch.ones(30, dtype=torch.float64)
    keep[lo] = keep[hi] = 0.0
    assert torch.autograd.gradcheck(lambda d: occlusion.depth_nodes(d, 4)[0].flatten() * keep, (d2,), eps=1e-6, atol=1e-7)
