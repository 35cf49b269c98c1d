"""CPU: the gradients of the occlusion-aware layered PSF-map render (aadff_render_psf_map_stack_occluded_bwd, csrc/conv_occl_bwd.hip;
aadff.diffrender.render_psf_map_occluded[_stack]) - the symbols and their binding, every argument error of the C entry before any HIP
call, the workspace query, the wrappers without a device, and the comparator, the indicator condition, the budget and the planted errors
of tests/occl_grad_common.py."""
import ctypes as C
import re
import subprocess

import pytest
import torch

import occl_grad_common as og
import occlusion_common as oc
from aadff import _abi
from aadff import diffrender
from aadff import occlusion

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
NAME = "aadff_render_psf_map_stack_occluded_bwd"
QUERY = "aadff_render_psf_map_stack_occluded_bwd_workspace"
IDS = [c.id for c in og.TABLE]


def _err(lib):
    return lib.aadff_last_error()


def test_symbols_are_declared_exported_and_bound(repo_root):
    lib = _abi.load_library()
    header = open(f"{repo_root}/include/aadff.h").read()
    assert f"int {NAME}(" in header and f"size_t {QUERY}(" in header
    assert NAME in _abi.PROTOTYPES and len(_abi.PROTOTYPES[NAME]) == 19 and getattr(lib, NAME).argtypes == _abi.PROTOTYPES[NAME]
    assert QUERY in _abi.SIZE_PROTOTYPES and len(_abi.SIZE_PROTOTYPES[QUERY]) == 9 and getattr(lib, QUERY).restype is C.c_size_t
    assert lib.aadff_abi_version() == _abi.ABI_VERSION == 9


def test_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    f = getattr(lib, NAME)
    big = C.c_size_t(1 << 40)

    def call(ptrs=(P8,) * 7, ws=P8, nbytes=big, B=1, Cn=3, S=1, L=2, H=64, W=64, grid=2, ks=3):
        return f(*ptrs, ws, nbytes, B, Cn, S, L, H, W, grid, ks, 1, None)

    for hole in range(3):                                                        # img, psf_maps, layer
        ptrs = [P8] * 7
        ptrs[hole] = None
        assert call(ptrs=ptrs) == -1 and b"NULL" in _err(lib)
    assert call(ptrs=(P8, P8, P8, None, None, P8, P8)) == -1 and b"d_out and d_cov are both NULL" in _err(lib)
    assert call(ptrs=(P8, P8, P8, P8, P8, None, None)) == -1 and b"d_img and d_maps are both NULL" in _err(lib)
    assert call(ks=4) == -1 and b"odd" in _err(lib)
    for ks in (1, 53, -1):
        assert call(ks=ks) == -1 and b"ks" in _err(lib) and b"outside [3,51]" in _err(lib)
    for L in (0, 33, -2):
        assert call(L=L) == -1 and b"layers outside [1,32]" in _err(lib)
    for grid in (0, 65):
        assert call(grid=grid) == -1 and b"grid" in _err(lib) and b"outside [1,64]" in _err(lib)
    assert call(H=5, W=64, grid=6) == -1 and b"grid 6 above min(H,W) = 5" in _err(lib)
    assert call(H=5, ks=11) == -1 and b"pad" in _err(lib)
    assert call(W=5, ks=11) == -1 and b"pad" in _err(lib)
    assert call(S=0) == -1 and b"empty" in _err(lib)
    assert call(B=0) == -1 and b"empty" in _err(lib)
    assert call(B=300, Cn=300) == -1 and b"too large" in _err(lib)
    assert call(Cn=1, H=65535 * 32) == -1 and b"too large" in _err(lib)
    # the workspace: at least one slice's worth, whatever S is; d_img alone needs less
    q = getattr(lib, QUERY)
    one, one_img = q(1, 3, 1, 2, 64, 64, 2, 3, 1), q(1, 3, 1, 2, 64, 64, 2, 3, 0)
    assert 0 < one_img < one
    assert call(S=4, nbytes=C.c_size_t(one - 4)) == -1 and b"workspace" in _err(lib) and b"too small" in _err(lib)
    assert call(ws=None, nbytes=C.c_size_t(one)) == -1 and b"workspace" in _err(lib)
    assert call(ptrs=(P8, P8, P8, P8, P8, P8, None), nbytes=C.c_size_t(one_img - 4)) == -1 and b"workspace" in _err(lib)


def test_workspace_is_monotone_and_matches_its_closed_form():
    lib = _abi.load_library()
    q = getattr(lib, QUERY)
    for c in og.TABLE:
        for need in (0, 1):
            assert q(c.B, c.C, c.S, c.L, c.H, c.W, c.grid, c.ks, need) == og.workspace_bytes(c, need_maps=bool(need)) > 0
            assert q(c.B, c.C, 1, c.L, c.H, c.W, c.grid, c.ks, need) * c.S == og.workspace_bytes(c, need_maps=bool(need))
    prev_b = prev_s = 0
    for n in range(1, 6):
        cur_b, cur_s = q(n, 3, 2, 4, 100, 90, 7, 11, 1), q(2, 3, n, 4, 100, 90, 7, 11, 1)
        assert cur_b > prev_b and cur_s > prev_s
        prev_b, prev_s = cur_b, cur_s
    assert q(1, 3, 1, 2, 64, 64, 2, 4, 1) == 0 and b"odd" in _err(lib)
    assert q(1, 3, 1, 2, 64, 64, 65, 3, 1) == 0 and b"grid" in _err(lib)
    assert q(1, 3, 1, 33, 64, 64, 2, 3, 1) == 0 and b"layers" in _err(lib)
    assert q(1, 3, 0, 2, 64, 64, 2, 3, 1) == 0 and b"empty" in _err(lib)


def test_wrappers_without_a_gpu(monkeypatch):
    img, maps, lay = torch.zeros(2, 3, 16, 16), torch.zeros(4, 3, 6, 6), torch.zeros(2, 16, 16, dtype=torch.uint8)
    f = diffrender.render_psf_map_occluded_stack
    # no grad: the forward-only functions themselves
    seen = []
    monkeypatch.setattr(occlusion, "render_psf_map_occluded_stack", lambda *a, **k: seen.append(a) or "delegated")
    assert f(img, maps, lay, 2, 2) == "delegated" and seen[-1][3:] == (2, 2, True, False)
    with torch.no_grad():
        assert f(img.clone().requires_grad_(), maps, lay, 2, 2, normalize=False, return_coverage=True) == "delegated"
        assert seen[-1][3:] == (2, 2, False, True)
    monkeypatch.undo()
    assert f(img[:0], maps, lay[:0], 2, 2).shape == (0, 3, 2, 16, 16)
    x = img.clone().requires_grad_()
    # the wrapper's assertions are the forward's
    with pytest.raises(AssertionError, match=r"\[B, C, H, W\]"):
        f(x[0], maps, lay, 2, 2)
    with pytest.raises(AssertionError, match="L should be in 1..32"):
        f(x, maps, lay, 33, 2)
    with pytest.raises(AssertionError, match="L maps per slice"):
        f(x, maps, lay, 3, 2)
    with pytest.raises(AssertionError, match="divisible by grid"):
        f(x, torch.zeros(4, 3, 7, 7), lay, 2, 2)
    with pytest.raises(AssertionError, match="should be odd"):
        f(x, torch.zeros(4, 3, 8, 8), lay, 2, 2)
    with pytest.raises(AssertionError, match="same channel"):
        f(x[:, :2], maps, lay, 2, 2)
    with pytest.raises(AssertionError, match=r"layer should be \[B, H, W\]"):
        f(x, maps, lay[:1], 2, 2)
    with pytest.raises(AssertionError, match="uint8 or int64"):
        f(x, maps, lay.float(), 2, 2)
    with pytest.raises(AssertionError, match="in 0..255"):
        f(x, maps, lay.long() - 1, 2, 2)
    with pytest.raises(AssertionError, match="PSF maps should be"):
        diffrender.render_psf_map_occluded(x, maps[0], lay, 2)
    # an empty batch and an empty stack stay in the graph, coverage included
    m = maps.clone().requires_grad_()
    out, cov = f(img[:0], m, lay[:0], 2, 2, return_coverage=True)
    assert out.shape == cov.shape == (0, 3, 2, 16, 16) and out.requires_grad and cov.requires_grad
    (out.sum() + cov.sum()).backward()
    assert m.grad is not None and not bool(m.grad.any())
    out = f(x, maps[:0], lay, 2, 2)
    assert out.shape == (2, 3, 0, 16, 16) and out.requires_grad
    out.sum().backward()
    assert x.grad is not None and not bool(x.grad.any())
    # no GPU: loud, and aadff.occlusion still refuses tensors that require grad
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    for a, b in ((img.clone().requires_grad_(), maps), (img, maps.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="no HIP device"):
            f(a, b, lay, 2, 2)
        with pytest.raises(RuntimeError, match="no HIP device"):
            diffrender.render_psf_map_occluded(a, b, lay.long(), 2)
        with pytest.raises(RuntimeError, match="forward-only HIP op"):
            occlusion.render_psf_map_occluded_stack(a, b, lay, 2, 2)


def test_table_reaches_every_instantiation():
    reached = set().union(*(og.kernels(c.ks) for c in og.TABLE))
    assert reached == og.expected_instantiations() and len(reached) == 14
    syms = subprocess.run(["nm", "-C", _abi.LIB_PATH], capture_output=True, text=True).stdout
    have = set(re.findall(r"(occl_grad_[a-z_]*kernel(?:<[^>]*>)?)\(", syms))
    assert have == reached, sorted(have ^ reached)
    assert not re.search(r"(conv_psf_map_|blend_d(img|maps)_)", "".join(have))
    assert [c.id for c in og.TABLE[:12]] == [c.id for c in oc.TABLE]
    assert any(c.H == c.ks // 2 + 1 and c.ks in og.TEMPLATED_KS for c in og.TABLE) and any(c.H == c.ks // 2 + 1 and c.ks not in og.TEMPLATED_KS for c in og.TABLE)
    assert og.WS_CASE.B == 2 and og.WS_CASE.S == 3 and og.CLAMP in og.TABLE
    for c in og.TABLE:
        img, maps, lay, g, h = og.case_inputs(c)
        assert bool((maps > 0).all()) and bool((g < 0).any()) and bool((g > 0).any()) and bool((h < 0).any()) and bool((h > 0).any())
        assert float(img.min()) >= -3.0 and float(img.max()) < 34.5


# ----------------------------------------------------------------------------------------------------------------- the comparator
@pytest.mark.parametrize("t", og.TINY, ids=[str(t) for t in og.TINY])
def test_comparator_is_the_literal_definition_and_the_closed_forms(t):
    B, Cn, S, L, H, W, grid, ks = t
    c = og.Case("tiny", B, Cn, S, L, H, W, grid, ks, "tiny", "")
    img, maps, lay, g, h = og.tiny_inputs(t)
    assert bool((lay >= L).any())
    V, A, out = og.occl_any(img.double(), maps.double(), lay, L, grid)
    r = oc.occl64(img, maps, lay, L, grid, want_bound=False)
    assert torch.equal(V, r.V) and torch.equal(A, r.A) and torch.equal(out, r.out)
    for normalize, with_h in og.COMBOS:
        hh = h if with_h else None
        gi, gm = og.autograd_ref(img, maps, lay, L, grid, g, hh, normalize)
        li, lm = og.loop64(img, maps, lay, L, grid, g, hh, normalize)
        for fast in (False, True):
            cl = og.closed64(c, img, maps, lay, g, hh, normalize, tap_by_tap=not fast)
            for got, want in ((li, gi), (lm, gm), (cl["d_img"], gi), (cl["d_maps"], gm)):
                assert float((got - want).abs().max()) <= 1e-12 * max(float(want.abs().max()), 1.0)
        hole = (lay >= L)[:, None].expand_as(img)
        assert bool((gi[hole] == 0).all())                                          # exactly 0 on a hole texel


def test_adjoint_identity_without_normalisation():
    for c in (og.TABLE[0], og.WS_CASE):
        img, maps, lay, g, _ = og.case_inputs(c)
        gi, _ = og.autograd_ref(img, maps, lay, c.L, c.grid, g, None, 0)
        V = oc.occl64(img, maps, lay, c.L, c.grid, want_bound=False).V
        lhs, rhs = float((g.double() * V).sum()), float((gi * img.double()).sum())
        assert abs(lhs - rhs) <= 1e-11 * float((g.double() * V).abs().sum())


# ------------------------------------------------------------------------------------------------------------- the discontinuity
@pytest.mark.parametrize("c", og.TABLE, ids=IDS)
def test_indicator_condition(c):
    margin = og.indicator_margin(c, og.case_parts(c))
    print(f"\n{c.id}: min |1 - a_l| / (16 ((ks^2 + 1) U a_l + U)) where anything lies behind = {margin:.1f}")
    assert margin >= 1.0


def test_clamp_case_makes_the_clamp_bite():
    c = og.CLAMP
    img, maps, lay, g, h = og.case_inputs(c)
    parts = og.case_parts(c)
    a0, a1 = parts.a[0][0], parts.a[0][1]
    bites = (a0 > 1) & (a1 > 0)
    share = float(bites.double().mean())
    print(f"\nclamp case: {100 * share:.1f} % of the pixels have a_0 > 1 with layer 1 in the window; min |1 - a_0| = {float((1 - a0).abs().min()):.3f}")
    assert share >= 0.05
    # there beta_0 = gA T_0 = gA with no R term: with g = 0 and normalize = 0, gA = h
    al, be, _, _ = og.alpha_beta(c, parts, torch.zeros_like(g), h, 0)
    assert torch.equal(be[:, :, 0, 0][bites], h[:, :, 0].double()[bites])
    assert bool((be[:, :, 0, 0][~bites & (a1 > 0)] != h[:, :, 0].double()[~bites & (a1 > 0)]).any())
    # and dropping the indicator changes the reference there
    dropped = og.alpha_beta(c, parts, g, h, 1, "the indicator dropped")[1]
    kept = og.alpha_beta(c, parts, g, h, 1)[1]
    assert bool((dropped[:, :, 0, 0][bites] != kept[:, :, 0, 0][bites]).all())


# --------------------------------------------------------------------------------------------------------------------- the budget
@pytest.mark.parametrize("c", og.TABLE, ids=IDS)
def test_stage_one_in_float32_stays_inside_its_running_bounds(c):
    img, maps, lay, g, h = og.case_inputs(c)
    for normalize in (1, 0):
        al, be, eal, ebe = og.alpha_beta(c, og.case_parts(c), g, h, normalize)
        al32, be32 = og.tree32_stage1(c, img, maps, lay, g, h, normalize)
        for name, got, ref, bound in (("alpha", al32, al, eal), ("beta", be32, be, ebe)):
            use, worst = og.compare(torch.from_numpy(got), ref, bound)
            print(f"\n{c.id} normalize={normalize}: float32 {name} planes use {use:.3f} of their running bound")
            assert use <= 1.0, (c.id, name, worst)


@pytest.mark.parametrize("c", og.TABLE, ids=IDS)
def test_budget_holds_float32_sums_and_rejects_planted_errors(c):
    img, maps, lay, g, h = og.case_inputs(c)
    parts = og.case_parts(c)
    r = og.reference(c, 1, True)
    assert bool((r.bi >= 0).all()) and bool((r.bm >= 0).all())
    # the closed forms are the comparator; the reference rounded to float32 and torch's own float32 autograd are inside the budget
    assert og.rel_l2(r.ci, r.gi) <= 1e-12 and og.rel_l2(r.cm, r.gm) <= 1e-12
    gi32, gm32 = og.autograd_ref(img, maps, lay, c.L, c.grid, g, h, 1, torch.float32)
    for name, ref, bound, f32 in (("d_img", r.gi, r.bi, gi32), ("d_maps", r.gm, r.bm, gm32)):
        clean, _ = og.compare(ref.float(), ref, bound)
        assert clean <= 1.0, (c.id, name, clean)
        print(f"\n{c.id} {name}: the rounded reference uses {clean:.3f} of the budget, torch float32 autograd {og.compare(f32, ref, bound)[0]:.3f}")
    # the kernels' summation order restated in numpy float32, all three stages chained
    al32, be32 = og.tree32_stage1(c, img, maps, lay, g, h, 1)
    t32 = {"d_img": og.tree32_dimg(c, maps, lay, al32), "d_maps": og.tree32_dmaps(c, img, lay, al32, be32)}
    for name, ref, bound in (("d_img", r.gi, r.bi), ("d_maps", r.gm, r.bm)):
        use, worst = og.compare(t32[name], ref, bound)
        print(f"{c.id} {name}: the float32 restatement of the kernels' order uses {use:.3f} of the budget; rel_l2 {og.rel_l2(t32[name], ref):.2e}")
        assert t32[name].dtype == torch.float32 and use <= 1.0, (c.id, name, worst)
    # every planted error is outside it
    ref = {"d_img": r.gi, "d_maps": r.gm}
    bound = {"d_img": r.bi, "d_maps": r.bm}
    for plant in og.PLANTS:
        if not og.plant_changes_a_term(c, plant, lay):
            continue
        for name, wrong in og.closed64(c, img, maps, lay, g, h, 1, plant, parts).items():
            use, _ = og.compare(wrong.float(), ref[name], bound[name])
            print(f"{c.id}: {plant} ({name}): {use:.1f} x the budget")
            assert use > 1.0, (c.id, plant, name)


def test_fast_linear_maps_are_the_tap_by_tap_ones():
    c = og.TABLE[0]
    img, maps, lay, g, h = og.case_inputs(c)
    a = og.closed64(c, img, maps, lay, g, h, 1)
    b = og.closed64(c, img, maps, lay, g, h, 1, tap_by_tap=True)
    for k in a:
        assert float((a[k] - b[k]).abs().max()) <= 1e-12 * float(b[k].abs().max())
    for plant in ("one tap dropped", "the unflipped PSF", "one slice missing", "one batch item missing"):
        a, b = og.closed64(c, img, maps, lay, g, h, 1, plant), og.closed64(c, img, maps, lay, g, h, 1, plant, tap_by_tap=True)
        for k in a:
            assert float((a[k] - b[k]).abs().max()) <= 1e-12 * float(b[k].abs().max()), (plant, k)
