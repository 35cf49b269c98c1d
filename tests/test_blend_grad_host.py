"""CPU: the gradients of the blended PSF-map render (aadff_render_psf_map_blend_stack_bwd, csrc/conv_blend_bwd.hip;
aadff.diffrender.render_psf_map_blend[_stack]) - the comparator of tests/blend_grad_common.py against the loop definition and the closed
forms, the kernels' summation trees (restated in numpy float32) inside the budget, every planted error outside it, the case table
against the library's symbol table, the workspace function, every argument error of the C entry before any HIP call, and the
wrapper without a GPU."""
import ctypes as C
import re
import subprocess

import pytest
import torch

import blend_common as bc
import blend_grad_common as bg
from aadff import _abi
from aadff import blend
from aadff import diffrender

P8 = C.c_void_p(8)          # a non-NULL pointer that is never dereferenced: validation comes first
IDS = [c.id for c in bg.TABLE]


def _err(lib):
    return lib.aadff_last_error()


def _host(values):
    return (C.c_float * len(values))(*values)


@pytest.mark.parametrize("t", bg.TINY, ids=[str(t) for t in bg.TINY])
def test_comparator_is_the_loop_definition_and_the_closed_forms(t):
    img, maps, dy, g, ny, nx = bg.tiny_inputs(t)
    gi, gm = bg.autograd64(img, maps, dy, g, ny, nx)
    li, lm = bg.loop64(img, maps, dy, g, ny, nx)
    d = bg.def64(img, maps, dy, g, bg.hats64(ny, img.shape[2])[0], bg.hats64(nx, img.shape[3])[0])
    for got in ((li, lm), (d["d_img"], d["d_maps"])):
        assert float((got[0] - gi).abs().max()) <= 1e-12 * float(gi.abs().max())
        assert float((got[1] - gm).abs().max()) <= 1e-12 * float(gm.abs().max())
    # the adjoint identity of a map that is linear in each input: <dy, out> = <d_img, img> = <d_maps, maps>
    out = bc.blend64(img, maps, g, ny, nx, want_bound=False).out64
    lhs = float((dy.double() * out).sum())
    assert abs(float((gi * img.double()).sum()) - lhs) <= 1e-12 * abs(lhs) and abs(float((gm * maps.double()).sum()) - lhs) <= 1e-12 * abs(lhs)


@pytest.mark.parametrize("c", bg.TABLE, ids=IDS)
def test_closed_forms_trees_and_planted_errors(c):
    r = bg.reference(c)
    bound = bg.bounds(r)
    ref = {"d_img": r.gi, "d_maps": r.gm}
    d = bg.def64(r.img, r.maps, r.dy, c.grid, r.Hy, r.Hx)
    for name in ref:
        assert float((d[name] - ref[name]).abs().max()) <= 1e-12 * float(ref[name].abs().max()), name
        assert bool((bound[name] >= 0).all()) and bool((ref[name].abs() <= (r.Ai if name == "d_img" else r.Am) * (1 + 1e-12)).all())
    # the kernels' own summation order, in float32, is inside the budget on every element
    tree = {"d_img": bg.dimg_tree32(c, r.maps, r.dy, r.ny, r.nx), "d_maps": bg.dmaps_tree32(c, r.img, r.dy, r.ny, r.nx)}
    for name in ref:
        use, worst, rel = bg.compare(tree[name], ref[name], bound[name])
        print(f"{c.id}: {name} tree restatement uses {use:.3f} of the budget, rel_l2 {rel:.2e}")
        assert use <= 1.0, (c.id, name, worst)
    # every planted error is outside it
    for plant in bg.PLANTS:
        if not bg.plant_changes_a_term(c, plant):
            continue
        for name, wrong in bg.planted(c, r, plant).items():
            assert float((wrong - ref[name]).abs().max()) > 0, (c.id, plant, name)
            use, _, _ = bg.compare(wrong.float(), ref[name], bound[name])
            clean, _, _ = bg.compare(ref[name].float(), ref[name], bound[name])
            print(f"{c.id}: {plant} ({name}): {use:.1f} x the budget (the rounded reference itself: {clean:.3f})")
            assert use > 1.0 and clean <= 1.0, (c.id, plant, name)


def test_unsupported_nodes_are_zero_in_the_reference():
    c = next(c for c in bg.TABLE if c.grid == 64)
    r = bg.reference(c)
    tiles = r.gm.reshape(c.S, c.C, c.grid, c.ks, c.grid, c.ks).abs().amax((0, 1, 3, 5))
    assert int((tiles == 0).sum()) > 3000 and int((tiles > 0).sum()) > 0           # 33 x 5 pixels under 64 x 64 nodes


def test_table_reaches_every_instantiation():
    reached = set().union(*(bg.kernels(c.ks) for c in bg.TABLE))
    assert reached == bg.expected_instantiations() and len(reached) == 19
    syms = subprocess.run(["nm", "-C", _abi.LIB_PATH], capture_output=True, text=True).stdout
    have = set(re.findall(r"(blend_d(?:img|maps)_[a-z_]*kernel(?:<[^>]*>)?)\(", syms))
    assert have == reached, sorted(have ^ reached)
    by = {c.reaches: c for c in bg.TABLE}
    assert any(c.H == c.ks // 2 + 1 and c.ks in bg.TEMPLATED_KS for c in bg.TABLE) and any(c.H == c.ks // 2 + 1 and c.ks not in bg.TEMPLATED_KS for c in bg.TABLE)
    assert any(c.B == 2 and c.S == 2 for c in bg.TABLE) and len(by) >= len(bg.TABLE) - 3
    narrow = next(c for c in bg.TABLE if "3 x 3 nodes" in c.reaches)
    sy = bg.hats64(bg.nodes_of(narrow)[0], narrow.H)[1]
    p = narrow.ks // 2
    assert max((sy[:, max(q - p, 0):q + p + 1].sum(1) > 0).sum() for q in range(narrow.H)) >= 3


def test_workspace_is_monotone_and_matches_its_closed_form():
    lib = _abi.load_library()
    f = lib.aadff_render_psf_map_blend_stack_bwd_workspace
    assert f.restype is C.c_size_t
    for c in bg.TABLE:
        assert f(c.B, c.C, c.S, c.H, c.W, c.grid, c.ks) == bg.workspace_bytes(c) > 0
        # the bound holds for the case's nodes: the tiles the kernels enumerate fit
        ny, nx = bg.nodes_of(c)
        nty, ntx = bg.tiles_of(ny, c.H)[1][-1], bg.tiles_of(nx, c.W)[1][-1]
        assert c.B * nty * ntx * c.S * c.C * 4 * c.ks * c.ks * 4 <= bg.workspace_bytes(c)
    prev = 0
    for n in range(1, 6):
        cur = f(n, 3, 2, 100, 90, 7, 11)
        assert cur > prev and f(2, 3, n, 100, 90, 7, 11) == f(n, 3, 2, 100, 90, 7, 11)
        prev = cur
    assert f(1, 3, 1, 64, 64, 2, 4) == 0 and b"odd" in _err(lib)
    assert f(1, 3, 1, 64, 64, 65, 3) == 0 and b"grid" in _err(lib)


def test_argument_errors_need_no_gpu():
    lib = _abi.load_library()
    name = "aadff_render_psf_map_blend_stack_bwd"
    assert name in _abi.PROTOTYPES and len(_abi.PROTOTYPES[name]) == 17 and lib.aadff_render_psf_map_blend_stack_bwd.argtypes == _abi.PROTOTYPES[name]
    assert lib.aadff_abi_version() == _abi.ABI_VERSION == 9
    f = lib.aadff_render_psf_map_blend_stack_bwd
    n2, n3 = _host([0.0, 63.0]), _host([0.0, 31.5, 63.0])
    big = C.c_size_t(1 << 40)

    def call(img=P8, maps=P8, dy=P8, d_img=P8, d_maps=P8, ws=P8, nbytes=big, ny=n2, nx=n2, shape=(1, 3, 1, 64, 64, 2, 3)):
        return f(img, maps, dy, d_img, d_maps, ws, nbytes, ny, nx, *shape, None)

    for hole in ("img", "maps", "dy", "ny", "nx"):
        assert call(**{hole: None}) == -1 and b"NULL" in _err(lib), hole
    assert call(d_img=None, d_maps=None) == -1 and b"both NULL" in _err(lib)
    assert call(shape=(1, 3, 1, 64, 64, 2, 4)) == -1 and b"odd" in _err(lib)
    assert call(shape=(1, 3, 1, 64, 64, 2, 53)) == -1 and b"ks" in _err(lib)
    assert call(shape=(1, 3, 1, 64, 64, 65, 3)) == -1 and b"grid" in _err(lib)
    assert call(shape=(1, 3, 1, 5, 64, 2, 11)) == -1 and b"pad" in _err(lib)
    assert call(shape=(1, 3, 0, 64, 64, 2, 3)) == -1 and b"empty" in _err(lib)
    assert call(shape=(300, 300, 1, 64, 64, 2, 3)) == -1 and b"too large" in _err(lib)
    assert call(ny=_host([0.0, float("nan"), 63.0]), nx=n3, shape=(1, 3, 1, 64, 64, 3, 3)) == -1 and b"node_y[1]" in _err(lib) and b"finite" in _err(lib)
    assert call(ny=_host([0.0, 31.5, 31.5]), nx=n3, shape=(1, 3, 1, 64, 64, 3, 3)) == -1
    assert b"node_y" in _err(lib) and b"strictly increasing" in _err(lib) and b"index 2" in _err(lib)
    assert call(ny=n3, nx=_host([5.0, 4.0, 63.0]), shape=(1, 3, 1, 64, 64, 3, 3)) == -1
    assert b"node_x" in _err(lib) and b"strictly increasing" in _err(lib) and b"index 1" in _err(lib)
    need = lib.aadff_render_psf_map_blend_stack_bwd_workspace(1, 3, 1, 64, 64, 2, 3)
    assert call(nbytes=C.c_size_t(need - 4)) == -1 and b"workspace" in _err(lib)
    assert call(ws=None, nbytes=C.c_size_t(need)) == -1 and b"workspace" in _err(lib)


def test_without_a_gpu_grad_inputs_raise_and_the_rest_delegates(monkeypatch):
    img, maps = torch.zeros(2, 3, 16, 16), torch.zeros(2, 3, 10, 10)
    # no grad: the same function results as aadff.blend, empty shapes included
    assert diffrender.render_psf_map_blend_stack(img[:0], maps, 2).shape == blend.render_psf_map_blend_stack(img[:0], maps, 2).shape == (0, 3, 2, 16, 16)
    assert diffrender.render_psf_map_blend_stack(img, maps[:0], 2).shape == (2, 3, 0, 16, 16)
    assert diffrender.render_psf_map_blend(img[:0], maps[0], 2).shape == (0, 3, 16, 16)
    seen = []
    monkeypatch.setattr(blend, "render_psf_map_blend_stack", lambda *a, **k: seen.append((a, k)) or "delegated")
    assert diffrender.render_psf_map_blend_stack(img, maps, 2, nodes="patch") == "delegated" and seen[-1][0][2:] == (2, "patch")
    with torch.no_grad():
        assert diffrender.render_psf_map_blend_stack(img.clone().requires_grad_(), maps, 2) == "delegated"
    monkeypatch.undo()
    # the wrapper's assertions are the forward's
    with pytest.raises(AssertionError, match="divisible by grid"):
        diffrender.render_psf_map_blend_stack(img.clone().requires_grad_(), maps, 3)
    with pytest.raises(AssertionError, match="PSF map should be"):
        diffrender.render_psf_map_blend(img.clone().requires_grad_(), maps, 2)
    # an empty stack stays in the graph
    x = img.clone().requires_grad_()
    out = diffrender.render_psf_map_blend_stack(x, maps[:0], 2)
    assert out.shape == (2, 3, 0, 16, 16) and out.requires_grad
    out.sum().backward()
    assert x.grad is not None and not bool(x.grad.any())
    # no GPU: loud
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    monkeypatch.setattr(_abi, "_gpu_ok", False)
    for a, b in ((img.clone().requires_grad_(), maps), (img, maps.clone().requires_grad_())):
        with pytest.raises(RuntimeError, match="no HIP device"):
            diffrender.render_psf_map_blend_stack(a, b, 2)
        with pytest.raises(RuntimeError, match="no HIP device"):
            diffrender.render_psf_map_blend(a, b[0], 2, nodes="patch")
        with pytest.raises(RuntimeError, match="forward-only HIP op.*aadff.diffrender"):
            blend.render_psf_map_blend_stack(a, b, 2)
