"""GPU tests (run with `-m gpu` on an MI355X): the gradients of the occlusion-aware layered PSF-map render
(aadff_render_psf_map_stack_occluded_bwd, csrc/conv_occl_bwd.hip; aadff.diffrender.render_psf_map_occluded[_stack]) against float64
autograd on the CPU.

tests/occl_grad_common.py has the case table (every instantiation of the kernels), the comparator and the derived elementwise budget;
tests/test_occl_grad_host.py anchors them on the CPU.  Every case asserts: both gradients through the public functions within the budget
on every element, none excluded, with `normalize` on and off and with and without a gradient to the coverage, and inside the rel-L2
gate 4 x d32 (d32: torch float32 autograd through the same comparator on the CPU); the forward under grad bit-equal to aadff.occlusion;
the C entry overwrites sentinel-filled outputs completely from a NaN-filled workspace; two runs bit-equal; either gradient alone
bit-equal to the pair; minimum and full workspace bit-equal; exact zeros at hole texels and at the maps of absent layers; NaNs planted
on hole texels change no bit; g scaled by 4 scales both gradients by 4 bit for bit; for S = 1 a batch equals its images in d_img.
No number here comes from the kernels under test.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import occl_grad_common as og                              # noqa: E402
from aadff import _abi                                     # noqa: E402
from aadff import diffrender                               # noqa: E402
from aadff import occlusion                                # noqa: E402

DEV = "cuda:0"
NAME = "aadff_render_psf_map_stack_occluded_bwd"


def _entry(c, img, maps, lay, g, h, normalize=1, want_img=True, want_maps=True, slices_per_pass=None):
    """The C entry into sentinel-filled outputs from a NaN-filled workspace: (d_img, d_maps) float32 on the CPU (None where not asked)."""
    B = img.shape[0]
    x, m, li = img.to(DEV).contiguous(), maps.to(DEV).contiguous(), lay.to(DEV).contiguous()
    gd = None if g is None else g.to(DEV).contiguous()
    hd = None if h is None else h.to(DEV).contiguous()
    gi = torch.full_like(x, og.SENTINEL) if want_img else None
    gm = torch.full_like(m, og.SENTINEL) if want_maps else None
    query = _abi.load_library().aadff_render_psf_map_stack_occluded_bwd_workspace
    nbytes = query(B, c.C, c.S if slices_per_pass is None else slices_per_pass, c.L, c.H, c.W, c.grid, c.ks, 1 if want_maps else 0)
    assert nbytes > 0
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV)
    _abi.call(NAME, _abi.ptr(x), _abi.ptr(m), _abi.ptr(li), _abi.ptr(gd), _abi.ptr(hd), _abi.ptr(gi), _abi.ptr(gm), _abi.ptr(ws),
              C.c_size_t(nbytes), B, c.C, c.S, c.L, c.H, c.W, c.grid, c.ks, normalize, _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    out = []
    for t in (gi, gm):
        if t is not None:
            t = t.cpu()
            left = int((t == og.SENTINEL).sum())
            assert left == 0, f"{left} of {t.numel()} elements were never written"
            assert bool(torch.isfinite(t).all())
        out.append(t)
    return out


@pytest.mark.parametrize("c", og.TABLE, ids=[c.id for c in og.TABLE])
def test_gradients_against_float64(c, margin):
    assert og.kernels(c.ks) <= og.expected_instantiations()
    img, maps, lay, g, h = og.case_inputs(c)
    for normalize, with_h in og.COMBOS:
        r = og.reference(c, normalize, with_h)
        x, m = img.to(DEV).requires_grad_(), maps.to(DEV).requires_grad_()
        out, cov = diffrender.render_psf_map_occluded_stack(x, m, lay, c.L, c.grid, normalize=bool(normalize), return_coverage=True)
        fo, fc = occlusion.render_psf_map_occluded_stack(x.detach(), m.detach(), lay, c.L, c.grid, normalize=bool(normalize), return_coverage=True)
        assert out.requires_grad and cov.requires_grad and torch.equal(out.detach(), fo) and torch.equal(cov.detach(), fc)
        if with_h:
            gi, gm = torch.autograd.grad((out, cov), (x, m), (g.to(DEV), h.to(DEV)))
        else:
            gi, gm = torch.autograd.grad(out, (x, m), g.to(DEV))
        got = {"d_img": gi.cpu(), "d_maps": gm.cpu()}
        tag = f"normalize={normalize}, {'g and h' if with_h else 'g alone'}"
        for name, ref, bound, d32 in (("d_img", r.gi, r.bi, r.d32i), ("d_maps", r.gm, r.bm, r.d32m)):
            assert got[name].dtype == torch.float32 and bool(torch.isfinite(got[name]).all())
            use, worst = og.compare(got[name], ref, bound)
            rel = og.rel_l2(got[name], ref)
            err = float((got[name].double() - ref).abs().flatten()[worst])
            print(f"\n{c.id} [{name}; {tag}]: largest use of the elementwise budget {use:.3f}; rel_l2 {rel:.3e} against 4 x d32 = {4 * d32:.3e}")
            assert use <= 1.0, f"{c.id} ({tag}): element {worst} of {name} {tuple(ref.shape)} is {err:.3e} from float64, {use:.2f} x its budget"
            assert rel <= 4 * d32, f"{c.id} ({tag}): {name} rel_l2 {rel:.3e} above 4 x d32 = {4 * d32:.3e}"
            margin(f"occl grad {c.id} {name} ({tag}): share of the elementwise budget", use, 1.0)
        if (normalize, with_h) == (1, True):
            ei, em = _entry(c, img, maps, lay, g, h, 1)
            assert torch.equal(ei, got["d_img"]) and torch.equal(em, got["d_maps"]), "the public functions and the C entry differ"
    # only the gradient autograd asks for
    x = img.to(DEV).requires_grad_()
    out = diffrender.render_psf_map_occluded_stack(x, maps.to(DEV), lay, c.L, c.grid)
    gi, = torch.autograd.grad(out, x, g.to(DEV))
    assert torch.equal(gi.cpu(), _entry(c, img, maps, lay, g, None, 1, want_maps=False)[0])


@pytest.mark.parametrize("c", og.TABLE, ids=[c.id for c in og.TABLE])
def test_entry_is_exact_where_the_contract_is(c):
    img, maps, lay, g, h = og.case_inputs(c)
    gi, gm = _entry(c, img, maps, lay, g, h)
    # two runs, either gradient alone, minimum workspace
    gi2, gm2 = _entry(c, img, maps, lay, g, h)
    assert torch.equal(gi, gi2) and torch.equal(gm, gm2)
    assert torch.equal(_entry(c, img, maps, lay, g, h, want_maps=False)[0], gi)
    assert torch.equal(_entry(c, img, maps, lay, g, h, want_img=False)[1], gm)
    lo_i, lo_m = _entry(c, img, maps, lay, g, h, slices_per_pass=1)
    assert torch.equal(lo_i, gi) and torch.equal(lo_m, gm)
    # exact zeros: hole texels, the maps of layers that occur nowhere
    hole = (lay >= c.L)[:, None].expand_as(img)
    assert bool((gi[hole] == 0).all())
    absent = [l for l in range(c.L) if not bool((lay == l).any())]
    for s in range(c.S):
        for l in absent:
            assert bool((gm[s * c.L + l] == 0).all()), (s, l)
    if c.scene == "even32":
        assert len(absent) == 16
    # NaNs on hole texels reach nothing
    if bool(hole.any()):
        bad = img.clone()
        bad[hole] = float("nan")
        ni, nm = _entry(c, bad, maps, lay, g, h)
        assert torch.equal(ni, gi) and torch.equal(nm, gm)
    # g scaled by 4: both gradients scaled by 4, bit for bit (no gradient to the coverage, which does not scale with g)
    for normalize in (1, 0):
        a_i, a_m = _entry(c, img, maps, lay, g, None, normalize)
        b_i, b_m = _entry(c, img, maps, lay, 4 * g, None, normalize)
        assert torch.equal(4 * a_i, b_i) and torch.equal(4 * a_m, b_m)
    # S = 1: a batch equals its images in d_img
    if c.S == 1 and c.B > 1:
        for b in range(c.B):
            one, _ = _entry(c, img[b:b + 1], maps, lay[b:b + 1], g[b:b + 1], h[b:b + 1])
            assert torch.equal(one[0], gi[b]), b


def test_minimum_and_full_workspace_on_a_batched_stack():
    c = og.WS_CASE
    assert c.B == 2 and c.S == 3
    img, maps, lay, g, h = og.case_inputs(c)
    full = _entry(c, img, maps, lay, g, h)
    for per_pass in (1, 2):                                                  # three passes; one of two slices and one of one
        part = _entry(c, img, maps, lay, g, h, slices_per_pass=per_pass)
        assert torch.equal(part[0], full[0]) and torch.equal(part[1], full[1]), per_pass


def test_double_backward_raises_and_single_slice_form():
    c = og.CLAMP
    img, maps, lay, g, h = og.case_inputs(c)
    x, m = img.to(DEV).requires_grad_(), maps.to(DEV).requires_grad_()
    out, cov = diffrender.render_psf_map_occluded(x, m, lay, c.grid, return_coverage=True)
    assert out.shape == (c.B, c.C, c.H, c.W)
    gi, gm = torch.autograd.grad((out, cov), (x, m), (g[:, :, 0].to(DEV), h[:, :, 0].to(DEV)), create_graph=True)
    ei, em = _entry(c, img, maps, lay, g, h)
    assert torch.equal(gi.detach().cpu(), ei) and torch.equal(gm.detach().cpu(), em)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gi.sum(), x)
    # without grad the twins are the forward-only functions
    with torch.no_grad():
        assert torch.equal(diffrender.render_psf_map_occluded(x, m, lay, c.grid), occlusion.render_psf_map_occluded(x.detach(), m.detach(), lay, c.grid))
