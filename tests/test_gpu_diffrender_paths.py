"""GPU tests (run with `-m gpu` on an MI355X): the gradient kernels of the image-space operators - map_dimg_kernel<11> / <0>,
map_dpsf_partial_kernel<11> / <1> with map_dpsf_sum_kernel (csrc/conv_bwd.hip), local_dimg_kernel and local_dpsf_kernel<11> / <0>
(csrc/gather.hip, gather_adjoint of csrc/gather_window.h) - element by element against float64 on the CPU.

tests/diffrender_paths_common.py has the case table (the smallest shapes at which each path can go wrong), the comparator (torch.autograd
through oracle.conv in float64) and the derived bounds; tests/test_diffrender_paths_host.py shows on the CPU that the comparator is the
definition, that the bounds are attainable and that they reject eight planted errors.  Every case goes through the C entry points
(aadff._abi.call) three times - both gradients, d_img alone (d_psf and the workspace NULL), d_psf alone - and every call asserts
  (a) every output element written: the outputs are pre-filled with a sentinel, none survives, all are finite;
  (b) nothing else written: outputs and workspace lie in one buffer between guard regions that must keep their pattern, the workspace is
      exactly the queried byte count and starts as NaN, so a NaN in d_psf is a slab the sum pass read and nobody wrote; inputs unchanged;
  (c) the single-output calls equal the joint call bit for bit;
  (d) every element within its bound, (N + 2) u A or (min(D, N) + 2) u A, no element excluded: the largest share goes through `margin`
      with tolerance 1, and a failure names the worst element, its error and its bound.
The relative L2 distance is printed in units of the oracle's own float32 distance d32, for information.  Two more tests go through
aadff.diffrender with cotangents that are not contiguous.  No number here comes from the kernels under test.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import diffrender_paths_common as dp                       # noqa: E402
import aadff.diffrender as dr                              # noqa: E402
from aadff import _abi                                     # noqa: E402

DEV = "cuda:0"
GUARD = 256                                                # floats around every region
PATTERN = 0x5A5A5A5A                                       # a finite float32 (1.5e16) no kernel here produces


class _Arena:
    """Regions of one device buffer, each between guards: [guard | region 0 | guard | region 1 | ... | guard], regions 256-byte aligned."""

    def __init__(self, sizes):
        self.spans, n = [], GUARD
        for s in sizes:
            self.spans.append((n, n + s))
            n = (n + s + 63) // 64 * 64 + GUARD
        self.buf = torch.empty(n, dtype=torch.float32, device=DEV)
        self.buf.view(torch.int32).fill_(PATTERN)

    def region(self, k):
        a, b = self.spans[k]
        return self.buf[a:b]

    def guards_intact(self):
        keep = torch.ones(self.buf.numel(), dtype=torch.bool, device=DEV)
        for a, b in self.spans:
            keep[a:b] = False
        return bool((self.buf.view(torch.int32)[keep] == PATTERN).all())


def _call(c, r, want_img, want_psf):
    """One call of the C entry point: (d_img or None, d_psf or None) on the CPU after (a) and (b)."""
    img, psf, dy = r.img.to(DEV), r.psf.to(DEV), r.dy.to(DEV)
    nbytes = 0
    if c.op == "map" and want_psf:
        nbytes = _abi.query_bytes("aadff_render_psf_map_stack_bwd_workspace", c.B, c.C, c.S, c.H, c.W, c.grid, c.ks)
        assert nbytes == dp.workspace_bytes(c) and nbytes % 4 == 0
    ar = _Arena([img.numel() if want_img else 0, psf.numel() if want_psf else 0, nbytes // 4])
    gi, gp, ws = ar.region(0), ar.region(1), ar.region(2)
    gi.fill_(dp.SENTINEL)
    gp.fill_(dp.SENTINEL)
    ws.fill_(float("nan"))
    ptr = lambda t: C.c_void_p(t.data_ptr()) if t.numel() else None      # noqa: E731
    st = _abi.stream_ptr(torch.device(DEV))
    if c.op == "map":
        _abi.call("aadff_render_psf_map_stack_bwd", _abi.ptr(img), _abi.ptr(psf), _abi.ptr(dy), ptr(gi), ptr(gp), ptr(ws), C.c_size_t(nbytes),
                  c.B, c.C, c.S, c.H, c.W, c.grid, c.ks, st)
    else:
        _abi.call("aadff_local_psf_render_bwd", _abi.ptr(img), _abi.ptr(psf), _abi.ptr(dy), ptr(gi), ptr(gp), c.B, c.C, c.H, c.W, c.ks, st)
    torch.cuda.synchronize()
    assert ar.guards_intact(), f"{c.id}: wrote outside its outputs and its workspace"                                      # (b)
    assert torch.equal(img.cpu(), r.img) and torch.equal(psf.cpu(), r.psf) and torch.equal(dy.cpu(), r.dy), f"{c.id}: an input changed"
    out = []
    for name, t, like in (("d_img", gi, r.img), ("d_psf", gp, r.psf)):
        if not t.numel():
            out.append(None)
            continue
        t = t.cpu().reshape(like.shape)
        left, bad = int((t == dp.SENTINEL).sum()), int((~torch.isfinite(t)).sum())
        assert left == 0, f"{c.id}: {left} of {t.numel()} elements of {name} were never written"                         # (a)
        assert bad == 0, f"{c.id}: {bad} elements of {name} are not finite (d_psf: the sum pass read a slab nobody wrote)"
        out.append(t)
    return out


def _check(c, name, got, ref64, bound, d32, margin, label=""):
    use, idx, err, b = dp.share(got, ref64, bound)
    rel = dp.rel_l2(got, ref64)
    print(f"\n[diffrender_paths] {dp.kernels(c)[name]} {c.id}{label} {name}: largest share of the elementwise bound {use:.4f} (element {idx}: "
          f"{err:.3e} of {b:.3e}); rel_l2 {rel:.3e} = {rel / d32 if d32 > 0 else 0.0:.2f} x d32 ({d32:.3e})")
    assert got.dtype == torch.float32
    margin(f"diffrender_paths {c.id}{label} {name} [{dp.kernels(c)[name]}]", use, 1.0)                                   # (d)


@pytest.mark.parametrize("c", dp.CASES, ids=[c.id for c in dp.CASES])
def test_gradients_against_float64(c, margin):
    r = dp.reference(c)
    bi, bp = dp.bounds(c, r)
    gi, gp = _call(c, r, True, True)
    gi_only, none_p = _call(c, r, True, False)
    none_i, gp_only = _call(c, r, False, True)
    assert none_p is None and none_i is None
    assert torch.equal(gi_only, gi) and torch.equal(gp_only, gp), f"{c.id}: a single-output call differs from the joint call"   # (c)
    _check(c, "d_img", gi, r.gi, bi, r.d32_img, margin)
    _check(c, "d_psf", gp, r.gp, bp, r.d32_psf, margin)


def test_ks1_map_d_img_is_the_slice_sum_of_rounded_products():
    """ks 1: one fmaf with a zero accumulator per slice, the slices added in order."""
    c = next(c for c in dp.MAP_CASES if c.ks == 1)
    r = dp.reference(c)
    _, pi = dp.patch_index(c.H, c.grid)
    _, pj = dp.patch_index(c.W, c.grid)
    w = r.psf[:, :, pi][:, :, :, pj]                                        # [S,C,H,W]: the tap of every pixel's patch
    want = None
    for s in range(c.S):
        prod = r.dy[:, :, s] * w[s][None]                                   # float32: fl(dy w)
        want = prod if want is None else want + prod
    assert torch.equal(_call(c, r, True, False)[0], want)


@pytest.mark.parametrize("c", dp.FRONT_CASES, ids=[c.id for c in dp.FRONT_CASES])
def test_front_end_with_cotangents_that_are_not_contiguous(c, margin):
    """aadff.diffrender -> torch.ops.aadff.*_bwd -> _f32(dy): an expanded (stride-0) cotangent from out.sum().backward() and a permuted view."""
    img, psf, dy = dp.inputs(c)

    def run(cotangent):
        x, w = img.to(DEV).requires_grad_(True), psf.to(DEV).requires_grad_(True)
        out = dr.render_psf_map_stack(x, w, c.grid) if c.op == "map" else dr.local_psf_render(x, w, kernel_size=c.ks)
        assert tuple(out.shape) == tuple(dy.shape)
        if cotangent is None:
            out.sum().backward()
        else:
            assert not cotangent.is_contiguous() and tuple(cotangent.shape) == tuple(out.shape)
            out.backward(cotangent)
        torch.cuda.synchronize()
        return x.grad.cpu(), w.grad.cpu()

    perm = (0, 2, 1, 4, 3) if c.op == "map" else (1, 0, 3, 2)              # its own inverse
    view = dy.permute(perm).contiguous().to(DEV).permute(perm)
    assert torch.equal(view.cpu(), dy)
    for label, cot, d in ((" dy=ones(expanded)", None, torch.ones_like(dy)), (" dy=permuted view", view, dy)):
        r = dp.build_reference(c, img, psf, d)
        bi, bp = dp.bounds(c, r)
        gi, gp = run(cot)
        assert gi.shape == img.shape and gp.shape == psf.shape
        _check(c, "d_img", gi, r.gi, bi, r.d32_img, margin, label)
        _check(c, "d_psf", gp, r.gp, bp, r.d32_psf, margin, label)
