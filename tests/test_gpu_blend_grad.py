"""GPU tests (run with `-m gpu` on an MI355X): the gradients of the blended PSF-map render (aadff_render_psf_map_blend_stack_bwd,
csrc/conv_blend_bwd.hip; aadff.diffrender.render_psf_map_blend[_stack]) against float64 autograd on the CPU.

tests/blend_grad_common.py has the case table (every instantiation of the three kernels), the comparator and the derived elementwise
budget; tests/test_blend_grad_host.py anchors them on the CPU.  Every case asserts: both gradients through the public functions within
the budget on every element, none excluded; the C entry overwrites sentinel-filled outputs completely, with exact zeros at the nodes
whose hat holds no pixel; two runs bit-equal; either gradient alone bit-equal to the pair; the forward value under grad bit-equal to
aadff.blend.  The relative L2 is printed and recorded, not gated.  No number here comes from the kernels under test.
"""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import blend_common as bc                                  # noqa: E402
import blend_grad_common as bg                             # noqa: E402
from aadff import _abi                                     # noqa: E402
from aadff import blend                                    # noqa: E402
from aadff import diffrender                               # noqa: E402

DEV = "cuda:0"


def _host_ptr(t):
    assert t.dtype == torch.float32 and t.is_contiguous() and not t.is_cuda
    return C.c_void_p(t.data_ptr())


def _entry(c, r, want_img=True, want_maps=True):
    """The C entry into sentinel-filled outputs: (d_img, d_maps) float32 on the CPU (None where not asked for)."""
    x, m, dy = r.img.to(DEV).contiguous(), r.maps.to(DEV).contiguous(), r.dy.to(DEV).contiguous()
    gi = torch.full_like(x, bg.SENTINEL) if want_img else None
    gm = torch.full_like(m, bg.SENTINEL) if want_maps else None
    nbytes = _abi.load_library().aadff_render_psf_map_blend_stack_bwd_workspace(c.B, c.C, c.S, c.H, c.W, c.grid, c.ks)
    assert nbytes == bg.workspace_bytes(c)
    ws = torch.full((nbytes // 4,), float("nan"), device=DEV) if want_maps else None
    _abi.call("aadff_render_psf_map_blend_stack_bwd", _abi.ptr(x), _abi.ptr(m), _abi.ptr(dy), _abi.ptr(gi), _abi.ptr(gm), _abi.ptr(ws),
              C.c_size_t(nbytes if want_maps else 0), _host_ptr(r.ny), _host_ptr(r.nx), c.B, c.C, c.S, c.H, c.W, c.grid, c.ks,
              _abi.stream_ptr(torch.device(DEV)))
    torch.cuda.synchronize()
    out = []
    for g in (gi, gm):
        if g is not None:
            g = g.cpu()
            left = int((g == bg.SENTINEL).sum())
            assert left == 0, f"{left} of {g.numel()} elements were never written"
            assert bool(torch.isfinite(g).all())
        out.append(g)
    return out


@pytest.mark.parametrize("c", bg.TABLE, ids=[c.id for c in bg.TABLE])
def test_case_against_float64(c, margin):
    assert bg.kernels(c.ks) <= bg.expected_instantiations()
    r = bg.reference(c)
    bound = bg.bounds(r)
    x, m = r.img.to(DEV).requires_grad_(), r.maps.to(DEV).requires_grad_()
    out = diffrender.render_psf_map_blend_stack(x, m, c.grid, nodes=(r.ny, r.nx))
    assert torch.equal(out.detach(), blend.render_psf_map_blend_stack(x.detach(), m.detach(), c.grid, nodes=(r.ny, r.nx)))
    out.backward(r.dy.to(DEV))
    got = {"d_img": x.grad.cpu(), "d_maps": m.grad.cpu()}
    for name, ref in (("d_img", r.gi), ("d_maps", r.gm)):
        assert got[name].dtype == torch.float32
        use, worst, rel = bg.compare(got[name], ref, bound[name])
        err = float((got[name].double() - ref).abs().flatten()[worst])
        print(f"\n{c.id} [{name}; {c.reaches}]: largest use of the elementwise budget {use:.3f}; rel_l2 {rel:.3e}")
        assert use <= 1.0, f"{c.id}: element {worst} of {name} {tuple(ref.shape)} is {err:.3e} from float64, {use:.2f} x its budget"
        margin(f"blend grad {c.id} {name}: share of the elementwise budget", use, 1.0)
        margin(f"blend grad {c.id} {name}: rel_l2 (reported, not gated)", rel, float("inf"))
    # the C entry: everything written, zeros exactly where no pixel lies under the hat, the same bits as through autograd
    gi, gm = _entry(c, r)
    assert torch.equal(gi, got["d_img"]) and torch.equal(gm, got["d_maps"])
    assert bool((gm[r.Mm == 0] == 0).all())
    # two runs; either gradient alone
    gi2, gm2 = _entry(c, r)
    assert torch.equal(gi, gi2) and torch.equal(gm, gm2)
    assert torch.equal(_entry(c, r, want_maps=False)[0], gi) and torch.equal(_entry(c, r, want_img=False)[1], gm)


def test_unsupported_nodes_get_exact_zeros():
    c = next(c for c in bg.TABLE if c.grid == 64)
    r = bg.reference(c)
    _, gm = _entry(c, r, want_img=False)
    tiles = gm.reshape(c.S, c.C, c.grid, c.ks, c.grid, c.ks).abs().amax((0, 1, 3, 5))
    want = r.Mm.reshape(c.S, c.C, c.grid, c.ks, c.grid, c.ks).amax((0, 1, 3, 5))
    assert bool(((tiles == 0) == (want == 0)).all()) and int((tiles == 0).sum()) > 3000


def test_single_slice_cpu_and_non_contiguous_inputs_and_one_sided_grads():
    c = bg.TABLE[0]                                                              # B 2, C 3, S 1
    r = bg.reference(c)
    gi, gm = _entry(c, r)
    # the single-slice function, CPU inputs that are views with strides
    x = r.img.transpose(2, 3).contiguous().transpose(2, 3).requires_grad_()
    m = r.maps[0].transpose(1, 2).contiguous().transpose(1, 2).requires_grad_()
    assert not x.is_contiguous() and not m.is_contiguous()
    out = diffrender.render_psf_map_blend(x, m, c.grid)                          # the default nodes are the case's
    assert out.device.type == "cpu" and out.shape == (c.B, c.C, c.H, c.W)
    with torch.no_grad():
        assert torch.equal(out, blend.render_psf_map_blend(x, m, c.grid))
    dy = r.dy[:, :, 0].transpose(2, 3).contiguous().transpose(2, 3)
    out.backward(dy)
    assert x.grad.device.type == "cpu" and torch.equal(x.grad, gi) and torch.equal(m.grad, gm[0])
    # one input requires grad: that gradient alone, the same bits
    x2 = r.img.to(DEV).requires_grad_()
    (g2,) = torch.autograd.grad(diffrender.render_psf_map_blend_stack(x2, r.maps.to(DEV), c.grid), x2, r.dy.to(DEV))
    assert torch.equal(g2.cpu(), gi)
    m2 = r.maps.to(DEV).requires_grad_()
    (g3,) = torch.autograd.grad(diffrender.render_psf_map_blend_stack(r.img.to(DEV), m2, c.grid), m2, r.dy.to(DEV))
    assert torch.equal(g3.cpu(), gm)
    # under no_grad the differentiable twin is the forward-only function
    with torch.no_grad():
        assert not diffrender.render_psf_map_blend_stack(x2, m2, c.grid).requires_grad


def test_double_backward_raises_and_an_empty_stack_backpropagates_zeros():
    c = bg.TABLE[0]
    r = bg.reference(c)
    x = r.img.to(DEV).requires_grad_()
    out = diffrender.render_psf_map_blend_stack(x, r.maps.to(DEV), c.grid)
    (g,) = torch.autograd.grad(out, x, r.dy.to(DEV), create_graph=True)
    with pytest.raises(RuntimeError):                                            # the gradient carries no graph
        g.sum().backward()
    out = diffrender.render_psf_map_blend_stack(x, r.maps.to(DEV), c.grid)
    (g,) = torch.autograd.grad(out, x, r.dy.to(DEV).requires_grad_(), create_graph=True)
    with pytest.raises(RuntimeError, match="once_differentiable|twice"):         # and one that would need it says so
        g.sum().backward()
    x = r.img.to(DEV).requires_grad_()
    m = r.maps[:0].to(DEV).requires_grad_()
    out = diffrender.render_psf_map_blend_stack(x, m, c.grid)
    assert out.shape == (c.B, c.C, 0, c.H, c.W)
    out.sum().backward()
    assert x.grad.shape == x.shape and not bool(x.grad.any()) and m.grad.shape == m.shape


def test_short_fit_descends_as_the_float64_run_does(margin):
    """The example's fit at 64 x 64, grid 3, ks 5: five Adam steps on the maps from the same start on the GPU (float32) and through the
    float64 comparator on the CPU.  Both losses fall at every step; at every step the GPU's gradient of the maps is within the budget of the
    float64 gradient at the SAME maps and the same dy (the one autograd handed the kernel)."""
    H = W = 64
    g, ks, steps = 3, 5, 5
    c = bg.Case("fit", 1, 3, 1, H, W, g, ks, "psf_map", False, "fit")
    gen = torch.Generator().manual_seed(4)
    img = torch.rand((1, 3, H, W), generator=gen)
    true = torch.rand((1, 3, g, ks, g, ks), generator=gen) + 0.05
    true = (true / true.sum((3, 5), keepdim=True)).reshape(1, 3, g * ks, g * ks)
    start = torch.full_like(true, 1.0 / (ks * ks))
    ny, nx = bc.closed_form_nodes(H, g, "psf_map"), bc.closed_form_nodes(W, g, "psf_map")
    target64 = bc.blend64(img, true, g, ny, nx, want_bound=False).out64
    target = blend.render_psf_map_blend_stack(img.to(DEV), true.to(DEV), g)

    m64 = start.double().clone().requires_grad_()
    opt64 = torch.optim.Adam([m64], lr=2e-3)
    m32 = start.to(DEV).clone().requires_grad_()
    opt32 = torch.optim.Adam([m32], lr=2e-3)
    x = img.to(DEV)
    loss64, loss32 = [], []
    for k in range(steps + 1):
        opt64.zero_grad()
        l64 = ((bc.blend64(img.double(), m64, g, ny, nx, want_bound=False).out64 - target64) ** 2).mean()
        l64.backward()
        loss64.append(float(l64.detach()))
        opt32.zero_grad()
        out = diffrender.render_psf_map_blend_stack(x, m32, g)
        out.retain_grad()
        l32 = ((out - target) ** 2).mean()
        l32.backward()
        loss32.append(float(l32.detach()))
        here, dy = m32.detach().cpu(), out.grad.cpu()
        r = bg.build_reference(c, img, here, dy, ny, nx)
        use, worst, rel = bg.compare(m32.grad.cpu(), r.gm, bg.bounds(r)["d_maps"])
        print(f"\nfit step {k}: loss {loss32[-1]:.6e} (float64 run {loss64[-1]:.6e}); d_maps uses {use:.3f} of the budget, rel_l2 {rel:.2e}")
        margin(f"blend fit step {k}: d_maps share of the elementwise budget", use, 1.0)
        opt64.step()
        opt32.step()
    assert all(b < a for a, b in zip(loss64, loss64[1:])), loss64
    assert all(b < a for a, b in zip(loss32, loss32[1:])), loss32
