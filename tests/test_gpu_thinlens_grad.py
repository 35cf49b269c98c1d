"""GPU tests (run with `-m gpu` on an MI355X) of aadff.diffrender.thinlens_render / thinlens_render_stack and ThinLens.render_stack:
the stack-fused forward and the fused backward of the thin-lens baseline (csrc/thinlens.hip) against torch.autograd through the
oracle evaluated in float64 on the CPU (tests/thinlens_grad_common.py has the comparator, the cases and the cotangent mask).

Budget of every gradient (relative L2, masked cotangent): 4 x r x d32, as for the PSF-network renderer.
  d32  the oracle's own float32 autograd against its float64 autograd, same inputs, computed here;
  4    the project's allowance for another summation order of the same fp32 terms (tests/test_gpu_diffrender.py);
  r    max(1, e_fwd / d32_fwd): how far the EXISTING forward kernel's output (ThinLens.render, which uses __expf) already is from
       float64, in units of the oracle's float32.
Every (error, d32, r) is printed and goes through the `margin` fixture; DESIGN.md 4.9 has the table.
"""
import pytest
import torch

pytestmark = pytest.mark.gpu

import aadff.diffrender as dr                              # noqa: E402
import thinlens_grad_common as tc                          # noqa: E402
from deeplens.psfnet import ThinLens                       # noqa: E402

DEV = "cuda:0"
FALLBACK = ("1x5x40x56_S2_ks15_fallback", 1, 5, 2, 40, 56, 15, (256, 256), 2.8, [(800.0, 2500.0)], -1, (500.0, 5000.0))


def _lens(case):
    foc_len, fnum, ks, ssize, sres = tc.lens_args(case)
    return ThinLens(foc_len=foc_len, fnum=fnum, kernel_size=ks, sensor_size=ssize, sensor_res=sres)


def _gpu_grads(lens, img, depth, fds, dy, which=(True, True, True), dev=DEV):
    x = img.to(dev).requires_grad_(which[0])
    d = depth.to(dev).requires_grad_(which[1])
    f = fds.to(dev).requires_grad_(which[2])
    out = dr.thinlens_render_stack(lens, x, d, f)
    out.backward(dy.to(dev))
    torch.cuda.synchronize()
    return out.detach(), x.grad, d.grad, f.grad


_ORACLE = {}


def _reference(case):
    """Masked cotangent, float64 and float32 oracle results of a case (cached)."""
    if case[0] not in _ORACLE:
        img, depth, fds, dy = tc.case_inputs(case)
        keep = tc.keep_rows(case, depth, fds)
        share = 1.0 - float(keep.mean())
        dym = dy * keep
        o64 = tc.oracle_grads(case, img, depth, fds, dym, torch.float64)
        o32 = tc.oracle_grads(case, img, depth, fds, dym, torch.float32)
        _ORACLE[case[0]] = (img, depth, fds, dym, share, o64, [tc.rel_l2(a, b) for a, b in zip(o32, o64)])
    return _ORACLE[case[0]]


def _check(tag, got, o64, d32, out_fwd, margin):
    """got = (d_img, d_depth, d_foc); out_fwd = the existing forward kernel's output."""
    e_fwd = tc.rel_l2(out_fwd, o64[0])
    r = max(1.0, e_fwd / d32[0])
    print(f"\n{tag}: forward e_fwd {e_fwd:.3e} d32_fwd {d32[0]:.3e} r {r:.2f}")
    failed = []
    for name, g, ref, d in zip(("d_img", "d_depth", "d_foc"), got, o64[1:], d32[1:]):
        err, tol = tc.rel_l2(g.reshape(ref.shape), ref), 4.0 * r * d
        print(f"{tag}: {name} err {err:.3e} d32 {d:.3e} r {r:.2f} budget {tol:.3e}")
        try:
            margin(f"thinlens_grad {tag} {name}", err, tol)
        except AssertionError as e:                          # every figure is printed and recorded before the test fails
            failed.append(str(e))
    assert not failed, "; ".join(failed)


def _slice_loop(lens, x, d, f):
    return torch.stack([lens.render(x, d, f[:, i]) for i in range(f.shape[1])], dim=2)


@pytest.mark.parametrize("case", tc.CASES, ids=[c[0] for c in tc.CASES])
def test_gradient_parity(case, margin):
    img, depth, fds, dym, share, o64, d32 = _reference(case)
    assert share <= tc.MAX_MASKED, f"{share:.3%} of the rows are excluded"
    assert all(v <= tc.MAX_D32 for v in d32[1:]), d32
    lens = _lens(case)
    out_fwd = _slice_loop(lens, img.to(DEV), depth.to(DEV), fds.to(DEV))                 # S launches of the existing kernel
    out, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dym)
    assert torch.equal(out, out_fwd)
    _check(case[0], (gi, gd, gf), o64, d32, out_fwd, margin)


@pytest.mark.parametrize("case", tc.CASES, ids=[c[0] for c in tc.CASES])
def test_render_stack_is_bit_equal_to_the_slice_loop(case):
    img, depth, fds, dy = tc.case_inputs(case)
    lens = _lens(case)
    x, d, f = img.to(DEV), depth.to(DEV), fds.to(DEV)
    want = _slice_loop(lens, x, d, f)
    got = lens.render_stack(x, d, f)
    assert got.shape == want.shape == (case[1], case[2], case[3], case[4], case[5]) and torch.equal(got, want)
    assert torch.equal(lens.render_stack(img, depth, fds), want.cpu())                   # inputs on the CPU: result on the CPU


@pytest.mark.parametrize("sign", (+1, -1), ids=("positive_depth", "negative_depth"))
@pytest.mark.parametrize("B,C,H,W,ks", ((2, 3, 5, 70, 11),            # every row clamped, a ragged second run
                                        (1, 4, 9, 64, 3),             # the run-time channel path, exactly one run
                                        (1, 1, 13, 130, 13)))         # the largest compiled ks, three runs
def test_single_focus_op_is_the_stack_op_with_one_slice(B, C, H, W, ks, sign):
    """The single-focus kernel and the stack kernel call one device body (render_slice, csrc/thinlens.hip): foc_dist [B] is foc_dists
    [B,1] and [B,C,H,W] the memory of [B,C,1,H,W].  Both depth conventions, so the kernels' `negate` word is 0 once and 1 once."""
    case = (f"{B}x{C}x{H}x{W}_S1_ks{ks}", B, C, 1, H, W, ks, (256, 256), 2.8, [(700.0 + 500.0 * n,) for n in range(B)], sign, (500.0, 5000.0))
    img, depth, fds, _ = tc.case_inputs(case)
    assert bool((depth < 0).any()) == (sign < 0)
    lens = _lens(case)
    x, d, f = img.to(DEV), depth.to(DEV), fds.to(DEV)
    consts = (ks, tc.FOC_LEN, 2.8, lens.ps, float(lens.d_min), float(lens.d_max))
    one = torch.ops.aadff.thinlens_render(x, d, f[:, 0].contiguous(), *consts)
    stack = torch.ops.aadff.thinlens_render_stack(x, d, f, *consts)
    assert one.shape == (B, C, H, W) and stack.shape == (B, C, 1, H, W)
    assert torch.equal(one, stack[:, :, 0]) and torch.isfinite(one).all() and not torch.equal(one, x)


def test_other_kernel_sizes_and_channels(margin):
    """Every other kernel size of the fused domain, 2 and 4 channels (runtime channel count), a width below one run: the stack forward
    is bit-equal to the slice loop everywhere, and two of the shapes go through the gradient budget."""
    for ks, C, H, W, grads in ((3, 2, 9, 70, False), (5, 4, 33, 64, True), (9, 2, 20, 17, True), (13, 4, 16, 129, False)):
        case = (f"2x{C}x{H}x{W}_S2_ks{ks}", 2, C, 2, H, W, ks, (256, 256), 2.8, [(700.0, 2500.0), (1200.0, 4000.0)], -1, (500.0, 5000.0))
        lens = _lens(case)
        if not grads:
            img, depth, fds, dy = tc.case_inputs(case)
            x, d, f = img.to(DEV), depth.to(DEV), fds.to(DEV)
            assert torch.equal(lens.render_stack(x, d, f), _slice_loop(lens, x, d, f)), (ks, C)
            for g in _gpu_grads(lens, img, depth, fds, dy)[1:]:
                assert torch.isfinite(g).all()
            continue
        img, depth, fds, dym, share, o64, d32 = _reference(case)
        out_fwd = _slice_loop(lens, img.to(DEV), depth.to(DEV), fds.to(DEV))
        out, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dym)
        assert torch.equal(out, out_fwd)
        _check(case[0], (gi, gd, gf), o64, d32, out_fwd, margin)


def test_wide_rows(margin):
    """Rows wider than two runs: the middle workgroups of the image-gradient kernel have no border lane and take its unchecked path."""
    case = ("1x3x24x200_S2_ks11_wide", 1, 3, 2, 24, 200, 11, (256, 256), 2.8, [(700.0, 2500.0)], -1, (500.0, 5000.0))
    img, depth, fds, dym, share, o64, d32 = _reference(case)
    assert share <= tc.MAX_MASKED
    lens = _lens(case)
    out_fwd = _slice_loop(lens, img.to(DEV), depth.to(DEV), fds.to(DEV))
    out, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dym)
    assert torch.equal(out, out_fwd)
    _check(case[0], (gi, gd, gf), o64, d32, out_fwd, margin)


def test_forward_bit_equal_with_and_without_grad():
    case = tc.CASES[1]
    img, depth, fds, dy = tc.case_inputs(case)
    lens = _lens(case)
    x, d, f = img.to(DEV), depth.to(DEV), fds.to(DEV)
    want = _slice_loop(lens, x, d, f)
    assert torch.equal(dr.thinlens_render_stack(lens, x, d, f), want)                     # nothing requires grad
    with torch.no_grad():
        assert torch.equal(dr.thinlens_render_stack(lens, x.clone().requires_grad_(True), d, f), want)
    out = dr.thinlens_render_stack(lens, x, d.clone().requires_grad_(True), f)
    assert out.requires_grad and torch.equal(out.detach(), want)
    out = dr.thinlens_render_stack(lens, x.clone().requires_grad_(True), d, f.clone().requires_grad_(True))
    assert out.requires_grad and torch.equal(out.detach(), want)
    want1 = lens.render(x, d, f[:, 1])
    assert torch.equal(dr.thinlens_render(lens, x, d, f[:, 1]), want1)
    out1 = dr.thinlens_render(lens, x, d.clone().requires_grad_(True), f[:, 1])
    assert out1.requires_grad and out1.shape == want1.shape and torch.equal(out1.detach(), want1)
    with pytest.raises(ValueError, match="3-D branch"):
        dr.thinlens_render(lens, x[0].clone().requires_grad_(True), d[0, 0], -1500.0)


def test_backward_is_deterministic_and_double_backward_raises():
    case = tc.CASES[1]
    img, depth, fds, dy = tc.case_inputs(case)
    lens = _lens(case)
    a = _gpu_grads(lens, img, depth, fds, dy)
    b = _gpu_grads(lens, img, depth, fds, dy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    with pytest.raises(RuntimeError):
        d = depth.to(DEV).requires_grad_(True)
        out = dr.thinlens_render_stack(lens, img.to(DEV), d, fds.to(DEV))
        (g,) = torch.autograd.grad(out.sum(), d, create_graph=True)
        g.sum().backward()


def test_clamp_and_floor_give_exact_zero():
    """Exactly 0.0 where the depth is outside [d_min, d_max] and where the 0.1 px floor is active (and, by the centred form, wherever
    only the centre tap is inside the disc); a whole batch in exact focus has no depth or focus gradient and d_img = dy."""
    case = tc.CASES[4]                                                                    # depths outside the clamp
    img, depth, fds, dy = tc.case_inputs(case)
    _, gi, gd, gf = _gpu_grads(_lens(case), img, depth, fds, dy)
    sg, d, f, dc, K, cp, r = tc.coc_chain(case, depth, fds)
    outside = ((d < tc.D_MIN) | (d > tc.D_MAX))[:, :, 0]
    assert 0.05 < float(outside.float().mean()) < 0.95
    assert (gd.cpu()[outside] == 0).all()
    live = (~outside) & (cp > 2.05).any(2)                                               # some slice has taps beside the centre
    assert float((gd.cpu()[live] != 0).float().mean()) > 0.99
    assert torch.isfinite(gd).all() and torch.isfinite(gi).all() and torch.isfinite(gf).all() and (gf != 0).all()

    case = tc.CASES[2]                                                                    # one slice: the floor of single rows
    img, depth, fds, dy = tc.case_inputs(case)
    _, gi, gd, gf = _gpu_grads(_lens(case), img, depth, fds, dy)
    sg, d, f, dc, K, cp, r = tc.coc_chain(case, depth, fds)
    floor = (cp < 0.0999)[:, :, 0]
    assert floor.any() and (gd.cpu()[floor] == 0).all()
    centre_only = (cp < 1.999)[:, :, 0]
    assert (gd.cpu()[centre_only] == 0).all()

    lens = _lens(tc.CASES[0])
    img, _, _, _ = tc.case_inputs(tc.CASES[0])
    depth = torch.full((1, 1, 64, 64), -1500.0)
    fds = torch.tensor([[-1500.0]])
    dy = torch.randn((1, 3, 1, 64, 64), generator=torch.Generator().manual_seed(5))
    out, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dy)
    assert torch.equal(out[:, :, 0].cpu(), img)                                           # delta PSF
    assert (gd == 0).all() and (gf == 0).all() and torch.equal(gi.cpu(), dy[:, :, 0])


def test_gradient_subsets():
    """Only the required gradients are computed: the image alone takes no per-workgroup partials (no input-gradient kernel), the depth
    alone takes no workspace at all (no pre-pass, no d_img kernel); the values do not depend on the subset."""
    case = tc.CASES[0]
    img, depth, fds, dy = tc.case_inputs(case)
    lens = _lens(case)
    _, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dy)
    _, gi1, gd1, gf1 = _gpu_grads(lens, img, depth, fds, dy, which=(False, True, False))
    assert gi1 is None and gf1 is None and torch.equal(gd1, gd)
    _, gi2, gd2, gf2 = _gpu_grads(lens, img, depth, fds, dy, which=(True, False, False))
    assert gd2 is None and gf2 is None and torch.equal(gi2, gi)
    _, gi3, gd3, gf3 = _gpu_grads(lens, img, depth, fds, dy, which=(False, False, True))
    assert gi3 is None and gd3 is None and torch.equal(gf3, gf)
    x, d, f, g = img.to(DEV), depth.to(DEV), fds.to(DEV), dy.to(DEV)
    consts = (11, 50.0, 2.8, lens.ps, float(lens.d_min), float(lens.d_max))
    a, b, c = torch.ops.aadff.thinlens_render_stack_bwd(x, d, f, g, *consts, True, False, False)
    assert torch.equal(a, gi) and b.numel() == 0 and c.numel() == 0
    a, b, c = torch.ops.aadff.thinlens_render_stack_bwd(x, d, f, g, *consts, False, True, False)
    assert a.numel() == 0 and torch.equal(b, gd) and c.numel() == 0
    from aadff import ops
    assert ops.thinlens_bwd_workspace_bytes(1, 3, 5, 64, 64, 11, True, False) == 8 * 5 * 64 * 64
    assert ops.thinlens_bwd_workspace_bytes(1, 3, 5, 64, 64, 11, False, False) == 0


def test_stack_gradient_is_the_fp32_sum_of_per_slice_calls():
    case = tc.CASES[1]
    img, depth, fds, dy = tc.case_inputs(case)
    lens = _lens(case)
    _, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dy)
    si = sd = None
    for s in range(fds.shape[1]):
        x, d, f = img.to(DEV).requires_grad_(True), depth.to(DEV).requires_grad_(True), fds[:, s].to(DEV).requires_grad_(True)
        dr.thinlens_render(lens, x, d, f).backward(dy[:, :, s].to(DEV))
        si = x.grad if si is None else si + x.grad
        sd = d.grad if sd is None else sd + d.grad
        assert torch.equal(f.grad, gf[:, s])
    assert torch.equal(si, gi) and torch.equal(sd, gd)


def test_fallback_domain_uses_the_tensor_form(margin):
    """C = 5, ks = 15 is outside the fused kernels: the forward is the tensor form, the gradients its torch autograd with this module's
    local_psf_render - within the same budget, nothing raised from inside backward, no silent zeros."""
    case = FALLBACK
    img, depth, fds, dym, share, o64, d32 = _reference(case)
    assert share <= tc.MAX_MASKED
    lens = _lens(case)
    out_fwd = _slice_loop(lens, img.to(DEV), depth.to(DEV), fds.to(DEV))
    out, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dym)
    assert torch.equal(out, out_fwd) and float(gd.abs().max()) > 0 and float(gf.abs().min()) > 0 and float(gi.abs().max()) > 0
    _check(case[0], (gi, gd, gf), o64, d32, out_fwd, margin)


def test_any_device_and_empty_batch():
    case = tc.CASES[3]
    img, depth, fds, dy = tc.case_inputs(case)
    lens = _lens(case)
    want = _gpu_grads(lens, img, depth, fds, dy)
    got = _gpu_grads(lens, img, depth, fds, dy, dev="cpu")                                # inputs on the CPU: results on the CPU
    assert all(g.device.type == "cpu" for g in got)
    for u, v in zip(got, want):
        assert torch.equal(u, v.cpu())
    x = torch.zeros((0, 3, 8, 8), device=DEV, requires_grad=True)
    d = torch.zeros((0, 1, 8, 8), device=DEV, requires_grad=True)
    f = torch.zeros((0, 2), device=DEV, requires_grad=True)
    out = dr.thinlens_render_stack(lens, x, d, f)
    assert out.shape == (0, 3, 2, 8, 8) and out.requires_grad
    out.sum().backward()
    assert x.grad.shape == x.shape and d.grad.shape == d.shape and f.grad.shape == f.shape


def test_opcheck():
    case = tc.CASES[3]
    img, depth, fds, dy = tc.case_inputs(case)
    lens = _lens(case)
    x, d, f, g = img.to(DEV), depth.to(DEV), fds.to(DEV), dy.to(DEV)
    consts = (11, 50.0, 4.0, lens.ps, float(lens.d_min), float(lens.d_max))
    torch.library.opcheck(torch.ops.aadff.thinlens_render_stack.default, (x, d, f, *consts))
    torch.library.opcheck(torch.ops.aadff.thinlens_render_stack_bwd.default, (x, d, f, g, *consts, True, True, True))
    torch.library.opcheck(torch.ops.aadff.thinlens_render_stack_bwd.default, (x, d, f, g, *consts, False, True, False))
    torch.library.opcheck(torch.ops.aadff.thinlens_render_stack_diff.default,
                          (x.clone().requires_grad_(True), d.clone().requires_grad_(True), f.clone().requires_grad_(True), *consts))
