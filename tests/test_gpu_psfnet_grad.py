"""GPU tests (run with `-m gpu` on an MI355X) of aadff.diffrender.psfnet_render / psfnet_render_stack: gradients of the fused
PSF-network renderer to the image, the depth map and the focus distances (csrc/psfnet_bwd.hip) against torch.autograd through the
oracle evaluated in float64 on the CPU (tests/psfnet_grad_common.py has the comparator, the cases and the cotangent mask).

Budget of every gradient (relative L2, masked cotangent): 4 x r x d32.
  d32  the oracle's own float32 autograd against its float64 autograd, same inputs, computed here;
  4    the project's allowance for another summation order of the same fp32 terms (tests/test_gpu_diffrender.py);
  r    max(1, e_fwd / d32_fwd): how far the EXISTING forward kernel's output (lens.render_stack) already is from float64, in units
       of the oracle's float32 - the backward uses the same fp16 hi/lo operand split and may be as far from plain fp32 as that.
Every (error, budget) is printed and goes through the `margin` fixture; DESIGN.md 4.8 has the table.
"""
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import aadff.diffrender as dr                              # noqa: E402
import psfnet_grad_common as pc                            # noqa: E402
from deeplens.psfnet import PSFNet                         # noqa: E402

DEV = "cuda:0"


def _lens(repo_root, H, W, wseed, mode="fp32"):
    """The renderers take the field axes from the image's shape; the lens's own sensor (square pixels required) plays no part in them."""
    net = PSFNet(os.path.join(repo_root, "lenses", "rf50mm", "lens.json"), sensor_res=(64, 64), kernel_size=pc.KS, device=DEV)
    net.psfnet.load_state_dict(pc.state_dict(wseed))
    net.mlp_precision = mode
    return net


def _gpu_grads(lens, img, depth, fds, dy, which=(True, True, True)):
    x = img.to(DEV).requires_grad_(which[0])
    d = depth.to(DEV).requires_grad_(which[1])
    f = fds.to(DEV).requires_grad_(which[2])
    out = dr.psfnet_render_stack(lens, x, d, f)
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return out.detach(), x.grad, d.grad, f.grad


_ORACLE = {}


def _reference(case):
    """Masked cotangent, float64 and float32 oracle results of a case (cached: two tests share them)."""
    if case[0] not in _ORACLE:
        sd, img, depth, fds, dy = pc.case_inputs(case)
        keep = pc.keep_rows(sd, depth, fds)
        share = 1.0 - float(keep.mean())
        dym = dy * keep
        o64 = pc.oracle_grads(sd, img, depth, fds, dym, torch.float64)
        o32 = pc.oracle_grads(sd, img, depth, fds, dym, torch.float32)
        _ORACLE[case[0]] = (img, depth, fds, dym, share, o64, [pc.rel_l2(a, b) for a, b in zip(o32, o64)])
    return _ORACLE[case[0]]


def _check(tag, got, o64, d32, out_fwd, margin):
    """got = (d_img, d_depth, d_foc); out_fwd = the existing forward kernel's output."""
    e_fwd = pc.rel_l2(out_fwd, o64[0])
    r = max(1.0, e_fwd / d32[0])
    print(f"\n{tag}: forward e_fwd {e_fwd:.3e} d32_fwd {d32[0]:.3e} r {r:.2f}")
    failed = []
    for name, g, ref, d in zip(("d_img", "d_depth", "d_foc"), got, o64[1:], d32[1:]):
        err, tol = pc.rel_l2(g.reshape(ref.shape), ref), 4.0 * r * d
        print(f"{tag}: {name} err {err:.3e} d32 {d:.3e} r {r:.2f} budget {tol:.3e}")
        try:
            margin(f"psfnet_grad {tag} {name}", err, tol)
        except AssertionError as e:                          # every figure is printed and recorded before the test fails
            failed.append(str(e))
    assert not failed, "; ".join(failed)


@pytest.mark.parametrize("case", pc.CASES, ids=[c[0] for c in pc.CASES])
def test_gradient_parity(case, repo_root, margin):
    name, N, C, S, H, W, wseed, _ = case
    img, depth, fds, dym, share, o64, d32 = _reference(case)
    assert share <= pc.MAX_MASKED, f"{share:.3%} of the rows are masked"
    lens = _lens(repo_root, H, W, wseed)
    out_fwd = lens.render_stack(img.to(DEV), depth.to(DEV), fds.to(DEV))
    out, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dym)
    assert torch.equal(out, out_fwd)
    _check(name, (gi, gd, gf), o64, d32, out_fwd, margin)


def test_gradient_parity_3d_branch(repo_root, margin):
    """psfnet_render with img [C,H,W], depth [H,W] and a scalar focus distance (a 0-d tensor that requires grad)."""
    case = ("3d_3x64x64", 1, 3, 1, 64, 64, 4321, [(-1500.0,)])
    img, depth, fds, dym, share, o64, d32 = _reference(case)
    assert share <= pc.MAX_MASKED
    lens = _lens(repo_root, 64, 64, 4321)
    out_fwd = lens.render(img[0].to(DEV), depth[0, 0].to(DEV), -1500.0)
    x = img[0].to(DEV).requires_grad_(True)
    d = depth[0, 0].to(DEV).requires_grad_(True)
    f = torch.tensor(-1500.0, device=DEV, requires_grad=True)
    out = dr.psfnet_render(lens, x, d, f)
    assert out.shape == out_fwd.shape == (3, 64, 64)
    out.backward(dym[0, :, 0].to(DEV))
    _check(case[0], (x.grad, d.grad, f.grad), o64, d32, out_fwd.reshape(1, 3, 1, 64, 64), margin)
    # 4-D branch of psfnet_render: the stack's slice
    x4, d4 = img.to(DEV).requires_grad_(True), depth.to(DEV).requires_grad_(True)
    f4 = torch.tensor([-1500.0], device=DEV, requires_grad=True)
    out4 = dr.psfnet_render(lens, x4, d4, f4)
    assert out4.shape == (1, 3, 64, 64)
    out4.backward(dym[:, :, 0].to(DEV))
    assert torch.equal(d4.grad[0, 0], d.grad) and torch.equal(x4.grad[0], x.grad) and torch.equal(f4.grad[0], f.grad)


def test_forward_bit_equal_with_and_without_grad(repo_root):
    sd, img, depth, fds, dy = pc.case_inputs(pc.CASES[1])
    lens = _lens(repo_root, 96, 128, 4321)
    want = lens.render_stack(img.to(DEV), depth.to(DEV), fds.to(DEV))
    x, d, f = img.to(DEV), depth.to(DEV), fds.to(DEV)
    assert torch.equal(dr.psfnet_render_stack(lens, x, d, f), want)                       # nothing requires grad
    with torch.no_grad():
        assert torch.equal(dr.psfnet_render_stack(lens, x.clone().requires_grad_(True), d, f), want)
    out = dr.psfnet_render_stack(lens, x, d.clone().requires_grad_(True), f)
    assert out.requires_grad and torch.equal(out.detach(), want)
    out = dr.psfnet_render_stack(lens, x.clone().requires_grad_(True), d, f.clone().requires_grad_(True))
    assert out.requires_grad and torch.equal(out.detach(), want)
    # psfnet_render against lens.render, 4-D branch
    want1 = lens.render(x, d, f[:, 1])
    assert torch.equal(dr.psfnet_render(lens, x, d, f[:, 1]), want1)
    out1 = dr.psfnet_render(lens, x, d.clone().requires_grad_(True), f[:, 1])
    assert out1.requires_grad and torch.equal(out1.detach(), want1)


def test_backward_is_deterministic(repo_root):
    sd, img, depth, fds, dy = pc.case_inputs(pc.CASES[1])
    lens = _lens(repo_root, 96, 128, 4321)
    a = _gpu_grads(lens, img, depth, fds, dy)
    b = _gpu_grads(lens, img, depth, fds, dy)
    for u, v in zip(a, b):
        assert torch.equal(u, v)
    with pytest.raises(RuntimeError):                                                    # double backward is not supported
        d = depth.to(DEV).requires_grad_(True)
        out = dr.psfnet_render_stack(lens, img.to(DEV), d, fds.to(DEV))
        (g,) = torch.autograd.grad(out.sum(), d, create_graph=True)
        g.sum().backward()


def test_depth_clamp_gives_exact_zero(repo_root):
    """depth2z = torch.clamp: a pixel at -100 mm or -30000 mm (outside [-20000, -200]) gets exactly 0; its neighbours do not.  A focus
    distance outside the range gets exactly 0 too."""
    sd, img, depth, fds, dy = pc.case_inputs(pc.CASES[0])
    depth = depth.clone()
    depth[0, 0, 10, 20], depth[0, 0, 40, 33] = -100.0, -30000.0
    fds = fds.clone()
    fds[0, 4] = -25000.0
    lens = _lens(repo_root, 64, 64, 4321)
    _, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dy)
    assert gd[0, 0, 10, 20].item() == 0.0 and gd[0, 0, 40, 33].item() == 0.0
    for y, x in ((10, 19), (10, 21), (9, 20), (11, 20), (40, 32), (40, 34), (39, 33), (41, 33)):
        assert gd[0, 0, y, x].item() != 0.0
    assert gf[0, 4].item() == 0.0 and all(gf[0, s].item() != 0.0 for s in range(4))
    assert torch.isfinite(gd).all() and torch.isfinite(gi).all()


def test_gradient_subsets(repo_root):
    sd, img, depth, fds, dy = pc.case_inputs(pc.CASES[0])
    lens = _lens(repo_root, 64, 64, 4321)
    _, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dy)
    _, gi1, gd1, gf1 = _gpu_grads(lens, img, depth, fds, dy, which=(False, True, False))
    assert gi1 is None and gf1 is None and torch.equal(gd1, gd)
    _, gi2, gd2, gf2 = _gpu_grads(lens, img, depth, fds, dy, which=(True, False, False))
    assert gd2 is None and gf2 is None and torch.equal(gi2, gi)
    _, gi3, gd3, gf3 = _gpu_grads(lens, img, depth, fds, dy, which=(False, False, True))
    assert gi3 is None and gd3 is None and torch.equal(gf3, gf)
    # no PSF workspace unless the image wants a gradient: 4 bytes per row + 4 per 64 rows against one slice of PSFs on top
    from aadff import ops
    rows = 5 * 64 * 64
    assert ops.psfnet_bwd_workspace_bytes(1, 5, 3, 64, 64, 11, True, False) == 4 * (rows + rows // 64)
    assert ops.psfnet_bwd_workspace_bytes(1, 5, 3, 64, 64, 11, False, True) == 4 * 64 * 64 * (4 + 121)


@pytest.mark.parametrize("case", pc.CASES[:2], ids=[c[0] for c in pc.CASES[:2]])
def test_torch_mode_agrees_and_gives_parameter_gradients(case, repo_root, margin):
    name, N, C, S, H, W, wseed, _ = case
    img, depth, fds, dym, share, o64, d32 = _reference(case)
    lens = _lens(repo_root, H, W, wseed, mode="torch")
    fwd = _lens(repo_root, H, W, wseed)
    out_fwd = fwd.render_stack(img.to(DEV), depth.to(DEV), fds.to(DEV))
    out, gi, gd, gf = _gpu_grads(lens, img, depth, fds, dym)
    _check("torch_mode " + name, (gi, gd, gf), o64, d32, out_fwd, margin)
    grads = [p.grad for p in lens.psfnet.parameters()]
    assert all(g is not None and torch.isfinite(g).all() for g in grads) and any(float(g.abs().max()) > 0 for g in grads)
    # the fused path leaves the parameters alone
    _gpu_grads(fwd, img, depth, fds, dym)
    assert all(p.grad is None for p in fwd.psfnet.parameters())


@pytest.mark.parametrize("mode", ["fp16", "bf16"])
def test_refused_modes(mode, repo_root):
    sd, img, depth, fds, dy = pc.case_inputs(pc.CASES[0])
    lens = _lens(repo_root, 64, 64, 4321, mode=mode)
    with pytest.raises(ValueError, match="'fp32'.*'torch'"):
        dr.psfnet_render_stack(lens, img.to(DEV), depth.to(DEV).requires_grad_(True), fds.to(DEV))
    with pytest.raises(ValueError, match="'fp32'.*'torch'"):
        dr.psfnet_render(lens, img.to(DEV), depth.to(DEV).requires_grad_(True), fds[:, 0].to(DEV))
    with torch.no_grad():                                                                # no gradient asked for: the lens's own renderer
        assert dr.psfnet_render_stack(lens, img.to(DEV), depth.to(DEV), fds.to(DEV)).shape == (1, 3, 5, 64, 64)


def test_unsupported_network_is_refused(repo_root):
    sd, img, depth, fds, dy = pc.case_inputs(pc.CASES[0])
    lens = _lens(repo_root, 64, 64, 4321)
    lens.psfnet.net[1] = torch.nn.Tanh()                                                 # psfnet_pack.supported is False
    with pytest.raises(ValueError, match="'fp32'.*'torch'"):
        dr.psfnet_render_stack(lens, img.to(DEV), depth.to(DEV).requires_grad_(True), fds.to(DEV))
