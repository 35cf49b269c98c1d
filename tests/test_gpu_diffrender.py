"""GPU tests (run with `-m gpu` on an MI355X) of aadff.diffrender: gradients of the image-space PSF operators from the HIP
kernels of csrc/conv_bwd.hip and csrc/gather.hip against torch.autograd through oracle/conv.py evaluated in float64 on the CPU.

Tolerance of every gradient: 4 x d32, where d32 is the relative-L2 distance of the oracle's OWN float32 autograd from its
float64 autograd on the same inputs, computed here; the factor 4 allows for a different summation order of the same fp32
terms.  The kernels carry plain fp32 operands, so no floor applies.  Every test prints the measured distance next to d32 and records
it through the `margin` fixture (terminal summary); DESIGN.md 4.7 has the expected figures.
"""
import importlib

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import aadff.diffrender as dr                              # noqa: E402
from aadff import ops as _ops                               # noqa: E402,F401
from oracle import conv as oconv                            # noqa: E402
rp = importlib.import_module("deeplens.render_psf")         # the package re-exports a same-named function

DEV = "cuda:0"


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())


def _gen(seed):
    return torch.Generator().manual_seed(seed)


def _map_inputs(seed, B, C, S, H, W, grid, ks):
    """image = seeded rand, PSFs = seeded rand normalised per PSF, dy = seeded randn (all on the CPU, float32)."""
    g = _gen(seed)
    img = torch.rand((B, C, H, W), generator=g)
    p = torch.rand((S, C, grid, grid, ks, ks), generator=g)
    p = p / p.sum((-1, -2), keepdim=True)
    maps = p.permute(0, 1, 2, 4, 3, 5).reshape(S, C, grid * ks, grid * ks).contiguous()
    dy = torch.randn((B, C, S, H, W), generator=g)
    return img, maps, dy


def _oracle_map_grads(img, maps, dy, grid, dtype):
    x = img.detach().clone().to(dtype).requires_grad_(True)
    m = maps.detach().clone().to(dtype).requires_grad_(True)
    out = torch.stack([oconv.render_psf_map(x, m[s], grid) for s in range(m.shape[0])], dim=2)
    return torch.autograd.grad(out, (x, m), dy.to(dtype))


def _gpu_map_grads(img, maps, dy, grid, which=(True, True)):
    x = img.to(DEV).requires_grad_(which[0])
    m = maps.to(DEV).requires_grad_(which[1])
    out = dr.render_psf_map_stack(x, m, grid)
    out.backward(dy.to(DEV))
    torch.cuda.synchronize()
    return x.grad, m.grad


MAP_CASES = [
    # name, B, C, S, H, W, grid, ks
    ("256_g11_ks11", 1, 3, 1, 256, 256, 11, 11),
    ("250x330_g7_ks21_B2", 2, 3, 1, 250, 330, 7, 21),
    ("1024_g11_ks11", 1, 3, 1, 1024, 1024, 11, 11),
    ("1024_g1_ks11_render_psf", 1, 3, 1, 1024, 1024, 1, 11),
    ("1024_g11_ks11_stack10", 1, 3, 10, 1024, 1024, 11, 11),
    ("50x46_g3_ks5_unequal", 2, 3, 1, 50, 46, 3, 5),
    ("67x131_g4_ks3", 1, 3, 1, 67, 131, 4, 3),
    ("67x131_g5_ks11_stack3", 1, 3, 3, 67, 131, 5, 11),
    ("120x100_g2_ks51_C1", 1, 1, 1, 120, 100, 2, 51),
    ("24x24_g11_ks11", 1, 3, 1, 24, 24, 11, 11),
    ("27x29_g2_ks51_folds_overlap", 2, 1, 2, 27, 29, 2, 51),
]


@pytest.mark.parametrize("case", MAP_CASES, ids=[c[0] for c in MAP_CASES])
def test_map_gradient_parity(case, margin):
    name, B, C, S, H, W, grid, ks = case
    img, maps, dy = _map_inputs(11, B, C, S, H, W, grid, ks)
    gi64, gp64 = _oracle_map_grads(img, maps, dy, grid, torch.float64)
    gi32, gp32 = _oracle_map_grads(img, maps, dy, grid, torch.float32)
    d32_img, d32_psf = rel_l2(gi32, gi64), rel_l2(gp32, gp64)
    gi, gp = _gpu_map_grads(img, maps, dy, grid)
    assert gi.shape == img.shape and gp.shape == maps.shape and gi.dtype == gp.dtype == torch.float32
    e_img, e_psf = rel_l2(gi, gi64), rel_l2(gp, gp64)
    print(f"\n[diffrender] map {name}: d_img {e_img:.3e} (oracle fp32 {d32_img:.3e})  d_psf {e_psf:.3e} (oracle fp32 {d32_psf:.3e})")
    margin(f"diffrender map {name} d_img", e_img, 4 * d32_img)
    margin(f"diffrender map {name} d_psf", e_psf, 4 * d32_psf)
    if S == 1:
        # the single-slice and single-PSF front ends are the same operator
        x = img.to(DEV).requires_grad_(True)
        m = maps[0].to(DEV).requires_grad_(True)
        out = dr.render_psf(x, m) if grid == 1 else dr.render_psf_map(x, m, grid)
        assert out.shape == img.shape
        out.backward(dy[:, :, 0].to(DEV))
        assert torch.equal(x.grad, gi) and torch.equal(m.grad, gp[0])


def test_stack_d_img_is_the_sum_over_slices():
    """The stack kernel finishes each slice's taps and then adds the slice results in slice order: bit-equal to the fp32 sum of the
    per-slice gradients taken in that order; the PSF gradients of a slice do not depend on the other slices at all."""
    B, C, S, H, W, grid, ks = 1, 3, 10, 1024, 1024, 11, 11
    img, maps, dy = _map_inputs(5, B, C, S, H, W, grid, ks)
    gi, gp = _gpu_map_grads(img, maps, dy, grid)
    total = None
    for s in range(S):
        gi_s, gp_s = _gpu_map_grads(img, maps[s:s + 1], dy[:, :, s:s + 1].contiguous(), grid)
        total = gi_s if total is None else total + gi_s
        assert torch.equal(gp_s[0], gp[s])
    assert torch.equal(total, gi)


def _local_inputs(seed, B, C, H, W, ks):
    g = _gen(seed)
    img = torch.rand((B, C, H, W), generator=g)
    p = torch.rand((B, H, W, ks, ks), generator=g)
    p = p / p.sum((-1, -2), keepdim=True)
    dy = torch.randn((B, C, H, W), generator=g)
    return img, p, dy


def _oracle_local_grads(img, psf, dy, ks, dtype):
    x = img.detach().clone().to(dtype).requires_grad_(True)
    p = psf.detach().clone().to(dtype).requires_grad_(True)
    return torch.autograd.grad(oconv.local_psf_render(x, p, ks), (x, p), dy.to(dtype))


def _gpu_local_grads(img, psf, dy, ks, which=(True, True)):
    x = img.to(DEV).requires_grad_(which[0])
    p = psf.to(DEV).requires_grad_(which[1])
    dr.local_psf_render(x, p, kernel_size=ks).backward(dy.to(DEV))
    torch.cuda.synchronize()
    return x.grad, p.grad


LOCAL_CASES = [
    ("2x3x120x160_ks11", 2, 3, 120, 160, 11),
    ("1x3x480x640_ks11", 1, 3, 480, 640, 11),
    ("1x1x67x131_ks5", 1, 1, 67, 131, 5),
    ("2x5x40x50_ks7", 2, 5, 40, 50, 7),
    ("1x3x9x70_ks21_window_taller_than_image", 1, 3, 9, 70, 21),
    ("1x2x33x31_ks3", 1, 2, 33, 31, 3),
]


@pytest.mark.parametrize("case", LOCAL_CASES, ids=[c[0] for c in LOCAL_CASES])
def test_local_gradient_parity(case, margin):
    name, B, C, H, W, ks = case
    img, psf, dy = _local_inputs(13, B, C, H, W, ks)
    gi64, gp64 = _oracle_local_grads(img, psf, dy, ks, torch.float64)
    gi32, gp32 = _oracle_local_grads(img, psf, dy, ks, torch.float32)
    d32_img, d32_psf = rel_l2(gi32, gi64), rel_l2(gp32, gp64)
    gi, gp = _gpu_local_grads(img, psf, dy, ks)
    assert gi.shape == img.shape and gp.shape == psf.shape
    e_img, e_psf = rel_l2(gi, gi64), rel_l2(gp, gp64)
    print(f"\n[diffrender] local {name}: d_img {e_img:.3e} (oracle fp32 {d32_img:.3e})  d_psf {e_psf:.3e} (oracle fp32 {d32_psf:.3e})")
    margin(f"diffrender local {name} d_img", e_img, 4 * d32_img)
    margin(f"diffrender local {name} d_psf", e_psf, 4 * d32_psf)


# ================================================================= structure
def test_needs_input_grad_selects_the_kernels():
    img, maps, dy = _map_inputs(3, 2, 3, 3, 70, 90, 3, 11)
    gi, gp = _gpu_map_grads(img, maps, dy, 3)
    gi_only, none_p = _gpu_map_grads(img, maps, dy, 3, which=(True, False))
    none_i, gp_only = _gpu_map_grads(img, maps, dy, 3, which=(False, True))
    assert none_p is None and none_i is None
    assert torch.equal(gi_only, gi) and torch.equal(gp_only, gp)
    img, psf, dy = _local_inputs(3, 2, 3, 40, 50, 7)
    gi, gp = _gpu_local_grads(img, psf, dy, 7)
    gi_only, none_p = _gpu_local_grads(img, psf, dy, 7, which=(True, False))
    none_i, gp_only = _gpu_local_grads(img, psf, dy, 7, which=(False, True))
    assert none_p is None and none_i is None
    assert torch.equal(gi_only, gi) and torch.equal(gp_only, gp)


def test_gradients_are_bit_reproducible_also_beside_a_busy_stream():
    img, maps, dy = _map_inputs(7, 1, 3, 4, 512, 512, 11, 11)
    a = _gpu_map_grads(img, maps, dy, 11)
    b = _gpu_map_grads(img, maps, dy, 11)
    assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1])
    limg, lpsf, ldy = _local_inputs(7, 1, 3, 96, 128, 11)
    la = _gpu_local_grads(limg, lpsf, ldy, 11)
    lb = _gpu_local_grads(limg, lpsf, ldy, 11)
    assert torch.equal(la[0], lb[0]) and torch.equal(la[1], lb[1])
    # once more while a second stream runs the forward stack convolution (matrix-core waves on the same CUs)
    big, bmaps, _ = _map_inputs(8, 1, 3, 10, 1024, 1024, 11, 11)
    big, bmaps = big.to(DEV), bmaps.to(DEV)
    side = torch.cuda.Stream(device=DEV)
    dimg, dmaps, ddy, dlimg, dlpsf, dldy = (t.to(DEV) for t in (img, maps, dy, limg, lpsf, ldy))
    torch.cuda.synchronize()
    got = []
    for _ in range(6):                                    # nothing below waits for the device: the two streams overlap
        with torch.cuda.stream(side):
            for _ in range(12):
                rp.render_psf_map_stack(big, bmaps, 11)
        got.append(torch.ops.aadff.render_psf_map_stack_bwd(dimg, dmaps, ddy, 11, True, True)
                   + torch.ops.aadff.local_psf_render_bwd(dlimg, dlpsf, dldy, 11, True, True))
    torch.cuda.synchronize()
    for c in got:
        assert torch.equal(a[0], c[0]) and torch.equal(a[1], c[1]) and torch.equal(la[0], c[2]) and torch.equal(la[1], c[3])


def test_locality_of_the_map_gradients():
    """dy non-zero inside one patch only: d_psf is exactly zero outside that patch's ks x ks tile, d_img exactly zero farther than
    p pixels from the patch."""
    B, C, S, H, W, grid, ks = 1, 3, 2, 150, 130, 5, 11
    p = ks // 2
    img, maps, dy = _map_inputs(2, B, C, S, H, W, grid, ks)
    hb, wb = oconv.patch_bounds(H, grid), oconv.patch_bounds(W, grid)
    for (i, j) in ((2, 1), (0, 4)):
        d = torch.zeros_like(dy)
        d[..., hb[i]:hb[i + 1], wb[j]:wb[j + 1]] = dy[..., hb[i]:hb[i + 1], wb[j]:wb[j + 1]]
        gi, gp = _gpu_map_grads(img, maps, d, grid)
        gp = gp.clone()
        assert gp[:, :, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks].abs().max().item() > 0
        gp[:, :, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks] = 0
        assert gp.abs().max().item() == 0.0
        gi = gi.clone()
        y0, y1, x0, x1 = max(hb[i] - p, 0), min(hb[i + 1] + p, H), max(wb[j] - p, 0), min(wb[j + 1] + p, W)
        assert gi[..., y0:y1, x0:x1].abs().max().item() > 0
        gi[..., y0:y1, x0:x1] = 0
        assert gi.abs().max().item() == 0.0


def test_delta_psfs_pass_dy_through():
    """Delta PSFs: the forward is the identity, so d_img == dy - exactly, the kernels are plain fp32."""
    B, C, H, W, grid, ks = 2, 3, 100, 90, 4, 11
    g = _gen(4)
    img, dy = torch.rand((B, C, H, W), generator=g), torch.randn((B, C, 1, H, W), generator=g)
    delta = torch.zeros(1, C, grid, grid, ks, ks)
    delta[..., ks // 2, ks // 2] = 1
    delta = delta.permute(0, 1, 2, 4, 3, 5).reshape(1, C, grid * ks, grid * ks).contiguous()
    gi, _ = _gpu_map_grads(img, delta, dy, grid, which=(True, False))
    assert torch.equal(gi.cpu(), dy[:, :, 0])
    ld = torch.zeros(B, H, W, ks, ks)
    ld[..., ks // 2, ks // 2] = 1
    gi, _ = _gpu_local_grads(img, ld, dy[:, :, 0].contiguous(), ks, which=(True, False))
    assert torch.equal(gi.cpu(), dy[:, :, 0])


def test_forward_is_the_forward_only_kernel():
    img, maps, _ = _map_inputs(6, 2, 3, 4, 200, 180, 7, 11)
    limg, lpsf, _ = _local_inputs(6, 2, 3, 96, 80, 11)
    img, maps, limg, lpsf = img.to(DEV), maps.to(DEV), limg.to(DEV), lpsf.to(DEV)
    with torch.no_grad():
        want = [rp.render_psf(img, maps[0, :, :11, :11]), rp.render_psf_map(img, maps[0], 7), rp.render_psf_map_stack(img, maps, 7),
                rp.local_psf_render(limg, lpsf, kernel_size=11), rp.local_psf_render_high_res(limg, lpsf, patch_size=[40, 48], kernel_size=11)]

    def run(x, m, lx, lp):
        return [dr.render_psf(x, m[0, :, :11, :11]), dr.render_psf_map(x, m[0], 7), dr.render_psf_map_stack(x, m, 7),
                dr.local_psf_render(lx, lp, kernel_size=11), dr.local_psf_render_high_res(lx, lp, patch_size=[40, 48], kernel_size=11)]

    with torch.no_grad():                                            # inputs that require grad, grad mode off
        got = run(img.clone().requires_grad_(True), maps.clone().requires_grad_(True), limg.clone().requires_grad_(True), lpsf.clone().requires_grad_(True))
    assert all(torch.equal(g, w) and not g.requires_grad for g, w in zip(got, want))
    got = run(img, maps, limg, lpsf)                                  # grad mode on, nothing requires grad
    assert all(torch.equal(g, w) and not g.requires_grad for g, w in zip(got, want))
    got = run(img.clone().requires_grad_(True), maps, limg, lpsf.clone().requires_grad_(True))      # the differentiable ops themselves
    assert all(torch.equal(g, w) and g.requires_grad for g, w in zip(got, want))
    # integer images are converted as in the forward and get no gradient
    m = maps[0].clone().requires_grad_(True)
    u8 = (img * 255).to(torch.uint8)
    out = dr.render_psf_map(u8, m, 7)
    assert torch.equal(out, rp.render_psf_map(u8, maps[0], 7))
    out.sum().backward()
    assert m.grad is not None and m.grad.shape == m.shape


def test_high_res_gradients_are_the_per_tile_composition():
    img, psf, dy = _local_inputs(9, 1, 3, 70, 100, 5)
    ps = [32, 48]
    x, p = img.to(DEV).requires_grad_(True), psf.to(DEV).requires_grad_(True)
    dr.local_psf_render_high_res(x, p, patch_size=ps, kernel_size=5).backward(dy.to(DEV))
    gi, gp = torch.zeros_like(img), torch.zeros_like(psf)
    for i0 in range(0, 70, ps[0]):
        for j0 in range(0, 100, ps[1]):
            i1, j1 = min(i0 + ps[0], 70), min(j0 + ps[1], 100)
            ti, tp = _gpu_local_grads(img[:, :, i0:i1, j0:j1].contiguous(), psf[:, i0:i1, j0:j1].contiguous(), dy[:, :, i0:i1, j0:j1].contiguous(), 5)
            gi[:, :, i0:i1, j0:j1], gp[:, i0:i1, j0:j1] = ti.cpu(), tp.cpu()
    assert torch.equal(x.grad.cpu(), gi) and torch.equal(p.grad.cpu(), gp)
    # and the seams are the reference's: same gradients as autograd through the oracle's tiled function
    xo, po = img.double().requires_grad_(True), psf.double().requires_grad_(True)
    oi, op = torch.autograd.grad(oconv.local_psf_render_high_res(xo, po, ps, 5), (xo, po), dy.double())
    assert rel_l2(x.grad, oi) <= 1e-6 and rel_l2(p.grad, op) <= 1e-6


def test_ops_schema_fake_autograd_and_compile():
    img, maps, dy = _map_inputs(10, 1, 3, 4, 48, 40, 3, 11)
    limg, lpsf, ldy = _local_inputs(10, 1, 3, 48, 40, 5)
    img, maps, dy, limg, lpsf, ldy = (t.to(DEV) for t in (img, maps, dy, limg, lpsf, ldy))
    tests = ("test_schema", "test_faketensor", "test_autograd_registration", "test_aot_dispatch_dynamic")
    torch.library.opcheck(torch.ops.aadff.render_psf_map_stack_bwd.default, (img, maps, dy, 3, True, True), test_utils=tests)
    torch.library.opcheck(torch.ops.aadff.render_psf_map_stack_bwd.default, (img, maps, dy, 3, False, True), test_utils=tests)
    torch.library.opcheck(torch.ops.aadff.local_psf_render_bwd.default, (limg, lpsf, ldy, 5, True, True), test_utils=tests)
    torch.library.opcheck(torch.ops.aadff.local_psf_render_bwd.default, (limg, lpsf, ldy, 5, True, False), test_utils=tests)
    rg = lambda t: t.clone().requires_grad_(True)                    # noqa: E731
    torch.library.opcheck(torch.ops.aadff.render_psf_map_stack_diff.default, (rg(img), rg(maps), 3), test_utils=tests)
    torch.library.opcheck(torch.ops.aadff.local_psf_render_diff.default, (rg(limg), rg(lpsf), 5), test_utils=tests)

    def f(x, m, p):
        a = torch.ops.aadff.render_psf_map_stack_diff(x, m, 3)           # [1,3,4,H,W]
        return (torch.ops.aadff.local_psf_render_diff(a[:, :, 0].contiguous(), p, 5) * ldy).sum() + (a * dy).sum()

    def grads(fn):
        x, m, p = rg(img), rg(maps), rg(lpsf)
        out = fn(x, m, p)
        out.backward()
        return out.detach(), x.grad, m.grad, p.grad

    want = grads(f)
    got = grads(torch.compile(f, backend="aot_eager", fullgraph=True))
    assert all(torch.equal(g, w) for g, w in zip(got, want))
    # double backward is not supported: it raises instead of returning wrong numbers
    x, m = rg(img), rg(maps)
    gx, = torch.autograd.grad(dr.render_psf_map_stack(x, m, 3), x, dy, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gx.sum(), m)
    lx, lp = rg(limg), rg(lpsf)
    gp, = torch.autograd.grad(dr.local_psf_render(lx, lp, kernel_size=5), lp, ldy, create_graph=True)
    with pytest.raises(RuntimeError):
        torch.autograd.grad(gp.sum(), lx)


def test_forward_only_names_still_refuse():
    img = torch.rand(1, 3, 32, 32, device=DEV)
    with pytest.raises(RuntimeError, match="forward-only"):
        rp.render_psf_map(img.clone().requires_grad_(True), torch.rand(3, 6, 6, device=DEV), 2)
    with pytest.raises(RuntimeError, match="forward-only"):
        rp.local_psf_render(img.clone().requires_grad_(True), torch.rand(1, 32, 32, 3, 3, device=DEV), kernel_size=3)
    y = torch.ops.aadff.render_psf_map(img.clone().requires_grad_(True), torch.rand(3, 6, 6, device=DEV), 2)
    with pytest.raises(RuntimeError):
        y.sum().backward()
