"""Shared by tests/test_thinlens_grad_host.py and tests/test_gpu_thinlens_grad.py (not a test module): the cases of the thin-lens
gradient tests, their comparator and the cotangent mask.

Comparator: oracle.psfnet.thinlens_render (the reference's tensor form, deeplens/psfnet.py:549-570) under torch.autograd, in float64
and in float32, one slice at a time, on aadff.synth scenes.

The PSF of a row (n, slice, y, x) is a Gaussian cut at rho < r^2, so the rendered pixel and its gradients JUMP where r^2 crosses a sum
of two squares; the coc floor (0.1 px) and the depth clamp are kinks.  A last-bit difference of r^2 there changes a whole ring of taps.
The tests therefore zero the cotangent on every row where, in float64,
  * r^2 is within relative 1e-5 of a value a^2 + b^2 with 0 <= a, b <= ks // 2, or
  * the unclamped coc in pixels is within relative 1e-5 of 0.1, or
  * the (sign-adjusted) depth is within relative 1e-6 of d_min or d_max.
An output pixel depends on its own row's PSF only, so such rows drop out of d_depth and d_foc completely.  The excluded share must stay
<= 0.5 % (MAX_MASKED), and the oracle's own float32-vs-float64 distance of every gradient <= 5e-5 (MAX_D32): a case whose PSF is nearly
uniform over the window has an almost vanishing true gradient and measures rounding noise, not the kernel."""
import numpy as np
import torch

from aadff.synth import synth_depth_mm, synth_rgb
from oracle import psfnet as opsf

MAX_MASKED, MAX_D32 = 0.005, 5e-5
FOC_LEN, SENSOR_H = 50.0, 24.0
D_MIN, D_MAX = float(opsf.DMIN), float(opsf.DMAX)

# name, N, C, S, H, W, ks, sensor_res, fnum, focus distances [N][S] (mm, > 0), sign of the convention, (dmin, dmax) of the scene in mm
CASES = [
    ("1x3x64x64_S5_ks11", 1, 3, 5, 64, 64, 11, (256, 256), 2.8, [(600.0, 900.0, 1500.0, 2500.0, 4000.0)], -1, (500.0, 5000.0)),
    ("2x3x96x128_S3_ks7", 2, 3, 3, 96, 128, 7, (256, 256), 4.0, [(700.0, 1200.0, 3000.0), (800.0, 2000.0, 4500.0)], -1, (500.0, 5000.0)),
    ("1x1x67x131_S1_ks13", 1, 1, 1, 67, 131, 13, (480, 640), 2.8, [(1500.0,)], +1, (500.0, 5000.0)),
    ("2x1x48x80_S3_ks11_pos", 2, 1, 3, 48, 80, 11, (480, 640), 4.0, [(650.0, 1100.0, 2600.0), (900.0, 1700.0, 3800.0)], +1, (500.0, 5000.0)),
    ("1x3x72x100_S5_ks13_clamp", 1, 3, 5, 72, 100, 13, (256, 256), 2.8, [(400.0, 800.0, 2000.0, 6000.0, 15000.0)], -1, (120.0, 30000.0)),
]


def tt(a):
    return torch.from_numpy(np.ascontiguousarray(a))


def lens_args(case):
    """(foc_len, fnum, ks, sensor_size, sensor_res) of a case; the pixel size is sensor_size[0] / sensor_res[0]."""
    ks, res, fnum = case[6], case[7], case[8]
    return FOC_LEN, fnum, ks, [SENSOR_H, SENSOR_H * res[1] / res[0]], res


def case_inputs(case):
    """(img [N,C,H,W], depth [N,1,H,W], fds [N,S], dy [N,C,S,H,W]) float32 on the CPU, depth and fds in the case's sign convention."""
    name, N, C, S, H, W, ks, res, fnum, fds, sign, (dmin, dmax) = case
    img = torch.stack([torch.cat([tt(synth_rgb(H, W, seed=11 + 100 * n + 7 * j)) for j in range((C + 2) // 3)])[:C] for n in range(N)])
    depth = torch.stack([tt(synth_depth_mm(H, W, seed=12 + 100 * n, dmin=dmin, dmax=dmax))[None] for n in range(N)])
    dy = torch.randn((N, C, S, H, W), generator=torch.Generator().manual_seed(31))
    return img, float(sign) * depth, float(sign) * torch.tensor(fds, dtype=torch.float32), dy


def oracle_grads(case, img, depth, fds, dy, dtype):
    """(out, d_img, d_depth, d_foc) of the oracle in `dtype`; one slice at a time (bounded memory), summed in slice order."""
    foc_len, fnum, ks, ssize, sres = lens_args(case)
    x = img.detach().to(dtype).requires_grad_(True)
    d = depth.detach().to(dtype).requires_grad_(True)
    f = fds.detach().to(dtype).requires_grad_(True)
    outs, gi, gd, gf = [], torch.zeros_like(x), torch.zeros_like(d), []
    for s in range(fds.shape[1]):
        out = opsf.thinlens_render(x, d, f[:, s], foc_len, fnum, ks, ssize, sres)
        a, b, c = torch.autograd.grad(out, (x, d, f), dy[:, :, s].to(dtype))
        gi, gd = gi + a, gd + b
        gf.append(c[:, s])
        outs.append(out.detach())
    return torch.stack(outs, dim=2), gi, gd, torch.stack(gf, dim=1)


def coc_chain(case, depth, fds):
    """float64 per-row quantities of `Mathematics` 1-2: (sg, d [N,1,1,H,W], f [N,1,S,1,1], dc, K, cp unclamped [N,1,S,H,W], r)."""
    foc_len, fnum, ks, ssize, sres = lens_args(case)
    ps = ssize[0] / sres[0]
    sg = -1.0 if bool((depth < 0).any()) else 1.0
    d = sg * depth.double().unsqueeze(2)
    f = sg * fds.double()[:, None, :, None, None]
    dc = d.clamp(D_MIN, D_MAX)
    A = foc_len / fnum
    K = A * foc_len / (f - foc_len)
    cp = K * (dc - f).abs() / dc / ps
    r = cp.clamp(min=0.1) / 2
    return sg, d, f, dc, K, cp, r


def keep_rows(case, depth, fds):
    """[N,1,S,H,W] float32 mask: 0 on the rows next to a jump or a kink (module docstring)."""
    p = case[6] // 2
    sg, d, f, dc, K, cp, r = coc_chain(case, depth, fds)
    r2 = r * r
    bad = torch.zeros_like(r2, dtype=torch.bool)
    for q in sorted({a * a + b * b for a in range(p + 1) for b in range(p + 1)} - {0}):
        bad |= (r2 - q).abs() <= 1e-5 * q
    bad |= (cp - 0.1).abs() <= 1e-5 * 0.1
    bad |= (((d - D_MIN).abs() <= 1e-6 * D_MIN) | ((d - D_MAX).abs() <= 1e-6 * D_MAX)).expand_as(bad)
    return (~bad).float()


def closed_form_grads(case, img, depth, fds, dy):
    """(d_img, d_depth, d_foc) from the closed forms of DESIGN.md 4.9 in float64 torch (no autograd)."""
    foc_len, fnum, ks, ssize, sres = lens_args(case)
    ps, p = ssize[0] / sres[0], ks // 2
    N, C, H, W = img.shape
    S = fds.shape[1]
    sg, d, f, dc, K, cp, r = coc_chain(case, depth, fds)
    A = foc_len / fnum
    k = torch.arange(ks, dtype=torch.float64) - p
    rho = (k[:, None] ** 2 + k[None, :] ** 2)                                    # [ks,ks], (a, e)
    r_ = r[:, 0, :, :, :, None, None]                                            # [N,S,H,W,1,1]
    w = (rho < r_ ** 2) * torch.exp(-rho / (2 * r_ ** 2))
    pk = w / w.sum((-1, -2), keepdim=True)                                       # [N,S,H,W,ks,ks]
    x, g = img.double(), dy.double()
    rows = [(torch.arange(H) + a - p).clamp(0, H - 1) for a in range(ks)]
    cols = [(torch.arange(W) + e - p).clamp(0, W - 1) for e in range(ks)]
    rho_bar = (pk * rho).sum((-1, -2))                                           # [N,S,H,W]
    d_r = torch.zeros((N, S, H, W), dtype=torch.float64)
    d_img = torch.zeros_like(x)
    for a in range(ks):
        for e in range(ks):
            head = torch.einsum("ncshw,nchw->nshw", g, x[:, :, rows[a]][:, :, :, cols[e]])        # g_k
            d_r += pk[..., a, e] * (rho[a, e] - rho_bar) * head
            t = torch.einsum("ncshw,nshw->nchw", g, pk[..., a, e])
            t = torch.zeros_like(t).index_add_(2, rows[a], t)
            d_img.index_add_(3, cols[e], t)
    d_r = (d_r / r[:, 0] ** 3).unsqueeze(1)                                      # [N,1,S,H,W]
    d_coc = torch.where(cp >= 0.1, d_r / (2 * ps), torch.zeros_like(d_r))
    sgn = torch.sign(dc - f)
    dcoc_ddc = K * sgn * f / dc ** 2
    dcoc_df = -A * foc_len * (sgn / (dc * (f - foc_len)) + (dc - f).abs() / (dc * (f - foc_len) ** 2))
    inside = ((d >= D_MIN) & (d <= D_MAX)).double()
    d_depth = sg * (d_coc * dcoc_ddc * inside).sum(2)                            # [N,1,H,W]
    d_foc = sg * (d_coc * dcoc_df).sum((1, 3, 4))                                # [N,S]
    return d_img, d_depth, d_foc


def rel_l2(a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return float((a - b).norm() / b.norm())
