"""Shared by tests/test_local_gather_host.py and tests/test_gpu_local_gather.py (not a test module): the cases, inputs, comparators and
budgets of the forward tests of the per-pixel PSF gather (aadff_local_psf_render, csrc/gather.hip) and of the thin-lens kernel.

Comparator: oracle.conv.local_psf_render (the reference's unfold form) in float64.

Unit of every relative-L2 budget: d32seq = rel_l2(sequential32, oracle64), where sequential32 restates the operation in float32 in the
order of the direct and the generic kernel: replicate padding, taps in row-major (u, v) order, one fused multiply-add per tap.  The
oracle's own float32 result is NOT the unit: torch sums the ks^2 products in blocks, and a sequential chain is 1 .. 10 x further from
float64 than that as ks goes from 3 to 47 (DESIGN.md 4.9.1 has the table) - "4 x d32 of the oracle" would pass ks 3 with enormous room
and fail a correct ks 31.

Elementwise bound (derived, not measured): a float32 sum of n exactly formed products (fma) in ANY order is within
n * 2^-24 * sum|x w| of the exact sum (every one of the at most n partial sums an element passes through is rounded once, to within
2^-24 of a value not above sum|x w|, to first order); the second term 2^-24 |out| covers the last rounding of a split sum (the waves of
the LDS-DMA form add their partial sums) and the first-order slack.  No element is excluded from it.
"""
import numpy as np
import torch

from oracle import conv as oconv

import thinlens_grad_common as tc

U = 2.0 ** -24                                      # unit roundoff of float32

TEMPLATED_KS = (3, 5, 7, 9, 11, 13)


def _cases():
    out = []
    for ks in TEMPLATED_KS:
        out.append((2, 3, 9, 132, ks))              # LDS-DMA, three runs (the middle one has no clamped lane), last run of 4 pixels
        out.append((2, 3, 9, 131, ks))              # direct, the same geometry with a ragged last run of 3
    for ks in (5, 11, 13):
        out.append((2, 1, 7, 64, ks))               # exactly one full run; the last DMA piece is partial
        out.append((2, 1, 7, 65, ks))               # direct, a second run of one pixel whose whole window is clamped on the right
        out.append((2, 2, 5, 68, ks))               # run-time C, DMA, a second run of 4 pixels in less than one piece
        out.append((2, 4, 5, 70, ks))               # run-time C, direct
    for ks in (13, 3):                              # images smaller than the window
        out += [(2, 3, 1, 4, ks), (2, 3, 2, 3, ks), (1, 1, 1, 1, ks)]
    return out


CASES = _cases()
GENERIC_CASES = [
    (1, 5, 6, 70, 11),                              # five channels, 64 pixels per workgroup, 47 KB of LDS
    (1, 1, 6, 70, 15),                              # 62 KB, under the 64 KB default
    (1, 3, 6, 70, 15),                              # 72 KB, needs the attribute call
    (2, 3, 5, 40, 21),                              # 16 pixels per workgroup, three workgroups per row, the last one of 8
    (1, 3, 5, 20, 31),                              # 79 KB
    (1, 2, 4, 9, 1),                                # ks 1: out = img * psf
    (1, 1, 5, 20, 47),                              # 153 032 B: the largest request local_check_shape admits
]
SIGNED_CASE = (2, 3, 9, 131, 11)
REFUSED_CASES = [(1, 2, 5, 20, 47), (1, 1, 5, 20, 51)]          # 164 688 B and 179 928 B of LDS
ALL_CASES = [(c, False) for c in CASES + GENERIC_CASES] + [(SIGNED_CASE, True)]


def case_id(case, signed=False):
    return "x".join(str(v) for v in case[:4]) + f"_ks{case[4]}" + ("_signed" if signed else "")


def generic_lds_bytes(case):
    """Dynamic LDS request of the generic kernel (csrc/gather.hip, aadff_local_psf_render)."""
    B, C, H, W, ks = case
    npx = 64 if ks <= 15 else 16
    return 4 * (npx * ks * ks + C * ks * (npx + ks - 1))


def inputs(case, seed=0, signed=False):
    """(img [B,C,H,W] in [-1, 3), psf [B,H,W,ks,ks]) float32 on the CPU.  The PSFs are positive and sum to 1 per pixel; signed=True
    gives taps of both signs with sum|w| = 1."""
    B, C, H, W, ks = case
    g = torch.Generator().manual_seed(1000 * seed + 7 * ks + W)
    img = torch.rand((B, C, H, W), generator=g) * 4.0 - 1.0
    psf = torch.rand((B, H, W, ks, ks), generator=g)
    if signed:
        psf = psf - 0.4
        psf = psf / psf.abs().sum((-1, -2), keepdim=True)
    else:
        psf = psf + 0.05
        psf = psf / psf.sum((-1, -2), keepdim=True)
    return img.contiguous(), psf.contiguous()


def oracle64(img, psf, ks):
    return oconv.local_psf_render(img.double(), psf.double(), ks)


def loop64(img, psf, ks):
    """The definition, pixel by pixel in Python floats (float64): for tiny cases only."""
    B, C, H, W = img.shape
    p = ks // 2
    x, w = img.double().tolist(), psf.double().tolist()
    out = torch.zeros((B, C, H, W), dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            for y in range(H):
                for xx in range(W):
                    s = 0.0
                    for u in range(ks):
                        yy = min(max(y - p + u, 0), H - 1)
                        for v in range(ks):
                            s += x[b][c][yy][min(max(xx - p + v, 0), W - 1)] * w[b][y][xx][u][v]
                    out[b, c, y, xx] = s
    return out


def _chain(acc, x64, w64):
    """One fma step of a float32 accumulator: the product of two float32 values is exact in float64."""
    return (acc.astype(np.float64) + x64 * w64).astype(np.float32)


def sequential32(img, psf, ks):
    """(out float32 [B,C,H,W], A = sum|x w| float64 [B,C,H,W]): the gather as the direct kernel orders it."""
    B, C, H, W = img.shape
    p = ks // 2
    x = np.pad(img.numpy().astype(np.float64), ((0, 0), (0, 0), (p, p), (p, p)), mode="edge")
    w = psf.numpy().astype(np.float64)
    acc = np.zeros((B, C, H, W), dtype=np.float32)
    A = np.zeros((B, C, H, W), dtype=np.float64)
    for u in range(ks):
        for v in range(ks):
            xs, ws = x[:, :, u:u + H, v:v + W], w[:, None, :, :, u, v]
            acc = _chain(acc, xs, ws)
            A += np.abs(xs * ws)
    return torch.from_numpy(acc), torch.from_numpy(A)


def elementwise_bound(n, A, out64):
    return n * U * A + U * out64.abs()


rel_l2 = tc.rel_l2

_REF = {}


def reference(case, signed=False):
    """(img, psf, out64, A, d32seq) of a case, computed once per process and shared: do not modify."""
    key = (case, signed)
    if key not in _REF:
        img, psf = inputs(case, 0, signed)
        ks = case[4]
        out64 = oracle64(img, psf, ks)
        seq, A = sequential32(img, psf, ks)
        _REF[key] = (img, psf, out64, A, rel_l2(seq, out64), seq)
    return _REF[key][:5]


def reference_seq(case, signed=False):
    reference(case, signed)
    return _REF[(case, signed)][5]


def ratio_to_torch_float32(case):
    """d32seq in units of the oracle's own float32 distance from float64 (the table of DESIGN.md 4.9.1)."""
    img, psf, out64, A, d32seq = reference(case)
    return d32seq / rel_l2(oconv.local_psf_render(img, psf, case[4]), out64)


# ---------------------------------------------------------------------------------------------------------------- thin lens
def _thin_case(ks, C, H, W):
    return (f"2x{C}x{H}x{W}_S2_ks{ks}", 2, C, 2, H, W, ks, (256, 256), 2.8, [(700.0, 2500.0), (1200.0, 4000.0)], -1, (500.0, 5000.0))


# the five gradient cases and the four shapes of test_other_kernel_sizes_and_channels (tests/test_gpu_thinlens_grad.py)
THIN_CASES = list(tc.CASES) + [_thin_case(ks, C, H, W) for ks, C, H, W in ((3, 2, 9, 70), (5, 4, 33, 64), (9, 2, 20, 17), (13, 4, 16, 129))]


def thin_sequential32(case, img, depth, fds):
    """float32 [N,C,S,H,W]: the thin-lens render as render_slice (csrc/thinlens.hip) orders it.  The coc chain in float32 in the reference's
    operation order through rad^2, weights exp(-du^2/2/rad^2) * exp(-dv^2/2/rad^2) with float32 torch.exp cut at du^2 + dv^2 < rad^2, the weight
    sum and the channel sums sequential in tap order, out = acc * (1 / wsum)."""
    foc_len, fnum, ks, ssize, sres = tc.lens_args(case)
    f32 = np.float32
    p = ks // 2
    N, C, H, W = img.shape
    S = fds.shape[1]
    d = depth.float().numpy()[:, :, None]                                   # [N,1,1,H,W]
    fd = fds.float().numpy()[:, None, :, None, None]                        # [N,1,S,1,1]
    if (d < 0).any():
        d, fd = -d, -fd
    d = np.minimum(np.maximum(d, f32(tc.D_MIN)), f32(tc.D_MAX))
    coc = f32(foc_len / fnum) * np.abs(d - fd)
    coc = coc / d
    coc = coc * f32(foc_len)
    coc = coc / (fd - f32(foc_len))
    coc = np.maximum(coc * f32(1.0 / (ssize[0] / sres[0])), f32(0.1))
    rad = coc * f32(0.5)
    rad2 = rad * rad                                                         # [N,1,S,H,W] float32
    assert rad2.dtype == np.float32
    e = [torch.exp(torch.from_numpy(f32(-(k * k)) * f32(0.5) / rad2)).numpy() for k in range(p + 1)]
    x = np.pad(img.numpy().astype(np.float64), ((0, 0), (0, 0), (p, p), (p, p)), mode="edge")[:, :, None]      # [N,C,1,H+2p,W+2p]
    acc = np.zeros((N, C, S, H, W), dtype=f32)
    wsum = np.zeros((N, 1, S, H, W), dtype=f32)
    for u in range(ks):
        for v in range(ks):
            du, dv = abs(u - p), abs(v - p)
            wv = np.where(f32(du * du + dv * dv) < rad2, e[du] * e[dv], f32(0.0)).astype(f32)
            wsum = wsum + wv
            acc = _chain(acc, x[:, :, :, u:u + H, v:v + W], wv.astype(np.float64))
    out = acc * (f32(1.0) / wsum)
    assert out.dtype == np.float32
    return torch.from_numpy(out)


_THIN = {}


def thin_reference(case):
    """(img, depth, fds, keep bool [N,C,S,H,W], excluded share, out64 [N,C,S,H,W], seq32, d32seq over the kept pixels), cached."""
    if case[0] not in _THIN:
        img, depth, fds, dy = tc.case_inputs(case)
        keep = tc.keep_rows(case, depth, fds)
        share = 1.0 - float(keep.mean())
        out64 = tc.oracle_grads(case, img, depth, fds, torch.zeros_like(dy), torch.float64)[0]
        keep = (keep > 0).expand_as(out64)
        seq = thin_sequential32(case, img, depth, fds)
        _THIN[case[0]] = (img, depth, fds, keep, share, out64, seq, rel_l2(seq[keep], out64[keep]))
    return _THIN[case[0]]
