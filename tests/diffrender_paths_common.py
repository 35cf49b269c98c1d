"""Shared by tests/test_diffrender_paths_host.py and tests/test_gpu_diffrender_paths.py (not a test module): the cases, inputs, comparators,
bounds and planted errors of the elementwise tests of the image-space GRADIENT kernels - map_dimg_kernel, map_dpsf_partial_kernel and
map_dpsf_sum_kernel (csrc/conv_bwd.hip), local_dpsf_kernel and local_dimg_kernel (csrc/gather.hip; gather_adjoint of csrc/gather_window.h).

Comparator: torch.autograd through oracle.conv.render_psf_map (slice by slice, stacked) and oracle.conv.local_psf_render in float64 on the
CPU.  `map_loop64` / `local_loop64` restate the definition as plain Python loops (tiny cases), `map_def64` / `local_def64` tap by tap in
numpy (every case; the planted errors are modifications of these).

Inputs (seeded, CPU): img in [-1, 3), PSFs of both signs with sum|w| = 1 per PSF (the `signed` form of local_gather_common.inputs),
dy = randn.

Bounds - derived, elementwise, no element excluded, nothing measured on the code under test.  u = 2^-24.  Both gradients are sums of
products of two inputs with coefficients 0 or 1, so the same float64 autograd call on other inputs gives, per element,
    A = the gradient at (|img|, |psf|, |dy|): the sum of the absolute values of the element's terms,
    N = the gradient at all-ones inputs:      the number of its terms.
A term that passes through R roundings carries a factor (1 + d_1) .. (1 + d_R), |d_i| <= u, so |got - exact| <= ((1 + u)^R - 1) A with R
the largest count over the element's terms; (1 + u)^R - 1 <= (R + 2) u for R <= 8192 (R u + R^2 u^2 / 2 + .. <= R u + 2 u).

  d_img of the map, d_img and d_psf of the gather:  |got - ref64| <= (N + 2) u A.
    A float32 sum of N exactly formed products (fmaf) in ANY order has R <= N: the first product of a zero-started chain is rounded once,
    every later rounding joins two non-empty sets of terms, and there are at most N - 1 such joins.  Terms masked to zero (the per-patch
    mask of map_dimg_kernel) and additions to a zero accumulator are exact and add no rounding.  N stays below 8192 (5618 at most for the
    map, 27 x 29 at ks 51; 4158 at a corner of the 9 x 70 ks 21 gather) on every case but the 5 x 20 ks 47 gather, whose corner pixel
    collects 110 x 290 = 31 900 clamped taps.  There R is not N but the depth of gather_adjoint's sums: one fmaf chain per dy row (at most
    24 x 290 = 6960 terms) and one addition per row, 6965 < 8192, so (N + 2) u A holds for it too.

  d_psf of the map:  |got - ref64| <= (min(D, N) + 2) u A.
    N = B x patch pixels, and N u A would not see one missing pixel.  D is the depth of the kernels' summation tree instead, read from
    csrc/conv_bwd.hip:
      map_dpsf_partial_kernel  `acc[m] = fmaf(d[k], v[..], acc[m])` over j < 4, k < 4: a chain of 16 fmaf per lane                      16
                               `wave_sum(acc[m])` (common.h): `v += __shfl_xor(v, off)` for off = 32 .. 1                                 6
      map_dpsf_sum_kernel      `sr += q[tx * per_slab]` over the patch's txn tile columns, started at 0.f: 0 + x is exact           txn - 1
                               `sb += sr` over its tyn tile rows, `sum += sb` over b < B, both started at 0.f               tyn - 1, B - 1
    D = 19 + txn + tyn + B with txn, tyn the tile counts of the ELEMENT's patch.  (22 + txn + tyn + B would count the three zero-started
    additions of the second pass as roundings; they are exact, so the smaller figure is the bound held.)  Where a patch has fewer than D
    pixels per batch item the any-order count N is the smaller one and is used.  `dpsf_tree32` restates exactly this tree in numpy float32;
    the host test holds it to the bound on every map case.
"""
import collections

import numpy as np
import torch

from oracle import conv as oconv

import local_gather_common as lg

U = 2.0 ** -24
BT = 32                                             # tile edge of csrc/conv_bwd.hip
SENTINEL = -12345.0

Case = collections.namedtuple("Case", "id op B C S H W grid ks why")


def _map(B, C, S, H, W, grid, ks, why):
    return Case(f"map-{B}x{C}x{S}x{H}x{W}-g{grid}-ks{ks}", "map", B, C, S, H, W, grid, ks, why)


def _local(B, C, H, W, ks, why):
    return Case(f"local-{B}x{C}x{H}x{W}-ks{ks}", "local", B, C, 1, H, W, 0, ks, why)


MAP_CASES = [
    _map(2, 2, 2, 6, 7, 1, 11, "tuned <11> instances at H = p + 1: rows 1-4 and columns 1-5 carry both folds (3 x 3 mirror positions), waves 2, 3 have no row"),
    _map(1, 2, 2, 12, 13, 3, 11, "patches of 4-5 pixels under a 5-pixel halo: the one tile meets all nine patches"),
    _map(1, 1, 1, 23, 25, 11, 11, "patches of 2-3 pixels, grid 11"),
    _map(2, 3, 2, 33, 97, 3, 11, "widths 32 / 32 / 33: 1, 1, 2 tiles per patch, slabs the sum pass must not read; second d_img tile row of one row; batch and slice sums"),
    _map(1, 1, 1, 96, 96, 2, 11, "the centre tile has no border thread and meets four patches (<11>)"),
    _map(1, 1, 1, 96, 96, 2, 5, "the same with the run-time instances"),
    _map(2, 2, 2, 4, 5, 1, 7, "run-time instances (<0>, EB = 1) at H = p + 1"),
    _map(1, 2, 1, 97, 33, 3, 5, "heights 32 / 32 / 33: unequal tile ROWS"),
    _map(2, 1, 2, 27, 29, 2, 51, "the largest ks: both folds of both axes overlap"),
    _map(1, 1, 1, 64, 65, 64, 3, "AADFF_MAX_GRID, one-pixel patches (columns 0-62 and 64; one of two pixels)"),
    _map(1, 2, 2, 5, 6, 2, 1, "ks 1: no padding, one product per term"),
]
LOCAL_CASES = [
    _local(2, 3, 3, 131, 11, "local_dpsf_kernel<11>; three runs, the last of 3 pixels"),
    _local(1, 3, 9, 70, 21, "the window is taller than the image: a corner collects 4158 terms"),
    _local(1, 2, 1, 70, 5, "H = 1: a pixel is the first and the last row at once and collects every tap row"),
    _local(1, 1, 5, 1, 5, "W = 1: first and last column at once"),
    _local(1, 8, 2, 64, 5, "two full channel groups of gather_adjoint, exactly one run"),
    _local(2, 5, 4, 66, 7, "a second channel group of one channel, a second run of 2 pixels"),
    _local(1, 4, 3, 65, 3, "ks 3, one full group, a second run of one pixel"),
    _local(2, 3, 2, 3, 13, "image smaller than the window"),
    _local(1, 1, 1, 1, 13, "one pixel: every tap clamps onto it"),
    _local(1, 2, 4, 9, 1, "ks 1"),
    _local(1, 1, 5, 20, 47, "the largest size local_check_shape admits"),
]
CASES = MAP_CASES + LOCAL_CASES
TINY = [c for c in CASES if c.B * c.C * c.S * c.H * c.W * c.ks * c.ks <= 80000]      # the Python-loop definitions take a second at most
FRONT_CASES = [MAP_CASES[3], LOCAL_CASES[0]]                                            # through aadff.diffrender, non-contiguous dy


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def patch_index(n, grid):
    """(bounds int(i / grid * n), patch of every pixel)."""
    hb = oconv.patch_bounds(n, grid)
    return hb, np.searchsorted(np.asarray(hb[1:]), np.arange(n), side="right")


def tiles(c):
    """(tile rows of every patch row, tile columns of every patch column, nty, ntx): plan_map_bwd / map_dpsf_sum_kernel."""
    hb, wb = oconv.patch_bounds(c.H, c.grid), oconv.patch_bounds(c.W, c.grid)
    tyn = [-(-(b - a) // BT) for a, b in zip(hb, hb[1:])]
    txn = [-(-(b - a) // BT) for a, b in zip(wb, wb[1:])]
    return tyn, txn, max(tyn), max(txn)


def workspace_bytes(c):
    """ws_bytes of plan_map_bwd: one slab of S C (grid ks)^2 floats per (b, tile of the largest patch)."""
    _, _, nty, ntx = tiles(c)
    return c.B * ntx * nty * c.S * c.C * c.grid * c.grid * c.ks * c.ks * 4


def kernels(c):
    """The instantiation behind each gradient of a case (aadff_render_psf_map_stack_bwd, aadff_local_psf_render_bwd)."""
    if c.op == "map":
        return {"d_img": "map_dimg<11>" if c.ks == 11 else "map_dimg<0>", "d_psf": "map_dpsf<11>" if c.ks == 11 else "map_dpsf<1>"}
    return {"d_img": "local_dimg", "d_psf": "local_dpsf<11>" if c.ks == 11 else "local_dpsf<0>"}


# ------------------------------------------------------------------------------------------------------------------------- inputs
def inputs(c):
    """(img [B,C,H,W], psf: maps [S,C,g ks,g ks] or per-pixel [B,H,W,ks,ks], dy [B,C,S,H,W] or [B,C,H,W]), float32, CPU."""
    if c.op == "local":
        img, psf = lg.inputs((c.B, c.C, c.H, c.W, c.ks), 0, signed=True)
        gen = torch.Generator().manual_seed(77 + 1000 * c.ks + 13 * c.W + c.H)
        return img, psf, torch.randn((c.B, c.C, c.H, c.W), generator=gen)
    gen = torch.Generator().manual_seed(2003 * c.ks + 31 * c.H + 7 * c.W + 3 * c.S + c.grid)
    img = torch.rand((c.B, c.C, c.H, c.W), generator=gen) * 4.0 - 1.0
    w = torch.rand((c.S, c.C, c.grid, c.ks, c.grid, c.ks), generator=gen) - 0.4
    w = w / w.abs().sum((3, 5), keepdim=True)
    dy = torch.randn((c.B, c.C, c.S, c.H, c.W), generator=gen)
    return img.contiguous(), w.reshape(c.S, c.C, c.grid * c.ks, c.grid * c.ks).contiguous(), dy


def autograd_grads(c, img, psf, dy, dtype=torch.float64):
    """(d_img, d_psf): torch.autograd through the oracle in `dtype`."""
    x = img.detach().to(dtype).clone().requires_grad_(True)
    w = psf.detach().to(dtype).clone().requires_grad_(True)
    if c.op == "map":
        out = torch.stack([oconv.render_psf_map(x, w[s], c.grid) for s in range(c.S)], dim=2)
    else:
        out = oconv.local_psf_render(x, w, c.ks)
    gi, gp = torch.autograd.grad(out, (x, w), dy.to(dtype))
    return gi.detach(), gp.detach()


# ------------------------------------------------------------------------------------------------- the definition, as Python loops
def _refl(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def map_loop64(c, img, maps, dy):
    """d_img[src] += dy psf_(i,j)[a][e], d_psf[s][c][i ks + a][j ks + e] += dy img[src], src = (refl(y + p - a), refl(x + p - e)), (i, j)
    the patch of the dy pixel (y, x).  Python floats, no autograd: tiny cases only."""
    ks, p, g = c.ks, c.ks // 2, c.grid
    _, pi = patch_index(c.H, g)
    _, pj = patch_index(c.W, g)
    x, w, d = img.double().tolist(), maps.double().tolist(), dy.double().tolist()
    gi = np.zeros((c.B, c.C, c.H, c.W))
    gp = np.zeros((c.S, c.C, g * ks, g * ks))
    for b in range(c.B):
        for ch in range(c.C):
            for s in range(c.S):
                for y in range(c.H):
                    for xx in range(c.W):
                        dv = d[b][ch][s][y][xx]
                        for a in range(ks):
                            sy, row = _refl(y + p - a, c.H), int(pi[y]) * ks + a
                            for e in range(ks):
                                sx, col = _refl(xx + p - e, c.W), int(pj[xx]) * ks + e
                                gi[b, ch, sy, sx] += dv * w[s][ch][row][col]
                                gp[s, ch, row, col] += dv * x[b][ch][sy][sx]
    return torch.from_numpy(gi), torch.from_numpy(gp)


def local_loop64(c, img, psf, dy):
    """The same with clamp for refl, the dy pixel's own PSF, no flip (src = (clamp(y + a - p), clamp(x + e - p))), d_psf summed over the
    channels."""
    ks, p = c.ks, c.ks // 2
    x, w, d = img.double().tolist(), psf.double().tolist(), dy.double().tolist()
    gi = np.zeros((c.B, c.C, c.H, c.W))
    gp = np.zeros((c.B, c.H, c.W, ks, ks))
    for b in range(c.B):
        for ch in range(c.C):
            for y in range(c.H):
                for xx in range(c.W):
                    dv = d[b][ch][y][xx]
                    for a in range(ks):
                        sy = min(max(y + a - p, 0), c.H - 1)
                        for e in range(ks):
                            sx = min(max(xx + e - p, 0), c.W - 1)
                            gi[b, ch, sy, sx] += dv * w[b][y][xx][a][e]
                            gp[b, y, xx, a, e] += dv * x[b][ch][sy][sx]
    return torch.from_numpy(gi), torch.from_numpy(gp)


# -------------------------------------------------------------------------------- the definition tap by tap in numpy, errors plantable
MAP_PLANTS = {
    "corner mirror terms dropped": "d_img",                 # the terms whose source is folded on BOTH axes
    "PSF of the target pixel's patch": "d_img",             # instead of the patch of the dy pixel
    "slice 0's PSF for every slice": "d_img",
    "d_psf window replicated": "d_psf",                     # clamp instead of reflect
    "last row of each 32-row tile dropped": "d_psf",
    "d_psf over batch item 0 only": "d_psf",
}
LOCAL_PLANTS = {
    "zero padding in d_img": "d_img",                       # instead of the clamped duplicates
    "d_psf over C - 1 channels": "d_psf",
}


def _scatter(src, n, keep=None):
    """[n, n] float64: M[src[y], y] = 1 (columns where keep is False stay zero)."""
    m = np.zeros((n, n))
    cols = np.arange(n) if keep is None else np.arange(n)[keep]
    m[src[cols], cols] = 1.0
    return m


def map_def64(c, img, maps, dy, plant=None):
    assert plant is None or plant in MAP_PLANTS
    ks, p, g = c.ks, c.ks // 2, c.grid
    x, w, d = img.double().numpy(), maps.double().numpy(), dy.double().numpy()
    hb, pi = patch_index(c.H, g)
    wb, pj = patch_index(c.W, g)
    ys, xs = np.arange(c.H), np.arange(c.W)
    dp = d
    if plant == "last row of each 32-row tile dropped":
        dp = d.copy()
        dp[:, :, :, (ys - np.asarray(hb)[pi]) % BT == BT - 1] = 0.0
    if plant == "d_psf over batch item 0 only":
        dp = d[:1]
    refl = lambda v, n: np.where(np.abs(v) >= n, 2 * n - 2 - np.abs(v), np.abs(v))      # noqa: E731
    gi = np.zeros((c.B, c.C, c.H, c.W))
    gp = np.zeros((c.S, c.C, g * ks, g * ks))
    for a in range(ks):
        uy = ys + p - a
        ry, fy = refl(uy, c.H), (uy < 0) | (uy >= c.H)
        My, Myf = _scatter(ry, c.H), _scatter(ry, c.H, fy)
        for e in range(ks):
            ux = xs + p - e
            rx, fx = refl(ux, c.W), (ux < 0) | (ux >= c.W)
            Mx, Mxf = _scatter(rx, c.W), _scatter(rx, c.W, fx)
            wt = w[:, :, (pi * ks + a)[:, None], (pj * ks + e)[None, :]].transpose(1, 0, 2, 3)[None]      # [1,C,S,H,W]: the dy pixel's patch
            if plant == "slice 0's PSF for every slice":
                wt = wt[:, :, :1]
            if plant == "PSF of the target pixel's patch":
                gi += ((My @ d @ Mx.T) * wt).sum(2)
            else:
                t = (d * wt).sum(2)
                gi += My @ t @ Mx.T
                if plant == "corner mirror terms dropped":
                    gi -= Myf @ t @ Mxf.T
            sy, sx = (np.clip(uy, 0, c.H - 1), np.clip(ux, 0, c.W - 1)) if plant == "d_psf window replicated" else (ry, rx)
            t = (dp * x[:dp.shape[0], :, None, sy[:, None], sx[None, :]]).sum(0)                           # [C,S,H,W]
            t = np.add.reduceat(np.add.reduceat(t, hb[:-1], axis=2), wb[:-1], axis=3)                      # [C,S,g,g]
            gp[:, :, a::ks, e::ks] = t.transpose(1, 0, 2, 3)
    return torch.from_numpy(gi), torch.from_numpy(gp)


def local_def64(c, img, psf, dy, plant=None):
    assert plant is None or plant in LOCAL_PLANTS
    ks, p = c.ks, c.ks // 2
    x, w, d = img.double().numpy(), psf.double().numpy(), dy.double().numpy()
    ys, xs = np.arange(c.H), np.arange(c.W)
    nc = c.C - 1 if plant == "d_psf over C - 1 channels" else c.C
    zero = plant == "zero padding in d_img"
    gi = np.zeros((c.B, c.C, c.H, c.W))
    gp = np.zeros((c.B, c.H, c.W, ks, ks))
    for a in range(ks):
        uy = ys + a - p
        cy = np.clip(uy, 0, c.H - 1)
        My = _scatter(cy, c.H, (uy == cy) if zero else None)
        for e in range(ks):
            ux = xs + e - p
            cx = np.clip(ux, 0, c.W - 1)
            Mx = _scatter(cx, c.W, (ux == cx) if zero else None)
            gi += My @ (d * w[:, None, :, :, a, e]) @ Mx.T
            gp[:, :, :, a, e] = (d[:, :nc] * x[:, :nc, cy[:, None], cx[None, :]]).sum(1)
    return torch.from_numpy(gi), torch.from_numpy(gp)


def definition64(c, img, psf, dy, plant=None):
    return (map_def64 if c.op == "map" else local_def64)(c, img, psf, dy, plant)


def loop64(c, img, psf, dy):
    return (map_loop64 if c.op == "map" else local_loop64)(c, img, psf, dy)


def plants(c):
    return MAP_PLANTS if c.op == "map" else LOCAL_PLANTS


# -------------------------------------------------------------------------------------------- the summation tree of d_psf of the map
def _fma32(acc, a64, b64):
    """One fmaf step of a float32 accumulator: the product of two float32 values is exact in float64."""
    return (acc.astype(np.float64) + a64 * b64).astype(np.float32)


def dpsf_tree32(c, img, dy):
    """float32 [S,C,g ks,g ks]: d_psf of the map summed as map_dpsf_partial_kernel and map_dpsf_sum_kernel sum it.  Per 32 x 32 tile of a patch
    and (b, c, s): lane = 8 lyr + lxg owns rows lyr + 8 j and columns 4 lxg + k, a chain of 16 fmaf in (j, k) order from 0; the wave
    butterfly v += v[lane ^ off], off = 32 .. 1; then per element the chains over tile columns, tile rows and b, each from 0."""
    ks, p, g = c.ks, c.ks // 2, c.grid
    hb, wb = oconv.patch_bounds(c.H, g), oconv.patch_bounds(c.W, g)
    tyn, txn, _, _ = tiles(c)
    x = np.pad(img.numpy().astype(np.float64), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect") if p else img.numpy().astype(np.float64)
    x = np.pad(x, ((0, 0), (0, 0), (0, BT), (0, BT)))                      # beyond the image: finite values that meet dy = 0 only
    d = dy.numpy().astype(np.float64)
    lanes = np.arange(64)
    out = np.zeros((c.S, c.C, g * ks, g * ks), dtype=np.float32)
    for i in range(g):
        for j in range(g):
            total = np.zeros((c.S, c.C, ks, ks), dtype=np.float32)
            for b in range(c.B):
                sb = np.zeros_like(total)
                for ty in range(tyn[i]):
                    sr = np.zeros_like(total)
                    for tx in range(txn[j]):
                        y0, x0 = hb[i] + ty * BT, wb[j] + tx * BT
                        y1, x1 = min(y0 + BT, hb[i + 1]), min(x0 + BT, wb[j + 1])
                        td = np.zeros((c.C, c.S, BT, BT))
                        td[:, :, :y1 - y0, :x1 - x0] = d[b, :, :, y0:y1, x0:x1]
                        win = x[b, :, y0:y0 + BT + 2 * p, x0:x0 + BT + 2 * p]                      # window row r = image row y0 - p + r
                        v = np.lib.stride_tricks.sliding_window_view(win, (BT, BT), axis=(1, 2))[:, ::-1, ::-1]      # [C,a,e,row,col]: window (row + 2p - a, col + 2p - e)
                        td = td.reshape(c.C, c.S, 1, 1, 4, 8, 8, 4)                                 # rows (j, lyr), columns (lxg, k)
                        v = v.reshape(c.C, 1, ks, ks, 4, 8, 8, 4)
                        acc = np.zeros((c.C, c.S, ks, ks, 8, 8), dtype=np.float32)
                        for jj in range(4):
                            for k in range(4):
                                acc = _fma32(acc, td[:, :, :, :, jj, :, :, k], v[:, :, :, :, jj, :, :, k])
                        acc = acc.reshape(c.C, c.S, ks, ks, 64)
                        for off in (32, 16, 8, 4, 2, 1):
                            acc = acc + acc[..., lanes ^ off]
                        assert acc.dtype == np.float32
                        sr = sr + acc[..., 0].transpose(1, 0, 2, 3)
                    sb = sb + sr
                total = total + sb
            out[:, :, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks] = total
    return torch.from_numpy(out)


def dpsf_depth(c):
    """D of the module docstring per element of the PSF map, float64 [g ks, g ks]."""
    tyn, txn, _, _ = tiles(c)
    D = 16 + 6 + (np.asarray(txn)[None, :] - 1) + (np.asarray(tyn)[:, None] - 1) + (c.B - 1)
    return torch.from_numpy(np.repeat(np.repeat(D, c.ks, axis=0), c.ks, axis=1).astype(np.float64))


# ------------------------------------------------------------------------------------------------------------------ references
Ref = collections.namedtuple("Ref", "img psf dy gi gp Ai Ap Ni Np gi32 gp32 d32_img d32_psf")
_REF = {}


def build_reference(c, img, psf, dy):
    gi, gp = autograd_grads(c, img, psf, dy)
    Ai, Ap = autograd_grads(c, img.abs(), psf.abs(), dy.abs())
    Ni, Np = autograd_grads(c, torch.ones_like(img), torch.ones_like(psf), torch.ones_like(dy))
    gi32, gp32 = autograd_grads(c, img, psf, dy, torch.float32)
    return Ref(img, psf, dy, gi, gp, Ai, Ap, Ni, Np, gi32, gp32, rel_l2(gi32, gi), rel_l2(gp32, gp))


def reference(c):
    """Ref of a case with its seeded inputs, computed once per process and shared: do not modify."""
    if c.id not in _REF:
        _REF[c.id] = build_reference(c, *inputs(c))
    return _REF[c.id]


def bounds(c, r):
    """(bound of d_img, bound of d_psf), float64, the shapes of the gradients."""
    bi = (r.Ni + 2.0) * U * r.Ai
    bp = (torch.minimum(dpsf_depth(c), r.Np) + 2.0) * U * r.Ap if c.op == "map" else (r.Np + 2.0) * U * r.Ap
    return bi, bp


def share(got, ref64, bound):
    """(largest |got - ref64| / bound over EVERY element, its index, its error, its bound)."""
    assert tuple(got.shape) == tuple(ref64.shape) == tuple(bound.shape), (got.shape, ref64.shape, bound.shape)
    assert bool(torch.isfinite(got).all()) and bool((bound > 0).all())
    err = (got.double() - ref64).abs()
    use = err / bound
    worst = int(use.argmax())
    idx = tuple(int(v) for v in np.unravel_index(worst, tuple(got.shape)))
    return float(use.flatten()[worst]), idx, float(err.flatten()[worst]), float(bound.flatten()[worst])
