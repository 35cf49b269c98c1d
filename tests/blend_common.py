"""Shared by tests/test_blend_host.py and tests/test_gpu_blend.py (not a test module): the case table, the seeded inputs, the float64
comparator and the budget of the blended PSF-map render (aadff_render_psf_map_blend_stack, csrc/conv_blend.hip).

Specification (include/aadff.h): for row y of a grid of g nodes, k = clamp(#{i : node_y[i] <= y} - 1, 0, g-2) and
fy = clamp((y - node_y[k]) / (node_y[k+1] - node_y[k]), 0, 1) (g == 1: k = 0, fy = 0); columns alike give l, fx; with R(i,j) the plain
render_psf of the image with tile (i,j) of the map (flip, reflect padding),
    out = (1-fy) [(1-fx) R(k,l) + fx R(k,l+1)] + fy [(1-fx) R(k+1,l) + fx R(k+1,l+1)].

Comparator: R(i,j) from oracle.conv.render_psf on .double() inputs; the weights from the SAME float32 nodes promoted to float64.

Inputs (seeded, CPU), as tests/conv_paths_common.py: images in [-3, 34.5); PSFs positive and normalised per tile; one signed case with
sum|w| = 1 per tile; with S >= 2 one slice scaled by 1e-3.

Budget - derived from the operation order of csrc/conv_blend.hip, no constant from a kernel's output, no element excluded.  U = 2^-24.
Per output element let beta_j (j = the four corners) be the exact weights, R_j the exact corner renders, A_j = sum_t |x_t w_{j,t}|,
A = sum_j beta_j A_j and M = max_j |R_j|.  Both kernels (conv_blend_kernel<KS>, conv_blend_generic_kernel) do, per lane and output:

  (1) four accumulators a_j, each one fma chain over the ks^2 exactly formed products of corner j in a fixed tap order:
          |a_j - R_j| <= ks^2 U A_j                      (any summation order: DESIGN.md 4.9.1; the excess of gamma_n over n U is
                                                          n^2 U^2 A_j <= 0.41 U A_j at ks 51, counted in c1 below)
  (2) blend_frac: fx = clamp(fl(fl(x - n_l) / fl(n_{l+1} - n_l)), 0, 1): three roundings, relative error <= 3 U (1 + 2 U) of the
      unclamped quotient; the clamp is 1-Lipschitz and a quotient that is off by more than its own error from [0, 1] clamps to the
      exact end, so |fx^ - fx| <= 3.1 U.  gx^ = fl(1 - fx^): one more rounding of a value <= 1: |gx^ - gx| <= 4.1 U.  Rows alike.
      The four computed weights are products a_y a_x of these, so
          sum_j |beta_j^ - beta_j| <= (gy^ + fy^)(|d gx| + |d fx|) + (gx + fx)(|d gy| + |d fy|) <= 2 * 7.2 U (1 + 5 U) < 15 U
      and the weight error moves the result by at most 15 U M: c2 = 15.
  (3) blend4: p = fl(gx^ a_0), t0 = fl(fx^ a_1 + p) (fma), the same for t1, q = fl(gy^ t0), out = fl(fy^ t1 + q) (fma).  Every corner term
      passes at most three roundings (p, t, q) before the last one, each relative to a partial result bounded by
      sum_j beta_j^ |a_j| <= A (1 + O(ks^2 U)):  <= 3 U A.  The last rounding is U |out|, which is the U |o64| term to first order.
      c1 = 3 (the blend's roundings) + 2 (every second-order term above: 0.41 from (1), the rest below 1e-4) = 5.

      |got - o64| <= (ks^2 + 5) U A + 15 U M + U |o64|

The relative L2 is reported through the `margin` fixture's printout in the GPU test and not gated.
"""
import collections

import numpy as np
import torch

from oracle import conv as oconv

U = 2.0 ** -24
C1, C2 = 5, 15
SENTINEL = -12345.0
TEMPLATED_KS = (3, 5, 7, 9, 11, 13, 15, 21)

Case = collections.namedtuple("Case", "id B C S H W grid ks nodes signed kernel reaches")


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


def dispatch(ks):
    """The instantiation aadff_render_psf_map_blend_stack launches (csrc/conv_blend.hip), as the library's symbol table spells it."""
    return f"conv_blend_kernel<{ks}>" if ks in TEMPLATED_KS else "conv_blend_generic_kernel"


def expected_instantiations():
    return {f"conv_blend_kernel<{k}>" for k in TEMPLATED_KS} | {"conv_blend_generic_kernel"}


EXPLICIT_Y = (-3.25, 17.5, 17.75, 58.0)             # H 50: below 0, two nodes inside the pixel interval (17, 18), above H - 1
EXPLICIT_X = (-7.5, 20.3, 20.8, 75.0)               # W 61: likewise


def _case(B, C, S, H, W, grid, ks, nodes, kernel, reaches, signed=False):
    cid = f"{B}x{C}x{S}x{H}x{W}-g{grid}-ks{ks}-{nodes}" + ("-signed" if signed else "")
    return Case(cid, B, C, S, H, W, grid, ks, nodes, signed, kernel, reaches)


TABLE = [
    _case(2, 3, 1, 37, 45, 3, 5, "psf_map", "conv_blend_kernel<5>", "ragged tiles, cells of 18 - 23 pixels"),
    _case(1, 1, 2, 100, 72, 2, 7, "patch", "conv_blend_kernel<7>", "one cell spanning 4 x 3 tiles, clamp margins on all four sides"),
    _case(1, 3, 3, 96, 130, 5, 11, "psf_map", "conv_blend_kernel<11>", "the stack path at the production ks, signed PSFs, a slice scaled by 1e-3", signed=True),
    _case(1, 2, 1, 40, 33, 1, 3, "psf_map", "conv_blend_kernel<3>", "single PSF"),
    _case(1, 1, 1, 9, 9, 7, 3, "psf_map", "conv_blend_kernel<3>", "cells of one and two pixels"),
    _case(1, 1, 2, 33, 5, 64, 3, "psf_map", "conv_blend_kernel<3>", "the grid limit, empty cells, W barely above the padding"),
    _case(1, 1, 2, 48, 64, 3, 17, "psf_map", "conv_blend_generic_kernel", "the run-time-ks kernel"),
    _case(1, 1, 2, 64, 64, 2, 51, "psf_map", "conv_blend_generic_kernel", "the run-time-ks kernel at the ks limit, padding of 25"),
    _case(1, 3, 2, 50, 61, 4, 9, "explicit", "conv_blend_kernel<9>", "uneven nodes: one below 0, one above W - 1, two inside one pixel interval"),
    _case(1, 1, 2, 48, 64, 3, 13, "psf_map", "conv_blend_kernel<13>", "the remaining templated sizes"),
    _case(1, 1, 2, 48, 64, 3, 15, "psf_map", "conv_blend_kernel<15>", "the remaining templated sizes"),
    _case(1, 1, 2, 48, 64, 3, 21, "psf_map", "conv_blend_kernel<21>", "the remaining templated sizes"),
]


# ------------------------------------------------------------------------------------------------------------------------- inputs
def nodes_of(c):
    """(node_y, node_x) float32 [grid] of a case, by the closed forms of the specification (restated here, not imported)."""
    if c.nodes == "explicit":
        return torch.tensor(EXPLICIT_Y, dtype=torch.float32), torch.tensor(EXPLICIT_X, dtype=torch.float32)
    return closed_form_nodes(c.H, c.grid, c.nodes), closed_form_nodes(c.W, c.grid, c.nodes)


def closed_form_nodes(n, g, mode):
    j = np.arange(g, dtype=np.float64)
    if mode == "patch":
        pos = (j + 0.5) / g * n - 0.5
    elif g == 1:
        pos = np.array([(n - 1) / 2.0])
    else:
        pos = ((-0.98 + 1.96 * j / (g - 1)) + 1.0) / 2.0 * n - 0.5
    return torch.from_numpy(pos.astype(np.float32))


def inputs(c):
    """(img [B,C,H,W], maps [S,C,g ks,g ks]) float32, CPU."""
    g, ks = c.grid, c.ks
    gen = torch.Generator().manual_seed(2003 * ks + 31 * c.H + 7 * c.W + 3 * c.S + c.grid + (500000 if c.signed else 0))
    img = torch.rand((c.B, c.C, c.H, c.W), generator=gen) * 37.5 - 3.0
    w = torch.rand((c.S, c.C, g, ks, g, ks), generator=gen)
    if c.signed:
        w = w - 0.4
        w = w / w.abs().sum((3, 5), keepdim=True)
    else:
        w = w + 0.05
        w = w / w.sum((3, 5), keepdim=True)
    if c.S >= 2:
        w[c.S // 2] *= 1e-3
    return img.contiguous(), w.reshape(c.S, c.C, g * ks, g * ks).contiguous()


# --------------------------------------------------------------------------------------------------------------------- comparator
def axis_weights(node, n):
    """(k int64 [n], f float64 [n]) of the specification for the float32 nodes `node`, promoted to float64."""
    nd = node.double().numpy()
    g = nd.shape[0]
    p = np.arange(n, dtype=np.float64)
    if g == 1:
        return np.zeros(n, dtype=np.int64), np.zeros(n)
    k = np.clip((nd[None, :] <= p[:, None]).sum(1) - 1, 0, g - 2)
    return k, np.clip((p - nd[k]) / (nd[k + 1] - nd[k]), 0.0, 1.0)


def _tile(m, i, j, ks):
    return m[:, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks]


Ref = collections.namedtuple("Ref", "out64 A M")


def blend64(img, maps, grid, node_y, node_x, want_bound=True):
    """Ref(out64, A, M), float64 [B,C,S,H,W]: the specification with R(i,j) = oracle.conv.render_psf in float64; A = sum_j beta_j A_j
    with A_j the same render of |img| with |tile|, M = max_j |R_j| over the four corners."""
    B, C, H, W = img.shape
    S, ks = maps.shape[0], maps.shape[-1] // grid
    x64, xa = img.double(), img.double().abs()
    ky, fy = axis_weights(node_y, H)
    kx, fx = axis_weights(node_x, W)
    out = torch.zeros((B, C, S, H, W), dtype=torch.float64)
    A, M = torch.zeros_like(out), torch.zeros_like(out)
    g1 = grid - 1
    for s in range(S):
        m64 = maps[s].double()
        cache = {}

        def R(i, j):
            if (i, j) not in cache:
                t = _tile(m64, i, j, ks)
                cache[(i, j)] = (oconv.render_psf(x64, t), oconv.render_psf(xa, t.abs()) if want_bound else None)
            return cache[(i, j)]

        for kk in np.unique(ky):
            rows = torch.from_numpy(np.nonzero(ky == kk)[0])
            wy1 = torch.from_numpy(fy[rows.numpy()])[:, None]
            for ll in np.unique(kx):
                cols = torch.from_numpy(np.nonzero(kx == ll)[0])
                wx1 = torch.from_numpy(fx[cols.numpy()])[None, :]
                k1, l1 = min(kk + 1, g1), min(ll + 1, g1)
                corners = ((kk, ll, (1 - wy1) * (1 - wx1)), (kk, l1, (1 - wy1) * wx1), (k1, ll, wy1 * (1 - wx1)), (k1, l1, wy1 * wx1))
                o = a = mm = 0.0
                for i, j, beta in corners:
                    r, ra = R(int(i), int(j))
                    r = r[:, :, rows][:, :, :, cols]
                    o = o + beta * r
                    if want_bound:
                        a = a + beta * ra[:, :, rows][:, :, :, cols]
                        mm = torch.maximum(r.abs(), mm) if torch.is_tensor(mm) else r.abs()
                idx = (slice(None), slice(None), s, rows[:, None], cols[None, :])
                out[idx] = o
                if want_bound:
                    A[idx], M[idx] = a, mm
    return Ref(out, A, M)


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def loop64(img, maps, grid, node_y, node_x):
    """The specification restated literally, pixel by pixel in Python floats: per pixel the count of nodes at or below it, the clamped
    fraction, the four flipped, reflect-padded correlations and their blend.  Tiny inputs only."""
    B, C, H, W = img.shape
    S, ks = maps.shape[0], maps.shape[-1] // grid
    p = ks // 2
    ny, nx = [float(v) for v in node_y.double()], [float(v) for v in node_x.double()]

    def frac(nodes, q):
        if grid == 1:
            return 0, 0.0
        k = min(max(sum(1 for v in nodes if v <= q) - 1, 0), grid - 2)
        return k, min(max((q - nodes[k]) / (nodes[k + 1] - nodes[k]), 0.0), 1.0)

    x64, w64 = img.double().tolist(), maps.double().tolist()
    out = torch.zeros((B, C, S, H, W), dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            for s in range(S):
                for y in range(H):
                    k, fy = frac(ny, y)
                    for x in range(W):
                        l, fx = frac(nx, x)
                        r = {}
                        for i in {k, min(k + 1, grid - 1)}:
                            for j in {l, min(l + 1, grid - 1)}:
                                acc = 0.0
                                for u in range(ks):
                                    for v in range(ks):
                                        acc += x64[b][c][_reflect(y - p + u, H)][_reflect(x - p + v, W)] * w64[s][c][i * ks + ks - 1 - u][j * ks + ks - 1 - v]
                                r[(i, j)] = acc
                        k1, l1 = min(k + 1, grid - 1), min(l + 1, grid - 1)
                        out[b, c, s, y, x] = (1 - fy) * ((1 - fx) * r[(k, l)] + fx * r[(k, l1)]) + fy * ((1 - fx) * r[(k1, l)] + fx * r[(k1, l1)])
    return out


def interpolated_psfs(maps_c, grid, node_y, node_x, H, W):
    """float64 [H,W,ks,ks]: the bilinear interpolation of the tiles of ONE [g ks, g ks] map at every pixel (the per-pixel PSF tensor the
    kernel never forms)."""
    ks = maps_c.shape[-1] // grid
    t = maps_c.double().reshape(grid, ks, grid, ks).permute(0, 2, 1, 3)                     # [g,g,ks,ks]
    ky, fy = axis_weights(node_y, H)
    kx, fx = axis_weights(node_x, W)
    k1, l1 = np.minimum(ky + 1, grid - 1), np.minimum(kx + 1, grid - 1)
    fy_, fx_ = torch.from_numpy(fy)[:, None, None, None], torch.from_numpy(fx)[None, :, None, None]
    ky, kx, k1, l1 = (torch.from_numpy(a) for a in (ky, kx, k1, l1))
    top = (1 - fx_) * t[ky][:, kx] + fx_ * t[ky][:, l1]
    bot = (1 - fx_) * t[k1][:, kx] + fx_ * t[k1][:, l1]
    return (1 - fy_) * top + fy_ * bot


def per_pixel64(img, psfs):
    """float64 [B,C,H,W]: every pixel rendered with ITS OWN [ks,ks] PSF of psfs [H,W,ks,ks] (the same for every channel), flipped,
    reflect padding - the per-pixel definition the blend is an exact rewriting of."""
    B, C, H, W = img.shape
    ks = psfs.shape[-1]
    p = ks // 2
    x = torch.from_numpy(np.pad(img.double().numpy(), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect"))
    out = torch.zeros((B, C, H, W), dtype=torch.float64)
    for u in range(ks):
        for v in range(ks):
            out += x[:, :, u:u + H, v:v + W] * psfs[None, None, :, :, ks - 1 - u, ks - 1 - v]
    return out


# ------------------------------------------------------------------------------------------------------------------ references
_REF = {}


def reference(c):
    """(img, maps, node_y, node_x, Ref) of a case, computed once per process and shared: do not modify."""
    if c.id not in _REF:
        img, maps = inputs(c)
        ny, nx = nodes_of(c)
        _REF[c.id] = (img, maps, ny, nx, blend64(img, maps, c.grid, ny, nx))
    return _REF[c.id]


def bound(ks, r):
    """The elementwise budget of the module docstring, float64 in the shape of the result."""
    return (ks * ks + C1) * U * r.A + C2 * U * r.M + U * r.out64.abs()


def plain_bound(ks, r):
    """The budget of a plain fp32 fma chain (tests/conv_paths_common.py, tests/local_gather_common.py): ks^2 U sum|x w| + U |o64|."""
    return ks * ks * U * r.A + U * r.out64.abs()


def compare(ks, got, r):
    """(largest |got - o64| / budget over EVERY element, its flat index, rel_l2(got, o64))."""
    assert tuple(got.shape) == tuple(r.out64.shape) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    use = (got.double() - r.out64).abs() / bound(ks, r)
    worst = int(use.argmax())
    return float(use.flatten()[worst]), worst, rel_l2(got, r.out64)
