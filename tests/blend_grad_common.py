"""Shared by tests/test_blend_grad_host.py and tests/test_gpu_blend_grad.py (not a test module): the cases, inputs, comparators, budgets,
planted errors and summation-tree restatements of the gradients of the blended PSF-map render (aadff_render_psf_map_blend_stack_bwd,
csrc/conv_blend_bwd.hip; aadff.diffrender.render_psf_map_blend[_stack]).

Specification (include/aadff.h).  With k, fy of the forward, the HAT of node i on row y is
    Hy_i(y) = [k(y) == i] (1 - fy(y)) + [min(k(y) + 1, g - 1) == i] fy(y)            (g == 1: 1 everywhere),
Hx_j(x) alike, p = ks / 2, refl = the reflect padding, and
    d_img[b,c,Y,X]             = sum_s sum_(i,j) sum_{y,x,a,e : refl(y + p - a) = Y, refl(x + p - e) = X} dy[b,c,s,y,x] Hy_i(y) Hx_j(x) w_sc[i ks + a][j ks + e]
    d_maps[s,c,i ks + a,j ks + e] = sum_b sum_(y,x) dy[b,c,s,y,x] Hy_i(y) Hx_j(x) img[b,c,refl(y + p - a),refl(x + p - e)]
(a = ks - 1 - u, e = ks - 1 - v of the forward's taps).

Comparator: torch.autograd.grad in float64 through blend_common.blend64 (the forward's comparator), dy = randn seeded.  `def64` restates
the two closed forms tap by tap in numpy for ANY hats (every case; A, M, N of the budget and the planted errors are calls of it),
`loop64` as plain Python loops (tiny cases).

Budget - elementwise, no element excluded, nothing taken from the code under test.  u = 2^-24.
    |got - ref64| <= (R + c1) u A + c2 u M + u |ref64|
  A   the same gradient at (|img|, |maps|, |dy|): the sum of the absolute values of the element's terms.
  M   that gradient with every hat replaced by 1 on its support (the rows of cells i - 1 and i).  The kernels' fy is blend_frac of the
      forward: three roundings and a clamp, |fy^ - fy| <= 3.1 u ABSOLUTE, and |fl(1 - fy^) - (1 - fy)| <= 4.1 u (blend_common, point (2)).
      A hat is one of the two (g == 1: their sum 1 + 0, exact), so |Hy^ - Hy| <= 4.1 u, and the exact product of two computed hats is
      within 4.1 u (Hx + Hy^) <= 8.2 u (1 + 5 u) < 9 u of Hy Hx: c2 = 9.
  c1  both kernels form fl(dy * fl(Hy^ * Hx^)) before the sums: two roundings relative to the term, and 2 for the excess of
      (1 + u)^(R + 2) - 1 over (R + 2) u while R <= 8192 (tests/diffrender_paths_common.py): c1 = 4.
  R   the roundings a term passes through in the sums, the smaller of
        N  the element's term count (`def64` at all-ones inputs with the hats replaced by 1 on their support): a float32 sum of N exactly
           formed products in any order rounds a term at most N times, and terms with a zero weight add exact zeros;
        D  the depth of the kernel's summation tree, read from csrc/conv_blend_bwd.hip:
      d_img, templated sizes (blend_dimg_kernel<KS>).  A mirror image of an element is one more pass of the direct code.  Per (slice, node,
        pass) a zero-started chain `acc = fmaf(T, w, acc)` over the ks^2 taps (ks^2 roundings; taps whose source is outside the image add exact
        zeros); `tot += acc` over the triples of the wave; the four waves' totals as ((w0 + w1) + w2) + w3 (3).  A node whose hat support
        misses the element's own source window [Y - p, Y + p] x [X - p, X + p] adds exact zeros, so with n(Y, X) the nodes that meet it and
        m(Y, X) = (1 + mirror rows of Y) (1 + mirror columns of X) <= 9 the passes the element takes part in
            D = ks^2 + S n m + 3
      d_img, run-time ks (blend_dimg_generic_kernel).  Per slice and node (i, j) in the order i, j: per tap column e a zero-started chain
        `part = fmaf(T, w, part)` over a < ks (ks roundings), `acc += part` (one each: ks per node); the node's mirror terms: a zero-started
        fmaf chain per mirror position over its sources (at most p rows x ks columns: a mirror row -y has the sources 0 .. p - y),
        `fold += m` over the at most 8 positions (8), `acc += fold` (one); `total += acc` over the slices:
            D = ks + n (ks + 1) + S                     elements without a mirror image
            D = p ks + 8 + n (ks + 1) + S               elements with one (1 <= Y <= p or H - 1 - p <= Y <= H - 2, columns alike)
      d_maps (blend_dmaps_partial_kernel, blend_dmaps_sum_kernel).  Per 32 x 32 tile of a cell and corner: a chain of 16 fmaf per lane (16),
        the wave butterfly (6); the second pass adds, each level started at 0 (0 + x is exact), the tile columns (txn - 1), the tile rows
        (tyn - 1), the at most four (cell, corner) pairs that are this node (3) and the batch (B - 1):
            D = 22 + max over the node's cells of (txn + tyn - 2) + 3 + B - 1
`dimg_tree32` and `dmaps_tree32` restate exactly these trees in numpy float32 (the hats by `frac32`, the forward's arithmetic); the host
test holds both to the budget on every case.
"""
import collections

import numpy as np
import torch

import blend_common as bc

U = bc.U
BT = 32
C1, C2 = 4, 9
SENTINEL = bc.SENTINEL
TEMPLATED_KS = bc.TEMPLATED_KS

Case = collections.namedtuple("Case", "id B C S H W grid ks nodes signed reaches")


def _case(B, C, S, H, W, grid, ks, nodes, reaches, signed=False):
    return Case(f"{B}x{C}x{S}x{H}x{W}-g{grid}-ks{ks}-{nodes}" + ("-signed" if signed else ""), B, C, S, H, W, grid, ks, nodes, signed, reaches)


TABLE = [Case(c.id, c.B, c.C, c.S, c.H, c.W, c.grid, c.ks, c.nodes, c.signed, c.reaches) for c in bc.TABLE] + [
    _case(1, 1, 2, 6, 7, 2, 11, "psf_map", "H = ks/2 + 1, templated: rows 1-4 carry both folds (3 x 3 mirror positions)"),
    _case(1, 1, 1, 10, 12, 2, 19, "psf_map", "H = ks/2 + 1 on the run-time-ks kernels"),
    _case(1, 1, 1, 24, 26, 4, 13, "patch", "cells of 6 pixels under a halo of 6: one window meets more than 3 x 3 nodes"),
    _case(2, 1, 2, 40, 70, 3, 7, "patch", "B = 2 and S = 2: the batch sum of d_maps, the slice sum of d_img, 2 - 3 tiles per cell row"),
]
TINY = [(1, 2, 2, 7, 9, 3, 3, "psf_map"), (2, 1, 1, 6, 5, 2, 3, "patch"), (1, 1, 1, 5, 6, 1, 3, "psf_map"), (1, 1, 2, 4, 7, 4, 5, "explicit")]


def kernels(ks):
    """The instantiations aadff_render_psf_map_blend_stack_bwd launches, as the library's symbol table spells them."""
    if ks in TEMPLATED_KS:
        return {f"blend_dimg_kernel<{ks}>", f"blend_dmaps_partial_kernel<{ks}>", "blend_dmaps_sum_kernel"}
    return {"blend_dimg_generic_kernel", "blend_dmaps_partial_kernel<0>", "blend_dmaps_sum_kernel"}


def expected_instantiations():
    return set().union(*(kernels(k) for k in TEMPLATED_KS + (17,)))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------------------------------- inputs
def nodes_of(c):
    return bc.nodes_of(c)


def inputs(c):
    """(img, maps, dy [B,C,S,H,W]) float32, CPU: the forward's seeded inputs and dy = randn."""
    img, maps = bc.inputs(c)
    gen = torch.Generator().manual_seed(991 + 2003 * c.ks + 31 * c.H + 7 * c.W + 3 * c.S + c.grid + 17 * c.B)
    return img, maps, torch.randn((c.B, c.C, c.S, c.H, c.W), generator=gen)


def tiny_inputs(t):
    B, Cn, S, H, W, g, ks, mode = t
    gen = torch.Generator().manual_seed(sum(t[:7]) + 1)
    img = torch.rand((B, Cn, H, W), generator=gen) * 4.0 - 1.0
    maps = torch.rand((S, Cn, g * ks, g * ks), generator=gen) - 0.3
    dy = torch.randn((B, Cn, S, H, W), generator=gen)
    if mode == "explicit":
        ny, nx = torch.tensor([-2.5, 1.25, 1.5, 11.0]), torch.tensor([0.0, 1.0, 3.5, 6.0])
    else:
        ny, nx = bc.closed_form_nodes(H, g, mode), bc.closed_form_nodes(W, g, mode)
    return img, maps, dy, g, ny, nx


# --------------------------------------------------------------------------------------------------------------------- comparator
def autograd64(img, maps, dy, grid, ny, nx):
    """(d_img, d_maps) float64: torch.autograd through the forward's float64 comparator."""
    x = img.detach().double().clone().requires_grad_(True)
    m = maps.detach().double().clone().requires_grad_(True)
    out = bc.blend64(x, m, grid, ny, nx, want_bound=False).out64
    gi, gm = torch.autograd.grad(out, (x, m), dy.double())
    return gi.detach(), gm.detach()


def hats64(node, n):
    """(H float64 [g, n], support float64 [g, n] of zeros and ones, k int64 [n]) of an axis."""
    g = node.shape[0]
    k, f = bc.axis_weights(node, n)
    k1, ar = np.minimum(k + 1, g - 1), np.arange(n)
    Hm, sup = np.zeros((g, n)), np.zeros((g, n))
    Hm[k, ar] += 1.0 - f
    Hm[k1, ar] += f
    sup[k, ar] = 1.0
    sup[k1, ar] = 1.0
    return Hm, sup, k


def _refl(v, n):
    v = np.abs(v)
    return np.where(v >= n, 2 * n - 2 - v, v)


def _scatter(src, n, keep=None):
    """[n, n] float64: M[src[y], y] = 1 (columns where keep is False stay zero)."""
    m = np.zeros((n, n))
    cols = np.arange(n) if keep is None else np.arange(n)[keep]
    m[src[cols], cols] = 1.0
    return m


PLANTS = {
    "one tap dropped": "d_img",
    "one mirror fold dropped": "d_img",                         # the terms folded over the top edge
    "one source pixel dropped from a d_maps sum": "d_maps",
    "fx and 1-fx swapped in one cell": "both",                  # the cell of column W / 3
    "the unflipped PSF": "both",
    "one slice missing from the d_img sum": "d_img",
    "one batch item missing from d_maps": "d_maps",
}


def plant_changes_a_term(c, plant):
    return not (plant == "fx and 1-fx swapped in one cell" and c.grid == 1)       # one node: there is no fx


def def64(img, maps, dy, grid, Hy, Hx, plant=None, want=("d_img", "d_maps")):
    """The two closed forms tap by tap, float64 numpy, for the hats Hy [g,H], Hx [g,W]: {name: tensor}."""
    assert plant is None or plant in PLANTS
    x, w, d = (t.double().numpy() for t in (img, maps, dy))
    B, Cn, H, W = x.shape
    S, g = w.shape[0], grid
    ks = w.shape[-1] // g
    p = ks // 2
    ys, xs = np.arange(H), np.arange(W)
    d_i, d_m = d, d
    if plant == "one slice missing from the d_img sum":
        d_i = d[:, :, :S - 1]
    if plant == "one batch item missing from d_maps":
        d_m = d[:B - 1]
    if plant == "one source pixel dropped from a d_maps sum":
        d_m = d.copy()
        d_m[:, :, :, H // 2, W // 2] = 0.0
    gi = np.zeros((B, Cn, H, W))
    gm = np.zeros((S, Cn, g * ks, g * ks))
    for a in range(ks):
        uy = ys + p - a
        ry = _refl(uy, H)
        My = _scatter(ry, H)
        for e in range(ks):
            ux = xs + p - e
            rx = _refl(ux, W)
            wa, we = (ks - 1 - a, ks - 1 - e) if plant == "the unflipped PSF" else (a, e)
            if "d_img" in want and not (plant == "one tap dropped" and (a, e) == (p, max(p - 1, 0))):
                wt = Hy.T @ w[:d_i.shape[2], :, wa::ks, we::ks] @ Hx                                 # [S,C,H,W]: the blended tap at every dy pixel
                t = (d_i * wt.transpose(1, 0, 2, 3)[None]).sum(2)
                gi += My @ t @ _scatter(rx, W).T
                if plant == "one mirror fold dropped":
                    gi -= _scatter(ry, H, uy < 0) @ t @ _scatter(rx, W).T
            if "d_maps" in want:
                t = (d_m * x[:d_m.shape[0], :, None, ry[:, None], rx[None, :]]).sum(0)               # [C,S,H,W]
                gm[:, :, wa::ks, we::ks] = (Hy @ t @ Hx.T).transpose(1, 0, 2, 3)
    return {k: torch.from_numpy(v) for k, v in (("d_img", gi), ("d_maps", gm)) if k in want}


def swapped_hat(node, n):
    """Hx with fx and 1 - fx swapped in the cell of pixel n / 3 (the centre pixel can sit at fx = 1/2, where the swap changes nothing)."""
    g = node.shape[0]
    Hm, _, k = hats64(node, n)
    cols = np.nonzero(k == k[n // 3])[0]
    c0, c1 = int(k[n // 3]), min(int(k[n // 3]) + 1, g - 1)
    Hm[[c0, c1], cols[:, None]] = Hm[[c1, c0], cols[:, None]]
    return Hm


def planted(c, r, plant):
    """{name: float64 gradient with the planted error} for the gradients the plant concerns."""
    which = PLANTS[plant]
    want = ("d_img", "d_maps") if which == "both" else (which,)
    Hx = swapped_hat(r.nx, c.W) if plant == "fx and 1-fx swapped in one cell" else r.Hx
    return def64(r.img, r.maps, r.dy, c.grid, r.Hy, Hx, plant, want)


def loop64(img, maps, dy, grid, node_y, node_x):
    """The definition as plain Python loops: per dy pixel its cell, the clamped fractions, the four corner weights; every tap of every
    corner scatters into d_img at the reflected source and into d_maps at the corner's tile.  Tiny inputs only."""
    B, Cn, H, W = img.shape
    S, ks = maps.shape[0], maps.shape[-1] // grid
    p = ks // 2
    ny, nx = [float(v) for v in node_y.double()], [float(v) for v in node_x.double()]

    def frac(nodes, q):
        if grid == 1:
            return 0, 0.0
        k = min(max(sum(1 for v in nodes if v <= q) - 1, 0), grid - 2)
        return k, min(max((q - nodes[k]) / (nodes[k + 1] - nodes[k]), 0.0), 1.0)

    refl = bc._reflect
    x64, w64, d64 = img.double().tolist(), maps.double().tolist(), dy.double().tolist()
    gi = np.zeros((B, Cn, H, W))
    gm = np.zeros((S, Cn, grid * ks, grid * ks))
    for b in range(B):
        for ch in range(Cn):
            for s in range(S):
                for y in range(H):
                    k, fy = frac(ny, y)
                    for xx in range(W):
                        l, fx = frac(nx, xx)
                        dv = d64[b][ch][s][y][xx]
                        k1, l1 = min(k + 1, grid - 1), min(l + 1, grid - 1)
                        for i, j, beta in ((k, l, (1 - fy) * (1 - fx)), (k, l1, (1 - fy) * fx), (k1, l, fy * (1 - fx)), (k1, l1, fy * fx)):
                            for u in range(ks):
                                for v in range(ks):
                                    sy, sx = refl(y - p + u, H), refl(xx - p + v, W)
                                    row, col = i * ks + ks - 1 - u, j * ks + ks - 1 - v
                                    gi[b, ch, sy, sx] += dv * beta * w64[s][ch][row][col]
                                    gm[s, ch, row, col] += dv * beta * x64[b][ch][sy][sx]
    return torch.from_numpy(gi), torch.from_numpy(gm)


# ------------------------------------------------------------------------------------------------------------------ the depths D
def tiles_of(node, n):
    """(b, ts) of csrc/blend_axis.h fill_axis: cell bounds and the first tile of every cell."""
    g = node.shape[0]
    ncell = max(g - 1, 1)
    b = [0] + [int(min(max(np.ceil(float(node[c])), 0), n)) for c in range(1, ncell)] + [n]
    ts = [0]
    for c in range(ncell):
        ts.append(ts[-1] + -(-(b[c + 1] - b[c]) // BT))
    return b, ts


def dimg_depth(c, sup_y, sup_x):
    """D of d_img per element, float64 [H, W]."""
    ks, p = c.ks, c.ks // 2

    def axis(sup, n):
        cnt = np.zeros(n)
        for q in range(n):
            cnt[q] = (sup[:, max(q - p, 0):min(q + p, n - 1) + 1].sum(1) > 0).sum()
        q = np.arange(n)
        return cnt, ((q >= 1) & (q <= p)) | ((q >= n - 1 - p) & (q <= n - 2))

    ny_, my = axis(sup_y, c.H)
    nx_, mx = axis(sup_x, c.W)
    mirror, n = my[:, None] | mx[None, :], ny_[:, None] * nx_[None, :]
    if ks in TEMPLATED_KS:
        q = np.arange(c.H)
        m_y = 1 + ((q >= 1) & (q <= p)).astype(int) + ((q >= c.H - 1 - p) & (q <= c.H - 2)).astype(int)
        q = np.arange(c.W)
        m_x = 1 + ((q >= 1) & (q <= p)).astype(int) + ((q >= c.W - 1 - p) & (q <= c.W - 2)).astype(int)
        return ks * ks + c.S * n * m_y[:, None] * m_x[None, :] + 3
    return np.where(mirror, p * ks + 8, ks) + n * (ks + 1) + c.S


def dmaps_depth(c, ny, nx):
    """D of d_maps per element of the map, float64 [g ks, g ks]."""
    g = c.grid
    ncell = max(g - 1, 1)

    def axis(node, n):
        _, ts = tiles_of(node, n)
        cnt = [ts[i + 1] - ts[i] for i in range(ncell)]
        return np.array([max(cnt[ci] for ci in range(max(i - 1, 0), min(i, ncell - 1) + 1)) for i in range(g)])

    ty, tx = axis(ny, c.H), axis(nx, c.W)
    D = 22 + np.maximum(ty[:, None] + tx[None, :] - 2, 0) + 3 + c.B - 1
    return np.repeat(np.repeat(D, c.ks, axis=0), c.ks, axis=1).astype(np.float64)


# ------------------------------------------------------------------------------------------------------------------ references
Ref = collections.namedtuple("Ref", "img maps dy ny nx Hy Hx gi gm Ai Am Mi Mm Ri Rm")
_REF = {}


def build_reference(c, img, maps, dy, ny, nx):
    Hy, sy, _ = hats64(ny, c.H)
    Hx, sx, _ = hats64(nx, c.W)
    gi, gm = autograd64(img, maps, dy, c.grid, ny, nx)
    A = def64(img.abs(), maps.abs(), dy.abs(), c.grid, Hy, Hx)
    M = def64(img.abs(), maps.abs(), dy.abs(), c.grid, sy, sx)
    N = def64(torch.ones_like(img), torch.ones_like(maps), torch.ones_like(dy), c.grid, sy, sx)
    Ri = torch.minimum(N["d_img"], torch.from_numpy(dimg_depth(c, sy, sx))[None, None])
    Rm = torch.minimum(N["d_maps"], torch.from_numpy(dmaps_depth(c, ny, nx))[None, None])
    return Ref(img, maps, dy, ny, nx, Hy, Hx, gi, gm, A["d_img"], A["d_maps"], M["d_img"], M["d_maps"], Ri, Rm)


def reference(c):
    """Ref of a case with its seeded inputs, computed once per process and shared: do not modify."""
    if c.id not in _REF:
        _REF[c.id] = build_reference(c, *inputs(c), *nodes_of(c))
    return _REF[c.id]


def bounds(r):
    """{name: the elementwise budget of the module docstring, float64}."""
    return {"d_img": (r.Ri + C1) * U * r.Ai + C2 * U * r.Mi + U * r.gi.abs(),
            "d_maps": (r.Rm + C1) * U * r.Am + C2 * U * r.Mm + U * r.gm.abs()}


def compare(got, ref64, bound):
    """(largest |got - ref64| / budget over EVERY element (0 / 0 = 0), its flat index, rel_l2)."""
    assert tuple(got.shape) == tuple(ref64.shape) and bool(torch.isfinite(got).all())
    err = (got.double() - ref64).abs()
    use = torch.where(err == 0, torch.zeros_like(err), err / bound)
    worst = int(use.argmax())
    return float(use.flatten()[worst]), worst, rel_l2(got, ref64) if float(ref64.norm()) > 0 else 0.0


# ------------------------------------------------------------------------------------------- the kernels' arithmetic in numpy float32
def frac32(node, n):
    """(k int64 [n], f float32 [n], 1 - f float32 [n]): blend_frac of csrc/blend_axis.h and __fsub_rn(1, f), step by step in float32."""
    g = node.shape[0]
    nd = node.numpy().astype(np.float32)
    k, _ = bc.axis_weights(node, n)
    if g == 1:
        f = np.zeros(n, dtype=np.float32)
    else:
        pix = np.arange(n).astype(np.float32)
        f = ((pix - nd[k]).astype(np.float32) / (nd[k + 1] - nd[k]).astype(np.float32)).astype(np.float32)
        f = np.minimum(np.maximum(f, np.float32(0)), np.float32(1))
    return k, f, (np.float32(1) - f).astype(np.float32)


def hats32(node, n):
    g = node.shape[0]
    k, f, gg = frac32(node, n)
    Hm = np.zeros((g, n), dtype=np.float32)
    ar = np.arange(n)
    Hm[k, ar] += gg
    Hm[np.minimum(k + 1, g - 1), ar] += f
    return Hm


def _fma32(acc, a, b):
    """One fmaf step of a float32 accumulator: the product of two float32 values is exact in float64."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def _mirrors(H, W, p):
    """The mirror positions of every element in the kernels' order: [(row index into the extended domain, column index, valid [H,W])]."""
    ys, xs = np.arange(H), np.arange(W)
    out = []
    for vu in range(3):
        Uv = (ys, -ys, 2 * (H - 1) - ys)[vu]
        oky = (np.ones(H, bool), (ys >= 1) & (ys <= p), (ys <= H - 2) & (ys >= H - 1 - p))[vu]
        for vv in range(3):
            Vv = (xs, -xs, 2 * (W - 1) - xs)[vv]
            okx = (np.ones(W, bool), (xs >= 1) & (xs <= p), (xs <= W - 2) & (xs >= W - 1 - p))[vv]
            if (vu, vv) != (0, 0):
                out.append((np.where(oky, Uv, 0) + p, np.where(okx, Vv, 0) + p, oky[:, None] & okx[None, :]))
    return out


def _node_T(c, d_s, Hy_i, Hx_j):
    """fl(dy * fl(Hy_i * Hx_j)) of one slice, zero-padded by 2 p: row U + a - p of the image is row U + a + p of the result."""
    p = c.ks // 2
    T = (d_s * (Hy_i[:, None] * Hx_j[None, :]).astype(np.float32)).astype(np.float32)
    return np.pad(T, ((0, 0), (0, 0), (2 * p, 2 * p), (2 * p, 2 * p)))


def _node_ext(c, Tp, wt):
    """g(U, V) of one node on the extended domain U = row - p, a zero-started fmaf chain over the taps in row-major order; taps whose
    source lies outside the image add exact zeros, so an element of it is the chain over its existing sources alone."""
    ks, p, H, W = c.ks, c.ks // 2, c.H, c.W
    ext = np.zeros((c.B, c.C, H + 2 * p, W + 2 * p), dtype=np.float32)
    for a in range(ks):
        for e in range(ks):
            ext = _fma32(ext, Tp[:, :, a:a + H + 2 * p, e:e + W + 2 * p], wt[None, :, a, e, None, None])
    return ext


def _node_fold(ext, mirrors, shape):
    fold = np.zeros(shape, dtype=np.float32)
    for iu, iv, ok in mirrors:
        fold = np.where(ok, fold + ext[:, :, iu[:, None], iv[None, :]], fold)
    return fold


def dimg_tree32(c, maps, dy, ny, nx):
    """float32 [B,C,H,W]: d_img summed as the kernel of the case's ks sums it (module docstring)."""
    return (_dimg_tree32_templated if c.ks in TEMPLATED_KS else _dimg_tree32_generic)(c, maps, dy, ny, nx)


def _pass_ext(c, Tp, wt, my, mx):
    """g(U, V) of one node on the part of the extended domain a mirror pass reads (rows U = row - p in [0, H) for my = 0, [-p, 0) for
    my = 1, [H, H + p) for my = 2; columns alike; zero elsewhere): a zero-started fmaf chain over the taps in the pass's order, a mirrored
    axis backwards."""
    ks, p, H, W = c.ks, c.ks // 2, c.H, c.W
    rows = (slice(p, p + H), slice(0, p), slice(H + p, H + 2 * p))[my]
    cols = (slice(p, p + W), slice(0, p), slice(W + p, W + 2 * p))[mx]
    ext = np.zeros((c.B, c.C, H + 2 * p, W + 2 * p), dtype=np.float32)
    sub = ext[:, :, rows, cols]
    for a in (range(ks) if my == 0 else range(ks - 1, -1, -1)):
        for e in (range(ks) if mx == 0 else range(ks - 1, -1, -1)):
            sub = _fma32(sub, Tp[:, :, rows.start + a:rows.stop + a, cols.start + e:cols.stop + e], wt[None, :, a, e, None, None])
    ext[:, :, rows, cols] = sub
    return ext


def _dimg_tree32_templated(c, maps, dy, ny, nx):
    """blend_dimg_kernel<KS>: per 32 x 32 tile the visited nodes (hat support meets the tile's window) and the mirror passes the tile has;
    the (slice, node, pass) triples s-major, then i, j, then the pass, dealt to the waves index % 4; per triple the chain in the pass's tap
    order, added where the element has that mirror image; per wave the triples in order; then the waves."""
    ks, p, g, H, W = c.ks, c.ks // 2, c.grid, c.H, c.W
    Hy, Hx = hats32(ny, H), hats32(nx, W)
    sup_y, sup_x = hats64(ny, H)[1], hats64(nx, W)[1]
    d = dy.numpy().astype(np.float32)
    w = maps.numpy().astype(np.float32)
    ys, xs = np.arange(H), np.arange(W)
    posy = [(ys, np.ones(H, bool)), (-ys, (ys >= 1) & (ys <= p)), (2 * (H - 1) - ys, (ys <= H - 2) & (ys >= H - 1 - p))]
    posx = [(xs, np.ones(W, bool)), (-xs, (xs >= 1) & (xs <= p)), (2 * (W - 1) - xs, (xs <= W - 2) & (xs >= W - 1 - p))]
    contrib = {}

    def get(s, i, j, my, mx):
        if (s, i, j, my, mx) not in contrib:
            ext = _pass_ext(c, _node_T(c, d[:, :, s], Hy[i], Hx[j]), w[s, :, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks], my, mx)
            (U, oky), (V, okx) = posy[my], posx[mx]
            contrib[(s, i, j, my, mx)] = (ext[:, :, np.where(oky, U, 0)[:, None] + p, np.where(okx, V, 0)[None, :] + p], oky[:, None] & okx[None, :])
        return contrib[(s, i, j, my, mx)]

    out = np.zeros((c.B, c.C, H, W), dtype=np.float32)
    for y0 in range(0, H, BT):
        for x0 in range(0, W, BT):
            y1, x1 = min(y0 + BT, H), min(x0 + BT, W)
            il = [i for i in range(g) if sup_y[i, max(y0 - p, 0):min(y0 + BT - 1 + p, H - 1) + 1].any()]
            jl = [j for j in range(g) if sup_x[j, max(x0 - p, 0):min(x0 + BT - 1 + p, W - 1) + 1].any()]
            pys = [m for m in range(3) if posy[m][1][y0:y1].any()]
            pxs = [m for m in range(3) if posx[m][1][x0:x1].any()]
            tot = [np.zeros((c.B, c.C, y1 - y0, x1 - x0), dtype=np.float32) for _ in range(4)]
            n = 0
            for s in range(c.S):
                for i in il:
                    for j in jl:
                        for my in pys:
                            for mx in pxs:
                                val, ok = get(s, i, j, my, mx)
                                tot[n % 4] = np.where(ok[y0:y1, x0:x1], tot[n % 4] + val[:, :, y0:y1, x0:x1], tot[n % 4])
                                n += 1
            out[:, :, y0:y1, x0:x1] = ((tot[0] + tot[1]) + tot[2]) + tot[3]
    assert out.dtype == np.float32
    return torch.from_numpy(out)


def _dimg_tree32_generic(c, maps, dy, ny, nx):
    """blend_dimg_generic_kernel: per slice the nodes in the order i, j; per node the ks column chains, then the fold."""
    ks, p, g, H, W = c.ks, c.ks // 2, c.grid, c.H, c.W
    Hy, Hx = hats32(ny, H), hats32(nx, W)
    sup_y, sup_x = hats64(ny, H)[1], hats64(nx, W)[1]
    d = dy.numpy().astype(np.float32)
    w = maps.numpy().astype(np.float32)
    mirrors = _mirrors(H, W, p)
    total = np.zeros((c.B, c.C, H, W), dtype=np.float32)
    for s in range(c.S):
        acc = np.zeros((c.B, c.C, H, W), dtype=np.float32)
        for i in range(g):
            if not sup_y[i].any():                                                               # a node no workgroup visits: it would add exact zeros
                continue
            for j in range(g):
                if not sup_x[j].any():
                    continue
                Tp = _node_T(c, d[:, :, s], Hy[i], Hx[j])
                wt = w[s, :, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks]                           # [C,ks,ks]
                for e in range(ks):
                    part = np.zeros_like(acc)
                    for a in range(ks):
                        part = _fma32(part, Tp[:, :, p + a:p + a + H, p + e:p + e + W], wt[None, :, a, e, None, None])
                    acc = acc + part
                if p:
                    acc = acc + _node_fold(_node_ext(c, Tp, wt), mirrors, acc.shape)
                assert acc.dtype == np.float32
        total = total + acc
    return torch.from_numpy(total)


def dmaps_tree32(c, img, dy, ny, nx):
    """float32 [S,C,g ks,g ks]: d_maps summed as blend_dmaps_partial_kernel and blend_dmaps_sum_kernel sum it.  Per 32 x 32 tile of a cell,
    corner q and (b, c, s): lane = 8 lyr + lxg owns rows lyr + 8 j and columns 4 lxg + k, a chain of 16 fmaf in (j, k) order from 0 over
    fl(dy * fl(wy * wx)); the wave butterfly v += v[lane ^ off], off = 32 .. 1; then per node the chains of the second pass."""
    ks, p, g, H, W = c.ks, c.ks // 2, c.grid, c.H, c.W
    ncell = max(g - 1, 1)
    by, tsy = tiles_of(ny, H)
    bx, tsx = tiles_of(nx, W)
    _, fy, gy = frac32(ny, H)
    _, fx, gx = frac32(nx, W)
    x = np.pad(img.numpy().astype(np.float32), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect") if p else img.numpy().astype(np.float32)
    x = np.pad(x, ((0, 0), (0, 0), (0, BT), (0, BT)))                      # beyond the image: finite values that meet dy = 0 only
    d = dy.numpy().astype(np.float32)
    lanes = np.arange(64)
    part = {}
    for ci in range(ncell):
        for cj in range(ncell):
            for b in range(c.B):
                for ty in range(tsy[ci + 1] - tsy[ci]):
                    for tx in range(tsx[cj + 1] - tsx[cj]):
                        y0, x0 = by[ci] + ty * BT, bx[cj] + tx * BT
                        y1, x1 = min(y0 + BT, by[ci + 1]), min(x0 + BT, bx[cj + 1])
                        win = x[b, :, y0:y0 + BT + 2 * p, x0:x0 + BT + 2 * p]
                        v = np.lib.stride_tricks.sliding_window_view(win, (BT, BT), axis=(1, 2))[:, ::-1, ::-1]      # [C,a,e,row,col]
                        v = v.reshape(c.C, 1, ks, ks, 4, 8, 8, 4)
                        for qy, wy in enumerate((gy, fy)):
                            for qx, wx in enumerate((gx, fx)):
                                wgt = np.zeros((BT, BT), dtype=np.float32)
                                wgt[:y1 - y0, :x1 - x0] = (wy[y0:y1, None] * wx[None, x0:x1]).astype(np.float32)
                                td = np.zeros((c.C, c.S, BT, BT), dtype=np.float32)
                                td[:, :, :y1 - y0, :x1 - x0] = d[b, :, :, y0:y1, x0:x1]
                                td = (td * wgt).astype(np.float32).reshape(c.C, c.S, 1, 1, 4, 8, 8, 4)
                                acc = np.zeros((c.C, c.S, ks, ks, 8, 8), dtype=np.float32)
                                for jj in range(4):
                                    for k in range(4):
                                        acc = _fma32(acc, td[:, :, :, :, jj, :, :, k], v[:, :, :, :, jj, :, :, k])
                                acc = acc.reshape(c.C, c.S, ks, ks, 64)
                                for off in (32, 16, 8, 4, 2, 1):
                                    acc = acc + acc[..., lanes ^ off]
                                assert acc.dtype == np.float32
                                part[(b, ci, cj, ty, tx, qy, qx)] = acc[..., 0].transpose(1, 0, 2, 3)
    out = np.zeros((c.S, c.C, g * ks, g * ks), dtype=np.float32)
    zero = np.zeros((c.S, c.C, ks, ks), dtype=np.float32)
    for i in range(g):
        for j in range(g):
            total = zero
            for b in range(c.B):
                sb = zero
                for ci in range(max(i - 1, 0), min(i, ncell - 1) + 1):
                    for cj in range(max(j - 1, 0), min(j, ncell - 1) + 1):
                        for qy in range(2):
                            if (min(ci + 1, g - 1) if qy else ci) != i:
                                continue
                            for qx in range(2):
                                if (min(cj + 1, g - 1) if qx else cj) != j:
                                    continue
                                scell = zero
                                for ty in range(tsy[ci + 1] - tsy[ci]):
                                    sr = zero
                                    for tx in range(tsx[cj + 1] - tsx[cj]):
                                        sr = sr + part[(b, ci, cj, ty, tx, qy, qx)]
                                    scell = scell + sr
                                sb = sb + scell
                total = total + sb
            out[:, :, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks] = total
    return torch.from_numpy(out)


def workspace_bytes(c):
    """aadff_render_psf_map_blend_stack_bwd_workspace: a bound of the tiles of an axis that holds for any nodes, (n + 31 min(ncell, n)) / 32."""
    ncell = max(c.grid - 1, 1)
    nt = lambda n: (n + (BT - 1) * min(ncell, n)) // BT      # noqa: E731
    return c.B * nt(c.H) * nt(c.W) * c.S * c.C * 4 * c.ks * c.ks * 4
