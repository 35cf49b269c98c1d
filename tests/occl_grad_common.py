"""Shared by tests/test_occl_grad_host.py and tests/test_gpu_occl_grad.py (not a test module): the cases, inputs, comparator, closed
forms, planted errors and the elementwise budget of the gradients of the occlusion-aware layered PSF-map render
(aadff_render_psf_map_stack_occluded_bwd, csrc/conv_occl_bwd.hip; aadff.diffrender.render_psf_map_occluded[_stack]).

Specification (include/aadff.h).  Forward per element (b,c,s,pi), tests/occlusion_common.py: a_l, q_l, f_l = max(1 - a_l, 0), T_l, V, A,
out.  Upstream gradients g (to out) and h (to the coverage A).
    step 1   normalize, A > 0: gV = g / A, gA = h - g out / A;   normalize, A = 0: gV = 0, gA = h;   normalize = 0: gV = g, gA = h
    step 2   G_l = gV q_l + gA a_l,  R_L = 0,  R_l = G_l + f_l R_{l+1},  alpha_l = gV T_l,  beta_l = gA T_l - [1 - a_l > 0] T_l R_{l+1}
    step 3   d_img[b,c,t] = sum_s sum_{pi, tap : refl(pi + tap - p) = t} alpha_{layer[b,t]}(b,c,s,pi) w^{s,layer[b,t]}_{patch(pi)}(tap)
             d_maps[s L + l, c, i ks + a, j ks + e] = sum_b sum_{pi in patch(i,j)} alpha_l(pi) (m_l(t) ? x(t) : 0) + beta_l(pi) (m_l(t) ? 1 : 0),
             t = refl(pi + p - (a,e))

Comparator: torch.autograd.grad in float64 through occlusion_common.occl64(..., want_bound=False) of
sum(g * out) + sum(h * A) (normalize = 0: V for out).  `occl_any` is the same comparator for any dtype (bit-equal to occl64 in float64;
its float32 autograd gives d32, the reference's own error); `closed64` evaluates the three steps above in float64 (steps 1-2 in torch,
step 3 tap by tap in numpy, `def64`), and `loop64` restates them as plain Python loops for tiny inputs.

The indicator [1 - a_l > 0] is the one discontinuity.  `indicator_margin` returns, over the elements where anything lies behind layer l
(sum_{k>l} a_k > 0), the smallest |1 - a_l| / (16 ((ks^2 + 1) U a_l + U)): the host test asserts it is >= 1 for every case, so the
float32 and the float64 indicator agree wherever R_{l+1} != 0 (where nothing lies behind, R_{l+1} is exactly 0 in both and the
indicator is irrelevant), and torch's clamp, which passes the gradient at equality, agrees with the contract.

Budget - elementwise, no element excluded, no constant taken from a kernel's output.  U = 2^-24, n = ks^2.  It is a running error
bound that follows csrc/conv_occl_bwd.hip operation by operation.  A computed float32 value x^ is carried as (x, e) with |x^ - x| <= e:
    fl(x^ y^)        : e0 = |x| ey + |y| ex + ex ey,                 e = e0 + U (|x y| + e0)
    fl(x^ y^ + z^)   : e0 = (the product's e0) + ez,                 e = e0 + U (|x y + z| + e0)          (one fma, one rounding)
    fl(1 - a^)       : e0 = ea,                                      e = e0 + U (|1 - a| + e0);   max(., 0) is 1-Lipschitz
    fl(x^ / y^)      : e0 = (ex + |x / y| ey) / (|y| - ey),          e = e0 + U (|x / y| + e0)            (|y| > ey is asserted)
(the rounding of an operation is at most U times the magnitude of its unrounded computed result, which is within e0 of the exact one).
  (1) stage 1, occl_grad_layers_*: q^_l, a^_l are the forward's chains, e_q = (n + 1) U Q_l, e_a = (n + 1) U a_l (occlusion_common,
      point (1)); f^_l = max(fl(1 - a^_l), 0); V, A, T by the forward's composite (fma, fma, product) - this reproduces E_l, e_V, e_A of
      occlusion_common - and out^ = fl(V^ / A^).
  (2) step 1: gV^ = fl(g / A^) and gA^ = fl(-gV^ out^ + h) (one fma), g and h exact; where A = 0 (an exact decision with positive PSFs)
      gV^ = 0 and gA^ = h exactly; normalize = 0: both exact.
  (3) the recursion, back to front: G^_l = fl(gV^ q^_l + fl(gA^ a^_l)), R^_l = fl(f^_l R^_{l+1} + G^_l), R_L = 0 exactly.  Then front to
      back alpha^_l = fl(gV^ T^_l), t^ = fl(gA^ T^_l), beta^_l = fl(-T^_l R^_{l+1} + t^) where 1 - a^_l > 0, else t^ (the same branch
      as the exact indicator under the margin condition above).  A layer absent from the staged tile is skipped by the kernel; it has
      q = a = 0 exactly, and carrying it through the same formulas only adds to the bound.
  (4) the sums.  A float32 sum of exactly formed products (every product is inside an fma) whose term passes at most D roundings is
      within ((1 + U)^D - 1) sum |term^| <= 1.01 D U sum |term^| (D U < 0.01) of the sum of its computed terms, and those are within
      sum |weight| e of the exact ones.  With lin(.) the linear map of step 3 evaluated at absolute values (`def64`):
          d_img : lin_img(e_alpha; |w|) + 1.01 (D + 1) U lin_img(|alpha| + e_alpha; |w|)
          d_maps: lin_maps(e_alpha, e_beta; |x|, m) + 1.01 (D + 1) U lin_maps(|alpha| + e_alpha, |beta| + e_beta; |x|, m)
      D is the smaller of the element's term count N (`def64` at all-ones inputs: terms that are exact zeros add nothing) and the depth
      of the kernel's summation tree, read from the code:
        occl_grad_dimg_kernel<KS>: per slice and the texel's layer: per patch that meets the wave's window (at most `pn` of them: the
          patches met by 8 + 2p rows times those met by 32 + 2p columns) and tap column a zero-started chain of ks fma (ks roundings),
          `acc += part` (one per column: pn ks), the mirror terms of the patch as one zero-started fma chain (at most 8 positions of at
          most ks^2 sources: 8 ks^2, elements with a mirror image only) and `acc += part` (pn); `total += keep` over the slices (S):
              D = ks + pn (ks + 1) + S  (+ 8 ks^2 for an element with a mirror image)
        occl_grad_dmaps_partial_kernel<EB> + occl_grad_dmaps_sum_kernel: a lane's zero-started chain of 32 fma (16 pixels, alpha then
          beta: 32), the wave butterfly (6); the second pass adds, each level started at 0 (0 + x is exact), the tile columns (txn - 1),
          the tile rows (tyn - 1) and the batch (B - 1):
              D = 38 + (txn - 1) + (tyn - 1) + (B - 1)
      Neither depends on how many slices a pass of the entry takes: d_img adds each slice's whole value to a running sum in ascending s
      and d_maps has no sum over slices.
Underflow is outside the model; the inputs (images in [-3, 34.5), tile-normalised PSFs >= 1e-3 / ks^2 / 21, randn gradients) keep every
product far above the subnormal range.

`tree32_stage1`, `tree32_dimg` and `tree32_dmaps` restate the three stages in numpy float32 in the kernels' operation and summation order
(an fma as the float64 sum of the exact product and the accumulator, rounded to float32); the host test chains them and holds the result
to the budget on every case.
"""
import collections

import numpy as np
import torch

import occlusion_common as oc
from oracle import conv as oconv

U = oc.U
GT = 32
SENTINEL = oc.SENTINEL
TEMPLATED_KS = oc.TEMPLATED_KS
HOLE = oc.HOLE

Case = collections.namedtuple("Case", "id B C S L H W grid ks scene reaches")


def _case(B, C, S, L, H, W, grid, ks, scene, reaches):
    return Case(f"{B}x{C}x{S}x{L}-{H}x{W}-g{grid}-ks{ks}", B, C, S, L, H, W, grid, ks, scene, reaches)


CLAMP = _case(1, 1, 1, 2, 24, 28, 2, 3, "clamp", "tiles 1.4/9 (1 + 0.01 r): a_0 > 1 with layer 1 in the window, the clamp bites")
WS_CASE = _case(2, 1, 3, 3, 40, 70, 3, 7, "random+hole2", "B = 2 and S = 3: minimum against full workspace, the batch and the slice sums")
TABLE = [Case(c.id, c.B, c.C, c.S, c.L, c.H, c.W, c.grid, c.ks, c.scene, c.reaches) for c in oc.TABLE] + [
    CLAMP,
    _case(1, 1, 2, 2, 6, 7, 2, 11, "random", "H = ks/2 + 1, templated: every row is mirrored and the corner folds run"),
    _case(1, 1, 1, 2, 10, 12, 2, 19, "random", "H = ks/2 + 1 on the run-time-ks kernel"),
    WS_CASE,
]
TINY = [(1, 2, 2, 3, 7, 9, 3, 3), (2, 1, 1, 2, 6, 5, 2, 3), (1, 1, 1, 2, 4, 5, 1, 5)]         # B, C, S, L, H, W, grid, ks
COMBOS = [(1, True), (1, False), (0, True), (0, False)]                                      # (normalize, with h)


def kernels(ks):
    """The instantiations aadff_render_psf_map_stack_occluded_bwd launches, as the library's symbol table spells them."""
    first = f"occl_grad_layers_kernel<{ks}>" if ks in TEMPLATED_KS else "occl_grad_layers_generic_kernel"
    tuned = ks == 11
    return {first, "occl_grad_dimg_kernel<11>" if tuned else "occl_grad_dimg_kernel<0>",
            "occl_grad_dmaps_partial_kernel<11>" if tuned else "occl_grad_dmaps_partial_kernel<1>", "occl_grad_dmaps_sum_kernel"}


def expected_instantiations():
    return set().union(*(kernels(k) for k in TEMPLATED_KS + (17,)))


def rel_l2(a, b):
    a, b = torch.as_tensor(a).double(), torch.as_tensor(b).double()
    n = float(b.norm())
    return float((a - b).norm()) / n if n > 0 else float((a - b).norm())


# ------------------------------------------------------------------------------------------------------------------------- inputs
def inputs(c):
    """(img, maps, layer uint8, g, h) on the CPU: the forward's seeded family, g and h = randn (both signs)."""
    if c.scene == "clamp":
        gen = torch.Generator().manual_seed(77)
        img = torch.rand((c.B, c.C, c.H, c.W), generator=gen) * 37.5 - 3.0
        r = torch.rand((c.S * c.L, c.C, c.grid * c.ks, c.grid * c.ks), generator=gen) * 2.0 - 1.0
        maps = (1.4 / 9.0 * (1.0 + 0.01 * r)).float().contiguous()
        lay = torch.randint(0, c.L, (c.B, c.H, c.W), generator=gen, dtype=torch.int64).to(torch.uint8)
    else:
        img, maps, lay = oc.inputs(oc.Case(c.id, c.B, c.C, c.S, c.L, c.H, c.W, c.grid, c.ks, c.scene, None, c.reaches))
    gen = torch.Generator().manual_seed(1301 + 2003 * c.ks + 31 * c.H + 7 * c.W + 3 * c.S + c.grid + 17 * c.B + 101 * c.L)
    g = torch.randn((c.B, c.C, c.S, c.H, c.W), generator=gen)
    h = torch.randn((c.B, c.C, c.S, c.H, c.W), generator=gen)
    return img.contiguous(), maps.contiguous(), lay.contiguous(), g, h


def tiny_inputs(t):
    B, Cn, S, L, H, W, grid, ks = t
    gen = torch.Generator().manual_seed(sum(t) + 3)
    img = torch.rand((B, Cn, H, W), generator=gen) * 37.5 - 3.0
    maps = oc.positive_maps(S * L, Cn, grid, ks, gen)
    lay = torch.randint(0, L + 1, (B, H, W), generator=gen).to(torch.uint8)                  # index L: holes
    g, h = torch.randn((B, Cn, S, H, W), generator=gen), torch.randn((B, Cn, S, H, W), generator=gen)
    return img, maps, lay, g, h


# --------------------------------------------------------------------------------------------------------------------- comparator
def occl_any(img, maps, layer, L, grid):
    """(V, A, out) in the dtype of `img`: occlusion_common.occl64's operations in its order (float64: bit-equal to it)."""
    B, Cn, H, W = img.shape
    S = maps.shape[0] // L
    lay = layer.to(torch.int64)[:, None].expand(B, Cn, H, W)
    Vs, As = [], []
    for s in range(S):
        T = torch.ones((B, Cn, H, W), dtype=img.dtype)
        v, a_ = torch.zeros_like(T), torch.zeros_like(T)
        for l in range(L):
            on = lay == l
            q = oconv.render_psf_map(torch.where(on, img, 0.0), maps[s * L + l], grid)
            a = oconv.render_psf_map(on.to(img.dtype), maps[s * L + l], grid)
            v, a_ = v + T * q, a_ + T * a
            T = T * torch.clamp(1.0 - a, min=0.0)
        Vs.append(v)
        As.append(a_)
    V, A = torch.stack(Vs, 2), torch.stack(As, 2)
    seen = A > 0
    return V, A, torch.where(seen, V / torch.where(seen, A, 1.0), 0.0)


def autograd_ref(img, maps, layer, L, grid, g, h, normalize, dtype=torch.float64):
    """(d_img, d_maps) in `dtype`: autograd of sum(g out) + sum(h A) through occl64 (float64) / occl_any (float32)."""
    x = img.detach().to(dtype).clone().requires_grad_(True)
    m = maps.detach().to(dtype).clone().requires_grad_(True)
    if dtype == torch.float64:
        r = oc.occl64(x, m, layer, L, grid, want_bound=False)
        V, A, out = r.V, r.A, r.out
    else:
        V, A, out = occl_any(x, m, layer, L, grid)
    loss = ((out if normalize else V) * g.to(dtype)).sum()
    if h is not None:
        loss = loss + (A * h.to(dtype)).sum()
    gi, gm = torch.autograd.grad(loss, (x, m))
    return gi.detach(), gm.detach()


# ------------------------------------------------------------------------------------------- running error bounds (module docstring)
class Q:
    """A computed float32 quantity: exact value v (float64) and a bound e of |computed - v|."""
    __slots__ = ("v", "e")

    def __init__(self, v, e=None):
        self.v = v
        self.e = torch.zeros_like(v) if e is None else e


def _rnd(v, e0):
    return Q(v, e0 + U * (v.abs() + e0))


def q_mul(x, y):
    return _rnd(x.v * y.v, x.v.abs() * y.e + y.v.abs() * x.e + x.e * y.e)


def q_fma(x, y, z):
    return _rnd(x.v * y.v + z.v, x.v.abs() * y.e + y.v.abs() * x.e + x.e * y.e + z.e)


def q_one_minus(a):
    return _rnd(1.0 - a.v, a.e)


def q_div(x, y, where):
    """x / y where `where` (there |y| - e_y > 0 is asserted), (0, 0) elsewhere."""
    den = torch.where(where, y.v.abs() - y.e, 1.0)
    assert bool((den > 0).all())
    v = torch.where(where, x.v / torch.where(where, y.v, 1.0), 0.0)
    r = _rnd(v, (x.e + v.abs() * y.e) / den)
    return Q(v, torch.where(where, r.e, 0.0))


Parts = collections.namedtuple("Parts", "q a Qabs")       # lists over s of lists over l of float64 [B,C,H,W]


def layer_parts(img, maps, layer, L, grid):
    B, Cn, H, W = img.shape
    S = maps.shape[0] // L
    x64, lay = img.double(), layer.to(torch.int64)[:, None].expand(B, Cn, H, W)
    q, a, Qa = [], [], []
    for s in range(S):
        qs, as_, Qs = [], [], []
        for l in range(L):
            on, m64 = lay == l, maps[s * L + l].double()
            qs.append(oconv.render_psf_map(torch.where(on, x64, 0.0), m64, grid))
            as_.append(oconv.render_psf_map(on.double(), m64, grid))
            Qs.append(oconv.render_psf_map(torch.where(on, x64.abs(), 0.0), m64, grid))
        q.append(qs)
        a.append(as_)
        Qa.append(Qs)
    return Parts(q, a, Qa)


PLANTS = {
    "one tap dropped": "d_img",
    "one mirror fold dropped": "d_img",
    "the beta term dropped": "d_maps",
    "the indicator dropped": "d_maps",
    "R accumulated front to back": "d_maps",
    "g out / A with the wrong sign": "d_maps",
    "one slice missing": "d_img",
    "one batch item missing": "d_maps",
    "the unflipped PSF": "both",
    "the image multiplied instead of selected": "d_maps",
}


def alpha_beta(c, parts, g, h, normalize, plant=None):
    """Steps 1 and 2 in float64 with their running error bounds: (alpha, beta, e_alpha, e_beta) float64 [B,C,S,L,H,W]."""
    n1 = c.ks * c.ks + 1
    zero = torch.zeros((c.B, c.C, c.H, c.W), dtype=torch.float64)
    out = [torch.zeros((c.B, c.C, c.S, c.L, c.H, c.W), dtype=torch.float64) for _ in range(4)]
    for s in range(c.S):
        qs = [Q(parts.q[s][l], n1 * U * parts.Qabs[s][l]) for l in range(c.L)]
        as_ = [Q(parts.a[s][l], n1 * U * parts.a[s][l]) for l in range(c.L)]
        f1 = [q_one_minus(a) for a in as_]
        fs = [Q(torch.clamp(f.v, min=0.0), f.e) for f in f1]
        T, V, A = [Q(torch.ones_like(zero))], Q(zero.clone()), Q(zero.clone())
        for l in range(c.L):
            V, A = q_fma(T[l], qs[l], V), q_fma(T[l], as_[l], A)
            T.append(q_mul(T[l], fs[l]))
        gq = Q(g[:, :, s].double())
        hq = Q(h[:, :, s].double() if h is not None else zero.clone())
        if normalize:
            seen = A.v > 0
            o = q_div(V, A, seen)
            gV = q_div(gq, A, seen)
            sign = 1.0 if plant == "g out / A with the wrong sign" else -1.0
            gA = q_fma(Q(sign * gV.v, gV.e), o, hq)
            gA = Q(torch.where(seen, gA.v, hq.v), torch.where(seen, gA.e, 0.0))
        else:
            gV, gA = gq, hq
        R = Q(zero.clone())
        Rn = [None] * c.L
        order = range(c.L) if plant == "R accumulated front to back" else range(c.L - 1, -1, -1)
        for l in order:
            Rn[l] = R
            R = q_fma(fs[l], R, q_fma(gV, qs[l], q_mul(gA, as_[l])))
        for l in range(c.L):
            al, tg = q_mul(gV, T[l]), q_mul(gA, T[l])
            full = q_fma(Q(-T[l].v, T[l].e), Rn[l], tg)
            ind = torch.ones_like(zero, dtype=torch.bool) if plant == "the indicator dropped" else f1[l].v > 0
            out[0][:, :, s, l], out[2][:, :, s, l] = al.v, al.e
            out[1][:, :, s, l], out[3][:, :, s, l] = torch.where(ind, full.v, tg.v), torch.where(ind, full.e, tg.e)
    if plant == "the beta term dropped":
        out[1] = torch.zeros_like(out[1])
    return out


def indicator_margin(c, parts):
    """min over (s, l, element with sum_{k>l} a_k > 0) of |1 - a_l| / (16 ((ks^2 + 1) U a_l + U)); inf if nothing ever lies behind."""
    n1, worst = c.ks * c.ks + 1, float("inf")
    for s in range(c.S):
        behind = torch.zeros_like(parts.a[s][0])
        for l in range(c.L - 1, -1, -1):
            a = parts.a[s][l]
            sel = behind > 0
            if bool(sel.any()):
                worst = min(worst, float(((1.0 - a).abs() / (16 * (n1 * U * a + U)))[sel].min()))
            behind = behind + a
    return worst


# --------------------------------------------------------------------------------------------------------- step 3, tap by tap
def _refl(v, n):
    v = np.abs(v)
    return np.where(v >= n, 2 * n - 2 - v, v)


def _scatter(src, n, keep=None):
    """[n, n] float64: M[src[y], y] = 1 (columns where keep is False stay zero)."""
    m = np.zeros((n, n))
    cols = np.arange(n) if keep is None else np.arange(n)[keep]
    m[src[cols], cols] = 1.0
    return m


def bounds_of(n, grid):
    return [int(i / grid * n) for i in range(grid + 1)]


def patch_index(n, grid):
    return np.searchsorted(np.array(bounds_of(n, grid)[1:]), np.arange(n), side="right")


def masked(img, layer, L, product=False):
    """(xm, mk) float64 numpy [L,B,C,H,W]: the image selected (or, as a planted error, multiplied) by the layer masks; the masks."""
    x = img.double().numpy()
    lay = layer.numpy().astype(np.int64)[None, :, None] == np.arange(L)[:, None, None, None, None]       # [L,B,1,H,W]
    mk = np.broadcast_to(lay, (L,) + x.shape).astype(np.float64)
    xm = x[None] * mk if product else np.where(mk > 0, x[None], 0.0)
    return xm, mk


def def64(c, xm, mk, w, al, be, layer, plant=None, want=("d_img", "d_maps")):
    """Step 3 tap by tap in float64 numpy for ANY planes: xm, mk [L,B,C,H,W], w [S L,C,G,G], al, be [B,C,S,L,H,W] -> {name: tensor}."""
    ks, p, g, H, W, S, L = c.ks, c.ks // 2, c.grid, c.H, c.W, c.S, c.L
    w6 = np.asarray(w, dtype=np.float64).reshape(S, L, c.C, g * ks, g * ks)
    al, be = np.asarray(al, dtype=np.float64), np.asarray(be, dtype=np.float64)
    ys, xs, iy, jx = np.arange(H), np.arange(W), patch_index(H, g), patch_index(W, g)
    Py, Px = np.zeros((g, H)), np.zeros((g, W))
    Py[iy, ys] = 1.0
    Px[jx, xs] = 1.0
    Si = S - 1 if plant == "one slice missing" else S
    Bm = c.B - 1 if plant == "one batch item missing" else c.B
    gil = np.zeros((c.B, c.C, L, H, W))
    gm = np.zeros((S, L, c.C, g * ks, g * ks))
    for a in range(ks):
        uy = ys + p - a
        ry = _refl(uy, H)
        My = _scatter(ry, H)
        for e in range(ks):
            rx = _refl(xs + p - e, W)
            MxT = _scatter(rx, W).T
            wa, we = (ks - 1 - a, ks - 1 - e) if plant == "the unflipped PSF" else (a, e)
            if "d_img" in want and not (plant == "one tap dropped" and (a, e) == (p, max(p - 1, 0))):
                wt = w6[:Si, :, :, (iy * ks + wa)[:, None], (jx * ks + we)[None, :]]                          # [S,L,C,H,W]
                t = np.einsum("bcslyx,slcyx->bclyx", al[:, :, :Si], wt)
                gil += My @ t @ MxT
                if plant == "one mirror fold dropped":
                    gil -= _scatter(ry, H, uy < 0) @ t @ MxT
            if "d_maps" in want:
                xv, mv = xm[:, :Bm][..., ry[:, None], rx[None, :]], mk[:, :Bm][..., ry[:, None], rx[None, :]]
                t = np.einsum("bcslyx,lbcyx->slcyx", al[:Bm], xv) + np.einsum("bcslyx,lbcyx->slcyx", be[:Bm], mv)
                gm[:, :, :, wa::ks, we::ks] = Py @ t @ Px.T
    res = {}
    if "d_img" in want:
        sel = layer.numpy().astype(np.int64)[:, None, None] == np.arange(L)[None, None, :, None, None]        # [B,1,L,H,W]
        res["d_img"] = torch.from_numpy(np.where(sel, gil, 0.0).sum(2))
    if "d_maps" in want:
        res["d_maps"] = torch.from_numpy(gm.reshape(S * L, c.C, g * ks, g * ks))
    return res


def lin_fast(c, xm, mk, w, al, be, layer):
    """`def64` without planted errors through torch's conv2d autograd (the step-3 maps are the two vector-Jacobian products of
    oracle.conv.render_psf_map, which is linear in the image and in the map): the same sums, not tap by tap.  The host test holds the
    two against each other."""
    xm, mk, w, al, be = (torch.as_tensor(np.ascontiguousarray(t), dtype=torch.float64) for t in (xm, mk, w, al, be))
    gi, gm = torch.zeros((c.B, c.C, c.H, c.W), dtype=torch.float64), torch.zeros_like(w)
    lay = layer.to(torch.int64)[:, None].expand(c.B, c.C, c.H, c.W)
    for s in range(c.S):
        for l in range(c.L):
            wv, xv = w[s * c.L + l].clone().requires_grad_(True), xm[l].clone().requires_grad_(True)
            dx, dw = torch.autograd.grad(oconv.render_psf_map(xv, wv, c.grid), (xv, wv), al[:, :, s, l].contiguous())
            dw2, = torch.autograd.grad(oconv.render_psf_map(mk[l].contiguous(), wv, c.grid), wv, be[:, :, s, l].contiguous())
            gi = gi + torch.where(lay == l, dx, 0.0)
            gm[s * c.L + l] = dw + dw2
    return {"d_img": gi, "d_maps": gm}


def _flip_tiles(w, grid, ks):
    n, Cn = w.shape[:2]
    return np.ascontiguousarray(w.reshape(n, Cn, grid, ks, grid, ks)[:, :, :, ::-1, :, ::-1]).reshape(n, Cn, grid * ks, grid * ks)


def closed64(c, img, maps, layer, g, h, normalize, plant=None, parts=None, tap_by_tap=False):
    """{d_img, d_maps} float64 by the closed forms (with a planted error of PLANTS: only the gradients it concerns).  Step 3 through
    `lin_fast`; tap by tap (`def64`) on request and for the dropped mirror fold, which only that form can express."""
    parts = parts or layer_parts(img, maps, layer, c.L, c.grid)
    al, be, _, _ = (t.numpy() for t in alpha_beta(c, parts, g, h, normalize, plant))
    which = PLANTS.get(plant, "both")
    want = ("d_img", "d_maps") if which == "both" else (which,)
    x, w, p = img, maps.double().numpy(), c.ks // 2
    if plant == "the image multiplied instead of selected":
        x = img.clone()
        x[layer[:, None].expand_as(img) >= c.L] = float("nan")
    xm, mk = masked(x, layer, c.L, product=plant == "the image multiplied instead of selected")
    if tap_by_tap or plant == "one mirror fold dropped":
        res = def64(c, xm, mk, w, al, be, layer, plant, want)
        return {k: res[k] for k in want}
    if plant == "one slice missing":
        al = al.copy()
        al[:, :, c.S - 1] = 0.0
    if plant == "one batch item missing":
        al, be = al.copy(), be.copy()
        al[c.B - 1], be[c.B - 1] = 0.0, 0.0
    if plant == "one tap dropped":
        w = w.copy()
        w.reshape(-1, c.C, c.grid, c.ks, c.grid, c.ks)[:, :, :, p, :, max(p - 1, 0)] = 0.0
    if plant == "the unflipped PSF":
        res = {"d_img": lin_fast(c, xm, mk, _flip_tiles(w, c.grid, c.ks), al, be, layer)["d_img"],
               "d_maps": torch.from_numpy(_flip_tiles(lin_fast(c, xm, mk, w, al, be, layer)["d_maps"].numpy(), c.grid, c.ks))}
    else:
        res = lin_fast(c, xm, mk, w, al, be, layer)
    return {k: res[k] for k in want}


def plant_changes_a_term(c, plant, layer):
    if plant == "the image multiplied instead of selected":
        return bool((layer >= c.L).any())                       # a NaN needs a hole to sit on
    if plant == "the indicator dropped":
        return c.scene == "clamp"                               # elsewhere 1 - a_l > 0 wherever anything lies behind
    if plant == "R accumulated front to back":
        return c.L >= 2
    return True


def loop64(img, maps, layer, L, grid, g, h, normalize):
    """The three steps as plain Python loops, element by element: (d_img, d_maps) float64.  Tiny inputs only."""
    B, Cn, H, W = img.shape
    S, ks = maps.shape[0] // L, maps.shape[-1] // grid
    p = ks // 2
    hb, wb = bounds_of(H, grid), bounds_of(W, grid)
    x64, w64, lay = img.double().tolist(), maps.double().tolist(), layer.tolist()
    g64, h64 = g.double().tolist(), (h.double().tolist() if h is not None else None)
    gi, gm = np.zeros((B, Cn, H, W)), np.zeros((S * L, Cn, grid * ks, grid * ks))
    for b in range(B):
        for ch in range(Cn):
            for s in range(S):
                for y in range(H):
                    i = max(k for k in range(grid) if hb[k] <= y)
                    for x in range(W):
                        j = max(k for k in range(grid) if wb[k] <= x)
                        taps = [(oc._reflect(y - p + u, H), oc._reflect(x - p + v, W), i * ks + ks - 1 - u, j * ks + ks - 1 - v)
                                for u in range(ks) for v in range(ks)]
                        q, a = [0.0] * L, [0.0] * L
                        for ty, tx, row, col in taps:
                            l = lay[b][ty][tx]
                            if l < L:
                                a[l] += w64[s * L + l][ch][row][col]
                                q[l] += w64[s * L + l][ch][row][col] * x64[b][ch][ty][tx]
                        T, V, A = [1.0], 0.0, 0.0
                        for l in range(L):
                            V, A = V + T[l] * q[l], A + T[l] * a[l]
                            T.append(T[l] * max(1.0 - a[l], 0.0))
                        gg, hh = g64[b][ch][s][y][x], (h64[b][ch][s][y][x] if h64 is not None else 0.0)
                        if normalize:
                            gV, gA = (gg / A, hh - gg * (V / A) / A) if A > 0 else (0.0, hh)
                        else:
                            gV, gA = gg, hh
                        R = 0.0
                        for l in range(L - 1, -1, -1):
                            alpha = gV * T[l]
                            beta = gA * T[l] - (T[l] * R if 1.0 - a[l] > 0 else 0.0)
                            R = gV * q[l] + gA * a[l] + max(1.0 - a[l], 0.0) * R
                            for ty, tx, row, col in taps:
                                if lay[b][ty][tx] == l:
                                    gi[b, ch, ty, tx] += alpha * w64[s * L + l][ch][row][col]
                                    gm[s * L + l, ch, row, col] += alpha * x64[b][ch][ty][tx] + beta
    return torch.from_numpy(gi), torch.from_numpy(gm)


# ------------------------------------------------------------------------------------------------------------------ the depths D
def _max_patches(n, grid, length):
    """The most patches of an axis that any window of `length` pixels (clipped to the image) meets."""
    idx = patch_index(n, grid)
    return max(int(idx[min(lo + length - 1, n - 1)] - idx[lo]) + 1 for lo in range(n))


def dimg_depth(c):
    ks, p = c.ks, c.ks // 2
    pn = _max_patches(c.H, c.grid, 8 + 2 * p) * _max_patches(c.W, c.grid, GT + 2 * p)
    ys, xs = np.arange(c.H), np.arange(c.W)
    my = ((ys >= 1) & (ys <= p)) | ((ys >= c.H - 1 - p) & (ys <= c.H - 2))
    mx = ((xs >= 1) & (xs <= p)) | ((xs >= c.W - 1 - p) & (xs <= c.W - 2))
    return ks + pn * (ks + 1) + c.S + np.where(my[:, None] | mx[None, :], 8 * ks * ks, 0)


def dmaps_depth(c):
    hb, wb = bounds_of(c.H, c.grid), bounds_of(c.W, c.grid)
    ty = np.array([-(-(hb[i + 1] - hb[i]) // GT) for i in range(c.grid)])
    tx = np.array([-(-(wb[i + 1] - wb[i]) // GT) for i in range(c.grid)])
    D = 38 + (ty[:, None] - 1) + (tx[None, :] - 1) + (c.B - 1)
    return np.repeat(np.repeat(D, c.ks, axis=0), c.ks, axis=1).astype(np.float64)


def workspace_bytes(c, S=None, need_maps=True):
    """aadff_render_psf_map_stack_occluded_bwd_workspace: alpha and beta per (b,c,s,l,pixel) and one partial per tile of a patch."""
    S = c.S if S is None else S
    hb, wb = bounds_of(c.H, c.grid), bounds_of(c.W, c.grid)
    nty = max(-(-(hb[i + 1] - hb[i]) // GT) for i in range(c.grid))
    ntx = max(-(-(wb[i + 1] - wb[i]) // GT) for i in range(c.grid))
    per = 2 * c.B * c.C * c.L * c.H * c.W + (c.B * ntx * nty * c.L * c.C * c.grid * c.grid * c.ks * c.ks if need_maps else 0)
    return S * per * 4


# ------------------------------------------------------------------------------------------------------------------ references
Ref = collections.namedtuple("Ref", "gi gm bi bm d32i d32m ci cm")
_IN, _PARTS, _N, _REF = {}, {}, {}, {}


def case_inputs(c):
    if c.id not in _IN:
        _IN[c.id] = inputs(c)
    return _IN[c.id]


def case_parts(c):
    if c.id not in _PARTS:
        img, maps, lay, _, _ = case_inputs(c)
        _PARTS[c.id] = layer_parts(img, maps, lay, c.L, c.grid)
    return _PARTS[c.id]


def _counts(c):
    """{d_img, d_maps}: the term counts N (`def64` at all-ones planes, maps and image, the masks as they are)."""
    if c.id not in _N:
        img, maps, lay, _, _ = case_inputs(c)
        _, mk = masked(img, lay, c.L)
        ones = np.ones((c.B, c.C, c.S, c.L, c.H, c.W))
        n = lin_fast(c, mk, mk, np.ones(tuple(maps.shape)), ones, ones, lay)
        _N[c.id] = {k: v.round() for k, v in n.items()}
    return _N[c.id]


def reference(c, normalize, with_h):
    """Ref of a case and combination: autograd64 gradients (gi, gm), the elementwise budgets (bi, bm), d32 of either gradient (the rel-L2
    of torch float32 autograd through the same comparator), and the closed-form gradients (ci, cm).  Computed once, shared: do not modify."""
    key = (c.id, normalize, with_h)
    if key not in _REF:
        img, maps, lay, g, h = case_inputs(c)
        hh = h if with_h else None
        gi, gm = autograd_ref(img, maps, lay, c.L, c.grid, g, hh, normalize)
        gi32, gm32 = autograd_ref(img, maps, lay, c.L, c.grid, g, hh, normalize, torch.float32)
        parts = case_parts(c)
        al, be, eal, ebe = (t.numpy() for t in alpha_beta(c, parts, g, hh, normalize))
        xm, mk = masked(img, lay, c.L)
        w = maps.double().numpy()
        closed = lin_fast(c, xm, mk, w, al, be, lay)
        lin_e = lin_fast(c, np.abs(xm), mk, np.abs(w), eal, ebe, lay)
        lin_a = lin_fast(c, np.abs(xm), mk, np.abs(w), np.abs(al) + eal, np.abs(be) + ebe, lay)
        n = _counts(c)
        Di = torch.minimum(n["d_img"], torch.from_numpy(dimg_depth(c).astype(np.float64))[None, None])
        Dm = torch.minimum(n["d_maps"], torch.from_numpy(dmaps_depth(c))[None, None])
        bi = lin_e["d_img"] + 1.01 * (Di + 1) * U * lin_a["d_img"]
        bm = lin_e["d_maps"] + 1.01 * (Dm + 1) * U * lin_a["d_maps"]
        _REF[key] = Ref(gi, gm, bi, bm, rel_l2(gi32, gi), rel_l2(gm32, gm), closed["d_img"], closed["d_maps"])
    return _REF[key]


def compare(got, ref64, bound):
    """(largest |got - ref64| / budget over EVERY element (0 / 0 = 0, a non-finite value or an error over a zero budget: inf), its index)."""
    assert tuple(got.shape) == tuple(ref64.shape)
    err = (got.double() - ref64).abs()
    err = torch.where(torch.isfinite(err), err, float("inf"))
    use = torch.where(err == 0, torch.zeros_like(err), err / torch.where(bound > 0, bound, 1.0))
    use = torch.where((err > 0) & ~(bound > 0), float("inf"), use)
    worst = int(use.argmax())
    return float(use.flatten()[worst]), worst


# ------------------------------------------------------------------------------------------- the kernels' arithmetic in numpy float32
def _fma32(a, b, acc):
    """One fmaf step: the product of two float32 values is exact in float64."""
    return (acc.astype(np.float64) + a.astype(np.float64) * b.astype(np.float64)).astype(np.float32)


def tree32_stage1(c, img, maps, layer, g, h, normalize):
    """(alpha, beta) float32 [B,C,S,L,H,W] as occl_grad_layers_* forms them: the forward's chains over the taps in row-major order from 0
    (a select on the layer byte), the composite, step 1 and the two walks of csrc/conv_occl_bwd.hip, operation by operation."""
    ks, p, gr, H, W, L = c.ks, c.ks // 2, c.grid, c.H, c.W, c.L
    x = np.pad(img.numpy().astype(np.float32), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect")
    lay = np.pad(layer.numpy().astype(np.int64), ((0, 0), (p, p), (p, p)), mode="reflect")[:, None]
    w = maps.numpy().astype(np.float32).reshape(c.S, L, c.C, gr * ks, gr * ks)
    iy, jx = patch_index(H, gr), patch_index(W, gr)
    one, zero = np.float32(1), np.float32(0)
    al = np.zeros((c.B, c.C, c.S, L, H, W), dtype=np.float32)
    be = np.zeros_like(al)
    for s in range(c.S):
        q = np.zeros((L, c.B, c.C, H, W), dtype=np.float32)
        a = np.zeros_like(q)
        for l in range(L):
            for u in range(ks):
                for v in range(ks):
                    wt = w[s, l][:, (iy * ks + ks - 1 - u)[:, None], (jx * ks + ks - 1 - v)[None, :]][None]          # [1,C,H,W]
                    on = lay[:, :, u:u + H, v:v + W] == l
                    q[l] = _fma32(wt, np.where(on, x[:, :, u:u + H, v:v + W], zero), q[l])
                    a[l] = _fma32(wt, np.where(on, one, zero).astype(np.float32), a[l])
        V, A, T = np.zeros_like(q[0]), np.zeros_like(q[0]), [np.ones_like(q[0])]
        for l in range(L):
            V, A = _fma32(T[l], q[l], V), _fma32(T[l], a[l], A)
            T.append((T[l] * np.maximum(one - a[l], zero)).astype(np.float32))
        gg = g[:, :, s].numpy().astype(np.float32)
        hh = h[:, :, s].numpy().astype(np.float32) if h is not None else np.zeros_like(gg)
        if normalize:
            seen = A > 0
            As = np.where(seen, A, one)
            gV = np.where(seen, (gg / As).astype(np.float32), zero)
            gA = np.where(seen, _fma32(-gV, (V / As).astype(np.float32), hh), hh)
        else:
            gV, gA = gg, hh
        R = np.zeros_like(gg)
        Rn = [None] * L
        for l in range(L - 1, -1, -1):
            Rn[l] = R
            R = _fma32(np.maximum(one - a[l], zero), R, _fma32(gV, q[l], (gA * a[l]).astype(np.float32)))
        for l in range(L):
            tg = (gA * T[l]).astype(np.float32)
            al[:, :, s, l] = (gV * T[l]).astype(np.float32)
            be[:, :, s, l] = np.where(one - a[l] > 0, _fma32(-T[l], Rn[l], tg), tg)
    assert al.dtype == np.float32 and be.dtype == np.float32
    return al, be


def tree32_dimg(c, maps, layer, al):
    """float32 [B,C,H,W]: d_img from float32 alpha planes [B,C,S,L,H,W], summed as occl_grad_dimg_kernel<KS> sums it.  Per slice and
    layer: the patches in the order (pi, pj); per patch the tap columns e, each a zero-started fma chain over the tap rows a of alpha
    masked to the patch, `acc += part`; then the patch's mirror terms as ONE zero-started fma chain over the positions (vu, vv) and
    their sources in row-major order, `acc += part`.  A texel keeps the accumulator of its own layer; the slices are added in ascending
    order.  The kernel visits only the patches that meet the wave's window and runs the mirror code on border threads only; what it
    skips are chains whose every term is an exact zero, which leave the accumulator unchanged, so all patches are visited here."""
    ks, p, gr, H, W, S, L = c.ks, c.ks // 2, c.grid, c.H, c.W, c.S, c.L
    w = maps.numpy().astype(np.float32).reshape(S, L, c.C, gr, ks, gr, ks)
    hb, wb = bounds_of(H, gr), bounds_of(W, gr)
    ys, xs = np.arange(H), np.arange(W)
    posy = [(ys, np.ones(H, bool)), (-ys, (ys >= 1) & (ys <= p)), (2 * (H - 1) - ys, (ys <= H - 2) & (ys >= H - 1 - p))]
    posx = [(xs, np.ones(W, bool)), (-xs, (xs >= 1) & (xs <= p)), (2 * (W - 1) - xs, (xs <= W - 2) & (xs >= W - 1 - p))]
    layn = layer.numpy().astype(np.int64)[:, None]
    total = np.zeros((c.B, c.C, H, W), dtype=np.float32)
    for s in range(S):
        keep = np.zeros_like(total)
        for l in range(L):
            if not (layn == l).any():
                continue                                                  # no texel keeps this layer's accumulator
            acc = np.zeros_like(total)
            for pi in range(gr):
                for pj in range(gr):
                    ap = np.zeros((c.B, c.C, H + 4 * p, W + 4 * p), dtype=np.float32)     # alpha masked to the patch, zero-padded by 2 p
                    ap[:, :, 2 * p + hb[pi]:2 * p + hb[pi + 1], 2 * p + wb[pj]:2 * p + wb[pj + 1]] = al[:, :, s, l, hb[pi]:hb[pi + 1], wb[pj]:wb[pj + 1]]
                    wt = w[s, l, :, pi, :, pj, :]                                         # [C,ks,ks]
                    for e in range(ks):
                        part = np.zeros_like(total)
                        for a in range(ks):
                            part = _fma32(ap[:, :, p + a:p + a + H, p + e:p + e + W], wt[None, :, a, e, None, None], part)
                        acc = acc + part
                    part = np.zeros_like(total)
                    for vu in range(3):
                        Uv, oky = posy[vu]
                        for vv in range(3):
                            Vv, okx = posx[vv]
                            if (vu, vv) == (0, 0) or not oky.any() or not okx.any():
                                continue
                            yy, xx = ys[oky], xs[okx]
                            blk = np.ix_(range(c.B), range(c.C), yy, xx)
                            sub = part[blk]
                            for a in range(ks):
                                for e in range(ks):
                                    src = ap[:, :, (Uv[yy] + p + a)[:, None], (Vv[xx] + p + e)[None, :]]
                                    sub = _fma32(src, wt[None, :, a, e, None, None], sub)
                            part[blk] = sub
                    acc = acc + part
            keep = np.where(layn == l, acc, keep)
        total = total + keep
    assert total.dtype == np.float32
    return torch.from_numpy(total)


def tree32_dmaps(c, img, layer, al, be):
    """float32 [S L,C,g ks,g ks]: d_maps from float32 planes, summed as occl_grad_dmaps_partial_kernel and occl_grad_dmaps_sum_kernel sum
    it.  Per 32 x 32 tile of a patch and (b, c, s, l, tap): lane = 8 lyr + lxg owns rows lyr + 8 j and columns 4 lxg + k, a zero-started
    chain in (j, k) order of fma(alpha, m ? x : 0) then fma(beta, m ? 1 : 0); the wave butterfly v += v[lane ^ off], off = 32 .. 1; the
    second pass adds the tile columns, the tile rows and the batch, each level started at 0.  (A layer absent from the tile's window
    gets a zero partial from the kernel; the chains give the same zero.)"""
    ks, p, gr, H, W, S, L = c.ks, c.ks // 2, c.grid, c.H, c.W, c.S, c.L
    hb, wb = bounds_of(H, gr), bounds_of(W, gr)
    x = np.pad(img.numpy().astype(np.float32), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect")
    lay = np.pad(layer.numpy().astype(np.int64), ((0, 0), (p, p), (p, p)), mode="reflect")
    x = np.pad(x, ((0, 0), (0, 0), (0, GT), (0, GT)))                       # beyond the image: finite values that meet zero planes only
    lay = np.pad(lay, ((0, 0), (0, GT), (0, GT)), constant_values=HOLE)
    lanes = np.arange(64)
    out = np.zeros((S, L, c.C, gr * ks, gr * ks), dtype=np.float32)
    zero = np.zeros((c.C, S, L, ks, ks), dtype=np.float32)
    for i in range(gr):
        for j in range(gr):
            total = zero
            for b in range(c.B):
                sb = zero
                for y0 in range(hb[i], hb[i + 1], GT):
                    sr = zero
                    for x0 in range(wb[j], wb[j + 1], GT):
                        y1, x1 = min(y0 + GT, hb[i + 1]), min(x0 + GT, wb[j + 1])
                        on = lay[b, y0:y0 + GT + 2 * p, x0:x0 + GT + 2 * p][None] == np.arange(L)[:, None, None]      # [L,TP,TP]
                        xm = np.where(on[None], x[b, :, None, y0:y0 + GT + 2 * p, x0:x0 + GT + 2 * p], np.float32(0)).astype(np.float32)
                        mk = np.broadcast_to(on[None].astype(np.float32), xm.shape)
                        # v[c,l,a,e,row,col] = window[row + 2p - a, col + 2p - e]
                        vx = np.lib.stride_tricks.sliding_window_view(xm, (GT, GT), axis=(2, 3))[:, :, ::-1, ::-1].reshape(c.C, 1, L, ks, ks, 4, 8, 8, 4)
                        vm = np.lib.stride_tricks.sliding_window_view(mk, (GT, GT), axis=(2, 3))[:, :, ::-1, ::-1].reshape(c.C, 1, L, ks, ks, 4, 8, 8, 4)
                        ta = np.zeros((c.C, S, L, GT, GT), dtype=np.float32)
                        tb = np.zeros_like(ta)
                        ta[..., :y1 - y0, :x1 - x0] = al[b, :, :, :, y0:y1, x0:x1]
                        tb[..., :y1 - y0, :x1 - x0] = be[b, :, :, :, y0:y1, x0:x1]
                        ta, tb = ta.reshape(c.C, S, L, 1, 1, 4, 8, 8, 4), tb.reshape(c.C, S, L, 1, 1, 4, 8, 8, 4)
                        acc = np.zeros((c.C, S, L, ks, ks, 8, 8), dtype=np.float32)
                        for jj in range(4):
                            for k in range(4):
                                acc = _fma32(ta[..., jj, :, :, k], vx[..., jj, :, :, k], acc)
                                acc = _fma32(tb[..., jj, :, :, k], vm[..., jj, :, :, k], acc)
                        acc = acc.reshape(c.C, S, L, ks, ks, 64)
                        for off in (32, 16, 8, 4, 2, 1):
                            acc = acc + acc[..., lanes ^ off]
                        assert acc.dtype == np.float32
                        sr = sr + acc[..., 0]
                    sb = sb + sr
                total = total + sb
            out[:, :, :, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks] = total.transpose(1, 2, 0, 3, 4)
    return torch.from_numpy(out.reshape(S * L, c.C, gr * ks, gr * ks))
