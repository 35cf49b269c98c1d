"""Shared by tests/test_occlusion_host.py and tests/test_gpu_occlusion.py (not a test module): the case table, the seeded inputs, the
float64 comparator, a literal restatement and the elementwise budget of the occlusion-aware layered PSF-map render
(aadff_render_psf_map_stack_occluded, csrc/conv_occl.hip; aadff/occlusion.py).

Specification (include/aadff.h), per output pixel of patch (i,j): with w_l the flipped tile (i,j) of map s L + l, channel c, and the
image and the layer map reflect-padded by ks/2 alike, m_l(t) = (layer[b,t] == l),
    a_l = sum_t w_l(t) (m_l(t) ? 1 : 0),   q_l = sum_t w_l(t) (m_l(t) ? img[b,c,t] : 0)          (a select, not a product)
    T = 1, V = 0, A = 0;  for l = 0 .. L-1:  V = fma(T, q_l, V), A = fma(T, a_l, A), T = T max(1 - a_l, 0)
    out = V / A where A > 0, else 0  (normalize = 0: out = V);  coverage = A.

Comparator (`occl64`): q_l, a_l from oracle.conv.render_psf_map on the masked .double() inputs (the select is a torch.where BEFORE the
convolution), the composite in float64.

Inputs (seeded, CPU), as tests/blend_common.py: images in [-3, 34.5); PSFs strictly positive and normalised per tile; with S >= 2 one
slice scaled by 1e-3.  Positive PSFs are a condition of the budget: they keep 1 - a_l in [0, 1] (up to the rounding of the tile sum)
and make A > 0 an exact decision - A is exactly 0, in float32 and float64 alike, if and only if no window texel lies on any layer (every
term of every chain is then a product with an exact 0; otherwise some T_l a_l > 0 with T_l >= the product of positive factors).  So no
element is excluded anywhere.

Budget - derived from the operation order of csrc/conv_occl.hip (both kernels: conv_occl_kernel<KS>, conv_occl_generic_kernel), no
constant from a kernel's output.  U = 2^-24, n = ks^2.  Per output element and layer l let Q_l = sum_t w_l |x| m_l (so |q_l| <= Q_l).

  (1) the two chains: one fma per tap from 0 in a fixed tap order, every product exact inside the fma:
          |q^_l - q_l| <= e_q,l = (n + 1) U Q_l,      |a^_l - a_l| <= e_a,l = (n + 1) U a_l
      (gamma_n = n U / (1 - n U) <= n U + 0.41 U at n = 51^2: the "+ 1").  A layer with no texel in the window has q^ = a^ = 0 exactly.
  (2) the transmittance: f^_l = max(fl(1 - a^_l), 0) with |fl(1 - a^_l) - (1 - a_l)| <= e_a,l + U (a^_l >= 0, so |1 - a^_l| <= 1 up to
      the rounding of a tile sum; the clamp is 1-Lipschitz), and 0 <= f^_l <= 1, 0 <= T^_l <= 1 hold exactly.  T^_{l+1} = fl(T^_l f^_l):
          E_{l+1} = |T^_{l+1} - T_{l+1}| <= E_l f^_l + T_l (e_a,l + U) + U T^_l f^_l <= E_l + e_a,l + 2 U,     E_0 = 0
      i.e. T_l is off by at most sum_{k<l} ((n + 1) a_k + 2) U.
  (3) the composites V^ <- fl(T^_l q^_l + V^) (one rounding each; A alike with a for q and Q):
          |T^_l q^_l - T_l q_l| <= (T_l + E_l) e_q,l + E_l |q_l|
          r_l = e_V,l + (T_l + E_l) e_q,l + E_l |q_l|,    e_V,l+1 = r_l + U (1 + 2 U) (P_{l+1} + r_l),   P_{l+1} = sum_{k<=l} T_k Q_k >= |V_{l+1}|
      (the rounding is relative to the computed partial sum, which is within r_l of an exact value of magnitude <= P_{l+1}).
  (4) the quotient, one IEEE division: with d = (e_V + |out| e_A) / (A - e_A)  (A^ >= A - e_A > 0 where A > 0),
          |out^ - out| <= d + U (|out| + d)
      and out^ = out = 0 exactly where A = 0.

`compare` returns the largest share of the budget used over EVERY element (0 / 0 counts as 0, anything over a zero budget as infinite).
"""
import collections

import numpy as np
import torch

from oracle import conv as oconv

U = 2.0 ** -24
SENTINEL = -12345.0
TEMPLATED_KS = (3, 5, 7, 9, 11, 13, 15, 21)
HOLE = 255

Case = collections.namedtuple("Case", "id B C S L H W grid ks scene kernel reaches")


def dispatch(ks):
    """The instantiation aadff_render_psf_map_stack_occluded launches (csrc/conv_occl.hip), as the library's symbol table spells it."""
    return f"conv_occl_kernel<{ks}>" if ks in TEMPLATED_KS else "conv_occl_generic_kernel"


def expected_instantiations():
    return {f"conv_occl_kernel<{k}>" for k in TEMPLATED_KS} | {"conv_occl_generic_kernel"}


def _case(B, C, S, L, H, W, grid, ks, scene, reaches):
    return Case(f"{B}x{C}x{S}x{L}-{H}x{W}-g{grid}-ks{ks}", B, C, S, L, H, W, grid, ks, scene, dispatch(ks), reaches)


TABLE = [
    _case(2, 3, 1, 3, 37, 45, 3, 5, "random+hole2", "random layer per texel plus a 2 x 2 hole; ragged tiles"),
    _case(1, 1, 2, 2, 100, 72, 2, 7, "bands+block", "a patch spanning several tiles; bands plus a block"),
    _case(1, 3, 3, 4, 96, 130, 5, 11, "disc", "the disc over a slanted background via depth_layers; one slice scaled 1e-3"),
    _case(1, 1, 1, 1, 40, 33, 1, 3, "hole6", "L = 1 with a 6 x 6 hole: zeros where A = 0"),
    _case(1, 1, 1, 32, 24, 40, 4, 3, "even32", "the layer limit; half the indices never occur, so the presence skip runs"),
    _case(5, 1, 1, 2, 32, 32, 4, 3, "random", "batch decode"),
    _case(1, 1, 2, 3, 48, 64, 3, 17, "blocks", "the run-time-ks kernel"),
    _case(1, 1, 1, 2, 64, 64, 2, 51, "blocks", "the run-time-ks kernel at the ks limit"),
    _case(1, 1, 2, 2, 48, 64, 3, 9, "blocks", "the remaining templated sizes"),
    _case(1, 1, 2, 2, 48, 64, 3, 13, "blocks", "the remaining templated sizes"),
    _case(1, 1, 2, 2, 48, 64, 3, 15, "blocks", "the remaining templated sizes"),
    _case(1, 1, 2, 2, 48, 64, 3, 21, "blocks", "the remaining templated sizes"),
]
DISC, HOLE6, BATCH = TABLE[2], TABLE[3], TABLE[5]


# ------------------------------------------------------------------------------------------------------------------------- inputs
def positive_maps(n, C, grid, ks, gen, scaled=None):
    """float32 [n,C,g ks,g ks]: strictly positive PSFs, normalised per tile; map `scaled` (if any) times 1e-3."""
    w = torch.rand((n, C, grid, ks, grid, ks), generator=gen) + 0.05
    w = w / w.sum((3, 5), keepdim=True)
    if scaled is not None:
        w[scaled] *= 1e-3
    return w.reshape(n, C, grid * ks, grid * ks).contiguous()


def layer_map(scene, B, H, W, L, gen):
    """uint8 [B,H,W] of a scene of the table."""
    if scene.startswith("random"):
        lay = torch.randint(0, L, (B, H, W), generator=gen, dtype=torch.int64)
        if scene.endswith("hole2"):
            lay[:, H // 2:H // 2 + 2, W // 3:W // 3 + 2] = HOLE
    elif scene == "even32":
        lay = 2 * torch.randint(0, L // 2, (B, H, W), generator=gen, dtype=torch.int64)
    elif scene == "bands+block":
        lay = ((torch.arange(H)[:, None] // 13 + torch.arange(W)[None, :] // 29) % L).expand(B, H, W).clone()
        lay[:, H // 3:H // 3 + 21, W // 4:W // 4 + 17] = 0
    elif scene == "blocks":
        coarse = torch.randint(0, L, (B, (H + 4) // 5, (W + 6) // 7), generator=gen, dtype=torch.int64)
        lay = coarse.repeat_interleave(5, 1).repeat_interleave(7, 2)[:, :H, :W]
    elif scene == "hole6":
        lay = torch.zeros((B, H, W), dtype=torch.int64)
        lay[:, 11:17, 20:26] = HOLE
    elif scene == "disc":
        from aadff.focal_stack import depth_layers
        from aadff.synth import synth_disc_depth_mm
        depth, _ = synth_disc_depth_mm(H, W)
        lay = depth_layers(torch.from_numpy(depth)[None], L)[0].expand(B, H, W)
    else:
        raise ValueError(scene)
    return lay.to(torch.uint8).contiguous()


def inputs(c):
    """(img [B,C,H,W] float32, maps [S L,C,g ks,g ks] float32, layer [B,H,W] uint8), CPU."""
    gen = torch.Generator().manual_seed(4001 * c.ks + 31 * c.H + 7 * c.W + 3 * c.S + c.grid + 101 * c.L)
    img = torch.rand((c.B, c.C, c.H, c.W), generator=gen) * 37.5 - 3.0
    w = positive_maps(c.S * c.L, c.C, c.grid, c.ks, gen).reshape(c.S, c.L, c.C, c.grid * c.ks, c.grid * c.ks)
    if c.S >= 2:
        w[c.S // 2] *= 1e-3
    return img.contiguous(), w.reshape(c.S * c.L, c.C, c.grid * c.ks, c.grid * c.ks).contiguous(), layer_map(c.scene, c.B, c.H, c.W, c.L, gen)


# --------------------------------------------------------------------------------------------------------------------- comparator
Ref = collections.namedtuple("Ref", "V A out eV eA eOut")


def occl64(img, maps, layer, L, grid, want_bound=True):
    """Ref(V, A, out, eV, eA, eOut), float64 [B,C,S,H,W]: the specification with q_l, a_l = oracle.conv.render_psf_map of the masked
    float64 inputs, the composite in float64, and the budgets of the module docstring for V (normalize = 0), A (coverage) and out."""
    B, C, H, W = img.shape
    S, ks = maps.shape[0] // L, maps.shape[-1] // grid
    n1 = ks * ks + 1
    x64, lay = img.double(), layer.to(torch.int64)[:, None].expand(B, C, H, W)
    zero = torch.zeros((B, C, S, H, W), dtype=torch.float64)
    V, A, eV, eA = zero.clone(), zero.clone(), zero.clone(), zero.clone()
    for s in range(S):
        T, E = torch.ones((B, C, H, W), dtype=torch.float64), torch.zeros((B, C, H, W), dtype=torch.float64)
        v, a_, ev, ea = (torch.zeros((B, C, H, W), dtype=torch.float64) for _ in range(4))
        pv, pa = torch.zeros_like(v), torch.zeros_like(v)
        for l in range(L):
            on = lay == l
            m64 = maps[s * L + l].double()
            q = oconv.render_psf_map(torch.where(on, x64, 0.0), m64, grid)
            a = oconv.render_psf_map(on.double(), m64, grid)
            if want_bound:
                Q = oconv.render_psf_map(torch.where(on, x64.abs(), 0.0), m64, grid)
                eq, eal = n1 * U * Q, n1 * U * a
                pv, pa = pv + T * Q, pa + T * a
                rv, ra = ev + (T + E) * eq + E * q.abs(), ea + (T + E) * eal + E * a
                ev, ea = rv + U * (1 + 2 * U) * (pv + rv), ra + U * (1 + 2 * U) * (pa + ra)
                E = E + eal + 2 * U
            v, a_ = v + T * q, a_ + T * a
            T = T * torch.clamp(1.0 - a, min=0.0)
        V[:, :, s], A[:, :, s], eV[:, :, s], eA[:, :, s] = v, a_, ev, ea
    seen = A > 0
    out = torch.where(seen, V / torch.where(seen, A, 1.0), 0.0)
    d = torch.where(seen, (eV + out.abs() * eA) / torch.where(seen, A - eA, 1.0), 0.0)
    assert not want_bound or bool((A - eA)[seen].gt(0).all())
    return Ref(V, A, out, eV, eA, d + U * (out.abs() + d))


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def loop64(img, maps, layer, L, grid):
    """The specification restated literally, pixel by pixel in Python floats: (V, A, out) float64 [B,C,S,H,W].  Tiny inputs only."""
    B, C, H, W = img.shape
    S, ks = maps.shape[0] // L, maps.shape[-1] // grid
    p = ks // 2
    hb, wb = [int(i / grid * H) for i in range(grid + 1)], [int(j / grid * W) for j in range(grid + 1)]
    x64, w64, lay = img.double().tolist(), maps.double().tolist(), layer.tolist()
    Vo, Ao, Oo = (torch.zeros((B, C, S, H, W), dtype=torch.float64) for _ in range(3))
    for b in range(B):
        for c in range(C):
            for s in range(S):
                for y in range(H):
                    i = max(k for k in range(grid) if hb[k] <= y)
                    for x in range(W):
                        j = max(k for k in range(grid) if wb[k] <= x)
                        T, V, A = 1.0, 0.0, 0.0
                        for l in range(L):
                            a = q = 0.0
                            for u in range(ks):
                                for v in range(ks):
                                    ty, tx = _reflect(y - p + u, H), _reflect(x - p + v, W)
                                    w = w64[s * L + l][c][i * ks + ks - 1 - u][j * ks + ks - 1 - v]
                                    if lay[b][ty][tx] == l:
                                        a += w
                                        q += w * x64[b][c][ty][tx]
                            V, A, T = V + T * q, A + T * a, T * max(1.0 - a, 0.0)
                        Vo[b, c, s, y, x], Ao[b, c, s, y, x], Oo[b, c, s, y, x] = V, A, (V / A if A > 0 else 0.0)
    return Vo, Ao, Oo


# ------------------------------------------------------------------------------------------------------------------ references
_REF = {}


def reference(c):
    """(img, maps, layer, Ref) of a case, computed once per process and shared: do not modify."""
    if c.id not in _REF:
        img, maps, layer = inputs(c)
        _REF[c.id] = (img, maps, layer, occl64(img, maps, layer, c.L, c.grid))
    return _REF[c.id]


def share(got, want, budget):
    """(largest |got - want| / budget over EVERY element, its flat index): 0 / 0 is 0, an error over a zero budget is infinite."""
    assert tuple(got.shape) == tuple(want.shape) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    err = (got.double() - want).abs()
    use = torch.where(budget > 0, err / torch.where(budget > 0, budget, 1.0), torch.where(err > 0, float("inf"), 0.0))
    worst = int(use.argmax())
    return float(use.flatten()[worst]), worst
