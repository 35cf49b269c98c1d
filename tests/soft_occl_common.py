"""Shared by tests/test_soft_occl_host.py and tests/test_gpu_soft_occl.py (not a test module): the case table, the coordinate scenes, the
float64 comparator, a literal restatement, a float32 restatement of the kernel's order and the elementwise budget of the soft-depth-layer
occluded PSF-map render (aadff_render_psf_map_stack_soft_occluded, csrc/conv_occl_soft.hip; aadff/occlusion.py).

Specification (include/aadff.h).  Per texel: !(pos >= 0) is a hole; else p = min(pos, L-1), k = min((int)p, L-1), f = p - k (exact in
float32), m0 = fl(1 - f), m1 = f, x0 = fl(m0 x), x1 = fl(m1 x).  Per output pixel of patch (i,j), slice s and slab k, with w_k the flipped
tile (i,j) of map s L + k and img, pos reflect-padded alike, four fma chains from 0 in row-major tap order, every term a select:
    q0 = sum_t w_k (slab==k ? x0 : 0),  a0 = sum_t w_k (slab==k ? m0 : 0),  q1 = sum_t w_{k+1} (slab==k ? x1 : 0),  a1 alike with m1,
    q_k = fl(q0 + q1),  a_k = fl(a0 + a1);  then the composite of tests/occlusion_common.py over k = 0 .. L-1, out = V / A where A > 0.

Comparator (`soft64`): k and f are taken from the FLOAT32 pos by the rule above (`decode`), so no decision differs between precisions;
then 1 - f, the products and the sums in float64: q_k, a_k from oracle.conv.render_psf_map on the weighted masked .double() inputs
(torch.where BEFORE the convolution), the composite in float64.

Cases: the twelve shapes of occlusion_common.TABLE with coordinate scenes in place of the layer scenes, plus one case of edge values.
Inputs as occlusion_common's (images in [-3, 34.5), strictly positive tile-normalised PSFs, one slice x 1e-3): `occlusion_common.inputs`
gives img and maps, `coordinate` the pos.

Budget - derived from the operation order of csrc/conv_occl_soft.hip (both kernels), no constant from a kernel's output.  U = 2^-24,
n = ks^2, g = (n + 1) U >= gamma_n (occlusion_common (1)).  Per output element and slab k, with Q0 = sum w_k (1-f)|x|, Q1 = sum w_{k+1} f|x|
and a0, a1 the exact coverage sums (all over the slab's texels in the window):

  (0) the inputs: m0^ = fl(1 - f) = (1 - f)(1 + d1), x0^ = fl(m0^ x) = (1 - f) x (1 + d1)(1 + d2), x1^ = fl(f x) = f x (1 + d3), m1 = f
      exact, |d| <= U: relative input errors  dx0 = 2 U + U^2,  dm0 = U,  dx1 = U,  dm1 = 0.
  (1) a chain over inputs of relative error d: |sum^ - sum| <= (d + g (1 + d)) * (the sum of magnitudes), so
          e_q0 = (dx0 + g (1 + dx0)) Q0,  e_a0 = (dm0 + g (1 + dm0)) a0,  e_q1 = (dx1 + g (1 + dx1)) Q1,  e_a1 = g a1.
  (2) the adds: q^ = fl(q0^ + q1^), one rounding relative to the computed sum, |q0^ + q1^| <= Q0 + Q1 + e_q0 + e_q1:
          e_q = (e_q0 + e_q1)(1 + U) + U (Q0 + Q1),      e_a = (e_a0 + e_a1)(1 + U) + U (a0 + a1).
      A slab with no texel in the window has q^ = a^ = 0 exactly; where no texel of the slab has f != 0 the kernel skips the second pass,
      which leaves q0^ + (+0) = q0^: inside the same bound.
  (3) occlusion_common's (2) - (4) with e_q, e_a for e_q,l, e_a,l and Q = Q0 + Q1, a = a0 + a1 for Q_l, a_l: the transmittance error
      E_{k+1} <= E_k + e_a + 2 U  (a_k <= 1 up to the rounding of a tile sum: it is a convex mix of two tile sums over a subset of the
      window), the composites and the quotient unchanged.

A > 0 is an exact decision: positive PSFs and m0^ >= 2^-24 (f <= 1 - 2^-24) make every slab with a texel in the window contribute
a0^ > 0, and T_k > 0 at the first such slab; A is exactly 0, in float32 and float64 alike, iff the window holds only holes.
`share` (occlusion_common) takes EVERY element.
"""
import numpy as np
import torch

import occlusion_common as oc
from oracle import conv as oconv

U = oc.U
SENTINEL = oc.SENTINEL


def dispatch(ks):
    return f"conv_occl_soft_kernel<{ks}>" if ks in oc.TEMPLATED_KS else "conv_occl_soft_generic_kernel"


def expected_instantiations():
    return {f"conv_occl_soft_kernel<{k}>" for k in oc.TEMPLATED_KS} | {"conv_occl_soft_generic_kernel"}


_SCENE = {"random+hole2": "random+hole2", "random": "random", "disc": "disc", "even32": "even32", "hole6": "above+hole6",
          "bands+block": "bands+frac", "blocks": "blocks+frac"}
HARD = list(oc.TABLE)                                     # the twelve hard cases (the integer-coordinate consequence runs on these)
TABLE = [c._replace(scene=_SCENE[c.scene], kernel=dispatch(c.ks)) for c in oc.TABLE]
EDGES = oc.Case("1x2x2x3-40x45-g2-ks5-edges", 1, 2, 2, 3, 40, 45, 2, 5, "edges", dispatch(5),
                "pos exactly L-1, above it, f = j 2^-24, f = 1 - 2^-24, -0.0, -1 and NaN holes")
TABLE.append(EDGES)
DISC, HOLE6, BATCH, GENERIC = TABLE[2], TABLE[3], TABLE[5], TABLE[6]


def edge_values(L):
    """float32 coordinates at the edges of the decode, for L >= 3."""
    t = 2.0 ** -24
    return torch.tensor([L - 1, L - 1 + 0.5, 1e30, float("inf"), t, 2 * t, 3 * t, 5 * t, 1 - t, 1.0, 1 + 2 * t, 2 - 2 * t, 0.0, -0.0, -1.0,
                         float("nan"), 0.5, L - 2 + 0.25], dtype=torch.float32)


def coordinate(c):
    """float32 pos [B,H,W] of a case's scene, CPU, seeded."""
    gen = torch.Generator().manual_seed(977 * c.ks + 13 * c.H + 5 * c.W + c.L)
    B, H, W, L = c.B, c.H, c.W, c.L
    frac = torch.rand((B, H, W), generator=gen)
    if c.scene.startswith("random"):
        pos = frac * (L - 1)
        if c.scene.endswith("hole2"):
            pos[:, H // 2:H // 2 + 2, W // 3:W // 3 + 2] = float("nan")
    elif c.scene == "even32":                                # only the even slabs are occupied: the presence skip runs
        pos = 2.0 * torch.randint(0, L // 2, (B, H, W), generator=gen) + frac
    elif c.scene == "above+hole6":                           # L = 1: every pos >= 0 is slab 0, f = 0
        pos = frac * 3.0
        pos[:, 11:17, 20:26] = -1.0
    elif c.scene in ("bands+frac", "blocks+frac"):           # the hard scene's index plus a fraction per texel (clamped at L - 1)
        pos = oc.layer_map(c.scene.split("+")[0] + ("+block" if c.scene.startswith("bands") else ""), B, H, W, L, gen).float() + frac
    elif c.scene == "disc":                                  # the disc over a slant crossing every slab
        from aadff.occlusion import depth_nodes
        from aadff.synth import synth_disc_depth_mm
        pos = depth_nodes(torch.from_numpy(synth_disc_depth_mm(H, W)[0])[None], L)[0].expand(B, H, W)
    elif c.scene == "edges":
        vals = edge_values(L)
        pos = vals[torch.randint(0, len(vals), (B, H, W), generator=gen)]
    else:
        raise ValueError(c.scene)
    return pos.to(torch.float32).contiguous()


def inputs(c):
    """(img [B,C,H,W], maps [S L,C,g ks,g ks], pos [B,H,W]) float32, CPU; img and maps are occlusion_common's for the same shape."""
    img, maps, _ = oc.inputs(c._replace(scene="random"))
    return img, maps, coordinate(c)


def decode(pos, L):
    """(k int64 [B,H,W], -1 on holes; f float32) from float32 pos by the contract's rule."""
    assert pos.dtype == torch.float32
    hole = ~(pos >= 0)
    p = torch.where(hole, torch.zeros_like(pos), torch.clamp(pos, max=float(L - 1)))
    k = torch.clamp(p.to(torch.int64), max=L - 1)            # the cast truncates
    f = p - k.to(torch.float32)
    assert bool(((f >= 0) & (f < 1)).all()) and bool((f.double() == p.double() - k.double()).all())
    return torch.where(hole, torch.full_like(k, -1), k), torch.where(hole, torch.zeros_like(f), f)


# --------------------------------------------------------------------------------------------------------------------- comparator
def soft64(img, maps, pos, L, grid, want_bound=True):
    """oc.Ref(V, A, out, eV, eA, eOut), float64 [B,C,S,H,W]: the specification in float64 on the float32 decode, with the budgets of the
    module docstring for V (normalize = 0), A (coverage) and out."""
    B, C, H, W = img.shape
    S, ks = maps.shape[0] // L, maps.shape[-1] // grid
    g = (ks * ks + 1) * U
    k32, f32 = decode(pos, L)
    x64 = img.double()
    slab, f = k32[:, None].expand(B, C, H, W), f32.double()[:, None].expand(B, C, H, W)
    dx0, dm0, dx1 = 2 * U + U * U, U, U
    R = oconv.render_psf_map
    zero = torch.zeros((B, C, S, H, W), dtype=torch.float64)
    V, A, eV, eA = zero.clone(), zero.clone(), zero.clone(), zero.clone()
    for s in range(S):
        T, E = torch.ones((B, C, H, W), dtype=torch.float64), torch.zeros((B, C, H, W), dtype=torch.float64)
        v, a_, ev, ea = (torch.zeros((B, C, H, W), dtype=torch.float64) for _ in range(4))
        pv, pa = torch.zeros_like(v), torch.zeros_like(v)
        for k in range(L):
            on = slab == k
            w0 = maps[s * L + k].double()
            m0, m1 = torch.where(on, 1.0 - f, 0.0), torch.where(on, f, 0.0)
            q, a = R(torch.where(on, (1.0 - f) * x64, 0.0), w0, grid), R(m0, w0, grid)
            Q0 = R(torch.where(on, (1.0 - f) * x64.abs(), 0.0), w0, grid) if want_bound else None
            Q1 = a1 = torch.zeros_like(q)
            if k + 1 < L:
                w1 = maps[s * L + k + 1].double()
                a1 = R(m1, w1, grid)
                q = q + R(torch.where(on, f * x64, 0.0), w1, grid)
                if want_bound:
                    Q1 = R(torch.where(on, f * x64.abs(), 0.0), w1, grid)
            else:
                assert not bool(m1.any())
            a0, a = a, a + a1
            if want_bound:
                Q = Q0 + Q1
                eq = ((dx0 + g * (1 + dx0)) * Q0 + (dx1 + g * (1 + dx1)) * Q1) * (1 + U) + U * Q
                eal = ((dm0 + g * (1 + dm0)) * a0 + g * a1) * (1 + U) + U * a
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
    return oc.Ref(V, A, out, eV, eA, d + U * (out.abs() + d))


def loop64(img, maps, pos, L, grid):
    """The specification restated literally, pixel by pixel in Python floats: (V, A, out) float64 [B,C,S,H,W].  Tiny inputs only."""
    B, C, H, W = img.shape
    S, ks = maps.shape[0] // L, maps.shape[-1] // grid
    p = ks // 2
    hb, wb = [int(i / grid * H) for i in range(grid + 1)], [int(j / grid * W) for j in range(grid + 1)]
    x64, w64, ps = img.double().tolist(), maps.double().tolist(), pos.double().tolist()
    Vo, Ao, Oo = (torch.zeros((B, C, S, H, W), dtype=torch.float64) for _ in range(3))
    for b in range(B):
        for c in range(C):
            for s in range(S):
                for y in range(H):
                    i = max(k for k in range(grid) if hb[k] <= y)
                    for x in range(W):
                        j = max(k for k in range(grid) if wb[k] <= x)
                        T, V, A = 1.0, 0.0, 0.0
                        for k in range(L):
                            a = q = 0.0
                            for u in range(ks):
                                for v in range(ks):
                                    ty, tx = oc._reflect(y - p + u, H), oc._reflect(x - p + v, W)
                                    pt = ps[b][ty][tx]
                                    if not pt >= 0:
                                        continue
                                    pt = min(pt, float(L - 1))
                                    kt = min(int(pt), L - 1)
                                    if kt != k:
                                        continue
                                    f = pt - kt
                                    w0 = w64[s * L + k][c][i * ks + ks - 1 - u][j * ks + ks - 1 - v]
                                    w1 = w64[s * L + k + 1][c][i * ks + ks - 1 - u][j * ks + ks - 1 - v] if k + 1 < L else 0.0
                                    mix = (1.0 - f) * w0 + f * w1
                                    a += mix
                                    q += mix * x64[b][c][ty][tx]
                            V, A, T = V + T * q, A + T * a, T * max(1.0 - a, 0.0)
                        Vo[b, c, s, y, x], Ao[b, c, s, y, x], Oo[b, c, s, y, x] = V, A, (V / A if A > 0 else 0.0)
    return Vo, Ao, Oo


# ------------------------------------------------------------------------------------- the kernel's order in float32, on the CPU
def _fma32(a, b, c):
    """fl32(a b + c): the product of two float32 is exact in float64; the sum is rounded to float64, then to float32 (a double rounding
    that differs from a true fma only on ties of the float64 sum: inside the budget, which is what this restatement is held to)."""
    return (a.astype(np.float64) * b.astype(np.float64) + c.astype(np.float64)).astype(np.float32)


PLANTS = ("swap", "node", "round", "product", "noclamp", "noflip", "slice", "batch")


def restate32(img, maps, pos, L, grid, plant=None):
    """(V, A, out) float32 [B,C,S,H,W]: the operation order of csrc/conv_occl_soft.hip restated in numpy float32 (the decode, fl(1 - f),
    the two products, four chains per slab in row-major tap order, the adds, the composite, the division).  `plant`: one deliberate
    error of PLANTS, which the budget must catch."""
    assert plant is None or plant in PLANTS
    f32 = np.float32
    x, w, ps = img.numpy().astype(f32), maps.numpy().astype(f32), pos.numpy().astype(f32)
    B, C, H, W = x.shape
    S, ks = w.shape[0] // L, w.shape[-1] // grid
    pd = ks // 2
    if plant == "batch":
        ps = np.roll(ps, 1, axis=0)
    with np.errstate(invalid="ignore", over="ignore"):
        hole = ~(ps >= 0)
        p = np.where(hole, f32(0), ps if plant == "noclamp" else np.minimum(ps, f32(L - 1)))
        ki = np.minimum(np.rint(p) if plant == "round" else np.trunc(np.minimum(p, f32(1e9))), L - 1).astype(np.int64)
        f = (p - ki.astype(f32)).astype(f32)
        m0, m1 = (f32(1) - f).astype(f32), f
        if plant == "swap":
            m0, m1 = m1, m0
        ki = np.where(hole, -1, ki)
        pad2 = ((0, 0), (pd, pd), (pd, pd))
        kp, m0p, m1p = np.pad(ki, pad2, mode="reflect"), np.pad(m0, pad2, mode="reflect"), np.pad(m1, pad2, mode="reflect")
        xp = np.pad(x, ((0, 0),) + pad2, mode="reflect")
        hb, wb = [int(i / grid * H) for i in range(grid + 1)], [int(j / grid * W) for j in range(grid + 1)]
        V, A = np.zeros((B, C, S, H, W), f32), np.zeros((B, C, S, H, W), f32)
        for s in range(S):
            sm = (s + 1) % S if plant == "slice" else s
            for i in range(grid):
                for j in range(grid):
                    ys, xs = slice(hb[i], hb[i + 1] + 2 * pd), slice(wb[j], wb[j + 1] + 2 * pd)
                    h, wd = hb[i + 1] - hb[i], wb[j + 1] - wb[j]
                    Vt, At, Tt = np.zeros((B, C, h, wd), f32), np.zeros((B, C, h, wd), f32), np.ones((B, C, h, wd), f32)
                    for k in range(L):
                        on = (kp[:, ys, xs] == k)[:, None]
                        if not on.any():
                            continue
                        ins = []
                        for m in (m0p[:, None, ys, xs], m1p[:, None, ys, xs]):
                            mx = (m * xp[:, :, ys, xs]).astype(f32)
                            if plant == "product":
                                ins.append(((mx * on).astype(f32), np.broadcast_to((m * on).astype(f32), mx.shape)))
                            else:
                                ins.append((np.where(on, mx, f32(0)), np.broadcast_to(np.where(on, m, f32(0)), mx.shape)))
                        acc = [[np.zeros((B, C, h, wd), f32) for _ in range(2)] for _ in range(2)]
                        for pss in range(2):
                            node = k + pss
                            if node >= L:
                                continue                     # slab L - 1: both chains of the second pass are exactly 0
                            if plant == "node":
                                node = k
                            tile = w[sm * L + node][:, i * ks:(i + 1) * ks, j * ks:(j + 1) * ks]
                            for u in range(ks):
                                for v in range(ks):
                                    wt = (tile[:, u, v] if plant == "noflip" else tile[:, ks - 1 - u, ks - 1 - v])[None, :, None, None]
                                    for ch in range(2):
                                        acc[pss][ch] = _fma32(wt, ins[pss][ch][:, :, u:u + h, v:v + wd], acc[pss][ch])
                        q, a = (acc[0][0] + acc[1][0]).astype(f32), (acc[0][1] + acc[1][1]).astype(f32)
                        Vt, At = _fma32(Tt, q, Vt), _fma32(Tt, a, At)
                        Tt = (Tt * np.maximum((f32(1) - a).astype(f32), f32(0))).astype(f32)
                    V[:, :, s, hb[i]:hb[i + 1], wb[j]:wb[j + 1]], A[:, :, s, hb[i]:hb[i + 1], wb[j]:wb[j + 1]] = Vt, At
        out = np.where(A > 0, (V / np.where(A > 0, A, f32(1))).astype(f32), f32(0))
    return torch.from_numpy(V), torch.from_numpy(A), torch.from_numpy(out)


# ------------------------------------------------------------------------------------------------------------------ references
_REF = {}


def reference(c):
    """(img, maps, pos, Ref) of a case, computed once per process and shared: do not modify."""
    if c.id not in _REF:
        img, maps, pos = inputs(c)
        _REF[c.id] = (img, maps, pos, soft64(img, maps, pos, c.L, c.grid))
    return _REF[c.id]


share = oc.share
