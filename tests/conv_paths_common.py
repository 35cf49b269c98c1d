"""Shared by tests/test_conv_paths_host.py and tests/test_gpu_conv_paths.py (not a test module): the case table, the inputs, the comparators
and the budgets of the forward tests of the patch convolution (aadff_render_psf_map and its stack / strided / layered / uniform-PSF
entries, csrc/conv.hip), one case for every kernel instantiation the dispatch can reach.  The rule that picks the instantiation lives in
csrc/conv_plan.cpp (conv_plan); `dispatch` below restates it independently, and the host module holds the library to the restatement.

Comparator: oracle.conv.render_psf_map on .double() inputs, slice by slice (`loop64` anchors it on tiny cases).

Inputs (seeded, CPU): images in [-3, 34.5) so that the power-of-two tile pre-scale of the matrix-core kernels matters; PSFs positive and
normalised per patch; one slice (one channel of a lone slice) scaled by 1e-3 so that the tap pre-scale matters; signed cases have taps of
both signs with sum|w| = 1 per patch.

Budgets - derived from the code, none from a kernel's output.  U = 2^-24; per output element, with the ks^2 taps w and window values x:

  plain fp32 (conv_psf_map_kernel, conv_psf_map_generic_kernel: fma chains of exactly formed products)
      |got - o64| <= ks^2 U sum|x w| + U |o64|                                                        (any summation order)
      and rel_l2(got, o64) <= 4 x d32seq, d32seq = rel_l2(sequential32, o64): the float32 fma chain in row-major tap order.

  matrix cores (sbatch, blk, blkw, mfma, toeplitz_wide).  Every family carries the same operand split (pow2_scale and the two
  (_Float16) conversions beside it, read in each of the five kernels): an operand group is scaled by s = 2^(9 - floor(log2 max|.|)) of
  the group (exact), so the scaled values lie below 2^10; hi = fp16(v) is off by at most 2^-2 (half an fp16 ulp below 2^10) and
  lo = fp16(v - hi) by at most 2^-14 (half an ulp below 2^-2; a flushed subnormal is below 2^-14 too).  Against the group maximum
  (>= 2^9 after the scale) the split residual is 2^-23.  The image group is one staged tile or band with its halo, the tap group one
  (slice, channel, patch) or tap-row set; from outside the kernel only the maximum over the whole (b, c) plane, Xmax, and over the whole
  (slice, channel) map, Wmax, bound them.  hi*hi, hi*lo and lo*hi are exact in fp32 and summed in fp32 by the MFMA; lo*lo is dropped:
  |lo| <= 2^-11 (1 + 2^-11) |v| for normal fp16 hi, 2^-33 of the group maximum otherwise.  The closing multiplication by 1/(sx sw) is
  exact.
      |got - o64| <=   ks^2 U sum|x w|                                   fp32 roundings of the accumulator
                     + 2^-23 Xmax sum|w|                                 split residual of x
                     + 2^-23 Wmax sum|x|                                 split residual of w
                     + 2^-22 (1 + 2^-9) sum|x w| + 2^-42 (Xmax sum|w| + Wmax sum|x|)        the dropped lo*lo products
                     + U |o64|                                           the last addition where waves split the tap rows
  The first term counts ks^2 roundings as for the plain kernels.  An accumulator passes 3 ks (Toeplitz forms) or 3 k-steps per tap-row
  window (block forms) MFMAs, each of which adds up to 32 products at once; counting one rounding per nonzero product instead would
  give 3 ks^2 - the tighter count is the one held.  Where the sum comes out above the tolerance the existing tests already enforce on
  this data range (tests/test_gpu_parity.py: 4e-6 x 40 absolute), that tolerance is the bound: MC_CAP.  rel_l2 is reported in d32seq
  units, not gated.

No element is excluded from any bound.
"""
import collections

import numpy as np
import torch

from oracle import conv as oconv

U = 2.0 ** -24
MC_CAP = 4e-6 * 40
SENTINEL = -12345.0
SWITCHES = ("AADFF_CONV_PATH", "AADFF_CONV_BLKW", "AADFF_CONV_BLKW_RB", "AADFF_CONV_NW", "AADFF_CONV_PAIR")
PLAIN = ("valu", "generic")
FAMILIES = ("valu", "generic", "mfma", "sbatch", "blk", "blkw", "toeplitz_wide")

Case = collections.namedtuple("Case", "id group entry env B C S H W grid ks signed L")


def rel_l2(a, b):
    a, b = a.double(), b.double()
    return float((a - b).norm() / b.norm())


# ------------------------------------------------------------------------------------------------------------- the dispatch, restated
def _bounds(n, grid):
    return oconv.patch_bounds(n, grid)


def dispatch(c):
    """The instantiation the library launches for a case: name as the library's symbol table spells it, family.  An independent statement
    of the rule of conv_plan (csrc/conv_plan.cpp); tests/test_conv_paths_host.py compares the two through aadff_conv_plan_describe."""
    env, ks, S = c.env, c.ks, c.S
    hb, wb = _bounds(c.H, c.grid), _bounds(c.W, c.grid)
    mh, mw = max(b - a for a, b in zip(hb, hb[1:])), max(b - a for a, b in zip(wb, wb[1:]))
    nc_of = lambda n: 1 if n <= 4 else (2 if n <= 8 else (3 if n <= 12 else 4))
    if c.entry == "layered":
        return f"conv_psf_map_sbatch_kernel<24, {nc_of(S * c.L)}, false, false, true>", "sbatch"
    path = env.get("AADFF_CONV_PATH")
    if 3 <= ks <= 21 and path is None:
        blkw = _atoi(env.get("AADFF_CONV_BLKW"), -1)
        if ks >= 13:
            auto = S == 1 or ks in (13, 17, 21)
        else:
            auto = (ks <= 9 or mh > 96) if S == 1 else ks == 5
        rb = _atoi(env.get("AADFF_CONV_BLKW_RB"), 0)
        if rb not in (24, 32, 48):
            if ks <= 11:
                per = -(-mw // 96) * c.grid * c.grid * c.B * c.C * S
                w24, w32 = per * -(-mh // 24), per * -(-mh // 32)
                rb = 32 if -(-w24 // 1536) > -(-w32 // 1536) else 24
            else:
                rb = 24 if mh <= 24 else (32 if mh <= 32 else (48 if mh <= 48 else (32 if mh <= 64 else (48 if mh <= 96 else 32))))
        if blkw == 1 or (blkw == -1 and auto):
            return f"conv_psf_map_blkw_kernel<{ks}, {rb}>", "blkw"
    if ks >= 13 and path is None:
        nk = (16 + ks - 1 + 31) // 32
        twp = thp = 32 + ks - 1
        P = (twp + 7) // 8 * 8
        while P % 16 != 8:
            P += 8
        if P < 32 * nk + 24:
            P = 32 * nk + 24
        while P % 16 != 8:
            P += 8
        tile_b, rows_b = 2 * thp * P * 2, ks * 2 * (32 * nk + 18) * 2
        ksplit = S < 2 or tile_b + 4 * rows_b > 64 * 1024 - 64 or ks > 31
        k = "true" if ksplit else "false"
        if ks <= 17:
            return f"conv_psf_map_toeplitz_wide_kernel<1, {k}, 12, {2 if ksplit else 5}>", "toeplitz_wide"
        if ks <= 21:
            return f"conv_psf_map_toeplitz_wide_kernel<2, {k}, 13, {2 if ksplit else 7}>", "toeplitz_wide"
        if ks <= 31:
            return f"conv_psf_map_toeplitz_wide_kernel<2, {k}, 16, {4 if ksplit else 16}>", "toeplitz_wide"
        if ks <= 49:
            return "conv_psf_map_toeplitz_wide_kernel<2, true, 20, 10>", "toeplitz_wide"
        return "conv_psf_map_toeplitz_wide_kernel<3, true, 21, 11>", "toeplitz_wide"
    if ks not in (3, 5, 7, 9, 11, 13, 15, 21):
        return "conv_psf_map_generic_kernel", "generic"
    maxnw = 5 if ks == 11 else 4
    nw, best = 1, 1 << 30
    for n in range(maxnw, (2 if S > 1 else 1) - 1, -1):
        if ks != 11 and n == 3:
            continue
        waste = -(-S // n) * n - S
        if waste < best:
            best, nw = waste, n
    if "AADFF_CONV_NW" in env and ks == 11:
        v = _atoi(env["AADFF_CONV_NW"], 0)
        if 1 <= v <= maxnw:
            nw = v
    if ks == 11 and S >= 3 and path is None:
        pair = "true" if max(0, _atoi(env.get("AADFF_CONV_PAIR"), 0)) > 0 else "false"
        return f"conv_psf_map_sbatch_kernel<24, {nc_of(S)}, {pair}, false, false>", "sbatch"
    if ks in (9, 11) and S == 1 and path is None:
        return f"conv_psf_map_blk_kernel<{ks}, false>", "blk"
    if ks <= 11 and not (path or "").startswith("v"):
        return f"conv_psf_map_mfma_kernel<{ks}, {nw}, 1>", "mfma"
    return f"conv_psf_map_kernel<{ks}, {nw}>", "valu"


def _atoi(s, default):
    if s is None:
        return default
    try:
        return int(s)
    except ValueError:
        return 0


def toeplitz_slices_per_workgroup(c):
    """spw of the wide Toeplitz launch (conv_plan): the slices one workgroup renders from its staged tile."""
    hb, wb = _bounds(c.H, c.grid), _bounds(c.W, c.grid)
    mh, mw = max(b - a for a, b in zip(hb, hb[1:])), max(b - a for a, b in zip(wb, wb[1:]))
    ksplit = "true" in dispatch(c)[0]
    tiles = -(-mw // 32) * c.grid * -(-mh // 32) * c.grid * c.B * c.C
    spw = c.S
    while spw > (1 if ksplit else 4) and tiles * -(-c.S // spw) < 2048:
        spw = (spw + 1) // 2
    return spw if ksplit else (spw + 3) // 4 * 4


def workgroups_block_gemm(c):
    """Workgroups of a blk / blkw launch: 65536 and above are decoded without the magic-number division."""
    name = dispatch(c)[0]
    rb = int(name.split(",")[1].strip(" >")) if "blkw" in name else 24
    hb, wb = _bounds(c.H, c.grid), _bounds(c.W, c.grid)
    mh, mw = max(b - a for a, b in zip(hb, hb[1:])), max(b - a for a, b in zip(wb, wb[1:]))
    return -(-mw // 96) * c.grid * -(-mh // rb) * c.grid * c.B * c.C * c.S


def expected_instantiations():
    """Every conv_psf_map_* instantiation of the library except the TIMED ones (reached through aadff_time_next_launch only)."""
    out = {"conv_psf_map_generic_kernel", "conv_psf_map_blk_kernel<9, false>", "conv_psf_map_blk_kernel<11, false>"}
    out |= {f"conv_psf_map_blkw_kernel<{k}, {rb}>" for k in range(3, 22, 2) for rb in (24, 32, 48)}
    for k in (3, 5, 7, 9, 13, 15, 21):
        out |= {f"conv_psf_map_kernel<{k}, {n}>" for n in (1, 2, 4)}
    for k in (3, 5, 7, 9):
        out |= {f"conv_psf_map_mfma_kernel<{k}, {n}, 1>" for n in (1, 2, 4)}
    out |= {f"conv_psf_map_kernel<11, {n}>" for n in range(1, 6)} | {f"conv_psf_map_mfma_kernel<11, {n}, 1>" for n in range(1, 6)}
    for nc in range(1, 5):
        out |= {f"conv_psf_map_sbatch_kernel<24, {nc}, {p}, false, {l}>" for p, l in (("false", "false"), ("true", "false"), ("false", "true"))}
    out |= {"conv_psf_map_toeplitz_wide_kernel<%s>" % t for t in ("1, false, 12, 5", "1, true, 12, 2", "2, false, 13, 7", "2, true, 13, 2",
                                                                 "2, false, 16, 16", "2, true, 16, 4", "2, true, 20, 10", "3, true, 21, 11")}
    return out


# ------------------------------------------------------------------------------------------------------------------------ the table
SMALL = dict(B=1, C=2, H=77, W=70, grid=2)            # 38/39 x 35 patches: 2 x 2 tiles of 32 x 32 per patch, the last ones partial


def _case(group, ks, S, env=None, entry=None, signed=False, L=0, tag="", **shape):
    sh = dict(SMALL, **shape)
    env = dict(env or {})
    entry = entry or ("map" if S == 1 else "stack")
    short = {"AADFF_CONV_PATH": "path", "AADFF_CONV_BLKW": "blkw", "AADFF_CONV_BLKW_RB": "rb", "AADFF_CONV_NW": "nw", "AADFF_CONV_PAIR": "pair"}
    cid = f"{group}-ks{ks}-S{S}" + (f"xL{L}" if L else "") + f"-{sh['B']}x{sh['C']}x{sh['H']}x{sh['W']}-g{sh['grid']}"
    cid += "".join(f"-{short[k]}={v}" for k, v in env.items()) + ("" if entry in ("map", "stack") else f"-{entry}") + ("-signed" if signed else "") + tag
    return Case(cid, group, entry, env, sh["B"], sh["C"], S, sh["H"], sh["W"], sh["grid"], ks, signed, L)


def _table():
    t = []
    TOE, VALU = {"AADFF_CONV_PATH": "toeplitz"}, {"AADFF_CONV_PATH": "valu"}
    # (A) blkw<K,RB>: all 30, last band and last 8-row group partial, patches wider than a 96-column tile that start at an odd column
    for ks in range(3, 22, 2):
        for rb in (24, 32, 48):
            t.append(_case("A", ks, 2, {"AADFF_CONV_BLKW": "1", "AADFF_CONV_BLKW_RB": str(rb)}, B=2, C=2, H=2 * (59 if rb == 48 else 41), W=202, grid=2))
    for ks in (21, 13):                                  # both sides of every threshold of the ks >= 13 band-height rule
        for H in (24, 25, 32, 33, 48, 49, 64, 65, 96, 97):
            t.append(_case("A", ks, 1, B=1, C=2, H=H, W=50, grid=1))
    t.append(_case("A", 5, 1, B=1, C=7, H=768, W=96, grid=8))            # 448 units x 4 bands: two rounds of 1536 slots, x 3: one -> 32 rows
    t.append(_case("A", 5, 1, B=5, C=13, H=32, W=32, grid=32))           # 66 560 workgroups: decoded without the magic division
    # (B) blk<9>, blk<11>
    for ks, env in ((9, {"AADFF_CONV_BLKW": "0"}), (11, {"AADFF_CONV_BLKW": "0"}), (11, {})):
        t.append(_case("B", ks, 1, env, H=77, W=202))
        t.append(_case("B", ks, 1, env, B=5, C=13, H=32, W=32, grid=32))
    t.append(_case("B", 11, 1, B=2, C=1, H=2 * 96, W=45, grid=2))        # the tallest patch the default still gives to blk<11>
    # (C) sbatch<24,NC,PAIR> and the layered entry
    for S in (3, 4, 5, 8, 9, 12, 13, 16, 17):
        for pair in ("0", "1"):
            t.append(_case("C", 11, S, {"AADFF_CONV_PAIR": pair}, H=82, W=202 if S == 5 else 106))
    for S, L in ((2, 2), (1, 5), (4, 3), (1, 13), (5, 4)):
        t.append(_case("C", 11, S, entry="layered", L=L, B=2, C=2, H=59, W=106))
    # (D) mfma<KS,NW,1>
    for ks in (3, 5, 7, 9):
        t += [_case("D", ks, S, TOE) for S in (1, 2, 4, 7)]
    t += [_case("D", 11, S, TOE) for S in (1, 2, 3, 4, 5, 9)]
    t += [_case("D", 11, 7, dict(TOE, AADFF_CONV_NW=v)) for v in ("1", "2", "3", "5")]
    # (E) packed-FMA and generic kernels
    for ks in (3, 5, 7, 9, 13, 15, 21):
        t += [_case("E", ks, S, VALU) for S in (1, 2, 4, 6)]
    t += [_case("E", 11, S, VALU) for S in (1, 2, 3, 4, 5)]
    t += [_case("E", 1, 1, VALU), _case("E", 1, 3, VALU)]
    t += [_case("E", ks, 2, VALU) for ks in (17, 19, 23, 51)]
    # (F) toeplitz_wide
    for ks in (13, 17, 19, 21):
        t += [_case("F", ks, S, {"AADFF_CONV_BLKW": "0"}) for S in (1, 5)]
    for ks in (23, 27, 31):
        t += [_case("F", ks, S) for S in (1, 2, 6)]
    for ks in (33, 41, 49, 51):
        t += [_case("F", ks, S) for S in (1, 3)]
    t.append(_case("F", 51, 1, B=1, C=2, H=26, W=27, grid=1))            # every row and column reflected
    t.append(_case("F", 13, 8, {"AADFF_CONV_BLKW": "0"}, B=1, C=8, H=48, W=48, grid=16))     # 2048 tiles: the workgroup keeps all 8 slices
    t.append(_case("F", 33, 4, B=1, C=8, H=48, W=48, grid=16))
    # (G) the uniform-PSF entry and the strided stack entry, one case per family
    for ks, env in ((7, VALU), (17, VALU), (7, TOE), (11, {}), (5, {}), (27, {})):
        t.append(_case("G", ks, 1, env, entry="psf", grid=1))
    for ks, S, env in ((7, 2, VALU), (17, 2, VALU), (7, 2, TOE), (11, 5, {}), (11, 1, {}), (21, 2, {}), (27, 2, {})):
        t.append(_case("G", ks, S, env, entry="strided"))
    # signed taps, one per family
    for ks, S, env in ((7, 2, VALU), (17, 2, VALU), (7, 2, TOE), (11, 5, {}), (11, 1, {}), (21, 1, {}), (27, 2, {})):
        t.append(_case("signed", ks, S, env, signed=True))
    return t


TABLE = _table()
NW_IGNORED = [_case("D", 11, 7, {"AADFF_CONV_PATH": "toeplitz", "AADFF_CONV_NW": v}) for v in ("9", "x")]
NW_DEFAULT = _case("D", 11, 7, {"AADFF_CONV_PATH": "toeplitz"})
TINY = [_case("tiny", 3, 2, B=2, C=2, H=5, W=7, grid=2), _case("tiny", 5, 1, B=1, C=2, H=4, W=6, grid=1, signed=True),
        _case("tiny", 1, 2, B=1, C=1, H=3, W=3, grid=3)]


def is_plain(c):
    return dispatch(c)[1] in PLAIN


# ------------------------------------------------------------------------------------------------------------------------- inputs
def inputs(c):
    """(img [B,C,H,W], maps [M,C,g ks,g ks] with M = S (S L for the layered entry), layer_idx uint8 [B,H,W] or None), float32, CPU."""
    M, g, ks = c.S * max(c.L, 1), c.grid, c.ks
    gen = torch.Generator().manual_seed(1009 * ks + 31 * c.H + 7 * c.W + 3 * M + c.grid + (500000 if c.signed else 0))
    img = torch.rand((c.B, c.C, c.H, c.W), generator=gen) * 37.5 - 3.0
    w = torch.rand((M, c.C, g, ks, g, ks), generator=gen)
    if c.signed:
        w = w - 0.4
        w = w / w.abs().sum((3, 5), keepdim=True)
    else:
        w = w + 0.05
        w = w / w.sum((3, 5), keepdim=True)
    if M >= 2:
        w[M // 2] *= 1e-3
    elif c.C >= 2:
        w[0, 0] *= 1e-3
    lidx = None
    if c.L:
        y, x, b = torch.arange(c.H)[None, :, None], torch.arange(c.W)[None, None, :], torch.arange(c.B)[:, None, None]
        lidx = ((7 * y + x + b) % c.L).to(torch.uint8).contiguous()      # changes from every pixel to the next: inside every 2 x 2 block, across every band border
    return img.contiguous(), w.reshape(M, c.C, g * ks, g * ks).contiguous(), lidx


def oracle64(img, maps, grid):
    """float64 [B,C,M,H,W]: oracle.conv.render_psf_map on double inputs, slice by slice."""
    return torch.stack([oconv.render_psf_map(img.double(), m.double(), grid) for m in maps], dim=2)


def oracle32(img, maps, grid):
    return torch.stack([oconv.render_psf_map(img, m, grid) for m in maps], dim=2)


def _reflect(i, n):
    i = -i if i < 0 else i
    return 2 * n - 2 - i if i >= n else i


def loop64(img, maps, grid):
    """The definition, pixel by pixel in Python floats: reflect padding, the patch of the OUTPUT pixel selects the PSF.  Tiny cases only."""
    B, C, H, W = img.shape
    M, ks = maps.shape[0], maps.shape[-1] // grid
    p = ks // 2
    hb, wb = _bounds(H, grid), _bounds(W, grid)
    pi = [max(i for i in range(grid) if hb[i] <= y) for y in range(H)]
    pj = [max(j for j in range(grid) if wb[j] <= x) for x in range(W)]
    x64, w64 = img.double().tolist(), maps.double().tolist()
    out = torch.zeros((B, C, M, H, W), dtype=torch.float64)
    for b in range(B):
        for c in range(C):
            for m in range(M):
                for y in range(H):
                    for x in range(W):
                        s = 0.0
                        for u in range(ks):
                            for v in range(ks):
                                wv = w64[m][c][pi[y] * ks + ks - 1 - u][pj[x] * ks + ks - 1 - v]
                                s += x64[b][c][_reflect(y - p + u, H)][_reflect(x - p + v, W)] * wv
                        out[b, c, m, y, x] = s
    return out


def _taps(img, maps, grid, clamp_row=False):
    """Yields, tap by tap in row-major (u, v) order, the window values [B,C,1,H,W] and the tap planes [1,C,M,H,W] in float64.
    clamp_row plants an error: image row -1 is read as row 0 (clamped) instead of row 1 (reflected)."""
    B, C, H, W = img.shape
    ks = maps.shape[-1] // grid
    p = ks // 2
    x = np.pad(img.numpy().astype(np.float64), ((0, 0), (0, 0), (p, p), (p, p)), mode="reflect")
    if clamp_row:
        x[:, :, p - 1] = x[:, :, p]
    w = maps.numpy().astype(np.float64)
    hb, wb = _bounds(H, grid), _bounds(W, grid)
    pi = np.searchsorted(np.asarray(hb[1:]), np.arange(H), side="right")
    pj = np.searchsorted(np.asarray(wb[1:]), np.arange(W), side="right")
    for u in range(ks):
        rows = w[:, :, pi * ks + ks - 1 - u, :]                                          # [M,C,H,g ks]
        for v in range(ks):
            yield x[:, :, None, u:u + H, v:v + W], rows[:, :, :, pj * ks + ks - 1 - v].transpose(1, 0, 2, 3)[None]


def definition64(img, maps, grid, clamp_row=False):
    """float64 [B,C,M,H,W]: the sum over the taps, in numpy (independent of torch's conv2d)."""
    out = 0.0
    for xs, ws in _taps(img, maps, grid, clamp_row):
        out = out + xs * ws
    return torch.from_numpy(out)


def sums(img, maps, grid):
    """sequential32 (the float32 fma chain in row-major tap order) [B,C,M,H,W], A = sum|x w| [B,C,M,H,W], SX = sum|x| [B,C,1,H,W],
    SW = sum|w| [1,C,M,H,W] (float64)."""
    B, C, H, W = img.shape
    M = maps.shape[0]
    acc = np.zeros((B, C, M, H, W), dtype=np.float32)
    A, prod, t64 = np.zeros((B, C, M, H, W)), np.empty((B, C, M, H, W)), np.empty((B, C, M, H, W))
    SX, SW = np.zeros((B, C, 1, H, W)), np.zeros((1, C, M, H, W))
    for xs, ws in _taps(img, maps, grid):
        np.multiply(xs, ws, out=prod)                       # exact: 48 bits
        np.add(acc, prod, out=t64)
        acc[...] = t64                                      # one fma step: the sum rounded to float32
        np.abs(prod, out=prod)
        A += prod
        SX += np.abs(xs)
        SW += np.abs(ws)
    return torch.from_numpy(acc), torch.from_numpy(A), torch.from_numpy(SX), torch.from_numpy(SW)


def _pow2_scale(amax):
    """pow2_scale of csrc/conv.hip: 2^(9 - floor(log2 amax)) elementwise (1 for 0)."""
    e = np.floor(np.log2(np.where(amax > 0, amax, 1.0)))
    return np.where(amax > 0, 2.0 ** (9 - e), 1.0)


def _split(v):
    hi = v.astype(np.float16).astype(np.float32)
    return hi, (v - hi).astype(np.float16).astype(np.float32)              # v - hi is exact in float32


def split_restatement(img, maps, grid):
    """float32 [B,C,M,H,W]: the matrix-core arithmetic with whole-plane scales - every operand split into fp16 hi + lo after its
    power-of-two scale, hi*hi, hi*lo and lo*hi formed exactly (22 bits: float32 holds them as float64 would) and added one by one to a
    float32 accumulator, lo*lo dropped."""
    sx = _pow2_scale(img.abs().amax((2, 3), keepdim=True).numpy().astype(np.float64))                 # [B,C,1,1]
    sw = _pow2_scale(maps.abs().amax((2, 3), keepdim=True).numpy().astype(np.float64))                # [M,C,1,1]
    xi = img.double() * torch.from_numpy(sx)
    wi = maps.double() * torch.from_numpy(sw)
    B, C, H, W = img.shape
    acc = np.zeros((B, C, maps.shape[0], H, W), dtype=np.float32)
    prod = np.empty_like(acc)
    for xs, ws in _taps(xi, wi, grid):
        xh, xl = _split(xs.astype(np.float32))
        wh, wl = _split(ws.astype(np.float32))
        for a, b in ((xh, wh), (xh, wl), (xl, wh)):
            np.multiply(a, b, out=prod)
            acc += prod
    inv = 1.0 / (sx[:, :, None] * sw.transpose(1, 0, 2, 3)[None])                                      # [B,C,M,1,1]
    return torch.from_numpy((acc.astype(np.float64) * inv).astype(np.float32))


_HOST = {}


def host_results(c):
    """(the oracle's own float32 result, the split restatement) over all maps of a case, cached by shape like the references."""
    key = _key(c)
    if key not in _HOST:
        f = _full(c)
        _HOST[key] = (oracle32(f.img, f.maps, c.grid), split_restatement(f.img, f.maps, c.grid))
    return _HOST[key]


# ------------------------------------------------------------------------------------------------------------------ references
Ref = collections.namedtuple("Ref", "img maps lidx out64 A SX SW Xmax Wmax seq d32seq")
_REF, _FULL = {}, {}


def _key(c):
    return (c.B, c.C, c.S * max(c.L, 1), c.H, c.W, c.grid, c.ks, c.signed, c.L)


def _full(c):
    key = _key(c)
    if key not in _FULL:
        img, maps, lidx = inputs(c)
        out64 = oracle64(img, maps, c.grid)
        seq, A, SX, SW = sums(img, maps, c.grid)
        Xmax = img.double().abs().amax((2, 3), keepdim=True)[:, :, None]                               # [B,C,1,1,1]
        Wmax = maps.double().abs().amax((2, 3), keepdim=True).permute(1, 0, 2, 3)[None]                # [1,C,M,1,1]
        _FULL[key] = Ref(img, maps, lidx, out64, A, SX, SW, Xmax, Wmax, seq, rel_l2(seq, out64))
    return _FULL[key]


def reference(c):
    """Ref of a case, computed once per process and shared: do not modify.  out64, A, SW, Wmax and seq have the shape of the result,
    [B,C,S,H,W]; for the layered entry they are slice s of layer layer_idx[b,y,x], composed here."""
    if c.id in _REF:
        return _REF[c.id]
    f = _full(c)
    if c.L:
        shape = (c.B, c.C, c.S, c.H, c.W)
        idx = (torch.arange(c.S)[None, None, :, None, None] * c.L + f.lidx.long()[:, None, None]).expand(shape)
        pick = lambda a: torch.gather(a.expand(c.B, c.C, c.S * c.L, c.H, c.W), 2, idx)
        seq, out64 = pick(f.seq), pick(f.out64)
        f = Ref(f.img, f.maps, f.lidx, out64, pick(f.A), f.SX, pick(f.SW), f.Xmax, pick(f.Wmax), seq, rel_l2(seq, out64))
    _REF[c.id] = f
    return f


def bound(c, r, plain=None):
    """The elementwise bound of the module docstring, [B,C,S,H,W] float64."""
    n = c.ks * c.ks
    plain = is_plain(c) if plain is None else plain
    if plain:
        return n * U * r.A + U * r.out64.abs()
    res = r.Xmax * r.SW + r.Wmax * r.SX
    b = n * U * r.A + 2.0 ** -23 * res + 2.0 ** -22 * (1 + 2.0 ** -9) * r.A + 2.0 ** -42 * res + U * r.out64.abs()
    return torch.minimum(b, torch.full_like(b, MC_CAP))


def compare(c, got, r, plain=None):
    """(largest |got - o64| / bound over EVERY element, its flat index, rel_l2 in d32seq units)."""
    assert tuple(got.shape) == tuple(r.out64.shape) and got.dtype == torch.float32
    assert bool(torch.isfinite(got).all())
    use = (got.double() - r.out64).abs() / bound(c, r, plain)
    worst = int(use.argmax())
    return float(use.flatten()[worst]), worst, (rel_l2(got, r.out64) / r.d32seq if r.d32seq > 0 else 0.0)
