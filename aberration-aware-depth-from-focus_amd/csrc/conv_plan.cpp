// Patch convolution, host side: the rule that picks the conv_psf_map_* instantiation (conv.hip) for a call, stated once, top to
// bottom in the order it applies.  conv_plan fills a ConvPlan or refuses; conv_launch (conv.hip) launches what the plan says and
// aadff_conv_plan_describe reports it.  No HIP call and no allocation here; nothing is cached across calls (the tests switch the
// environment between launches).
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include "conv_plan.h"

// common.h's, which this unit does not include (no HIP here)
#define AADFF_CHECK_ARG(cond, ...)                    \
    do {                                              \
        if (!(cond)) {                                \
            ::aadff::set_error(__VA_ARGS__);          \
            return AADFF_EINVAL;                      \
        }                                             \
    } while (0)

#ifndef AADFF_CONV_PAIR_DEFAULT
#define AADFF_CONV_PAIR_DEFAULT 0      // measured: every pairing is slower than one band per workgroup
#endif

namespace aadff {

// the shape domain of the patch convolution, shared by the forward entries and their backward (conv_bwd.hip)
int conv_check_shape(int B, int C, int S, int H, int W, int grid, int ks) {
    AADFF_CHECK_ARG(B > 0 && C > 0 && S > 0 && H > 0 && W > 0, "render_psf_map: empty tensor (B=%d C=%d S=%d H=%d W=%d)", B, C, S, H, W);
    AADFF_CHECK_ARG(grid >= 1 && grid <= AADFF_MAX_GRID, "render_psf_map: grid %d outside [1,%d]", grid, AADFF_MAX_GRID);
    AADFF_CHECK_ARG(ks % 2 == 1, "PSF kernel size should be odd");
    AADFF_CHECK_ARG(ks >= 1 && ks <= AADFF_MAX_KS, "render_psf_map: ks %d outside [1,%d]", ks, AADFF_MAX_KS);
    AADFF_CHECK_ARG(ks / 2 < H && ks / 2 < W, "render_psf_map: reflect padding %d needs H,W > pad", ks / 2);
    AADFF_CHECK_ARG(grid <= H && grid <= W, "render_psf_map: grid %d larger than image %dx%d", grid, H, W);
    AADFF_CHECK_ARG((size_t)B * C <= 65535, "render_psf_map: B*C too large");
    return 0;
}

namespace {

// a 3-D launch of ntx x nty tiles (or bands) per patch, B * C * nchunk planes deep, decoded with the magic multipliers
void grid_3d(ConvPlan& pl, int ntx, int nty, int nchunk, int B, int C) {
    pl.ntx = ntx; pl.nty = nty; pl.nchunk = nchunk;
    pl.gx = (unsigned)(ntx * pl.grid); pl.gy = (unsigned)(nty * pl.grid); pl.gz = (unsigned)(B * C * nchunk);
    pl.pb.m_ntx = magic_of(ntx); pl.pb.m_nty = magic_of(nty); pl.pb.m_nchunk = magic_of(nchunk); pl.pb.m_c = magic_of(C);
}

// a 1-D launch of `total` workgroups in XCD order (xcd_remap, common.h) over bntx x bnty bands per patch, one slice each
void grid_xcd(ConvPlan& pl, int bntx, int bnty, size_t gx, size_t gy, size_t total, int C, int S) {
    pl.ntx = bntx; pl.nty = bnty; pl.nchunk = S;
    pl.gx = (unsigned)total; pl.gy = pl.gz = 1;
    PatchBounds& pbb = pl.pb;
    pbb.m_ntx = magic_of(bntx); pbb.m_nty = magic_of(bnty); pbb.m_nchunk = magic_of(S); pbb.m_c = magic_of(C);
    pbb.gx = (unsigned)gx; pbb.gy = (unsigned)gy;
    const bool magic = total < 65536;
    pbb.m_gx = magic ? (gx == 1 ? 1u : magic_of((unsigned)gx)) : 0u;           // (udiv_magic returns n for d == 1; the flag is m_gx != 0)
    pbb.m_gy = magic ? (gy == 1 ? 1u : magic_of((unsigned)gy)) : 0u;
    pbb.xcd_q = total >= 64 ? (unsigned)(total / 8) : 0u;
    pbb.xcd_r = (unsigned)(total % 8);
}

// the slice-batched kernel's geometry for `maps` maps: NC chunks of 4 maps per workgroup, npass passes over them, bands of 24 rows
int plan_sbatch(ConvPlan& pl, const char* who, int maps, bool pair, bool layered, int B, int C, int mh, int mw) {
    constexpr int RB = kConvSbRows;          // band rows (8/12/16/32/48 measured slower)
    const int nc = maps <= 4 ? 1 : (maps <= 8 ? 2 : (maps <= 12 ? 3 : 4));
    const int npass = (maps + 4 * nc - 1) / (4 * nc);
    const int sntx = (mw + kConvBandCols - 1) / kConvBandCols, snty = (mh + RB - 1) / RB;
    AADFF_CHECK_ARG((size_t)B * C * npass <= 65535 && (size_t)snty * pl.grid <= 65535, "%s: grid too large", who);
    pl.family = ConvFamily::sbatch;
    pl.targ[0] = RB; pl.targ[1] = nc; pl.targ[2] = pair; pl.targ[3] = 0; pl.targ[4] = layered;
    pl.block = 64 * nc;
    pl.S = maps;
    grid_3d(pl, sntx, snty, npass, B, C);
    return 0;
}

int plan_layered(ConvPlan& pl, bool ptrs_ok, int B, int C, int S, int L, int H, int W, int grid, int ks) {
    AADFF_CHECK_ARG(ptrs_ok, "render_psf_map_stack_layered: NULL pointer");
    AADFF_CHECK_ARG(B > 0 && C > 0 && S > 0 && L >= 1 && L <= 254 && H > 0 && W > 0, "render_psf_map_stack_layered: B=%d C=%d S=%d L=%d H=%d W=%d", B, C, S, L, H, W);
    AADFF_CHECK_ARG(grid >= 1 && grid <= AADFF_MAX_GRID && grid <= H && grid <= W, "render_psf_map_stack_layered: grid %d", grid);
    if (ks != 11) {
        set_error("render_psf_map_stack_layered: the fused form exists for ks 11 only (ks %d: compose aadff_render_psf_map_stack and a gather)", ks);
        return AADFF_EUNSUPPORTED;
    }
    AADFF_CHECK_ARG(5 < H && 5 < W, "render_psf_map_stack_layered: reflect padding 5 needs H,W > pad");
    return 0;
}

}  // namespace

int conv_plan(ConvPlan& pl, ConvEntry entry, bool ptrs_ok, int B, int C, int S, int L, int H, int W, int grid, int ks, long sbc, long ss) {
    std::memset(&pl, 0, sizeof(pl));
    const bool layered = entry == ConvEntry::layered;
    if (layered) {
        if (int rc = plan_layered(pl, ptrs_ok, B, C, S, L, H, W, grid, ks)) return rc;
    } else {
        if (entry == ConvEntry::strided) {
            AADFF_CHECK_ARG(sbc >= (long)H * W && ss >= (long)H * W, "render_psf_map_stack_strided: strides %ld / %ld below one plane (%d x %d)",
                            sbc, ss, H, W);
            // the S*B*C planes must not overlap: either slices are innermost (stride_bc >= S*stride_s) or (b, c) planes are (stride_s >= B*C*stride_bc)
            AADFF_CHECK_ARG(sbc >= (long)S * ss || ss >= (long)B * C * sbc,
                            "render_psf_map_stack_strided: planes overlap (stride_bc %ld, stride_s %ld, B*C %d, S %d)", sbc, ss, B * C, S);
        }
        AADFF_CHECK_ARG(ptrs_ok, "render_psf_map: NULL pointer");
        if (int rc = conv_check_shape(B, C, S, H, W, grid, ks)) return rc;
    }
    pl.C = C; pl.S = S; pl.L = 1; pl.H = H; pl.W = W; pl.grid = grid; pl.ks = ks;
    fill_bounds(pl.pb.hb, grid, H);
    fill_bounds(pl.pb.wb, grid, W);
    int mh = 0, mw = 0;                                       // the largest patch
    for (int i = 0; i < grid; ++i) {
        mh = std::max(mh, pl.pb.hb[i + 1] - pl.pb.hb[i]);
        mw = std::max(mw, pl.pb.wb[i + 1] - pl.pb.wb[i]);
    }
    if (layered) {
        // one launch of the slice-batched kernel over the S * L (slice, layer) maps; the events of aadff_time_next_launch go around it
        if (int rc = plan_sbatch(pl, "render_psf_map_stack_layered", S * L, false, true, B, C, mh, mw)) return rc;
        AADFF_CHECK_ARG((size_t)H * W <= ((size_t)1 << 27) && 4 * ((size_t)S * ss + (size_t)H * W) < ((size_t)1 << 32),
                        "render_psf_map_stack_layered: a (b, c) plane stack above 2^30 elements is not supported");
        pl.L = L;
        return 0;
    }

    // the switches, each read once per call
    const char* penv = getenv("AADFF_CONV_PATH");              // path: "mfma" (Toeplitz GEMM on fp16-split MFMA, KS <= 11) or "valu" (packed fp32 FMA); AADFF_CONV_PATH overrides
    const char* benv = getenv("AADFF_CONV_BLKW");
    const char* renv = getenv("AADFF_CONV_BLKW_RB");
    const char* nenv = getenv("AADFF_CONV_NW");                // tuning override, validated: garbage / out-of-range values are ignored
    const char* qenv = getenv("AADFF_CONV_PAIR");

    const int ntx = (mw + kConvTile - 1) / kConvTile, nty = (mh + kConvTile - 1) / kConvTile;
    if (ks >= 3 && ks <= 21 && !penv) {
        // block-GEMM form (conv_psf_map_blkw_kernel): AADFF_CONV_BLKW = 0 never, 1 always, unset: where it measured faster
        // (tools/conv_blkw_probe.py -> profiles/r05_y_conv_blkw_probe.txt, 1024^2, us per launch blkw / wide Toeplitz / packed-FMA -
        // lone slices at grid 7: ks 13 15.0 / 31.6 / 30.8, ks 15 22.3 / 32.0 / 41.3, ks 17 21.4 / 33.5 / 94.8, ks 19 30.7 / 41.4 / 110.5,
        // ks 21 27.3 / 43.6 / 79.8 (grid 11: 24.3 / 38.7 / 80.4); 10-slice stacks (one workgroup per slice and band here, the Toeplitz
        // form shares its staged tile between four slices) at grid 7 / 11: ks 13 105 / 113 and 78 / 105, ks 15 156 / 124 and 113 / 109,
        // ks 17 134 / 131 and 100 / 124, ks 19 291 / 247 and 198 / 217, ks 21 224 / 270 and 158 / 237)
        const int blkw = benv ? atoi(benv) : -1;
        // ks 9 / 11 lone slices (us, conv_psf_map_blk_kernel / this kernel with 24- / 32- / 48-row bands; ks 9's window here is 12 x 12 =
        // 5 k-steps, the older kernel's fixed 14 x 14 = 7): ks 9 grid 7 16.3 / 13.0 / 12.1 / 13.2, grid 11 12.9 / 11.1 / 11.4 / 12.0, grid 5
        // 15.1 / 11.7 / 12.1 / 12.8; ks 11 grid 7 15.4 / 15.9 / 13.2 / 14.9, grid 11 12.3 / 12.9 / 13.4 / 12.9, grid 5 14.8 / 15.7 / 14.0 / 14.7
        // ks 3 / 5 / 7 (window ks + 3: 2 / 2 / 4 k-steps; the Toeplitz kernel (b) issues 3 ks MFMAs per 16 x 16 block, this form 3 NST per
        // 16 x 16): lone slices 9 - 12 us against 13 - 17 at every grid, 10-slice stacks faster at ks 5 only (grid 7 / 11: 53 / 47 against 62 / 54)
        const bool use = blkw == 1 || (blkw == -1 && (ks >= 13 ? (S == 1 || ks == 13 || ks == 17 || ks == 21)
                                                                : (S == 1 ? (ks <= 9 || mh > 96) : ks == 5)));
        // rows per band: every workgroup pays ~5.5 us of loads / staging / fragment building in front of 0.76 us of matrix work per
        // 8-row group (tools/conv_single_timeline.py --ks 21: profiles/r05_y_conv_blkw_timeline_ks21.json), so taller bands win until the
        // launch is too few workgroups for two rounds on 512 slots.  Measured at 1024^2 (ks 21, us, RB 24 / 32 / 48): grid 7 (147-row
        // patches) 32.4 / 27.8 / 30.6, grid 11 (94) 25.2 / 25.3 / 24.2, grid 5 (205) 29.1 / 26.8 / 25.4; the other ks alike.
        int rb = renv ? atoi(renv) : 0;
        if (rb != 24 && rb != 32 && rb != 48) {
            if (ks <= 11) {
                // 6 workgroups per CU: 32-row bands when that saves a round of workgroups on the chip's 1536 slots (1024^2: grid 7 yes,
                // grid 5 / 11 no - measured, ks 5: 9.4 / 9.1, 9.2 / 9.7, 8.7 / 8.9 us with 24 / 32 rows)
                const size_t per = (size_t)((mw + 95) / 96) * grid * grid * B * C * S;
                const size_t w24 = per * ((mh + 23) / 24), w32 = per * ((mh + 31) / 32);
                rb = (w24 + 1535) / 1536 > (w32 + 1535) / 1536 ? 32 : 24;
            } else rb = mh <= 24 ? 24 : (mh <= 32 ? 32 : (mh <= 48 ? 48 : (mh <= 64 ? 32 : (mh <= 96 ? 48 : 32))));
        }
        const int bntx = (mw + kConvBandCols - 1) / kConvBandCols, bnty = (mh + rb - 1) / rb;
        const size_t gx = (size_t)bntx * grid, gy = (size_t)bnty * grid, total = gx * gy * B * C * S;
        if (use && total < ((size_t)1 << 31) && (size_t)H * W <= ((size_t)1 << 30)) {
            pl.family = ConvFamily::blkw;
            pl.targ[0] = ks; pl.targ[1] = rb;
            pl.block = 192;
            grid_xcd(pl, bntx, bnty, gx, gy, total, C, S);
            return 0;
        }
    }
    if (ks >= 13 && !penv) {
        // large kernels on the matrix cores (Toeplitz GEMM over NK k-steps); AADFF_CONV_PATH=valu keeps the packed-FMA / generic kernels
        const int nk = (16 + ks - 1 + 31) / 32;                         // 1: ks <= 17, 2: ks <= 49, 3: ks 51
        const int twp = kConvTile + ks - 1, thp = kConvTile + ks - 1;
        int P = (twp + 7) / 8 * 8;
        while (P % 16 != 8) P += 8;                                      // P / 2 dwords = 4 (mod 8): conflict-free A-fragment reads
        if (P < 32 * nk + 16 + 8) P = 32 * nk + 24;                      // the last k-step's 8 halves stay inside the row (zero padding)
        while (P % 16 != 8) P += 8;
        const size_t tile_b = (size_t)2 * thp * P * 2, rows_b = (size_t)ks * 2 * (32 * nk + 18) * 2;      // fp16: 2 bytes
        // waves = slices when four tap-row sets fit beside the tile and there are slices to share it; else the waves split the tap rows
        const bool ksplit = S < 2 || tile_b + 4 * rows_b > 64 * 1024 - 64 || ks > 31;
        const size_t lds = tile_b + (ksplit ? std::max(rows_b, (size_t)16384) : 4 * rows_b);
        AADFF_CHECK_ARG(lds <= 64 * 1024 - 64, "render_psf_map: ks %d needs %zu bytes of LDS", ks, lds);
        // slices per workgroup: the whole stack from one staged tile unless that leaves the chip short of workgroups
        const long tiles = (long)ntx * grid * nty * grid * B * C;
        int spw = S;
        while (spw > (ksplit ? 1 : 4) && tiles * ((S + spw - 1) / spw) < 2048) spw = (spw + 1) / 2;
        if (!ksplit) spw = (spw + 3) / 4 * 4;
        const int nchunk = (S + spw - 1) / spw;
        AADFF_CHECK_ARG((size_t)B * C * nchunk <= 65535, "render_psf_map: B*C*chunks too large");
        pl.family = ConvFamily::toeplitz_wide;
        // size classes: rows per thread = ceil((32 + ks - 1) / 4), taps per thread = ceil(ks^2 / 256) (tap rows split) or / 64 (slices split)
        const int maxr = ks <= 17 ? 12 : (ks <= 21 ? 13 : (ks <= 31 ? 16 : (ks <= 49 ? 20 : 21)));
        const int maxt = ks <= 17 ? (ksplit ? 2 : 5) : (ks <= 21 ? (ksplit ? 2 : 7) : (ks <= 31 ? (ksplit ? 4 : 16) : (ks <= 49 ? 10 : 11)));
        pl.targ[0] = nk; pl.targ[1] = ksplit; pl.targ[2] = maxr; pl.targ[3] = maxt;
        pl.block = 256; pl.lds = lds; pl.P = P; pl.spw = spw;
        grid_3d(pl, ntx, nty, nchunk, B, C);
        return 0;
    }
    if (ks != 3 && ks != 5 && ks != 7 && ks != 9 && ks != 11 && ks != 13 && ks != 15 && ks != 21) {
        // generic kernel: no magic multipliers, all slices in one workgroup
        pl.family = ConvFamily::generic;
        pl.block = 256;
        pl.lds = ((size_t)(kConvTile + ks - 1) * (kConvTile + ks - 1) + (size_t)ks * ks) * sizeof(float);
        pl.ntx = ntx; pl.nty = nty; pl.nchunk = 1;
        pl.gx = (unsigned)(ntx * grid); pl.gy = (unsigned)(nty * grid); pl.gz = (unsigned)(B * C);
        return 0;
    }
    // waves per workgroup = slices of one chunk (one slice per wave): least padding, at most 5
    int nw = 1, best = 1 << 30;
    const int maxnw = ks == 11 ? 5 : 4;
    for (int n = maxnw; n >= (S > 1 ? 2 : 1); --n) {      // larger n wins ties; a lone wave per tile only for S == 1
        if (ks != 11 && n == 3) continue;
        const int waste = (S + n - 1) / n * n - S;
        if (waste < best) { best = waste; nw = n; }
    }
    if (nenv && ks == 11) {
        const int v = atoi(nenv);
        if (v >= 1 && v <= maxnw) nw = v;
    }
    const int nchunk = (S + nw - 1) / nw;
    AADFF_CHECK_ARG((size_t)B * C * nchunk <= 65535, "render_psf_map: B*C*chunks too large");
    const bool use_mfma = ks <= 11 && !(penv && penv[0] == 'v');
    // stacks: slice-batched GEMM (the image is the shared operand); "toeplitz" / "valu" force the older paths
    if (ks == 11 && S >= 3 && !penv) {
        // paired bands (default): a workgroup renders two consecutive bands of its patch, the second one prefetched by LDS-DMA
        // AADFF_CONV_PAIR: 0 = one band per workgroup (round-2 form), N >= 1 = bands in pairs for every N-th (patch, plane)
        const int pv = qenv ? atoi(qenv) : AADFF_CONV_PAIR_DEFAULT;   // read per launch: tests switch it
        const int pair_mod = pv < 0 ? 0 : pv;
        if (int rc = plan_sbatch(pl, "render_psf_map", S, pair_mod > 0, false, B, C, mh, mw)) return rc;
        AADFF_CHECK_ARG((size_t)H * W <= ((size_t)1 << 27) && 16 * (size_t)ss + 4 * (size_t)H * W < ((size_t)1 << 32),
                        "render_psf_map: image planes above 2^27 pixels / slice strides above 2^28 elements are not supported on the stack path");
        static const int stagger = [] { const char* e = getenv("AADFF_CONV_STAGGER"); const int v = e ? atoi(e) : 1; return v < 0 ? 0 : (v > 64 ? 64 : v); }();   // default 1: -1 % in bench, -7 % back to back
        pl.stagger = stagger; pl.pair_mod = pair_mod;
        // aadff_time_next_launch: the two events ride ON this dispatch (kernel begin / end timestamps)
        pl.attach = true;
        return 0;
    }
    if (ks == 9 || ks == 11) {
        // lone slices (render_psf_map / render_psf as the reference calls them) and pairs: block-GEMM form, 21 instead of 33
        // MFMAs per 256 outputs and the slice-batched kernel's staging; AADFF_CONV_PATH = toeplitz / valu force the older paths
        // S == 1 only - measured (tools/conv_paths_bench.py, 1024^2, us): ks 11: S = 1 14.5-16.6 against 19.3-19.8 Toeplitz, S = 2
        // 23.2 / 23.0 (re-staging per slice cancels the gain; a form that renders three slices from one staged band was built
        // and was no faster: 23.0 / 28.9 for S = 2 / 3); ks 9: S = 1 14.5 / 18.5, S = 2 23.8 / 21.0, S = 10 86 / 72-78
        if (S == 1 && B * C <= 65535 && !penv && (size_t)H * W <= ((size_t)1 << 30)) {
            const int bntx = (mw + kConvBandCols - 1) / kConvBandCols, bnty = (mh + kConvBlkRows - 1) / kConvBlkRows;
            const size_t gx = (size_t)bntx * grid, gy = (size_t)bnty * grid, total = gx * gy * B * C * S;
            if (total < ((size_t)1 << 31)) {
                pl.family = ConvFamily::blk;
                pl.targ[0] = ks; pl.targ[1] = 0;
                pl.block = 64 * kConvBlkWaves;
                grid_xcd(pl, bntx, bnty, gx, gy, total, C, S);
                return 0;
            }
        }
    }
    if (use_mfma) {
        pl.family = ConvFamily::mfma;
        pl.targ[0] = ks; pl.targ[1] = nw; pl.targ[2] = AADFF_MFMA_SPW;
        pl.block = 64 * nw;
        grid_3d(pl, ntx, nty, (S + nw * AADFF_MFMA_SPW - 1) / (nw * AADFF_MFMA_SPW), B, C);
        return 0;
    }
    pl.family = ConvFamily::valu;
    pl.targ[0] = ks; pl.targ[1] = nw;
    pl.block = 64 * nw;
    grid_3d(pl, ntx, nty, nchunk, B, C);
    return 0;
}

void conv_plan_name(const ConvPlan& pl, char* buf, size_t len) {
    const int* t = pl.targ;
    const auto b = [](int v) { return v ? "true" : "false"; };
    switch (pl.family) {
        case ConvFamily::valu: snprintf(buf, len, "conv_psf_map_kernel<%d, %d>", t[0], t[1]); break;
        case ConvFamily::generic: snprintf(buf, len, "conv_psf_map_generic_kernel"); break;
        case ConvFamily::mfma: snprintf(buf, len, "conv_psf_map_mfma_kernel<%d, %d, %d>", t[0], t[1], t[2]); break;
        case ConvFamily::toeplitz_wide: snprintf(buf, len, "conv_psf_map_toeplitz_wide_kernel<%d, %s, %d, %d>", t[0], b(t[1]), t[2], t[3]); break;
        case ConvFamily::sbatch: snprintf(buf, len, "conv_psf_map_sbatch_kernel<%d, %d, %s, %s, %s>", t[0], t[1], b(t[2]), b(t[3]), b(t[4])); break;
        case ConvFamily::blk: snprintf(buf, len, "conv_psf_map_blk_kernel<%d, %s>", t[0], b(t[1])); break;
        case ConvFamily::blkw: snprintf(buf, len, "conv_psf_map_blkw_kernel<%d, %d>", t[0], t[1]); break;
    }
}

}  // namespace aadff

using namespace aadff;

extern "C" int aadff_conv_plan_describe(const char* entry, int B, int C, int S, int L, int H, int W, int grid, int ks, long stride_bc,
                                        long stride_s, char* name, int name_len, long long* info) {
    AADFF_CHECK_ARG(entry && name && name_len > 0 && info, "conv_plan_describe: NULL pointer");
    static const char* const names[] = {"map", "psf", "stack", "strided", "layered"};
    int e = 0;
    while (e < 5 && std::strcmp(entry, names[e]) != 0) ++e;
    AADFF_CHECK_ARG(e < 5, "conv_plan_describe: entry '%s' is none of map, psf, stack, strided, layered", entry);
    const ConvEntry en = (ConvEntry)e;
    // the entries' own argument conventions (conv.hip): one slice for map / psf, a 1 x 1 grid for psf, contiguous output unless strided
    if (en == ConvEntry::map || en == ConvEntry::psf) S = 1;
    if (en == ConvEntry::psf) grid = 1;
    if (en != ConvEntry::strided) { stride_s = (long)H * W; stride_bc = (long)S * stride_s; }
    ConvPlan pl;
    if (int rc = conv_plan(pl, en, true, B, C, S, L, H, W, grid, ks, stride_bc, stride_s)) return rc;
    conv_plan_name(pl, name, (size_t)name_len);
    info[0] = (long long)pl.gx * pl.gy * pl.gz;
    info[1] = pl.block;
    info[2] = (long long)pl.lds;
    info[3] = pl.spw;
    info[4] = pl.attach;
    return 0;
}
