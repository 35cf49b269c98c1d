// Backward of the blended PSF-map render for gfx950 (MI355X): gradients to the image and to the PSF maps, as closed forms in plain fp32.
// Semantics: include/aadff.h (aadff_render_psf_map_blend_stack_bwd); design, operation order and measurements: DESIGN.md 4.19.
//
// The forward is out = sum over nodes (i, j) of Hy_i(y) Hx_j(x) R(i,j)[y, x], with Hy_i the HAT of node i: 1 - fy on the rows of cell i,
// fy on the rows of cell i - 1 (both when g == 1: the one node has weight 1), 0 elsewhere.  fy, fx are blend_frac of the forward
// (blend_axis.h), 1 - fy is __fsub_rn(1, fy) as there.  Both gradients are those of the patch convolution (conv_bwd.hip) with dy
// weighted by the hat of the node instead of masked to a patch.  Every sum has a fixed order, no float atomics, every output element is
// written exactly once: bit-reproducible.  No per-pixel PSF is formed.
#include <algorithm>
#include "blend_axis.h"

namespace aadff {

// ------------------------------------------------------------------------------------
// (1) d_img.  In image coordinates (U, V) = padded position minus p, with T_ij = dy * (Hy_i Hx_j) (zero outside the image):
//   g_ij(U, V) = sum_{a, e < ks} T_ij[U + a - p][V + e - p] * psf_ij[a][e]
//   d_img[y][x] = sum_s sum_{nodes (i,j)} { g_ij(y, x) + g_ij at the mirror images of (y, x) under the reflect padding } (up to 3 x 3 positions).
// Workgroup = one 32 x 32 tile of one (b, c) plane, all S slices.  The hats come from per-row / per-column tables (cell, fy, 1 - fy) of
// the dy window (tile + p halo), built once per workgroup with the forward's blend_frac; only the nodes whose hat support meets the
// window are visited (a window inside one cell: its four corners, the forward's four FMAs per tap).  T_ij = fl(dy * fl(Hy_i * Hx_j)) is
// staged in LDS, zero outside the image, and the taps of PSF tile (i, j) run over it with wave-uniform weights (scalar loads, SGPR
// operands).  The mirror images' sources lie inside the direct window, so they are read from the same T tile (border lanes only,
// per-lane weights): a mirror of row y is -y (1 <= y <= p) or 2 (H - 1) - y (H - 1 - p <= y <= H - 2), columns alike.
// ------------------------------------------------------------------------------------
struct HatTables {
    float *fy, *gy, *fx, *gx;                   // [TP] fy, 1 - fy of the window row; fx, 1 - fx of the window column
    int *ky, *kx;                               // [TP] cell of the window row / column, -2 outside the image
};
struct DimgWindow { int wy_lo, wy_hi, wx_lo, wx_hi, ci_lo, ci_hi, cj_lo, cj_hi; };

__device__ __forceinline__ DimgWindow dimg_window(const BlendCells& bc, int ncy, int ncx, int y0, int x0, int p, int H, int W) {
    DimgWindow w;
    w.wy_lo = max(y0 - p, 0); w.wy_hi = min(y0 + BT - 1 + p, H - 1);
    w.wx_lo = max(x0 - p, 0); w.wx_hi = min(x0 + BT - 1 + p, W - 1);
    w.ci_lo = cell_of_pixel(bc.y, ncy, w.wy_lo); w.ci_hi = cell_of_pixel(bc.y, ncy, w.wy_hi);
    w.cj_lo = cell_of_pixel(bc.x, ncx, w.wx_lo); w.cj_hi = cell_of_pixel(bc.x, ncx, w.wx_hi);
    return w;
}
// thread t < TP fills entry t of both axes: a uniform walk over the window's cells, the nodes as scalar operands
__device__ __forceinline__ void fill_hat_tables(const HatTables& h, const BlendCells& bc, const DimgWindow& w, int t, int y0, int x0, int p, int grid) {
    const bool single = grid == 1;
    const int yy = y0 - p + t, xx = x0 - p + t;
    h.ky[t] = -2; h.fy[t] = 0.f; h.gy[t] = 0.f;
    h.kx[t] = -2; h.fx[t] = 0.f; h.gx[t] = 0.f;
    for (int cc = w.ci_lo; cc <= w.ci_hi; ++cc) {
        const float n0 = bc.y.node[cc], n1 = bc.y.node[min(cc + 1, grid - 1)];
        if (yy >= bc.y.b[cc] && yy < bc.y.b[cc + 1]) {
            const float f = blend_frac(yy, n0, n1, single);
            h.ky[t] = cc; h.fy[t] = f; h.gy[t] = __fsub_rn(1.f, f);
        }
    }
    for (int cc = w.cj_lo; cc <= w.cj_hi; ++cc) {
        const float n0 = bc.x.node[cc], n1 = bc.x.node[min(cc + 1, grid - 1)];
        if (xx >= bc.x.b[cc] && xx < bc.x.b[cc + 1]) {
            const float f = blend_frac(xx, n0, n1, single);
            h.kx[t] = cc; h.fx[t] = f; h.gx[t] = __fsub_rn(1.f, f);
        }
    }
}
// does the hat of node i (the pixels of cells i - 1 and i) hold a pixel of [lo, hi]?
__device__ __forceinline__ bool hat_meets(const BlendAxis& a, int ncell, int i, int lo, int hi) {
    return max(a.b[max(i - 1, 0)], lo) < min(a.b[min(i + 1, ncell)], hi + 1);
}
__device__ __forceinline__ float hat_of(int k, float f, float g, int i, int grid) {
    return (k == i ? g : 0.f) + (min(k + 1, grid - 1) == i ? f : 0.f);
}
// the mirror terms of output (y, x) from the T tile of one node (pitch P, origin (y0 - p, x0 - p)): one zero-started fmaf chain per
// mirror position over its sources in row-major order, the chains added in the order of the positions
__device__ __forceinline__ float dimg_fold(const float* T, int P, const float* wp, int G, int y, int x, int y0, int x0, int p, int H, int W) {
    float fold = 0.f;
    for (int vu = 0; vu < 3; ++vu) {
        const int Uv = vu == 0 ? y : (vu == 1 ? -y : 2 * (H - 1) - y);
        if ((vu == 1 && !(y >= 1 && y <= p)) || (vu == 2 && !(y <= H - 2 && y >= H - 1 - p))) continue;
        const int r_lo = max(Uv - p, 0), r_hi = min(Uv + p, H - 1);
        for (int vv = 0; vv < 3; ++vv) {
            const int Vv = vv == 0 ? x : (vv == 1 ? -x : 2 * (W - 1) - x);
            if ((vv == 1 && !(x >= 1 && x <= p)) || (vv == 2 && !(x <= W - 2 && x >= W - 1 - p))) continue;
            if (vu == 0 && vv == 0) continue;
            const int c_lo = max(Vv - p, 0), c_hi = min(Vv + p, W - 1);
            float m = 0.f;
            for (int r = r_lo; r <= r_hi; ++r)
                for (int cc = c_lo; cc <= c_hi; ++cc)
                    m = __fmaf_rn(T[(r - (y0 - p)) * P + cc - (x0 - p)], wp[(size_t)(p + r - Uv) * G + p + cc - Vv], m);
            fold = __fadd_rn(fold, m);
        }
    }
    return fold;
}

// Templated sizes (ks 3 .. 15, 21).  Lane = 4 x 4 outputs (the forward's layout: columns 4q .. 4q+3, rows 4k .. 4k+3), so ONE wave covers
// the tile; the four waves take the (slice, node) pairs p = wave, wave + 4, ... of the enumeration s-major, then i, then j over the visited
// nodes, each in a T tile of its own (pitch rule of BlendCfg: ds_read_b128 rows on disjoint bank quarters).  Per pair the taps run in
// blocks of four tap rows (dimg_tap_block): 7 input rows read for 64 KS FMAs per lane, the taps as scalar operands.
// A mirror image is one more PASS of the same code: g(-y, V) is the correlation of the row-flipped T with the row-flipped PSF at y, so a
// tile that holds outputs with a mirror image runs its pairs once per mirror position (edge tiles twice, corner tiles four times, up to
// nine when H or W barely exceeds p) with T staged through the mirror and the taps read backwards; pass index fastest in the
// enumeration, order (0, -y, 2 (H - 1) - y) x (0, -x, 2 (W - 1) - x) over the positions the tile has.
// Sums, per element: per (pair, pass) a zero-started chain of KS^2 fmaf in the pass's row-major tap order, added to the wave's total in
// the order of its passes (only where the element has that mirror image); the four waves' totals as ((w0 + w1) + w2) + w3 through LDS.
template <int KS>
struct DimgCfg {
    static constexpr int PAD = KS / 2;
    static constexpr int TP = BT + KS - 1;                       // staged rows and columns
    static constexpr int NIN = 4 + KS - 1, NV = (NIN + 3) / 4;   // inputs a lane needs per row, ds_read_b128 per row
    static constexpr int need = (BT / 4 - 1) * 4 + 4 * NV;
    static constexpr int P = (((need > TP ? need : TP) - 8 + 15) / 16) * 16 + 8;
};

// NB consecutive tap rows a0 .. a0 + NB - 1 over the lane's 4 x 4 outputs: the NB x KS taps are wave-uniform scalar loads (one batch in
// front of the block, as in conv_blend_kernel), each of the NB + 3 input rows is read once and feeds the output rows r with tap row
// b = t - r.  Per output the order is (a, e) ascending: the row-major chain.  wrow points at tap (a0, 0) of the pass; rs, cs are the
// strides of a tap row and a tap column in the map (G, 1; negative on a mirrored axis, where the pass runs the PSF backwards).
template <int KS, int NB, int NV>
__device__ __forceinline__ void dimg_tap_block(float (&acc)[4][4], const float* trow, int P, const float* wrow, int rs, int cs) {
    float m[NB][KS];                                            // wave-uniform: scalar registers
#pragma unroll
    for (int b = 0; b < NB; ++b)
#pragma unroll
        for (int e = 0; e < KS; ++e) m[b][e] = wrow[b * rs + e * cs];
#pragma unroll
    for (int t = 0; t < NB + 3; ++t) {
        float in[4 * NV];
        const float4* ap = reinterpret_cast<const float4*>(trow + t * P);
#pragma unroll
        for (int v = 0; v < NV; ++v) {
            const float4 f4 = ap[v];
            in[4 * v] = f4.x; in[4 * v + 1] = f4.y; in[4 * v + 2] = f4.z; in[4 * v + 3] = f4.w;
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const int b = t - r;
            if (b >= 0 && b < NB) {
#pragma unroll
                for (int e = 0; e < KS; ++e)
#pragma unroll
                    for (int i = 0; i < 4; ++i) acc[r][i] = __fmaf_rn(in[i + e], m[b][e], acc[r][i]);
            }
        }
    }
}

template <int KS>
__global__ __launch_bounds__(256) void blend_dimg_kernel(const float* __restrict__ psf, const float* __restrict__ dy, float* __restrict__ dimg,
                                                         int C, int S, int H, int W, int grid, int ncy, int ncx, BlendCells bc) {
    using Cfg = DimgCfg<KS>;
    constexpr int P = Cfg::P, TP = Cfg::TP, p = Cfg::PAD;
    static_assert(TP <= kWave, "staging maps one tile column to one lane");
    static_assert(TP * P >= BT * BT, "the T tiles double as the buffer of the last reduction");
    __shared__ __attribute__((aligned(16))) float tiles[4][TP * P];
    __shared__ float tab_f[4][TP];
    __shared__ int tab_k[2][TP];
    __shared__ int ilist[AADFF_MAX_GRID], jlist[AADFF_MAX_GRID], counts[2];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int plane_i = blockIdx.z, c = plane_i % C;
    const int x0 = blockIdx.x * BT, y0 = blockIdx.y * BT;
    const int G = grid * KS;
    const DimgWindow w = dimg_window(bc, ncy, ncx, y0, x0, p, H, W);
    const HatTables h{tab_f[0], tab_f[1], tab_f[2], tab_f[3], tab_k[0], tab_k[1]};
    if (tid < TP) fill_hat_tables(h, bc, w, tid, y0, x0, p, grid);
    if (tid == 64) {                                            // the visited nodes of each axis
        int n = 0;
        for (int i = w.ci_lo; i <= min(w.ci_hi + 1, grid - 1); ++i)
            if (hat_meets(bc.y, ncy, i, w.wy_lo, w.wy_hi)) ilist[n++] = i;
        counts[0] = n;
        n = 0;
        for (int j = w.cj_lo; j <= min(w.cj_hi + 1, grid - 1); ++j)
            if (hat_meets(bc.x, ncx, j, w.wx_lo, w.wx_hi)) jlist[n++] = j;
        counts[1] = n;
    }
    __syncthreads();
    const int NJ = __builtin_amdgcn_readfirstlane(counts[1]), NN = __builtin_amdgcn_readfirstlane(counts[0]) * NJ;
    // the mirror passes of this tile: 0 = the position itself, 1 = the mirror -y (outputs 1 <= y <= p), 2 = the mirror 2 (H - 1) - y
    // (outputs H - 1 - p <= y <= H - 2); a pass exists where the tile holds such an output.  Columns alike.
    const int ty_hi = min(y0 + BT - 1, H - 1), tx_hi = min(x0 + BT - 1, W - 1);
    const bool top = p > 0 && y0 <= p && ty_hi >= 1, bot = p > 0 && y0 <= H - 2 && ty_hi >= H - 1 - p;
    const bool lef = p > 0 && x0 <= p && tx_hi >= 1, rig = p > 0 && x0 <= W - 2 && tx_hi >= W - 1 - p;
    const int nmy = 1 + top + bot, nmx = 1 + lef + rig, NM = nmy * nmx, NP = S * NN * NM;

    const int q = lane % 8, k = lane / 8;
    const int x = x0 + 4 * q, yb = y0 + 4 * k;
    float* T = tiles[wave];
    const float* trow = T + (4 * k) * P + 4 * q;

    float tot[4][4];
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int i = 0; i < 4; ++i) tot[r][i] = 0.f;

    for (int it = 0; it * 4 < NP; ++it) {
        const int pq = it * 4 + wave;
        const bool have = pq < NP;
        const int pn = have ? pq / NM : 0, mm = have ? pq - pn * NM : 0;
        const int s = pn / NN, n = pn - s * NN;
        const int ii = n / NJ, i = __builtin_amdgcn_readfirstlane(ilist[ii]), j = __builtin_amdgcn_readfirstlane(jlist[n - ii * NJ]);
        const int iy = mm / nmx, ix = mm - iy * nmx;
        const int my = iy == 0 ? 0 : (iy == 1 && top ? 1 : 2), mx = ix == 0 ? 0 : (ix == 1 && lef ? 1 : 2);
        const float* wp = psf + ((size_t)(s * C + c) * G + i * KS) * G + j * KS;
        if (have) {     // stage T_ij of slice s as the pass sees it: position Y holds the source Y, -Y or 2 (H - 1) - Y; zero where that is
                        // outside the image or outside the window (such a source feeds no output of the pass).  Column = lane, every load in
                        // flight before the first LDS write.
            const float* dyp = dy + ((size_t)plane_i * S + s) * H * W;
            const int X = x0 - p + lane, xs = mx == 0 ? X : (mx == 1 ? -X : 2 * (W - 1) - X), tc = xs - (x0 - p);
            const bool scol = lane < TP && xs >= 0 && xs < W && tc >= 0 && tc < TP;
            const int tcc = scol ? tc : 0;
            const float hx = scol ? hat_of(h.kx[tcc], h.fx[tcc], h.gx[tcc], j, grid) : 0.f;
            float v[TP];
#pragma unroll
            for (int r = 0; r < TP; ++r) {
                const int Y = y0 - p + r, ys = my == 0 ? Y : (my == 1 ? -Y : 2 * (H - 1) - Y), tr = ys - (y0 - p);
                v[r] = (scol && ys >= 0 && ys < H && tr >= 0 && tr < TP) ? dyp[(size_t)ys * W + xs] : 0.f;
            }
#pragma unroll
            for (int r = 0; r < TP; ++r) {
                const int Y = y0 - p + r, ys = my == 0 ? Y : (my == 1 ? -Y : 2 * (H - 1) - Y), tr = min(max(ys - (y0 - p), 0), TP - 1);
                if (lane < TP) T[r * P + lane] = __fmul_rn(v[r], __fmul_rn(hat_of(h.ky[tr], h.fy[tr], h.gy[tr], i, grid), hx));
            }
        }
        __syncthreads();
        if (have) {
            float acc[4][4];
#pragma unroll
            for (int r = 0; r < 4; ++r)
#pragma unroll
                for (int m = 0; m < 4; ++m) acc[r][m] = 0.f;
            // blocks of four tap rows (a last one of KS % 4), the block loop not unrolled: its body is the forward's, 64 KS FMAs per lane
            const int rs = my == 0 ? G : -G, cs = mx == 0 ? 1 : -1;
            const float* w0 = wp + (my == 0 ? 0 : (KS - 1) * G) + (mx == 0 ? 0 : KS - 1);
#pragma unroll 1
            for (int a0 = 0; a0 + 4 <= KS; a0 += 4) dimg_tap_block<KS, 4, Cfg::NV>(acc, trow + a0 * P, P, w0 + a0 * rs, rs, cs);
            dimg_tap_block<KS, KS % 4, Cfg::NV>(acc, trow + (KS - KS % 4) * P, P, w0 + (KS - KS % 4) * rs, rs, cs);
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int y = yb + r;
                const bool oky = my == 0 ? true : (my == 1 ? (y >= 1 && y <= p) : (y <= H - 2 && y >= H - 1 - p));
#pragma unroll
                for (int m = 0; m < 4; ++m) {
                    const int xx = x + m;
                    const bool okx = mx == 0 ? true : (mx == 1 ? (xx >= 1 && xx <= p) : (xx <= W - 2 && xx >= W - 1 - p));
                    if (oky && okx) tot[r][m] = __fadd_rn(tot[r][m], acc[r][m]);
                }
            }
        }
        __syncthreads();
    }
    // the four waves' totals, in the order ((w0 + w1) + w2) + w3
#pragma unroll
    for (int r = 0; r < 4; ++r)
#pragma unroll
        for (int m = 0; m < 4; ++m) T[(4 * k + r) * BT + 4 * q + m] = tot[r][m];
    __syncthreads();
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const int e = tid + 256 * m, yy = y0 + (e >> 5), xx = x0 + (e & 31);
        const float v = __fadd_rn(__fadd_rn(__fadd_rn(tiles[0][e], tiles[1][e]), tiles[2][e]), tiles[3][e]);
        if (yy < H && xx < W) dimg[(size_t)plane_i * H * W + (size_t)yy * W + xx] = v;
    }
}

// Every other odd ks up to AADFF_MAX_KS: ks at run time, dynamic LDS.  Lane = column, 4 rows per thread (the layout of map_dimg_kernel);
// per slice the dy window is staged once and every visited node's T tile is built from it, one node after the other for the whole
// workgroup.  Sums, per element: a chain of ks fmaf per tap column e -> added to the slice's accumulator in the order (i, j, e), the
// node's mirror terms (dimg_fold) after its ks columns -> added over the slices.
__global__ __launch_bounds__(256) void blend_dimg_generic_kernel(const float* __restrict__ psf, const float* __restrict__ dy, float* __restrict__ dimg,
                                                                 int C, int S, int H, int W, int grid, int ks, int ncy, int ncx, BlendCells bc) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int p = ks / 2, TP = BT + 2 * p, G = grid * ks;
    float* win = smem;                          // [TP][TP] dy
    float* T = win + TP * TP;                   // [TP][TP] dy * hat of the current node
    float* tf = T + TP * TP;
    const HatTables h{tf, tf + TP, tf + 2 * TP, tf + 3 * TP, reinterpret_cast<int*>(tf + 4 * TP), reinterpret_cast<int*>(tf + 5 * TP)};

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lx = lane & 31, lyg = wave * 2 + (lane >> 5);
    const int plane_i = blockIdx.z, c = plane_i % C;
    const int x0 = blockIdx.x * BT, y0 = blockIdx.y * BT;
    const int x = x0 + lx, yb = y0 + 4 * lyg;
    const DimgWindow w = dimg_window(bc, ncy, ncx, y0, x0, p, H, W);
    if (tid < TP) fill_hat_tables(h, bc, w, tid, y0, x0, p, grid);
    const bool border = x <= p || x >= W - 1 - p || yb <= p || yb + 3 >= H - 1 - p;
    const int i_hi = min(w.ci_hi + 1, grid - 1), j_hi = min(w.cj_hi + 1, grid - 1);

    float total[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
        const float* dyp = dy + ((size_t)plane_i * S + s) * H * W;
        __syncthreads();                                        // the tables are written; the last node's T and win are read
        for (int e = tid; e < TP * TP; e += 256) {
            const int r = e / TP, cc = e - r * TP;
            const int yy = y0 - p + r, xx = x0 - p + cc;
            win[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? dyp[(size_t)yy * W + xx] : 0.f;
        }
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int i = w.ci_lo; i <= i_hi; ++i) {
            if (!hat_meets(bc.y, ncy, i, w.wy_lo, w.wy_hi)) continue;
            for (int j = w.cj_lo; j <= j_hi; ++j) {
                if (!hat_meets(bc.x, ncx, j, w.wx_lo, w.wx_hi)) continue;
                __syncthreads();                                // win is staged; the previous node's T is read
                for (int e = tid; e < TP * TP; e += 256) {
                    const int r = e / TP, cc = e - r * TP;
                    T[e] = __fmul_rn(win[e], __fmul_rn(hat_of(h.ky[r], h.fy[r], h.gy[r], i, grid), hat_of(h.kx[cc], h.fx[cc], h.gx[cc], j, grid)));
                }
                __syncthreads();
                const float* wp = psf + ((size_t)(s * C + c) * G + i * ks) * G + j * ks;
                // source row of output row yb + k and tap row a is yb + k + a - p = tile row 4 lyg + k + a
                const float* trow = T + (4 * lyg) * TP + lx;
#pragma unroll 1
                for (int e = 0; e < ks; ++e) {
                    float part[4] = {0.f, 0.f, 0.f, 0.f};
                    for (int a = 0; a < ks; ++a) {
                        const float wv = wp[(size_t)a * G + e];
#pragma unroll
                        for (int k = 0; k < 4; ++k) part[k] = __fmaf_rn(trow[(a + k) * TP + e], wv, part[k]);
                    }
#pragma unroll
                    for (int k = 0; k < 4; ++k) acc[k] = __fadd_rn(acc[k], part[k]);
                }
                if (border) {
#pragma unroll 1
                    for (int k = 0; k < 4; ++k)
                        if (yb + k < H && x < W) acc[k] = __fadd_rn(acc[k], dimg_fold(T, TP, wp, G, yb + k, x, y0, x0, p, H, W));
                }
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) total[k] = __fadd_rn(total[k], acc[k]);
    }
    if (x < W) {
        float* o = dimg + (size_t)plane_i * H * W + x;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (yb + k < H) o[(size_t)(yb + k) * W] = total[k];
    }
}

// ------------------------------------------------------------------------------------
// (2) d_maps:  d_maps[s][c][i ks + a][j ks + e] = sum_b sum_{(y, x)} dy[b][c][s][y][x] Hy_i(y) Hx_j(x) img[b][c][refl(y + p - a)][refl(x + p - e)]
// First pass: the forward's cell decomposition.  Workgroup = one 32 x 32 tile of one cell and one (b, c) plane; inside a cell the four
// nodes with a non-zero hat are its corners, q = 0 .. 3 = (ci, cj), (ci, cj1), (ci1, cj), (ci1, cj1), with the forward's weights
// gy gx, gy fx, fy gx, fy fx.  The reflect-padded image window is staged once for all S slices; per slice the four weighted dy tiles
// fl(dy * fl(wy * wx)) (zero outside the cell).  Wave w takes the units (q, a, tap block) w, w + 4, ...; a lane owns 4 x 4 pixels and EB
// taps of the row at a time (the loop of map_dpsf_partial_kernel).  Sums: 16 fmaf per lane -> wave butterfly -> one partial per
// (b, tile, s, c, q) in the workspace.  Second pass: per node the partials of the corners that ARE this node, over the at most 2 x 2 cells
// around it and over b, in a fixed order.  EB = ks for the templated sizes, 1 for any ks.
// ------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(256) void blend_dmaps_partial_kernel(const float* __restrict__ img, const float* __restrict__ dy, float* __restrict__ part,
                                                                  int C, int S, int H, int W, int grid, int ks_rt, int ncy, int ncx, BlendCells bc) {
    constexpr int EB = KS > 0 ? KS : 1;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ks = KS > 0 ? KS : ks_rt, p = ks / 2, TP = BT + 2 * p, kk = ks * ks;
    float* tdy = smem;                      // [4][32][32]
    float* timg = smem + 4 * BT * BT;       // [TP][TP]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cj = cell_of_tile(bc.x, ncx, blockIdx.x), ci = cell_of_tile(bc.y, ncy, blockIdx.y);
    const int x0 = bc.x.b[cj] + ((int)blockIdx.x - bc.x.ts[cj]) * BT, y0 = bc.y.b[ci] + ((int)blockIdx.y - bc.y.ts[ci]) * BT;
    const int x_hi = bc.x.b[cj + 1], y_hi = bc.y.b[ci + 1];
    const int plane_i = blockIdx.z, c = plane_i % C;
    if (x0 >= x_hi || y0 >= y_hi) return;                       // (never: only non-empty tiles are enumerated)

    const float* plane = img + (size_t)plane_i * H * W;
    for (int e = tid; e < TP * TP; e += 256) {
        const int r = e / TP, cc = e - r * TP;
        timg[e] = plane[(size_t)reflect_idx(y0 - p + r, H) * W + reflect_idx(x0 - p + cc, W)];
    }
    // the weights of the four pixels this thread stages: column tid % 32, rows tid / 32 + 8 m
    const bool single = grid == 1;
    const int ci1 = min(ci + 1, grid - 1), cj1 = min(cj + 1, grid - 1);
    const int sx = x0 + (tid & 31);
    const float fx = blend_frac(sx, bc.x.node[cj], bc.x.node[cj1], single), gx = __fsub_rn(1.f, fx);
    float w4[4][4];
#pragma unroll
    for (int m = 0; m < 4; ++m) {
        const float fy = blend_frac(y0 + (tid >> 5) + 8 * m, bc.y.node[ci], bc.y.node[ci1], single), gy = __fsub_rn(1.f, fy);
        w4[m][0] = __fmul_rn(gy, gx); w4[m][1] = __fmul_rn(gy, fx); w4[m][2] = __fmul_rn(fy, gx); w4[m][3] = __fmul_rn(fy, fx);
    }

    const int lxg = lane & 7, lyr = lane >> 3;
    const int nblk = (ks + EB - 1) / EB, units = 4 * ks * nblk;
    const size_t slab = ((size_t)(plane_i / C) * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x;
    for (int s = 0; s < S; ++s) {
        const float* dyp = dy + ((size_t)plane_i * S + s) * H * W;
        __syncthreads();
#pragma unroll
        for (int m = 0; m < 4; ++m) {
            const int e = tid + 256 * m, y = y0 + (e >> 5);
            const float d = (y < y_hi && sx < x_hi) ? dyp[(size_t)y * W + sx] : 0.f;
#pragma unroll
            for (int q = 0; q < 4; ++q) tdy[q * BT * BT + e] = __fmul_rn(d, w4[m][q]);
        }
        __syncthreads();
        float* po = part + (((size_t)slab * S + s) * C + c) * 4 * kk;
        for (int u = wave; u < units; u += 4) {
            const int q = u / (ks * nblk), u2 = u - q * ks * nblk;
            const int a = u2 / nblk, e0 = (u2 - a * nblk) * EB;
            const float* td = tdy + q * BT * BT;
            float acc[EB];
#pragma unroll
            for (int m = 0; m < EB; ++m) acc[m] = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = lyr + 8 * j;
                const float4 d4 = *reinterpret_cast<const float4*>(td + row * BT + 4 * lxg);
                const float d[4] = {d4.x, d4.y, d4.z, d4.w};
                // pixel column 4 lxg + k and tap e0 + m read image column 4 lxg + k + 2p - e0 - m of the window
                const float* tr = timg + (row + 2 * p - a) * TP + 4 * lxg + 2 * p - e0 - (EB - 1);
                float v[EB + 3];
#pragma unroll
                for (int t = 0; t < EB + 3; ++t) v[t] = tr[t];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int m = 0; m < EB; ++m) acc[m] = __fmaf_rn(d[k], v[k + EB - 1 - m], acc[m]);
            }
            float mine = 0.f;
#pragma unroll
            for (int m = 0; m < EB; ++m) {
                const float t = wave_sum(acc[m]);
                if (lane == m) mine = t;
            }
            if (lane < EB && e0 + lane < ks) po[q * kk + a * ks + e0 + lane] = mine;
        }
    }
}

// second pass: workgroup = one node (i, j) of one (s, c), thread = tap (a, e).  Order: b { cell row { cell column { corner row { corner
// column { tile row { tile column } } } } } }, every level started at 0.  A node without a pixel under its hat gets exact zeros.
__global__ __launch_bounds__(256) void blend_dmaps_sum_kernel(const float* __restrict__ part, float* __restrict__ dmaps, int B, int C, int S, int grid,
                                                              int ks, int ncy, int ncx, int ntx, int nty, BlendCells bc) {
    const int kk = ks * ks, G = grid * ks;
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= kk) return;
    const int i = blockIdx.y / grid, j = blockIdx.y - i * grid;
    const int sc = blockIdx.z, s = sc / C, c = sc - s * C;
    float sum = 0.f;
    for (int b = 0; b < B; ++b) {
        float sb = 0.f;
        for (int ci = max(i - 1, 0); ci <= min(i, ncy - 1); ++ci)
            for (int cj = max(j - 1, 0); cj <= min(j, ncx - 1); ++cj)
                for (int qy = 0; qy < 2; ++qy) {
                    if ((qy ? min(ci + 1, grid - 1) : ci) != i) continue;
                    for (int qx = 0; qx < 2; ++qx) {
                        if ((qx ? min(cj + 1, grid - 1) : cj) != j) continue;
                        float scell = 0.f;
                        for (int ty = bc.y.ts[ci]; ty < bc.y.ts[ci + 1]; ++ty) {
                            float sr = 0.f;
                            for (int tx = bc.x.ts[cj]; tx < bc.x.ts[cj + 1]; ++tx) {
                                const size_t slab = ((size_t)b * nty + ty) * ntx + tx;
                                sr = __fadd_rn(sr, part[((((size_t)slab * S + s) * C + c) * 4 + 2 * qy + qx) * kk + t]);
                            }
                            scell = __fadd_rn(scell, sr);
                        }
                        sb = __fadd_rn(sb, scell);
                    }
                }
        sum = __fadd_rn(sum, sb);
    }
    const int a = t / ks, e = t - a * ks;
    dmaps[((size_t)sc * G + i * ks + a) * G + j * ks + e] = sum;
}

// an upper bound of the tiles of one axis that holds for any nodes: sum over the m <= min(ncell, n) non-empty cells of ceil(len / 32) with
// the lengths adding up to n is at most (n + 31 m) / 32
static size_t max_tiles(int n, int grid) {
    const int ncell = grid > 1 ? grid - 1 : 1;
    return ((size_t)n + (size_t)(BT - 1) * std::min(ncell, n)) / BT;
}

static size_t blend_bwd_ws_bytes(int B, int C, int S, int H, int W, int grid, int ks) {
    return (size_t)B * max_tiles(H, grid) * max_tiles(W, grid) * S * C * 4 * ks * ks * sizeof(float);
}

}  // namespace aadff

using namespace aadff;

extern "C" {

size_t aadff_render_psf_map_blend_stack_bwd_workspace(int B, int C, int S, int H, int W, int grid, int ks) {
    if (blend_check_shape(B, C, S, H, W, grid, ks)) return 0;
    return blend_bwd_ws_bytes(B, C, S, H, W, grid, ks);
}

int aadff_render_psf_map_blend_stack_bwd(const float* img, const float* psf_maps, const float* dy, float* d_img_or_null, float* d_maps_or_null,
                                         void* workspace, size_t workspace_bytes, const float* node_y, const float* node_x, int B, int C, int S,
                                         int H, int W, int grid, int ks, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && psf_maps && dy && node_y && node_x, "render_psf_map_blend_stack_bwd: NULL pointer (img, psf_maps, dy, node_y, node_x)");
    AADFF_CHECK_ARG(d_img_or_null || d_maps_or_null, "render_psf_map_blend_stack_bwd: d_img and d_maps are both NULL");
    if (int rc = blend_check_shape(B, C, S, H, W, grid, ks)) return rc;
    if (int rc = check_nodes(node_y, grid, "node_y")) return rc;
    if (int rc = check_nodes(node_x, grid, "node_x")) return rc;
    AADFF_CHECK_ARG((size_t)S * C <= 65535, "render_psf_map_blend_stack_bwd: S*C too large");
    const size_t need = blend_bwd_ws_bytes(B, C, S, H, W, grid, ks);
    if (d_maps_or_null)
        AADFF_CHECK_ARG(workspace && workspace_bytes >= need, "render_psf_map_blend_stack_bwd: workspace of %zu bytes is too small, d_maps needs %zu",
                        workspace ? workspace_bytes : (size_t)0, need);

    BlendCells bc;
    std::memset(&bc, 0, sizeof(bc));
    const int nty = fill_axis(bc.y, node_y, grid, H), ntx = fill_axis(bc.x, node_x, grid, W);
    const int ncell = grid > 1 ? grid - 1 : 1;
    hipStream_t st = (hipStream_t)stream;
    const int TP = BT + ks - 1;
#define AADFF_BLEND_SIZES(X) X(3) X(5) X(7) X(9) X(11) X(13) X(15) X(21)
    if (d_img_or_null) {
        dim3 g((W + BT - 1) / BT, (H + BT - 1) / BT, B * C);
        const size_t lds = ((size_t)2 * TP * TP + 6 * TP) * sizeof(float);
        switch (ks) {
#define AADFF_CASE(K) case K: hipLaunchKernelGGL((blend_dimg_kernel<K>), g, dim3(256), 0, st, psf_maps, dy, d_img_or_null, C, S, H, W, grid, ncell, ncell, bc); break;
            AADFF_BLEND_SIZES(AADFF_CASE)
#undef AADFF_CASE
            default: hipLaunchKernelGGL(blend_dimg_generic_kernel, g, dim3(256), lds, st, psf_maps, dy, d_img_or_null, C, S, H, W, grid, ks, ncell, ncell, bc);
        }
        AADFF_CHECK_LAUNCH();
    }
    if (d_maps_or_null) {
        dim3 g(ntx, nty, B * C);
        const size_t lds = ((size_t)4 * BT * BT + (size_t)TP * TP) * sizeof(float);
        float* part = static_cast<float*>(workspace);
        switch (ks) {
#define AADFF_CASE(K) case K: hipLaunchKernelGGL((blend_dmaps_partial_kernel<K>), g, dim3(256), lds, st, img, dy, part, C, S, H, W, grid, ks, ncell, ncell, bc); break;
            AADFF_BLEND_SIZES(AADFF_CASE)
#undef AADFF_CASE
            default: hipLaunchKernelGGL((blend_dmaps_partial_kernel<0>), g, dim3(256), lds, st, img, dy, part, C, S, H, W, grid, ks, ncell, ncell, bc);
        }
        AADFF_CHECK_LAUNCH();
        dim3 g2((ks * ks + 255) / 256, grid * grid, S * C);
        hipLaunchKernelGGL(blend_dmaps_sum_kernel, g2, dim3(256), 0, st, part, d_maps_or_null, B, C, S, grid, ks, ncell, ncell, ntx, nty, bc);
        AADFF_CHECK_LAUNCH();
    }
#undef AADFF_BLEND_SIZES
    return 0;
}

}  // extern "C"
