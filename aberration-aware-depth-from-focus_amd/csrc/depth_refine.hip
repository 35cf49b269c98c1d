// Confidence-guided depth refinement: one iteration of a confidence-weighted joint bilateral filter of u [N,1,H,W]
// (in practice 1 / depth) with confidence c [N,1,H,W], guided by g [N,C,H,W] (the all-in-focus image), over the (2r+1)^2 window
// clipped to the image:
//
//   w(p,q) = expf(max(-((dy^2 + dx^2) ks + sum_ch (g(p) - g(q))^2 kr), -64)),   c(q) < 2^-30 counts as 0,
//   A = sum w c(q) u(q),  D = sum w c(q)  (taps with c(q) = 0 are skipped: their u may be anything),  Wn = sum w,
//   u'(p) = A / D where D > 0, else u(p) bit for bit;   c'(p) = D / Wn.
//
//   stencil<RB, C, false>  forward.  A workgroup owns a 16 x 64 tile of pixels; the C planes of g, c u and c of the tile and a halo of
//                          r are put into LDS once (cells outside the image carry c = -1: such a tap does not exist).  A wave owns four
//                          rows of the tile, a lane one column of them: its four pixels lie below one another, so a tap read from LDS
//                          serves up to four pixels, and neighbouring lanes read neighbouring words.
//                          A row of cells lies in the windows of a fixed range of the four pixels, so the row runs with that
//                          range as a template argument (sweep): no branch between the pixels, whose exponentials overlap.
//   stencil<RB, C, true>   first pass of the backward: the same sums again (nothing of the forward is kept), then, for the cotangents
//                          gu', gc':  alpha = gu' / D (0 where D = 0),  u' (0 where D = 0),  beta = gc' / Wn  and the pass-through
//                          term  [D = 0] gu'  into four planes of the caller's workspace.
//   gather<RB, C>          second pass: the same tile with alpha, u' and beta in LDS (zero outside the image);
//                          d_u(q) = c(q) sum_p w alpha(p) + [D(q) = 0] gu'(q),   d_c(q) = sum_p w (alpha(p) (u(q) - u'(p)) + beta(p)).
//                          The window is symmetric and clipped symmetrically, so the pixels p that read q are the window of q.
// Both passes are gathers: no atomics, every output is the same bits from run to run, and d_u does not depend on whether d_c is
// asked for.  The weight is one function of the two guide pixels used by all three kernels; it is symmetric bit for bit.
// RB bounds r (4 or 8) and with C sizes the LDS tile; r itself is a kernel argument.
#include "common.h"

namespace aadff {
namespace rf {

constexpr int NT = 256;
constexpr int TW = 64, TH = 16;                               // pixels of a workgroup's tile
constexpr int PPT = TH / (NT / TW);                           // rows of a wave = pixels of a thread: 4
constexpr float CMIN = 0x1p-30f;                              // a confidence below this is zero

struct Args {
    const float* u;
    const float* c;
    const float* g;
    float* u_out;                                             // forward
    float* c_out;
    const float* gu;                                          // backward: the cotangents of u' and c'
    const float* gc;
    float* work;                                              // backward: alpha, u', beta, pass-through: four planes [N,H,W]
    float* d_u;                                               // or NULL
    float* d_c;                                               // or NULL
    int N, H, W, r, tx, ty;                                   // tx, ty: tiles per image
    float ks, kr;
};

template <int C>
__device__ __forceinline__ float weight(const float (&a)[C], const float (&b)[C], float space, float kr) {
    float s = 0.f;
#pragma unroll
    for (int ch = 0; ch < C; ++ch) {
        const float d = a[ch] - b[ch];
        s = fmaf(d, d, s);
    }
    return expf(fmaxf(-fmaf(s, kr, space), -64.f));
}

// the workgroup's tile origin and image
struct Tile {
    unsigned n;
    int x0, y0;
};

__device__ __forceinline__ Tile tile_of(const Args& A) {
    const unsigned per = (unsigned)A.tx * (unsigned)A.ty;
    const unsigned n = blockIdx.x / per, rem = blockIdx.x % per;
    Tile T;
    T.n = n, T.x0 = (int)(rem % (unsigned)A.tx) * TW, T.y0 = (int)(rem / (unsigned)A.tx) * TH;
    return T;
}

// The sweep of a lane over the cells of its four windows.  LDS row row0 + ry of the tile is row dy = ry - r - j of pixel j's window,
// inside it for j in [max(0, ry - 2r), min(PPT - 1, ry)].  That range is one of seven and constant along a row, so a row runs with
// the range as a template argument: no branch between the pixels of a lane, whose exponentials then overlap.  Per pixel the taps
// come in the order rows, then columns.  B::load reads a cell's words from LDS, B::tap adds the cell to pixel j.
template <class B, int JLO, int JHI>
__device__ __forceinline__ void sweep_row(B& b, const float* rowp, int plane, int r, int ry) {
#pragma unroll 2
    for (int dx = -r; dx <= r; ++dx) {
        b.load(rowp, plane, dx);
#pragma unroll
        for (int j = JLO; j <= JHI; ++j) {
            const int dy = ry - r - j;
            b.tap(j, (float)(dy * dy + dx * dx));
        }
    }
}

template <class B>
__device__ __forceinline__ void sweep(B& b, const float* first, int tw, int plane, int r) {
    for (int ry = 0; ry < 2 * r + PPT; ++ry) {
        const float* rowp = first + ry * tw;
        const int jlo = max(0, ry - 2 * r), jhi = min(PPT - 1, ry);
        if (jlo == 0 && jhi == 3) sweep_row<B, 0, 3>(b, rowp, plane, r, ry);
        else if (jlo == 0 && jhi == 0) sweep_row<B, 0, 0>(b, rowp, plane, r, ry);
        else if (jlo == 0 && jhi == 1) sweep_row<B, 0, 1>(b, rowp, plane, r, ry);
        else if (jlo == 0) sweep_row<B, 0, 2>(b, rowp, plane, r, ry);
        else if (jlo == 1) sweep_row<B, 1, 3>(b, rowp, plane, r, ry);
        else if (jlo == 2) sweep_row<B, 2, 3>(b, rowp, plane, r, ry);
        else sweep_row<B, 3, 3>(b, rowp, plane, r, ry);
    }
}
static_assert(PPT == 4, "sweep() lists the ranges of four pixels per lane");

// forward sums of a lane's four pixels
template <int C>
struct Sums {
    float gp[PPT][C], Aa[PPT], Dd[PPT], Wn[PPT];              // the pixels' guide values; A, D, Wn
    float gq[C], cu, cq, ks, kr;                              // the cell in hand
    __device__ __forceinline__ void load(const float* rowp, int plane, int dx) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) gq[ch] = rowp[ch * plane + dx];
        cu = rowp[C * plane + dx], cq = rowp[(C + 1) * plane + dx];
    }
    __device__ __forceinline__ void tap(int j, float d2) {
        const float w = weight<C>(gp[j], gq, d2 * ks, kr);
        const float we = cq >= 0.f ? w : 0.f;                 // a tap outside the image does not exist
        Wn[j] += we;
        Aa[j] = fmaf(we, cu, Aa[j]);
        Dd[j] = fmaf(we, cq, Dd[j]);
    }
};

// backward sums of a lane's four pixels q over the pixels p that read them
template <int C>
struct Grads {
    float gq[PPT][C], uq[PPT], S1[PPT], S2[PPT];
    float gp[C], al, uo, be, ks, kr;
    __device__ __forceinline__ void load(const float* rowp, int plane, int dx) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) gp[ch] = rowp[ch * plane + dx];
        al = rowp[C * plane + dx], uo = rowp[(C + 1) * plane + dx], be = rowp[(C + 2) * plane + dx];
    }
    __device__ __forceinline__ void tap(int j, float d2) {
        const float w = weight<C>(gp, gq[j], d2 * ks, kr);
        S1[j] = fmaf(w, al, S1[j]);
        S2[j] = fmaf(w, fmaf(al, uq[j] - uo, be), S2[j]);     // the difference first: exact where the two are close
    }
};

template <int RB, int C, bool PASS1>
__global__ __launch_bounds__(NT) void stencil(Args A) {
    __shared__ float sm[(C + 2) * (TH + 2 * RB) * (TW + 2 * RB)];   // g (C planes), c u, c; the rows are TW + 2 r long
    const int r = A.r, th = TH + 2 * r, tw = TW + 2 * r, plane = th * tw;
    const int lane = (int)threadIdx.x % TW, wv = (int)threadIdx.x / TW;
    const Tile T = tile_of(A);
    const size_t HW = (size_t)A.H * A.W;
    const float* up = A.u + (size_t)T.n * HW;
    const float* cp = A.c + (size_t)T.n * HW;
    const float* gp = A.g + (size_t)T.n * C * HW;
    float* sc = sm + C * plane;                               // c u, then c
    for (int ly = wv; ly < th; ly += NT / TW) {
        const int y = T.y0 - r + ly;
        for (int lx = lane; lx < tw; lx += TW) {
            const int x = T.x0 - r + lx, o = ly * tw + lx;
            const bool in = y >= 0 && y < A.H && x >= 0 && x < A.W;
            const size_t px = in ? (size_t)y * A.W + x : 0;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) sm[ch * plane + o] = in ? gp[(size_t)ch * HW + px] : 0.f;
            float cq = -1.f, cu = 0.f;
            if (in) {
                cq = cp[px];
                cq = cq >= CMIN ? cq : 0.f;                   // (a nan is zero too)
                cu = cq > 0.f ? cq * up[px] : 0.f;            // u under a zero confidence is never touched
            }
            sc[o] = cu, sc[plane + o] = cq;
        }
    }
    __syncthreads();
    const int x = T.x0 + lane;
    if (x >= A.W) return;

    const int row0 = wv * PPT;                                // tile row of the thread's first pixel; LDS row of pixel j: row0 + j + r
    Sums<C> S;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) S.gp[j][ch] = sm[ch * plane + (row0 + j + r) * tw + lane + r];
        S.Aa[j] = S.Dd[j] = S.Wn[j] = 0.f;
    }
    S.ks = A.ks, S.kr = A.kr;
    sweep(S, sm + row0 * tw + lane + r, tw, plane, r);
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int y = T.y0 + row0 + j;
        if (y >= A.H) break;
        const size_t px = (size_t)T.n * HW + (size_t)y * A.W + x;
        const bool some = S.Dd[j] > 0.f;
        if (!PASS1) {
            A.u_out[px] = some ? S.Aa[j] / S.Dd[j] : A.u[px];
            A.c_out[px] = S.Dd[j] / S.Wn[j];
        } else {
            const size_t NHW = (size_t)A.N * HW;
            const float gu = A.gu[px];
            const float al = some ? gu / S.Dd[j] : 0.f;
            A.work[px] = al;
            A.work[NHW + px] = some ? S.Aa[j] / S.Dd[j] : 0.f;
            A.work[2 * NHW + px] = A.gc[px] / S.Wn[j];
            A.work[3 * NHW + px] = some ? 0.f : gu;
        }
    }
}

template <int RB, int C>
__global__ __launch_bounds__(NT) void gather(Args A) {
    __shared__ float sm[(C + 3) * (TH + 2 * RB) * (TW + 2 * RB)];   // g (C planes), alpha, u', beta
    const int r = A.r, th = TH + 2 * r, tw = TW + 2 * r, plane = th * tw;
    const int lane = (int)threadIdx.x % TW, wv = (int)threadIdx.x / TW;
    const Tile T = tile_of(A);
    const size_t HW = (size_t)A.H * A.W, NHW = (size_t)A.N * HW;
    const float* gp = A.g + (size_t)T.n * C * HW;
    const float* wp = A.work + (size_t)T.n * HW;
    for (int ly = wv; ly < th; ly += NT / TW) {
        const int y = T.y0 - r + ly;
        for (int lx = lane; lx < tw; lx += TW) {
            const int x = T.x0 - r + lx, o = ly * tw + lx;
            const bool in = y >= 0 && y < A.H && x >= 0 && x < A.W;
            const size_t px = in ? (size_t)y * A.W + x : 0;
#pragma unroll
            for (int ch = 0; ch < C; ++ch) sm[ch * plane + o] = in ? gp[(size_t)ch * HW + px] : 0.f;
#pragma unroll
            for (int k = 0; k < 3; ++k) sm[(C + k) * plane + o] = in ? wp[(size_t)k * NHW + px] : 0.f;   // zero: no pixel there reads q
        }
    }
    __syncthreads();
    const int x = T.x0 + lane;
    if (x >= A.W) return;

    const int row0 = wv * PPT;
    Grads<C> G;
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
#pragma unroll
        for (int ch = 0; ch < C; ++ch) G.gq[j][ch] = sm[ch * plane + (row0 + j + r) * tw + lane + r];
        const int y = T.y0 + row0 + j;
        G.uq[j] = y < A.H ? A.u[(size_t)T.n * HW + (size_t)y * A.W + x] : 0.f;
        G.S1[j] = G.S2[j] = 0.f;
    }
    G.ks = A.ks, G.kr = A.kr;
    sweep(G, sm + row0 * tw + lane + r, tw, plane, r);
#pragma unroll
    for (int j = 0; j < PPT; ++j) {
        const int y = T.y0 + row0 + j;
        if (y >= A.H) break;
        const size_t px = (size_t)T.n * HW + (size_t)y * A.W + x;
        if (A.d_u) {
            float cq = A.c[px];
            cq = cq >= CMIN ? cq : 0.f;
            A.d_u[px] = (cq > 0.f ? cq * G.S1[j] : 0.f) + A.work[3 * NHW + px];
        }
        if (A.d_c) A.d_c[px] = G.S2[j];
    }
}

static int check(const char* who, const void* u, const void* c, const void* g, int N, int C, int H, int W, int radius, float ks, float kr,
                 Args& A, long& blocks) {
    AADFF_CHECK_ARG(u, "%s: u is NULL", who);
    AADFF_CHECK_ARG(c, "%s: c is NULL", who);
    AADFF_CHECK_ARG(g, "%s: g is NULL", who);
    AADFF_CHECK_ARG(C >= 1 && C <= 4, "%s: C = %d, the guide has 1 to 4 channels", who, C);
    AADFF_CHECK_ARG(radius >= 1 && radius <= 8, "%s: radius = %d is not in 1..8", who, radius);
    AADFF_CHECK_ARG(ks > 0.f && ks < INFINITY, "%s: ks = %g is not a positive number", who, (double)ks);
    AADFF_CHECK_ARG(kr > 0.f && kr < INFINITY, "%s: kr = %g is not a positive number", who, (double)kr);
    AADFF_CHECK_ARG(N > 0 && H > 0 && W > 0, "%s: N = %d, H = %d, W = %d must be positive", who, N, H, W);
    A.N = N, A.H = H, A.W = W, A.r = radius, A.ks = ks, A.kr = kr;
    A.tx = (W + TW - 1) / TW, A.ty = (H + TH - 1) / TH;
    blocks = (long)A.tx * A.ty * N;
    AADFF_CHECK_ARG((long)H * W < (1L << 31) - 8 && blocks < (1L << 31), "%s: N = %d, H = %d, W = %d are too large for one launch", who, N, H, W);
    return 0;
}

enum Kind { FORWARD, PASS1, GATHER };

template <int RB, int C>
static void launch(Kind k, const Args& A, long blocks, hipStream_t st) {
    const dim3 grid((unsigned)blocks), block(NT);
    if (k == FORWARD) hipLaunchKernelGGL((stencil<RB, C, false>), grid, block, 0, st, A);
    else if (k == PASS1) hipLaunchKernelGGL((stencil<RB, C, true>), grid, block, 0, st, A);
    else hipLaunchKernelGGL((gather<RB, C>), grid, block, 0, st, A);
}

template <int RB>
static void launch(Kind k, int C, const Args& A, long blocks, hipStream_t st) {
    switch (C) {
        case 1: launch<RB, 1>(k, A, blocks, st); break;
        case 2: launch<RB, 2>(k, A, blocks, st); break;
        case 3: launch<RB, 3>(k, A, blocks, st); break;
        default: launch<RB, 4>(k, A, blocks, st); break;
    }
}

static void launch(Kind k, int C, const Args& A, long blocks, hipStream_t st) {
    if (A.r <= 4) launch<4>(k, C, A, blocks, st);
    else launch<8>(k, C, A, blocks, st);
}

}  // namespace rf
}  // namespace aadff

using namespace aadff;

extern "C" int aadff_depth_refine_fwd(const float* u, const float* c, const float* g, float* u_out, float* c_out, int N, int C, int H, int W,
                                      int radius, float ks, float kr, aadff_stream_t stream) {
    rf::Args A = {};
    long blocks = 0;
    if (int rc = rf::check("depth_refine_fwd", u, c, g, N, C, H, W, radius, ks, kr, A, blocks)) return rc;
    AADFF_CHECK_ARG(u_out, "depth_refine_fwd: u_out is NULL");
    AADFF_CHECK_ARG(c_out, "depth_refine_fwd: c_out is NULL");
    AADFF_CHECK_ARG(u_out != u && u_out != c && c_out != u && c_out != c && u_out != c_out,
                    "depth_refine_fwd: an output aliases an input or the other output: every pixel reads its neighbours' inputs");
    A.u = u, A.c = c, A.g = g, A.u_out = u_out, A.c_out = c_out;
    rf::launch(rf::FORWARD, C, A, blocks, (hipStream_t)stream);
    AADFF_CHECK_LAUNCH();
    return 0;
}

extern "C" int aadff_depth_refine_bwd(const float* u, const float* c, const float* g, const float* g_u_out, const float* g_c_out,
                                      float* d_u_or_null, float* d_c_or_null, void* work, size_t work_bytes, int N, int C, int H, int W,
                                      int radius, float ks, float kr, aadff_stream_t stream) {
    rf::Args A = {};
    long blocks = 0;
    if (int rc = rf::check("depth_refine_bwd", u, c, g, N, C, H, W, radius, ks, kr, A, blocks)) return rc;
    AADFF_CHECK_ARG(g_u_out, "depth_refine_bwd: g_u_out is NULL");
    AADFF_CHECK_ARG(g_c_out, "depth_refine_bwd: g_c_out is NULL");
    AADFF_CHECK_ARG(d_u_or_null || d_c_or_null, "depth_refine_bwd: no gradient is asked for");
    const size_t need = 4 * sizeof(float) * (size_t)N * H * W;
    AADFF_CHECK_ARG(work && work_bytes >= need, "depth_refine_bwd: workspace of %zu bytes, %zu are needed", work_bytes, need);
    A.u = u, A.c = c, A.g = g, A.gu = g_u_out, A.gc = g_c_out, A.work = (float*)work, A.d_u = d_u_or_null, A.d_c = d_c_or_null;
    rf::launch(rf::PASS1, C, A, blocks, (hipStream_t)stream);
    AADFF_CHECK_LAUNCH();
    rf::launch(rf::GATHER, C, A, blocks, (hipStream_t)stream);
    AADFF_CHECK_LAUNCH();
    return 0;
}
