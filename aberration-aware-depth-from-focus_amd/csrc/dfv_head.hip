// Cost-volume depth head: what the reference's DFVNet puts between a decoder level's cost volume and its loss
// (DFV_models/DFFNet.py:94-95, 102-115 with disparityregression of DFV_models/submodule.py:63-77) without the upsampled cost and the
// softmax at full resolution.
//
//   head_fwd      cost [B,S,h,w], foc [B,S] -> pred, std [B,1,H,W] (and prob [B,S,H,W] when asked for).  A thread owns one output pixel
//                 of a 64 x 4 tile; its four source cells and weights are formed once (ATen's bilinear rule, align_corners = False) and
//                 serve every slice.  Three loops over S: the maximum of the interpolated costs, the normaliser with pred, then std
//                 in the reference's form sum p (pred - f)^2 (and the probabilities).
//   bwd_reduce_x  a workgroup owns TC neighbouring cells of one cost row for R output rows and up to SC slices.  Its threads walk the
//                 footprint - every output pixel that reads one of the cells, found by inverting the forward's own index function
//                 (axis_range) - recompute the softmax from the cost, put dz_s = p_s (f_s - pred) g into LDS and gather it, weighted
//                 along x, into one sum per (row, cell, slice): t [B,S,H,w], a scratch of 1 / ratio of the full resolution.  The
//                 pixels whose left cell lies in the tile also give the partial sums of d_foc, gathered from LDS the same way.
//   bwd_reduce_y  d_cost[b,s,i,j] = sum over the output rows that read cost row i of their weight times t[b,s,y,j].
//   final_sum     adds the d_foc partials in a fixed order.
// Gather form throughout, no atomics: every output is bit-identical from run to run and does not depend on which gradients are asked
// for.  fp contraction is off: the index arithmetic must round the same way wherever it is evaluated.
#include "common.h"

namespace aadff {
namespace dv {

constexpr int NT = 256;
constexpr int TX = 64, TY = 4;                                // forward: output pixels per workgroup
constexpr int SC = 16;                                        // backward: slices per workgroup
constexpr int SREG = SC;                                      // up to this many slices a thread keeps its softmax terms in registers
constexpr int MAXTC = 8, MAXR = 8;                            // backward: at most this many cells of a row and output rows per workgroup

struct Args {
    const float* cost;
    const float* foc;
    float* pred;                                              // forward
    float* std;
    float* prob;                                              // or NULL
    const float* g;                                           // backward: g_pred
    float* t;                                                 // [B,S,H,w], or NULL when d_cost is not asked for
    float* part;                                              // d_foc partials [B,S,rgroups * tiles], or NULL
    float* d_cost;
    int S, h, w, H, W;
    float sh, sw;                                             // float(in) / out per axis
    int tx, ty;                                               // forward: tiles per image; bwd_reduce_y: tx workgroups per plane
    int TC, R, tiles, rgroups;                                // backward: cells and rows per workgroup, workgroups per row and per column
};

// ATen's source position of an output index for align_corners = False: the cell below, the cell above (the same on the last one)
// and the weight of the latter
struct Src {
    int i0, i1;
    float lam;
};

__device__ __forceinline__ Src axis_src(int dst, float scale, int in) {
#pragma clang fp contract(off)
    float s = scale * ((float)dst + 0.5f) - 0.5f;
    s = s < 0.f ? 0.f : s;
    int i0 = (int)s;
    i0 = i0 < in - 1 ? i0 : in - 1;                           // (never taken when out >= in; keeps every read inside the plane)
    Src r;
    r.i0 = i0, r.i1 = i0 + 1 < in ? i0 + 1 : in - 1, r.lam = s - (float)i0;
    return r;
}

// first output index whose i0 is at least k (`out` if there is none).  i0 is monotone in the output index - every float32 step of
// axis_src is - so an estimate from the inverse formula is corrected by stepping with axis_src itself until it is exact.
__device__ __forceinline__ int first_at_least(int k, float scale, int in, int out) {
#pragma clang fp contract(off)
    if (k <= 0) return 0;
    if (k > in - 1) return out;
    const float guess = ((float)k + 0.5f) / scale - 0.5f;
    int x = guess < 0.f ? 0 : (guess < (float)out ? (int)guess : out);
    while (x > 0 && axis_src(x - 1, scale, in).i0 >= k) --x;
    while (x < out && axis_src(x, scale, in).i0 < k) ++x;
    return x;
}

// the output indices [lo, hi) that read cell j: i0 == j, or i1 == j, which is i0 == j - 1 (and i0 == j on the last cell)
__device__ __forceinline__ void axis_range(int j, float scale, int in, int out, int& lo, int& hi) {
    lo = first_at_least(j - 1, scale, in, out);
    hi = first_at_least(j + 1, scale, in, out);
}

// weight with which an output index reads cell j
__device__ __forceinline__ float axis_weight(int i0, int i1, float lam, int j) {
#pragma clang fp contract(off)
    return (i0 == j ? 1.f - lam : 0.f) + (i1 == j ? lam : 0.f);
}

// the four cells of a pixel as element offsets in a cost plane, and their weights
struct Tap {
    int o00, o01, o10, o11;
    float wx0, wx1, wy0, wy1;
};

__device__ __forceinline__ Tap make_tap(const Src& sy, const Src& sx, int w) {
#pragma clang fp contract(off)
    Tap T;
    T.o00 = sy.i0 * w + sx.i0, T.o01 = sy.i0 * w + sx.i1, T.o10 = sy.i1 * w + sx.i0, T.o11 = sy.i1 * w + sx.i1;
    T.wx0 = 1.f - sx.lam, T.wx1 = sx.lam, T.wy0 = 1.f - sy.lam, T.wy1 = sy.lam;
    return T;
}

__device__ __forceinline__ float interp(const float* p, const Tap& T) {
#pragma clang fp contract(off)
    return T.wy0 * (T.wx0 * p[T.o00] + T.wx1 * p[T.o01]) + T.wy1 * (T.wx0 * p[T.o10] + T.wx1 * p[T.o11]);
}

// softmax over the slices of a pixel's interpolated costs: the maximum m, the normaliser l = sum exp(z - m) and pred = sum p f
__device__ __forceinline__ void softmax_stats(const float* c, size_t hw, int S, const Tap& T, const float* f, float& m, float& l, float& pred) {
#pragma clang fp contract(off)
    m = -INFINITY;
    for (int s = 0; s < S; ++s) m = fmaxf(m, interp(c + (size_t)s * hw, T));
    float acc = 0.f;
    l = 0.f;
    for (int s = 0; s < S; ++s) {
        const float e = expf(interp(c + (size_t)s * hw, T) - m);
        l += e;
        acc += e * f[s];
    }
    pred = acc / l;
}

// the same for S <= SREG slices with the terms kept in registers: e[s] = exp(z_s - m), so that the later loops neither interpolate
// nor exponentiate again.  The steps and their order are those of softmax_stats: both paths give the same bits.
__device__ __forceinline__ void softmax_small(const float* c, size_t hw, int S, const Tap& T, const float* f, float (&e)[SREG], float& l, float& pred) {
#pragma clang fp contract(off)
    float m = -INFINITY;
#pragma unroll
    for (int s = 0; s < SREG; ++s) {
        e[s] = s < S ? interp(c + (size_t)s * hw, T) : -INFINITY;
        m = fmaxf(m, e[s]);
    }
    float acc = 0.f;
    l = 0.f;
#pragma unroll
    for (int s = 0; s < SREG; ++s) {
        if (s < S) {
            e[s] = expf(e[s] - m);
            l += e[s];
            acc += e[s] * f[s];
        }
    }
    pred = acc / l;
}

__global__ __launch_bounds__(NT) void head_fwd(Args A) {
#pragma clang fp contract(off)
    const unsigned per = (unsigned)A.tx * (unsigned)A.ty;
    const unsigned b = blockIdx.x / per, rem = blockIdx.x % per;
    const int x = (int)(rem % (unsigned)A.tx) * TX + (int)(threadIdx.x % TX);
    const int y = (int)(rem / (unsigned)A.tx) * TY + (int)(threadIdx.x / TX);
    if (x >= A.W || y >= A.H) return;
    const int S = A.S;
    const size_t hw = (size_t)A.h * A.w, HW = (size_t)A.H * A.W;
    const float* c = A.cost + (size_t)b * S * hw;
    const float* f = A.foc + (size_t)b * S;
    const Tap T = make_tap(axis_src(y, A.sh, A.h), axis_src(x, A.sw, A.w), A.w);
    const size_t pix = (size_t)y * A.W + x;
    float m, l, pred, var = 0.f;
    if (S <= SREG) {
        float e[SREG];
        softmax_small(c, hw, S, T, f, e, l, pred);
#pragma unroll
        for (int s = 0; s < SREG; ++s) {
            if (s < S) {
                const float p = e[s] / l;
                const float d = pred - f[s];
                var += p * (d * d);
                if (A.prob) A.prob[((size_t)b * S + s) * HW + pix] = p;
            }
        }
    } else {
        softmax_stats(c, hw, S, T, f, m, l, pred);
        for (int s = 0; s < S; ++s) {
            const float p = expf(interp(c + (size_t)s * hw, T) - m) / l;
            const float d = pred - f[s];
            var += p * (d * d);
            if (A.prob) A.prob[((size_t)b * S + s) * HW + pix] = p;
        }
    }
    A.pred[(size_t)b * HW + pix] = pred;
    A.std[(size_t)b * HW + pix] = sqrtf(var);
}

__global__ __launch_bounds__(NT) void bwd_reduce_x(Args A) {
#pragma clang fp contract(off)
    __shared__ float sdz[SC][NT + 1];                         // dz of the chunk's pixels (+ 1: the gather reads a column per lane)
    __shared__ float sq[SC][NT + 1];                          // p g of the chunk's pixels the tile owns, 0 for the others
    __shared__ float sacc[MAXR * MAXTC * SC];                 // one sum per (row, cell, slice), each owned by one thread
    __shared__ double sfoc[MAXR * SC];                        // one d_foc sum per (row, slice), likewise; float64: up to W terms in turn
    __shared__ int s_i0[NT], s_i1[NT];
    __shared__ float s_lam[NT];
    __shared__ int s_lo[MAXTC], s_hi[MAXTC];

    const int t = (int)threadIdx.x, S = A.S;
    const unsigned per = (unsigned)A.rgroups * (unsigned)A.tiles;
    const unsigned b = blockIdx.x / per, rem = blockIdx.x % per;
    const int rg = (int)(rem / (unsigned)A.tiles), tile = (int)(rem % (unsigned)A.tiles);
    const int y0 = rg * A.R, rows = min(A.R, A.H - y0);
    const int c0 = tile * A.TC, nc = min(A.TC, A.w - c0);
    const int s0 = (int)blockIdx.y * SC, ns = min(SC, S - s0);
    const bool want_cost = A.t != nullptr, want_foc = A.part != nullptr;

    if (t < nc) axis_range(c0 + t, A.sw, A.w, A.W, s_lo[t], s_hi[t]);
    __syncthreads();
    const int xbeg = s_lo[0], fw = s_hi[nc - 1] - xbeg;      // the footprint: fw pixels of each of the rows
    const long npx = (long)rows * fw;
    const bool small = npx <= 0x7fffffffL;                    // 32-bit division where it is enough: the 64-bit one is emulated
    const int items = rows * nc * ns, fitems = rows * ns;
    // an item, a sum over pixels of the chunk, belongs to the same thread in every chunk; the d_foc items go to the last threads
    for (int it = t; it < items; it += NT) sacc[it] = 0.f;
    for (int it = NT - 1 - t; it < fitems; it += NT) sfoc[it] = 0.0;

    const size_t hw = (size_t)A.h * A.w, HW = (size_t)A.H * A.W;
    const float* c = A.cost + (size_t)b * S * hw;
    const float* f = A.foc + (size_t)b * S;
    for (long base = 0; base < npx; base += NT) {
        const long p = base + t;
        const bool live = p < npx;
        int r = 0, xo = 0;
        if (live) {
            if (small) r = (int)p / fw, xo = (int)p - r * fw;
            else r = (int)(p / fw), xo = (int)(p - (long)r * fw);
        }
        const int x = min(xbeg + xo, A.W - 1), y = y0 + r;   // (the clamp never acts on a live lane)
        const Src sx = axis_src(x, A.sw, A.w);
        const Tap T = make_tap(axis_src(y, A.sh, A.h), sx, A.w);
        s_i0[t] = sx.i0, s_i1[t] = sx.i1, s_lam[t] = sx.lam;
        const float g = A.g[(size_t)b * HW + (size_t)y * A.W + x];
        const bool own = live && sx.i0 >= c0 && sx.i0 < c0 + nc;                // every pixel has one left cell: counted once for d_foc
        float m, l, pred;
        if (S <= SREG) {                                      // one slab: s0 = 0, ns = S
            float e[SREG];
            softmax_small(c, hw, S, T, f, e, l, pred);
#pragma unroll
            for (int sl = 0; sl < SREG; ++sl) {
                if (sl < S) {
                    const float pr = e[sl] / l;
                    sdz[sl][t] = live ? pr * (f[sl] - pred) * g : 0.f;
                    sq[sl][t] = own ? pr * g : 0.f;
                }
            }
        } else {
            softmax_stats(c, hw, S, T, f, m, l, pred);
            for (int sl = 0; sl < ns; ++sl) {
                const float pr = expf(interp(c + (size_t)(s0 + sl) * hw, T) - m) / l;
                sdz[sl][t] = live ? pr * (f[s0 + sl] - pred) * g : 0.f;
                sq[sl][t] = own ? pr * g : 0.f;
            }
        }
        __syncthreads();
        if (want_cost) {
            for (int it = t; it < items; it += NT) {          // slices fastest: lanes read different rows of sdz
                const int sl = it % ns, cc = (it / ns) % nc, rr = it / (ns * nc);
                const long first = (long)rr * fw + (s_lo[cc] - xbeg), last = (long)rr * fw + (s_hi[cc] - xbeg);
                const int a = first > base ? (int)(first - base) : 0, e = last < base + NT ? (int)(last - base) : NT;
                float sum = 0.f;
                for (int i = a; i < e; ++i) sum += axis_weight(s_i0[i], s_i1[i], s_lam[i], c0 + cc) * sdz[sl][i];
                sacc[it] += sum;
            }
        }
        if (want_foc) {
            for (int it = NT - 1 - t; it < fitems; it += NT) {                   // the row's pixels of the chunk, in order
                const int sl = it % ns, rr = it / ns;
                const long first = (long)rr * fw, last = first + fw;
                const int a = first > base ? (int)(first - base) : 0, e = last < base + NT ? (int)(last - base) : NT;
                double sum = 0.0;
                for (int i = a; i < e; ++i) sum += (double)sq[sl][i];
                sfoc[it] += sum;
            }
        }
        __syncthreads();
    }
    if (want_cost) {
        for (int it = t; it < items; it += NT) {              // cells fastest: neighbouring lanes write neighbouring elements
            const int cc = it % nc, sl = (it / nc) % ns, rr = it / (nc * ns);
            A.t[(((size_t)b * S + s0 + sl) * A.H + y0 + rr) * A.w + c0 + cc] = sacc[(rr * nc + cc) * ns + sl];
        }
    }
    if (want_foc && t < ns) {
        double v = sfoc[t];
        for (int rr = 1; rr < rows; ++rr) v += sfoc[rr * ns + t];
        A.part[((size_t)b * S + s0 + t) * per + rem] = (float)v;  // one rounding per workgroup; final_sum adds in float64 again
    }
}

// a workgroup owns 256 neighbouring elements of one plane of d_cost (A.tx workgroups per plane)
__global__ __launch_bounds__(NT) void bwd_reduce_y(Args A) {
#pragma clang fp contract(off)
    const unsigned bs = blockIdx.x / (unsigned)A.tx;
    const unsigned e = (blockIdx.x % (unsigned)A.tx) * NT + threadIdx.x;
    if (e >= (unsigned)A.h * (unsigned)A.w) return;
    const int i = (int)(e / (unsigned)A.w), j = (int)(e - (unsigned)i * (unsigned)A.w);
    int lo, hi;
    axis_range(i, A.sh, A.h, A.H, lo, hi);
    const float* tp = A.t + (size_t)bs * A.H * A.w + j;
    float sum = 0.f;
    for (int y = lo; y < hi; ++y) {
        const Src sy = axis_src(y, A.sh, A.h);
        sum += axis_weight(sy.i0, sy.i1, sy.lam, i) * tp[(size_t)y * A.w];
    }
    A.d_cost[(size_t)bs * A.h * A.w + e] = sum;
}

// second stage of d_foc: workgroup r adds the `count` partials of row r in a fixed order and in float64 - thread t takes t, t + 256,
// ... in turn, then a fixed tree over the threads
__global__ __launch_bounds__(NT) void final_sum(const float* part, long count, float* out) {
    __shared__ double sh[NT];
    const float* p = part + (size_t)blockIdx.x * count;
    double acc = 0.0;
    for (long i = threadIdx.x; i < count; i += NT) acc += (double)p[i];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int wd = NT / 2; wd > 0; wd >>= 1) {
        if ((int)threadIdx.x < wd) sh[threadIdx.x] += sh[threadIdx.x + wd];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (float)sh[0];
}

static int check(const char* who, const void* cost, const void* foc, int B, int S, int h, int w, int H, int W, Args& A) {
    AADFF_CHECK_ARG(cost, "%s: cost is NULL", who);
    AADFF_CHECK_ARG(foc, "%s: foc_dists is NULL", who);
    AADFF_CHECK_ARG(S >= 1, "%s: S = %d, at least one slice is needed", who, S);
    AADFF_CHECK_ARG(B > 0, "%s: B = %d is not positive", who, B);
    AADFF_CHECK_ARG(h > 0 && w > 0, "%s: the cost is %d x %d", who, h, w);
    AADFF_CHECK_ARG(H >= h && W >= w, "%s: the output %d x %d is smaller than the cost %d x %d: shrinking is not supported", who, H, W, h, w);
    AADFF_CHECK_ARG((long)H * W < (1L << 31) - 8 && (long)B * S < (1L << 31), "%s: B = %d, S = %d, H = %d, W = %d are too large for one launch", who, B, S, H, W);
    A.S = S, A.h = h, A.w = w, A.H = H, A.W = W;
    A.sh = (float)h / (float)H, A.sw = (float)w / (float)W;
    return 0;
}

// cells of a row and output rows per workgroup of bwd_reduce_x: about one chunk of 256 footprint pixels (include/aadff.h)
static void bwd_tiling(int w, int W, Args& A) {
    const int ratio = (W + w - 1) / w;
    const int tc = 240 / ratio - 1;
    A.TC = tc < 1 ? 1 : (tc > MAXTC ? MAXTC : tc);
    const long width = ((long)A.TC + 1) * ratio + 1;
    const long r = NT / width;
    A.R = r < 1 ? 1 : (r > MAXR ? MAXR : (int)r);
    A.tiles = (w + A.TC - 1) / A.TC, A.rgroups = (A.H + A.R - 1) / A.R;
}

}  // namespace dv
}  // namespace aadff

using namespace aadff;

extern "C" int aadff_dfv_head_fwd(const float* cost, const float* foc_dists, float* pred, float* std, float* prob_or_null, int B, int S, int h,
                                  int w, int H, int W, aadff_stream_t stream) {
    dv::Args A = {};
    if (int rc = dv::check("dfv_head_fwd", cost, foc_dists, B, S, h, w, H, W, A)) return rc;
    AADFF_CHECK_ARG(pred, "dfv_head_fwd: pred is NULL");
    AADFF_CHECK_ARG(std, "dfv_head_fwd: std is NULL");
    A.cost = cost, A.foc = foc_dists, A.pred = pred, A.std = std, A.prob = prob_or_null;
    A.tx = (W + dv::TX - 1) / dv::TX, A.ty = (H + dv::TY - 1) / dv::TY;
    const long blocks = (long)A.tx * A.ty * B;
    AADFF_CHECK_ARG(blocks < (1L << 31), "dfv_head_fwd: B = %d, H = %d, W = %d are too large for one launch", B, H, W);
    hipLaunchKernelGGL(dv::head_fwd, dim3((unsigned)blocks), dim3(dv::NT), 0, (hipStream_t)stream, A);
    AADFF_CHECK_LAUNCH();
    return 0;
}

extern "C" int aadff_dfv_head_bwd(const float* cost, const float* foc_dists, const float* g_pred, float* d_cost_or_null, float* d_foc_or_null,
                                  void* workspace, size_t workspace_bytes, int B, int S, int h, int w, int H, int W, aadff_stream_t stream) {
    dv::Args A = {};
    if (int rc = dv::check("dfv_head_bwd", cost, foc_dists, B, S, h, w, H, W, A)) return rc;
    AADFF_CHECK_ARG(g_pred, "dfv_head_bwd: g_pred is NULL");
    AADFF_CHECK_ARG(d_cost_or_null || d_foc_or_null, "dfv_head_bwd: no gradient is asked for");
    dv::bwd_tiling(w, W, A);
    const size_t n_t = d_cost_or_null ? (size_t)B * S * H * w : 0, per = (size_t)A.rgroups * A.tiles;
    const size_t n_part = d_foc_or_null ? (size_t)B * S * per : 0, need = sizeof(float) * (n_t + n_part);
    AADFF_CHECK_ARG(workspace && workspace_bytes >= need, "dfv_head_bwd: workspace of %zu bytes, %zu are needed", workspace_bytes, need);
    const long blocks = (long)per * B, slabs = ((long)S + dv::SC - 1) / dv::SC;
    A.tx = (int)(((long)h * w + dv::NT - 1) / dv::NT);       // bwd_reduce_y: workgroups per plane of d_cost
    const long blocks_y = (long)A.tx * B * S;
    AADFF_CHECK_ARG(blocks < (1L << 31) && slabs < 65536 && blocks_y < (1L << 31), "dfv_head_bwd: B = %d, S = %d, H = %d, W = %d are too large for one launch",
                    B, S, H, W);
    A.cost = cost, A.foc = foc_dists, A.g = g_pred, A.d_cost = d_cost_or_null;
    A.t = d_cost_or_null ? (float*)workspace : nullptr;
    A.part = d_foc_or_null ? (float*)workspace + n_t : nullptr;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(dv::bwd_reduce_x, dim3((unsigned)blocks, (unsigned)slabs), dim3(dv::NT), 0, st, A);
    AADFF_CHECK_LAUNCH();
    if (d_cost_or_null) {
        hipLaunchKernelGGL(dv::bwd_reduce_y, dim3((unsigned)blocks_y), dim3(dv::NT), 0, st, A);
        AADFF_CHECK_LAUNCH();
    }
    if (d_foc_or_null) {
        hipLaunchKernelGGL(dv::final_sum, dim3((unsigned)(B * S)), dim3(dv::NT), 0, st, (const float*)A.part, (long)per, d_foc_or_null);
        AADFF_CHECK_LAUNCH();
    }
    return 0;
}
