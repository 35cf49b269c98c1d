// Evaluation metrics on the GPU: what the reference's validate() computes on the host, per sample, with nine numpy passes
// (dff/metrics.py) and scikit-image's PSNR / SSIM, as two kernel families that leave per-image float64 sums on the device.
//
//   depth_sums<VEC>      est, gt [N,1,H,W] (+ mask, + conf) -> one row of 16 partial sums per workgroup: a thread owns four neighbouring
//                        pixels of the flattened image (16-byte accesses with VEC, the same arithmetic element by element without),
//                        forms every term in float64 from the exactly converted float32 values (IEEE division, the device's float64
//                        log) and adds them in float64; fixed-order wave and workgroup sums.  depth_final adds the rows of an image.
//   image_ssim<VEC>      pred, target [N,C,H,W] -> per workgroup the exact integer sum of squared differences of its own pixels and the
//                        float64 sum of the SSIM index over its 32 x 64 tile of 7 x 7 windows.  Both images are quantised to bytes into
//                        LDS (tile plus a 3-pixel halo on every side: 38 x 70), the five window sums are formed in int32, horizontally
//                        then vertically, the variance and covariance numerators in int64, and only the last step is float64.
//   image_sse<VEC>       the squared differences alone, for any extent (PSNR without SSIM).  image_final adds the partials of an image.
// No atomics anywhere: every output is bit-identical from run to run.  The unit is built with -ffp-contract=off: the quantisation is the
// literal float32 step sequence of torch's `img.mul(255).add_(0.5).clamp_(0, 255).to(torch.uint8)`.
#include "common.h"

namespace aadff {
namespace mt {

constexpr int NT = 256, WAVES = NT / kWave;
constexpr int COLS = AADFF_DEPTH_METRIC_COLS;
constexpr int TH = AADFF_SSIM_TILE_H, TW = AADFF_SSIM_TILE_W;  // windows per tile
constexpr int RH = TH + 6, RW = TW + 6, RS = 72;               // staged rows and columns; RS: bytes per staged row (18 groups of four)
static_assert(TW == 64 && RS % 4 == 0 && RS >= RW, "the tile indexing below assumes 64 windows per row");

// one image value -> byte, each step rounded separately in float32 (a nan, which torch leaves undefined, gives 0)
__host__ __device__ __forceinline__ int quantise(float v) {
#pragma clang fp contract(off)
    float t = v * 255.f;
    t = t + 0.5f;
    t = t < 0.f ? 0.f : t;                                    // also -0.0 -> compares equal, truncates to 0 either way
    t = t > 255.f ? 255.f : t;
    return t == t ? (int)t : 0;
}

__device__ __forceinline__ double wave_sum_f64(double v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}
__device__ __forceinline__ long long wave_sum_i64(long long v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
    return v;
}

// ------------------------------------------------------------------ depth
struct DepthArgs {
    const float* est;
    const float* gt;
    const unsigned char* mask;                                // or NULL
    const float* conf;                                        // or NULL
    double* part;                                             // [N][bpn][COLS]
    long HW;
    unsigned bpn;                                             // workgroups per image
    int finite;
};

__device__ __forceinline__ bool is_inf(double v) { return __builtin_isinf(v); }

// a thread's sums: named scalars, the counts as integers (an array of sixteen doubles indexed in a loop went to scratch memory)
struct Acc {
    double ad, d2, rel, sq, l2, c, cad, cd2;
    int n, lt1, lt2, lt3, n_rel, n_sq, n_log, n_q;
};

// the terms of one pixel (include/aadff.h has the column numbering)
__device__ __forceinline__ void add_pixel(Acc& a, float ef, float gf, float cf, bool valid, bool finite) {
    const double e = (double)ef, g = (double)gf, c = (double)cf;
    const double d = g - e, ad = fabs(d), d2 = d * d;
    const double rel = ad / g, sq = d2 / g;
    const double lg = log(g), le = log(e), dl = lg - le, l2 = dl * dl;
    const double qa = e / g, qb = g / e;
    const bool qnan = qa != qa || qb != qb;                   // numpy's maximum hands a nan on
    const double q = fmax(qa, qb);
    if (!(finite || valid)) return;
    // FINITE (dff/metrics.py:10-43): an infinite term is left out of its sum and each function has its own idea of "infinite"
    const bool ri = finite && is_inf(rel), si = finite && is_inf(sq), li = finite && is_inf(l2);
    a.n += 1, a.ad += ad, a.d2 += d2;
    a.rel += ri ? 0.0 : rel, a.sq += si ? 0.0 : sq, a.l2 += li ? 0.0 : l2;
    a.lt1 += !qnan && q < 1.25, a.lt2 += !qnan && q < 1.5625, a.lt3 += !qnan && q < 1.953125;
    a.c += c, a.cad += c * ad, a.cd2 += c * d2;
    if (finite) {
        a.n_rel += !ri, a.n_sq += !si;
        a.n_log += !(is_inf(le) || is_inf(lg));
        a.n_q += qnan || !is_inf(q);
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void depth_sums(DepthArgs A) {
    __shared__ double sh[WAVES][COLS];
    const unsigned n = blockIdx.x / A.bpn;
    const long i0 = ((long)(blockIdx.x % A.bpn) * NT + threadIdx.x) * 4;
    const bool live = i0 < A.HW;
    const size_t base = (size_t)n * (size_t)A.HW;
    float e[4], g[4], c[4] = {0.f, 0.f, 0.f, 0.f};
    bool ok[4], m[4];
    if (VEC) {                                                // HW % 4 == 0: a group is inside or outside as a whole
        const size_t o = base + (size_t)(live ? i0 : 0);
        const float4 te = *reinterpret_cast<const float4*>(A.est + o), tg = *reinterpret_cast<const float4*>(A.gt + o);
        e[0] = te.x, e[1] = te.y, e[2] = te.z, e[3] = te.w;
        g[0] = tg.x, g[1] = tg.y, g[2] = tg.z, g[3] = tg.w;
        if (A.conf) {
            const float4 tc = *reinterpret_cast<const float4*>(A.conf + o);
            c[0] = tc.x, c[1] = tc.y, c[2] = tc.z, c[3] = tc.w;
        }
        uchar4 tm = make_uchar4(1, 1, 1, 1);
        if (A.mask) tm = *reinterpret_cast<const uchar4*>(A.mask + o);
        m[0] = tm.x != 0, m[1] = tm.y != 0, m[2] = tm.z != 0, m[3] = tm.w != 0;
#pragma unroll
        for (int j = 0; j < 4; ++j) ok[j] = live;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            ok[j] = i0 + j < A.HW;
            const size_t o = base + (size_t)(ok[j] ? i0 + j : 0);  // a lane beyond the image reads pixel 0 and adds nothing
            e[j] = A.est[o], g[j] = A.gt[o];
            if (A.conf) c[j] = A.conf[o];
            m[j] = A.mask ? A.mask[o] != 0 : true;
        }
    }
    Acc a = {};
    if (ok[0]) add_pixel(a, e[0], g[0], c[0], m[0], A.finite != 0);
    if (ok[1]) add_pixel(a, e[1], g[1], c[1], m[1], A.finite != 0);
    if (ok[2]) add_pixel(a, e[2], g[2], c[2], m[2], A.finite != 0);
    if (ok[3]) add_pixel(a, e[3], g[3], c[3], m[3], A.finite != 0);
    const double col[COLS] = {(double)a.n, a.ad, a.d2, a.rel, a.sq, a.l2, (double)a.lt1, (double)a.lt2, (double)a.lt3, a.c, a.cad, a.cd2,
                              (double)a.n_rel, (double)a.n_sq, (double)a.n_log, (double)a.n_q};
#pragma unroll
    for (int k = 0; k < COLS; ++k) {
        const double v = wave_sum_f64(col[k]);
        if (threadIdx.x % kWave == 0) sh[threadIdx.x / kWave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < COLS) {
        double v = sh[0][threadIdx.x];
        for (int w = 1; w < WAVES; ++w) v += sh[w][threadIdx.x];
        A.part[(size_t)blockIdx.x * COLS + threadIdx.x] = v;
    }
}

// second stage: workgroup n adds the bpn partial rows of image n in a fixed order - thread (j, c) takes rows j, j + 16, ... of column c
// in turn, then a fixed tree over j
__global__ __launch_bounds__(NT) void depth_final(const double* part, long bpn, double* out) {
    __shared__ double sh[NT];
    const int c = threadIdx.x % COLS, j = threadIdx.x / COLS;
    const double* p = part + (size_t)blockIdx.x * (size_t)bpn * COLS;
    double acc = 0.0;
    for (long i = j; i < bpn; i += NT / COLS) acc += p[i * COLS + c];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = NT / 2; w >= COLS; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x < COLS) out[(size_t)blockIdx.x * COLS + threadIdx.x] = sh[threadIdx.x];
}

// ------------------------------------------------------------------ images
struct ImageArgs {
    const float* x;
    const float* y;
    long long* part_sse;                                      // [N][bpi]
    double* part_ssim;                                        // [N][bpi]
    int C, H, W, tiles_y, tiles_x;
    long CHW;
    unsigned bpi;                                             // workgroups per image
};

// workgroup sums of the two partials, written by thread 0
__device__ __forceinline__ void block_store(const ImageArgs& A, long long sse, double ssim, long long* shi, double* shd) {
    sse = wave_sum_i64(sse);
    ssim = wave_sum_f64(ssim);
    if (threadIdx.x % kWave == 0) shi[threadIdx.x / kWave] = sse, shd[threadIdx.x / kWave] = ssim;
    __syncthreads();
    if (threadIdx.x == 0) {
        long long a = shi[0];
        double b = shd[0];
        for (int w = 1; w < WAVES; ++w) a += shi[w], b += shd[w];
        A.part_sse[blockIdx.x] = a;
        A.part_ssim[blockIdx.x] = b;
    }
}

template <bool VEC>
__global__ __launch_bounds__(NT) void image_ssim(ImageArgs A) {
    __shared__ unsigned int q4x[RH * RS / 4], q4y[RH * RS / 4];   // the quantised tile with its halo, one byte per pixel
    __shared__ int hs[RH * TW], hxx[RH * TW], hyy[RH * TW], hxy[RH * TW];   // sums over seven columns; hs = sum x | sum y << 16
    __shared__ long long shi[WAVES];
    __shared__ double shd[WAVES];
    unsigned char* qx = reinterpret_cast<unsigned char*>(q4x);
    unsigned char* qy = reinterpret_cast<unsigned char*>(q4y);
    const int H = A.H, W = A.W;
    const unsigned n = blockIdx.x / A.bpi;
    unsigned r = blockIdx.x % A.bpi;
    const int tj = (int)(r % (unsigned)A.tiles_x);
    r /= (unsigned)A.tiles_x;
    const int ti = (int)(r % (unsigned)A.tiles_y), ch = (int)(r / (unsigned)A.tiles_y);
    const size_t plane = ((size_t)n * A.C + ch) * (size_t)H * W;
    const int y0 = ti * TH, x0 = tj * TW;
    // every pixel is counted once in the squared error: a tile owns its TH x TW corner, the last tile of a row / column the halo as well
    const int own_h = ti == A.tiles_y - 1 ? RH : TH, own_w = tj == A.tiles_x - 1 ? RS : TW;
    long long sse = 0;
    if (VEC) {                                                // W % 4 == 0 and x0 % 4 == 0: a group of four is inside or outside as a whole
        for (int idx = threadIdx.x; idx < RH * (RS / 4); idx += NT) {
            const int rr = idx / (RS / 4), c4 = (idx % (RS / 4)) * 4, yy = y0 + rr, xx = x0 + c4;
            unsigned px = 0, py = 0;
            if (yy < H && xx < W) {
                const size_t o = plane + (size_t)yy * W + xx;
                const float4 a = *reinterpret_cast<const float4*>(A.x + o), b = *reinterpret_cast<const float4*>(A.y + o);
                const float av[4] = {a.x, a.y, a.z, a.w}, bv[4] = {b.x, b.y, b.z, b.w};
#pragma unroll
                for (int k = 0; k < 4; ++k) {
                    const int u = quantise(av[k]), v = quantise(bv[k]);
                    px |= (unsigned)u << (8 * k), py |= (unsigned)v << (8 * k);
                    if (rr < own_h && c4 + k < own_w) sse += (long long)((u - v) * (u - v));
                }
            }
            q4x[idx] = px, q4y[idx] = py;
        }
    } else {
        for (int idx = threadIdx.x; idx < RH * RS; idx += NT) {
            const int rr = idx / RS, cc = idx % RS, yy = y0 + rr, xx = x0 + cc;
            int u = 0, v = 0;
            if (yy < H && xx < W) {
                const size_t o = plane + (size_t)yy * W + xx;
                u = quantise(A.x[o]), v = quantise(A.y[o]);
                if (rr < own_h && cc < own_w) sse += (long long)((u - v) * (u - v));
            }
            qx[idx] = (unsigned char)u, qy[idx] = (unsigned char)v;
        }
    }
    __syncthreads();
    for (int idx = threadIdx.x; idx < RH * TW; idx += NT) {   // sums over columns cc .. cc + 6 of every staged row
        const int rr = idx / TW, cc = idx % TW;
        const unsigned char* a = qx + rr * RS + cc;
        const unsigned char* b = qy + rr * RS + cc;
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int u = a[k], v = b[k];
            sx += u, sy += v, sxx += u * u, syy += v * v, sxy += u * v;
        }
        hs[idx] = sx | (sy << 16), hxx[idx] = sxx, hyy[idx] = syy, hxy[idx] = sxy;
    }
    __syncthreads();
    // (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)) with u = S / 49 and v = (49 Sxx - Sx^2) / (49 * 48), both factors of
    // numerator and denominator multiplied through by 49^2 and 49 * 48: the integer parts are exact, the constants are rounded once
    const double K1 = (0.01 * 255.0) * (0.01 * 255.0) * 2401.0, K2 = (0.03 * 255.0) * (0.03 * 255.0) * 2352.0;
    double ssim = 0.0;
    const int wj = threadIdx.x % TW;
    for (int wi = threadIdx.x / TW; wi < TH; wi += NT / TW) {
        if (y0 + wi > H - 7 || x0 + wj > W - 7) continue;     // the window would leave the image
        int sx = 0, sy = 0, sxx = 0, syy = 0, sxy = 0;
#pragma unroll
        for (int k = 0; k < 7; ++k) {
            const int o = (wi + k) * TW + wj, p = hs[o];
            sx += p & 0xffff, sy += p >> 16, sxx += hxx[o], syy += hyy[o], sxy += hxy[o];
        }
        const long long lx = sx, ly = sy;
        const long long nx = 49LL * sxx - lx * lx, ny = 49LL * syy - ly * ly, nxy = 49LL * sxy - lx * ly;
        const double a1 = (double)(2 * lx * ly) + K1, a2 = (double)(2 * nxy) + K2;
        const double b1 = (double)(lx * lx + ly * ly) + K1, b2 = (double)(nx + ny) + K2;
        ssim += (a1 * a2) / (b1 * b2);
    }
    block_store(A, sse, ssim, shi, shd);
}

template <bool VEC>
__global__ __launch_bounds__(NT) void image_sse(ImageArgs A) {
    __shared__ long long shi[WAVES];
    __shared__ double shd[WAVES];
    const unsigned n = blockIdx.x / A.bpi;
    const long i0 = ((long)(blockIdx.x % A.bpi) * NT + threadIdx.x) * 4;
    const size_t base = (size_t)n * (size_t)A.CHW;
    long long sse = 0;
    if (VEC) {
        if (i0 < A.CHW) {
            const float4 a = *reinterpret_cast<const float4*>(A.x + base + i0), b = *reinterpret_cast<const float4*>(A.y + base + i0);
            const int d0 = quantise(a.x) - quantise(b.x), d1 = quantise(a.y) - quantise(b.y), d2 = quantise(a.z) - quantise(b.z),
                      d3 = quantise(a.w) - quantise(b.w);
            sse = (long long)(d0 * d0 + d1 * d1 + d2 * d2 + d3 * d3);
        }
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (i0 + j < A.CHW) {
                const int d = quantise(A.x[base + i0 + j]) - quantise(A.y[base + i0 + j]);
                sse += (long long)(d * d);
            }
    }
    block_store(A, sse, 0.0, shi, shd);
}

// second stage: workgroup n adds the partials of image n - the integers exactly, the float64 values in a fixed order (thread t takes
// t, t + 256, ... in turn, then a fixed tree); sums [N][2]
__global__ __launch_bounds__(NT) void image_final(const long long* part_sse, const double* part_ssim, long bpi, double* out) {
    __shared__ long long shi[NT];
    __shared__ double shd[NT];
    const size_t o = (size_t)blockIdx.x * (size_t)bpi;
    long long a = 0;
    double b = 0.0;
    for (long i = threadIdx.x; i < bpi; i += NT) a += part_sse[o + i], b += part_ssim[o + i];
    shi[threadIdx.x] = a, shd[threadIdx.x] = b;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) shi[threadIdx.x] += shi[threadIdx.x + w], shd[threadIdx.x] += shd[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[2 * (size_t)blockIdx.x] = (double)shi[0], out[2 * (size_t)blockIdx.x + 1] = shd[0];
}

}  // namespace mt
}  // namespace aadff

using namespace aadff;

extern "C" int aadff_depth_metric_sums(const float* est, const float* gt, const unsigned char* mask_or_null, const float* conf_or_null,
                                       double* sums, void* workspace, size_t workspace_bytes, int N, int H, int W, int valid_mode,
                                       aadff_stream_t stream) {
    AADFF_CHECK_ARG(est, "depth_metric_sums: est is NULL");
    AADFF_CHECK_ARG(gt, "depth_metric_sums: gt is NULL");
    AADFF_CHECK_ARG(sums, "depth_metric_sums: sums is NULL");
    AADFF_CHECK_ARG(valid_mode == AADFF_VALID_MASK || valid_mode == AADFF_VALID_FINITE, "depth_metric_sums: valid_mode = %d is neither MASK nor FINITE",
                    valid_mode);
    AADFF_CHECK_ARG(valid_mode == AADFF_VALID_MASK || !mask_or_null, "depth_metric_sums: mask must be NULL in FINITE mode, where every pixel takes part");
    AADFF_CHECK_ARG(N > 0, "depth_metric_sums: N = %d is not positive", N);
    AADFF_CHECK_ARG(H > 0, "depth_metric_sums: H = %d is not positive", H);
    AADFF_CHECK_ARG(W > 0, "depth_metric_sums: W = %d is not positive", W);
    const long HW = (long)H * W, bpn = ((HW + 3) / 4 + mt::NT - 1) / mt::NT;
    AADFF_CHECK_ARG(HW < (1L << 31) - 8 && bpn * N < (1L << 31), "depth_metric_sums: N = %d, H = %d, W = %d are too large for one launch", N, H, W);
    const size_t need = sizeof(double) * mt::COLS * (size_t)bpn * (size_t)N;
    AADFF_CHECK_ARG(workspace && workspace_bytes >= need, "depth_metric_sums: workspace of %zu bytes, %zu are needed", workspace_bytes, need);
    mt::DepthArgs A = {est, gt, mask_or_null, conf_or_null, (double*)workspace, HW, (unsigned)bpn, valid_mode == AADFF_VALID_FINITE};
    const uintptr_t bits = (uintptr_t)est | (uintptr_t)gt | (uintptr_t)conf_or_null;
    const bool vec = HW % 4 == 0 && bits % 16 == 0 && (uintptr_t)mask_or_null % 4 == 0;      // every image then starts on 16 bytes (mask: 4)
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(bpn * N));
    if (vec) hipLaunchKernelGGL(mt::depth_sums<true>, grid, dim3(mt::NT), 0, st, A);
    else hipLaunchKernelGGL(mt::depth_sums<false>, grid, dim3(mt::NT), 0, st, A);
    AADFF_CHECK_LAUNCH();
    hipLaunchKernelGGL(mt::depth_final, dim3((unsigned)N), dim3(mt::NT), 0, st, (const double*)workspace, bpn, sums);
    AADFF_CHECK_LAUNCH();
    return 0;
}

extern "C" int aadff_image_metric_sums(const float* pred, const float* target, double* sums, void* workspace, size_t workspace_bytes, int N,
                                       int C, int H, int W, int want_ssim, aadff_stream_t stream) {
    AADFF_CHECK_ARG(pred, "image_metric_sums: pred is NULL");
    AADFF_CHECK_ARG(target, "image_metric_sums: target is NULL");
    AADFF_CHECK_ARG(sums, "image_metric_sums: sums is NULL");
    AADFF_CHECK_ARG(N > 0, "image_metric_sums: N = %d is not positive", N);
    AADFF_CHECK_ARG(C >= 1 && C <= 4, "image_metric_sums: C = %d is outside 1..4", C);
    AADFF_CHECK_ARG(H > 0, "image_metric_sums: H = %d is not positive", H);
    AADFF_CHECK_ARG(W > 0, "image_metric_sums: W = %d is not positive", W);
    AADFF_CHECK_ARG(!want_ssim || (H >= 7 && W >= 7), "image_metric_sums: SSIM needs H >= 7 and W >= 7 (the 7 x 7 window), got H = %d, W = %d", H, W);
    const long CHW = (long)C * H * W;
    mt::ImageArgs A = {};
    long bpi;
    if (want_ssim) {
        A.tiles_y = (H - 6 + mt::TH - 1) / mt::TH, A.tiles_x = (W - 6 + mt::TW - 1) / mt::TW;
        bpi = (long)C * A.tiles_y * A.tiles_x;
    } else {
        bpi = ((CHW + 3) / 4 + mt::NT - 1) / mt::NT;
    }
    AADFF_CHECK_ARG(CHW < (1L << 31) - 8 && bpi * N < (1L << 31), "image_metric_sums: N = %d, C = %d, H = %d, W = %d are too large for one launch", N, C, H, W);
    const size_t need = 16 * (size_t)bpi * (size_t)N;
    AADFF_CHECK_ARG(workspace && workspace_bytes >= need, "image_metric_sums: workspace of %zu bytes, %zu are needed", workspace_bytes, need);
    AADFF_CHECK_ARG((uintptr_t)workspace % 8 == 0, "image_metric_sums: workspace is not aligned to 8 bytes");
    A.x = pred, A.y = target, A.part_sse = (long long*)workspace, A.part_ssim = (double*)workspace + (size_t)bpi * N;
    A.C = C, A.H = H, A.W = W, A.CHW = CHW, A.bpi = (unsigned)bpi;
    const bool aligned = ((uintptr_t)pred | (uintptr_t)target) % 16 == 0;
    hipStream_t st = (hipStream_t)stream;
    const dim3 grid((unsigned)(bpi * N));
    if (want_ssim) {
        if (aligned && W % 4 == 0) hipLaunchKernelGGL(mt::image_ssim<true>, grid, dim3(mt::NT), 0, st, A);
        else hipLaunchKernelGGL(mt::image_ssim<false>, grid, dim3(mt::NT), 0, st, A);
    } else {
        if (aligned && CHW % 4 == 0) hipLaunchKernelGGL(mt::image_sse<true>, grid, dim3(mt::NT), 0, st, A);
        else hipLaunchKernelGGL(mt::image_sse<false>, grid, dim3(mt::NT), 0, st, A);
    }
    AADFF_CHECK_LAUNCH();
    hipLaunchKernelGGL(mt::image_final, dim3((unsigned)N), dim3(mt::NT), 0, st, (const long long*)A.part_sse, (const double*)A.part_ssim, bpi, sums);
    AADFF_CHECK_LAUNCH();
    return 0;
}

extern "C" int aadff_quantise_u8_host(const float* values, unsigned char* out, long n) {
    AADFF_CHECK_ARG(values, "quantise_u8_host: values is NULL");
    AADFF_CHECK_ARG(out, "quantise_u8_host: out is NULL");
    AADFF_CHECK_ARG(n >= 0, "quantise_u8_host: n = %ld is negative", n);
    for (long i = 0; i < n; ++i) out[i] = (unsigned char)mt::quantise(values[i]);
    return 0;
}
