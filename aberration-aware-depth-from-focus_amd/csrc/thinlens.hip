// Thin-lens baseline (ThinLens.coc + ThinLens.render, deeplens/psfnet.py:503-570; in the reference plain torch under autograd) with
// the PSF evaluated IN the gather kernel: the forward (one focus distance or a stack of S) and the fused backward to the image, the
// depth map and the focus distances.  DESIGN.md 4.4, 4.9.
//
// Forward, per pixel: coc -> Gaussian exp(-(x^2+y^2)/(2 rad^2)) cut at x^2+y^2 < rad^2 -> L1 normalise -> ks x ks gather over the
// replicate-padded image (render_psf.py:76-107, no flip).  24 B/pixel of HBM traffic + 4 B of depth instead of the 508 B/pixel of
// materialising the [N,H,W,ks,ks] PSF tensor and streaming it through local_psf_render.
//   coc chain in the reference's fp32 op order with IEEE divisions (the hard cut r^2 < rad^2 is discontinuous: a 1-ulp
//   difference in rad^2 next to an integer would flip a whole ring of taps), Gaussian as a product of two 1-D factors
//   (differs from exp of the sum by rounding only), normalisation folded into one division of the gathered sums.
//
//   thinlens_kernel             forward of one focus distance; thinlens_stack_kernel: of S focus distances per pixel run, the image
//                               window staged ONCE and a slice loop inside.  Both call the one body render_slice, so every slice of
//                               the stack is bit-equal to the single-focus render.
//   thinlens_input_grad_kernel  d_depth and the per-workgroup partials of d_foc: per row (n, slice, y, x) the PSF is re-evaluated from
//                               the staged window, d_r = sum_k p_k (rho_k - rho_bar) g_k / r^3 (centred form), chained through the coc.
//   thinlens_foc_sum_kernel     d_foc[n][s] = fixed-order double sum of the partials.
//   thinlens_rows_kernel        light pre-pass of the image gradient: r^2 and 1/Z of every row, 8 B per (n, slice, pixel).
//   thinlens_dimg_kernel        adjoint gather: a target pixel collects dy * p of every source pixel whose (clamped) tap lands on it,
//                               the source pixels' Gaussians evaluated in the kernel from r^2.
// No [N,H,W,ks,ks] tensor, no float atomics: every sum has a fixed order and the gradients are bit-identical from run to run.  The disc
// cut rho < r^2 is discontinuous, so r^2 is computed with the forward's exact operation order (fp contract off, IEEE divisions) and the
// weights as e[du] * e[dv]: the backward differentiates the PSF of the pixels that were actually rendered.
#include "common.h"
#include "gather_window.h"

namespace aadff {
namespace tlb {

struct Lens { float a_coc, foc_len, inv_ps, d_min, d_max; };      // a_coc = foc_len / fnum

// The coc chain, in the reference's operation order: d and fd already carry the sign convention.
struct Coc { float dc, cp, rad, rad2; };      // clamped depth, unclamped coc in pixels, r = max(cp, 0.1) / 2, r^2
__device__ __forceinline__ Coc coc_of(float d, float fd, const Lens& L) {
#pragma clang fp contract(off)
    Coc c;
    c.dc = fminf(fmaxf(d, L.d_min), L.d_max);
    float coc = L.a_coc * fabsf(c.dc - fd);                  // foc_len / fnum * |depth - foc_dist| / depth * foc_len / (foc_dist - foc_len)
    coc = coc / c.dc;
    coc = coc * L.foc_len;
    coc = coc / (fd - L.foc_len);
    c.cp = coc * L.inv_ps;
    c.rad = fmaxf(c.cp, 0.1f) * 0.5f;
    c.rad2 = c.rad * c.rad;
    return c;
}

// Unnormalised PSF of one pixel: the Gaussian exp(-rho / (2 r^2)) as a product of two 1-D factors, cut hard at rho = du^2 + dv^2 < r^2.
// Forward and backward evaluate the weights through this one form, so the backward differentiates the taps that were rendered.
template <int PAD>
__device__ __forceinline__ void disc_factors(float (&e)[PAD + 1], float rad2) {      // e[k] = exp(-k^2 / 2 / rad^2), k = 0..PAD
#pragma unroll
    for (int k = 0; k <= PAD; ++k) e[k] = __expf((float)(-(k * k)) * 0.5f / rad2);
}
template <int PAD>
__device__ __forceinline__ float disc_weight(const float (&e)[PAD + 1], float rad2, int u, int v, float& rho) {
    const int du = u < PAD ? PAD - u : u - PAD, dv = v < PAD ? PAD - v : v - PAD;
    rho = (float)(du * du + dv * dv);
    return rho < rad2 ? e[du] * e[dv] : 0.f;
}

// The forward of one focus distance for one 64-pixel run, from the staged window `tl`: coc -> 1-D factors -> cut, weights and gather ->
// one division -> store.  d and fd carry the sign convention; `out` is the lane's pixel in channel 0 of the slice, channel c at + c * cstride.
template <int KS, int CN>
__device__ __forceinline__ void render_slice(const float* tl, int lane, bool act, int C, float d, float fd, const Lens& L, float* __restrict__ out,
                                             size_t cstride) {
    constexpr int MC = CN > 0 ? CN : LP_MAXC;
    constexpr int TWD = LP_NPX + KS - 1;
    const float rad2 = coc_of(d, fd, L).rad2;
    float e[KS / 2 + 1], rho;
    disc_factors<KS / 2>(e, rad2);
    float acc[MC] = {};
    float wsum = 0.f;
#pragma unroll
    for (int u = 0; u < KS; ++u) {
#pragma unroll
        for (int v = 0; v < KS; ++v) {
            const float wv = disc_weight<KS / 2>(e, rad2, u, v, rho);
            wsum += wv;
#pragma unroll
            for (int cc = 0; cc < MC; ++cc)
                if (CN > 0 || cc < C) acc[cc] = fmaf(tl[(cc * KS + u) * TWD + lane + v], wv, acc[cc]);
        }
    }
    if (act) {
        const float inv = 1.f / wsum;
#pragma unroll
        for (int cc = 0; cc < MC; ++cc)
            if (CN > 0 || cc < C) out[cc * cstride] = acc[cc] * inv;
    }
}

// One focus distance per image: out [B,C,H,W].  A kernel of its own beside the stack kernel: the same call sent through
// thinlens_stack_kernel with S = 1 ran 17 % slower (measured; the cause was not isolated).  Here the focus distance is
// fetched before the window is staged and there is no slice loop.
template <int KS, int CN>
__global__ __launch_bounds__(64) void thinlens_kernel(const float* __restrict__ img, const float* __restrict__ depth,
                                                       const float* __restrict__ foc_dist, const int* __restrict__ negate,
                                                       float* __restrict__ out, int C, int H, int W, Lens L) {
    constexpr int MC = CN > 0 ? CN : LP_MAXC;
    constexpr int TWD = LP_NPX + KS - 1;
    __shared__ float tl[MC * KS * TWD];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * LP_NPX, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(LP_NPX, W - x0);
    const bool act = lane < npx;
    float d = depth[((size_t)b * H + y) * W + x0 + (act ? lane : 0)];
    float fd = foc_dist[b];
    stage_window<KS, CN>(img, tl, b, C, H, W, y, x0, lane);
    __syncthreads();
    if (negate && *negate) { d = -d; fd = -fd; }            // `if (depth < 0).any()` is a whole-tensor test (psfnet.py:505)
    render_slice<KS, CN>(tl, lane, act, C, d, fd, L, out + ((size_t)b * C * H + y) * W + x0 + lane, (size_t)H * W);
}

// S focus distances per image: out [B,C,S,H,W], the image window staged ONCE for all slices
template <int KS, int CN>
__global__ __launch_bounds__(64) void thinlens_stack_kernel(const float* __restrict__ img, const float* __restrict__ depth,
                                                             const float* __restrict__ foc_dists, const int* __restrict__ negate,
                                                             float* __restrict__ out, int C, int S, int H, int W, Lens L) {
    constexpr int MC = CN > 0 ? CN : LP_MAXC;
    constexpr int TWD = LP_NPX + KS - 1;
    __shared__ float tl[MC * KS * TWD];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * LP_NPX, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(LP_NPX, W - x0);
    const bool act = lane < npx;
    float d = depth[((size_t)b * H + y) * W + x0 + (act ? lane : 0)];
    stage_window<KS, CN>(img, tl, b, C, H, W, y, x0, lane);
    __syncthreads();
    const bool neg = negate && *negate;                      // `if (depth < 0).any()` is a whole-tensor test (psfnet.py:505)
    if (neg) d = -d;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        float fd = foc_dists[(size_t)b * S + s];
        if (neg) fd = -fd;
        render_slice<KS, CN>(tl, lane, act, C, d, fd, L, out + (((size_t)b * C * S + s) * H + y) * W + x0 + lane, (size_t)S * H * W);
    }
}

// d_depth [N,1,H,W] (sum over the slices in slice order, in registers) and foc_part [N*S][tiles]: one partial of d_foc per workgroup
// (tile = y * gridDim.x + blockIdx.x) from a fixed wave butterfly.  Either output may be NULL.
template <int KS, int CN>
__global__ __launch_bounds__(64) void thinlens_input_grad_kernel(const float* __restrict__ img, const float* __restrict__ depth,
                                                                  const float* __restrict__ foc_dists, const int* __restrict__ negate,
                                                                  const float* __restrict__ dy, float* __restrict__ d_depth,
                                                                  float* __restrict__ foc_part, int C, int S, int H, int W, Lens L) {
#pragma clang fp contract(off)
    constexpr int MC = CN > 0 ? CN : LP_MAXC;
    constexpr int TWD = LP_NPX + KS - 1;
    __shared__ float tl[MC * KS * TWD];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * LP_NPX, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(LP_NPX, W - x0);
    const bool act = lane < npx;
    const size_t pix = ((size_t)b * H + y) * W + x0 + (act ? lane : 0);
    float d = depth[pix];
    stage_window<KS, CN>(img, tl, b, C, H, W, y, x0, lane);
    __syncthreads();
    const bool neg = negate && *negate;
    const float sg = neg ? -1.f : 1.f;
    if (neg) d = -d;
    const bool inside = d >= L.d_min && d <= L.d_max;         // torch.clamp passes the gradient at equality
    const int tiles = gridDim.x * gridDim.y, tile = y * gridDim.x + blockIdx.x;
    float dd = 0.f;
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        float fd = foc_dists[(size_t)b * S + s];
        if (neg) fd = -fd;
        const Coc c = coc_of(d, fd, L);
        const float rad2 = c.rad2;
        float e[KS / 2 + 1];
        disc_factors<KS / 2>(e, rad2);
        float z = 0.f, zr = 0.f;                              // Z and sum w rho: registers only
#pragma unroll
        for (int u = 0; u < KS; ++u) {
#pragma unroll
            for (int v = 0; v < KS; ++v) {
                float rho;
                const float wv = disc_weight<KS / 2>(e, rad2, u, v, rho);
                z += wv;
                zr = fmaf(wv, rho, zr);
            }
        }
        const float inv = 1.f / z;
        const float rho_bar = zr * inv;
        float dyv[MC];
#pragma unroll
        for (int cc = 0; cc < MC; ++cc)
            dyv[cc] = (act && (CN > 0 || cc < C)) ? dy[(((size_t)(b * C + cc) * S + s) * H + y) * W + x0 + lane] : 0.f;
        float acc = 0.f;                                      // sum w (rho - rho_bar) g: exactly 0 when only the centre tap is inside
#pragma unroll
        for (int u = 0; u < KS; ++u) {
#pragma unroll
            for (int v = 0; v < KS; ++v) {
                float rho;
                const float wv = disc_weight<KS / 2>(e, rad2, u, v, rho);
                float g = 0.f;                                // head: sum_c dy[c] * img[c][clamp(y+u-p)][clamp(x+v-p)]
#pragma unroll
                for (int cc = 0; cc < MC; ++cc)
                    if (CN > 0 || cc < C) g = fmaf(dyv[cc], tl[(cc * KS + u) * TWD + lane + v], g);
                acc = fmaf(wv * (rho - rho_bar), g, acc);
            }
            __builtin_amdgcn_sched_barrier(0);                // one window row of LDS reads in flight, not all KS: registers
        }
        const float d_r = acc * inv / (c.rad * rad2);
        const float d_coc = c.cp >= 0.1f ? d_r * 0.5f * L.inv_ps : 0.f;      // clamp(min=0.1): gradient passes at equality
        const float diff = c.dc - fd;
        const float sgn = diff > 0.f ? 1.f : (diff < 0.f ? -1.f : 0.f);
        const float fm = fd - L.foc_len;
        const float af = L.a_coc * L.foc_len;
        const float dcoc_ddc = af / fm * sgn * fd / (c.dc * c.dc);
        const float dcoc_df = -af * (sgn / (c.dc * fm) + fabsf(diff) / (c.dc * fm * fm));
        const float term = inside ? sg * d_coc * dcoc_ddc : 0.f;
        dd += term;
        if (foc_part) {                                       // wave-uniform
            const float tot = wave_sum(act ? sg * d_coc * dcoc_df : 0.f);
            if (lane == 0) foc_part[((size_t)b * S + s) * tiles + tile] = tot;
        }
    }
    if (d_depth && act) d_depth[pix] = dd;
}

// d_foc[n][s] = sum of the workgroup partials of (n, s): one wave each, lane-strided double sums, fixed butterfly
__global__ __launch_bounds__(64) void thinlens_foc_sum_kernel(const float* __restrict__ part, float* __restrict__ d_foc, int tiles) {
    const float* p = part + (size_t)blockIdx.x * tiles;
    double a = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 64) a += (double)p[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, kWave);
    if (threadIdx.x == 0) d_foc[blockIdx.x] = (float)a;
}

// r^2 and 1 / Z of every row (n, slice, pixel): Z summed in the forward's tap order, so 1 / Z is the forward's normalisation
template <int KS>
__global__ __launch_bounds__(256) void thinlens_rows_kernel(const float* __restrict__ depth, const float* __restrict__ foc_dists,
                                                             const int* __restrict__ negate, float* __restrict__ rad2_rows,
                                                             float* __restrict__ invz_rows, size_t rows, int S, int hw, Lens L) {
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= rows) return;
    const size_t ns = i / hw;
    const int rem = (int)(i - ns * hw);
    const size_t n = ns / S;
    float d = depth[n * hw + rem], fd = foc_dists[ns];
    if (negate && *negate) { d = -d; fd = -fd; }
    const float rad2 = coc_of(d, fd, L).rad2;
    float e[KS / 2 + 1], rho;
    disc_factors<KS / 2>(e, rad2);
    float wsum = 0.f;
#pragma unroll
    for (int u = 0; u < KS; ++u) {
#pragma unroll
        for (int v = 0; v < KS; ++v) wsum += disc_weight<KS / 2>(e, rad2, u, v, rho);
    }
    rad2_rows[i] = rad2;
    invz_rows[i] = 1.f / wsum;
}

// d_img[n][c][Y][X] = sum over the slices (slice order, each slice summed from zero) of sum dy[n][c][s][y][x] * p_{s,(y,x)}[a][e] over the
// source pixels (y, x) and taps (a, e) with clamp(y+a-p) = Y and clamp(x+e-p) = X.  One 64-pixel run of row Y per workgroup; per (slice,
// source row) the lanes stage r^2, the 1-D Gaussian factors and dy / Z of the 64+KS-1 source columns in LDS, then gather.
template <int KS>
__global__ __launch_bounds__(64) void thinlens_dimg_kernel(const float* __restrict__ dy, const float* __restrict__ rad2_rows,
                                                            const float* __restrict__ invz_rows, float* __restrict__ d_img, int C, int S,
                                                            int H, int W) {
#pragma clang fp contract(off)
    constexpr int PAD = KS / 2, TWD = LP_NPX + KS - 1;
    __shared__ float s_r2[TWD], s_e[(PAD + 1) * TWD], s_b[LP_MAXC * TWD];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * LP_NPX, Y = blockIdx.y, n = blockIdx.z;
    const int X = x0 + lane;
    const bool act = X < W;
    const int y_lo = max(Y - PAD, 0), y_hi = min(Y + PAD, H - 1);
    const bool interior = x0 >= PAD && x0 + LP_NPX - 1 + PAD <= W - 1;      // wave-uniform: no lane at a border, no source outside
    float tot[LP_MAXC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        float part[LP_MAXC] = {0.f, 0.f, 0.f, 0.f};
#pragma unroll 1
        for (int y = y_lo; y <= y_hi; ++y) {
            __syncthreads();                                  // the previous row's readers are done
            for (int j = lane; j < TWD; j += LP_NPX) {
                const int xs = x0 - PAD + j;
                const bool valid = xs >= 0 && xs < W;         // every source pixel once: no clamped duplicates
                const size_t row = (((size_t)n * S + s) * H + y) * W + (valid ? xs : 0);
                const float r2 = valid ? rad2_rows[row] : 0.f;        // 0: no tap passes rho < r^2
                const float iz = valid ? invz_rows[row] : 0.f;
                s_r2[j] = r2;
#pragma unroll
                for (int k = 0; k <= PAD; ++k) s_e[k * TWD + j] = valid ? __expf((float)(-(k * k)) * 0.5f / r2) : 0.f;
#pragma unroll
                for (int cc = 0; cc < LP_MAXC; ++cc)
                    if (cc < C) s_b[cc * TWD + j] = valid ? dy[(((size_t)(n * C + cc) * S + s) * H + y) * W + xs] * iz : 0.f;
            }
            __syncthreads();
            const int a_lo = Y == 0 ? 0 : Y - y + PAD, a_hi = Y == H - 1 ? KS - 1 : Y - y + PAD;     // tap rows that clamp onto Y
#pragma unroll 1
            for (int a = a_lo; a <= a_hi; ++a) {
                const int du = a < PAD ? PAD - a : a - PAD;
                const float* eu = s_e + du * TWD;
                if (interior) {                               // every tap has exactly one source, all of them staged: no bounds
#pragma unroll
                    for (int e = 0; e < KS; ++e) {
                        const int dv = e < PAD ? PAD - e : e - PAD;
                        const float rho = (float)(du * du + dv * dv);
                        const int j = lane + 2 * PAD - e;
                        const float wv = rho < s_r2[j] ? eu[j] * s_e[dv * TWD + j] : 0.f;
#pragma unroll
                        for (int cc = 0; cc < LP_MAXC; ++cc)
                            if (cc < C) part[cc] = fmaf(s_b[cc * TWD + j], wv, part[cc]);
                    }
                    continue;
                }
#pragma unroll
                for (int e = 0; e < KS; ++e) {
                    const int dv = e < PAD ? PAD - e : e - PAD;
                    const float rho = (float)(du * du + dv * dv);
                    const int xs = X - e + PAD;               // tap columns that clamp onto X: one source, or a run at a border
                    int lo = X == 0 ? 0 : xs, hi = X == W - 1 ? W - 1 : xs;
                    lo = max(lo, 0);
                    hi = act ? min(hi, W - 1) : -1;
                    for (int x = lo; x <= hi; ++x) {
                        const int j = x - x0 + PAD;           // in [0, TWD): x0 - PAD <= x <= x0 + 63 + PAD
                        const float wv = rho < s_r2[j] ? eu[j] * s_e[dv * TWD + j] : 0.f;
#pragma unroll
                        for (int cc = 0; cc < LP_MAXC; ++cc)
                            if (cc < C) part[cc] = fmaf(s_b[cc * TWD + j], wv, part[cc]);
                    }
                }
            }
        }
#pragma unroll
        for (int cc = 0; cc < LP_MAXC; ++cc) tot[cc] += part[cc];
    }
    if (act) {
#pragma unroll
        for (int cc = 0; cc < LP_MAXC; ++cc)
            if (cc < C) d_img[((size_t)(n * C + cc) * H + Y) * W + X] = tot[cc];
    }
}

struct Plan { int tiles; size_t off_rad2, off_invz, off_part, bytes; };      // offsets in floats

static void plan_bwd(Plan& pl, int B, int S, int H, int W, bool need_img, bool need_foc) {
    const size_t rows = (size_t)B * S * H * W;
    pl.tiles = H * ((W + LP_NPX - 1) / LP_NPX);
    size_t o = 0;
    pl.off_rad2 = o;
    if (need_img) o += rows;
    pl.off_invz = o;
    if (need_img) o += rows;
    pl.off_part = o;
    if (need_foc) o += (size_t)B * S * pl.tiles;
    pl.bytes = o * sizeof(float);
}

static int check_sizes(const char* who, int B, int C, int S, int H, int W, int ks) {
    AADFF_CHECK_ARG(B > 0 && C > 0 && S > 0 && H > 0 && W > 0, "%s: empty tensor (B=%d C=%d S=%d H=%d W=%d)", who, B, C, S, H, W);
    AADFF_CHECK_ARG(C <= LP_MAXC, "%s: at most %d channels", who, LP_MAXC);
    AADFF_CHECK_ARG(ks == 3 || ks == 5 || ks == 7 || ks == 9 || ks == 11 || ks == 13, "%s: ks %d not in {3,5,...,13}", who, ks);
    AADFF_CHECK_ARG(H <= 65535 && B <= 65535, "%s: H or B too large for the launch grid", who);
    AADFF_CHECK_ARG((long)H * W < (1L << 30) && (long)B * S < (1L << 24) && (long)B * S * H * ((W + LP_NPX - 1) / LP_NPX) < (1L << 31) && (long)B * S * H * W < (1L << 38),
                    "%s: B=%d S=%d H=%d W=%d too large for one launch", who, B, S, H, W);
    return 0;
}

// KERNEL<ks, C == 3 ? 3 : 0> over grid `g`, one wave per 64-pixel run (3 channels compiled in, any other count on the run-time path)
#define AADFF_TL_CASE(KERNEL, K, ...) \
    case K: if (C == 3) hipLaunchKernelGGL((KERNEL<K, 3>), g, dim3(64), 0, st, __VA_ARGS__); \
            else hipLaunchKernelGGL((KERNEL<K, 0>), g, dim3(64), 0, st, __VA_ARGS__); break;
#define AADFF_TL_LAUNCH(KERNEL, ...) \
    switch (ks) { AADFF_TL_CASE(KERNEL, 3, __VA_ARGS__) AADFF_TL_CASE(KERNEL, 5, __VA_ARGS__) AADFF_TL_CASE(KERNEL, 7, __VA_ARGS__) \
                  AADFF_TL_CASE(KERNEL, 9, __VA_ARGS__) AADFF_TL_CASE(KERNEL, 11, __VA_ARGS__) AADFF_TL_CASE(KERNEL, 13, __VA_ARGS__) }

}  // namespace tlb
}  // namespace aadff

using namespace aadff;

extern "C" {

int aadff_thinlens_render(const float* img, const float* depth, const float* foc_dist, const int* negate_or_null, float* out,
                          int B, int C, int H, int W, int ks, float foc_len_over_fnum, float foc_len, float inv_pixel_size,
                          float d_min, float d_max, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && depth && foc_dist && out, "thinlens_render: NULL pointer");
    AADFF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "thinlens_render: empty tensor");
    AADFF_CHECK_ARG(C <= LP_MAXC, "thinlens_render: at most %d channels", LP_MAXC);
    AADFF_CHECK_ARG(ks == 3 || ks == 5 || ks == 7 || ks == 9 || ks == 11 || ks == 13, "thinlens_render: ks %d not in {3,5,...,13}", ks);
    AADFF_CHECK_ARG(H <= 65535 && B <= 65535, "thinlens_render: H or B too large for the launch grid");
    hipStream_t st = (hipStream_t)stream;
    const tlb::Lens L{foc_len_over_fnum, foc_len, inv_pixel_size, d_min, d_max};
    dim3 g((W + LP_NPX - 1) / LP_NPX, H, B);
    AADFF_TL_LAUNCH(tlb::thinlens_kernel, img, depth, foc_dist, negate_or_null, out, C, H, W, L);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_thinlens_render_stack(const float* img, const float* depth, const float* foc_dists, const int* negate_or_null, float* out,
                                int B, int C, int S, int H, int W, int ks, float foc_len_over_fnum, float foc_len, float inv_pixel_size,
                                float d_min, float d_max, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && depth && foc_dists && out, "thinlens_render_stack: NULL pointer");
    if (int rc = tlb::check_sizes("thinlens_render_stack", B, C, S, H, W, ks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    const tlb::Lens L{foc_len_over_fnum, foc_len, inv_pixel_size, d_min, d_max};
    dim3 g((W + LP_NPX - 1) / LP_NPX, H, B);
    AADFF_TL_LAUNCH(tlb::thinlens_stack_kernel, img, depth, foc_dists, negate_or_null, out, C, S, H, W, L);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_thinlens_render_stack_bwd_workspace(int B, int C, int S, int H, int W, int ks, int need_img, int need_foc, size_t* bytes) {
    AADFF_CHECK_ARG(bytes, "thinlens_render_stack_bwd_workspace: bytes is NULL");
    if (int rc = tlb::check_sizes("thinlens_render_stack_bwd_workspace", B, C, S, H, W, ks)) return rc;
    tlb::Plan pl;
    tlb::plan_bwd(pl, B, S, H, W, need_img != 0, need_foc != 0);
    *bytes = pl.bytes;
    return 0;
}

int aadff_thinlens_render_stack_bwd(const float* img, const float* depth, const float* foc_dists, const int* negate_or_null, const float* dy,
                                    float* d_img_or_null, float* d_depth_or_null, float* d_foc_or_null, void* workspace,
                                    size_t workspace_bytes, int B, int C, int S, int H, int W, int ks, float foc_len_over_fnum,
                                    float foc_len, float inv_pixel_size, float d_min, float d_max, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && depth && foc_dists && dy, "thinlens_render_stack_bwd: NULL pointer");
    AADFF_CHECK_ARG(d_img_or_null || d_depth_or_null || d_foc_or_null, "thinlens_render_stack_bwd: d_img, d_depth and d_foc are all NULL");
    if (int rc = tlb::check_sizes("thinlens_render_stack_bwd", B, C, S, H, W, ks)) return rc;
    const bool need_img = d_img_or_null != nullptr, need_foc = d_foc_or_null != nullptr;
    tlb::Plan pl;
    tlb::plan_bwd(pl, B, S, H, W, need_img, need_foc);
    AADFF_CHECK_ARG(pl.bytes == 0 || (workspace && workspace_bytes >= pl.bytes), "thinlens_render_stack_bwd: workspace of %zu bytes is too small, %zu needed",
                    workspace ? workspace_bytes : (size_t)0, pl.bytes);
    hipStream_t st = (hipStream_t)stream;
    float* ws = static_cast<float*>(workspace);
    const tlb::Lens L{foc_len_over_fnum, foc_len, inv_pixel_size, d_min, d_max};
    dim3 g((W + LP_NPX - 1) / LP_NPX, H, B);
    if (d_depth_or_null || need_foc) {
        float* part = need_foc ? ws + pl.off_part : nullptr;
        AADFF_TL_LAUNCH(tlb::thinlens_input_grad_kernel, img, depth, foc_dists, negate_or_null, dy, d_depth_or_null, part, C, S, H, W, L);
        AADFF_CHECK_LAUNCH();
        if (need_foc) {
            hipLaunchKernelGGL(tlb::thinlens_foc_sum_kernel, dim3((unsigned)(B * S)), dim3(64), 0, st, part, d_foc_or_null, pl.tiles);
            AADFF_CHECK_LAUNCH();
        }
    }
    if (need_img) {
        const size_t rows = (size_t)B * S * H * W;
        float* rad2_rows = ws + pl.off_rad2;
        float* invz_rows = ws + pl.off_invz;
        const dim3 gr((unsigned)((rows + 255) / 256));
#define AADFF_TL(K) case K: \
            hipLaunchKernelGGL((tlb::thinlens_rows_kernel<K>), gr, dim3(256), 0, st, depth, foc_dists, negate_or_null, rad2_rows, invz_rows, rows, S, H * W, L); \
            hipLaunchKernelGGL((tlb::thinlens_dimg_kernel<K>), g, dim3(64), 0, st, dy, rad2_rows, invz_rows, d_img_or_null, C, S, H, W); break;
        switch (ks) { AADFF_TL(3) AADFF_TL(5) AADFF_TL(7) AADFF_TL(9) AADFF_TL(11) AADFF_TL(13) }
#undef AADFF_TL
        AADFF_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
