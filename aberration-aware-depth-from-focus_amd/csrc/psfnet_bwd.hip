// Backward of the fused PSF-surrogate renderer for gfx950 (MI355X): gradients of the rendered RGB-D focal stack
// (aadff_psfnet_render_rgbd, csrc/psfnet.hip) to the depth map, the focus distances and the image.  What torch.autograd derives for
// the reference's deeplens/psfnet.py:393-450 (render, depth2z) over deeplens/psfnet_arch.py:24-47 (MLP, ReLU, Sigmoid, F.normalize
// p=1) and deeplens/render_psf.py:76-107 (per-pixel gather), without storing anything between forward and backward: a ReLU network
// needs one mask bit per hidden unit to back-propagate to its INPUT, so the kernel recomputes the forward and keeps the bits.
//
// psfnet_input_grad_kernel, workgroup = 64 rows (pixels of one (n, slice)) x 8 waves:
//   1. forward recompute: the arithmetic of psfnet_fused_kernel (same fragment order, same fp16 hi/lo operand split, same order of
//      the three products), so the masks belong to the PSFs the forward rendered.  A lane's write-back of a layer covers
//      2 tiles x 4 pixel tiles x 4 features = 32 hidden units: ONE 32-bit mask word per lane and layer, kept in LDS (2 KB per layer);
//      the backward GEMM's output fragment has the same shape, so the same lane reads its own word back.
//   2. head: s = sigmoid outputs, p = s / sum(s);  g_k = sum_c dy[c] img[c][clamp(y + a - pad)][clamp(x + e - pad)] from the staged
//      image window;  d_s_k = (g_k - sum_j g_j p_j) / sum(s);  d_a_k = d_s_k s_k (1 - s_k).
//   3. chain: layers n-1 .. 0, d_h_{l-1} = W_l^T (d_h_l . mask_l) on v_mfma_f32_16x16x32_f16 with the forward's three-product split;
//      the transposed weights come pre-packed in fragment order, every layer times a power of two that puts its largest weight in
//      [2^9, 2^10) (aadff/psfnet_pack.py), so that the lo halves of small weights stay normal fp16 numbers.
//      Scaling: gradients are ~1e-7 and smaller, below fp16's normal range.  Every row carries a power-of-two scale, renewed after
//      every layer so that the row's largest magnitude lies in [2^7, 2^8) before the split (the chain is linear in the row), and
//      undone once at the end.  Exact: powers of two.
//      Bias: the matrix core aligns the products of an instruction to the largest addend, the accumulator included, and cuts the
//      bits below - towards minus infinity, whatever the sign (measured: the chain is not odd in dy, and (f(dy) - f(-dy)) / 2 is
//      20x closer to float64).  Per row that is ~2^-24 of the row's size and invisible; summed over the rows it does not average
//      out, and d_foc_z is a sum of terms that cancel to a few thousandths of their size (8e-6 .. 1e-4 relative error, 8 .. 14 x the
//      budget).  Two measures, neither costs an instruction on the matrix cores: (i) the small products hi*lo and lo*hi go to an
//      accumulator of their own, which is added to the main one in fp32 at the end of the k-loop (they are then cut relative to
//      their own size, 2^-11 of the row's: the bias drops 6x and the rows come out closer to float64 than torch's fp32 does);
//      (ii) the rows of a checkerboard in (x + y) run through the chain with their sign flipped, which is undone with the scale,
//      so what is left of the bias enters neighbouring rows with opposite signs and cancels in sums over the rows.
//      The forward recompute does neither: it has to reproduce the forward kernel's bits.
//   4. outputs: component 2 of layer 0's input gradient times the derivative of depth2z -> d_z row (n, slice, y, x);
//      component 3 summed over the workgroup's rows (fixed butterfly) -> one partial per workgroup.
// psfnet_grad_reduce kernels add the slices of a pixel in slice order and the partials of a (n, slice) in a fixed order (double).
// No float atomics: bitwise reproducible from run to run.
//
// d_img (only when asked for): per (n, slice) the PSFs of the forward (aadff_psfnet_forward, mode 0) into a workspace of ONE slice,
// then the adjoint of the gather, accumulated over the slices in slice order.
#include <algorithm>
#include <cmath>
#include <type_traits>
#include "common.h"
#include "gather_window.h"
#include "psfnet_common.h"

namespace aadff {
namespace pnb {

using namespace pn;                     // workgroup shape, activation layout and operand split of the forward (psfnet_common.h)

constexpr int TP = 64;                  // rows per workgroup
constexpr int NPT = TP / 16;            // pixel tiles
constexpr int PP = 132;                 // floats per row of the fp32 sigmoid outputs
constexpr int PLANE = TP * AP;
constexpr int MAXKS = 11;               // n_out <= 128

struct Layers {
    int n;
    int kpad[MAXL], npad[MAXL], woff[MAXL], boff[MAXL];        // forward pack (psfnet.hip)
    int tkpad[MAXL], tnpad[MAXL], twoff[MAXL];                 // transposed pack: K = out_features (pad 32), N = in_features (pad 16)
    int texp;                                                  // sum of the transposed pack's per-layer power-of-two exponents
};

// out^T[feat][px] (+)= sum_k A[feat][k] B[px][k] for this wave's NTL feature tiles (wave, wave + 8) and all TP pixels: the k-loop of
// psfnet_fused_kernel (weights streamed two k-steps ahead, products hi*hi, hi*lo, lo*hi in that order).
template <int NTL, bool SEP = false>
__device__ __forceinline__ void gemm_tiles(float4v (&acc)[2][NPT], const uint4v* __restrict__ wl, int nks, const _Float16* a0, const _Float16* a1,
                                           int wave, int lane, int kg, int lo4) {
    const uint4v* wq[2];
    uint4v ah[2], al[2], nh[2], nl[2];
    float4v small[2][NPT];
    if constexpr (SEP) {
#pragma unroll
        for (int j = 0; j < NTL; ++j)
#pragma unroll
            for (int p = 0; p < NPT; ++p) small[j][p] = (float4v){0.f, 0.f, 0.f, 0.f};
    }
#pragma unroll
    for (int j = 0; j < NTL; ++j) {
        wq[j] = wl + ((size_t)(wave + NWV * j) * nks * 2) * 64 + lane;
        ah[j] = wq[j][0];
        al[j] = wq[j][64];
        const int s1 = nks > 1 ? 1 : 0;
        nh[j] = wq[j][s1 * 128];
        nl[j] = wq[j][s1 * 128 + 64];
    }
#pragma unroll 1
    for (int s = 0; s < nks; ++s) {
        half8v th[2], tl[2];
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            th[j] = __builtin_bit_cast(half8v, ah[j]);
            ah[j] = nh[j];
            tl[j] = __builtin_bit_cast(half8v, al[j]);
            al[j] = nl[j];
        }
        const int s2 = s + 2 < nks ? s + 2 : nks - 1;
#pragma unroll
        for (int j = 0; j < NTL; ++j) {
            nh[j] = wq[j][s2 * 128];
            nl[j] = wq[j][s2 * 128 + 64];
        }
        const int boffs = swz(lo4, 32 * s + 8 * kg);
#pragma unroll
        for (int p = 0; p < NPT; ++p) {
            const half8v bh = *reinterpret_cast<const half8v*>(&a0[16 * p * AP + boffs]);
            const half8v bl = *reinterpret_cast<const half8v*>(&a1[16 * p * AP + boffs]);
#pragma unroll
            for (int j = 0; j < NTL; ++j) {
                acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(th[j], bh, acc[j][p], 0, 0, 0);
                if constexpr (SEP) {
                    small[j][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(th[j], bl, small[j][p], 0, 0, 0);
                    small[j][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tl[j], bh, small[j][p], 0, 0, 0);
                } else {
                    acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(th[j], bl, acc[j][p], 0, 0, 0);
                    acc[j][p] = __builtin_amdgcn_mfma_f32_16x16x32_f16(tl[j], bh, acc[j][p], 0, 0, 0);
                }
            }
        }
    }
    if constexpr (SEP) {
#pragma unroll
        for (int j = 0; j < NTL; ++j)
#pragma unroll
            for (int p = 0; p < NPT; ++p) acc[j][p] += small[j][p];
    }
}

// Power-of-two exponent k that brings a row maximum m >= 0 into [2^7, 2^8); 0 (scale 1) for zero, subnormal, huge or NaN rows.
__device__ __forceinline__ int scale_exp(float m) {
    const int e = (int)(__builtin_bit_cast(unsigned, m) >> 23) - 127;
    return (e < -100 || e > 100) ? 0 : 7 - e;
}
__device__ __forceinline__ float pow2i(int k) { return __builtin_bit_cast(float, (unsigned)(k + 127) << 23); }    // k in [-126, 127]

__global__ __launch_bounds__(NTH, 2) void psfnet_input_grad_kernel(const uint4v* __restrict__ wpack, const float* __restrict__ bias,
                                                                   const uint4v* __restrict__ wtpack, Layers L, int nout,
                                                                   const float* __restrict__ img, const float* __restrict__ dy, int C, int H, int W,
                                                                   int ks, int S, int tiles, Coord coord, float* __restrict__ dz_rows,
                                                                   float* __restrict__ dfoc_part) {
    __shared__ __attribute__((aligned(16))) _Float16 act_raw[2 * PLANE];       // [hi | lo]; the fp32 sigmoid outputs + image window in between
    __shared__ unsigned masks[(MAXL - 1) * NTH];                                // ReLU mask word of (layer, thread)
    __shared__ float rowmax[NWV * TP];                                          // per-wave row maxima of a layer; d_foc_z rows at the end
    __shared__ int rowexp[TP];                                                  // accumulated power-of-two scale of every row
    _Float16* const act0 = act_raw;
    _Float16* const act1 = act_raw + PLANE;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int kg = lane >> 4, lo4 = lane & 15;
    const int hw = H * W;
    const int ns = blockIdx.x / tiles, tile = blockIdx.x - ns * tiles;          // (n, slice) = n * S + slice
    const int n = ns / S, sl = ns - n * S;
    const int rem0 = tile * TP;
    const int nvalid = min(TP, hw - rem0);                                      // rows of this workgroup inside the slice

    // ---- layer-0 input: (xs[x], ys[y], depth2z(depth), foc_z), zero-padded to 32 ----
    for (int e = tid; e < TP * 8; e += NTH) {
        const int px = e >> 3, g4 = e & 7;
        float4v v = {0.f, 0.f, 0.f, 0.f};
        if (g4 == 0 && px < nvalid) {
            const int rem = rem0 + px;
            const int yy = rem / W, xx = rem - yy * W;
            const float z = fminf(fmaxf((coord.depth[(size_t)n * hw + rem] - coord.d_min) * coord.inv_range, 0.f), 1.f);
            v = (float4v){coord.xs[xx], coord.ys[yy], z, coord.foc_z[ns]};
        }
        half4v h, l;
        split4(v, h, l);
        *reinterpret_cast<half4v*>(&act0[swz(px, 4 * g4)]) = h;
        *reinterpret_cast<half4v*>(&act1[swz(px, 4 * g4)]) = l;
    }
    __syncthreads();

    float4v acc[2][NPT];
    // ---- 1. forward recompute (psfnet_fused_kernel), keeping the ReLU masks ----
#pragma unroll 1
    for (int l = 0; l < L.n; ++l) {
        const int nks = L.kpad[l] >> 5, ntile = L.npad[l] >> 4;
        const bool t0 = wave < ntile, t1 = wave + NWV < ntile;
        const bool last = l == L.n - 1;
#pragma unroll
        for (int j = 0; j < 2; ++j) {
            const float4v b = (j == 0 ? t0 : t1) ? *reinterpret_cast<const float4v*>(bias + L.boff[l] + 16 * (wave + NWV * j) + 4 * kg)
                                                 : (float4v){0.f, 0.f, 0.f, 0.f};
#pragma unroll
            for (int p = 0; p < NPT; ++p) acc[j][p] = b;
        }
        if (t1) gemm_tiles<2>(acc, wpack + L.woff[l], nks, act0, act1, wave, lane, kg, lo4);
        else if (t0) gemm_tiles<1>(acc, wpack + L.woff[l], nks, act0, act1, wave, lane, kg, lo4);
        __syncthreads();
        if (!last) {
            unsigned mw = 0;
            if (t0) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 1 && !t1) break;
                    const int f0 = 16 * (wave + NWV * j) + 4 * kg;
#pragma unroll
                    for (int p = 0; p < NPT; ++p) {
                        float4v v = acc[j][p];
#pragma unroll
                        for (int i = 0; i < 4; ++i) {
                            mw |= v[i] > 0.f ? 1u << (16 * j + 4 * p + i) : 0u;
                            v[i] = fmaxf(v[i], 0.f);
                        }
                        half4v h, lo;
                        split4(v, h, lo);
                        const int o = swz(16 * p + lo4, f0);
                        *reinterpret_cast<half4v*>(&act0[o]) = h;
                        *reinterpret_cast<half4v*>(&act1[o]) = lo;
                    }
                }
            }
            masks[l * NTH + tid] = mw;
            const int kn = L.kpad[l + 1], nn = L.npad[l];
            if (kn > nn) {
                const int gw = (kn - nn) >> 2;
                for (int e = tid; e < TP * gw; e += NTH) {
                    const int px = e / gw, g4 = e - px * gw;
                    *reinterpret_cast<half4v*>(&act0[swz(px, nn + 4 * g4)]) = (half4v){0, 0, 0, 0};
                    *reinterpret_cast<half4v*>(&act1[swz(px, nn + 4 * g4)]) = (half4v){0, 0, 0, 0};
                }
            }
        } else {
            float* psf = reinterpret_cast<float*>(act_raw);
            if (t0) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 1 && !t1) break;
                    const int f0 = 16 * (wave + NWV * j) + 4 * kg;
#pragma unroll
                    for (int p = 0; p < NPT; ++p) {
                        float4v v = acc[j][p];
#pragma unroll
                        for (int i = 0; i < 4; ++i) v[i] = 1.f / (1.f + expf(-v[i]));
                        *reinterpret_cast<float4v*>(&psf[(16 * p + lo4) * PP + f0]) = v;
                    }
                }
            }
        }
        __syncthreads();
    }

    // ---- 2. head: 8 threads per row; thread q takes taps q, q + 8, ... ----
    {
        const float* psf = reinterpret_cast<const float*>(act_raw);
        float* win = reinterpret_cast<float*>(act_raw) + TP * PP;              // [C][ks][TP + ks - 1], behind the sigmoid outputs
        constexpr int TPP = NTH / TP, NT = 128 / TPP;                           // 8 threads per row, 16 taps per thread
        const int px = tid / TPP, q = tid % TPP;
        const bool valid = px < nvalid;
        const int rem = rem0 + min(px, nvalid - 1);
        const int y = rem / W, x = rem - y * W;
        const int pad = ks >> 1, ww = TP + ks - 1;
        const int y0 = rem0 / W, xs0 = rem0 - y0 * W;
        // <= 3 channels and all TP rows inside one image row (workgroup-uniform): the image window is staged once
        const bool row_tile = C <= 3 && nvalid == TP && xs0 + TP <= W;
        if (row_tile) {
            for (int e = tid; e < C * ks * ww; e += NTH) {
                const int cu = e / ww, col = e - cu * ww;
                const int c = cu / ks, u = cu - c * ks;
                const int yy = min(max(y0 + u - pad, 0), H - 1), xx = min(max(xs0 + col - pad, 0), W - 1);
                win[e] = img[((size_t)n * C + c) * hw + (size_t)yy * W + xx];
            }
            __syncthreads();
        }
        const float* row = psf + px * PP;
        const float* dyp = dy + (((size_t)n * C) * S + sl) * hw + rem;          // channel c: + c * S * hw
        float sv[NT], g[NT];
        float sum = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            const int t = q + TPP * i;
            sv[i] = t < nout ? row[t] : 0.f;
            sum += sv[i];
            g[i] = 0.f;
        }
#pragma unroll
        for (int m = 1; m < TPP; m <<= 1) sum += __shfl_xor(sum, m, kWave);
        if (row_tile) {
            float dv[3];
#pragma unroll
            for (int c = 0; c < 3; ++c) dv[c] = c < C ? dyp[(size_t)c * S * hw] : 0.f;
#pragma unroll
            for (int i = 0; i < NT; ++i) {
                const int t = q + TPP * i;
                if (t < nout) {
                    const int u = t / ks, v = t - u * ks;
                    float a = 0.f;
#pragma unroll
                    for (int c = 0; c < 3; ++c)
                        if (c < C) a = fmaf(dv[c], win[(c * ks + u) * ww + px + v], a);
                    g[i] = a;
                }
            }
        } else if (valid) {
            for (int c = 0; c < C; ++c) {
                const float dv = dyp[(size_t)c * S * hw];
                const float* plane = img + ((size_t)n * C + c) * hw;
#pragma unroll
                for (int i = 0; i < NT; ++i) {
                    const int t = q + TPP * i;
                    if (t < nout) {
                        const int u = t / ks, v = t - u * ks;
                        g[i] = fmaf(dv, plane[(size_t)min(max(y + u - pad, 0), H - 1) * W + min(max(x + v - pad, 0), W - 1)], g[i]);
                    }
                }
            }
        }
        // p = s * inv, inv = 1 / max(sum, 1e-12) (F.normalize): d_s_k = (g_k - sum_j g_j p_j) * inv; below the eps the norm is the constant
        const float inv = 1.f / fmaxf(sum, 1e-12f);
        float dot = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i) dot = fmaf(g[i], sv[i], dot);
#pragma unroll
        for (int m = 1; m < TPP; m <<= 1) dot += __shfl_xor(dot, m, kWave);
        dot = sum > 1e-12f ? dot * inv : 0.f;
        float amax = 0.f;
#pragma unroll
        for (int i = 0; i < NT; ++i) {
            g[i] = valid ? (g[i] - dot) * inv * (sv[i] * (1.f - sv[i])) : 0.f;   // d_a_k (sv = 0 beyond n_out)
            amax = fmaxf(amax, fabsf(g[i]));
        }
#pragma unroll
        for (int m = 1; m < TPP; m <<= 1) amax = fmaxf(amax, __shfl_xor(amax, m, kWave));
        const int k = scale_exp(amax);
        const float f = ((x + y) & 1) ? -pow2i(k) : pow2i(k);                   // checkerboard sign, see the header comment
        if (q == 0) rowexp[px] = k;
        __syncthreads();                                                        // every thread is done with the sigmoid outputs and the window
#pragma unroll
        for (int i = 0; i < NT; ++i) {                                          // features q + 8 i < 128 = K padding of the last layer's transpose
            const float v = g[i] * f;
            const _Float16 h = (_Float16)v;
            const int o = swz(px, q + TPP * i);
            act0[o] = h;
            act1[o] = (_Float16)(v - (float)h);
        }
        __syncthreads();
    }

    // ---- 3. backward chain: d_h_{l-1} = W_l^T (d_a_l), d_a_{l-1} = d_h_{l-1} . mask_{l-1}, rescaled per row ----
#pragma unroll 1
    for (int l = L.n - 1; l >= 0; --l) {
        const int nks = L.tkpad[l] >> 5, ntile = L.tnpad[l] >> 4;
        const bool t0 = wave < ntile, t1 = wave + NWV < ntile;
#pragma unroll
        for (int j = 0; j < 2; ++j)
#pragma unroll
            for (int p = 0; p < NPT; ++p) acc[j][p] = (float4v){0.f, 0.f, 0.f, 0.f};
        if (t1) gemm_tiles<2, true>(acc, wtpack + L.twoff[l], nks, act0, act1, wave, lane, kg, lo4);
        else if (t0) gemm_tiles<1, true>(acc, wtpack + L.twoff[l], nks, act0, act1, wave, lane, kg, lo4);
        __syncthreads();                                                        // every wave is done reading d_a_l
        if (l > 0) {
            const unsigned mw = masks[(l - 1) * NTH + tid];
            float pm[NPT];
#pragma unroll
            for (int p = 0; p < NPT; ++p) {
                float m = 0.f;
#pragma unroll
                for (int j = 0; j < 2; ++j)
#pragma unroll
                    for (int i = 0; i < 4; ++i) {
                        const float v = (mw >> (16 * j + 4 * p + i)) & 1u ? acc[j][p][i] : 0.f;
                        acc[j][p][i] = v;
                        m = fmaxf(m, fabsf(v));
                    }
                m = fmaxf(m, __shfl_xor(m, 16, kWave));
                m = fmaxf(m, __shfl_xor(m, 32, kWave));
                pm[p] = m;
            }
            if (kg == 0) {
#pragma unroll
                for (int p = 0; p < NPT; ++p) rowmax[wave * TP + 16 * p + lo4] = pm[p];
            }
            __syncthreads();
#pragma unroll
            for (int p = 0; p < NPT; ++p) {
                float m = 0.f;
#pragma unroll
                for (int w = 0; w < NWV; ++w) m = fmaxf(m, rowmax[w * TP + 16 * p + lo4]);
                const int k = scale_exp(m);
                if (wave == 0 && kg == 0) rowexp[16 * p + lo4] += k;
                pm[p] = pow2i(k);
            }
            if (t0) {
#pragma unroll
                for (int j = 0; j < 2; ++j) {
                    if (j == 1 && !t1) break;
                    const int f0 = 16 * (wave + NWV * j) + 4 * kg;
#pragma unroll
                    for (int p = 0; p < NPT; ++p) {
                        half4v h, lo;
                        split4(acc[j][p] * pm[p], h, lo);
                        const int o = swz(16 * p + lo4, f0);
                        *reinterpret_cast<half4v*>(&act0[o]) = h;
                        *reinterpret_cast<half4v*>(&act1[o]) = lo;
                    }
                }
            }
            const int kn = L.tkpad[l - 1], nn = L.tnpad[l];
            if (kn > nn) {
                const int gw = (kn - nn) >> 2;
                for (int e = tid; e < TP * gw; e += NTH) {
                    const int px = e / gw, g4 = e - px * gw;
                    *reinterpret_cast<half4v*>(&act0[swz(px, nn + 4 * g4)]) = (half4v){0, 0, 0, 0};
                    *reinterpret_cast<half4v*>(&act1[swz(px, nn + 4 * g4)]) = (half4v){0, 0, 0, 0};
                }
            }
            __syncthreads();
        } else {
            // ---- 4. layer 0: rows 0..3 of tile 0 are the gradients of (x, y, z, foc_z); wave 0, lanes kg == 0 hold them ----
            if (wave == 0 && kg == 0) {
#pragma unroll
                for (int p = 0; p < NPT; ++p) {
                    const int px = 16 * p + lo4;
                    float sc = ldexpf(1.f, -(rowexp[px] + L.texp));
                    float dfz = 0.f;
                    if (px < nvalid) {
                        const int rem = rem0 + px;
                        if ((rem / W + rem % W) & 1) sc = -sc;
                        const float zr = (coord.depth[(size_t)n * hw + rem] - coord.d_min) * coord.inv_range;
                        // autograd of torch.clamp(min=0, max=1): the gradient passes on [0, 1], bounds included
                        dz_rows[(size_t)ns * hw + rem] = (zr >= 0.f && zr <= 1.f) ? acc[0][p][2] * sc * coord.inv_range : 0.f;
                        dfz = acc[0][p][3] * sc;
                    }
                    rowmax[px] = dfz;
                }
            }
            __syncthreads();
            if (wave == 0) {
                const float tot = wave_sum(rowmax[lane]);                       // TP == 64: one row per lane, fixed butterfly
                if (lane == 0) dfoc_part[(size_t)ns * tiles + tile] = tot;
            }
        }
    }
}

// d_depth[n][y][x] = sum over the slices, in slice order
__global__ __launch_bounds__(256) void psfnet_grad_depth_sum_kernel(const float* __restrict__ dz_rows, float* __restrict__ d_depth, long N, int S, int hw) {
    const long i = (long)blockIdx.x * 256 + threadIdx.x;
    if (i >= N * hw) return;
    const long n = i / hw;
    const int rem = (int)(i - n * hw);
    float a = 0.f;
    for (int s = 0; s < S; ++s) a += dz_rows[((size_t)n * S + s) * hw + rem];
    d_depth[i] = a;
}

// d_foc_z[n][s] = sum of the workgroup partials of (n, s): one wave each, lane-strided double sums, fixed butterfly
__global__ __launch_bounds__(64) void psfnet_grad_foc_sum_kernel(const float* __restrict__ part, float* __restrict__ d_foc_z, int tiles) {
    const float* p = part + (size_t)blockIdx.x * tiles;
    double a = 0.0;
    for (int t = threadIdx.x; t < tiles; t += 64) a += (double)p[t];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) a += __shfl_xor(a, off, kWave);
    if (threadIdx.x == 0) d_foc_z[blockIdx.x] = (float)a;
}

// network input rows of one (n, slice) for aadff_psfnet_forward (the rows psfnet_fused_kernel generates from the depth map)
__global__ __launch_bounds__(256) void psfnet_rows_kernel(Coord coord, long n, long ns, int H, int W, float* __restrict__ rows) {
    const int rem = blockIdx.x * 256 + threadIdx.x;
    if (rem >= H * W) return;
    const int yy = rem / W, xx = rem - yy * W;
    const float z = fminf(fmaxf((coord.depth[(size_t)n * H * W + rem] - coord.d_min) * coord.inv_range, 0.f), 1.f);
    *reinterpret_cast<float4v*>(rows + (size_t)rem * 4) = (float4v){coord.xs[xx], coord.ys[yy], z, coord.foc_z[ns]};
}

// Adjoint of the per-pixel gather for one (n, slice): gather_adjoint (gather_window.h) with the stack's dy strides, added to d_img
// when `accumulate`: the slices are launched in slice order on one stream, so the sum over the slices has a fixed order.
__global__ __launch_bounds__(64) void psfnet_dimg_kernel(const float* __restrict__ psf, const float* __restrict__ dy, size_t dy_cstride,
                                                         float* __restrict__ dimg, int C, int H, int W, int ks, int accumulate) {
    const size_t hw = (size_t)H * W;
    if (accumulate) gather_adjoint<true>(psf, dy, dy_cstride, dimg, hw, C, H, W, ks);
    else gather_adjoint<false>(psf, dy, dy_cstride, dimg, hw, C, H, W, ks);
}

struct Plan { int tiles; size_t off_part, off_rows, off_psf, bytes; };       // offsets in floats

static void plan_bwd(Plan& pl, long N, int S, int H, int W, int ks, bool need_input, bool need_img) {
    const size_t hw = (size_t)H * W;
    pl.tiles = (int)((hw + TP - 1) / TP);
    size_t o = 0;
    if (need_input) o += (size_t)N * S * hw;                                    // d_z rows
    pl.off_part = o;
    if (need_input) o += (size_t)N * S * pl.tiles;                              // d_foc_z partials
    o = (o + 3) / 4 * 4;
    pl.off_rows = o;
    if (need_img) o += hw * 4;                                                  // network input rows of one slice
    pl.off_psf = o;
    if (need_img) o += hw * ks * ks;                                            // PSFs of one slice
    pl.bytes = o * sizeof(float);
}

static int check_sizes(const char* who, long N, int S, int C, int H, int W, int ks) {
    AADFF_CHECK_ARG(N >= 1 && S >= 1 && C >= 1 && H >= 1 && W >= 1, "%s: empty tensor (N=%ld S=%d C=%d H=%d W=%d)", who, N, S, C, H, W);
    AADFF_CHECK_ARG(ks >= 1 && ks <= MAXKS && ks % 2 == 1, "%s: ks %d should be odd and <= %d", who, ks, MAXKS);
    AADFF_CHECK_ARG((long)H * W < (1L << 30) && N * S < (1L << 24) && N * S * (((long)H * W + TP - 1) / TP) < (1L << 31) && H <= 65535,
                    "%s: N=%ld S=%d H=%d W=%d too large for one launch", who, N, S, H, W);
    return 0;
}

}  // namespace pnb
}  // namespace aadff

using namespace aadff;

extern "C" {

int aadff_psfnet_render_rgbd_bwd_workspace(long N, int S, int C, int H, int W, int ks, int need_input, int need_img, size_t* bytes) {
    AADFF_CHECK_ARG(bytes, "psfnet_render_rgbd_bwd_workspace: bytes is NULL");
    if (int rc = pnb::check_sizes("psfnet_render_rgbd_bwd_workspace", N, S, C, H, W, ks)) return rc;
    pnb::Plan pl;
    pnb::plan_bwd(pl, N, S, H, W, ks, need_input != 0, need_img != 0);
    *bytes = pl.bytes;
    return 0;
}

int aadff_psfnet_render_rgbd_bwd(const float* depth, const float* xs, const float* ys, const float* foc_z, float d_min, float inv_range, long N,
                                 int S, const void* wpack, const float* bias, const void* wtpack, const int* wt_exp, int n_layers,
                                 const int* in_features, const int* out_features, const float* img, const float* dy, int C, int H, int W, int ks,
                                 float* d_img_or_null, float* d_depth_or_null, float* d_foc_z_or_null, void* workspace,
                                 size_t workspace_bytes, aadff_stream_t stream) {
    AADFF_CHECK_ARG(depth && xs && ys && foc_z && wpack && bias && in_features && out_features && img && dy, "psfnet_render_rgbd_bwd: NULL pointer");
    AADFF_CHECK_ARG(d_img_or_null || d_depth_or_null || d_foc_z_or_null, "psfnet_render_rgbd_bwd: d_img, d_depth and d_foc_z are all NULL");
    if (int rc = pnb::check_sizes("psfnet_render_rgbd_bwd", N, S, C, H, W, ks)) return rc;
    const bool need_input = d_depth_or_null || d_foc_z_or_null, need_img = d_img_or_null != nullptr;
    AADFF_CHECK_ARG(!need_input || (wtpack && wt_exp), "psfnet_render_rgbd_bwd: NULL transposed weight pack");
    AADFF_CHECK_ARG(n_layers >= 1 && n_layers <= AADFF_PSFNET_MAX_LAYERS, "psfnet_render_rgbd_bwd: %d layers outside [1,%d]", n_layers, AADFF_PSFNET_MAX_LAYERS);
    pnb::Layers L;
    std::memset(&L, 0, sizeof(L));
    L.n = n_layers;
    int woff = 0, boff = 0, twoff = 0;
    for (int l = 0; l < n_layers; ++l) {
        const int k = in_features[l], n = out_features[l];
        AADFF_CHECK_ARG(k >= 1 && k <= 256 && n >= 1 && n <= 256, "psfnet_render_rgbd_bwd: layer %d is %d -> %d, widths above 256 are not supported", l, k, n);
        AADFF_CHECK_ARG(l == 0 ? k == 4 : k == out_features[l - 1], "psfnet_render_rgbd_bwd: layer %d input width %d does not chain", l, k);
        L.kpad[l] = (k + 31) / 32 * 32;
        L.npad[l] = (n + 15) / 16 * 16;
        L.woff[l] = woff;
        L.boff[l] = boff;
        woff += (L.npad[l] / 16) * (L.kpad[l] / 32) * 2 * 64;
        boff += L.npad[l];
        L.tkpad[l] = (n + 31) / 32 * 32;
        L.tnpad[l] = (k + 15) / 16 * 16;
        L.twoff[l] = twoff;
        twoff += (L.tnpad[l] / 16) * (L.tkpad[l] / 32) * 2 * 64;
        if (need_input) {
            AADFF_CHECK_ARG(wt_exp[l] >= -64 && wt_exp[l] <= 64, "psfnet_render_rgbd_bwd: scale exponent %d of layer %d outside [-64,64]", wt_exp[l], l);
            L.texp += wt_exp[l];
        }
    }
    const int nout = out_features[n_layers - 1];
    AADFF_CHECK_ARG(nout == ks * ks && nout <= 128, "psfnet_render_rgbd_bwd: ks %d does not match %d outputs (ks^2 <= 128)", ks, nout);
    pnb::Plan pl;
    pnb::plan_bwd(pl, N, S, H, W, ks, need_input, need_img);
    AADFF_CHECK_ARG(pl.bytes == 0 || (workspace && workspace_bytes >= pl.bytes), "psfnet_render_rgbd_bwd: workspace of %zu bytes is too small, %zu needed",
                    workspace ? workspace_bytes : (size_t)0, pl.bytes);

    hipStream_t st = (hipStream_t)stream;
    float* ws = static_cast<float*>(workspace);
    const pnb::Coord coord{depth, xs, ys, foc_z, d_min, inv_range};
    const int hw = H * W;
    if (need_input) {
        float* dz_rows = ws;
        float* part = ws + pl.off_part;
        hipLaunchKernelGGL(pnb::psfnet_input_grad_kernel, dim3((unsigned)(N * S * pl.tiles)), dim3(pnb::NTH), 0, st,
                           reinterpret_cast<const pnb::uint4v*>(wpack), bias, reinterpret_cast<const pnb::uint4v*>(wtpack), L, nout, img, dy, C, H, W,
                           ks, S, pl.tiles, coord, dz_rows, part);
        AADFF_CHECK_LAUNCH();
        if (d_depth_or_null) {
            hipLaunchKernelGGL(pnb::psfnet_grad_depth_sum_kernel, dim3((unsigned)((N * hw + 255) / 256)), dim3(256), 0, st, dz_rows, d_depth_or_null, N, S, hw);
            AADFF_CHECK_LAUNCH();
        }
        if (d_foc_z_or_null) {
            hipLaunchKernelGGL(pnb::psfnet_grad_foc_sum_kernel, dim3((unsigned)(N * S)), dim3(64), 0, st, part, d_foc_z_or_null, pl.tiles);
            AADFF_CHECK_LAUNCH();
        }
    }
    if (need_img) {
        float* rows = ws + pl.off_rows;
        float* psf = ws + pl.off_psf;
        for (long n = 0; n < N; ++n)
            for (int s = 0; s < S; ++s) {
                hipLaunchKernelGGL(pnb::psfnet_rows_kernel, dim3((unsigned)((hw + 255) / 256)), dim3(256), 0, st, coord, n, n * S + s, H, W, rows);
                AADFF_CHECK_LAUNCH();
                if (int rc = aadff_psfnet_forward(rows, hw, wpack, bias, n_layers, in_features, out_features, 0, psf, nullptr, nullptr, 0, 0, 0, 0, 0, 0,
                                                  nullptr, stream))
                    return rc;
                hipLaunchKernelGGL(pnb::psfnet_dimg_kernel, dim3((W + 63) / 64, H), dim3(64), 0, st, psf, dy + (((size_t)n * C) * S + s) * hw,
                                   (size_t)S * hw, d_img_or_null + (size_t)n * C * hw, C, H, W, ks, s > 0 ? 1 : 0);
                AADFF_CHECK_LAUNCH();
            }
    }
    return 0;
}

}  // extern "C"
