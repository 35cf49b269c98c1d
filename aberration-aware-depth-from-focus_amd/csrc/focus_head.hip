// Differentiable depth head over a focal stack and its loss: the attention stage and the loss of the reference's
// AiFDepthNet (dff/AiFNet.py:376-434, 450-584) without the [B,.,S,H,W] temporaries of the torch composition.
//
//   head_fwd<CA, VEC>    scores [N,K,S,H,W], stack [N,Ct,S,H,W], foc [N,S] -> depth [N,1,H,W] = sum_s pd_s foc_s, aif [N,CA,H,W] =
//                        sum_s pa_s stack[:, :CA].  A thread owns four neighbouring pixels of a row (16-byte accesses with VEC, the same
//                        arithmetic element by element without).  Two loops over S: the first finds the normaliser of each attention
//                        (softmax: the maximum; normalised softplus: T = sum softplus), the second forms the weights and the sums.
//   head_bwd<CA, VEC>    recomputes the attention from the scores (nothing is kept from the forward), then a third loop writes
//                        d_scores, d_stack and per-wave partial sums of d_foc; final_sum adds the partials in a fixed order.
//   loss_sums / loss_bwd the six sums of the loss (masked |e|, mask count, masked e^2, |aif - gt|, the two edge-aware smoothness sums)
//                        as per-workgroup float64 partials plus a fixed-order final sum, and the gradients to depth and aif.
// No atomics anywhere: every output is bit-identical from run to run and independent of which gradients are asked for.  fp contraction
// is off so that the shared (K = 1) and the separate (K = 2) attention take the same rounded steps.
#include "common.h"

namespace aadff {
namespace fh {

constexpr int NT = 256, WAVES = NT / kWave;
constexpr int MAXC = 4;
constexpr int LOSS_PPT = 4, LOSS_SUMS = 6;                    // pixels per thread of loss_sums; Se, count, Se2, Sa, Sx, Sy

struct HeadArgs {
    const float* scores;
    const float* stack;
    const float* foc;
    float* depth;                                             // forward
    float* aif;
    const float* g_depth;                                     // backward
    const float* g_aif;
    float* d_scores;
    float* d_stack;
    float* ws;                                                // d_foc partials [N][S][4 bpn], or NULL
    int K, Ct, S, H, W, GW;                                   // GW: groups of four pixels per row
    unsigned bpn;                                             // workgroups per batch item
    int normalize;
};

// torch's softplus (beta 1, threshold 20) and its derivative
__device__ __forceinline__ float softplus(float z) { return z > 20.f ? z : log1pf(expf(z)); }
__device__ __forceinline__ float softplus_grad(float z) {
#pragma clang fp contract(off)
    if (z > 20.f) return 1.f;
    const float e = expf(z);
    return e / (e + 1.f);
}

// the thread's four pixels: element offsets relative to the first (clamped into the row) and which of them exist
struct Px {
    int off[4];
    bool ok[4];
    bool live;
};

template <bool VEC>
__device__ __forceinline__ void load4(const float* p, const Px& P, float v[4]) {
    if (VEC) {
        const float4 t = *reinterpret_cast<const float4*>(p);
        v[0] = t.x, v[1] = t.y, v[2] = t.z, v[3] = t.w;
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) v[j] = p[P.off[j]];
    }
}

template <bool VEC>
__device__ __forceinline__ void store4(float* p, const Px& P, const float v[4]) {
    if (VEC) {
        if (P.live) *reinterpret_cast<float4*>(p) = make_float4(v[0], v[1], v[2], v[3]);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j)
            if (P.ok[j]) p[j] = v[j];
    }
}

// the scores of the second attention: the second channel, or with one channel the values already loaded (element by element: a choice
// between the two arrays by address would put both into scratch memory)
template <bool VEC>
__device__ __forceinline__ void load_second(bool two, const float* p, const Px& P, const float z[4], float z2[4]) {
    if (two) {
        load4<VEC>(p, P, z2);
    } else {
#pragma unroll
        for (int j = 0; j < 4; ++j) z2[j] = z[j];
    }
}

// position of the thread: batch item n, offset of its first pixel in a plane (0 for a thread beyond the image: it loads valid memory
// and stores nothing)
__device__ __forceinline__ void locate(const HeadArgs& A, unsigned& n, size_t& pix, Px& P) {
    n = blockIdx.x / A.bpn;
    const long item = (long)(blockIdx.x % A.bpn) * NT + threadIdx.x;
    P.live = item < (long)A.H * A.GW;
    const int y = P.live ? (int)(item / A.GW) : 0;
    const int x0 = P.live ? (int)(item % A.GW) * 4 : 0;
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        P.ok[j] = P.live && x0 + j < A.W;
        P.off[j] = min(x0 + j, A.W - 1) - x0;
    }
    pix = (size_t)y * A.W + x0;
}

// One attention over the slices.  `st`: its normaliser, the maximum (softmax) or T = sum softplus (normalised softplus).
typedef float f4v __attribute__((ext_vector_type(4)));      // register values under [j]: arrays in a struct stayed in scratch memory
struct Att {
    f4v st;
    f4v l;                                                    // softmax: sum of the weights; normalised softplus: 1
};

__device__ __forceinline__ void att_init(Att& a, bool soft) {
#pragma unroll
    for (int j = 0; j < 4; ++j) a.st[j] = soft ? 0.f : -INFINITY, a.l[j] = 0.f;
}
__device__ __forceinline__ void att_scan(Att& a, bool soft, const float z[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) a.st[j] = soft ? a.st[j] + softplus(z[j]) : fmaxf(a.st[j], z[j]);
}
// unnormalised weight of a slice: softmax exp(z - max), to be divided by l at the end; normalised softplus: softplus(z) / T, final
__device__ __forceinline__ void att_weight(const Att& a, bool soft, const float z[4], float w[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) w[j] = soft ? softplus(z[j]) / a.st[j] : expf(z[j] - a.st[j]);
}
__device__ __forceinline__ void att_add(Att& a, const float w[4]) {
#pragma clang fp contract(off)
#pragma unroll
    for (int j = 0; j < 4; ++j) a.l[j] += w[j];
}
__device__ __forceinline__ float att_finish(const Att& a, bool soft, int j, float acc) {
#pragma clang fp contract(off)
    return soft ? acc : acc / a.l[j];
}
// d weight_j / d z_j relative to the final probability: softmax p_j itself (p_j = w_j / l), normalised softplus sigma(z_j) / T
__device__ __forceinline__ float att_slope(const Att& a, bool soft, int j, float z, float w) {
#pragma clang fp contract(off)
    return soft ? softplus_grad(z) / a.st[j] : w / a.l[j];
}

template <int CA, bool VEC>
__global__ __launch_bounds__(NT) void head_fwd(HeadArgs A) {
#pragma clang fp contract(off)
    unsigned n;
    size_t pix;
    Px P;
    locate(A, n, pix, P);
    if (!P.live) return;
    const int S = A.S, K = A.K;
    const size_t HW = (size_t)A.H * A.W;
    const float* zd = A.scores + (size_t)n * K * S * HW + pix;
    const float* za = zd + (size_t)(K - 1) * S * HW;
    const float* xs = A.stack + (size_t)n * A.Ct * S * HW + pix;
    const float* u = A.foc + (size_t)n * S;
    const bool soft_d = A.normalize != 0, soft_a = soft_d && K == 2;
    const bool two = K == 2;                                  // a second score channel to load
    const bool same = !two && !soft_d;                        // one attention serves both outputs

    Att ad, aa;
    att_init(ad, soft_d);
    att_init(aa, soft_a);
    for (int s = 0; s < S; ++s) {
        float z[4], z2[4];
        load4<VEC>(zd + (size_t)s * HW, P, z);
        att_scan(ad, soft_d, z);
        if (same) continue;
        load_second<VEC>(two, za + (size_t)s * HW, P, z, z2);
        att_scan(aa, soft_a, z2);
    }

    float accd[4] = {0.f, 0.f, 0.f, 0.f}, acca[CA][4];
#pragma unroll
    for (int c = 0; c < CA; ++c)
#pragma unroll
        for (int j = 0; j < 4; ++j) acca[c][j] = 0.f;
    for (int s = 0; s < S; ++s) {
        float z[4], z2[4], wd[4], wa[4], x[CA][4];
        load4<VEC>(zd + (size_t)s * HW, P, z);
        load_second<VEC>(two, za + (size_t)s * HW, P, z, z2);
#pragma unroll
        for (int c = 0; c < CA; ++c) load4<VEC>(xs + ((size_t)c * S + s) * HW, P, x[c]);
        att_weight(ad, soft_d, z, wd);
        att_add(ad, wd);
        if (same) {
#pragma unroll
            for (int j = 0; j < 4; ++j) wa[j] = wd[j];
        } else {
            att_weight(aa, soft_a, z2, wa);
            att_add(aa, wa);
        }
        const float us = u[s];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            accd[j] += wd[j] * us;
#pragma unroll
            for (int c = 0; c < CA; ++c) acca[c][j] += wa[j] * x[c][j];
        }
    }
    if (same) {
#pragma unroll
        for (int j = 0; j < 4; ++j) aa.st[j] = ad.st[j], aa.l[j] = ad.l[j];
    }
    float o[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) o[j] = att_finish(ad, soft_d, j, accd[j]);
    store4<VEC>(A.depth + (size_t)n * HW + pix, P, o);
#pragma unroll
    for (int c = 0; c < CA; ++c) {
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = att_finish(aa, soft_a, j, acca[c][j]);
        store4<VEC>(A.aif + ((size_t)n * CA + c) * HW + pix, P, o);
    }
}

template <int CA, bool VEC>
__global__ __launch_bounds__(NT) void head_bwd(HeadArgs A) {
#pragma clang fp contract(off)
    unsigned n;
    size_t pix;
    Px P;
    locate(A, n, pix, P);                                     // no early exit: the wave sums below need every lane
    const int S = A.S, K = A.K;
    const size_t HW = (size_t)A.H * A.W;
    const float* zd = A.scores + (size_t)n * K * S * HW + pix;
    const float* za = zd + (size_t)(K - 1) * S * HW;
    const float* xs = A.stack + (size_t)n * A.Ct * S * HW + pix;
    const float* u = A.foc + (size_t)n * S;
    const bool soft_d = A.normalize != 0, soft_a = soft_d && K == 2;
    const bool two = K == 2, same = !two && !soft_d;
    const bool want_z = A.d_scores != nullptr, want_x = A.d_stack != nullptr, want_u = A.ws != nullptr;

    float gd[4], ga[CA][4];
    load4<VEC>(A.g_depth + (size_t)n * HW + pix, P, gd);
#pragma unroll
    for (int c = 0; c < CA; ++c) load4<VEC>(A.g_aif + ((size_t)n * CA + c) * HW + pix, P, ga[c]);

    Att ad, aa;
    att_init(ad, soft_d);
    att_init(aa, soft_a);
    for (int s = 0; s < S; ++s) {
        float z[4], z2[4];
        load4<VEC>(zd + (size_t)s * HW, P, z);
        att_scan(ad, soft_d, z);
        if (same) continue;
        load_second<VEC>(two, za + (size_t)s * HW, P, z, z2);
        att_scan(aa, soft_a, z2);
    }

    // the expectations the gradients of the scores are centred on: depth, and qbar = sum_s pa_s q_s with q_s = sum_c g_aif_c stack_c,s
    float dep[4] = {0.f, 0.f, 0.f, 0.f}, qbar[4] = {0.f, 0.f, 0.f, 0.f};
    for (int s = 0; s < S; ++s) {
        float z[4], z2[4], wd[4], wa[4];
        load4<VEC>(zd + (size_t)s * HW, P, z);
        load_second<VEC>(two, za + (size_t)s * HW, P, z, z2);
        att_weight(ad, soft_d, z, wd);
        att_add(ad, wd);
        if (same) {
#pragma unroll
            for (int j = 0; j < 4; ++j) wa[j] = wd[j];
        } else {
            att_weight(aa, soft_a, z2, wa);
            att_add(aa, wa);
        }
        const float us = u[s];
#pragma unroll
        for (int j = 0; j < 4; ++j) dep[j] += wd[j] * us;
        if (want_z) {
            float x[CA][4];
#pragma unroll
            for (int c = 0; c < CA; ++c) load4<VEC>(xs + ((size_t)c * S + s) * HW, P, x[c]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float q = ga[0][j] * x[0][j];
#pragma unroll
                for (int c = 1; c < CA; ++c) q += ga[c][j] * x[c][j];
                qbar[j] += wa[j] * q;
            }
        }
    }
    if (same) {
#pragma unroll
        for (int j = 0; j < 4; ++j) aa.st[j] = ad.st[j], aa.l[j] = ad.l[j];
    }
#pragma unroll
    for (int j = 0; j < 4; ++j) dep[j] = att_finish(ad, soft_d, j, dep[j]), qbar[j] = att_finish(aa, soft_a, j, qbar[j]);

    const unsigned wave = (blockIdx.x % A.bpn) * WAVES + threadIdx.x / kWave;
    for (int s = 0; s < S; ++s) {
        float z[4], z2[4], wd[4], wa[4];
        load4<VEC>(zd + (size_t)s * HW, P, z);
        load_second<VEC>(two, za + (size_t)s * HW, P, z, z2);
        att_weight(ad, soft_d, z, wd);
        if (same) {
#pragma unroll
            for (int j = 0; j < 4; ++j) wa[j] = wd[j];
        } else {
            att_weight(aa, soft_a, z2, wa);
        }
        const float us = u[s];
        float pd[4], pa[4];                                   // the final probabilities
#pragma unroll
        for (int j = 0; j < 4; ++j) pd[j] = soft_d ? wd[j] : wd[j] / ad.l[j], pa[j] = soft_a ? wa[j] : wa[j] / aa.l[j];
        if (want_z) {
            float x[CA][4], dzd[4], dza[4];
#pragma unroll
            for (int c = 0; c < CA; ++c) load4<VEC>(xs + ((size_t)c * S + s) * HW, P, x[c]);
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                float q = ga[0][j] * x[0][j];
#pragma unroll
                for (int c = 1; c < CA; ++c) q += ga[c][j] * x[c][j];
                dzd[j] = gd[j] * att_slope(ad, soft_d, j, z[j], wd[j]) * (us - dep[j]);
                dza[j] = att_slope(aa, soft_a, j, z2[j], wa[j]) * (q - qbar[j]);
            }
            float* dz = A.d_scores + (size_t)n * K * S * HW + (size_t)s * HW + pix;
            if (two) {
                store4<VEC>(dz, P, dzd);
                store4<VEC>(dz + (size_t)S * HW, P, dza);
            } else {
#pragma unroll
                for (int j = 0; j < 4; ++j) dzd[j] += dza[j];
                store4<VEC>(dz, P, dzd);
            }
        }
        if (want_x) {
            float* dx = A.d_stack + (size_t)n * A.Ct * S * HW + (size_t)s * HW + pix;
#pragma unroll
            for (int c = 0; c < CA; ++c) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = ga[c][j] * pa[j];
                store4<VEC>(dx + (size_t)c * S * HW, P, o);
            }
            for (int c = CA; c < A.Ct; ++c) {
                float o[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) o[j] = 0.f;
                store4<VEC>(dx + (size_t)c * S * HW, P, o);
            }
        }
        if (want_u) {
            float t = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) t += P.ok[j] ? gd[j] * pd[j] : 0.f;
            t = wave_sum(t);
            if (threadIdx.x % kWave == 0) A.ws[((size_t)n * S + s) * ((size_t)A.bpn * WAVES) + wave] = t;
        }
    }
}

// second stage of a reduction: workgroup r adds the `count` partials of row r (stride `stride` elements apart) in a fixed order and in
// float64 - thread t takes t, t + 256, ... in turn, then a fixed tree over the threads
template <typename Tin, typename Tout>
__global__ __launch_bounds__(NT) void final_sum(const Tin* part, long count, long row_stride, long stride, Tout* out) {
    __shared__ double sh[NT];
    const Tin* p = part + (size_t)blockIdx.x * row_stride;
    double acc = 0.0;
    for (long i = threadIdx.x; i < count; i += NT) acc += (double)p[i * stride];
    sh[threadIdx.x] = acc;
    __syncthreads();
    for (int w = NT / 2; w > 0; w >>= 1) {
        if ((int)threadIdx.x < w) sh[threadIdx.x] += sh[threadIdx.x + w];
        __syncthreads();
    }
    if (threadIdx.x == 0) out[blockIdx.x] = (Tout)sh[0];
}

// ------------------------------------------------------------------ the loss
struct LossArgs {
    const float* depth;                                       // [N,1,Hd,Wd]
    const float* aif;                                         // [N,Ca,Ha,Wa] or NULL
    const float* gtd;                                         // [N,1,Hg,Wg] or NULL
    const float* gta;                                         // [N,Ca,Hi,Wi] or NULL
    const float* range;                                       // {lo, hi} or NULL: mask gt > 0
    const double* g;                                          // backward: cotangents of the six sums
    double* part;                                             // forward: [blocks][6]
    float* d_depth;
    float* d_aif;
    int N, Ca, Hd, Wd, Ha, Wa, Hg, Wg, Hi, Wi, h, w, Hm, Wm;  // h x w: the common window; Hm x Wm: the backward's thread grid
};

__device__ __forceinline__ bool in_mask(const LossArgs& A, float g, float lo, float hi) { return A.range ? (g >= lo && g <= hi) : g > 0.f; }

// edge weight between pixel (y, x) and its neighbour at element distance `step` of gt_aif: exp(-mean_c (150 (g' - g))^2)
__device__ __forceinline__ float edge_weight(const LossArgs& A, size_t o, size_t step) {
#pragma clang fp contract(off)
    const size_t plane = (size_t)A.Hi * A.Wi;
    float m = 0.f;
    for (int c = 0; c < A.Ca; ++c) {
        const float t = 150.f * (A.gta[o + c * plane + step] - A.gta[o + c * plane]);
        m += t * t;
    }
    return expf(-(m / (float)A.Ca));
}

__global__ __launch_bounds__(NT) void loss_sums(LossArgs A) {
#pragma clang fp contract(off)
    __shared__ double sh[WAVES][LOSS_SUMS];
    const long hw = (long)A.h * A.w, total = (long)A.N * hw;
    float lo = 0.f, hi = 0.f;
    if (A.range) lo = A.range[0], hi = A.range[1];
    double acc[LOSS_SUMS] = {0.0, 0.0, 0.0, 0.0, 0.0, 0.0};
    for (int k = 0; k < LOSS_PPT; ++k) {
        const long i = ((long)blockIdx.x * LOSS_PPT + k) * NT + threadIdx.x;
        if (i >= total) continue;
        const int n = (int)(i / hw), y = (int)((i % hw) / A.w), x = (int)(i % A.w);
        const size_t od = ((size_t)n * A.Hd + y) * A.Wd + x;
        const float d = A.depth[od];
        if (A.gtd) {
            const float g = A.gtd[((size_t)n * A.Hg + y) * A.Wg + x];
            if (in_mask(A, g, lo, hi)) {
                const float e = d - g;
                acc[0] += (double)fabsf(e);
                acc[1] += 1.0;
                acc[2] += (double)(e * e);
            }
        }
        if (A.gta) {
            const size_t oi = ((size_t)n * A.Ca * A.Hi + y) * A.Wi + x, oa = ((size_t)n * A.Ca * A.Ha + y) * A.Wa + x;
            for (int c = 0; c < A.Ca; ++c)
                acc[3] += (double)fabsf(A.aif[oa + (size_t)c * A.Ha * A.Wa] - A.gta[oi + (size_t)c * A.Hi * A.Wi]);
            if (y + 1 < A.h) {
                const float dg = A.depth[od + A.Wd] - d;
                acc[4] += (double)(edge_weight(A, oi, A.Wi) * sqrtf(dg * dg + 1e-6f));
            }
            if (x + 1 < A.w) {
                const float dg = A.depth[od + 1] - d;
                acc[5] += (double)(edge_weight(A, oi, 1) * sqrtf(dg * dg + 1e-6f));
            }
        }
    }
#pragma unroll
    for (int k = 0; k < LOSS_SUMS; ++k) {
        double v = acc[k];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
        if (threadIdx.x % kWave == 0) sh[threadIdx.x / kWave][k] = v;
    }
    __syncthreads();
    if (threadIdx.x < LOSS_SUMS) {
        double v = sh[0][threadIdx.x];
        for (int wv = 1; wv < WAVES; ++wv) v += sh[wv][threadIdx.x];
        A.part[(size_t)blockIdx.x * LOSS_SUMS + threadIdx.x] = v;
    }
}

// d (w r(dg)) / d dg = w dg / r
__device__ __forceinline__ float smooth_slope(float w, float dg) {
#pragma clang fp contract(off)
    return w * dg / sqrtf(dg * dg + 1e-6f);
}

__global__ __launch_bounds__(NT) void loss_bwd(LossArgs A) {
#pragma clang fp contract(off)
    const long hwm = (long)A.Hm * A.Wm;
    const long i = (long)blockIdx.x * NT + threadIdx.x;
    if (i >= (long)A.N * hwm) return;
    const int n = (int)(i / hwm), y = (int)((i % hwm) / A.Wm), x = (int)(i % A.Wm);
    const bool inside = y < A.h && x < A.w;
    const float c0 = (float)A.g[0], c3 = (float)A.g[3], c4 = (float)A.g[4], c5 = (float)A.g[5];
    if (A.d_depth && y < A.Hd && x < A.Wd) {
        const size_t od = ((size_t)n * A.Hd + y) * A.Wd + x;
        float v = 0.f;
        if (inside) {
            const float d = A.depth[od];
            if (A.gtd) {
                float lo = 0.f, hi = 0.f;
                if (A.range) lo = A.range[0], hi = A.range[1];
                const float g = A.gtd[((size_t)n * A.Hg + y) * A.Wg + x];
                const float e = d - g;
                if (in_mask(A, g, lo, hi)) v = e > 0.f ? c0 : (e < 0.f ? -c0 : 0.f);
            }
            if (A.gta) {
                const size_t oi = ((size_t)n * A.Ca * A.Hi + y) * A.Wi + x;
                if (y >= 1) v += c4 * smooth_slope(edge_weight(A, oi - A.Wi, A.Wi), d - A.depth[od - A.Wd]);
                if (y + 1 < A.h) v -= c4 * smooth_slope(edge_weight(A, oi, A.Wi), A.depth[od + A.Wd] - d);
                if (x >= 1) v += c5 * smooth_slope(edge_weight(A, oi - 1, 1), d - A.depth[od - 1]);
                if (x + 1 < A.w) v -= c5 * smooth_slope(edge_weight(A, oi, 1), A.depth[od + 1] - d);
            }
        }
        A.d_depth[od] = v;
    }
    if (A.d_aif && y < A.Ha && x < A.Wa) {
        const size_t pa = (size_t)A.Ha * A.Wa, pi = (size_t)A.Hi * A.Wi;
        const size_t oa = (size_t)n * A.Ca * pa + (size_t)y * A.Wa + x;
        for (int c = 0; c < A.Ca; ++c) {
            float v = 0.f;
            if (inside && A.gta) {
                const float e = A.aif[oa + c * pa] - A.gta[(size_t)n * A.Ca * pi + c * pi + (size_t)y * A.Wi + x];
                v = e > 0.f ? c3 : (e < 0.f ? -c3 : 0.f);
            }
            A.d_aif[oa + c * pa] = v;
        }
    }
}

template <bool VEC>
static void launch_head(bool bwd, int Ca, dim3 grid, hipStream_t st, const HeadArgs& A) {
#define AADFF_HEAD_CASE(C)                                                                         \
    case C:                                                                                        \
        if (bwd) hipLaunchKernelGGL((head_bwd<C, VEC>), grid, dim3(NT), 0, st, A);                 \
        else hipLaunchKernelGGL((head_fwd<C, VEC>), grid, dim3(NT), 0, st, A);                     \
        break;
    switch (Ca) {
        AADFF_HEAD_CASE(1)
        AADFF_HEAD_CASE(2)
        AADFF_HEAD_CASE(3)
        default:
        AADFF_HEAD_CASE(4)
    }
#undef AADFF_HEAD_CASE
}

static int head_check(const char* who, const void* scores, const void* stack, const void* foc, int N, int K, int Ct, int Ca, int S, int H, int W,
                      HeadArgs& A) {
    AADFF_CHECK_ARG(scores, "%s: scores is NULL", who);
    AADFF_CHECK_ARG(stack, "%s: stack is NULL", who);
    AADFF_CHECK_ARG(foc, "%s: foc_dists is NULL", who);
    AADFF_CHECK_ARG(K == 1 || K == 2, "%s: K = %d is neither 1 nor 2", who, K);
    AADFF_CHECK_ARG(Ct >= 1 && Ct <= MAXC, "%s: Ct = %d is outside 1..%d", who, Ct, MAXC);
    AADFF_CHECK_ARG(Ca >= 1 && Ca <= Ct, "%s: Ca = %d is outside 1..Ct = %d", who, Ca, Ct);
    AADFF_CHECK_ARG(S >= 1, "%s: S = %d, at least one slice is needed", who, S);
    AADFF_CHECK_ARG(N > 0, "%s: N = %d is not positive", who, N);
    AADFF_CHECK_ARG(H > 0, "%s: H = %d is not positive", who, H);
    AADFF_CHECK_ARG(W > 0, "%s: W = %d is not positive", who, W);
    const long GW = ((long)W + 3) / 4, bpn = ((long)H * GW + NT - 1) / NT;
    AADFF_CHECK_ARG((long)H * W < (1L << 31) - 8 && bpn * N < (1L << 31), "%s: N = %d, H = %d, W = %d are too large for one launch", who, N, H, W);
    A.K = K, A.Ct = Ct, A.S = S, A.H = H, A.W = W, A.GW = (int)GW, A.bpn = (unsigned)bpn;
    return 0;
}

}  // namespace fh
}  // namespace aadff

using namespace aadff;

extern "C" int aadff_attention_depth(const float* scores, const float* stack, const float* foc_dists, float* depth, float* aif, int N, int K,
                                     int Ct, int Ca, int S, int H, int W, int normalize, aadff_stream_t stream) {
    fh::HeadArgs A = {};
    if (int rc = fh::head_check("attention_depth", scores, stack, foc_dists, N, K, Ct, Ca, S, H, W, A)) return rc;
    AADFF_CHECK_ARG(depth, "attention_depth: depth is NULL");
    AADFF_CHECK_ARG(aif, "attention_depth: aif is NULL");
    A.scores = scores, A.stack = stack, A.foc = foc_dists, A.depth = depth, A.aif = aif, A.normalize = normalize != 0;
    const uintptr_t bits = (uintptr_t)scores | (uintptr_t)stack | (uintptr_t)depth | (uintptr_t)aif;
    const bool vec = (W % 4 == 0) && (bits % 16 == 0);        // every plane then starts on 16 bytes: H * W is a multiple of four
    const dim3 grid(A.bpn * (unsigned)N);
    if (vec) fh::launch_head<true>(false, Ca, grid, (hipStream_t)stream, A);
    else fh::launch_head<false>(false, Ca, grid, (hipStream_t)stream, A);
    AADFF_CHECK_LAUNCH();
    return 0;
}

extern "C" int aadff_attention_depth_bwd(const float* scores, const float* stack, const float* foc_dists, const float* g_depth, const float* g_aif,
                                         float* d_scores_or_null, float* d_stack_or_null, float* d_foc_or_null, void* workspace,
                                         size_t workspace_bytes, int N, int K, int Ct, int Ca, int S, int H, int W, int normalize,
                                         aadff_stream_t stream) {
    fh::HeadArgs A = {};
    if (int rc = fh::head_check("attention_depth_bwd", scores, stack, foc_dists, N, K, Ct, Ca, S, H, W, A)) return rc;
    AADFF_CHECK_ARG(g_depth, "attention_depth_bwd: g_depth is NULL");
    AADFF_CHECK_ARG(g_aif, "attention_depth_bwd: g_aif is NULL");
    AADFF_CHECK_ARG(d_scores_or_null || d_stack_or_null || d_foc_or_null, "attention_depth_bwd: no gradient is asked for");
    const size_t waves = (size_t)A.bpn * fh::WAVES, need = d_foc_or_null ? sizeof(float) * (size_t)N * S * waves : 0;
    AADFF_CHECK_ARG(!need || (workspace && workspace_bytes >= need), "attention_depth_bwd: workspace of %zu bytes, %zu are needed", workspace_bytes, need);
    A.scores = scores, A.stack = stack, A.foc = foc_dists, A.g_depth = g_depth, A.g_aif = g_aif, A.normalize = normalize != 0;
    A.d_scores = d_scores_or_null, A.d_stack = d_stack_or_null, A.ws = d_foc_or_null ? (float*)workspace : nullptr;
    const uintptr_t bits = (uintptr_t)scores | (uintptr_t)stack | (uintptr_t)g_depth | (uintptr_t)g_aif | (uintptr_t)d_scores_or_null | (uintptr_t)d_stack_or_null;
    const bool vec = (W % 4 == 0) && (bits % 16 == 0);
    const dim3 grid(A.bpn * (unsigned)N);
    hipStream_t st = (hipStream_t)stream;
    if (vec) fh::launch_head<true>(true, Ca, grid, st, A);
    else fh::launch_head<false>(true, Ca, grid, st, A);
    AADFF_CHECK_LAUNCH();
    if (d_foc_or_null) {
        hipLaunchKernelGGL((fh::final_sum<float, float>), dim3((unsigned)(N * S)), dim3(fh::NT), 0, st, (const float*)workspace, (long)waves, (long)waves, 1L,
                           d_foc_or_null);
        AADFF_CHECK_LAUNCH();
    }
    return 0;
}

static int loss_check(const char* who, const float* depth, const float* aif, const float* gtd, const float* gta, int N, int Ca, int Hd, int Wd, int Ha,
                      int Wa, int Hg, int Wg, int Hi, int Wi, fh::LossArgs& A) {
    AADFF_CHECK_ARG(depth, "%s: depth is NULL", who);
    AADFF_CHECK_ARG(gtd || gta, "%s: neither gt_depth nor gt_aif is given", who);
    AADFF_CHECK_ARG(!gta || aif, "%s: gt_aif is given but aif is NULL", who);
    AADFF_CHECK_ARG(N > 0, "%s: N = %d is not positive", who, N);
    AADFF_CHECK_ARG(Hd > 0 && Wd > 0, "%s: depth is %d x %d", who, Hd, Wd);
    AADFF_CHECK_ARG(!gtd || (Hg > 0 && Wg > 0), "%s: gt_depth is %d x %d", who, Hg, Wg);
    if (gta) {
        AADFF_CHECK_ARG(Ca >= 1 && Ca <= fh::MAXC, "%s: Ca = %d is outside 1..%d", who, Ca, fh::MAXC);
        AADFF_CHECK_ARG(Ha > 0 && Wa > 0, "%s: aif is %d x %d", who, Ha, Wa);
        AADFF_CHECK_ARG(Hi > 0 && Wi > 0, "%s: gt_aif is %d x %d", who, Hi, Wi);
    }
    int h = Hd, w = Wd;
    if (gtd) h = h < Hg ? h : Hg, w = w < Wg ? w : Wg;
    if (gta) h = h < Ha ? h : Ha, w = w < Wa ? w : Wa, h = h < Hi ? h : Hi, w = w < Wi ? w : Wi;
    const long big = (1L << 31) - 8;
    AADFF_CHECK_ARG((long)N * Hd * Wd < big && (!gta || (long)N * Ha * Wa < big), "%s: N = %d with %d x %d is too large for one launch", who, N, Hd, Wd);
    A.depth = depth, A.aif = gta ? aif : nullptr, A.gtd = gtd, A.gta = gta;
    A.N = N, A.Ca = gta ? Ca : 0, A.Hd = Hd, A.Wd = Wd, A.Ha = Ha, A.Wa = Wa, A.Hg = Hg, A.Wg = Wg, A.Hi = Hi, A.Wi = Wi, A.h = h, A.w = w;
    return 0;
}

extern "C" int aadff_dff_loss_sums(const float* depth, const float* aif_or_null, const float* gt_depth_or_null, const float* gt_aif_or_null,
                                   const float* range_or_null, double* sums, void* workspace, size_t workspace_bytes, int N, int Ca, int Hd,
                                   int Wd, int Ha, int Wa, int Hg, int Wg, int Hi, int Wi, aadff_stream_t stream) {
    fh::LossArgs A = {};
    if (int rc = loss_check("dff_loss_sums", depth, aif_or_null, gt_depth_or_null, gt_aif_or_null, N, Ca, Hd, Wd, Ha, Wa, Hg, Wg, Hi, Wi, A)) return rc;
    AADFF_CHECK_ARG(sums, "dff_loss_sums: sums is NULL");
    const long per = (long)fh::NT * fh::LOSS_PPT, blocks = ((long)N * A.h * A.w + per - 1) / per;
    const size_t need = sizeof(double) * fh::LOSS_SUMS * (size_t)blocks;
    AADFF_CHECK_ARG(workspace && workspace_bytes >= need, "dff_loss_sums: workspace of %zu bytes, %zu are needed", workspace_bytes, need);
    A.range = range_or_null, A.part = (double*)workspace;
    hipStream_t st = (hipStream_t)stream;
    hipLaunchKernelGGL(fh::loss_sums, dim3((unsigned)blocks), dim3(fh::NT), 0, st, A);
    AADFF_CHECK_LAUNCH();
    hipLaunchKernelGGL((fh::final_sum<double, double>), dim3(fh::LOSS_SUMS), dim3(fh::NT), 0, st, (const double*)workspace, blocks, 1L, (long)fh::LOSS_SUMS, sums);
    AADFF_CHECK_LAUNCH();
    return 0;
}

extern "C" int aadff_dff_loss_bwd(const float* depth, const float* aif_or_null, const float* gt_depth_or_null, const float* gt_aif_or_null,
                                  const float* range_or_null, const double* g_sums, float* d_depth_or_null, float* d_aif_or_null, int N, int Ca,
                                  int Hd, int Wd, int Ha, int Wa, int Hg, int Wg, int Hi, int Wi, aadff_stream_t stream) {
    fh::LossArgs A = {};
    if (int rc = loss_check("dff_loss_bwd", depth, aif_or_null, gt_depth_or_null, gt_aif_or_null, N, Ca, Hd, Wd, Ha, Wa, Hg, Wg, Hi, Wi, A)) return rc;
    AADFF_CHECK_ARG(g_sums, "dff_loss_bwd: g_sums is NULL");
    AADFF_CHECK_ARG(d_depth_or_null || d_aif_or_null, "dff_loss_bwd: no gradient is asked for");
    AADFF_CHECK_ARG(!d_aif_or_null || (aif_or_null && Ca >= 1 && Ca <= fh::MAXC && Ha > 0 && Wa > 0), "dff_loss_bwd: d_aif is asked for without aif [N,%d,%d,%d]", Ca, Ha, Wa);
    A.range = range_or_null, A.g = g_sums, A.d_depth = d_depth_or_null, A.d_aif = d_aif_or_null;
    if (d_aif_or_null) A.aif = aif_or_null, A.Ca = Ca;        // without gt_aif the gradient is zero, but it still has aif's shape
    A.Hm = d_depth_or_null ? Hd : 0, A.Wm = d_depth_or_null ? Wd : 0;
    if (d_aif_or_null) A.Hm = A.Hm > Ha ? A.Hm : Ha, A.Wm = A.Wm > Wa ? A.Wm : Wa;
    const long blocks = ((long)N * A.Hm * A.Wm + fh::NT - 1) / fh::NT;
    AADFF_CHECK_ARG(blocks < (1L << 31), "dff_loss_bwd: N = %d with %d x %d is too large for one launch", N, A.Hm, A.Wm);
    hipLaunchKernelGGL(fh::loss_bwd, dim3((unsigned)blocks), dim3(fh::NT), 0, (hipStream_t)stream, A);
    AADFF_CHECK_LAUNCH();
    return 0;
}
