// Per-pixel PSF gather for gfx950 (MI355X), forward and backward (local_psf_render, deeplens/render_psf.py:76-107 of the
// reference, and the gradients torch.autograd derives for it, as closed forms in plain fp32).  See include/aadff.h for the
// entry points, DESIGN.md 4.4 for the forward's design and 4.7 for the backward's.
//
// Every sum of the backward has a fixed order (no float atomics): results are bitwise reproducible from run to run.
#include <cstdlib>
#include "common.h"
#include "gather_window.h"

namespace aadff {

// ------------------------------------------------------------------------------------
// Per-pixel PSF gather (local_psf_render): HBM-bound on the PSF tensor (ks*ks*4 B/pixel + 24 B/pixel).
// One wave per run of 64 consecutive pixels of one image row:
//   * lane l streams ITS pixel's ks*ks taps straight from global memory with 16-byte loads (the taps of
//     a pixel are contiguous; every byte of every cache line is used, the lines live in L1 for the few
//     loads that share them) - no LDS round trip for the 484 B/pixel stream, so 8+ waves per CU keep
//     tens of KB of loads in flight;
//   * only the C x ks x (64+ks-1) replicate-clamped image window is staged in LDS (read at lane+v:
//     conflict-free);
//   * no flip (render_psf.py:99-105 multiplies unfold() patches with the kernel as is).
// ------------------------------------------------------------------------------------

struct __attribute__((packed, aligned(4))) f4u { float x, y, z, w; };   // 16-byte load / store at 4-byte alignment

template <int KS, int CN>
__global__ __launch_bounds__(64) void local_psf_kernel(const float* __restrict__ img, const float* __restrict__ psf,
                                                        float* __restrict__ out, int C, int H, int W) {
    constexpr int MC = CN > 0 ? CN : LP_MAXC;
    constexpr int KK = KS * KS, TWD = LP_NPX + KS - 1;
    __shared__ float tl[MC * KS * TWD];
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * LP_NPX, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(LP_NPX, W - x0);
    const bool act = lane < npx;
    const float* pp = psf + ((size_t)(b * H + y) * W + x0 + (act ? lane : 0)) * KK;

    // first batch of tap loads is in flight while the image window is staged
    constexpr int NB = 8;                                    // 16-byte loads per batch
    constexpr int NV = KK / 4, REM = KK - 4 * NV;            // KK = 4*NV + REM
    f4u wq[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i)
        if (i < NV) wq[i] = *reinterpret_cast<const f4u*>(pp + 4 * i);

    stage_window<KS, CN>(img, tl, b, C, H, W, y, x0, lane);
    __syncthreads();

    float acc[MC] = {};
    auto tap = [&](int t, float wv) {
        const int u = t / KS, v = t - u * KS;
#pragma unroll
        for (int cc = 0; cc < MC; ++cc)
            if (CN > 0 || cc < C) acc[cc] = fmaf(tl[(cc * KS + u) * TWD + lane + v], wv, acc[cc]);
    };
#pragma unroll
    for (int base = 0; base < NV; base += NB) {
        f4u cur[NB];
#pragma unroll
        for (int i = 0; i < NB; ++i) cur[i] = wq[i];
#pragma unroll
        for (int i = 0; i < NB; ++i)                           // next batch goes out before this one is consumed
            if (base + NB + i < NV) wq[i] = *reinterpret_cast<const f4u*>(pp + 4 * (base + NB + i));
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (base + i < NV) {
                const int t = 4 * (base + i);
                tap(t, cur[i].x); tap(t + 1, cur[i].y); tap(t + 2, cur[i].z); tap(t + 3, cur[i].w);
            }
        }
    }
#pragma unroll
    for (int i = 0; i < REM; ++i) tap(4 * NV + i, pp[4 * NV + i]);
    if (act) {
#pragma unroll
        for (int cc = 0; cc < MC; ++cc)
            if (CN > 0 || cc < C) out[((size_t)(b * C + cc) * H + y) * W + x0 + lane] = acc[cc];
    }
}

// LDS-DMA form (default when the rows are 16-byte aligned: W % 4 == 0).  The taps of a 64-pixel run are ONE contiguous
// block of 64*ks*ks*4 bytes (30 976 B at ks 11), so the run is fetched by `global_load_lds_dwordx4` wave-instructions of
// 1 KiB each (64 lanes x 16 consecutive bytes: every request a full line, nothing passes through VGPRs) that are all in
// flight at once, and each lane then reads ITS pixel's taps from LDS at a pitch of ks*ks dwords (odd: the 32 lanes of a
// ds_read_b32 group hit 32 different banks).  The old form let every lane walk its own 484-byte row with 16-byte loads:
// one wave-instruction touched 64 different rows.  One wave per workgroup, 40 KB of LDS -> 4 runs (120 KB) in flight
// per CU while other workgroups of the CU compute.  A workgroup is 2 or 4 waves that split the pieces, the window rows and the
// tap rows of the run (partial sums meet through the freed tap buffer): the shorter a workgroup computes, the larger the
// share of its life it spends with loads in flight.
#ifndef AADFF_LP_DMA_AUX
#define AADFF_LP_DMA_AUX 0          // 2 = nt (streamed-once hint)
#endif
template <int KS, int CN, int NWV>
__global__ __launch_bounds__(64 * NWV) void local_psf_dma_kernel(const float* __restrict__ img, const float* __restrict__ psf,
                                                                  float* __restrict__ out, int C, int H, int W) {
    constexpr int KK = KS * KS, TWD = LP_NPX + KS - 1;
    constexpr int RUN_BYTES = LP_NPX * KK * 4, PIECES = (RUN_BYTES + 1023) / 1024;
    extern __shared__ __attribute__((aligned(16))) float lp_smem[];      // (64*KK + C*KS*TWD) floats: 40 744 B at ks 11, C 3 -> 4 per CU
    float* wl = lp_smem;
    float* tl = lp_smem + LP_NPX * KK;
    const int lane = threadIdx.x & 63;
    const int wave = NWV > 1 ? __builtin_amdgcn_readfirstlane(threadIdx.x >> 6) : 0;
    const int x0 = blockIdx.x * LP_NPX, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(LP_NPX, W - x0);
    const int bytes = npx * KK * 4;                          // multiple of 16 (W % 4 == 0)
    const char* src = reinterpret_cast<const char*>(psf + ((size_t)(b * H + y) * W + x0) * KK);
#pragma unroll
    for (int p = 0; p < PIECES; ++p) {
        if (NWV > 1 && p % NWV != wave) continue;           // the waves of a workgroup share the run's pieces
        const int off = p * 1024 + lane * 16;
        if (off < bytes)
            __builtin_amdgcn_global_load_lds((lp_gptr_t)(src + off), (lp_lptr_t)(reinterpret_cast<char*>(wl) + p * 1024), 16, 0, AADFF_LP_DMA_AUX);
    }
    stage_window<KS, CN, NWV>(img, tl, b, C, H, W, y, x0, lane, wave);
    __syncthreads();                                         // also waits for the DMA pieces (vmcnt(0))
    constexpr int MC = CN > 0 ? CN : LP_MAXC;
    const float* wr = wl + lane * KK;
    float acc[MC] = {};
    // One wave per SIMD cannot hide LDS latency by occupancy: read a whole tap row (KS taps + MC*KS window values)
    // into registers in one burst, one row ahead of the FMAs that consume it.  With NWV = 2 the tap rows alternate
    // between the two waves (half the compute latency per run: the workgroup spends more of its life with loads in flight).
    auto load_row = [&](int u, float (&w)[KS], float (&x)[MC][KS]) {
#pragma unroll
        for (int v = 0; v < KS; ++v) w[v] = wr[u * KS + v];
#pragma unroll
        for (int cc = 0; cc < MC; ++cc)
            if (CN > 0 || cc < C) {
#pragma unroll
                for (int v = 0; v < KS; ++v) x[cc][v] = tl[(cc * KS + u) * TWD + lane + v];
            }
    };
    float w0[KS], x0r[MC][KS], w1[KS], x1r[MC][KS];
    const int ustart = wave;                                 // rows ustart, ustart + NWV, ...
    if (ustart < KS) load_row(ustart, w0, x0r);
#pragma unroll
    for (int k = 0; k < (KS + NWV - 1) / NWV; ++k) {
        const int u = ustart + k * NWV;
        if (u >= KS) break;
        if (u + NWV < KS) {
            if (k & 1) load_row(u + NWV, w0, x0r); else load_row(u + NWV, w1, x1r);
        }
        asm volatile("" ::: "memory");                       // keep the next row's reads ahead of this row's FMAs
#pragma unroll
        for (int v = 0; v < KS; ++v) {
#pragma unroll
            for (int cc = 0; cc < MC; ++cc)
                if (CN > 0 || cc < C) acc[cc] = fmaf((k & 1) ? x1r[cc][v] : x0r[cc][v], (k & 1) ? w1[v] : w0[v], acc[cc]);
        }
    }
    if (NWV > 1) {                                           // wave 1 hands its partial sums over through the (now free) tap buffer
        __syncthreads();
        if (wave != 0) {
#pragma unroll
            for (int cc = 0; cc < MC; ++cc) wl[((wave - 1) * MC + cc) * 64 + lane] = acc[cc];
        }
        __syncthreads();
        if (wave != 0) return;
#pragma unroll
        for (int w = 1; w < NWV; ++w)
#pragma unroll
            for (int cc = 0; cc < MC; ++cc) acc[cc] += wl[((w - 1) * MC + cc) * 64 + lane];
    }
    if (lane >= npx) return;
#pragma unroll
    for (int cc = 0; cc < MC; ++cc)
        if (CN > 0 || cc < C) out[((size_t)(b * C + cc) * H + y) * W + x0 + lane] = acc[cc];
}

// any odd ks / any channel count: PSFs through LDS (the previous design), correctness path
template <int NPX>
__global__ __launch_bounds__(64) void local_psf_generic_kernel(const float* __restrict__ img, const float* __restrict__ psf,
                                                                float* __restrict__ out, int C, int H, int W, int ks) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int kk = ks * ks, pad = ks / 2, tw = NPX + ks - 1;
    float* wl = smem;                 // [NPX][kk]
    float* tl = smem + NPX * kk;      // [C][ks][tw]
    const int lane = threadIdx.x;
    const int x0 = blockIdx.x * NPX, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(NPX, W - x0);

    const float* pp = psf + ((size_t)(b * H + y) * W + x0) * kk;
    for (int e = lane; e < npx * kk; e += kWave) wl[e] = pp[e];
    for (int e = lane; e < C * ks * tw; e += kWave) {
        const int cc = e / (ks * tw), rem = e - cc * ks * tw;
        const int u = rem / tw, xx = rem - u * tw;
        const int yy = min(max(y - pad + u, 0), H - 1);
        const int xs = min(max(x0 - pad + xx, 0), W - 1);
        tl[e] = img[((size_t)(b * C + cc) * H + yy) * W + xs];
    }
    __syncthreads();
    if (lane < npx) {
        const float* wr = wl + lane * kk;
        for (int cc = 0; cc < C; ++cc) {
            const float* tr = tl + cc * ks * tw + lane;
            float acc = 0.f;
            for (int u = 0; u < ks; ++u)
                for (int v = 0; v < ks; ++v) acc = fmaf(tr[u * tw + v], wr[u * ks + v], acc);
            out[((size_t)(b * C + cc) * H + y) * W + x0 + lane] = acc;
        }
    }
}

// ------------------------------------------------------------------------------------
// (b1) d_psf of the per-pixel gather: d_psf[b][y][x][a][e] = sum_c dy[b][c][y][x] * img[b][c][clamp(y + a - p)][clamp(x + e - p)].
// C FMAs per output, bound by the B H W ks^2 floats it writes: a workgroup writes the contiguous run of 64 pixels' PSF gradients,
// consecutive threads consecutive floats; the image window comes through the caches (every pixel is read ks^2 times).
// ------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(256) void local_dpsf_kernel(const float* __restrict__ img, const float* __restrict__ dy, float* __restrict__ dpsf,
                                                         int C, int H, int W, int ks_rt) {
    const int ks = KS > 0 ? KS : ks_rt, kk = ks * ks, p = ks / 2;
    const int x0 = blockIdx.x * 64, y = blockIdx.y, b = blockIdx.z;
    const int npx = min(64, W - x0);
    float* out = dpsf + (((size_t)b * H + y) * W + x0) * kk;
    const size_t hw = (size_t)H * W;
    const float* ib = img + (size_t)b * C * hw;
    const float* db = dy + (size_t)b * C * hw + (size_t)y * W + x0;
    for (int idx = threadIdx.x; idx < npx * kk; idx += 256) {
        const int px = idx / kk, t = idx - px * kk;
        const int a = t / ks, e = t - a * ks;
        const int yy = min(max(y + a - p, 0), H - 1), xx = min(max(x0 + px + e - p, 0), W - 1);
        const float* ip = ib + (size_t)yy * W + xx;
        float acc = 0.f;
        for (int cc = 0; cc < C; ++cc) acc = fmaf(db[cc * hw + px], ip[cc * hw], acc);
        out[idx] = acc;
    }
}

// (b2) d_img of the per-pixel gather: gather_adjoint (gather_window.h) on image b = blockIdx.z of a contiguous [B,C,H,W] batch
__global__ __launch_bounds__(64) void local_dimg_kernel(const float* __restrict__ psf, const float* __restrict__ dy, float* __restrict__ dimg,
                                                        int C, int H, int W, int ks) {
    const size_t b = blockIdx.z, hw = (size_t)H * W;
    gather_adjoint<false>(psf + b * hw * ks * ks, dy + b * C * hw, hw, dimg + b * C * hw, hw, C, H, W, ks);
}

// the shape domain of the per-pixel gather, shared by its forward and its backward
int local_check_shape(int B, int C, int H, int W, int ks) {
    AADFF_CHECK_ARG(B > 0 && C > 0 && H > 0 && W > 0, "local_psf_render: empty tensor");
    AADFF_CHECK_ARG(ks % 2 == 1 && ks >= 1 && ks <= AADFF_MAX_KS, "local_psf_render: ks %d must be odd and <= %d", ks, AADFF_MAX_KS);
    AADFF_CHECK_ARG(H <= 65535 && B <= 65535, "local_psf_render: H or B too large for the launch grid");
    if (!(C <= LP_MAXC && (ks == 3 || ks == 5 || ks == 7 || ks == 9 || ks == 11 || ks == 13))) {       // generic kernel: PSFs and window in LDS
        const int npx = ks <= 15 ? 64 : 16;
        const size_t lds = ((size_t)npx * ks * ks + (size_t)C * ks * (npx + ks - 1)) * sizeof(float);
        AADFF_CHECK_ARG(lds <= 160 * 1024, "local_psf_render: C=%d ks=%d needs %zu B of LDS", C, ks, lds);
    }
    return 0;
}

}  // namespace aadff

using namespace aadff;

extern "C" {

int aadff_local_psf_render(const float* img, const float* psf, float* out, int B, int C, int H, int W, int ks,
                           aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && psf && out, "local_psf_render: NULL pointer");
    if (int rc = local_check_shape(B, C, H, W, ks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (C <= LP_MAXC && (ks == 3 || ks == 5 || ks == 7 || ks == 9 || ks == 11 || ks == 13)) {
        dim3 g((W + LP_NPX - 1) / LP_NPX, H, B);
        // LDS-DMA form needs 16-byte aligned runs (rows of W*ks*ks floats, W % 4 == 0); AADFF_LOCAL_PSF=direct forces the
        // per-lane streaming form for A/B runs
        static const bool force_direct = [] { const char* e = std::getenv("AADFF_LOCAL_PSF"); return e && e[0] == 'd'; }();
        const bool dma = !force_direct && W % 4 == 0 && (reinterpret_cast<uintptr_t>(psf) & 15) == 0;
        const size_t dlds = (size_t)(64 * ks * ks + C * ks * (64 + ks - 1)) * sizeof(float);
        // waves per workgroup (they split the run's DMA pieces, window rows and tap rows; ks 11 at 1024^2: 1 -> 145 us,
        // 2 -> 122, 4 -> 101, 8 -> 111; ks 5: 2 -> 25, 4 -> 27): 4 for ks >= 9, 2 below
#define AADFF_LPC(K, CN) do { constexpr int NWV_ = K >= 9 ? 4 : 2; \
                              if (dma) hipLaunchKernelGGL((local_psf_dma_kernel<K, CN, NWV_>), g, dim3(64 * NWV_), dlds, st, img, psf, out, C, H, W); \
                              else hipLaunchKernelGGL((local_psf_kernel<K, CN>), g, dim3(64), 0, st, img, psf, out, C, H, W); } while (0)
#define AADFF_LP(K) case K: if (C == 3) AADFF_LPC(K, 3); else if (C == 1) AADFF_LPC(K, 1); else AADFF_LPC(K, 0); break;
        switch (ks) {
            AADFF_LP(3) AADFF_LP(5) AADFF_LP(7) AADFF_LP(9) AADFF_LP(11) AADFF_LP(13)
        }
#undef AADFF_LP
#undef AADFF_LPC
    } else {
        const int npx = ks <= 15 ? 64 : 16;
        const size_t lds = ((size_t)npx * ks * ks + (size_t)C * ks * (npx + ks - 1)) * sizeof(float);
        dim3 g((W + npx - 1) / npx, H, B);
        if (npx == 64) {
            if (lds > 64 * 1024)
                AADFF_CHECK_HIP(hipFuncSetAttribute((const void*)local_psf_generic_kernel<64>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(local_psf_generic_kernel<64>, g, dim3(64), lds, st, img, psf, out, C, H, W, ks);
        } else {
            if (lds > 64 * 1024)
                AADFF_CHECK_HIP(hipFuncSetAttribute((const void*)local_psf_generic_kernel<16>, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds));
            hipLaunchKernelGGL(local_psf_generic_kernel<16>, g, dim3(64), lds, st, img, psf, out, C, H, W, ks);
        }
    }
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_local_psf_render_bwd(const float* img, const float* psf, const float* dy, float* d_img_or_null, float* d_psf_or_null, int B, int C,
                               int H, int W, int ks, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && psf && dy, "local_psf_render_bwd: NULL pointer (img, psf, dy)");
    AADFF_CHECK_ARG(d_img_or_null || d_psf_or_null, "local_psf_render_bwd: d_img and d_psf are both NULL");
    if (int rc = local_check_shape(B, C, H, W, ks)) return rc;
    hipStream_t st = (hipStream_t)stream;
    dim3 g((W + 63) / 64, H, B);
    if (d_img_or_null) {
        hipLaunchKernelGGL(local_dimg_kernel, g, dim3(64), 0, st, psf, dy, d_img_or_null, C, H, W, ks);
        AADFF_CHECK_LAUNCH();
    }
    if (d_psf_or_null) {
        if (ks == 11) hipLaunchKernelGGL(local_dpsf_kernel<11>, g, dim3(256), 0, st, img, dy, d_psf_or_null, C, H, W, ks);
        else hipLaunchKernelGGL(local_dpsf_kernel<0>, g, dim3(256), 0, st, img, dy, d_psf_or_null, C, H, W, ks);
        AADFF_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
