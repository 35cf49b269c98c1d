// Device primitives of the per-pixel PSF gather, shared by every unit that gathers over a 64-pixel run of one image row
// (gather.hip, thinlens.hip) or back-propagates through the gather (gather.hip, psfnet_bwd.hip).
#pragma once
#include "common.h"

namespace aadff {

constexpr int LP_NPX = 64, LP_MAXC = 4;

// Replicate-clamped image window [C][KS][64+KS-1] of one 64-pixel run into LDS.  Every (channel, row) is one coalesced
// load of 64 floats plus a KS-1 float tail, and ALL of them are issued before the first is written to LDS: as a loop of
// dependent load -> store iterations this staging was a chain of ~38 memory latencies per run and, not the PSF stream,
// set the speed of the gather kernels (measured: 196 -> see DESIGN.md).
template <int KS, int CN, int NWV = 1>      // CN > 0: compile-time channel count (no per-channel branches); CN == 0: runtime C <= LP_MAXC
__device__ __forceinline__ void stage_window(const float* __restrict__ img, float* tl, int b, int C, int H, int W, int y, int x0, int lane,
                                             int wave = 0) {                            // NWV waves share the rows: row index % NWV == wave
    constexpr int PAD = KS / 2, TWD = LP_NPX + KS - 1;
    constexpr int MC = CN > 0 ? CN : LP_MAXC;
    float v0[MC * KS], v1[MC * KS];
    const int xa = min(max(x0 - PAD + lane, 0), W - 1);
    const int xb = min(max(x0 - PAD + LP_NPX + lane, 0), W - 1);
#pragma unroll
    for (int cc = 0; cc < MC; ++cc) {
        if (CN > 0 || cc < C) {
#pragma unroll
            for (int u = 0; u < KS; ++u) {
                if (NWV > 1 && (cc * KS + u) % NWV != wave) continue;
                const int yy = min(max(y - PAD + u, 0), H - 1);
                const float* row = img + ((size_t)(b * C + cc) * H + yy) * W;
                v0[cc * KS + u] = row[xa];
                v1[cc * KS + u] = lane < KS - 1 ? row[xb] : 0.f;
            }
        }
    }
#pragma unroll
    for (int cc = 0; cc < MC; ++cc) {
        if (CN > 0 || cc < C) {
#pragma unroll
            for (int u = 0; u < KS; ++u) {
                if (NWV > 1 && (cc * KS + u) % NWV != wave) continue;
                tl[(cc * KS + u) * TWD + lane] = v0[cc * KS + u];
                if (lane < KS - 1) tl[(cc * KS + u) * TWD + LP_NPX + lane] = v1[cc * KS + u];
            }
        }
    }
}

// Adjoint of the per-pixel gather for ONE image: every (pixel (y, x), tap (a, e)) whose replicate-clamped source is (Y, X) contributes
// dy[c][y][x] * psf[y][x][a][e].  Inside the image that is one tap per source pixel of the ks x ks window (a = Y - y + p);
// on the first / last row the taps that clamp onto it (a <= p - y, a >= H - 1 - y + p), the same in x.  One thread per (Y, X) =
// (blockIdx.y, 64 blockIdx.x + threadIdx.x), the PSF value read once for up to 4 channels.  Sums: one partial per source row, added
// to the pixel's accumulator in row order.
//   psf [H][W][ks][ks];  dy, dimg: channel c's plane [H][W] at + c * its channel stride;  ACCUMULATE: dimg += instead of dimg =
template <bool ACCUMULATE>
__device__ __forceinline__ void gather_adjoint(const float* __restrict__ psf, const float* __restrict__ dy, size_t dy_cstride,
                                               float* __restrict__ dimg, size_t dimg_cstride, int C, int H, int W, int ks) {
    const int kk = ks * ks, p = ks / 2;
    const int X = blockIdx.x * 64 + threadIdx.x, Y = blockIdx.y;
    if (X >= W) return;
    const int y_lo = max(Y - p, 0), y_hi = min(Y + p, H - 1), x_lo = max(X - p, 0), x_hi = min(X + p, W - 1);
    for (int c0 = 0; c0 < C; c0 += 4) {
        const int nc = min(4, C - c0);
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        for (int y = y_lo; y <= y_hi; ++y) {
            const int a_lo = Y == 0 ? 0 : Y - y + p, a_hi = Y == H - 1 ? ks - 1 : Y - y + p;
            float part[4] = {0.f, 0.f, 0.f, 0.f};
            for (int x = x_lo; x <= x_hi; ++x) {
                const int e_lo = X == 0 ? 0 : X - x + p, e_hi = X == W - 1 ? ks - 1 : X - x + p;
                const float* dp = dy + (size_t)c0 * dy_cstride + (size_t)y * W + x;
                float dv[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) dv[j] = j < nc ? dp[j * dy_cstride] : 0.f;
                const float* pp = psf + ((size_t)y * W + x) * kk;
                for (int a = a_lo; a <= a_hi; ++a)
                    for (int e = e_lo; e <= e_hi; ++e) {
                        const float w = pp[a * ks + e];
#pragma unroll
                        for (int j = 0; j < 4; ++j) part[j] = fmaf(dv[j], w, part[j]);
                    }
            }
#pragma unroll
            for (int j = 0; j < 4; ++j) acc[j] += part[j];
        }
        for (int j = 0; j < nc; ++j) {
            float* o = dimg + (c0 + j) * dimg_cstride + (size_t)Y * W + X;
            *o = ACCUMULATE ? *o + acc[j] : acc[j];
        }
    }
}

}  // namespace aadff
