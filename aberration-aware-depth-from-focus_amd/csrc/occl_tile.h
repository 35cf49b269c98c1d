// What the occlusion-aware layered render (conv_occl.hip) and its backward (conv_occl_bwd.hip) share: the tile enumeration of a patch
// grid, the staging of the reflect-padded image and layer-byte tiles with the presence word, the {q, a} tap chains of one layer (the
// templated and the run-time-ks form), the composite step and the argument domain.  The backward recomputes q_l, a_l with exactly the
// forward's chains, so both units call the same code.  Contract: include/aadff.h; design: DESIGN.md 4.20, 4.21.
#pragma once
#include "common.h"

namespace aadff {

constexpr int OT = 32;                        // tile edge: OT x OT pixels of one patch
constexpr int OCX = 4, ORR = 4, OQN = OT / OCX;   // lane = (k = lane / 8, q = lane % 8): columns 4q .. 4q+3, rows 4k .. 4k+3
constexpr int ONW = 4;                        // waves per workgroup: wave w renders slices w, w + 4, ... from the one staged tile

typedef float f2 __attribute__((ext_vector_type(2)));

// One axis of the tile enumeration, by value in the kernel arguments (scalar loads): patch i covers b[i] <= p < b[i + 1]
// (b = int(i / grid * n), fill_bounds) and its tiles are ts[i] <= t < ts[i + 1].
struct OcclAxis {
    int b[AADFF_MAX_GRID + 1];
    int ts[AADFF_MAX_GRID + 1];
};
struct OcclPatches { OcclAxis y, x; };

__device__ __forceinline__ int patch_of_tile(const OcclAxis& a, int grid, int t) {
    int i = 0;
    while (i + 1 < grid && t >= a.ts[i + 1]) ++i;
    return i;
}

static inline int fill_occl_axis(OcclAxis& a, int grid, int n) {
    fill_bounds(a.b, grid, n);
    a.ts[0] = 0;
    for (int i = 0; i < grid; ++i) a.ts[i + 1] = a.ts[i] + (a.b[i + 1] - a.b[i] + OT - 1) / OT;
    return a.ts[grid];
}

__device__ __forceinline__ unsigned wave_or(unsigned v) {
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) v |= (unsigned)__shfl_xor((int)v, off, kWave);
    return v;
}

// step 6 of the contract for one layer, and step 7
__device__ __forceinline__ void composite(float q, float a, float& V, float& A, float& T) {
    V = __fmaf_rn(T, q, V);
    A = __fmaf_rn(T, a, A);
    T = __fmul_rn(T, fmaxf(__fsub_rn(1.f, a), 0.f));
}
__device__ __forceinline__ float resolve(float V, float A, int normalize) {
    return normalize ? (A > 0.f ? __fdiv_rn(V, A) : 0.f) : V;
}

template <int KS>
struct OcclCfg {
    static constexpr int PAD = KS / 2;
    static constexpr int TWP = OT + KS - 1, THP = OT + KS - 1;  // staged columns, rows
    static constexpr int NIN = OCX + KS - 1;                     // inputs a lane needs per row
    static constexpr int NV = (NIN + 3) / 4;                     // ds_read_b128 (image) / dwords of layer bytes per row
    // image pitch: the 16-B slot step between lane-rows (4 tile rows apart) is 8 (mod 16), so the lane-rows of a ds_read_b128 group
    // fall on disjoint bank quarters (the rule of BlendCfg in conv_blend.hip)
    static constexpr int need = (OQN - 1) * OCX + 4 * NV;
    static constexpr int P = (((need > TWP ? need : TWP) - 8 + 15) / 16) * 16 + 8;
    // layer-byte pitch in BYTES: four tile rows are PB bytes = PB / 4 * 4 dwords apart; PB = 8 (mod 32) puts the 4 x 8 lanes of a
    // ds_read_b32 half on 32 distinct banks
    static constexpr int PB = (((need > TWP ? need : TWP) - 8 + 31) / 32) * 32 + 8;
    static_assert(TWP <= kWave, "staging maps one tile column to one lane");
    static_assert(PB % 4 == 0 && PB >= TWP && PB >= (OQN - 1) * OCX + 4 * NV, "layer rows are read as whole dwords");
};

// Templated sizes: stage the tile of (x0, y0) of one (b, c) plane, 64 * ONW threads: column = lane (reflected once), rows strided over
// the waves; every load in flight before the first LDS write.  The caller's __syncthreads() follows; then `occl_present`.
template <int KS>
__device__ __forceinline__ void occl_stage(const float* __restrict__ plane, const unsigned char* __restrict__ lplane, float* tile,
                                           unsigned char* ltile, unsigned* present_w, int x0, int y0, int L, int H, int W, int lane, int wave) {
    using Cfg = OcclCfg<KS>;
    constexpr int P = Cfg::P, PB = Cfg::PB;
    constexpr int NR = (Cfg::THP + ONW - 1) / ONW;
    const int xx = reflect_idx(x0 - Cfg::PAD + lane, W);
    float v[NR];
    unsigned lv[NR];
    unsigned seen = 0;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int r = wave + j * ONW;
        const int yy = reflect_idx(y0 - Cfg::PAD + r, H);
        const bool in = lane < Cfg::TWP && r < Cfg::THP;
        v[j] = in ? plane[(size_t)yy * W + xx] : 0.f;
        lv[j] = in ? (unsigned)lplane[(size_t)yy * W + xx] : 255u;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int r = wave + j * ONW;
        if (lane < Cfg::TWP && r < Cfg::THP) {
            tile[r * P + lane] = v[j];
            ltile[r * PB + lane] = (unsigned char)lv[j];
            if (lv[j] < (unsigned)L) seen |= 1u << lv[j];
        }
    }
    seen = wave_or(seen);
    if (lane == 0) present_w[wave] = seen;
}

// the 32-bit mask of the layers present in the staged tile (four waves in either kernel form), wave-uniform
__device__ __forceinline__ unsigned occl_present(const unsigned* present_w) {
    return __builtin_amdgcn_readfirstlane(present_w[0] | present_w[1] | present_w[2] | present_w[3]);
}

// Templated sizes: the {q, a} chains of layer l for the lane's ORR x OCX outputs.  The wave walks the KS + 3 staged rows its 4 output
// rows read: row rho is read once (ds_read_b128 + the layer bytes), masked once into {x or 0, 1 or 0} pairs, and feeds output row r with
// tap row u = rho - r wherever 0 <= u < KS (wave-uniform), so every output's chain runs over its window in row-major order (u, then v).
// w: tile (pi, pj) of the layer's map and channel (conv2d is a correlation with the FLIPPED PSF: w(u,v) = psf[KS-1-u][KS-1-v]).
template <int KS>
__device__ __forceinline__ void occl_chains(const float* trow, const unsigned char* lrow, const float* __restrict__ w, int G, int l,
                                            f2 (&acc)[ORR][OCX]) {
    using Cfg = OcclCfg<KS>;
    constexpr int P = Cfg::P, PB = Cfg::PB;
#pragma unroll
    for (int r = 0; r < ORR; ++r)
#pragma unroll
        for (int i = 0; i < OCX; ++i) acc[r][i] = (f2){0.f, 0.f};

#pragma unroll 1
    for (int rho = 0; rho < KS + ORR - 1; ++rho) {
        f2 in[4 * Cfg::NV];
        {
            const float4* ap = reinterpret_cast<const float4*>(trow + rho * P);
            const unsigned* lp = reinterpret_cast<const unsigned*>(lrow + rho * PB);
#pragma unroll
            for (int h = 0; h < Cfg::NV; ++h) {
                const float4 t = ap[h];
                const unsigned lw = lp[h];
                const float xs[4] = {t.x, t.y, t.z, t.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool on = ((lw >> (8 * e)) & 255u) == (unsigned)l;
                    in[4 * h + e] = (f2){on ? xs[e] : 0.f, on ? 1.f : 0.f};          // a select: nothing of another layer passes
                }
            }
        }
#pragma unroll
        for (int r = 0; r < ORR; ++r) {
            const int u = rho - r;
            if (u >= 0 && u < KS) {                                 // wave-uniform
                const float* wr = w + (size_t)(KS - 1 - u) * G;
                float m[KS];                                        // wave-uniform: scalar registers
#pragma unroll
                for (int t = 0; t < KS; ++t) m[t] = wr[t];
#pragma unroll
                for (int v = 0; v < KS; ++v) {
                    const f2 mm = (f2){m[KS - 1 - v], m[KS - 1 - v]};
#pragma unroll
                    for (int i = 0; i < OCX; ++i) acc[r][i] = __builtin_elementwise_fma(mm, in[i + v], acc[r][i]);
                }
            }
        }
    }
}

// Run-time ks: the two tiles in dynamic LDS ((32 + ks - 1)^2 floats and as many bytes), 256 threads.
__device__ __forceinline__ void occl_stage_generic(const float* __restrict__ plane, const unsigned char* __restrict__ lplane, float* gtile,
                                                   unsigned char* gl, unsigned* present_w, int x0, int y0, int pad, int twp, int thp, int L,
                                                   int H, int W, int tid) {
    unsigned seen = 0;
    for (int e = tid; e < thp * twp; e += 256) {
        const int r = e / twp, cc = e - r * twp;
        const size_t src = (size_t)reflect_idx(y0 - pad + r, H) * W + reflect_idx(x0 - pad + cc, W);
        const unsigned lv = lplane[src];
        gtile[e] = plane[src];
        gl[e] = (unsigned char)lv;
        if (lv < (unsigned)L) seen |= 1u << lv;
    }
    seen = wave_or(seen);
    if ((tid & 63) == 0) present_w[tid >> 6] = seen;
}

static inline size_t occl_generic_lds(int ks) {
    const size_t n = (size_t)(OT + ks - 1) * (OT + ks - 1);
    return n * sizeof(float) + ((n + 3) & ~(size_t)3);
}

// Run-time ks: thread (lx, ly) owns column lx of rows 4 ly .. 4 ly + 3; the taps are wave-uniform loads straight from the map.  The
// same chains in the same tap order as the templated form.
__device__ __forceinline__ void occl_chains_generic(const float* gtile, const unsigned char* gl, const float* __restrict__ w, int G, int ks,
                                                    int twp, int lx, int ly, int l, float (&qa)[4], float (&aa)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { qa[r] = 0.f; aa[r] = 0.f; }
    for (int u = 0; u < ks; ++u) {
        const size_t mo = (size_t)(ks - 1 - u) * G + (ks - 1);
        const int base = (4 * ly + u) * twp + lx;
        for (int v = 0; v < ks; ++v) {
            const float m = w[mo - v];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const bool on = gl[base + r * twp + v] == (unsigned char)l;
                qa[r] = __fmaf_rn(m, on ? gtile[base + r * twp + v] : 0.f, qa[r]);
                aa[r] = __fmaf_rn(m, on ? 1.f : 0.f, aa[r]);
            }
        }
    }
}

// The argument domain of the forward and the backward entry (`who` names the entry in the message); 0 or AADFF_EINVAL.  No HIP call.
static inline int occl_check_shape(const char* who, int B, int C, int S, int L, int H, int W, int grid, int ks) {
    AADFF_CHECK_ARG(B > 0 && C > 0 && S > 0 && H > 0 && W > 0, "%s: empty tensor (B=%d C=%d S=%d H=%d W=%d)", who, B, C, S, H, W);
    AADFF_CHECK_ARG(ks % 2 != 0, "PSF kernel size should be odd");
    AADFF_CHECK_ARG(ks >= 3 && ks <= AADFF_MAX_KS, "%s: ks %d outside [3,%d]", who, ks, AADFF_MAX_KS);
    AADFF_CHECK_ARG(L >= 1 && L <= AADFF_RENDER_MAX_LAYERS, "%s: L=%d layers outside [1,%d]", who, L, AADFF_RENDER_MAX_LAYERS);
    AADFF_CHECK_ARG(grid >= 1 && grid <= AADFF_MAX_GRID, "%s: grid %d outside [1,%d]", who, grid, AADFF_MAX_GRID);
    AADFF_CHECK_ARG(grid <= H && grid <= W, "%s: grid %d above min(H,W) = %d: a patch without a pixel", who, grid, H < W ? H : W);
    AADFF_CHECK_ARG(ks / 2 < H && ks / 2 < W, "%s: reflect padding %d needs H,W > pad", who, ks / 2);
    AADFF_CHECK_ARG((size_t)B * C <= 65535, "%s: B*C too large", who);
    AADFF_CHECK_ARG((size_t)S * L <= ((size_t)1 << 24), "%s: S*L too large", who);
    AADFF_CHECK_ARG((size_t)H + (size_t)OT * grid <= (size_t)65535 * OT && (size_t)W + (size_t)OT * grid <= ((size_t)1 << 30),
                    "%s: H=%d W=%d too large for the launch grid", who, H, W);
    return 0;
}

}  // namespace aadff
