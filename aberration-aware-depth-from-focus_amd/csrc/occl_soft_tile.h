// The soft-depth-layer form of the occlusion-aware layered render (conv_occl_soft.hip): the layers are NODES in depth, a texel carries a
// continuous layer coordinate pos, lies in slab k = (int)min(pos, L-1) and is blurred with the PSF interpolated linearly between nodes k
// and k + 1 by f = pos - k.  This header adds the slab decode, the staging of the image tile with the slab byte AND the fraction f, and
// the two {q, a} chain passes of one slab; the tile enumeration, the presence word, `composite`, `resolve` and the argument domain are
// occl_tile.h's, whose code the hard forward and backward compile unchanged.  Contract: include/aadff.h
// (aadff_render_psf_map_stack_soft_occluded); design: DESIGN.md 4.22.
#pragma once
#include "occl_tile.h"

namespace aadff {

constexpr unsigned kSoftHole = 255u;          // the slab byte of a hole: never equal to a slab index (< 32)

// pos -> (slab byte, fraction).  !(pos >= 0) (NaN included) is a hole; else p = min(pos, L-1), k = min((int)p, L-1), f = p - k: exact
// in float32 (p and k share a binade or k = 0), in [0, 1), and 0 whenever k = L-1 (then p = L-1).
__device__ __forceinline__ void soft_slab(float pos, int L, unsigned& k, float& f) {
    if (!(pos >= 0.f)) { k = kSoftHole; f = 0.f; return; }
    const float p = fminf(pos, (float)(L - 1));
    int ki = (int)p;
    ki = ki < L - 1 ? ki : L - 1;
    k = (unsigned)ki;
    f = __fsub_rn(p, (float)ki);
}

// Templated sizes: occl_stage with the fraction tile beside the image tile (same pitch) and two words per wave: word_w[wave] the slabs
// present, word_w[ONW + wave] the slabs that hold a texel with f != 0 (only those need the second pass).
template <int KS>
__device__ __forceinline__ void occl_soft_stage(const float* __restrict__ plane, const float* __restrict__ pplane, float* tile, float* ftile,
                                                unsigned char* ltile, unsigned* word_w, int x0, int y0, int L, int H, int W, int lane, int wave) {
    using Cfg = OcclCfg<KS>;
    constexpr int P = Cfg::P, PB = Cfg::PB;
    constexpr int NR = (Cfg::THP + ONW - 1) / ONW;
    const int xx = reflect_idx(x0 - Cfg::PAD + lane, W);
    float v[NR], pv[NR];
    unsigned seen = 0, frac = 0;
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int r = wave + j * ONW;
        const int yy = reflect_idx(y0 - Cfg::PAD + r, H);
        const bool in = lane < Cfg::TWP && r < Cfg::THP;
        v[j] = in ? plane[(size_t)yy * W + xx] : 0.f;
        pv[j] = in ? pplane[(size_t)yy * W + xx] : -1.f;
    }
#pragma unroll
    for (int j = 0; j < NR; ++j) {
        const int r = wave + j * ONW;
        if (lane < Cfg::TWP && r < Cfg::THP) {
            unsigned k;
            float f;
            soft_slab(pv[j], L, k, f);
            tile[r * P + lane] = v[j];
            ftile[r * P + lane] = f;
            ltile[r * PB + lane] = (unsigned char)k;
            if (k < (unsigned)L) {
                seen |= 1u << k;
                if (f != 0.f) frac |= 1u << k;
            }
        }
    }
    seen = wave_or(seen);
    frac = wave_or(frac);
    if (lane == 0) { word_w[wave] = seen; word_w[ONW + wave] = frac; }
}

// Templated sizes: one pass of the {q, a} chains of slab l, the row walk of occl_chains.  PASS 0: inputs {x0, m0} = {fl(fl(1 - f) x),
// fl(1 - f)} against w = w_l; PASS 1: {x1, m1} = {fl(f x), f} against w = w_{l+1}.  Each input is a select on the slab byte.
template <int KS, int PASS>
__device__ __forceinline__ void occl_soft_chains(const float* trow, const float* frow, const unsigned char* lrow, const float* __restrict__ w,
                                                 int G, int l, f2 (&acc)[ORR][OCX]) {
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
            const float4* fp = reinterpret_cast<const float4*>(frow + rho * P);
            const unsigned* lp = reinterpret_cast<const unsigned*>(lrow + rho * PB);
#pragma unroll
            for (int h = 0; h < Cfg::NV; ++h) {
                const float4 t = ap[h], ff = fp[h];
                const unsigned lw = lp[h];
                const float xs[4] = {t.x, t.y, t.z, t.w}, fs[4] = {ff.x, ff.y, ff.z, ff.w};
#pragma unroll
                for (int e = 0; e < 4; ++e) {
                    const bool on = ((lw >> (8 * e)) & 255u) == (unsigned)l;
                    const float m = PASS ? fs[e] : __fsub_rn(1.f, fs[e]);
                    in[4 * h + e] = (f2){on ? __fmul_rn(m, xs[e]) : 0.f, on ? m : 0.f};   // a select: nothing of another slab passes
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

// Run-time ks: the image tile, the fraction tile and the slab bytes in dynamic LDS (2 (32 + ks - 1)^2 floats and as many bytes), 256
// threads; word_w as in occl_soft_stage.
__device__ __forceinline__ void occl_soft_stage_generic(const float* __restrict__ plane, const float* __restrict__ pplane, float* gtile,
                                                        float* gf, unsigned char* gl, unsigned* word_w, int x0, int y0, int pad, int twp,
                                                        int thp, int L, int H, int W, int tid) {
    unsigned seen = 0, frac = 0;
    for (int e = tid; e < thp * twp; e += 256) {
        const int r = e / twp, cc = e - r * twp;
        const size_t src = (size_t)reflect_idx(y0 - pad + r, H) * W + reflect_idx(x0 - pad + cc, W);
        unsigned k;
        float f;
        soft_slab(pplane[src], L, k, f);
        gtile[e] = plane[src];
        gf[e] = f;
        gl[e] = (unsigned char)k;
        if (k < (unsigned)L) {
            seen |= 1u << k;
            if (f != 0.f) frac |= 1u << k;
        }
    }
    seen = wave_or(seen);
    frac = wave_or(frac);
    if ((tid & 63) == 0) { word_w[tid >> 6] = seen; word_w[4 + (tid >> 6)] = frac; }
}

static inline size_t occl_soft_generic_lds(int ks) {
    const size_t n = (size_t)(OT + ks - 1) * (OT + ks - 1);
    return 2 * n * sizeof(float) + ((n + 3) & ~(size_t)3);
}

// Run-time ks: one pass of the chains of slab l for thread (lx, ly), the tap walk of occl_chains_generic.
template <int PASS>
__device__ __forceinline__ void occl_soft_chains_generic(const float* gtile, const float* gf, const unsigned char* gl,
                                                         const float* __restrict__ w, int G, int ks, int twp, int lx, int ly, int l,
                                                         float (&qa)[4], float (&aa)[4]) {
#pragma unroll
    for (int r = 0; r < 4; ++r) { qa[r] = 0.f; aa[r] = 0.f; }
    for (int u = 0; u < ks; ++u) {
        const size_t mo = (size_t)(ks - 1 - u) * G + (ks - 1);
        const int base = (4 * ly + u) * twp + lx;
        for (int v = 0; v < ks; ++v) {
            const float wt = w[mo - v];
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                const int e = base + r * twp + v;
                const bool on = gl[e] == (unsigned char)l;
                const float m = PASS ? gf[e] : __fsub_rn(1.f, gf[e]);
                qa[r] = __fmaf_rn(wt, on ? __fmul_rn(m, gtile[e]) : 0.f, qa[r]);
                aa[r] = __fmaf_rn(wt, on ? m : 0.f, aa[r]);
            }
        }
    }
}

}  // namespace aadff
