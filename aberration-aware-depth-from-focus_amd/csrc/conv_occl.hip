// Occlusion-aware layered PSF-map rendering for gfx950 (MI355X): every depth layer's premultiplied image and its mask are blurred with
// that layer's grid PSF and the layers are composited front to back with a transmittance, in one launch per stack.
// Semantics and arithmetic contract: include/aadff.h (aadff_render_psf_map_stack_occluded); design: DESIGN.md 4.20.
//
// Modelled on conv_blend.hip: a workgroup is one 32 x 32 tile of ONE patch and ONE (b, c) plane, the reflect-padded image tile and the
// reflect-padded layer-byte tile are staged in LDS once for all S slices, waves take slices w, w + 4, ..., taps are wave-uniform scalar
// loads.  Per layer a lane keeps one {q, a} pair per output (radiance and coverage share every tap, so the two chains are the two halves
// of one packed FMA), and V, A, T across layers.  At staging the workgroup builds the 32-bit mask of the layers present in the staged
// tile; the layer loop visits only its set bits (a layer that is absent adds fma(T, 0, V): no bit changes).  Plain fp32 FMA chains in a
// fixed tap order, no atomics, every output written once: bit-reproducible.
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
};

// Fast path, ks in {3,5,7,9,11,13,15,21}.  Per slice and layer present the wave walks the KS + 3 staged rows its 4 output rows read:
// row rho is read once (ds_read_b128 + the layer bytes), masked once into {x or 0, 1 or 0} pairs, and feeds output row r with tap row
// u = rho - r wherever 0 <= u < KS (wave-uniform), so every output's chain runs over its window in row-major order (u, then v).
template <int KS>
__global__ __launch_bounds__(64 * ONW) void conv_occl_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, const unsigned char* __restrict__ layer, float* __restrict__ out,
    float* __restrict__ cov, int C, int S, int L, int H, int W, int grid, int normalize, OcclPatches pb) {
    using Cfg = OcclCfg<KS>;
    constexpr int P = Cfg::P, PB = Cfg::PB;
    static_assert(Cfg::TWP <= kWave, "staging maps one tile column to one lane");
    static_assert(PB % 4 == 0 && PB >= Cfg::TWP && PB >= (OQN - 1) * OCX + 4 * Cfg::NV, "layer rows are read as whole dwords");
    __shared__ __attribute__((aligned(16))) float tile[Cfg::THP * P];
    __shared__ __attribute__((aligned(16))) unsigned char ltile[Cfg::THP * PB];
    __shared__ unsigned present_w[ONW];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pj = patch_of_tile(pb.x, grid, blockIdx.x), pi = patch_of_tile(pb.y, grid, blockIdx.y);
    const int x0 = pb.x.b[pj] + ((int)blockIdx.x - pb.x.ts[pj]) * OT, y0 = pb.y.b[pi] + ((int)blockIdx.y - pb.y.ts[pi]) * OT;
    const int x_hi = pb.x.b[pj + 1], y_hi = pb.y.b[pi + 1];
    const int plane_i = blockIdx.z, c = plane_i % C, b = plane_i / C;
    if (x0 >= x_hi || y0 >= y_hi) return;                       // (never: only non-empty tiles are enumerated)

    {   // stage: column = lane (reflected once), rows strided over the waves; every load in flight before the first LDS write
        const float* plane = img + (size_t)plane_i * H * W;
        const unsigned char* lplane = layer + (size_t)b * H * W;
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
    __syncthreads();
    const unsigned present = __builtin_amdgcn_readfirstlane(present_w[0] | present_w[1] | present_w[2] | present_w[3]);

    const int q = lane % OQN, k = lane / OQN;
    const int x = x0 + OCX * q, yb = y0 + ORR * k;
    const int G = grid * KS;
    const float* trow = &tile[(ORR * k) * P + OCX * q];
    const unsigned char* lrow = &ltile[(ORR * k) * PB + OCX * q];
    for (int s = wave; s < S; s += ONW) {
        float V[ORR][OCX], A[ORR][OCX], T[ORR][OCX];
#pragma unroll
        for (int r = 0; r < ORR; ++r)
#pragma unroll
            for (int i = 0; i < OCX; ++i) { V[r][i] = 0.f; A[r][i] = 0.f; T[r][i] = 1.f; }

        for (unsigned rest = present; rest; rest &= rest - 1) {
            const int l = __builtin_ctz(rest);
            // conv2d is a correlation with the FLIPPED PSF: w(u,v) = psf[KS-1-u][KS-1-v] of tile (pi, pj) of map s L + l, channel c
            const float* w = psf + ((size_t)(s * L + l) * C + c) * G * G + ((size_t)pi * KS) * G + pj * KS;
            f2 acc[ORR][OCX];
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
#pragma unroll
            for (int r = 0; r < ORR; ++r)
#pragma unroll
                for (int i = 0; i < OCX; ++i) composite(acc[r][i].x, acc[r][i].y, V[r][i], A[r][i], T[r][i]);
        }

        const size_t o0 = ((size_t)plane_i * S + s) * H * W + (size_t)yb * W + x;
#pragma unroll
        for (int r = 0; r < ORR; ++r) {
            if (yb + r < y_hi) {
#pragma unroll
                for (int i = 0; i < OCX; ++i)
                    if (x + i < x_hi) {
                        out[o0 + (size_t)r * W + i] = resolve(V[r][i], A[r][i], normalize);
                        if (cov) cov[o0 + (size_t)r * W + i] = A[r][i];
                    }
            }
        }
    }
}

// Every other odd ks up to AADFF_MAX_KS: ks a run-time value, the two tiles in dynamic LDS ((32 + ks - 1)^2 floats and as many bytes,
// 33.6 KB at ks 51), 32 x 8 threads with four rows each, the slices one after the other; the taps are wave-uniform loads straight from
// the maps.  The same chains in the same tap order as the fast path.
__global__ __launch_bounds__(256) void conv_occl_generic_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, const unsigned char* __restrict__ layer, float* __restrict__ out,
    float* __restrict__ cov, int C, int S, int L, int H, int W, int grid, int ks, int normalize, OcclPatches pb) {
    extern __shared__ __attribute__((aligned(16))) float gtile[];
    __shared__ unsigned present_w[4];
    const int pad = ks / 2, twp = OT + ks - 1, thp = OT + ks - 1;
    unsigned char* gl = reinterpret_cast<unsigned char*>(gtile + thp * twp);
    const int tid = threadIdx.x;
    const int pj = patch_of_tile(pb.x, grid, blockIdx.x), pi = patch_of_tile(pb.y, grid, blockIdx.y);
    const int x0 = pb.x.b[pj] + ((int)blockIdx.x - pb.x.ts[pj]) * OT, y0 = pb.y.b[pi] + ((int)blockIdx.y - pb.y.ts[pi]) * OT;
    const int x_hi = pb.x.b[pj + 1], y_hi = pb.y.b[pi + 1];
    const int plane_i = blockIdx.z, c = plane_i % C, b = plane_i / C;
    if (x0 >= x_hi || y0 >= y_hi) return;
    const float* plane = img + (size_t)plane_i * H * W;
    const unsigned char* lplane = layer + (size_t)b * H * W;
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
    __syncthreads();
    const unsigned present = __builtin_amdgcn_readfirstlane(present_w[0] | present_w[1] | present_w[2] | present_w[3]);

    const int lx = tid & 31, ly = tid >> 5;
    const int x = x0 + lx, yb = y0 + 4 * ly;
    const int G = grid * ks;
    for (int s = 0; s < S; ++s) {
        float V[4], A[4], T[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { V[r] = 0.f; A[r] = 0.f; T[r] = 1.f; }
        for (unsigned rest = present; rest; rest &= rest - 1) {
            const int l = __builtin_ctz(rest);
            const float* w = psf + ((size_t)(s * L + l) * C + c) * G * G + ((size_t)pi * ks) * G + pj * ks;
            float qa[4], aa[4];
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
#pragma unroll
            for (int r = 0; r < 4; ++r) composite(qa[r], aa[r], V[r], A[r], T[r]);
        }
        const size_t o0 = ((size_t)plane_i * S + s) * H * W;
        if (x < x_hi) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (yb + r < y_hi) {
                    out[o0 + (size_t)(yb + r) * W + x] = resolve(V[r], A[r], normalize);
                    if (cov) cov[o0 + (size_t)(yb + r) * W + x] = A[r];
                }
        }
    }
}

}  // namespace aadff

using namespace aadff;

extern "C" int aadff_render_psf_map_stack_occluded(const float* img, const float* psf_maps, const unsigned char* layer, float* out,
                                                   float* coverage_or_null, int B, int C, int S, int L, int H, int W, int grid, int ks,
                                                   int normalize, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && psf_maps && layer && out, "render_psf_map_stack_occluded: NULL pointer");
    AADFF_CHECK_ARG(B > 0 && C > 0 && S > 0 && H > 0 && W > 0, "render_psf_map_stack_occluded: empty tensor (B=%d C=%d S=%d H=%d W=%d)", B, C, S, H, W);
    AADFF_CHECK_ARG(ks % 2 != 0, "PSF kernel size should be odd");
    AADFF_CHECK_ARG(ks >= 3 && ks <= AADFF_MAX_KS, "render_psf_map_stack_occluded: ks %d outside [3,%d]", ks, AADFF_MAX_KS);
    AADFF_CHECK_ARG(L >= 1 && L <= AADFF_RENDER_MAX_LAYERS, "render_psf_map_stack_occluded: L=%d layers outside [1,%d]", L, AADFF_RENDER_MAX_LAYERS);
    AADFF_CHECK_ARG(grid >= 1 && grid <= AADFF_MAX_GRID, "render_psf_map_stack_occluded: grid %d outside [1,%d]", grid, AADFF_MAX_GRID);
    AADFF_CHECK_ARG(grid <= H && grid <= W, "render_psf_map_stack_occluded: grid %d above min(H,W) = %d: a patch without a pixel", grid, H < W ? H : W);
    AADFF_CHECK_ARG(ks / 2 < H && ks / 2 < W, "render_psf_map_stack_occluded: reflect padding %d needs H,W > pad", ks / 2);
    AADFF_CHECK_ARG((size_t)B * C <= 65535, "render_psf_map_stack_occluded: B*C too large");
    AADFF_CHECK_ARG((size_t)S * L <= ((size_t)1 << 24), "render_psf_map_stack_occluded: S*L too large");
    AADFF_CHECK_ARG((size_t)H + (size_t)OT * grid <= (size_t)65535 * OT && (size_t)W + (size_t)OT * grid <= ((size_t)1 << 30),
                    "render_psf_map_stack_occluded: H=%d W=%d too large for the launch grid", H, W);

    OcclPatches pb;
    std::memset(&pb, 0, sizeof(pb));
    const int nty = fill_occl_axis(pb.y, grid, H), ntx = fill_occl_axis(pb.x, grid, W);
    hipStream_t st = (hipStream_t)stream;
    dim3 g(ntx, nty, B * C);
    switch (ks) {
#define AADFF_CASE(K) case K: hipLaunchKernelGGL((conv_occl_kernel<K>), g, dim3(64 * ONW), 0, st, img, psf_maps, layer, out, coverage_or_null, C, S, L, H, W, grid, normalize, pb); break;
        AADFF_CASE(3) AADFF_CASE(5) AADFF_CASE(7) AADFF_CASE(9) AADFF_CASE(11) AADFF_CASE(13) AADFF_CASE(15) AADFF_CASE(21)
#undef AADFF_CASE
        default: {
            const size_t n = (size_t)(OT + ks - 1) * (OT + ks - 1);
            const size_t lds = n * sizeof(float) + ((n + 3) & ~(size_t)3);
            hipLaunchKernelGGL(conv_occl_generic_kernel, g, dim3(256), lds, st, img, psf_maps, layer, out, coverage_or_null, C, S, L, H, W, grid, ks,
                               normalize, pb);
        }
    }
    AADFF_CHECK_LAUNCH();
    return 0;
}
