// Occlusion-aware layered PSF-map rendering for gfx950 (MI355X): every depth layer's premultiplied image and its mask are blurred with
// that layer's grid PSF and the layers are composited front to back with a transmittance, in one launch per stack.
// Semantics and arithmetic contract: include/aadff.h (aadff_render_psf_map_stack_occluded); design: DESIGN.md 4.20.
//
// Modelled on conv_blend.hip: a workgroup is one 32 x 32 tile of ONE patch and ONE (b, c) plane, the reflect-padded image tile and the
// reflect-padded layer-byte tile are staged in LDS once for all S slices, waves take slices w, w + 4, ..., taps are wave-uniform scalar
// loads.  Per layer a lane keeps one {q, a} pair per output (radiance and coverage share every tap, so the two chains are the two halves
// of one packed FMA), and V, A, T across layers.  At staging the workgroup builds the 32-bit mask of the layers present in the staged
// tile; the layer loop visits only its set bits (a layer that is absent adds fma(T, 0, V): no bit changes).  Plain fp32 FMA chains in a
// fixed tap order, no atomics, every output written once: bit-reproducible.  The tile enumeration, the staging and the chains are in
// occl_tile.h, shared with the backward (conv_occl_bwd.hip).
#include "occl_tile.h"

namespace aadff {

// Fast path, ks in {3,5,7,9,11,13,15,21}.  Per slice and layer present the wave walks the KS + 3 staged rows its 4 output rows read:
// row rho is read once (ds_read_b128 + the layer bytes), masked once into {x or 0, 1 or 0} pairs, and feeds output row r with tap row
// u = rho - r wherever 0 <= u < KS (wave-uniform), so every output's chain runs over its window in row-major order (u, then v).
template <int KS>
__global__ __launch_bounds__(64 * ONW) void conv_occl_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, const unsigned char* __restrict__ layer, float* __restrict__ out,
    float* __restrict__ cov, int C, int S, int L, int H, int W, int grid, int normalize, OcclPatches pb) {
    using Cfg = OcclCfg<KS>;
    constexpr int P = Cfg::P, PB = Cfg::PB;
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

    occl_stage<KS>(img + (size_t)plane_i * H * W, layer + (size_t)b * H * W, tile, ltile, present_w, x0, y0, L, H, W, lane, wave);
    __syncthreads();
    const unsigned present = occl_present(present_w);

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
            occl_chains<KS>(trow, lrow, w, G, l, acc);
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
    occl_stage_generic(img + (size_t)plane_i * H * W, layer + (size_t)b * H * W, gtile, gl, present_w, x0, y0, pad, twp, thp, L, H, W, tid);
    __syncthreads();
    const unsigned present = occl_present(present_w);

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
            occl_chains_generic(gtile, gl, w, G, ks, twp, lx, ly, l, qa, aa);
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
    if (int rc = occl_check_shape("render_psf_map_stack_occluded", B, C, S, L, H, W, grid, ks)) return rc;

    OcclPatches pb;
    std::memset(&pb, 0, sizeof(pb));
    const int nty = fill_occl_axis(pb.y, grid, H), ntx = fill_occl_axis(pb.x, grid, W);
    hipStream_t st = (hipStream_t)stream;
    dim3 g(ntx, nty, B * C);
    switch (ks) {
#define AADFF_CASE(K) case K: hipLaunchKernelGGL((conv_occl_kernel<K>), g, dim3(64 * ONW), 0, st, img, psf_maps, layer, out, coverage_or_null, C, S, L, H, W, grid, normalize, pb); break;
        AADFF_CASE(3) AADFF_CASE(5) AADFF_CASE(7) AADFF_CASE(9) AADFF_CASE(11) AADFF_CASE(13) AADFF_CASE(15) AADFF_CASE(21)
#undef AADFF_CASE
        default:
            hipLaunchKernelGGL(conv_occl_generic_kernel, g, dim3(256), occl_generic_lds(ks), st, img, psf_maps, layer, out, coverage_or_null, C, S, L, H, W,
                               grid, ks, normalize, pb);
    }
    AADFF_CHECK_LAUNCH();
    return 0;
}
