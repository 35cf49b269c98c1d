// Soft depth layers for the occlusion-aware layered PSF-map render, gfx950 (MI355X): the L maps of a slice are NODES in depth, every
// texel carries a continuous layer coordinate and is blurred with the PSF interpolated linearly between the two nodes around it, and
// the slabs between nodes are composited front to back as conv_occl.hip composites its layers, in one launch per stack.
// Semantics and arithmetic contract: include/aadff.h (aadff_render_psf_map_stack_soft_occluded); design: DESIGN.md 4.22.
//
// The shape is conv_occl.hip's: a workgroup is one 32 x 32 tile of ONE patch and ONE (b, c) plane, staged once for all S slices, waves
// take slices w, w + 4, ..., taps are wave-uniform scalar loads.  Staged per texel: the image value, the slab as a byte (255: a hole)
// and the fraction f as a float, so the slab test is the byte compare of the hard kernel.  Per slab present the row-walking chain
// routine runs twice: inputs {fl((1-f) x), 1-f} against node k's tile, then {fl(f x), f} against node k+1's; the two {q, a} pairs are
// added and composited.  A slab none of whose staged texels has f != 0 (wave-uniform) skips the second pass, which would produce exact
// zeros, and runs the hard kernel's own chain routine for the first (m0 = 1, x0 = x exactly), so integral coordinates run its code.
// Plain fp32 FMA chains in a fixed tap order, no atomics, every output written once: bit-reproducible.
#include "occl_soft_tile.h"

namespace aadff {

template <int KS>
__global__ __launch_bounds__(64 * ONW) void conv_occl_soft_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, const float* __restrict__ pos, float* __restrict__ out,
    float* __restrict__ cov, int C, int S, int L, int H, int W, int grid, int normalize, OcclPatches pb) {
    using Cfg = OcclCfg<KS>;
    constexpr int P = Cfg::P, PB = Cfg::PB;
    __shared__ __attribute__((aligned(16))) float tile[Cfg::THP * P];
    __shared__ __attribute__((aligned(16))) float ftile[Cfg::THP * P];
    __shared__ __attribute__((aligned(16))) unsigned char ltile[Cfg::THP * PB];
    __shared__ unsigned word_w[2 * ONW];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pj = patch_of_tile(pb.x, grid, blockIdx.x), pi = patch_of_tile(pb.y, grid, blockIdx.y);
    const int x0 = pb.x.b[pj] + ((int)blockIdx.x - pb.x.ts[pj]) * OT, y0 = pb.y.b[pi] + ((int)blockIdx.y - pb.y.ts[pi]) * OT;
    const int x_hi = pb.x.b[pj + 1], y_hi = pb.y.b[pi + 1];
    const int plane_i = blockIdx.z, c = plane_i % C, b = plane_i / C;
    if (x0 >= x_hi || y0 >= y_hi) return;                       // (never: only non-empty tiles are enumerated)

    occl_soft_stage<KS>(img + (size_t)plane_i * H * W, pos + (size_t)b * H * W, tile, ftile, ltile, word_w, x0, y0, L, H, W, lane, wave);
    __syncthreads();
    const unsigned present = occl_present(word_w), frac = occl_present(word_w + ONW);

    const int q = lane % OQN, k = lane / OQN;
    const int x = x0 + OCX * q, yb = y0 + ORR * k;
    const int G = grid * KS;
    const float* trow = &tile[(ORR * k) * P + OCX * q];
    const float* frow = &ftile[(ORR * k) * P + OCX * q];
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
            if (!(((frac >> l) & 1u) && l + 1 < L)) {            // wave-uniform: every staged texel of the slab has f = 0, so m0 = 1 and
                occl_chains<KS>(trow, lrow, w, G, l, acc);       // x0 = x exactly: the hard kernel's pass, the fraction tile not read
            } else {                                             // f != 0 implies l < L - 1: node l + 1 exists
                occl_soft_chains<KS, 0>(trow, frow, lrow, w, G, l, acc);
                f2 acc1[ORR][OCX];
                occl_soft_chains<KS, 1>(trow, frow, lrow, w + (size_t)C * G * G, G, l, acc1);
#pragma unroll
                for (int r = 0; r < ORR; ++r)
#pragma unroll
                    for (int i = 0; i < OCX; ++i) acc[r][i] = acc[r][i] + acc1[r][i];
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

// Every other odd ks up to AADFF_MAX_KS: ks a run-time value, the three tiles in dynamic LDS (2 (32 + ks - 1)^2 floats and as many
// bytes, 60.5 KB at ks 51), 32 x 8 threads with four rows each, the slices one after the other.  The same chains in the same tap order.
__global__ __launch_bounds__(256) void conv_occl_soft_generic_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, const float* __restrict__ pos, float* __restrict__ out,
    float* __restrict__ cov, int C, int S, int L, int H, int W, int grid, int ks, int normalize, OcclPatches pb) {
    extern __shared__ __attribute__((aligned(16))) float gtile[];
    __shared__ unsigned word_w[8];
    const int pad = ks / 2, twp = OT + ks - 1, thp = OT + ks - 1;
    float* gf = gtile + thp * twp;
    unsigned char* gl = reinterpret_cast<unsigned char*>(gf + thp * twp);
    const int tid = threadIdx.x;
    const int pj = patch_of_tile(pb.x, grid, blockIdx.x), pi = patch_of_tile(pb.y, grid, blockIdx.y);
    const int x0 = pb.x.b[pj] + ((int)blockIdx.x - pb.x.ts[pj]) * OT, y0 = pb.y.b[pi] + ((int)blockIdx.y - pb.y.ts[pi]) * OT;
    const int x_hi = pb.x.b[pj + 1], y_hi = pb.y.b[pi + 1];
    const int plane_i = blockIdx.z, c = plane_i % C, b = plane_i / C;
    if (x0 >= x_hi || y0 >= y_hi) return;
    occl_soft_stage_generic(img + (size_t)plane_i * H * W, pos + (size_t)b * H * W, gtile, gf, gl, word_w, x0, y0, pad, twp, thp, L, H, W, tid);
    __syncthreads();
    const unsigned present = occl_present(word_w), frac = occl_present(word_w + 4);

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
            if (!(((frac >> l) & 1u) && l + 1 < L)) {
                occl_chains_generic(gtile, gl, w, G, ks, twp, lx, ly, l, qa, aa);
            } else {
                occl_soft_chains_generic<0>(gtile, gf, gl, w, G, ks, twp, lx, ly, l, qa, aa);
                float q1[4], a1[4];
                occl_soft_chains_generic<1>(gtile, gf, gl, w + (size_t)C * G * G, G, ks, twp, lx, ly, l, q1, a1);
#pragma unroll
                for (int r = 0; r < 4; ++r) { qa[r] = __fadd_rn(qa[r], q1[r]); aa[r] = __fadd_rn(aa[r], a1[r]); }
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

extern "C" int aadff_render_psf_map_stack_soft_occluded(const float* img, const float* psf_maps, const float* pos, float* out,
                                                        float* coverage_or_null, int B, int C, int S, int L, int H, int W, int grid,
                                                        int ks, int normalize, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && psf_maps && pos && out, "render_psf_map_stack_soft_occluded: NULL pointer");
    if (int rc = occl_check_shape("render_psf_map_stack_soft_occluded", B, C, S, L, H, W, grid, ks)) return rc;

    OcclPatches pb;
    std::memset(&pb, 0, sizeof(pb));
    const int nty = fill_occl_axis(pb.y, grid, H), ntx = fill_occl_axis(pb.x, grid, W);
    hipStream_t st = (hipStream_t)stream;
    dim3 g(ntx, nty, B * C);
    switch (ks) {
#define AADFF_CASE(K) case K: hipLaunchKernelGGL((conv_occl_soft_kernel<K>), g, dim3(64 * ONW), 0, st, img, psf_maps, pos, out, coverage_or_null, C, S, L, H, W, grid, normalize, pb); break;
        AADFF_CASE(3) AADFF_CASE(5) AADFF_CASE(7) AADFF_CASE(9) AADFF_CASE(11) AADFF_CASE(13) AADFF_CASE(15) AADFF_CASE(21)
#undef AADFF_CASE
        default:
            hipLaunchKernelGGL(conv_occl_soft_generic_kernel, g, dim3(256), occl_soft_generic_lds(ks), st, img, psf_maps, pos, out,
                               coverage_or_null, C, S, L, H, W, grid, ks, normalize, pb);
    }
    AADFF_CHECK_LAUNCH();
    return 0;
}
