// Seam-free PSF-map rendering for gfx950 (MI355X): every pixel's PSF is the bilinear interpolation of the four grid PSFs whose
// nodes surround it (the space-variant blur of Efficient Filter Flow / Hirsch et al. 2010), computed straight from the
// [S,C,grid*ks,grid*ks] maps of psf_map.  Semantics: include/aadff.h (aadff_render_psf_map_blend_stack); design: DESIGN.md 4.18.
//
// The convolution is linear in the PSF, so the blend of the four PSFs is the blend of the four plain renders R(k,l), R(k,l+1),
// R(k+1,l), R(k+1,l+1) of render_psf (flip, reflect padding).  The host cuts each axis into the g-1 CELLS between consecutive nodes
// (the clamp margins folded into the outer cells): inside a cell the four PSFs are the same for every pixel, so a workgroup that
// renders one tile of one cell has wave-uniform taps (scalar operands), exactly as a patch tile of conv_psf_map_kernel has; each lane
// keeps four accumulators per output, one per corner PSF, and blends them at the end with its own fx, fy.  Plain fp32 FMA chains, no
// atomics, every output written once: bit-reproducible.
#include "blend_axis.h"

namespace aadff {

// from blend_axis.h: BlendAxis, BlendCells, BT, cell_of_tile, blend_frac, fill_axis, check_nodes
constexpr int BCX = 4, BRR = 4, BQN = BT / BCX;   // lane = (k = lane / 8, q = lane % 8): columns 4q .. 4q+3, rows 4k .. 4k+3
constexpr int BNW = 4;                        // waves per workgroup: wave w renders slices w, w + 4, ... from the one staged tile

// (1-fy) [(1-fx) a00 + fx a01] + fy [(1-fx) a10 + fx a11] in a fixed order of four roundings per row pair
__device__ __forceinline__ float blend4(float a00, float a01, float a10, float a11, float fx, float gx, float fy, float gy) {
    const float t0 = __fmaf_rn(fx, a01, __fmul_rn(gx, a00));
    const float t1 = __fmaf_rn(fx, a11, __fmul_rn(gx, a10));
    return __fmaf_rn(fy, t1, __fmul_rn(gy, t0));
}

template <int KS>
struct BlendCfg {
    static constexpr int PAD = KS / 2;
    static constexpr int TWP = BT + KS - 1, THP = BT + KS - 1;  // staged columns, rows
    static constexpr int NIN = BCX + KS - 1;                     // inputs a lane needs per row
    static constexpr int NV = (NIN + 3) / 4;                     // ds_read_b128 per row
    // pitch: the 16-B slot step between lane-rows (4 tile rows apart) is 8 (mod 16), so the lane-rows of a ds_read_b128 group
    // fall on disjoint bank quarters (the rule of ConvCfg in conv.hip)
    static constexpr int need = (BQN - 1) * BCX + 4 * NV;
    static constexpr int P = (((need > TWP ? need : TWP) - 8 + 15) / 16) * 16 + 8;
};

// Fast path, ks in {3,5,7,9,11,13,15,21}.  Workgroup = 4 waves = one 32 x 32 tile of ONE cell and ONE (b, c) plane; the
// reflect-padded image tile is staged in LDS once for all S slices.  Per slice and tap row u the wave holds the 4 x KS taps of the
// four corner PSFs in SGPRs (one tap row at a time: 84 scalars at ks 21), reads the four input rows its outputs need and issues
// 4 PSFs x 4 rows x 4 columns x KS FMAs with a scalar tap operand.
template <int KS>
__global__ __launch_bounds__(64 * BNW) void conv_blend_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, float* __restrict__ out, int C, int S, int H, int W, int grid,
    int ncy, int ncx, BlendCells bc) {
    using Cfg = BlendCfg<KS>;
    constexpr int P = Cfg::P;
    static_assert(Cfg::TWP <= kWave, "staging maps one tile column to one lane");
    __shared__ __attribute__((aligned(16))) float tile[Cfg::THP * P];

    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int cj = cell_of_tile(bc.x, ncx, blockIdx.x), ci = cell_of_tile(bc.y, ncy, blockIdx.y);
    const int x0 = bc.x.b[cj] + ((int)blockIdx.x - bc.x.ts[cj]) * BT, y0 = bc.y.b[ci] + ((int)blockIdx.y - bc.y.ts[ci]) * BT;
    const int x_hi = bc.x.b[cj + 1], y_hi = bc.y.b[ci + 1];
    const int plane_i = blockIdx.z, c = plane_i % C;
    if (x0 >= x_hi || y0 >= y_hi) return;                       // (never: only non-empty tiles are enumerated)

    {   // stage: column = lane (reflected once), rows strided over the waves; every load in flight before the first LDS write
        const float* plane = img + (size_t)plane_i * H * W;
        constexpr int NR = (Cfg::THP + BNW - 1) / BNW;
        const int xx = reflect_idx(x0 - Cfg::PAD + lane, W);
        float v[NR];
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int r = wave + j * BNW;
            const int yy = reflect_idx(y0 - Cfg::PAD + r, H);
            v[j] = (lane < Cfg::TWP && r < Cfg::THP) ? plane[(size_t)yy * W + xx] : 0.f;
        }
#pragma unroll
        for (int j = 0; j < NR; ++j) {
            const int r = wave + j * BNW;
            if (lane < Cfg::TWP && r < Cfg::THP) tile[r * P + lane] = v[j];
        }
    }
    __syncthreads();

    const int q = lane % BQN, k = lane / BQN;
    const int x = x0 + BCX * q, yb = y0 + BRR * k;
    const bool single = grid == 1;
    const int ci1 = min(ci + 1, grid - 1), cj1 = min(cj + 1, grid - 1);
    float fx[BCX], gx[BCX], fy[BRR], gy[BRR];
#pragma unroll
    for (int i = 0; i < BCX; ++i) {
        fx[i] = blend_frac(x + i, bc.x.node[cj], bc.x.node[cj1], single);
        gx[i] = __fsub_rn(1.f, fx[i]);
    }
#pragma unroll
    for (int r = 0; r < BRR; ++r) {
        fy[r] = blend_frac(yb + r, bc.y.node[ci], bc.y.node[ci1], single);
        gy[r] = __fsub_rn(1.f, fy[r]);
    }

    const int G = grid * KS;
    const float* trow = &tile[(BRR * k) * P + BCX * q];
    for (int s = wave; s < S; s += BNW) {
        // the four corner PSFs; conv2d is a correlation with the FLIPPED PSF: w(u,v) = psf[KS-1-u][KS-1-v]
        const float* map = psf + (size_t)(s * C + c) * G * G;
        const float* w00 = map + ((size_t)ci * KS) * G + cj * KS;
        const float* w01 = map + ((size_t)ci * KS) * G + cj1 * KS;
        const float* w10 = map + ((size_t)ci1 * KS) * G + cj * KS;
        const float* w11 = map + ((size_t)ci1 * KS) * G + cj1 * KS;
        float acc[4][BRR][BCX];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < BRR; ++r)
#pragma unroll
                for (int i = 0; i < BCX; ++i) acc[j][r][i] = 0.f;

#pragma unroll 1
        for (int u = 0; u < KS; ++u) {
            const size_t mo = (size_t)(KS - 1 - u) * G;
            float m[4][KS];                                     // wave-uniform: scalar registers
#pragma unroll
            for (int t = 0; t < KS; ++t) {
                m[0][t] = w00[mo + t];
                m[1][t] = w01[mo + t];
                m[2][t] = w10[mo + t];
                m[3][t] = w11[mo + t];
            }
#pragma unroll
            for (int r = 0; r < BRR; ++r) {
                float in[4 * Cfg::NV];
                const float4* ap = reinterpret_cast<const float4*>(trow + (r + u) * P);
#pragma unroll
                for (int h = 0; h < Cfg::NV; ++h) {
                    const float4 t = ap[h];
                    in[4 * h] = t.x; in[4 * h + 1] = t.y; in[4 * h + 2] = t.z; in[4 * h + 3] = t.w;
                }
#pragma unroll
                for (int v = 0; v < KS; ++v)
#pragma unroll
                    for (int j = 0; j < 4; ++j)
#pragma unroll
                        for (int i = 0; i < BCX; ++i) acc[j][r][i] = __fmaf_rn(m[j][KS - 1 - v], in[i + v], acc[j][r][i]);
            }
        }

        float* o = out + ((size_t)plane_i * S + s) * H * W + (size_t)yb * W + x;
#pragma unroll
        for (int r = 0; r < BRR; ++r) {
            if (yb + r < y_hi) {
#pragma unroll
                for (int i = 0; i < BCX; ++i)
                    if (x + i < x_hi) o[i] = blend4(acc[0][r][i], acc[1][r][i], acc[2][r][i], acc[3][r][i], fx[i], gx[i], fy[r], gy[r]);
            }
            o += W;
        }
    }
}

// Every other odd ks up to AADFF_MAX_KS: ks a run-time value, the tile in dynamic LDS ((32 + ks - 1)^2 floats, 26.9 KB at ks 51), 32 x 8
// threads with four rows each, the slices one after the other; the taps are wave-uniform loads straight from the maps.
__global__ __launch_bounds__(256) void conv_blend_generic_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, float* __restrict__ out, int C, int S, int H, int W, int grid, int ks,
    int ncy, int ncx, BlendCells bc) {
    extern __shared__ float gtile[];
    const int pad = ks / 2, twp = BT + ks - 1, thp = BT + ks - 1;
    const int tid = threadIdx.x;
    const int cj = cell_of_tile(bc.x, ncx, blockIdx.x), ci = cell_of_tile(bc.y, ncy, blockIdx.y);
    const int x0 = bc.x.b[cj] + ((int)blockIdx.x - bc.x.ts[cj]) * BT, y0 = bc.y.b[ci] + ((int)blockIdx.y - bc.y.ts[ci]) * BT;
    const int x_hi = bc.x.b[cj + 1], y_hi = bc.y.b[ci + 1];
    const int plane_i = blockIdx.z, c = plane_i % C;
    if (x0 >= x_hi || y0 >= y_hi) return;
    const float* plane = img + (size_t)plane_i * H * W;
    for (int e = tid; e < thp * twp; e += 256) {
        const int r = e / twp, cc = e - r * twp;
        gtile[e] = plane[(size_t)reflect_idx(y0 - pad + r, H) * W + reflect_idx(x0 - pad + cc, W)];
    }
    __syncthreads();

    const int lx = tid & 31, ly = tid >> 5;
    const int x = x0 + lx, yb = y0 + 4 * ly;
    const bool single = grid == 1;
    const int ci1 = min(ci + 1, grid - 1), cj1 = min(cj + 1, grid - 1);
    const float fx = blend_frac(x, bc.x.node[cj], bc.x.node[cj1], single), gx = __fsub_rn(1.f, fx);
    float fy[4], gy[4];
#pragma unroll
    for (int r = 0; r < 4; ++r) {
        fy[r] = blend_frac(yb + r, bc.y.node[ci], bc.y.node[ci1], single);
        gy[r] = __fsub_rn(1.f, fy[r]);
    }
    const int G = grid * ks;
    for (int s = 0; s < S; ++s) {
        const float* map = psf + (size_t)(s * C + c) * G * G;
        const float* w00 = map + ((size_t)ci * ks) * G + cj * ks;
        const float* w01 = map + ((size_t)ci * ks) * G + cj1 * ks;
        const float* w10 = map + ((size_t)ci1 * ks) * G + cj * ks;
        const float* w11 = map + ((size_t)ci1 * ks) * G + cj1 * ks;
        float acc[4][4];
#pragma unroll
        for (int j = 0; j < 4; ++j)
#pragma unroll
            for (int r = 0; r < 4; ++r) acc[j][r] = 0.f;
        for (int u = 0; u < ks; ++u) {
            const size_t mo = (size_t)(ks - 1 - u) * G + (ks - 1);
            const float* trow = gtile + (4 * ly + u) * twp + lx;
            for (int v = 0; v < ks; ++v) {
                const float m0 = w00[mo - v], m1 = w01[mo - v], m2 = w10[mo - v], m3 = w11[mo - v];
#pragma unroll
                for (int r = 0; r < 4; ++r) {
                    const float xv = trow[r * twp + v];
                    acc[0][r] = __fmaf_rn(m0, xv, acc[0][r]);
                    acc[1][r] = __fmaf_rn(m1, xv, acc[1][r]);
                    acc[2][r] = __fmaf_rn(m2, xv, acc[2][r]);
                    acc[3][r] = __fmaf_rn(m3, xv, acc[3][r]);
                }
            }
        }
        float* o = out + ((size_t)plane_i * S + s) * H * W;
        if (x < x_hi) {
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (yb + r < y_hi) o[(size_t)(yb + r) * W + x] = blend4(acc[0][r], acc[1][r], acc[2][r], acc[3][r], fx, gx, fy[r], gy[r]);
        }
    }
}

}  // namespace aadff

using namespace aadff;

extern "C" int aadff_render_psf_map_blend_stack(const float* img, const float* psf_maps, float* out, const float* node_y, const float* node_x,
                                                int B, int C, int S, int H, int W, int grid, int ks, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && psf_maps && out && node_y && node_x, "render_psf_map_blend: NULL pointer");
    if (int rc = blend_check_shape(B, C, S, H, W, grid, ks)) return rc;
    if (int rc = check_nodes(node_y, grid, "node_y")) return rc;
    if (int rc = check_nodes(node_x, grid, "node_x")) return rc;

    BlendCells bc;
    std::memset(&bc, 0, sizeof(bc));
    const int nty = fill_axis(bc.y, node_y, grid, H), ntx = fill_axis(bc.x, node_x, grid, W);
    const int ncell = grid > 1 ? grid - 1 : 1;
    hipStream_t st = (hipStream_t)stream;
    dim3 g(ntx, nty, B * C);
    switch (ks) {
#define AADFF_CASE(K) case K: hipLaunchKernelGGL((conv_blend_kernel<K>), g, dim3(64 * BNW), 0, st, img, psf_maps, out, C, S, H, W, grid, ncell, ncell, bc); break;
        AADFF_CASE(3) AADFF_CASE(5) AADFF_CASE(7) AADFF_CASE(9) AADFF_CASE(11) AADFF_CASE(13) AADFF_CASE(15) AADFF_CASE(21)
#undef AADFF_CASE
        default: {
            const size_t lds = (size_t)(BT + ks - 1) * (BT + ks - 1) * sizeof(float);
            hipLaunchKernelGGL(conv_blend_generic_kernel, g, dim3(256), lds, st, img, psf_maps, out, C, S, H, W, grid, ks, ncell, ncell, bc);
        }
    }
    AADFF_CHECK_LAUNCH();
    return 0;
}
