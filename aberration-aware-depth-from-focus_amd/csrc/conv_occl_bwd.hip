// Backward of the occlusion-aware layered PSF-map render for gfx950 (MI355X): the gradients of aadff_render_psf_map_stack_occluded to
// the image and the PSF maps, from upstream gradients to the output and to the coverage.  Closed forms and arithmetic contract:
// include/aadff.h (aadff_render_psf_map_stack_occluded_bwd); design and measurements: DESIGN.md 4.21.
//
// Three stages per pass over a run of slices (as many as the workspace holds):
//   1. occl_grad_layers_kernel<KS> / occl_grad_layers_generic_kernel: the forward kernel's tile, staging and {q, a} chains (occl_tile.h).
//      A lane stores q_l, a_l of its outputs to the workspace planes, forms gV, gA, walks the layers back to front over its own stores
//      for R_{l+1} and front to back again for T_l, and leaves alpha_l = dL/dq_l and beta_l = dL/da_l in the planes.  Layers absent from
//      the staged tile get zeros (their alpha, beta meet no texel of that layer in any later sum).
//   2. occl_grad_dimg_kernel<KS>: per 32 x 32 texel tile and layer present among its texels the transposed taps of the patch route
//      (map_dimg_kernel of conv_bwd.hip, mirror folds included) over alpha_l, kept where layer[t] == l: a select, not a sum.
//   3. occl_grad_dmaps_partial_kernel<EB> + occl_grad_dmaps_sum_kernel: the patch route's d_psf (map_dpsf_partial_kernel) with the two
//      products alpha_l * (m_l ? x : 0) + beta_l * (m_l ? 1 : 0) in one accumulator, one partial per tile, a fixed-order second pass.
// Plain fp32 fma, every sum in a fixed order, no atomics, every output written once: bit-reproducible, and independent of the number of
// slices a pass takes (d_img adds each slice's whole contribution to a running sum in ascending s; d_maps has no sum over slices).
#include <algorithm>
#include "occl_tile.h"

namespace aadff {

constexpr int GT = 32;                  // tile edge of stages 2 and 3 (pixels)

__device__ __forceinline__ unsigned layer_mask(int L) { return L >= 32 ? 0xffffffffu : ((1u << L) - 1u); }

// step 1 of the contract: (gV, gA) from V, A and the upstream gradients g (to out) and h (to the coverage)
__device__ __forceinline__ void occl_grad_seed(float V, float A, float g, float h, int normalize, float& gV, float& gA) {
    if (normalize) {
        if (A > 0.f) {
            gV = __fdiv_rn(g, A);
            gA = __fmaf_rn(-gV, __fdiv_rn(V, A), h);       // h - g out / A with out = V / A as the forward rounds it
        } else {
            gV = 0.f;
            gA = h;
        }
    } else {
        gV = g;
        gA = h;
    }
}
// step 2, back to front: R_l = G_l + f_l R_{l+1} from (q_l, a_l); returns the new R
__device__ __forceinline__ float occl_grad_R(float q, float a, float gV, float gA, float Rn) {
    const float G = __fmaf_rn(gV, q, __fmul_rn(gA, a));
    return __fmaf_rn(fmaxf(__fsub_rn(1.f, a), 0.f), Rn, G);
}
// step 2, front to back: alpha_l, beta_l from T_l, a_l, R_{l+1}; T advances as in the forward
__device__ __forceinline__ void occl_grad_ab(float a, float Rn, float gV, float gA, float& T, float& alpha, float& beta) {
    const float f = __fsub_rn(1.f, a);
    const float tg = __fmul_rn(gA, T);
    alpha = __fmul_rn(gV, T);
    beta = f > 0.f ? __fmaf_rn(-T, Rn, tg) : tg;
    T = __fmul_rn(T, fmaxf(f, 0.f));
}

// ------------------------------------------------------------------------------------
// Stage 1, ks in {3,5,7,9,11,13,15,21}.  wa, wb: the workspace planes [B C][Sp][L][H][W]; wave w takes the pass's slices w, w + 4, ...
// ------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(64 * ONW) void occl_grad_layers_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, const unsigned char* __restrict__ layer, const float* __restrict__ g,
    const float* __restrict__ h, float* wa, float* wb, int C, int S, int L, int H, int W, int grid, int normalize, int s0, int Sp,
    OcclPatches pb) {
    using Cfg = OcclCfg<KS>;
    __shared__ __attribute__((aligned(16))) float tile[Cfg::THP * Cfg::P];
    __shared__ __attribute__((aligned(16))) unsigned char ltile[Cfg::THP * Cfg::PB];
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
    const unsigned absent = ~present & layer_mask(L);

    const int q = lane % OQN, k = lane / OQN;
    const int x = x0 + OCX * q, yb = y0 + ORR * k;
    const int G = grid * KS;
    const size_t HW = (size_t)H * W;
    const float* trow = &tile[(ORR * k) * Cfg::P + OCX * q];
    const unsigned char* lrow = &ltile[(ORR * k) * Cfg::PB + OCX * q];
    const size_t pix = (size_t)yb * W + x;
    for (int sl = wave; sl < Sp; sl += ONW) {
        const int s = s0 + sl;
        const size_t w0 = ((size_t)plane_i * Sp + sl) * L * HW + pix;                // + l HW + r W + i
        float V[ORR][OCX], A[ORR][OCX], T[ORR][OCX];
#pragma unroll
        for (int r = 0; r < ORR; ++r)
#pragma unroll
            for (int i = 0; i < OCX; ++i) { V[r][i] = 0.f; A[r][i] = 0.f; T[r][i] = 1.f; }

        for (unsigned rest = present; rest; rest &= rest - 1) {
            const int l = __builtin_ctz(rest);
            const float* w = psf + ((size_t)(s * L + l) * C + c) * G * G + ((size_t)pi * KS) * G + pj * KS;
            f2 acc[ORR][OCX];
            occl_chains<KS>(trow, lrow, w, G, l, acc);
            const size_t o = w0 + (size_t)l * HW;
#pragma unroll
            for (int r = 0; r < ORR; ++r)
#pragma unroll
                for (int i = 0; i < OCX; ++i) {
                    if (yb + r < y_hi && x + i < x_hi) {
                        wa[o + (size_t)r * W + i] = acc[r][i].x;
                        wb[o + (size_t)r * W + i] = acc[r][i].y;
                    }
                    composite(acc[r][i].x, acc[r][i].y, V[r][i], A[r][i], T[r][i]);
                }
        }
        for (unsigned rest = absent; rest; rest &= rest - 1) {
            const size_t o = w0 + (size_t)__builtin_ctz(rest) * HW;
#pragma unroll
            for (int r = 0; r < ORR; ++r)
#pragma unroll
                for (int i = 0; i < OCX; ++i)
                    if (yb + r < y_hi && x + i < x_hi) {
                        wa[o + (size_t)r * W + i] = 0.f;
                        wb[o + (size_t)r * W + i] = 0.f;
                    }
        }

        // step 1: V <- gV, A <- gA
        const size_t g0 = ((size_t)plane_i * S + s) * HW + pix;
#pragma unroll
        for (int r = 0; r < ORR; ++r)
#pragma unroll
            for (int i = 0; i < OCX; ++i) {
                const bool ok = yb + r < y_hi && x + i < x_hi;
                const float gg = (g && ok) ? g[g0 + (size_t)r * W + i] : 0.f;
                const float hh = (h && ok) ? h[g0 + (size_t)r * W + i] : 0.f;
                float gV, gA;
                occl_grad_seed(V[r][i], A[r][i], gg, hh, normalize, gV, gA);
                V[r][i] = gV;
                A[r][i] = gA;
                T[r][i] = 0.f;                                   // R_L = 0
            }
        // back to front over the lane's own stores: the q plane takes R_{l+1}
        for (unsigned rest = present; rest;) {
            const int l = 31 - __builtin_clz(rest);
            rest &= ~(1u << l);
            const size_t o = w0 + (size_t)l * HW;
#pragma unroll
            for (int r = 0; r < ORR; ++r)
#pragma unroll
                for (int i = 0; i < OCX; ++i)
                    if (yb + r < y_hi && x + i < x_hi) {
                        const size_t e = o + (size_t)r * W + i;
                        const float Rn = T[r][i];
                        T[r][i] = occl_grad_R(wa[e], wb[e], V[r][i], A[r][i], Rn);
                        wa[e] = Rn;
                    }
        }
#pragma unroll
        for (int r = 0; r < ORR; ++r)
#pragma unroll
            for (int i = 0; i < OCX; ++i) T[r][i] = 1.f;
        for (unsigned rest = present; rest; rest &= rest - 1) {
            const size_t o = w0 + (size_t)__builtin_ctz(rest) * HW;
#pragma unroll
            for (int r = 0; r < ORR; ++r)
#pragma unroll
                for (int i = 0; i < OCX; ++i)
                    if (yb + r < y_hi && x + i < x_hi) {
                        const size_t e = o + (size_t)r * W + i;
                        float al, be;
                        occl_grad_ab(wb[e], wa[e], V[r][i], A[r][i], T[r][i], al, be);
                        wa[e] = al;
                        wb[e] = be;
                    }
        }
    }
}

// Stage 1, every other odd ks up to AADFF_MAX_KS: the forward's run-time-ks form, 32 x 8 threads with four rows each, the slices one
// after the other.
__global__ __launch_bounds__(256) void occl_grad_layers_generic_kernel(
    const float* __restrict__ img, const float* __restrict__ psf, const unsigned char* __restrict__ layer, const float* __restrict__ g,
    const float* __restrict__ h, float* wa, float* wb, int C, int S, int L, int H, int W, int grid, int ks, int normalize, int s0, int Sp,
    OcclPatches pb) {
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
    const unsigned absent = ~present & layer_mask(L);

    const int lx = tid & 31, ly = tid >> 5;
    const int x = x0 + lx, yb = y0 + 4 * ly;
    const int G = grid * ks;
    const size_t HW = (size_t)H * W;
    const size_t pix = (size_t)yb * W + x;
    if (x >= x_hi) return;                                        // (after the last barrier)
    for (int sl = 0; sl < Sp; ++sl) {
        const int s = s0 + sl;
        const size_t w0 = ((size_t)plane_i * Sp + sl) * L * HW + pix;
        float V[4], A[4], T[4];
#pragma unroll
        for (int r = 0; r < 4; ++r) { V[r] = 0.f; A[r] = 0.f; T[r] = 1.f; }
        for (unsigned rest = present; rest; rest &= rest - 1) {
            const int l = __builtin_ctz(rest);
            const float* w = psf + ((size_t)(s * L + l) * C + c) * G * G + ((size_t)pi * ks) * G + pj * ks;
            float qa[4], aa[4];
            occl_chains_generic(gtile, gl, w, G, ks, twp, lx, ly, l, qa, aa);
            const size_t o = w0 + (size_t)l * HW;
#pragma unroll
            for (int r = 0; r < 4; ++r) {
                if (yb + r < y_hi) {
                    wa[o + (size_t)r * W] = qa[r];
                    wb[o + (size_t)r * W] = aa[r];
                }
                composite(qa[r], aa[r], V[r], A[r], T[r]);
            }
        }
        for (unsigned rest = absent; rest; rest &= rest - 1) {
            const size_t o = w0 + (size_t)__builtin_ctz(rest) * HW;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (yb + r < y_hi) {
                    wa[o + (size_t)r * W] = 0.f;
                    wb[o + (size_t)r * W] = 0.f;
                }
        }
        const size_t g0 = ((size_t)plane_i * S + s) * HW + pix;
#pragma unroll
        for (int r = 0; r < 4; ++r) {
            const bool ok = yb + r < y_hi;
            const float gg = (g && ok) ? g[g0 + (size_t)r * W] : 0.f;
            const float hh = (h && ok) ? h[g0 + (size_t)r * W] : 0.f;
            float gV, gA;
            occl_grad_seed(V[r], A[r], gg, hh, normalize, gV, gA);
            V[r] = gV;
            A[r] = gA;
            T[r] = 0.f;
        }
        for (unsigned rest = present; rest;) {
            const int l = 31 - __builtin_clz(rest);
            rest &= ~(1u << l);
            const size_t o = w0 + (size_t)l * HW;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (yb + r < y_hi) {
                    const size_t e = o + (size_t)r * W;
                    const float Rn = T[r];
                    T[r] = occl_grad_R(wa[e], wb[e], V[r], A[r], Rn);
                    wa[e] = Rn;
                }
        }
#pragma unroll
        for (int r = 0; r < 4; ++r) T[r] = 1.f;
        for (unsigned rest = present; rest; rest &= rest - 1) {
            const size_t o = w0 + (size_t)__builtin_ctz(rest) * HW;
#pragma unroll
            for (int r = 0; r < 4; ++r)
                if (yb + r < y_hi) {
                    const size_t e = o + (size_t)r * W;
                    float al, be;
                    occl_grad_ab(wb[e], wa[e], V[r], A[r], T[r], al, be);
                    wa[e] = al;
                    wb[e] = be;
                }
        }
    }
}

// ------------------------------------------------------------------------------------
// Stage 2: d_img.  In image coordinates (U, V) = padded position minus p, for the layer l of texel (y, x):
//   g_l(U, V) = sum_{a, e < ks} alpha_l[U + a - p][V + e - p] * psf^{s,l}_{patch of that alpha pixel}[a][e]      (terms whose pixel exists)
//   d_img[y][x] = sum_s ( g_l(y, x) + g_l at the mirror images of (y, x) under the reflect padding )
// Workgroup = one 32 x 32 tile of one (b, c) plane; lane = column, 4 rows per thread.  Per slice of the pass and layer present among
// the tile's TEXELS the alpha_l window (tile + p halo, zero outside the image) is staged in LDS and map_dimg_kernel's sums run over it:
// per patch that meets the wave's window, alpha masked to that patch (wave-uniform weights), ks-term column partials -> the layer's
// accumulator; the mirror images from the same tile (border threads).  A texel keeps the accumulator of ITS layer (a hole: 0); the
// slice's value is added to the running sum, which starts at 0 in the first pass and at the stored d_img in a later one.
// ------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(256) void occl_grad_dimg_kernel(const float* __restrict__ psf, const unsigned char* __restrict__ layer,
                                                             const float* __restrict__ wa, float* dimg, int C, int L, int H, int W,
                                                             int grid, int ks_rt, int s0, int Sp, PatchBounds pb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ unsigned present_w[4];
    const int ks = KS > 0 ? KS : ks_rt, p = ks / 2, TP = GT + 2 * p, G = grid * ks;
    float* tile = smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lx = lane & 31, lyg = wave * 2 + (lane >> 5);
    const int bc = blockIdx.z, c = bc % C, b = bc / C;
    const int x0 = blockIdx.x * GT, y0 = blockIdx.y * GT;
    const int x = x0 + lx, yb = y0 + 4 * lyg;
    const size_t HW = (size_t)H * W;

    unsigned lt[4];
    unsigned seen = 0;
#pragma unroll
    for (int k = 0; k < 4; ++k) {
        lt[k] = (x < W && yb + k < H) ? (unsigned)layer[(size_t)b * HW + (size_t)(yb + k) * W + x] : 255u;
        if (lt[k] < (unsigned)L) seen |= 1u << lt[k];
    }
    seen = wave_or(seen);
    if (lane == 0) present_w[wave] = seen;
    __syncthreads();
    const unsigned present = occl_present(present_w);

    // patches that hold a source pixel of this tile / of this wave's rows (uniform: bounds from the kernel arguments, scalar code)
    const int sx_lo = max(x0 - p, 0), sx_hi = min(x0 + GT - 1 + p, W - 1);
    const int wy_lo = max(y0 + 8 * wave - p, 0), wy_hi = min(y0 + 8 * wave + 7 + p, H - 1);
    int pj_lo = 0, pj_hi = 0, pi_lo = 0, pi_hi = 0;
    for (int i = 0; i < grid; ++i) {
        if (pb.wb[i] <= sx_lo) pj_lo = i;
        if (pb.wb[i] <= sx_hi) pj_hi = i;
        if (pb.hb[i] <= wy_lo) pi_lo = i;
        if (pb.hb[i] <= wy_hi) pi_hi = i;
    }
    const bool border = x <= p || x >= W - 1 - p || yb <= p || yb + 3 >= H - 1 - p;

    float total[4] = {0.f, 0.f, 0.f, 0.f};
    if (s0 > 0 && x < W) {
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (yb + k < H) total[k] = dimg[(size_t)bc * HW + (size_t)(yb + k) * W + x];
    }
    for (int sl = 0; sl < Sp; ++sl) {
        float keep[4] = {0.f, 0.f, 0.f, 0.f};
        for (unsigned rest = present; rest; rest &= rest - 1) {
            const int l = __builtin_ctz(rest);
            const float* ap = wa + (((size_t)bc * Sp + sl) * L + l) * HW;
            __syncthreads();
            for (int e = tid; e < TP * TP; e += 256) {
                const int r = e / TP, cc = e - r * TP;
                const int yy = y0 - p + r, xx = x0 - p + cc;
                tile[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? ap[(size_t)yy * W + xx] : 0.f;
            }
            __syncthreads();
            float acc[4] = {0.f, 0.f, 0.f, 0.f};
            if (wy_lo <= wy_hi) {
                for (int pi = pi_lo; pi <= pi_hi; ++pi) {
                    const int ry0 = pb.hb[pi], ry1 = pb.hb[pi + 1];
                    for (int pj = pj_lo; pj <= pj_hi; ++pj) {
                        const int cx0 = pb.wb[pj], cx1 = pb.wb[pj + 1];
                        const float* wp = psf + ((size_t)((size_t)(s0 + sl) * L + l) * C + c) * G * G + ((size_t)pi * ks) * G + pj * ks;
                        // ---- the position itself: source row of output row yb + k and tap row a is yb + k + a - p = tile row 4 lyg + k + a ----
                        const float* trow = tile + (4 * lyg) * TP + lx;
#pragma unroll 1
                        for (int e = 0; e < ks; ++e) {
                            const int xs = x + e - p;
                            const bool cm = xs >= cx0 && xs < cx1;
                            float part[4] = {0.f, 0.f, 0.f, 0.f};
                            auto tap_row = [&](int a) {
                                const float w = wp[(size_t)a * G + e];
#pragma unroll
                                for (int k = 0; k < 4; ++k) {
                                    const int ys = yb - p + a + k;
                                    const float d = (cm && ys >= ry0 && ys < ry1) ? trow[(a + k) * TP + e] : 0.f;
                                    part[k] = fmaf(d, w, part[k]);
                                }
                            };
                            if constexpr (KS > 0) {
#pragma unroll
                                for (int a = 0; a < KS; ++a) tap_row(a);
                            } else {
                                for (int a = 0; a < ks; ++a) tap_row(a);
                            }
#pragma unroll
                            for (int k = 0; k < 4; ++k) acc[k] += part[k];
                        }
                        // ---- its mirror images under the reflect padding: sources inside the direct window, the same tile (conv_bwd.hip) ----
                        if (border) {
#pragma unroll 1
                            for (int k = 0; k < 4; ++k) {
                                const int y = yb + k;
                                if (y >= H || x >= W) continue;
                                float part = 0.f;
                                for (int vu = 0; vu < 3; ++vu) {
                                    const int Uv = vu == 0 ? y : (vu == 1 ? -y : 2 * (H - 1) - y);
                                    if ((vu == 1 && !(y >= 1 && y <= p)) || (vu == 2 && !(y <= H - 2 && y >= H - 1 - p))) continue;
                                    const int r_lo = max(max(Uv - p, 0), ry0), r_hi = min(min(Uv + p, H - 1), ry1 - 1);
                                    for (int vv = 0; vv < 3; ++vv) {
                                        const int Vv = vv == 0 ? x : (vv == 1 ? -x : 2 * (W - 1) - x);
                                        if ((vv == 1 && !(x >= 1 && x <= p)) || (vv == 2 && !(x <= W - 2 && x >= W - 1 - p))) continue;
                                        if (vu == 0 && vv == 0) continue;
                                        const int c_lo = max(max(Vv - p, 0), cx0), c_hi = min(min(Vv + p, W - 1), cx1 - 1);
                                        for (int r = r_lo; r <= r_hi; ++r)
                                            for (int cc = c_lo; cc <= c_hi; ++cc)
                                                part = fmaf(tile[(r - (y0 - p)) * TP + cc - (x0 - p)], wp[(size_t)(p + r - Uv) * G + p + cc - Vv], part);
                                    }
                                }
                                acc[k] += part;
                            }
                        }
                    }
                }
            }
#pragma unroll
            for (int k = 0; k < 4; ++k) keep[k] = lt[k] == (unsigned)l ? acc[k] : keep[k];       // a select by the texel's layer
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) total[k] += keep[k];
    }
    if (x < W) {
        float* o = dimg + (size_t)bc * HW + x;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (yb + k < H) o[(size_t)(yb + k) * W] = total[k];
    }
}

// ------------------------------------------------------------------------------------
// Stage 3: d_maps[s L + l][c][i ks + a][j ks + e] = sum_b sum_{(y, x) in patch (i, j)}
//              alpha_l[y][x] * (m_l(t) ? img[t] : 0) + beta_l[y][x] * (m_l(t) ? 1 : 0),     t = (refl(y + p - a), refl(x + p - e)).
// First pass (map_dpsf_partial_kernel's layout): workgroup = one 32 x 32 tile of one patch and (b, c) plane.  Per layer present in the
// tile's reflect-padded window the masked image window and the mask window are staged once for the pass's slices, the alpha and beta
// tiles (zero outside the patch) per slice.  Wave w takes the tap rows a = w, w + 4, ...; a lane owns 4 x 4 pixels and EB taps of the
// row at a time; per pixel and tap the two fma go into the one accumulator, alpha first.  Sums: 32 fma per lane -> wave tree -> one
// partial per (tile, b, slice, layer).  A layer absent from the window gets a zero partial.  EB = ks for the tuned size, 1 for any ks.
// ------------------------------------------------------------------------------------
template <int EB>
__global__ __launch_bounds__(256) void occl_grad_dmaps_partial_kernel(const float* __restrict__ img, const unsigned char* __restrict__ layer,
                                                                      const float* __restrict__ wa, const float* __restrict__ wb,
                                                                      float* __restrict__ part, int C, int L, int H, int W, int grid, int ks,
                                                                      int Sp, int ntx, int nty, PatchBounds pb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    __shared__ unsigned present_w[4];
    const int p = ks / 2, TP = GT + 2 * p, kk = ks * ks;
    float* tda = smem;                      // [32][32] alpha
    float* tdb = smem + GT * GT;            // [32][32] beta
    float* txm = smem + 2 * GT * GT;        // [TP][TP] m ? x : 0
    float* tm = txm + TP * TP;              // [TP][TP] m ? 1 : 0
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pj = blockIdx.x / ntx, tx = blockIdx.x - pj * ntx;
    const int pi = blockIdx.y / nty, ty = blockIdx.y - pi * nty;
    const int bc = blockIdx.z, b = bc / C, c = bc - b * C;
    const int x_hi = pb.wb[pj + 1], y_hi = pb.hb[pi + 1];
    const int x0 = pb.wb[pj] + tx * GT, y0 = pb.hb[pi] + ty * GT;
    if (x0 >= x_hi || y0 >= y_hi) return;
    const size_t HW = (size_t)H * W;
    const float* plane = img + (size_t)bc * HW;
    const unsigned char* lplane = layer + (size_t)b * HW;

    unsigned seen = 0;
    for (int e = tid; e < TP * TP; e += 256) {
        const int r = e / TP, cc = e - r * TP;
        const unsigned lv = lplane[(size_t)reflect_idx(y0 - p + r, H) * W + reflect_idx(x0 - p + cc, W)];
        if (lv < (unsigned)L) seen |= 1u << lv;
    }
    seen = wave_or(seen);
    if (lane == 0) present_w[wave] = seen;
    __syncthreads();
    const unsigned present = occl_present(present_w);

    const int lxg = lane & 7, lyr = lane >> 3;
    const int nblk = (ks + EB - 1) / EB, units = ks * nblk;
    const size_t slab = (size_t)b * ntx * nty + (size_t)ty * ntx + tx;
    for (int l = 0; l < L; ++l) {
        if (!((present >> l) & 1u)) {
            for (int sl = 0; sl < Sp; ++sl) {
                float* po = part + (((((size_t)slab * Sp + sl) * L + l) * C + c) * grid * grid + (size_t)pi * grid + pj) * kk;
                for (int e = tid; e < kk; e += 256) po[e] = 0.f;
            }
            continue;
        }
        __syncthreads();
        for (int e = tid; e < TP * TP; e += 256) {
            const int r = e / TP, cc = e - r * TP;
            const size_t src = (size_t)reflect_idx(y0 - p + r, H) * W + reflect_idx(x0 - p + cc, W);
            const bool on = (unsigned)lplane[src] == (unsigned)l;
            txm[e] = on ? plane[src] : 0.f;                        // a select: a NaN of another layer's texel or of a hole stays out
            tm[e] = on ? 1.f : 0.f;
        }
        for (int sl = 0; sl < Sp; ++sl) {
            const size_t o = (((size_t)bc * Sp + sl) * L + l) * HW;
            __syncthreads();
            for (int e = tid; e < GT * GT; e += 256) {
                const int y = y0 + (e >> 5), xx = x0 + (e & 31);
                const bool in = y < y_hi && xx < x_hi;
                tda[e] = in ? wa[o + (size_t)y * W + xx] : 0.f;
                tdb[e] = in ? wb[o + (size_t)y * W + xx] : 0.f;
            }
            __syncthreads();
            float* po = part + (((((size_t)slab * Sp + sl) * L + l) * C + c) * grid * grid + (size_t)pi * grid + pj) * kk;
            for (int u = wave; u < units; u += 4) {
                const int a = u / nblk, e0 = (u - a * nblk) * EB;
                float acc[EB];
#pragma unroll
                for (int m = 0; m < EB; ++m) acc[m] = 0.f;
#pragma unroll
                for (int j = 0; j < 4; ++j) {
                    const int row = lyr + 8 * j;
                    const float4 a4 = *reinterpret_cast<const float4*>(tda + row * GT + 4 * lxg);
                    const float4 b4 = *reinterpret_cast<const float4*>(tdb + row * GT + 4 * lxg);
                    const float da[4] = {a4.x, a4.y, a4.z, a4.w};
                    const float db[4] = {b4.x, b4.y, b4.z, b4.w};
                    // pixel column 4 lxg + k and tap e0 + m read window column 4 lxg + k + 2p - e0 - m
                    const int off = (row + 2 * p - a) * TP + 4 * lxg + 2 * p - e0 - (EB - 1);
                    float v[EB + 3], vm[EB + 3];
#pragma unroll
                    for (int q = 0; q < EB + 3; ++q) { v[q] = txm[off + q]; vm[q] = tm[off + q]; }
#pragma unroll
                    for (int k = 0; k < 4; ++k)
#pragma unroll
                        for (int m = 0; m < EB; ++m) {
                            acc[m] = fmaf(da[k], v[k + EB - 1 - m], acc[m]);
                            acc[m] = fmaf(db[k], vm[k + EB - 1 - m], acc[m]);
                        }
                }
                float mine = 0.f;
#pragma unroll
                for (int m = 0; m < EB; ++m) {
                    const float t = wave_sum(acc[m]);
                    if (lane == m) mine = t;
                }
                if (lane < EB && e0 + lane < ks) po[a * ks + e0 + lane] = mine;
            }
        }
    }
}

// second pass: one thread per element of the pass's maps (n = slice-layer pair of the pass); its partials in the order b, tile row,
// tile column (tile rows summed first), every level started at 0
__global__ __launch_bounds__(256) void occl_grad_dmaps_sum_kernel(const float* __restrict__ part, float* __restrict__ dmaps, int B, int C, int N,
                                                                  int grid, int ks, int ntx, int nty, PatchBounds pb) {
    const int G = grid * ks, kk = ks * ks;
    const size_t n = (size_t)N * C * G * G;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int col = (int)(idx % G), row = (int)((idx / G) % G);
    const size_t sc = idx / ((size_t)G * G);
    const int pi = row / ks, a = row - pi * ks, pj = col / ks, e = col - pj * ks;
    const int ph = pb.hb[pi + 1] - pb.hb[pi], pw = pb.wb[pj + 1] - pb.wb[pj];
    const int tyn = (ph + GT - 1) / GT, txn = (pw + GT - 1) / GT;
    const size_t per_slab = (size_t)N * C * grid * grid * kk;
    const float* src = part + (sc * grid * grid + (size_t)pi * grid + pj) * kk + a * ks + e;
    float sum = 0.f;
    for (int b = 0; b < B; ++b) {
        float sb = 0.f;
        for (int ty = 0; ty < tyn; ++ty) {
            const float* q = src + ((size_t)b * ntx * nty + (size_t)ty * ntx) * per_slab;
            float sr = 0.f;
#pragma unroll 4
            for (int tx = 0; tx < txn; ++tx) sr += q[(size_t)tx * per_slab];
            sb += sr;
        }
        sum += sb;
    }
    dmaps[idx] = sum;
}

struct OcclBwdPlan {
    PatchBounds pb;
    int ntx, nty;
    size_t ab_floats, part_floats;      // per slice: one of the two planes; the partial slabs
};

static void plan_occl_bwd(OcclBwdPlan& pl, int B, int C, int L, int H, int W, int grid, int ks) {
    std::memset(&pl.pb, 0, sizeof(pl.pb));
    fill_bounds(pl.pb.hb, grid, H);
    fill_bounds(pl.pb.wb, grid, W);
    int mh = 0, mw = 0;
    for (int i = 0; i < grid; ++i) {
        mh = std::max(mh, pl.pb.hb[i + 1] - pl.pb.hb[i]);
        mw = std::max(mw, pl.pb.wb[i + 1] - pl.pb.wb[i]);
    }
    pl.ntx = (mw + GT - 1) / GT;
    pl.nty = (mh + GT - 1) / GT;
    pl.ab_floats = (size_t)B * C * L * H * W;
    pl.part_floats = (size_t)B * pl.ntx * pl.nty * L * C * grid * grid * ks * ks;
}

static size_t occl_bwd_bytes_per_slice(const OcclBwdPlan& pl, bool need_maps) {
    return (2 * pl.ab_floats + (need_maps ? pl.part_floats : 0)) * sizeof(float);
}

}  // namespace aadff

using namespace aadff;

extern "C" {

size_t aadff_render_psf_map_stack_occluded_bwd_workspace(int B, int C, int S, int L, int H, int W, int grid, int ks, int need_maps) {
    if (occl_check_shape("render_psf_map_stack_occluded_bwd_workspace", B, C, S, L, H, W, grid, ks)) return 0;
    OcclBwdPlan pl;
    plan_occl_bwd(pl, B, C, L, H, W, grid, ks);
    return (size_t)S * occl_bwd_bytes_per_slice(pl, need_maps != 0);
}

int aadff_render_psf_map_stack_occluded_bwd(const float* img, const float* psf_maps, const unsigned char* layer, const float* d_out_or_null,
                                            const float* d_cov_or_null, float* d_img_or_null, float* d_maps_or_null, void* workspace,
                                            size_t workspace_bytes, int B, int C, int S, int L, int H, int W, int grid, int ks, int normalize,
                                            aadff_stream_t stream) {
    static const char* who = "render_psf_map_stack_occluded_bwd";
    AADFF_CHECK_ARG(img && psf_maps && layer, "%s: NULL pointer (img, psf_maps, layer)", who);
    AADFF_CHECK_ARG(d_out_or_null || d_cov_or_null, "%s: d_out and d_cov are both NULL", who);
    AADFF_CHECK_ARG(d_img_or_null || d_maps_or_null, "%s: d_img and d_maps are both NULL", who);
    if (int rc = occl_check_shape(who, B, C, S, L, H, W, grid, ks)) return rc;
    OcclBwdPlan pl;
    plan_occl_bwd(pl, B, C, L, H, W, grid, ks);
    const size_t per_slice = occl_bwd_bytes_per_slice(pl, d_maps_or_null != nullptr);
    AADFF_CHECK_ARG(workspace && workspace_bytes >= per_slice, "%s: workspace of %zu bytes is too small, one slice needs %zu", who,
                    workspace ? workspace_bytes : (size_t)0, per_slice);
    const int Smax = (int)std::min<size_t>((size_t)S, workspace_bytes / per_slice);      // slices per pass

    OcclPatches op;
    std::memset(&op, 0, sizeof(op));
    const int nty = fill_occl_axis(op.y, grid, H), ntx = fill_occl_axis(op.x, grid, W);
    hipStream_t st = (hipStream_t)stream;
    const int TP = GT + ks - 1, G = grid * ks;
    for (int s0 = 0; s0 < S; s0 += Smax) {
        const int Sp = std::min(Smax, S - s0);
        float* wa = static_cast<float*>(workspace);
        float* wb = wa + pl.ab_floats * Sp;
        float* part = wb + pl.ab_floats * Sp;
        {
            dim3 g(ntx, nty, B * C);
            switch (ks) {
#define AADFF_CASE(K) case K: hipLaunchKernelGGL((occl_grad_layers_kernel<K>), g, dim3(64 * ONW), 0, st, img, psf_maps, layer, d_out_or_null, d_cov_or_null, wa, wb, C, S, L, H, W, grid, normalize, s0, Sp, op); break;
                AADFF_CASE(3) AADFF_CASE(5) AADFF_CASE(7) AADFF_CASE(9) AADFF_CASE(11) AADFF_CASE(13) AADFF_CASE(15) AADFF_CASE(21)
#undef AADFF_CASE
                default:
                    hipLaunchKernelGGL(occl_grad_layers_generic_kernel, g, dim3(256), occl_generic_lds(ks), st, img, psf_maps, layer, d_out_or_null,
                                       d_cov_or_null, wa, wb, C, S, L, H, W, grid, ks, normalize, s0, Sp, op);
            }
            AADFF_CHECK_LAUNCH();
        }
        if (d_img_or_null) {
            dim3 g((W + GT - 1) / GT, (H + GT - 1) / GT, B * C);
            const size_t lds = (size_t)TP * TP * sizeof(float);
            if (ks == 11) hipLaunchKernelGGL(occl_grad_dimg_kernel<11>, g, dim3(256), lds, st, psf_maps, layer, wa, d_img_or_null, C, L, H, W, grid, ks, s0, Sp, pl.pb);
            else hipLaunchKernelGGL(occl_grad_dimg_kernel<0>, g, dim3(256), lds, st, psf_maps, layer, wa, d_img_or_null, C, L, H, W, grid, ks, s0, Sp, pl.pb);
            AADFF_CHECK_LAUNCH();
        }
        if (d_maps_or_null) {
            dim3 g(pl.ntx * grid, pl.nty * grid, B * C);
            const size_t lds = (size_t)(2 * GT * GT + 2 * TP * TP) * sizeof(float);
            if (ks == 11) hipLaunchKernelGGL(occl_grad_dmaps_partial_kernel<11>, g, dim3(256), lds, st, img, layer, wa, wb, part, C, L, H, W, grid, ks, Sp, pl.ntx, pl.nty, pl.pb);
            else hipLaunchKernelGGL(occl_grad_dmaps_partial_kernel<1>, g, dim3(256), lds, st, img, layer, wa, wb, part, C, L, H, W, grid, ks, Sp, pl.ntx, pl.nty, pl.pb);
            AADFF_CHECK_LAUNCH();
            const size_t n = (size_t)Sp * L * C * G * G;
            hipLaunchKernelGGL(occl_grad_dmaps_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part,
                               d_maps_or_null + (size_t)s0 * L * C * G * G, B, C, Sp * L, grid, ks, pl.ntx, pl.nty, pl.pb);
            AADFF_CHECK_LAUNCH();
        }
    }
    return 0;
}

}  // extern "C"
