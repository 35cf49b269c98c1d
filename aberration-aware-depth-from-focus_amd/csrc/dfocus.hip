// Depth from a focal stack, the classical estimator: per slice the window-summed modified Laplacian of the gray image,
// the first argmax over the slices and a three-point peak fit, in ONE launch and one pass over stack [N,C,S,H,W].
//
//   depth_from_stack_kernel<R, C>   a workgroup of 256 threads owns a 32 x 64 output tile, a thread 2 x 4 of its pixels (rows ty and
//                                   ty + 16, four consecutive columns).  Per slice: gray of the tile plus a halo of R + 1 goes to LDS
//                                   (the thread's own pixels as 16-byte loads that stay in registers for `aif`, the halo ring as clamped
//                                   scalar loads; both are issued one slice ahead), ML of the tile plus R is formed from it, summed along
//                                   the rows and then along the columns, and the running state of every pixel (best F, its index, the F
//                                   before it, the F after it, the last F, the C centre values of the best slice) is updated in registers.
// No atomics, no workspace, no second read of the stack except the halos: the outputs are bit-identical from run to run and do not
// depend on which optional outputs are written or on the access width.  ML is exactly rounded operation by operation (fp contract
// off), the window sum adds non-negative terms only (rows left to right, then columns top to bottom).
#include "common.h"

namespace aadff {
namespace dfs {

constexpr int TW = 64, TH = 32, NT = 256;
constexpr int GX = TW / 4, GY = NT / GX, PY = TH / GY;       // 16 column groups of four pixels, 16 thread rows, 2 rows per thread
constexpr int MAXC = 4;

template <int R>
struct Geo {
    static constexpr int P = R + 1;                           // gray halo
    static constexpr int GW = TW + 2 * P, GH = TH + 2 * P;    // staged gray
    static constexpr int MW = TW + 2 * R, MH = TH + 2 * R;    // ML region
    static constexpr int MWP = (MW + 3) & ~3;                 // its row stride: 16-byte rows for the row sums
    static constexpr int NBAND = 2 * P * GW;                  // halo ring: the rows above and below, then the columns beside the tile
    static constexpr int NHALO = NBAND + 2 * P * TH;
    static constexpr int HPT = (NHALO + NT - 1) / NT;         // halo elements per thread
};

struct Args {
    const float* stack;
    const float* coords;
    float* depth;
    int* index;
    float* peak;
    float* aif;
    float* volume;
    int S, H, W, tiles_x, tiles_y;
    unsigned xcd_q, xcd_r;
    int interp, vec;
    float eps, inv_c;
};

// Offset of the fitted peak from u0 (specification step 5): the vertex of the parabola through (u0 - hm, fm), (u0, f0), (u0 + hp, fp),
// or through the logarithms written as log1p of non-negative ratios.  a, b >= 0, so den adds same-sign terms.
__device__ __forceinline__ float fit_offset(float f0, float fm, float fp, float u0, float um, float up, int interp, float eps) {
#pragma clang fp contract(off)
    const float hm = u0 - um, hp = up - u0;
    float a, b;
    if (interp == AADFF_DFOCUS_GAUSSIAN) {
        a = log1pf((f0 - fm) / (fm + eps));
        b = log1pf((f0 - fp) / (fp + eps));
    } else {
        a = f0 - fm;
        b = f0 - fp;
    }
    const float den = 2.f * (b * hm + a * hp);
    const float x = den == 0.f ? 0.f : (a * hp * hp - b * hm * hm) / den;
    return fminf(fmaxf(x, fminf(-hm, hp)), fmaxf(-hm, hp));
}

template <int R, int C>
__global__ __launch_bounds__(NT) void depth_from_stack_kernel(Args A) {
#pragma clang fp contract(off)
    using G = Geo<R>;
    constexpr int P = G::P, GW = G::GW, MW = G::MW, MH = G::MH, MWP = G::MWP, HPT = G::HPT;
    __shared__ __align__(16) float s_gray[G::GH * GW];
    __shared__ __align__(16) float s_ml[MH * MWP];
    __shared__ __align__(16) float s_rs[MH * TW];

    const int t = threadIdx.x;
    const int S = A.S, H = A.H, W = A.W;
    unsigned b = xcd_remap(blockIdx.x, A.xcd_q, A.xcd_r);     // neighbouring tiles share halos: keep them on one L2
    const int x0 = (int)(b % (unsigned)A.tiles_x) * TW;
    b /= (unsigned)A.tiles_x;
    const int y0 = (int)(b % (unsigned)A.tiles_y) * TH;
    const int n = (int)(b / (unsigned)A.tiles_y);
    const size_t HW = (size_t)H * W;
    const size_t chan = (size_t)S * HW;                       // stack[n][c][s]: channel stride
    const float* base = A.stack + (size_t)n * C * chan;

    const int ty = t / GX, tx4 = (t % GX) * 4;
    const int px = x0 + tx4;
    // the thread's own pixels: rows py[q], columns px .. px + 3
    int py[PY], ioff[PY][4];
    bool in4[PY];                                             // the four pixels are inside the image and 16-byte loadable
#pragma unroll
    for (int q = 0; q < PY; ++q) {
        py[q] = y0 + ty + q * GY;
        in4[q] = A.vec && py[q] < H && px < W;                // W % 4 == 0: a group of four is inside or outside as a whole
        const int yy = min(py[q], H - 1);
#pragma unroll
        for (int j = 0; j < 4; ++j) ioff[q][j] = yy * W + min(px + j, W - 1);
    }
    // the thread's share of the halo ring: clamped pixel offset and LDS slot (-1: none)
    int hoff[HPT], hlds[HPT];
#pragma unroll
    for (int h = 0; h < HPT; ++h) {
        const int i = t + h * NT;
        int gy, gx;
        if (i < G::NBAND) {
            const int row = i / GW;
            gx = i - row * GW;
            gy = row < P ? row : TH + row;
        } else {
            const int j = i - G::NBAND, row = j / (2 * P), k = j - row * (2 * P);
            gy = P + row;
            gx = k < P ? k : TW + k;
        }
        const bool valid = i < G::NHALO;
        const int yy = min(max(y0 - P + gy, 0), H - 1), xx = min(max(x0 - P + gx, 0), W - 1);
        hoff[h] = valid ? yy * W + xx : 0;
        hlds[h] = valid ? gy * GW + gx : -1;
    }

    float nc[PY][C][4], nh[HPT][C];                           // the slice in flight: own pixels, halo elements
    auto load_slice = [&](int s) {
        const float* sl = base + (size_t)s * HW;
#pragma unroll
        for (int q = 0; q < PY; ++q) {
#pragma unroll
            for (int c = 0; c < C; ++c) {
                const float* pl = sl + c * chan;
                if (in4[q]) {
                    const float4 v = *reinterpret_cast<const float4*>(pl + ioff[q][0]);
                    nc[q][c][0] = v.x, nc[q][c][1] = v.y, nc[q][c][2] = v.z, nc[q][c][3] = v.w;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j) nc[q][c][j] = pl[ioff[q][j]];
                }
            }
        }
#pragma unroll
        for (int h = 0; h < HPT; ++h) {
#pragma unroll
            for (int c = 0; c < C; ++c) nh[h][c] = hlds[h] >= 0 ? sl[c * chan + hoff[h]] : 0.f;
        }
    };
    auto gray_of = [&](const float* v, int stride) {          // ((c0 + c1) + c2 ...) * float32(1 / C)
        float g = v[0];
#pragma unroll
        for (int c = 1; c < C; ++c) g += v[c * stride];
        return g * A.inv_c;
    };

    float best[PY][4], fprev[PY][4], fnext[PY][4], last[PY][4], cen[PY][C][4];
    int bidx[PY][4];
#pragma unroll
    for (int q = 0; q < PY; ++q) {
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            best[q][j] = fprev[q][j] = fnext[q][j] = last[q][j] = 0.f;
            bidx[q][j] = 0;
#pragma unroll
            for (int c = 0; c < C; ++c) cen[q][c][j] = 0.f;
        }
    }

    load_slice(0);
#pragma unroll 1
    for (int s = 0; s < S; ++s) {
        float cc[PY][C][4];                                   // this slice's centre values, kept for aif
        // gray of the tile and its halo -> LDS (the readers of the previous slice's gray passed the barrier after ML)
#pragma unroll
        for (int q = 0; q < PY; ++q) {
            float g[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
#pragma unroll
                for (int c = 0; c < C; ++c) cc[q][c][j] = nc[q][c][j];
                g[j] = gray_of(&nc[q][0][j], 4);
            }
            float* dst = s_gray + (P + ty + q * GY) * GW + P + tx4;
#pragma unroll
            for (int j = 0; j < 4; ++j) dst[j] = g[j];
        }
#pragma unroll
        for (int h = 0; h < HPT; ++h)
            if (hlds[h] >= 0) s_gray[hlds[h]] = gray_of(&nh[h][0], 1);
        __syncthreads();
        if (s + 1 < S) load_slice(s + 1);                     // in flight during the arithmetic of slice s

        // modified Laplacian of the tile plus R, at the clamped position: replicate padding of the ML map
        for (int i = t; i < MH * MW; i += NT) {
            const int my = i / MW, mx = i - my * MW;
            const int cy = min(max(y0 - R + my, 0), H - 1), cx = min(max(x0 - R + mx, 0), W - 1);
            const float* gp = s_gray + (cy - (y0 - P)) * GW + (cx - (x0 - P));
            const float g2 = 2.f * gp[0];
            s_ml[my * MWP + mx] = fabsf((g2 - gp[-1]) - gp[1]) + fabsf((g2 - gp[-GW]) - gp[GW]);
        }
        __syncthreads();
        // row sums: four neighbouring windows per item share their 4 + 2R values
        for (int i = t; i < MH * GX; i += NT) {
            const int my = i / GX, g4 = (i - my * GX) * 4;
            const float* mp = s_ml + my * MWP + g4;
            float v[4 + 2 * R];
#pragma unroll
            for (int k = 0; k < 4 + 2 * R; ++k) v[k] = mp[k];
            float o[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                o[j] = v[j];
#pragma unroll
                for (int k = 1; k <= 2 * R; ++k) o[j] += v[j + k];
            }
            *reinterpret_cast<float4*>(s_rs + my * TW + g4) = make_float4(o[0], o[1], o[2], o[3]);
        }
        __syncthreads();
        // column sums -> F of the thread's pixels, then the running state
#pragma unroll
        for (int q = 0; q < PY; ++q) {
            const float* rp = s_rs + (ty + q * GY) * TW + tx4;
            float4 f = *reinterpret_cast<const float4*>(rp);
#pragma unroll
            for (int k = 1; k <= 2 * R; ++k) {
                const float4 w = *reinterpret_cast<const float4*>(rp + k * TW);
                f.x += w.x, f.y += w.y, f.z += w.z, f.w += w.w;
            }
            const float F[4] = {f.x, f.y, f.z, f.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (s == 0) {
                    best[q][j] = F[j];
                } else if (F[j] > best[q][j]) {               // strict: the first of equal maxima stays
                    fprev[q][j] = last[q][j];
                    best[q][j] = F[j];
                    bidx[q][j] = s;
                } else if (bidx[q][j] == s - 1) {
                    fnext[q][j] = F[j];
                }
                if (bidx[q][j] == s) {
#pragma unroll
                    for (int c = 0; c < C; ++c) cen[q][c][j] = cc[q][c][j];
                }
                last[q][j] = F[j];
            }
            if (A.volume && py[q] < H) {
                float* vp = A.volume + ((size_t)n * S + s) * HW + (size_t)py[q] * W + px;
                if (in4[q]) {
                    *reinterpret_cast<float4*>(vp) = f;
                } else {
#pragma unroll
                    for (int j = 0; j < 4; ++j)
                        if (px + j < W) vp[j] = F[j];
                }
            }
        }
    }

    const float* u = A.coords + (size_t)n * S;
#pragma unroll
    for (int q = 0; q < PY; ++q) {
        if (py[q] >= H) continue;
        float d[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int k = bidx[q][j];
            const float u0 = u[k];
            float x = 0.f;
            if (A.interp != AADFF_DFOCUS_NONE && k > 0 && k < S - 1)
                x = fit_offset(best[q][j], fprev[q][j], fnext[q][j], u0, u[k - 1], u[k + 1], A.interp, A.eps);
            d[j] = u0 + x;
        }
        const size_t o = (size_t)n * HW + (size_t)py[q] * W + px;
        if (in4[q]) {
            *reinterpret_cast<float4*>(A.depth + o) = make_float4(d[0], d[1], d[2], d[3]);
            *reinterpret_cast<int4*>(A.index + o) = make_int4(bidx[q][0], bidx[q][1], bidx[q][2], bidx[q][3]);
            *reinterpret_cast<float4*>(A.peak + o) = make_float4(best[q][0], best[q][1], best[q][2], best[q][3]);
            if (A.aif) {
#pragma unroll
                for (int c = 0; c < C; ++c)
                    *reinterpret_cast<float4*>(A.aif + ((size_t)n * C + c) * HW + (size_t)py[q] * W + px) =
                        make_float4(cen[q][c][0], cen[q][c][1], cen[q][c][2], cen[q][c][3]);
            }
        } else {
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                if (px + j >= W) continue;
                A.depth[o + j] = d[j];
                A.index[o + j] = bidx[q][j];
                A.peak[o + j] = best[q][j];
                if (A.aif) {
#pragma unroll
                    for (int c = 0; c < C; ++c) A.aif[((size_t)n * C + c) * HW + (size_t)py[q] * W + px + j] = cen[q][c][j];
                }
            }
        }
    }
}

template <int R>
static void launch_r(int C, dim3 grid, hipStream_t st, const Args& A) {
    switch (C) {
        case 1: hipLaunchKernelGGL((depth_from_stack_kernel<R, 1>), grid, dim3(NT), 0, st, A); break;
        case 2: hipLaunchKernelGGL((depth_from_stack_kernel<R, 2>), grid, dim3(NT), 0, st, A); break;
        case 3: hipLaunchKernelGGL((depth_from_stack_kernel<R, 3>), grid, dim3(NT), 0, st, A); break;
        default: hipLaunchKernelGGL((depth_from_stack_kernel<R, 4>), grid, dim3(NT), 0, st, A); break;
    }
}

}  // namespace dfs
}  // namespace aadff

using namespace aadff;

extern "C" int aadff_depth_from_stack(const float* stack, const float* coords, float* depth, int* index, float* peak, float* aif_or_null,
                                      float* volume_or_null, int N, int C, int S, int H, int W, int window, int interp, float eps,
                                      aadff_stream_t stream) {
    AADFF_CHECK_ARG(stack, "depth_from_stack: stack is NULL");
    AADFF_CHECK_ARG(coords, "depth_from_stack: coords is NULL");
    AADFF_CHECK_ARG(depth, "depth_from_stack: depth is NULL");
    AADFF_CHECK_ARG(index, "depth_from_stack: index is NULL");
    AADFF_CHECK_ARG(peak, "depth_from_stack: peak is NULL");
    AADFF_CHECK_ARG(C >= 1 && C <= dfs::MAXC, "depth_from_stack: C = %d is outside 1..%d", C, dfs::MAXC);
    AADFF_CHECK_ARG(S >= 1, "depth_from_stack: S = %d, at least one slice is needed", S);
    AADFF_CHECK_ARG(N > 0, "depth_from_stack: N = %d is not positive", N);
    AADFF_CHECK_ARG(H > 0, "depth_from_stack: H = %d is not positive", H);
    AADFF_CHECK_ARG(W > 0, "depth_from_stack: W = %d is not positive", W);
    AADFF_CHECK_ARG(window >= 1 && window <= 9 && (window & 1), "depth_from_stack: window = %d is not one of 1, 3, 5, 7, 9", window);
    AADFF_CHECK_ARG(interp == AADFF_DFOCUS_NONE || interp == AADFF_DFOCUS_PARABOLA || interp == AADFF_DFOCUS_GAUSSIAN,
                    "depth_from_stack: interp = %d is unknown (0 none, 1 parabola, 2 gaussian)", interp);
    AADFF_CHECK_ARG(eps > 0.f, "depth_from_stack: eps = %g is not positive", (double)eps);
    const long tiles_x = (W + dfs::TW - 1) / dfs::TW, tiles_y = (H + dfs::TH - 1) / dfs::TH;
    const long blocks = tiles_x * tiles_y * N;
    AADFF_CHECK_ARG((long)H * W < (1L << 31) - 8 && blocks < (1L << 31), "depth_from_stack: N = %d, H = %d, W = %d are too large for one launch", N, H, W);

    dfs::Args A;
    A.stack = stack, A.coords = coords, A.depth = depth, A.index = index, A.peak = peak, A.aif = aif_or_null, A.volume = volume_or_null;
    A.S = S, A.H = H, A.W = W, A.tiles_x = (int)tiles_x, A.tiles_y = (int)tiles_y;
    A.xcd_q = (unsigned)(blocks / 8), A.xcd_r = (unsigned)(blocks % 8);
    A.interp = interp, A.eps = eps, A.inv_c = (float)(1.0 / C);
    const uintptr_t bits = (uintptr_t)stack | (uintptr_t)depth | (uintptr_t)index | (uintptr_t)peak | (uintptr_t)aif_or_null | (uintptr_t)volume_or_null;
    A.vec = (W % 4 == 0) && (bits % 16 == 0);                 // every plane then starts on 16 bytes: H * W is a multiple of four
    const dim3 grid((unsigned)blocks);
    hipStream_t st = (hipStream_t)stream;
    switch (window / 2) {
        case 0: dfs::launch_r<0>(C, grid, st, A); break;
        case 1: dfs::launch_r<1>(C, grid, st, A); break;
        case 2: dfs::launch_r<2>(C, grid, st, A); break;
        case 3: dfs::launch_r<3>(C, grid, st, A); break;
        default: dfs::launch_r<4>(C, grid, st, A); break;
    }
    AADFF_CHECK_LAUNCH();
    return 0;
}
