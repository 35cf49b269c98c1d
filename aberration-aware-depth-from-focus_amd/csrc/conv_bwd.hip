// Backward of the patch-wise PSF convolution for gfx950 (MI355X): the gradients torch.autograd derives for the reference's
// deeplens/render_psf.py:12-73, as closed forms in plain fp32 (the per-pixel gather's backward: gather.hip).
// See include/aadff.h for the entry points and DESIGN.md 4.7 for the design and the measurements.
//
// Every sum has a fixed order (no float atomics): results are bitwise reproducible from run to run.  Sums across workgroups
// (d_psf of the patch convolution) go through per-workgroup partial slabs and a second pass that adds them in a fixed order.
#include <algorithm>
#include "common.h"

namespace aadff {

constexpr int BT = 32;                  // tile edge of the patch-convolution gradients (pixels)

// ------------------------------------------------------------------------------------
// (a1) d_img of the patch convolution.  In image coordinates (U, V) = padded position minus p:
//   g(U, V) = sum_{a, e < ks} dy[U + a - p][V + e - p] * psf_{patch of that dy pixel}[a][e]          (terms whose dy pixel exists)
//   d_img[y][x] = g(y, x) + g at the mirror images of (y, x) under the reflect padding (-y for 1 <= y <= p, 2 (H - 1) - y for
//   H - 1 - p <= y <= H - 2; the same in x; up to 3 x 3 positions when H or W is barely larger than p).
// Workgroup = one 32 x 32 tile of one (b, c) plane, all S slices; lane = column, 4 rows per thread.  The dy window (tile + p halo,
// zero outside the image) is staged in LDS per slice.  The PSF belongs to the SOURCE pixel, so the taps run once per patch that
// meets the wave's window, dy masked to that patch: the weights are then wave-uniform (scalar loads, SGPR operands).  A masked
// term adds an exact zero.  Every mirror image's sources lie inside the direct window, so they are read from the same tile (border
// threads only, per-lane weights).  Sums: ks-term column partials -> the slice's accumulator -> added over the slices.
// ------------------------------------------------------------------------------------
template <int KS>
__global__ __launch_bounds__(256) void map_dimg_kernel(const float* __restrict__ psf, const float* __restrict__ dy, float* __restrict__ dimg,
                                                       int C, int S, int H, int W, int grid, int ks_rt, PatchBounds pb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int ks = KS > 0 ? KS : ks_rt, p = ks / 2, TP = BT + 2 * p, G = grid * ks;
    float* tile = smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int lx = lane & 31, lyg = wave * 2 + (lane >> 5);
    const int bc = blockIdx.z, c = bc % C;
    const int x0 = blockIdx.x * BT, y0 = blockIdx.y * BT;
    const int x = x0 + lx, yb = y0 + 4 * lyg;

    // patches that hold a source pixel of this tile / of this wave's rows (uniform: bounds from the kernel arguments, scalar code)
    const int sx_lo = max(x0 - p, 0), sx_hi = min(x0 + BT - 1 + p, W - 1);
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
    for (int s = 0; s < S; ++s) {
        const float* dyp = dy + ((size_t)bc * S + s) * H * W;
        __syncthreads();
        for (int e = tid; e < TP * TP; e += 256) {
            const int r = e / TP, cc = e - r * TP;
            const int yy = y0 - p + r, xx = x0 - p + cc;
            tile[e] = (yy >= 0 && yy < H && xx >= 0 && xx < W) ? dyp[(size_t)yy * W + xx] : 0.f;
        }
        __syncthreads();
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (wy_lo <= wy_hi) {
            for (int pi = pi_lo; pi <= pi_hi; ++pi) {
                const int ry0 = pb.hb[pi], ry1 = pb.hb[pi + 1];
                for (int pj = pj_lo; pj <= pj_hi; ++pj) {
                    const int cx0 = pb.wb[pj], cx1 = pb.wb[pj + 1];
                    const float* wp = psf + ((size_t)(s * C + c) * G + pi * ks) * G + pj * ks;
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
                    // ---- its mirror images under the reflect padding.  A mirror of row y is -y (y <= p) or 2 (H - 1) - y (y >= H - 1 - p); its sources
                    //      [mirror - p, mirror + p] clipped to the image are [0, p - y] or [2 (H - 1) - y - p, H - 1], both inside the direct window
                    //      [y - p, y + p]: the same tile rows, and patches inside this wave's [wy_lo, wy_hi].  Columns alike. ----
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
        for (int k = 0; k < 4; ++k) total[k] += acc[k];
    }
    if (x < W) {
        float* o = dimg + (size_t)bc * H * W + x;
#pragma unroll
        for (int k = 0; k < 4; ++k)
            if (yb + k < H) o[(size_t)(yb + k) * W] = total[k];
    }
}

// ------------------------------------------------------------------------------------
// (a2) d_psf of the patch convolution:
//   d_psf[s][c][i ks + a][j ks + e] = sum_b sum_{(y, x) in patch (i, j)} dy[b][c][s][y][x] * img[b][c][refl(y + p - a)][refl(x + p - e)]
// First pass: workgroup = one 32 x 32 tile of one patch and (b, c) plane; the reflect-padded image window is staged once for all S
// slices, the dy tile (zero outside the patch) per slice.  Wave w takes the tap rows a = w, w + 4, ...; a lane owns 4 x 4 pixels
// (4 consecutive columns in 4 rows) and EB taps of the row at a time, a sliding window of EB + 3 image values per pixel row.
// Sums: 16 terms per lane -> wave tree -> one partial per (tile, b) in the slab.  Second pass: the partials of a tap in a fixed order.
// EB = ks for the tuned size, 1 for any ks.
// ------------------------------------------------------------------------------------
template <int EB>
__global__ __launch_bounds__(256) void map_dpsf_partial_kernel(const float* __restrict__ img, const float* __restrict__ dy, float* __restrict__ part,
                                                               int C, int S, int H, int W, int grid, int ks, int ntx, int nty, PatchBounds pb) {
    extern __shared__ __attribute__((aligned(16))) float smem[];
    const int p = ks / 2, TP = BT + 2 * p, kk = ks * ks;
    float* tdy = smem;                      // [32][32]
    float* timg = smem + BT * BT;           // [TP][TP]
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);
    const int pj = blockIdx.x / ntx, tx = blockIdx.x - pj * ntx;
    const int pi = blockIdx.y / nty, ty = blockIdx.y - pi * nty;
    const int bc = blockIdx.z, b = bc / C, c = bc - b * C;
    const int x_hi = pb.wb[pj + 1], y_hi = pb.hb[pi + 1];
    const int x0 = pb.wb[pj] + tx * BT, y0 = pb.hb[pi] + ty * BT;
    if (x0 >= x_hi || y0 >= y_hi) return;

    const float* plane = img + (size_t)bc * H * W;
    for (int e = tid; e < TP * TP; e += 256) {
        const int r = e / TP, cc = e - r * TP;
        timg[e] = plane[(size_t)reflect_idx(y0 - p + r, H) * W + reflect_idx(x0 - p + cc, W)];
    }
    const int lxg = lane & 7, lyr = lane >> 3;
    const int nblk = (ks + EB - 1) / EB, units = ks * nblk;
    const size_t slab = (size_t)b * ntx * nty + (size_t)ty * ntx + tx;
    for (int s = 0; s < S; ++s) {
        const float* dyp = dy + ((size_t)bc * S + s) * H * W;
        __syncthreads();
        for (int e = tid; e < BT * BT; e += 256) {
            const int y = y0 + (e >> 5), xx = x0 + (e & 31);
            tdy[e] = (y < y_hi && xx < x_hi) ? dyp[(size_t)y * W + xx] : 0.f;
        }
        __syncthreads();
        float* po = part + ((((size_t)slab * S + s) * C + c) * grid * grid + (size_t)pi * grid + pj) * kk;
        for (int u = wave; u < units; u += 4) {
            const int a = u / nblk, e0 = (u - a * nblk) * EB;
            float acc[EB];
#pragma unroll
            for (int m = 0; m < EB; ++m) acc[m] = 0.f;
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const int row = lyr + 8 * j;
                const float4 d4 = *reinterpret_cast<const float4*>(tdy + row * BT + 4 * lxg);
                const float d[4] = {d4.x, d4.y, d4.z, d4.w};
                // pixel column 4 lxg + k and tap e0 + m read image column 4 lxg + k + 2p - e0 - m of the window
                const float* tr = timg + (row + 2 * p - a) * TP + 4 * lxg + 2 * p - e0 - (EB - 1);
                float v[EB + 3];
#pragma unroll
                for (int q = 0; q < EB + 3; ++q) v[q] = tr[q];
#pragma unroll
                for (int k = 0; k < 4; ++k)
#pragma unroll
                    for (int m = 0; m < EB; ++m) acc[m] = fmaf(d[k], v[k + EB - 1 - m], acc[m]);
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

// second pass: one thread per PSF-map element; its partials in the order b, tile row, tile column (tile rows summed first)
__global__ __launch_bounds__(256) void map_dpsf_sum_kernel(const float* __restrict__ part, float* __restrict__ dpsf, int B, int C, int S,
                                                           int grid, int ks, int ntx, int nty, PatchBounds pb) {
    const int G = grid * ks, kk = ks * ks;
    const size_t n = (size_t)S * C * G * G;
    const size_t idx = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (idx >= n) return;
    const int col = (int)(idx % G), row = (int)((idx / G) % G);
    const size_t sc = idx / ((size_t)G * G);
    const int pi = row / ks, a = row - pi * ks, pj = col / ks, e = col - pj * ks;
    const int ph = pb.hb[pi + 1] - pb.hb[pi], pw = pb.wb[pj + 1] - pb.wb[pj];
    const int tyn = (ph + BT - 1) / BT, txn = (pw + BT - 1) / BT;
    const size_t per_slab = (size_t)S * C * grid * grid * kk;
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
    dpsf[idx] = sum;
}

struct BwdPlan { PatchBounds pb; int ntx, nty; size_t ws_bytes; };

static void plan_map_bwd(BwdPlan& pl, int B, int C, int S, int H, int W, int grid, int ks) {
    std::memset(&pl.pb, 0, sizeof(pl.pb));
    fill_bounds(pl.pb.hb, grid, H);
    fill_bounds(pl.pb.wb, grid, W);
    int mh = 0, mw = 0;
    for (int i = 0; i < grid; ++i) {
        mh = std::max(mh, pl.pb.hb[i + 1] - pl.pb.hb[i]);
        mw = std::max(mw, pl.pb.wb[i + 1] - pl.pb.wb[i]);
    }
    pl.ntx = (mw + BT - 1) / BT;
    pl.nty = (mh + BT - 1) / BT;
    // one slab of S * C * (grid ks)^2 floats per (b, tile of a patch)
    pl.ws_bytes = (size_t)B * pl.ntx * pl.nty * S * C * grid * grid * ks * ks * sizeof(float);
}

}  // namespace aadff

using namespace aadff;

extern "C" {

int aadff_render_psf_map_stack_bwd_workspace(int B, int C, int S, int H, int W, int grid, int ks, size_t* bytes) {
    AADFF_CHECK_ARG(bytes, "render_psf_map_stack_bwd_workspace: bytes is NULL");
    if (int rc = conv_check_shape(B, C, S, H, W, grid, ks)) return rc;
    BwdPlan pl;
    plan_map_bwd(pl, B, C, S, H, W, grid, ks);
    *bytes = pl.ws_bytes;
    return 0;
}

int aadff_render_psf_map_stack_bwd(const float* img, const float* psf_maps, const float* dy, float* d_img_or_null, float* d_psf_or_null,
                                   void* workspace, size_t workspace_bytes, int B, int C, int S, int H, int W, int grid, int ks,
                                   aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && psf_maps && dy, "render_psf_map_stack_bwd: NULL pointer (img, psf_maps, dy)");
    AADFF_CHECK_ARG(d_img_or_null || d_psf_or_null, "render_psf_map_stack_bwd: d_img and d_psf are both NULL");
    if (int rc = conv_check_shape(B, C, S, H, W, grid, ks)) return rc;
    BwdPlan pl;
    plan_map_bwd(pl, B, C, S, H, W, grid, ks);
    if (d_psf_or_null)
        AADFF_CHECK_ARG(workspace && workspace_bytes >= pl.ws_bytes, "render_psf_map_stack_bwd: workspace of %zu bytes is too small, d_psf needs %zu",
                        workspace ? workspace_bytes : (size_t)0, pl.ws_bytes);
    AADFF_CHECK_ARG((size_t)(H + BT - 1) / BT <= 65535 && (size_t)pl.nty * grid <= 65535, "render_psf_map_stack_bwd: H %d too large for the launch grid", H);
    hipStream_t st = (hipStream_t)stream;
    const int TP = BT + ks - 1;
    if (d_img_or_null) {
        dim3 g((W + BT - 1) / BT, (H + BT - 1) / BT, B * C);
        const size_t lds = (size_t)TP * TP * sizeof(float);
        if (ks == 11) hipLaunchKernelGGL(map_dimg_kernel<11>, g, dim3(256), lds, st, psf_maps, dy, d_img_or_null, C, S, H, W, grid, ks, pl.pb);
        else hipLaunchKernelGGL(map_dimg_kernel<0>, g, dim3(256), lds, st, psf_maps, dy, d_img_or_null, C, S, H, W, grid, ks, pl.pb);
        AADFF_CHECK_LAUNCH();
    }
    if (d_psf_or_null) {
        dim3 g(pl.ntx * grid, pl.nty * grid, B * C);
        const size_t lds = (size_t)(BT * BT + TP * TP) * sizeof(float);
        float* part = static_cast<float*>(workspace);
        if (ks == 11) hipLaunchKernelGGL(map_dpsf_partial_kernel<11>, g, dim3(256), lds, st, img, dy, part, C, S, H, W, grid, ks, pl.ntx, pl.nty, pl.pb);
        else hipLaunchKernelGGL(map_dpsf_partial_kernel<1>, g, dim3(256), lds, st, img, dy, part, C, S, H, W, grid, ks, pl.ntx, pl.nty, pl.pb);
        AADFF_CHECK_LAUNCH();
        const size_t n = (size_t)S * C * grid * ks * grid * ks;
        hipLaunchKernelGGL(map_dpsf_sum_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, st, part, d_psf_or_null, B, C, S, grid, ks, pl.ntx,
                           pl.nty, pl.pb);
        AADFF_CHECK_LAUNCH();
    }
    return 0;
}

}  // extern "C"
