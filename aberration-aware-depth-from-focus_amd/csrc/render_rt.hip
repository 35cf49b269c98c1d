// Ray-traced image rendering for gfx950: the plane render, the layered RGB-D render and the jitter generator, with their C entries.  The
// two kernels share render_pixel, sensor_point, render_ray and scene_taps (each kernel still forms its own scene coordinates, see the layered one).
#include <algorithm>
#include <cmath>
#include <type_traits>
#include "trace_core.h"

namespace aadff {

// ------------------------------------------------------------------------------------
// Ray-traced image rendering: sensor pixel -> exit pupil -> backwards through the lens -> object plane ->
// bilinear sample of the scene.  One lane owns one (pixel, channel): it loops over the spp samples and keeps the valid
// count and the running sums of up to kRenderMaxB images in registers (the rays do not depend on the image), so there is
// no atomic and no cross-lane reduction, every output is written once and a launch is bit-reproducible.  A wave covers an
// 8 x 8 pixel block, a workgroup 16 x 16, blockIdx.z is the channel (= wavelength: the surface table stays wave-uniform);
// neighbouring lanes land on neighbouring texels, which ordinary global loads then fetch from the same cache lines.
// ------------------------------------------------------------------------------------
constexpr int kRenderTile = 16, kRenderMaxB = 4, kRenderAngles = 8;

// Jitter uniform number `idx` of a render with `seed`: output idx of the SplitMix64 sequence seeded with `seed` (Steele, Lea,
// Flood 2014), top 24 bits -> [0, 1).  idx is the flat index into u[3, spp, 2, H, W]: ((channel * spp + sample) * 2 + which) * H * W
// + pixel, so the value is a pure function of (seed, channel, sample, which, pixel) and aadff_sensor_uniforms reproduces it.
__device__ __forceinline__ float sensor_uniform(unsigned long long seed, unsigned long long idx) {
    unsigned long long z = seed + (idx + 1ull) * 0x9E3779B97F4A7C15ull;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return (float)(unsigned)(z >> 40) * 5.9604644775390625e-8f;          // 24 bits * 2^-24
}

__global__ __launch_bounds__(256) void sensor_uniforms_kernel(unsigned long long seed, size_t n, float* __restrict__ out) {
    const size_t i = (size_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i < n) out[i] = sensor_uniform(seed, i);
}

struct RenderGeom {
    int H, W, spp, rings;                 // rings = spp / 8
    float pupil_z, r2_step;               // r2_step = pupil_r^2 / spp * 8 (sample_pupil, optics.py:579)
    float x0, y0, ps;                     // sensor point of pixel (i, j): (x0 + (j+1) ps, y0 - (i+1) ps), x0 = -Ws/2, y0 = Hs/2
    float depth, inv_texel, cu, cv;       // uj = cu - px inv_texel, vi = cv + py inv_texel; inv_texel = 1 / (scale ps), cu = W/2 - 1, cv = H/2 - 1
};

// The pieces that the two render kernels share.  Each is straight-line code on values (no branch, no result through a reference): in
// that form the kernels compile to the code they had with the text written out in place; with a branch or a reference in a shared
// function they did not (profiles/split_trace_units_kernel_hashes.md).
// pixel of the lane: a wave covers 8 x 8 pixels, a workgroup 16 x 16
struct RenderPixel { int i, j; };
__device__ __forceinline__ RenderPixel render_pixel() {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    return {(int)(blockIdx.y * kRenderTile + (wave >> 1) * 8 + (lane >> 3)), (int)(blockIdx.x * kRenderTile + (wave & 1) * 8 + (lane & 7))};
}
struct SensorPoint { float x, y; };
__device__ __forceinline__ SensorPoint sensor_point(const RenderGeom& g, int i, int j) { return {g.x0 + (float)(j + 1) * g.ps, g.y0 - (float)(i + 1) * g.ps}; }
// the ray of a draw, from the sensor point to the pupil point of sector `sec`, ring `ring` jittered by (ut, ur): sample s = sector * rings
// + ring (optics.py:574-582)
__device__ __forceinline__ Ray render_ray(const RenderGeom& g, float sx, float sy, float d_sensor, float ut, float ur, int sec, int ring) {
    const float rev = (ut + (float)sec) * (1.f / kRenderAngles);      // theta / (2 pi)
    const float rr = fsqrt((ur + (float)ring) * g.r2_step);
    return ray_to(sx, sy, d_sensor, rr * __builtin_amdgcn_cosf(rev), rr * __builtin_amdgcn_sinf(rev), g.pupil_z);
}
// Bilinear weights and the four taps of scene coordinates inside the window [-1, W] x [-1, H], replicate border: columns xa, xb, row
// offsets ra, rb.  The caller tests the window first (NaN-safe: other coordinates are never turned into an index).
struct SceneTaps { float ax, ay; int xa, xb; size_t ra, rb; };
__device__ __forceinline__ SceneTaps scene_taps(const RenderGeom& g, float uj, float vi) {
    const float fu = floorf(uj), fv = floorf(vi);
    const int xi = (int)fu, yi = (int)fv;
    return {uj - fu, vi - fv, min(max(xi, 0), g.W - 1), min(max(xi + 1, 0), g.W - 1), (size_t)min(max(yi, 0), g.H - 1) * g.W,
            (size_t)min(max(yi + 1, 0), g.H - 1) * g.W};
}

template <int NB>
__global__ __launch_bounds__(kRenderTile * kRenderTile) void render_raytraced_kernel(
    const float* __restrict__ img, const float* __restrict__ u, unsigned long long seed, const aadff_surface_t* __restrict__ surf, int n_surf,
    RenderGeom g, int vignetting, const aadff_lens_state_t* __restrict__ state, float* __restrict__ out, float* __restrict__ count,
    unsigned char* __restrict__ valid_out, int* flags) {
    const float d_sensor = fresh_uniform(&state->d_sensor);
    const int c = blockIdx.z;
    const RenderPixel pxl = render_pixel();
    const int i = pxl.i, j = pxl.j;
    if (i >= g.H || j >= g.W) return;
    const size_t HW = (size_t)g.H * g.W, pix = (size_t)i * g.W + j;
    const aadff_surface_t* tab = surf + (size_t)c * n_surf;
    const float* im = img + (size_t)c * HW;                               // image b: im + b * 3 * HW
    const SensorPoint sp = sensor_point(g, i, j);
    const float sx = sp.x, sy = sp.y;
    const float fW = (float)g.W, fH = (float)g.H;
    float acc[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) acc[b] = 0.f;
    float cnt = 0.f;
    int nan_flag = 0, sec = 0, ring = 0;
#pragma unroll 1
    for (int s = 0; s < g.spp; ++s) {
        // sample s = sector * rings + ring (optics.py:574-582); theta draw, then r^2 draw
        const size_t k = (size_t)(c * g.spp + s) * 2 * HW + pix;
        float ut, ur;
        if (u) { ut = u[k]; ur = u[k + HW]; }
        else { ut = sensor_uniform(seed, k); ur = sensor_uniform(seed, k + HW); }
        Ray r = render_ray(g, sx, sy, d_sensor, ut, ur, sec, ring);
        trace_range<false>(tab, 0, n_surf, false, r, nan_flag);
        propagate_to(r, g.depth);
        const float uj = g.cu - r.ox * g.inv_texel, vi = g.cv + r.oy * g.inv_texel;
        // NaN-safe: a dead ray's coordinates are never turned into an index
        const bool ok = (r.ra > 0.f) && (uj >= -1.f) && (uj <= fW) && (vi >= -1.f) && (vi <= fH);
        if (valid_out) valid_out[(size_t)(c * g.spp + s) * HW + pix] = ok ? 1 : 0;
        if (ok) {
            const SceneTaps tp = scene_taps(g, uj, vi);
            const float ax = tp.ax, ay = tp.ay;
            const int xa = tp.xa, xb = tp.xb;
            const size_t ra = tp.ra, rb = tp.rb;
            cnt += 1.f;
            // every fusion is written out and none is left to the compiler, which contracts differently from one instantiation
            // to the next: an image must render to the same bits whichever launch of a chunked batch it falls into
            {
#pragma clang fp contract(off)
                const float bx = 1.f - ax, by = 1.f - ay;
#pragma unroll
                for (int b = 0; b < NB; ++b) {
                    const float* p = im + (size_t)b * 3 * HW;
                    const float top = __builtin_fmaf(ax, p[ra + xb], bx * p[ra + xa]);
                    const float bot = __builtin_fmaf(ax, p[rb + xb], bx * p[rb + xa]);
                    acc[b] += __builtin_fmaf(ay, bot, by * top);
                }
            }
        }
        if (++ring == g.rings) { ring = 0; ++sec; }
    }
    const float den = vignetting ? (float)g.spp : cnt;
#pragma unroll
    for (int b = 0; b < NB; ++b) out[((size_t)b * 3 + c) * HW + pix] = cnt > 0.f ? acc[b] / den : 0.f;
    if (count) count[(size_t)c * HW + pix] = cnt;
    if (nan_flag && flags) atomicOr(flags, 1);    // found nan in ft in non-diff newton method (surfaces.py:555-558)
}

// ------------------------------------------------------------------------------------
// Ray-traced rendering of a layered RGB-D scene: the scene is L fronto-parallel planes z_0 > ... > z_{L-1}
// (nearest first) and a map layer[b] [H,W] that says which plane a texel lies on.  The lane layout, the rays and the sampling
// are render_raytraced_kernel's (the shared functions above); a ray that survived the lens is propagated from its
// last surface to every plane in turn and composites front to back with a transmittance T (per ray and image: V += T q,
// A += T a, T *= 1 - a, where a and q are the bilinear forms of the texels' membership in the plane and of their
// membership-selected values).  Per image the lane keeps the sums of V and A over its rays; no atomics, every output written
// once.  The plane table is a kernel argument: indexed by the wave-uniform loop counter it is read through scalar loads.  With
// L = 1 and layer == 0 the taps are the plane render's own (scene_taps) and every step of the blend reduces to
// render_raytraced_kernel's, to the bit (a = 1 exactly, V = q, A = 1).
// ------------------------------------------------------------------------------------
struct RenderLayers {
    int L;
    float z[AADFF_RENDER_MAX_LAYERS], inv_texel[AADFF_RENDER_MAX_LAYERS];    // inv_texel[l] = 1 / (scale_l ps)
};

template <int NB>
__global__ __launch_bounds__(kRenderTile * kRenderTile) void render_raytraced_layered_kernel(
    const float* __restrict__ img, const unsigned char* __restrict__ layer, const float* __restrict__ u, unsigned long long seed,
    const aadff_surface_t* __restrict__ surf, int n_surf, RenderGeom g, RenderLayers lt, int vignetting,
    const aadff_lens_state_t* __restrict__ state, float* __restrict__ out, float* __restrict__ coverage, float* __restrict__ alive_out,
    unsigned char* __restrict__ alive_rays, int* flags) {
    const float d_sensor = fresh_uniform(&state->d_sensor);
    const int c = blockIdx.z;
    const RenderPixel pxl = render_pixel();
    const int i = pxl.i, j = pxl.j;
    if (i >= g.H || j >= g.W) return;
    const size_t HW = (size_t)g.H * g.W, pix = (size_t)i * g.W + j;
    const aadff_surface_t* tab = surf + (size_t)c * n_surf;
    const float* im = img + (size_t)c * HW;                               // image b: im + b * 3 * HW, its layer map: layer + b * HW
    const SensorPoint sp = sensor_point(g, i, j);
    const float sx = sp.x, sy = sp.y;
    const float fW = (float)g.W, fH = (float)g.H;
    float sumV[NB], sumA[NB];
#pragma unroll
    for (int b = 0; b < NB; ++b) { sumV[b] = 0.f; sumA[b] = 0.f; }
    float cnt = 0.f;
    int nan_flag = 0, sec = 0, ring = 0;
#pragma unroll 1
    for (int s = 0; s < g.spp; ++s) {
        const size_t k = (size_t)(c * g.spp + s) * 2 * HW + pix;
        float ut, ur;
        if (u) { ut = u[k]; ur = u[k + HW]; }
        else { ut = sensor_uniform(seed, k); ur = sensor_uniform(seed, k + HW); }
        Ray r = render_ray(g, sx, sy, d_sensor, ut, ur, sec, ring);
        trace_range<false>(tab, 0, n_surf, false, r, nan_flag);
        const bool live = r.ra > 0.f;
        if (alive_rays) alive_rays[(size_t)(c * g.spp + s) * HW + pix] = live ? 1 : 0;
        if (live) {
            cnt += 1.f;
            float V[NB], A[NB], T[NB];
#pragma unroll
            for (int b = 0; b < NB; ++b) { V[b] = 0.f; A[b] = 0.f; T[b] = 1.f; }
#pragma unroll 1
            for (int l = 0; l < lt.L; ++l) {
                // propagate_to(r, z_l) from the last surface for every plane, and the scene coordinates, with the fusions that the
                // compiler makes in render_raytraced_kernel written out: here, inside the plane loop, it left vi unfused; written
                // out over there as well, the one-image plane render is 0.3 % slower, so L = 1 is the plane render
                // for as long as the compiler fuses there (the L = 1 identity is the default build's; tests/test_gpu_raytrace_layered.py)
                const float t = fdiv(lt.z[l] - r.oz, r.dz), inv_texel = lt.inv_texel[l];
                const float px = __builtin_fmaf(r.dx, t, r.ox), py = __builtin_fmaf(r.dy, t, r.oy);
                const float uj = __builtin_fmaf(-px, inv_texel, g.cu), vi = __builtin_fmaf(py, inv_texel, g.cv);
                // NaN-safe: coordinates that are not in the window are never turned into an index
                const bool ok = (uj >= -1.f) && (uj <= fW) && (vi >= -1.f) && (vi <= fH);
                if (ok) {
                    const SceneTaps tp = scene_taps(g, uj, vi);
                    const float ax = tp.ax, ay = tp.ay;
                    const int xa = tp.xa, xb = tp.xb;
                    const size_t ra = tp.ra, rb = tp.rb;
                    {
#pragma clang fp contract(off)
                        const float bx = 1.f - ax, by = 1.f - ay;
#pragma unroll
                        for (int b = 0; b < NB; ++b) {
#ifndef AADFF_LAYERED_NO_MAP
                            const unsigned char* lay = layer + (size_t)b * HW;
                            const bool m00 = lay[ra + xa] == l, m01 = lay[ra + xb] == l, m10 = lay[rb + xa] == l, m11 = lay[rb + xb] == l;
#else       // measurement build (the cost of L = 1): every texel on plane 0, the map is not read
                            const bool m00 = l == 0, m01 = m00, m10 = m00, m11 = m00;
#endif
                            if (m00 || m01 || m10 || m11) {               // none of the four on this plane: a = q = 0 exactly, nothing changes
                                const float* q = im + (size_t)b * 3 * HW;
                                const float atop = __builtin_fmaf(ax, m01 ? 1.f : 0.f, bx * (m00 ? 1.f : 0.f));
                                const float abot = __builtin_fmaf(ax, m11 ? 1.f : 0.f, bx * (m10 ? 1.f : 0.f));
                                const float a = __builtin_fmaf(ay, abot, by * atop);
                                const float qtop = __builtin_fmaf(ax, m01 ? q[ra + xb] : 0.f, bx * (m00 ? q[ra + xa] : 0.f));
                                const float qbot = __builtin_fmaf(ax, m11 ? q[rb + xb] : 0.f, bx * (m10 ? q[rb + xa] : 0.f));
                                const float qv = __builtin_fmaf(ay, qbot, by * qtop);
                                const float tq = T[b] * qv, ta = T[b] * a;
                                V[b] = V[b] + tq;
                                A[b] = A[b] + ta;
                                T[b] = T[b] * (1.f - a);
                            }
                        }
                    }
                    bool opaque = true;
#pragma unroll
                    for (int b = 0; b < NB; ++b) opaque = opaque && T[b] == 0.f;
                    if (opaque) break;                                    // nothing behind can add to any image of this launch
                }
            }
#pragma unroll
            for (int b = 0; b < NB; ++b) { sumV[b] += V[b]; sumA[b] += A[b]; }
        }
        if (++ring == g.rings) { ring = 0; ++sec; }
    }
#pragma unroll
    for (int b = 0; b < NB; ++b) {
        const float den = vignetting ? (float)g.spp : sumA[b];
        out[((size_t)b * 3 + c) * HW + pix] = sumA[b] > 0.f ? sumV[b] / den : 0.f;
        if (coverage) coverage[((size_t)b * 3 + c) * HW + pix] = sumA[b];
    }
    if (alive_out) alive_out[(size_t)c * HW + pix] = cnt;
    if (nan_flag && flags) atomicOr(flags, 1);    // found nan in ft in non-diff newton method (surfaces.py:555-558)
}

}  // namespace aadff

using namespace aadff;

// The argument checks that the two render entries share (who: the entry's name in the messages), the geometry and the grid.  The
// scene plane of g (depth, inv_texel) is the caller's to fill.
static int render_setup(const char* who, int B, int H, int W, int spp, int n_surf, float pupil_z, float pupil_r, float sensor_w, float sensor_h,
                        float pixel_size, RenderGeom& g, dim3& grid) {
    AADFF_CHECK_ARG(B >= 1 && H >= 1 && W >= 1, "%s: bad sizes B=%d H=%d W=%d", who, B, H, W);
    AADFF_CHECK_ARG(spp > 0 && spp % kRenderAngles == 0, "%s: spp=%d must be a positive multiple of %d (stratified pupil samples)", who, spp,
                    kRenderAngles);
    AADFF_CHECK_ARG(n_surf > 0 && n_surf <= AADFF_MAX_SURF, "%s: n_surf %d outside [1,%d]", who, n_surf, AADFF_MAX_SURF);
    AADFF_CHECK_ARG(std::isfinite(pupil_z) && std::isfinite(pupil_r) && pupil_r >= 0.f, "%s: bad pupil (z=%g, r=%g)", who, (double)pupil_z,
                    (double)pupil_r);
    AADFF_CHECK_ARG(std::isfinite(sensor_w) && std::isfinite(sensor_h) && sensor_w > 0.f && sensor_h > 0.f, "%s: bad sensor size (%g x %g mm)", who,
                    (double)sensor_w, (double)sensor_h);
    grid = dim3((W + kRenderTile - 1) / kRenderTile, (H + kRenderTile - 1) / kRenderTile, 3);     // grid.y: checked by the caller, last
    g.H = H; g.W = W; g.spp = spp; g.rings = spp / kRenderAngles;
    g.pupil_z = pupil_z;
    g.r2_step = r2_step(pupil_r, spp, kRenderAngles);
    g.x0 = (float)(-(double)sensor_w / 2); g.y0 = (float)((double)sensor_h / 2); g.ps = pixel_size;
    g.cu = (float)(W / 2.0 - 1.0); g.cv = (float)(H / 2.0 - 1.0);
    return 0;
}

// The rays do not depend on the image: B images are rendered kRenderMaxB at a time, every launch tracing the same samples for its
// images.  launch(NB, b0) launches the kernel instantiated for NB::value images on the images from b0.
template <class F>
static int render_chunks(int B, F launch) {
    for (int b0 = 0; b0 < B; b0 += kRenderMaxB) {
        switch (std::min(kRenderMaxB, B - b0)) {
            case 1: launch(std::integral_constant<int, 1>{}, b0); break;
            case 2: launch(std::integral_constant<int, 2>{}, b0); break;
            case 3: launch(std::integral_constant<int, 3>{}, b0); break;
            default: launch(std::integral_constant<int, 4>{}, b0); break;
        }
        AADFF_CHECK_LAUNCH();
    }
    return 0;
}

extern "C" {

int aadff_sensor_uniforms(unsigned long long seed, int spp, int H, int W, float* out, aadff_stream_t stream) {
    AADFF_CHECK_ARG(out, "sensor_uniforms: NULL pointer");
    AADFF_CHECK_ARG(spp > 0 && spp % kRenderAngles == 0, "sensor_uniforms: spp=%d must be a positive multiple of %d", spp, kRenderAngles);
    AADFF_CHECK_ARG(H >= 1 && W >= 1, "sensor_uniforms: bad sizes H=%d W=%d", H, W);
    const size_t n = (size_t)3 * spp * 2 * H * W;
    AADFF_CHECK_ARG((n + 255) / 256 <= 0x7fffffffull, "sensor_uniforms: 3*spp*2*H*W = %zu is too large for one launch", n);
    hipLaunchKernelGGL(sensor_uniforms_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, seed, n, out);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_render_raytraced(const float* img, int B, int H, int W, const float* u_or_null, unsigned long long seed, int spp,
                           const aadff_surface_t* surf_rgb, int n_surf, float pupil_z, float pupil_r, float sensor_w, float sensor_h,
                           float pixel_size, float depth, float scale, int vignetting, const aadff_lens_state_t* state, float* out,
                           float* count_or_null, unsigned char* valid_or_null, int* flags_or_null, aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && surf_rgb && state && out, "render_raytraced: NULL pointer");
    RenderGeom g;
    dim3 grid;
    if (const int rc = render_setup("render_raytraced", B, H, W, spp, n_surf, pupil_z, pupil_r, sensor_w, sensor_h, pixel_size, g, grid)) return rc;
    const double texel = (double)scale * (double)pixel_size;
    AADFF_CHECK_ARG(std::isfinite(texel) && texel > 0.0 && pixel_size > 0.f,
                    "render_raytraced: scale * pixel_size must be positive (scale=%g, pixel_size=%g)", (double)scale, (double)pixel_size);
    AADFF_CHECK_ARG(depth < 0.f && std::isfinite(depth), "render_raytraced: depth %g must be negative (object plane in front of the lens)",
                    (double)depth);
    AADFF_CHECK_ARG(grid.y <= 65535u, "render_raytraced: H=%d exceeds %d rows", H, 65535 * kRenderTile);
    g.depth = depth; g.inv_texel = (float)(1.0 / texel);
    const size_t plane = (size_t)3 * H * W;
    return render_chunks(B, [&](auto nb, int b0) {
        hipLaunchKernelGGL(render_raytraced_kernel<decltype(nb)::value>, grid, dim3(kRenderTile * kRenderTile), 0, (hipStream_t)stream,
                           img + (size_t)b0 * plane, u_or_null, seed, surf_rgb, n_surf, g, vignetting, state, out + (size_t)b0 * plane,
                           b0 == 0 ? count_or_null : nullptr, b0 == 0 ? valid_or_null : nullptr, flags_or_null);
    });
}

int aadff_render_raytraced_layered(const float* img, const unsigned char* layer, int B, int H, int W, const float* u_or_null,
                                   unsigned long long seed, int spp, const aadff_surface_t* surf_rgb, int n_surf, float pupil_z,
                                   float pupil_r, float sensor_w, float sensor_h, float pixel_size, int L, const float* layer_depths,
                                   const float* scales, int vignetting, const aadff_lens_state_t* state, float* out,
                                   float* coverage_or_null, float* alive_or_null, unsigned char* alive_rays_or_null, int* flags_or_null,
                                   aadff_stream_t stream) {
    AADFF_CHECK_ARG(img && layer && surf_rgb && layer_depths && scales && state && out, "render_raytraced_layered: NULL pointer");
    RenderGeom g;
    dim3 grid;
    if (const int rc = render_setup("render_raytraced_layered", B, H, W, spp, n_surf, pupil_z, pupil_r, sensor_w, sensor_h, pixel_size, g, grid))
        return rc;
    AADFF_CHECK_ARG(L >= 1 && L <= AADFF_RENDER_MAX_LAYERS, "render_raytraced_layered: L=%d layers outside [1,%d]", L, AADFF_RENDER_MAX_LAYERS);
    RenderLayers lt{};
    lt.L = L;
    for (int l = 0; l < L; ++l) {
        const float z = layer_depths[l];
        AADFF_CHECK_ARG(z < 0.f && std::isfinite(z), "render_raytraced_layered: layer depth %d = %g must be negative (planes in front of the lens)",
                        l, (double)z);
        AADFF_CHECK_ARG(l == 0 || z < layer_depths[l - 1],
                        "render_raytraced_layered: layer depths must be strictly decreasing, nearest first (depth %d = %g after %g)", l, (double)z,
                        (double)layer_depths[l - 1]);
        const double texel = (double)scales[l] * (double)pixel_size;
        AADFF_CHECK_ARG(std::isfinite(texel) && texel > 0.0 && pixel_size > 0.f,
                        "render_raytraced_layered: scale * pixel_size must be positive (layer %d: scale=%g, pixel_size=%g)", l, (double)scales[l],
                        (double)pixel_size);
        lt.z[l] = z;
        lt.inv_texel[l] = (float)(1.0 / texel);
    }
    AADFF_CHECK_ARG(grid.y <= 65535u, "render_raytraced_layered: H=%d exceeds %d rows", H, 65535 * kRenderTile);
    g.depth = lt.z[0]; g.inv_texel = lt.inv_texel[0];                     // not read: the planes come from the table
    const size_t HW = (size_t)H * W;
    return render_chunks(B, [&](auto nb, int b0) {
        hipLaunchKernelGGL(render_raytraced_layered_kernel<decltype(nb)::value>, grid, dim3(kRenderTile * kRenderTile), 0, (hipStream_t)stream,
                           img + (size_t)b0 * 3 * HW, layer + (size_t)b0 * HW, u_or_null, seed, surf_rgb, n_surf, g, lt, vignetting, state,
                           out + (size_t)b0 * 3 * HW, coverage_or_null ? coverage_or_null + (size_t)b0 * 3 * HW : nullptr,
                           b0 == 0 ? alive_or_null : nullptr, b0 == 0 ? alive_rays_or_null : nullptr, flags_or_null);
    });
}

}  // extern "C"
