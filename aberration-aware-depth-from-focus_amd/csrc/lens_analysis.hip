// Ray-traced lens analysis for gfx950: spot moments and MTF of field points, with their C entries.  Both kernels sum with
// block_sums; the stratified pupil pair is written out in each: drawn through one shared function, mtf_points_kernel compiled to
// other code than before (two instructions in another order) in every form tried, profiles/split_trace_units_kernel_hashes.md.
#include <cmath>
#include "trace_core.h"

namespace aadff {

constexpr int kSpotThreads = 256, kSpotWaves = kSpotThreads / 64;
constexpr int kSpotMaxPairs = 4;          // two rays per lane: spp <= 2 * 256 * 4 = 2048 (analysis_rms: GEO_SPP)

// Sums of v... over the workgroup in a fixed order: wave butterfly, lane 0 of each wave to red[wave * n + i], then thread 0 adds waves
// 0..3 in order and runs then(totals...); it alone gets the totals back, the other threads their wave's sums.  red is free again after
// the caller's next barrier.  (Values in, values out, thread 0's work in one block: taking the sums by reference, or a second
// `if (tid == 0)` behind the call, compiles both kernels to other code than the text written out in place.)
template <int N> struct BlockSums { float v[N]; };
template <class Then, class... F>
__device__ __forceinline__ BlockSums<sizeof...(F)> block_sums(float* red, int tid, Then then, F... v) {
    constexpr int n = sizeof...(F);
    ((v = wave_sum(v)), ...);
    if ((tid & 63) == 0) { int i = 0; ((red[(tid >> 6) * n + i++] = v), ...); }
    __syncthreads();
    if (tid == 0) {
        ((v = 0.f), ...);
        for (int w = 0; w < kSpotWaves; ++w) { int i = 0; ((v += red[n * w + i++]), ...); }
        then(v...);
    }
    return {{v...}};
}
// ------------------------------------------------------------------------------------
// Spot moments of the ray-traced lens analysis: stratified pupil samples (deeplens/optics.py:539-591) from an object
// point grid (sample_point_source :400-454), traced and projected to d_sensor, reduced per field point - the rays are never
// stored.  One workgroup per field point runs every pass (wavelength) of that point in order, so pass 0's centroid stays in
// LDS as the green reference of analysis_rms (:1975-2012); each lane keeps its hits in registers for the second phase.
// Reductions run in a fixed order (wave butterfly, then waves 0..3), so a launch is bit-reproducible.
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(kSpotThreads) void spot_moments_kernel(const float* __restrict__ points, int P, const float* __restrict__ u,
                                                                    int spp, int num_angle, int n_pass,
                                                                    const aadff_surface_t* __restrict__ surf, int n_surf, float pupil_z,
                                                                    float r2_step, const aadff_lens_state_t* __restrict__ state, int ref_mode,
                                                                    int want_s2, float4* __restrict__ moments, int* flags) {
    __shared__ float red[3 * kSpotWaves];
    __shared__ float centre[2];
    const int p = blockIdx.x, tid = threadIdx.x;
    const float d_sensor = fresh_uniform(&state->d_sensor);
    const float px = points[3 * p], py = points[3 * p + 1], pz = points[3 * p + 2];
    const int rings = spp / num_angle;
    const float inv_a = 1.f / (float)num_angle;
    const int n_iter = (spp + 2 * kSpotThreads - 1) / (2 * kSpotThreads);
    int nan_flag = 0;
    for (int q = 0; q < n_pass; ++q) {
        const float* uq = u + (size_t)q * 2 * spp * P;
        const aadff_surface_t* tab = surf + (size_t)q * n_surf;
        f2 hx[kSpotMaxPairs], hy[kSpotMaxPairs];
        i2 ok[kSpotMaxPairs];
#pragma unroll
        for (int k = 0; k < kSpotMaxPairs; ++k) { hx[k] = hy[k] = f2s(0.f); ok[k] = (i2){0, 0}; }
        float sx = 0.f, sy = 0.f, sn = 0.f;
#pragma unroll 1
        for (int k = 0; k < n_iter; ++k) {
            const int s0 = tid + k * 2 * kSpotThreads;
            if (s0 >= spp) break;
            const int s1 = s0 + kSpotThreads;
            const i2 act = {-1, s1 < spp ? -1 : 0};
            const int sb = act.y ? s1 : s0;
            // sample s = i * (spp / A) + j: sector i, ring j; theta block then r^2 block of P draws each (optics.py:571-582)
            const int i0 = s0 / rings, ib = sb / rings;
            const f2 ut = {uq[(size_t)(2 * s0) * P + p], uq[(size_t)(2 * sb) * P + p]};
            const f2 ur = {uq[(size_t)(2 * s0 + 1) * P + p], uq[(size_t)(2 * sb + 1) * P + p]};
            const f2 rev = (ut + (f2){(float)i0, (float)ib}) * inv_a;                       // theta / (2 pi)
            const f2 rr = vsqrt((ur + (f2){(float)(s0 - i0 * rings), (float)(sb - ib * rings)}) * r2_step);
            const f2 x2 = rr * (f2){__builtin_amdgcn_cosf(rev.x), __builtin_amdgcn_cosf(rev.y)};
            const f2 y2 = rr * (f2){__builtin_amdgcn_sinf(rev.x), __builtin_amdgcn_sinf(rev.y)};
            const Ray2 r = trace_pair_to_sensor(px, py, pz, x2, y2, pupil_z, act, tab, n_surf, d_sensor, nan_flag);
            const f2 wx = vsel(r.alive, r.ox, f2s(0.f)), wy = vsel(r.alive, r.oy, f2s(0.f));
            sx += wx.x + wx.y; sy += wy.x + wy.y;
            sn += (r.alive.x ? 1.f : 0.f) + (r.alive.y ? 1.f : 0.f);
#pragma unroll
            for (int kk = 0; kk < kSpotMaxPairs; ++kk)       // constant register indices (a runtime index would spill to scratch)
                if (kk == k) { hx[kk] = wx; hy[kk] = wy; ok[kk] = r.alive; }
        }
        {
            const auto t = block_sums(red, tid, [=](float x, float y, float n) {
                if (!ref_mode || q == 0) {           // optics.py:1987,1997: the centroid divides by count + 0.0001
                    centre[0] = x / (n + 1e-4f);
                    centre[1] = y / (n + 1e-4f);
                }
            }, sx, sy, sn);
            sx = t.v[0]; sy = t.v[1]; sn = t.v[2];
        }
        __syncthreads();
        float s2 = 0.f;
        if (want_s2) {
            // wave-uniform, so in SGPRs: a VGPR pair {cx, cy} would make the compiler read cy through op_sel from its high half
            // (the packed form tools/check_isa.py refuses)
            const float cx = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, centre[0])));
            const float cy = __builtin_bit_cast(float, __builtin_amdgcn_readfirstlane(__builtin_bit_cast(int, centre[1])));
#pragma unroll
            for (int k = 0; k < kSpotMaxPairs; ++k) {
                const f2 dx = hx[k] - cx, dy = hy[k] - cy;
                const f2 e = vsel(ok[k], dx * dx + dy * dy, f2s(0.f));
                s2 += e.x + e.y;
            }
            s2 = block_sums(red, tid, [](float) {}, s2).v[0];
        }
        if (tid == 0) moments[(size_t)q * P + p] = make_float4(sn, sx, sy, s2);
        __syncthreads();                          // red / centre are rewritten by the next pass
    }
    if (nan_flag && flags) atomicOr(flags, 1);    // found nan in ft in non-diff newton method (surfaces.py:555-558)
}

// ------------------------------------------------------------------------------------
// Ray-traced MTF: the geometric OTF as the Fourier transform of the traced hits themselves - no histogram, no
// window.  Phase 1 is spot_moments_kernel's (same draws, same pupil points, same trace, same order of sums: block_sums), except that every
// ray's hit (x, y) at d_sensor, its slopes (a, b) = (dx/dz, dy/dz) behind the last surface and its validity stay in LDS.  Behind
// the lens a ray is a straight line, so on the plane d_sensor + delta it lands at (x + a delta, y + b delta): a sensor plane costs
// one multiply-add per coordinate.  Between the phases the valid rays are moved to the front of the LDS array in index order
// (a prefix count over the validity words) with the pass's means subtracted: the phase is formed from the small centred
// coordinates.  Phase 2: one lane owns one output entry (delta, axis, nu), walks those rays in order (every lane reads the same
// LDS address: a broadcast; a counted loop, so the reads of the next rays are in flight while this one is used) and adds cos /
// sin of 2 pi nu e.(h - c) into its own two registers.  No cross-lane sum in phase 2, no atomics, every output written once: a
// launch is bit-reproducible.
// ------------------------------------------------------------------------------------
constexpr int kMtfMaxSpp = 2 * kSpotThreads * kSpotMaxPairs;      // 2048 rays x 16 B = 32 KB of LDS
constexpr int kMtfMaxF = 128, kMtfMaxZ = 16;
struct MtfGrid { float freq[kMtfMaxF]; float defocus[kMtfMaxZ]; };  // copied into the kernel arguments by the call

__global__ __launch_bounds__(kSpotThreads) void mtf_points_kernel(const float* __restrict__ points, int P, const float* __restrict__ u,
                                                                  int spp, int num_angle, int n_pass,
                                                                  const aadff_surface_t* __restrict__ surf, int n_surf, float pupil_z,
                                                                  float r2_step, const aadff_lens_state_t* __restrict__ state,
                                                                  const MtfGrid grid, int F, int Z, int axes_mode,
                                                                  float2* __restrict__ otf, float* __restrict__ moments, int* flags) {
    __shared__ float4 hit[kMtfMaxSpp];                     // (x, y, a, b) of ray s; before phase 2 the valid ones, centred, in index order
    __shared__ unsigned alive_bits[kMtfMaxSpp / 32];       // bit s % 32 of word s / 32: ray s is valid
    __shared__ unsigned short before[kMtfMaxSpp / 32];     // valid rays in the words before word w
    __shared__ int n_alive;
    __shared__ float red[5 * kSpotWaves];
    __shared__ float mean[5];                              // x, y, a, b means and the valid count
    const int p = blockIdx.x, tid = threadIdx.x;
    const float d_sensor = fresh_uniform(&state->d_sensor);
    const float px = points[3 * p], py = points[3 * p + 1], pz = points[3 * p + 2];
    // tangential axis: the direction of the object point itself, an input (a computed centroid's direction is noise near the axis)
    float tx = 1.f, ty = 0.f;
    if (axes_mode == 0 && (px != 0.f || py != 0.f)) {
        const float h = sqrtf(px * px + py * py);
        tx = px / h; ty = py / h;
    }
    const int rings = spp / num_angle;
    const float inv_a = 1.f / (float)num_angle;
    const int n_iter = (spp + 2 * kSpotThreads - 1) / (2 * kSpotThreads);
    const int E = Z * 2 * F;
    int nan_flag = 0;
    for (int q = 0; q < n_pass; ++q) {
        const float* uq = u + (size_t)q * 2 * spp * P;
        const aadff_surface_t* tab = surf + (size_t)q * n_surf;
        float sx = 0.f, sy = 0.f, sa = 0.f, sb = 0.f, sn = 0.f;
#pragma unroll 1
        for (int k = 0; k < n_iter; ++k) {
            const int s0 = tid + k * 2 * kSpotThreads;
            if (s0 >= spp) break;
            const int s1 = s0 + kSpotThreads;
            const i2 act = {-1, s1 < spp ? -1 : 0};
            const int sb_ = act.y ? s1 : s0;
            const int i0 = s0 / rings, ib = sb_ / rings;
            const f2 ut = {uq[(size_t)(2 * s0) * P + p], uq[(size_t)(2 * sb_) * P + p]};
            const f2 ur = {uq[(size_t)(2 * s0 + 1) * P + p], uq[(size_t)(2 * sb_ + 1) * P + p]};
            const f2 rev = (ut + (f2){(float)i0, (float)ib}) * inv_a;                       // theta / (2 pi)
            const f2 rr = vsqrt((ur + (f2){(float)(s0 - i0 * rings), (float)(sb_ - ib * rings)}) * r2_step);
            const f2 x2 = rr * (f2){__builtin_amdgcn_cosf(rev.x), __builtin_amdgcn_cosf(rev.y)};
            const f2 y2 = rr * (f2){__builtin_amdgcn_sinf(rev.x), __builtin_amdgcn_sinf(rev.y)};
            const Ray2 r = trace_pair_to_sensor(px, py, pz, x2, y2, pupil_z, act, tab, n_surf, d_sensor, nan_flag);
            const f2 iz = vrcp(r.dz);
            const f2 wx = vsel(r.alive, r.ox, f2s(0.f)), wy = vsel(r.alive, r.oy, f2s(0.f));
            const f2 wa = vsel(r.alive, r.dx * iz, f2s(0.f)), wb = vsel(r.alive, r.dy * iz, f2s(0.f));
            sx += wx.x + wx.y; sy += wy.x + wy.y;
            sa += wa.x + wa.y; sb += wb.x + wb.y;
            sn += (r.alive.x ? 1.f : 0.f) + (r.alive.y ? 1.f : 0.f);
            hit[s0] = make_float4(wx.x, wy.x, wa.x, wb.x);
            if (act.y) hit[s1] = make_float4(wx.y, wy.y, wa.y, wb.y);
            // a wave's 64 first rays (and its 64 second rays) are consecutive and start at a multiple of 64: two words each.  Lane 0
            // of a wave has the wave's smallest s0, so it is here whenever any lane of the wave is.
            const unsigned long long b0 = __ballot(r.alive.x != 0), b1 = __ballot(r.alive.y != 0);
            if ((tid & 63) == 0) {
                alive_bits[s0 >> 5] = (unsigned)b0; alive_bits[(s0 >> 5) + 1] = (unsigned)(b0 >> 32);
                alive_bits[s1 >> 5] = (unsigned)b1; alive_bits[(s1 >> 5) + 1] = (unsigned)(b1 >> 32);
            }
        }
        block_sums(red, tid, [=](float sx, float sy, float sa, float sb, float sn) {
            float* m = moments + ((size_t)q * P + p) * 8;
            m[0] = sn; m[1] = sx; m[2] = sy; m[3] = sa; m[4] = sb; m[5] = 0.f; m[6] = 0.f; m[7] = 0.f;
            const float den = sn > 0.f ? sn : 1.f;          // plain means: no + 1e-4 (this is not analysis_rms's centroid)
            mean[0] = sx / den; mean[1] = sy / den; mean[2] = sa / den; mean[3] = sb / den; mean[4] = sn;
        }, sx, sy, sa, sb, sn);
        if (tid < 64) {                           // valid rays before word tid: an inclusive scan over wave 0, less the word's own
            const unsigned c = tid < (spp + 31) / 32 ? __popc(alive_bits[tid]) : 0u;
            unsigned incl = c;
            for (int d = 1; d < 64; d <<= 1) {
                const unsigned v = __shfl_up(incl, d);
                if (tid >= d) incl += v;
            }
            before[tid] = (unsigned short)(incl - c);
            if (tid == 63) n_alive = (int)incl;
        }
        __syncthreads();
        const float n_valid = mean[4];
        const int n_rays = __builtin_amdgcn_readfirstlane(n_alive);
        {
            // the valid rays move to the front in index order, centred: phase 2 then runs a counted loop over 0 .. n - 1
            const float mx = mean[0], my = mean[1], ma = mean[2], mb = mean[3];
            float4 keep[2 * kSpotMaxPairs];
            int dest[2 * kSpotMaxPairs];
#pragma unroll
            for (int i = 0; i < 2 * kSpotMaxPairs; ++i) {                  // constant register indices
                const int s = tid + i * kSpotThreads;
                dest[i] = -1;
                keep[i] = make_float4(0.f, 0.f, 0.f, 0.f);
                if (s < spp) {
                    const unsigned w = alive_bits[s >> 5], bit = 1u << (s & 31);
                    if (w & bit) {
                        const float4 h = hit[s];
                        keep[i] = make_float4(h.x - mx, h.y - my, h.z - ma, h.w - mb);
                        dest[i] = (int)before[s >> 5] + __popc(w & (bit - 1u));
                    }
                }
            }
            __syncthreads();
#pragma unroll
            for (int i = 0; i < 2 * kSpotMaxPairs; ++i)
                if (dest[i] >= 0) hit[dest[i]] = keep[i];
        }
        __syncthreads();
        // phase 2: entry e = (z * 2 + axis) * F + f; every lane runs every trip (the ray loop is wave-uniform), the store is masked
        for (int base = 0; base < E; base += kSpotThreads) {
            if (base + (tid & ~63) >= E) continue;                         // a wave without an entry leaves its SIMD to the others
            const int e = min(base + tid, E - 1);
            const int za = e / F, f = e - za * F, axis = za & 1, z = za >> 1;
            const float nu = grid.freq[f], dl = grid.defocus[z];
            const float ex = axis ? -ty : tx, ey = axis ? tx : ty;     // e_T, or e_S = (-e_T.y, e_T.x)
            float re = 0.f, im = 0.f;
#pragma unroll 4
            for (int k = 0; k < n_rays; ++k) {
                const float4 h = hit[k];
                const float t = ex * (h.x + h.z * dl) + ey * (h.y + h.w * dl);         // e . (h(delta) - c(delta)), mm
                const float rv = __builtin_amdgcn_fractf(nu * t);                       // revolutions, reduced to [0, 1)
                re += __builtin_amdgcn_cosf(rv);
                im -= __builtin_amdgcn_sinf(rv);                                        // exp(-2 pi i nu t)
            }
            if (base + tid < E) {
                const bool any = n_valid > 0.f;
                otf[((size_t)q * P + p) * E + e] = make_float2(any ? re / n_valid : 0.f, any ? im / n_valid : 0.f);
            }
        }
        __syncthreads();                          // hit / alive_bits / before / red / mean are rewritten by the next pass
    }
    if (nan_flag && flags) atomicOr(flags, 1);    // found nan in ft in non-diff newton method (surfaces.py:555-558)
}

}  // namespace aadff

using namespace aadff;

extern "C" {

int aadff_spot_moments(const float* points, int P, const float* u, int spp, int num_angle, int n_pass, const aadff_surface_t* surf,
                       int n_surf, float pupil_z, float pupil_r, const aadff_lens_state_t* state, int ref_mode, int want_s2,
                       float* moments, int* flags_or_null, aadff_stream_t stream) {
    AADFF_CHECK_ARG(points && u && surf && state && moments, "spot_moments: NULL pointer");
    AADFF_CHECK_ARG(P > 0 && P <= (1 << 20) && n_pass > 0 && n_pass <= 16, "spot_moments: bad sizes P=%d n_pass=%d", P, n_pass);
    AADFF_CHECK_ARG(n_surf > 0 && n_surf <= AADFF_MAX_SURF, "spot_moments: n_surf %d outside [1,%d]", n_surf, AADFF_MAX_SURF);
    AADFF_CHECK_ARG(num_angle > 0 && spp > 0 && spp % num_angle == 0 && spp <= 2 * kSpotThreads * kSpotMaxPairs,
                    "spot_moments: spp=%d must be a positive multiple of num_angle=%d and at most %d (stratified pupil samples only)",
                    spp, num_angle, 2 * kSpotThreads * kSpotMaxPairs);
    AADFF_CHECK_ARG(ref_mode == 0 || ref_mode == 1, "spot_moments: ref_mode %d is 0 or 1", ref_mode);
    AADFF_CHECK_ARG(std::isfinite(pupil_z) && std::isfinite(pupil_r) && pupil_r >= 0.f, "spot_moments: bad pupil (z=%g, r=%g)",
                    (double)pupil_z, (double)pupil_r);
    hipLaunchKernelGGL(spot_moments_kernel, dim3(P), dim3(kSpotThreads), 0, (hipStream_t)stream, points, P, u, spp, num_angle, n_pass,
                       surf, n_surf, pupil_z, r2_step(pupil_r, spp, num_angle), state, ref_mode, want_s2, reinterpret_cast<float4*>(moments), flags_or_null);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_mtf_points(const float* points, int P, const float* u, int spp, int num_angle, int n_pass, const aadff_surface_t* surf,
                     int n_surf, float pupil_z, float pupil_r, const aadff_lens_state_t* state, const float* freqs, int F,
                     const float* defocus, int Z, int axes_mode, float* otf, float* moments, int* flags_or_null, aadff_stream_t stream) {
    AADFF_CHECK_ARG(points && u && surf && state && freqs && defocus && otf && moments, "mtf_points: NULL pointer");
    AADFF_CHECK_ARG(P > 0 && P <= (1 << 20) && n_pass > 0 && n_pass <= 16, "mtf_points: bad sizes P=%d n_pass=%d", P, n_pass);
    AADFF_CHECK_ARG(n_surf > 0 && n_surf <= AADFF_MAX_SURF, "mtf_points: n_surf %d outside [1,%d]", n_surf, AADFF_MAX_SURF);
    AADFF_CHECK_ARG(num_angle > 0 && spp > 0 && spp % num_angle == 0 && spp <= kMtfMaxSpp,
                    "mtf_points: spp=%d must be a positive multiple of num_angle=%d and at most %d (stratified pupil samples, kept in LDS)",
                    spp, num_angle, kMtfMaxSpp);
    AADFF_CHECK_ARG(F >= 1 && F <= kMtfMaxF, "mtf_points: F=%d frequencies outside [1,%d]", F, kMtfMaxF);
    AADFF_CHECK_ARG(Z >= 1 && Z <= kMtfMaxZ, "mtf_points: Z=%d sensor planes outside [1,%d]", Z, kMtfMaxZ);
    AADFF_CHECK_ARG(axes_mode == 0 || axes_mode == 1, "mtf_points: axes_mode %d is 0 (radial) or 1 (xy)", axes_mode);
    AADFF_CHECK_ARG(std::isfinite(pupil_z) && std::isfinite(pupil_r) && pupil_r >= 0.f, "mtf_points: bad pupil (z=%g, r=%g)",
                    (double)pupil_z, (double)pupil_r);
    MtfGrid grid = {};
    for (int f = 0; f < F; ++f) {
        AADFF_CHECK_ARG(std::isfinite(freqs[f]) && freqs[f] >= 0.f, "mtf_points: frequency %d = %g is not finite and >= 0", f, (double)freqs[f]);
        grid.freq[f] = freqs[f];
    }
    for (int z = 0; z < Z; ++z) {
        AADFF_CHECK_ARG(std::isfinite(defocus[z]), "mtf_points: defocus %d = %g is not finite", z, (double)defocus[z]);
        grid.defocus[z] = defocus[z];
    }
    hipLaunchKernelGGL(mtf_points_kernel, dim3(P), dim3(kSpotThreads), 0, (hipStream_t)stream, points, P, u, spp, num_angle, n_pass,
                       surf, n_surf, pupil_z, r2_step(pupil_r, spp, num_angle), state, grid, F, Z, axes_mode, reinterpret_cast<float2*>(otf), moments,
                       flags_or_null);
    AADFF_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
