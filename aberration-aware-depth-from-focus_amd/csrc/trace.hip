// The PSF grid and what feeds it, for gfx950: the chief-centre fit, the bulk trace kernels, the splat, the fused PSF-grid kernel family and
// refocus, with their C entries.  The ray trace itself: trace_core.h; spot moments and MTF: lens_analysis.hip; rendering: render_rt.hip.
#include <algorithm>
#include <cmath>
#include <cstdint>
#include <cstdlib>
#include <cstring>
#include <hip/hip_ext.h>
#include "trace_core.h"
#include "chief_fit_tables.h"

namespace aadff {

// ------------------------------------------------------------------------------------
// Chief-centre fit.  The chief centre of a field point is the mean, over the spp_chief drawn points of the shrunk
// pupil, of the sensor hit - a smooth function of the pupil position, i.e. a low-order polynomial where no ray is vignetted.  The
// mean of a polynomial over the draws is sum_k w_k p(node_k) for fixed nodes, with w = pinv(V)^T m and m the monomial moments of
// THIS draw: the sample mean of the same uniforms, not the continuous pupil integral.  The draw is shared by every field point of a
// (state, wavelength), so the weights are computed once per (state, wavelength): chief_fit_weights_kernel, float64, one workgroup
// each.  Nodes and pinv(V)^T are constants (chief_fit_tables.h, tools/gen_chief_fit_tables.py); two weight vectors, degree d and
// d - 2 over the same nodes, feed the truncation guard of the PSF kernel.
// ------------------------------------------------------------------------------------
constexpr int kChiefNodes = AADFF_CHIEF_NODES, kChiefRays = AADFF_CHIEF_RAYS;
constexpr int kFitMono = AADFF_CHIEF_FIT_MONOMIALS, kFitMonoLow = AADFF_CHIEF_FIT_MONOMIALS_LOW, kFitDegree = AADFF_CHIEF_DEGREE;
constexpr int kFitThreads = 512, kFitBatch = 4, kFitSplit = kFitThreads / kChiefNodes, kFitPiece = (kFitMono + kFitSplit - 1) / kFitSplit;
constexpr int kFitChunk = kFitThreads / 64;
static_assert(kChiefRays == 128 && kChiefNodes <= kChiefRays && kChiefNodes >= 64, "one wave of 64 lanes x 2 rays; every lane's first ray is a node");
static_assert(kFitMono == (kFitDegree + 1) * (kFitDegree + 2) / 2 && kFitMonoLow == (kFitDegree - 1) * kFitDegree / 2, "monomials by total degree");
static_assert(kFitMono <= kFitThreads && 2 * kChiefNodes <= kFitThreads, "chief_fit_weights_kernel: one thread per moment / per weight");
static_assert(kFitBatch % 2 == 0, "chief_fit_weights_kernel<true>: the draws of a batch go through disc_sample2 in pairs");
static const double h_chief_node_xy[kChiefRays * 2] = AADFF_CHIEF_NODE_XY_INIT;
static const double h_chief_fit[kFitMono * kChiefNodes] = AADFF_CHIEF_FIT_INIT;
static const double h_chief_fit_low[kFitMonoLow * kChiefNodes] = AADFF_CHIEF_FIT_LOW_INIT;
__device__ const float d_chief_node_xy[kChiefRays * 2] = AADFF_CHIEF_NODE_XY_INIT;
__device__ const double d_chief_fit[kFitMono * kChiefNodes] = AADFF_CHIEF_FIT_INIT;
__device__ const double d_chief_fit_low[kFitMonoLow * kChiefNodes] = AADFF_CHIEF_FIT_LOW_INIT;
// A fitted centre is taken only where the degree-d and degree-(d - 2) centres agree within this (mm, either axis).  Among the
// workgroups of the bench configuration whose node and ring rays are all alive the difference is float32 trace noise, 1.2e-7 mm in the
// median and 2.1e-6 mm at most; 1.3 % of them exceed the tolerance and trace every draw
constexpr float kChiefFitTol = AADFF_CHIEF_FIT_TOL;

// The pupil points of a launch with points (PTS, aadff_chief_fit_prologue): the draws of a (state, wavelength) are mapped to the pupil
// here, once, by disc_sample2 itself, and not again by each of the N point workgroups of the PSF launch.  pupil_xy
// [S][L] blocks of {main x [spp], main y [spp], chief x [spp_chief], chief y [spp_chief]}: the block of raw draws with every theta
// row replaced by x and every r row by y, so the PSF kernel reads it through the pointers and strides it reads draws through.
struct PupilArgs {
    const float* u_main;      // raw main draws, as the PSF launch gets them; u_main_late: their address in the mapped pinned block
    const float* u_main_late;
    long main_ss, main_sl;
    int spp;
    float enp_r2, enp_r2_shrunk;
    float* xy;
};
// grid (L, S), with PTS (L, S, 2): z = 0 the chief draws, their points and the weights, z = 1 the points of the main draws; u_late:
// the address u_chief has in the mapped pinned block for states >= late_from (staged launches), else unused
template <bool PTS>
__global__ __launch_bounds__(kFitThreads) void chief_fit_weights_kernel(const float* __restrict__ u_chief, const float* __restrict__ u_late, int late_from,
                                                                         int L, int spp_chief, long chief_ss, long chief_sl, float* __restrict__ weights,
                                                                         PupilArgs pa) {
    __shared__ double buf[kFitChunk][kFitThreads];
    __shared__ double mom[kFitMono];
    __shared__ double wsum[kFitSplit][2][kChiefNodes];
    const int l = blockIdx.x, s = blockIdx.y, tid = threadIdx.x;
    const float* ut = (s >= late_from ? u_late : u_chief) + (size_t)s * chief_ss + (size_t)l * chief_sl;
    const float* ur = ut + spp_chief;
    [[maybe_unused]] float* const pxy = PTS ? pa.xy + (size_t)(s * L + l) * (2 * (size_t)pa.spp + 2 * (size_t)spp_chief) : nullptr;
    if constexpr (PTS) if (blockIdx.z == 1) {
        // a workgroup of its own for the main draws, beside the one with the chief draws: the late states' draws come over PCIe, and one
        // workgroup that waits for both, one after the other, took 28 us where the weights alone take 19.
        // Two draws at a time through disc_sample2, as the PSF kernel took them; the same batches of loads as below
        const float* mt = (s >= late_from ? pa.u_main_late : pa.u_main) + (size_t)s * pa.main_ss + (size_t)l * pa.main_sl;
        const float* mr = mt + pa.spp;
        for (int i0 = tid; i0 < pa.spp; i0 += kFitBatch * kFitThreads) {
            float ua[kFitBatch], ub[kFitBatch];
#pragma unroll
            for (int q = 0; q < kFitBatch; ++q) {
                const int i = min(i0 + q * kFitThreads, pa.spp - 1);
                ua[q] = mt[i]; ub[q] = mr[i];
            }
#pragma unroll
            for (int q = 0; q < kFitBatch; q += 2) {
                const int ia = i0 + q * kFitThreads, ib = ia + kFitThreads;
                f2 x2, y2;
                disc_sample2((f2){ua[q], ua[q + 1]}, (f2){ub[q], ub[q + 1]}, pa.enp_r2, x2, y2);
                if (ia < pa.spp) { pxy[ia] = x2.x; pxy[pa.spp + ia] = y2.x; }
                if (ib < pa.spp) { pxy[ib] = x2.y; pxy[pa.spp + ib] = y2.y; }
            }
        }
        return;                                          // whole workgroups
    }
    double acc[kFitMono];
#pragma unroll
    for (int j = 0; j < kFitMono; ++j) acc[j] = 0.0;
    for (int i0 = tid; i0 < spp_chief; i0 += kFitBatch * kFitThreads) {
        float ua[kFitBatch], ub[kFitBatch];              // a batch of loads in flight at once: the draws of a staged launch come over PCIe
#pragma unroll
        for (int q = 0; q < kFitBatch; ++q) {
            const int i = min(i0 + q * kFitThreads, spp_chief - 1);
            ua[q] = ut[i]; ub[q] = ur[i];
        }
        if constexpr (PTS) {
            float* const cxy = pxy + 2 * (size_t)pa.spp;
#pragma unroll
            for (int q = 0; q < kFitBatch; q += 2) {
                const int ia = i0 + q * kFitThreads, ib = ia + kFitThreads;
                f2 x2, y2;
                disc_sample2((f2){ua[q], ua[q + 1]}, (f2){ub[q], ub[q + 1]}, pa.enp_r2_shrunk, x2, y2);
                if (ia < spp_chief) { cxy[ia] = x2.x; cxy[spp_chief + ia] = y2.x; }
                if (ib < spp_chief) { cxy[ib] = x2.y; cxy[spp_chief + ib] = y2.y; }
            }
        }
#pragma unroll
        for (int q = 0; q < kFitBatch; ++q) {
            if (i0 + q * kFitThreads >= spp_chief) break;
            // the unit-disc point of disc_sample2 (same square root, same sine and cosine), without the pupil radius
            const float rr = fsqrt(ub[q]), ang = ua[q];
#ifndef AADFF_LIBM_SINCOS
            const double x = (double)(rr * __builtin_amdgcn_cosf(ang)), y = (double)(rr * __builtin_amdgcn_sinf(ang));
#else
            const double x = (double)(rr * cosf(ang * 2.f * kTwoPiHi)), y = (double)(rr * sinf(ang * 2.f * kTwoPiHi));
#endif
            double px[kFitDegree + 1], py[kFitDegree + 1];
            px[0] = py[0] = 1.0;
#pragma unroll
            for (int k = 1; k <= kFitDegree; ++k) { px[k] = px[k - 1] * x; py[k] = py[k - 1] * y; }
            int j = 0;
#pragma unroll
            for (int d = 0; d <= kFitDegree; ++d)
#pragma unroll
                for (int b = 0; b <= d; ++b) acc[j++] += px[d - b] * py[b];
        }
    }
    // sums over the threads, kFitChunk moments at a time through LDS: a wave per moment adds the waves' partial sums lane by lane
    // and finishes with one shuffle tree (a shuffle tree per moment and wave is 66 x 6 LDS permutes of doubles, one after the other)
#pragma unroll
    for (int c = 0; c < kFitMono; c += kFitChunk) {
#pragma unroll
        for (int q = 0; q < kFitChunk; ++q)
            if (c + q < kFitMono) buf[q][tid] = acc[c + q];
        __syncthreads();
        const int m = tid >> 6, sub = tid & 63;
        double v = 0.0;
#pragma unroll
        for (int e = 0; e < kFitThreads / 64; ++e) v += buf[m][sub + 64 * e];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) v += __shfl_xor(v, off, kWave);
        if (sub == 0 && c + m < kFitMono) mom[c + m] = v / (double)spp_chief;
        __syncthreads();
    }
    // w = pinv(V)^T m: the rows of a node split over kFitSplit threads (a thread alone waits for 111 loads one after the other)
    const int k = tid % kChiefNodes, piece = tid / kChiefNodes;
    if (piece < kFitSplit) {
        double w = 0.0, wl = 0.0;
#pragma unroll
        for (int q = 0; q < kFitPiece; ++q) {
            const int j = piece * kFitPiece + q;
            if (j < kFitMono) w += d_chief_fit[j * kChiefNodes + k] * mom[j];
            if (j < kFitMonoLow) wl += d_chief_fit_low[j * kChiefNodes + k] * mom[j];
        }
        wsum[piece][0][k] = w; wsum[piece][1][k] = wl;
    }
    __syncthreads();
    if (tid < 2 * kChiefNodes) {
        const int which = tid / kChiefNodes;
        double w = 0.0;
#pragma unroll
        for (int q = 0; q < kFitSplit; ++q) w += wsum[q][which][k];
        weights[(size_t)(s * L + l) * 2 * kChiefNodes + tid] = (float)w;
    }
}

// ------------------------------------------------------------------------------------
// generic kernels
// ------------------------------------------------------------------------------------
__global__ __launch_bounds__(256) void trace_rays_kernel(const float* o_in, const float* d_in, const float* ra_in,
                                                          float* o_out, float* d_out, float* ra_out, int n,
                                                          const aadff_surface_t* __restrict__ surf, int first, int last,
                                                          int forward, const aadff_lens_state_t* __restrict__ state,
                                                          int* flags) {
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    Ray r;
    r.ox = o_in[3 * i]; r.oy = o_in[3 * i + 1]; r.oz = o_in[3 * i + 2];
    r.dx = d_in[3 * i]; r.dy = d_in[3 * i + 1]; r.dz = d_in[3 * i + 2];
    r.ra = ra_in ? ra_in[i] : 1.f;
    int nan_flag = 0;
    trace_range<true>(surf, first, last, forward != 0, r, nan_flag);
    if (state) propagate_to(r, state->d_sensor);
    o_out[3 * i] = r.ox; o_out[3 * i + 1] = r.oy; o_out[3 * i + 2] = r.oz;
    d_out[3 * i] = r.dx; d_out[3 * i + 1] = r.dy; d_out[3 * i + 2] = r.dz;
    ra_out[i] = r.ra;
    if (nan_flag && flags) atomicOr(flags, 1);
}

__global__ __launch_bounds__(256) void trace_points_kernel(const float* __restrict__ pts, int N,
                                                            const float* __restrict__ u_theta,
                                                            const float* __restrict__ u_r, int spp, float pupil_z,
                                                            float pupil_r2, const aadff_surface_t* __restrict__ surf,
                                                            int n_surf, const aadff_lens_state_t* __restrict__ state,
                                                            float* o_out, float* d_out, float* ra_out) {
    // x: sample (fastest across the wave so a wave shares one object point), y: point
    const int i = blockIdx.x * blockDim.x + threadIdx.x;
    const int n = blockIdx.y;
    if (i >= spp) return;
    float x2, y2;
    disc_sample(u_theta[i], u_r[i], pupil_r2, x2, y2);
    Ray r = ray_to(pts[3 * n], pts[3 * n + 1], pts[3 * n + 2], x2, y2, pupil_z);
    int nan_flag = 0;
    trace_range<true>(surf, 0, n_surf, true, r, nan_flag);
    propagate_to(r, state->d_sensor);
    const size_t e = (size_t)i * N + n;
    o_out[3 * e] = r.ox; o_out[3 * e + 1] = r.oy; o_out[3 * e + 2] = r.oz;
    d_out[3 * e] = r.dx; d_out[3 * e + 1] = r.dy; d_out[3 * e + 2] = r.dz;
    ra_out[e] = r.ra;
}

// ------------------------------------------------------------------------------------
// PSF histogram: deeplens/monte_carlo.py:9-121
// ------------------------------------------------------------------------------------
struct SplatGeom {
    float lo, hi, lim, scale, half;        // all float64 -> fp32 once
    int ks;
};

// Bin coordinates of monte_carlo.py:86-92, (Y - hi) / (lo - hi) (ks - 1) and (X - lo) / (hi - lo) (ks - 1), are, with -lo = hi,
// -Y scale + half and X scale + half: scale = (ks - 1) / (hi - lo) pixels per mm, half = (ks - 1) / 2 (a float: the centre's coordinate)
__host__ __device__ inline SplatGeom make_splat_geom(float pixel_size, int ks) {
    const double ps = (double)pixel_size;
    const double lo = (-ks / 2.0 + 0.5) * ps, hi = (ks / 2.0 - 0.5) * ps;
    SplatGeom g;
    g.lo = (float)lo; g.hi = (float)hi;
    g.lim = (float)(hi - 0.01 * ps);
    g.scale = (float)((ks - 1) / (hi - lo));           // ks = 1: never read, the window (lim < 0) holds no hit
    g.half = (float)((ks - 1) / 2.0);
    g.ks = ks;
    return g;
}

// hit (ox,oy) on the sensor -> 4 bilinear taps into hist[ks*ks] (LDS), weight ra
// WEIGHTED: ra may be any weight, and the reference scales the centred hit by it as well (`points_shift *= ra`, monte_carlo.py:38)
// before it bins it.  The traces of this file hand over 0 or 1, for which that product is the identity: only aadff_psf_splat, whose
// caller supplies ra, asks for it.
template <bool WEIGHTED = false>
__device__ __forceinline__ void splat_hit(float* hist, const SplatGeom& g, float ox, float oy, float ra, float cx, float cy) {
    float X = -ox - cx, Y = -oy - cy;                 // image flip, then centre
    const bool in = (fabsf(X) < g.lim) && (fabsf(Y) < g.lim) && (ra > 0.f);
    if (!in) return;                                   // zero-weight taps at the centre bin are skipped
    if constexpr (WEIGHTED) {
        X *= ra; Y *= ra;
        if (!(fabsf(X) < g.lim && fabsf(Y) < g.lim)) return;   // a weight above 1 can carry the hit past the grid, where the reference stops with an index error
    }
    // One fma per coordinate, and exact where it has to be: a hit on the centre (X = 0) is at `half`.  The quotient hi / (2 hi) of the
    // reference's form came out of a bare reciprocal as 0.49999997; at ks = 3 that is column 0.99999994, and the reference's
    // floor(f + 1), kept below, rounds 1.99999994 up to 2 - the whole weight of the ray in column 2 where the reference, dividing
    // exactly, has it in column 1.
    const float rowf = fmaf(-Y, g.scale, g.half);
    const float colf = fmaf(X, g.scale, g.half);
    const float fr = floorf(rowf), fc = floorf(colf);
    const float wb = rowf - fr, wr = colf - fc;
    const int r0 = (int)fr, c0 = (int)fc;
    const int r1 = (int)floorf(rowf + 1.f), c1 = (int)floorf(colf + 1.f);
    const int ks = g.ks;
    atomicAdd(&hist[r0 * ks + c0], (1.f - wb) * (1.f - wr) * ra);
    atomicAdd(&hist[r0 * ks + c1], (1.f - wb) * wr * ra);
    atomicAdd(&hist[r1 * ks + c0], wb * (1.f - wr) * ra);
    atomicAdd(&hist[(r0 + 1) * ks + (c0 + 1)], wb * wr * ra);
}

// "Edge-exact" PSF grid (Lensgroup(parity="edge"), aadff_psf_points_edge): the only discontinuity of the histogram is the window
// test of deeplens/monte_carlo.py:37 - a hit within the float32 noise of the window's edge lands inside or outside depending on
// the LAST BIT of the trace, and one flipped border ray changes a cropped PSF by 1 / (rays inside).  The fast kernel therefore does
// not decide such rays: a live ray whose hit lies within `delta` of the edge (and not further outside than delta in the other
// coordinate) is not splatted but appended as (point << 16 | sample) to the list of its (focus state, wavelength) job;
// aadff_strict_edge_retrace (csrc/strict_fused.hip) re-traces exactly those rays in the reference's own float32 operation
// order, decides them and adds their taps, and aadff_psf_normalise divides.  Every other ray is the fast kernel's.
struct EdgeArgs {
    float delta;              // half-width of the undecided band around the window edge [mm]
    unsigned* count;          // [S*L] rays appended per job (zeroed by the caller)
    unsigned* list;           // [S*L][cap]
    int cap;
    float* raw;               // [S*L][N][ks*ks] unnormalised histograms (every element written)
    float* slope;             // [S*L][N][2] or NULL: mean direction tangents (dx/dz, dy/dz) of the valid chief rays at the sensor - what
                              // moves the centre when the sensor plane moves (the re-trace corrects the centre for the caller's exact
                              // d_sensor when this launch ran on provisional lens states, aadff_strict_edge_retrace)
};

// returns true when the hit was left to the re-trace (appended or, beyond cap, counted: the host sees count > cap)
__device__ __forceinline__ bool edge_defer(const SplatGeom& g, const EdgeArgs& e, float ox, float oy, bool alive, float cx, float cy, int job, int n,
                                           int sample) {
    const float ax = fabsf(-ox - cx), ay = fabsf(-oy - cy);
    const float out = g.lim + e.delta;
    const bool near = (fabsf(ax - g.lim) < e.delta) || (fabsf(ay - g.lim) < e.delta);
    if (!(alive && near && ax < out && ay < out)) return false;
    const unsigned slot = atomicAdd(e.count + job, 1u);
    if (slot < (unsigned)e.cap) e.list[(size_t)job * e.cap + slot] = ((unsigned)n << 16) | (unsigned)sample;
    return true;
}

__global__ __launch_bounds__(256) void psf_splat_kernel(const float* __restrict__ o, const float* __restrict__ ra,
                                                         const float* __restrict__ centre, int spp, int N,
                                                         SplatGeom g, float* psf_raw, float* psf) {
    extern __shared__ float hist[];                      // ks * ks floats (dynamic: ks up to AADFF_MAX_KS = 51)
    __shared__ float red[4];
    const int n = blockIdx.x, kk = g.ks * g.ks;
    for (int e = threadIdx.x; e < kk; e += blockDim.x) hist[e] = 0.f;
    __syncthreads();
    const float cx = centre[2 * n], cy = centre[2 * n + 1];
    for (int i = threadIdx.x; i < spp; i += blockDim.x) {
        const size_t e = (size_t)i * N + n;
        splat_hit<true>(hist, g, o[3 * e], o[3 * e + 1], ra[e], cx, cy);
    }
    __syncthreads();
    float part = 0.f;
    for (int e = threadIdx.x; e < kk; e += blockDim.x) part += hist[e];
    part = wave_sum(part);
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = part;
    __syncthreads();
    const float total = red[0] + red[1] + red[2] + red[3];
    for (int e = threadIdx.x; e < kk; e += blockDim.x) {
        if (psf_raw) psf_raw[(size_t)n * kk + e] = hist[e];
        psf[(size_t)n * kk + e] = hist[e] / total;        // 0/0 -> NaN as in deeplens/optics.py:978
    }
}

// ------------------------------------------------------------------------------------
// Fused PSF kernel: workgroup = (point n, wavelength l, focus state s).
//   phase 1  chief-ray centre (shrunk pupil, chief table): deeplens/optics.py:888-913
//   phase 2  main rays -> LDS histogram                    deeplens/optics.py:933-976
//   phase 3  normalise, write (optionally in psf_map tiling, optics.py:1025)
// ------------------------------------------------------------------------------------
// Upload riding on a psf_points launch (see aadff_stage_t in include/aadff.h).
struct StageArgs {
    const float4* src;
    float4* dst;
    long slice_n4;
    int first_slice, copy_wgs;
    unsigned* counters;
    unsigned target;
};

#ifndef AADFF_PSF_THREADS
#define AADFF_PSF_THREADS 512
#endif
#ifndef AADFF_STAGE_SPIN_MAX
#define AADFF_STAGE_SPIN_MAX (1 << 22)      // x s_sleep(16): ~0.1 s; -DAADFF_STAGE_SPIN_MAX=0 forces the late path (tests)
#endif
constexpr int kPsfThreads = AADFF_PSF_THREADS, kPsfWaves = kPsfThreads / 64;
constexpr int kCompactMax = 2048;         // rays per compaction chunk of the main pass (48 KB of LDS)
// sum of the histogram and the normalised write (deeplens/optics.py:978, psf_map tiling :1025): the tail of the fused kernel and the
// whole of psf_normalise_kernel - one summation order, so a PSF without deferred rays is bit for bit the fused kernel's
__device__ __forceinline__ void normalise_and_write(const float* hist, float* red, const SplatGeom& g, int map_grid, float* psf, int s, int l, int n, int N,
                                                    int L) {
    const int tid = threadIdx.x, kk = g.ks * g.ks;
    float part = 0.f;
    for (int e = tid; e < kk; e += kPsfThreads) part += hist[e];
    part = wave_sum(part);
    __syncthreads();
    if ((tid & 63) == 0) red[tid >> 6] = part;
    __syncthreads();
    float total = 0.f;
#pragma unroll
    for (int w = 0; w < kPsfWaves; ++w) total += red[w];
    const int ks = g.ks;
    for (int e = tid; e < kk; e += kPsfThreads) {
        const float v = hist[e] / total;
        if (map_grid > 0) {
            const int gi = n / map_grid, gj = n - gi * map_grid, u = e / ks, w = e - u * ks;
            const int G = map_grid * ks;
            psf[((size_t)(s * L + l) * G + gi * ks + u) * G + gj * ks + w] = v;
        } else {
            psf[(((size_t)s * N + n) * L + l) * kk + e] = v;
        }
    }
}

// the workgroup's static LDS, declared once per kernel: psf_points_body is instantiated per kind sequence
struct PsfLds {
    float* red;
    int* stage_late;
#if !defined(AADFF_PSF_SCALAR) && !defined(AADFF_PSF_NO_COMPACT)
    float (*cbuf)[kCompactMax];
    unsigned short* cidx;
    int* c_count;
#endif
};
template <bool EDGE>
__device__ __forceinline__ PsfLds psf_lds() {
    __shared__ float red[(EDGE ? 5 : 3) * kPsfWaves];
    __shared__ int stage_late;
#if !defined(AADFF_PSF_SCALAR) && !defined(AADFF_PSF_NO_COMPACT)
    __shared__ float cbuf[6][kCompactMax];               // survivors of the first surfaces: origin and direction
    __shared__ unsigned short cidx[EDGE ? kCompactMax : 1];   // EDGE: and which sample each of them is
    __shared__ int c_count;
    return {red, &stage_late, cbuf, cidx, &c_count};
#else
    return {red, &stage_late};
#endif
}

// FIT: the launch carries fitted chief centres (fit_c); without it the body is the code of a launch that never had any
// PTS (fit launches): u_main / u_chief are blocks of pupil points (chief_fit_weights_kernel<true>), an x row where a block of draws has
// its theta row and a y row for its r row: read, not mapped.  Such a launch stages nothing: its points are in device memory
template <bool EDGE, class SEQ, bool FIT = false, bool PTS = false>
__device__ __forceinline__ void psf_points_body(const PsfLds& lds, const float* __restrict__ points, int N, int L,
                                                          const aadff_surface_t* __restrict__ surf_main,
                                                          const aadff_surface_t* __restrict__ surf_chief,
                                                          aadff_lens_const_t lc,
                                                          const aadff_lens_state_t* __restrict__ states,
                                                          const float* __restrict__ u_main, int spp, long main_ss,
                                                          long main_sl, const float* __restrict__ u_chief,
                                                          int spp_chief, long chief_ss, long chief_sl, SplatGeom g, int centre_mode, int map_grid, float* psf,
                                                          float* centre_out, int* flags, StageArgs stage, const EdgeArgs& edge,
                                                          const float* __restrict__ fit_c = nullptr) {
    extern __shared__ float hist[];                      // ks * ks floats (dynamic: ks up to AADFF_MAX_KS = 51)
    float* const red = lds.red;
    int& stage_late = *lds.stage_late;
#if !defined(AADFF_PSF_SCALAR) && !defined(AADFF_PSF_NO_COMPACT)
    float (*const cbuf)[kCompactMax] = lds.cbuf;
    unsigned short* const cidx = lds.cidx;
    int& c_count = *lds.c_count;
#endif
    const int n = blockIdx.x, l = blockIdx.y;
    int s = blockIdx.z;
    const int tid = threadIdx.x, kk = g.ks * g.ks;
    static_assert(!PTS || (FIT && !EDGE), "pupil points: launches with fitted centres only");
    if constexpr (PTS) {
        // a launch with points that replaces a staged one keeps the counters of the states it would have staged in step with the
        // caller's generation count: the next launch on them may stage again
        if (stage.counters && blockIdx.x == 0 && blockIdx.y == 0 && tid == 0 && s >= stage.first_slice)
            __hip_atomic_fetch_add(stage.counters + s, (unsigned)stage.copy_wgs, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    } else if (stage.src) {
        // Staged launch (aadff_psf_points_staged): the z = 0 plane of the grid is dispatched first; its first
        // stage.copy_wgs workgroups stream the uniform blocks of focus states >= first_slice from pinned host
        // memory into HBM and publish a per-state counter; PSF workgroups of those states wait on it.
        if (s == 0) {
            const int w = blockIdx.y * gridDim.x + blockIdx.x;
            if (w >= stage.copy_wgs) return;
            const int S = (int)gridDim.z - 1;
            const long stride = (long)stage.copy_wgs * kPsfThreads;
            for (int sl = stage.first_slice; sl < S; ++sl) {
                const float4* src = stage.src + (long)sl * stage.slice_n4;
                float4* dst = stage.dst + (long)sl * stage.slice_n4;
                for (long i = (long)w * kPsfThreads + tid; i < stage.slice_n4; i += stride) dst[i] = src[i];
                __syncthreads();
                if (tid == 0) __hip_atomic_fetch_add(stage.counters + sl, 1u, __ATOMIC_RELEASE, __HIP_MEMORY_SCOPE_AGENT);
            }
            return;
        }
        s -= 1;
        if (s >= stage.first_slice) {
            // HIP promises no dispatch order: if the copy workgroups have not delivered this state's block within the
            // bound (they normally lead by tens of microseconds), do not trace stale samples — read this state's draws
            // straight from the mapped pinned block over PCIe (slow, still correct) and raise flag bit 3 so the host
            // learns that the overlap was lost.
            if (tid == 0) {
                int spins = 0, late = 0;
                while ((int)(__hip_atomic_load(stage.counters + s, __ATOMIC_ACQUIRE, __HIP_MEMORY_SCOPE_AGENT) - stage.target) < 0) {
                    __builtin_amdgcn_s_sleep(16);
                    if (++spins > AADFF_STAGE_SPIN_MAX) { if (flags) atomicOr(flags, 8); late = 1; break; }     // never hang the queue
                }
                stage_late = late;
            }
            __syncthreads();
            if (stage_late) {
                u_main = reinterpret_cast<const float*>(stage.src) + (u_main - reinterpret_cast<const float*>(stage.dst));
                if (u_chief) u_chief = reinterpret_cast<const float*>(stage.src) + (u_chief - reinterpret_cast<const float*>(stage.dst));
            }
        }
    }
    // (coherent loads, common.h: fresh - the per-call API and the strict / edge paths re-upload lens states to a fixed address)
    struct { float d_sensor, tan_hfov; } st;
    st.d_sensor = fresh_uniform(&states[s].d_sensor);
    st.tan_hfov = fresh_uniform(&states[s].tan_hfov);
    // a focus state whose refocus found no valid ray has d_sensor = 0/0: the reference stops there with "sensor position is
    // negative." (deeplens/optics.py:1176); in a pipelined stack the condition travels in the flags word (bit 2)
    if (tid == 0 && !(st.d_sensor > 0.f) && flags) atomicOr(flags, 4);
    for (int e = tid; e < kk; e += kPsfThreads) hist[e] = 0.f;

    // object-space point: deeplens/optics.py:953-959 with calc_scale_pinhole (:1286-1290)
    const float* pt = points + ((size_t)s * N + n) * 3;
    const float xn = pt[0], yn = pt[1], depth = pt[2];
    const float scale = (-depth) * st.tan_hfov / lc.r_last;
    const float px = xn * scale * lc.sensor_w / 2.f;
    const float py = yn * scale * lc.sensor_h / 2.f;
    int nan_flag = 0;

    float cx, cy;
    if (centre_mode == 1) {
        const float* ut = u_chief + (size_t)s * chief_ss + (size_t)l * chief_sl;
        const float* ur = ut + spp_chief;
        float sx = 0.f, sy = 0.f, sw = 0.f;
        [[maybe_unused]] float tx = 0.f, ty = 0.f;       // EDGE: sums of the direction tangents of the valid chief rays
        // fit launches: chief_fit_centres_kernel has left {hit x, hit y, guards passed, -} for every workgroup;
        // where the guards passed the centre stands and no chief ray is traced here, elsewhere every draw is, as without a fit
        const float* fc = FIT && !EDGE && fit_c ? fit_c + ((size_t)(s * L + l) * N + n) * 4 : nullptr;
        const bool fitted = fc && fc[2] != 0.f;          // workgroup-uniform
        const int n_chief = fitted ? 0 : spp_chief;
#ifndef AADFF_PSF_SCALAR
        for (int i = tid; i < n_chief; i += 2 * kPsfThreads) {
            const int i1 = i + kPsfThreads;
            const i2 act = {-1, i1 < spp_chief ? -1 : 0};
            const int j1 = act.y ? i1 : i;
            f2 x2, y2;
            // (EDGE: the stack's uniforms are a block the host re-uploads to one address: coherent loads, common.h: fresh)
            if constexpr (PTS) { x2 = (f2){ut[i], ut[j1]}; y2 = (f2){ur[i], ur[j1]}; }
            else
            disc_sample2(EDGE ? (f2){fresh(ut + i), fresh(ut + j1)} : (f2){ut[i], ut[j1]}, EDGE ? (f2){fresh(ur + i), fresh(ur + j1)} : (f2){ur[i], ur[j1]},
                         lc.enp_r2_shrunk, x2, y2);
            const Ray2 r = trace_pair_to_sensor<SEQ>(px, py, depth, x2, y2, lc.enp_z, act, surf_chief, lc.n_surf, st.d_sensor, nan_flag);
            const f2 wx = r.ox * r.ra, wy = r.oy * r.ra;
            sx += wx.x + wx.y; sy += wy.x + wy.y; sw += r.ra.x + r.ra.y;
            if (EDGE) {
                const f2 iz = vrcp(r.dz);
                const f2 ax = vsel(r.alive, r.dx * iz, f2s(0.f)), ay = vsel(r.alive, r.dy * iz, f2s(0.f));
                tx += ax.x + ax.y; ty += ay.x + ay.y;
            }
        }
#else
        for (int i = tid; i < n_chief; i += kPsfThreads) {
            float x2, y2;
            if constexpr (PTS) { x2 = ut[i]; y2 = ur[i]; }
            else disc_sample(ut[i], ur[i], lc.enp_r2_shrunk, x2, y2);
            Ray r = ray_to(px, py, depth, x2, y2, lc.enp_z);
            trace_range<false>(surf_chief, 0, lc.n_surf, true, r, nan_flag);
            propagate_to(r, st.d_sensor);
            sx += r.ox * r.ra; sy += r.oy * r.ra; sw += r.ra;
        }
#endif
        if (fitted) {
            cx = -fc[0]; cy = -fc[1];
            __syncthreads();
        } else {
            sx = wave_sum(sx); sy = wave_sum(sy); sw = wave_sum(sw);
            if (EDGE) { tx = wave_sum(tx); ty = wave_sum(ty); }
            if ((tid & 63) == 0) {
                red[(tid >> 6) * 3] = sx; red[(tid >> 6) * 3 + 1] = sy; red[(tid >> 6) * 3 + 2] = sw;
                if (EDGE) { red[3 * kPsfWaves + (tid >> 6) * 2] = tx; red[3 * kPsfWaves + (tid >> 6) * 2 + 1] = ty; }
            }
            __syncthreads();
            sx = sy = sw = 0.f;
#pragma unroll
            for (int w = 0; w < kPsfWaves; ++w) { sx += red[3 * w]; sy += red[3 * w + 1]; sw += red[3 * w + 2]; }
            cx = -(sx / (sw + kEps));
            cy = -(sy / (sw + kEps));
            if (EDGE && edge.slope && tid == 0) {
                tx = ty = 0.f;
                for (int w = 0; w < kPsfWaves; ++w) { tx += red[3 * kPsfWaves + 2 * w]; ty += red[3 * kPsfWaves + 2 * w + 1]; }
                float* so = edge.slope + ((size_t)(s * L + l) * N + n) * 2;
                so[0] = tx / (sw + kEps); so[1] = ty / (sw + kEps);
            }
            if (sw == 0.f && tid == 0 && flags) atomicOr(flags, 2);      // "No sampled rays is valid." (optics.py:901)
        }
    } else {
        cx = xn * (lc.sensor_w / 2.f);                               // optics.py:972-974
        cy = yn * (lc.sensor_h / 2.f);
        __syncthreads();
    }
    if (centre_out && tid == 0) {
        float* co = centre_out + ((size_t)(s * L + l) * N + n) * 2;
        co[0] = cx; co[1] = cy;
    }

    const aadff_surface_t* tab = surf_main + (size_t)l * lc.n_surf;
#if !defined(AADFF_PSF_SCALAR) && !defined(AADFF_PSF_NO_COMPACT)
    [[maybe_unused]] int split = lc.n_surf / 2;           // compaction point: two surfaces behind the stop (KindSeq::split)
    if constexpr (SEQ::n == 0)
        for (int i = 0; i < lc.n_surf; ++i)
            if (tab[i].kind == AADFF_SURF_STOP) { split = min(i + 2, lc.n_surf); break; }
#endif
    const float* ut = u_main + (size_t)s * main_ss + (size_t)l * main_sl;
    const float* ur = ut + spp;
#ifndef AADFF_PSF_SCALAR
#ifndef AADFF_PSF_NO_COMPACT
    // Main pass in two phases with the survivors compacted in between: a third of the rays of an off-axis point die
    // at the apertures right behind the stop, scattered over all lanes, so no wave ever finishes early; after the
    // compaction the remaining surfaces (both aspheres of rf50mm) run on full waves only.  Chunks of kCompactMax rays.
    for (int c0 = 0; c0 < spp; c0 += kCompactMax) {
        const int cn = min(spp - c0, kCompactMax);
        if (tid == 0) c_count = 0;
        __syncthreads();
        for (int i = tid; i < cn; i += 2 * kPsfThreads) {
            const int i1 = i + kPsfThreads;
            const i2 act = {-1, i1 < cn ? -1 : 0};
            const int j1 = act.y ? i1 : i;
            f2 x2, y2;
            if constexpr (PTS) { x2 = (f2){ut[c0 + i], ut[c0 + j1]}; y2 = (f2){ur[c0 + i], ur[c0 + j1]}; }
            else
            disc_sample2(EDGE ? (f2){fresh(ut + c0 + i), fresh(ut + c0 + j1)} : (f2){ut[c0 + i], ut[c0 + j1]},
                         EDGE ? (f2){fresh(ur + c0 + i), fresh(ur + c0 + j1)} : (f2){ur[c0 + i], ur[c0 + j1]}, lc.enp_r2, x2, y2);
            Ray2 r;
            r.ox = f2s(px); r.oy = f2s(py); r.oz = f2s(depth);
            r.dx = x2 - px; r.dy = y2 - py; r.dz = f2s(lc.enp_z - depth);
            const f2 inv = vrsq(vmax(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz, f2s(1e-24f)));
            r.dx *= inv; r.dy *= inv; r.dz *= inv;
            r.alive = act;
            if constexpr (SEQ::n == 0) trace_part2(tab, 0, split, r, nan_flag);
            else trace_seq2<SEQ, 0, SEQ::split>(tab, r, nan_flag);
            // append the survivors: one LDS atomic per wave, slots by ballot prefix
            const unsigned long long bx = __ballot(r.alive.x != 0), by = __ballot(r.alive.y != 0);
            const int nx = __popcll(bx), ny = __popcll(by);
            int base = 0;
            if ((tid & 63) == 0) base = atomicAdd(&c_count, nx + ny);
            base = __builtin_amdgcn_readfirstlane(base);
            const unsigned long long below = (1ull << (tid & 63)) - 1ull;
            if (r.alive.x) {
                const int k = base + __popcll(bx & below);
                cbuf[0][k] = r.ox.x; cbuf[1][k] = r.oy.x; cbuf[2][k] = r.oz.x; cbuf[3][k] = r.dx.x; cbuf[4][k] = r.dy.x; cbuf[5][k] = r.dz.x;
                if (EDGE) cidx[k] = (unsigned short)(c0 + i);
            }
            if (r.alive.y) {
                const int k = base + nx + __popcll(by & below);
                cbuf[0][k] = r.ox.y; cbuf[1][k] = r.oy.y; cbuf[2][k] = r.oz.y; cbuf[3][k] = r.dx.y; cbuf[4][k] = r.dy.y; cbuf[5][k] = r.dz.y;
                if (EDGE) cidx[k] = (unsigned short)(c0 + j1);
            }
        }
        __syncthreads();
        const int ns = c_count;
        for (int q = tid; 2 * q < ns; q += kPsfThreads) {
            const bool two = 2 * q + 1 < ns;
            const int k0 = 2 * q, k1 = two ? k0 + 1 : k0;
            Ray2 r;
            r.ox = (f2){cbuf[0][k0], cbuf[0][k1]}; r.oy = (f2){cbuf[1][k0], cbuf[1][k1]}; r.oz = (f2){cbuf[2][k0], cbuf[2][k1]};
            r.dx = (f2){cbuf[3][k0], cbuf[3][k1]}; r.dy = (f2){cbuf[4][k0], cbuf[4][k1]}; r.dz = (f2){cbuf[5][k0], cbuf[5][k1]};
            r.alive = (i2){-1, two ? -1 : 0};
            if constexpr (SEQ::n == 0) trace_part2(tab, split, lc.n_surf, r, nan_flag);
            else trace_seq2<SEQ, SEQ::split, SEQ::n>(tab, r, nan_flag);
            const f2 t = (st.d_sensor - r.oz) * vrcp(r.dz);
            r.ox += r.dx * t; r.oy += r.dy * t;
            if (!(EDGE && edge_defer(g, edge, r.ox.x, r.oy.x, r.alive.x != 0, cx, cy, s * L + l, n, cidx[EDGE ? k0 : 0])))
                splat_hit(hist, g, r.ox.x, r.oy.x, r.alive.x ? 1.f : 0.f, cx, cy);
            if (!(EDGE && edge_defer(g, edge, r.ox.y, r.oy.y, r.alive.y != 0, cx, cy, s * L + l, n, cidx[EDGE ? k1 : 0])))
                splat_hit(hist, g, r.ox.y, r.oy.y, r.alive.y ? 1.f : 0.f, cx, cy);
        }
        __syncthreads();                                  // cbuf / c_count are reused by the next chunk
    }
#else
    for (int i = tid; i < spp; i += 2 * kPsfThreads) {
        const int i1 = i + kPsfThreads;
        const i2 act = {-1, i1 < spp ? -1 : 0};
        const int j1 = act.y ? i1 : i;
        f2 x2, y2;
        if constexpr (PTS) { x2 = (f2){ut[i], ut[j1]}; y2 = (f2){ur[i], ur[j1]}; }
        else disc_sample2((f2){ut[i], ut[j1]}, (f2){ur[i], ur[j1]}, lc.enp_r2, x2, y2);
        const Ray2 r = trace_pair_to_sensor<SEQ>(px, py, depth, x2, y2, lc.enp_z, act, tab, lc.n_surf, st.d_sensor, nan_flag);
        if (!(EDGE && edge_defer(g, edge, r.ox.x, r.oy.x, r.ra.x > 0.f, cx, cy, s * L + l, n, i))) splat_hit(hist, g, r.ox.x, r.oy.x, r.ra.x, cx, cy);
        if (!(EDGE && edge_defer(g, edge, r.ox.y, r.oy.y, r.ra.y > 0.f, cx, cy, s * L + l, n, j1))) splat_hit(hist, g, r.ox.y, r.oy.y, r.ra.y, cx, cy);
    }
#endif
#else
    for (int i = tid; i < spp; i += kPsfThreads) {
        float x2, y2;
        if constexpr (PTS) { x2 = ut[i]; y2 = ur[i]; }
        else disc_sample(ut[i], ur[i], lc.enp_r2, x2, y2);
        Ray r = ray_to(px, py, depth, x2, y2, lc.enp_z);
        trace_range<false>(tab, 0, lc.n_surf, true, r, nan_flag);
        propagate_to(r, st.d_sensor);
        if (!(EDGE && edge_defer(g, edge, r.ox, r.oy, r.ra > 0.f, cx, cy, s * L + l, n, i))) splat_hit(hist, g, r.ox, r.oy, r.ra, cx, cy);
    }
#endif
    __syncthreads();
    if (EDGE) {                                          // unnormalised: the re-trace adds the deferred rays, aadff_psf_normalise divides
        float* raw = edge.raw + ((size_t)(s * L + l) * N + n) * kk;
        for (int e = tid; e < kk; e += kPsfThreads) raw[e] = hist[e];
    } else {
        normalise_and_write(hist, red, g, map_grid, psf, s, l, n, N, L);
    }
    if (nan_flag && flags) atomicOr(flags, 1);
}

// Chief-centre fit, the node rays: one wave per (point, state) traces the kChiefRays node and guard-ring rays of the shrunk
// pupil, lane i the rays i and i + 64, through the PSF kernel's own trace_pair_to_sensor, and leaves {hit x, hit y, ok, 0} in
// out [S][L][N][4] for the wavelengths [l0, l1): the chief table, the nodes, the point and the state are the same for every
// wavelength, so the rays are, and only the weights of (state, wavelength) differ - one trace, l1 - l0 weighted sums in the order a wave
// per wavelength took them (AADFF_CHIEF_CENTRES=per_wavelength launches this kernel with such waves, l1 = l0 + 1: the same bits).  The hit is h_0 + sum_k w_k (h_k - h_0) with h_0 the centre node's (an error in sum w then multiplies a spot size,
// not a sensor coordinate); ok unless a node or ring ray died (vignetting reaches into the shrunk pupil: the hit is no polynomial
// there) or the degree-d and degree-(d - 2) hits disagree.  A kernel of its own, not a first pass of the PSF kernel's workgroups: there
// one wave traced while seven waited, the workgroup kept its LDS and wave slots meanwhile, and of the 45 % of the instructions saved
// for three workgroups in five the kernel got 5 % faster.
constexpr int kNodeWaves = 4;
template <class SEQ>
__device__ __forceinline__ void chief_fit_centre_body(const float* __restrict__ points, int N, int L, const aadff_surface_t* __restrict__ surf_chief,
                                                      aadff_lens_const_t lc, const aadff_lens_state_t* __restrict__ states,
                                                      const float* __restrict__ fit_w, float* __restrict__ out, int n, int l0, int l1, int s) {
    const int i = threadIdx.x & 63, j1 = i + 64;
    const float d_sensor = fresh_uniform(&states[s].d_sensor), tan_hfov = fresh_uniform(&states[s].tan_hfov);
    const float* pt = points + ((size_t)s * N + n) * 3;
    const float xn = pt[0], yn = pt[1], depth = pt[2];
    const float scale = (-depth) * tan_hfov / lc.r_last;            // as psf_points_body
    const float px = xn * scale * lc.sensor_w / 2.f;
    const float py = yn * scale * lc.sensor_h / 2.f;
    const float rs = fsqrt(lc.enp_r2_shrunk);
    const f2 x2 = (f2){d_chief_node_xy[2 * i], d_chief_node_xy[2 * j1]} * rs, y2 = (f2){d_chief_node_xy[2 * i + 1], d_chief_node_xy[2 * j1 + 1]} * rs;
    int nan_flag = 0;                                               // a NaN in a ray that is not one of the reference's is no error of the reference's
    const Ray2 r = trace_pair_to_sensor<SEQ>(px, py, depth, x2, y2, lc.enp_z, (i2){-1, -1}, surf_chief, lc.n_surf, d_sensor, nan_flag);
    const float hx0 = __shfl(r.ox.x, 0, kWave), hy0 = __shfl(r.oy.x, 0, kWave);
    const bool node1 = j1 < kChiefNodes;                            // i < 64 <= kChiefNodes: a lane's first ray always is a node
    const f2 ex = r.ox - hx0, ey = r.oy - hy0;
    const bool all_alive = __all(r.alive.x != 0 && r.alive.y != 0);  // guard (a): the rays', shared; guard (b): each wavelength's own
    for (int l = l0; l < l1; ++l) {
        const float* w = fit_w + (size_t)(s * L + l) * 2 * kChiefNodes;
        const f2 wd = {w[i], node1 ? w[j1] : 0.f}, wl = {w[kChiefNodes + i], node1 ? w[kChiefNodes + j1] : 0.f};
        const f2 adx = wd * ex, ady = wd * ey, alx = wl * ex, aly = wl * ey;
        const float fx = wave_sum(adx.x + adx.y), fy = wave_sum(ady.x + ady.y);
        const float gx = wave_sum(alx.x + alx.y), gy = wave_sum(aly.x + aly.y);
        if (i == 0) {
            const bool ok = all_alive && fabsf(fx - gx) <= kChiefFitTol && fabsf(fy - gy) <= kChiefFitTol;
            *reinterpret_cast<float4*>(out + ((size_t)(s * L + l) * N + n) * 4) = make_float4(hx0 + fx, hy0 + fy, ok ? 1.f : 0.f, 0.f);
        }
    }
}
// grid (ceil(N / kNodeWaves), 1, S), or with per_l (ceil(N / kNodeWaves), L, S) and a wave per wavelength; surf_main: the table whose
// kinds decide the trace with surf_chief's, as in psf_points_dispatch (the kinds are the same in every wavelength's table)
__global__ __launch_bounds__(kNodeWaves * 64) void chief_fit_centres_kernel(const float* __restrict__ points, int N, int L,
                                                                             const aadff_surface_t* __restrict__ surf_main,
                                                                             const aadff_surface_t* __restrict__ surf_chief, aadff_lens_const_t lc,
                                                                             const aadff_lens_state_t* __restrict__ states,
                                                                             const float* __restrict__ fit_w, int trace_mode, int per_l,
                                                                             float* __restrict__ out) {
    const int n = blockIdx.x * kNodeWaves + (threadIdx.x >> 6), s = blockIdx.z;
    const int l0 = per_l ? (int)blockIdx.y : 0, l1 = per_l ? l0 + 1 : L;
    if (n >= N) return;                                             // whole waves
    auto body = [&](auto seq) { chief_fit_centre_body<decltype(seq)>(points, N, L, surf_chief, lc, states, fit_w, out, n, l0, l1, s); };
    [[maybe_unused]] const int path = psf_seq_path(surf_main + (size_t)l0 * lc.n_surf, surf_chief, lc.n_surf, trace_mode == 1);
#ifndef AADFF_PSF_NO_SEQ
    if (path == 1) body(seq::Rf50mm{});
    else if (path == 2) body(seq::F28{});
    else
#endif
        body(KindLoop{});
}

// One body per kind sequence, chosen once per workgroup.  The kinds are the same in every wavelength's table (only the indices
// differ); this workgroup's own is the one checked, and the chief table where the chief pass runs.  trace_mode (AADFF_PSF_TRACE):
// 1 = the loop for every lens; 2 = as 0, and a workgroup that takes a compiled sequence ORs kPsfSeqFlag << (path - 1) into flags.
constexpr int kPsfSeqFlag = 256;
template <bool FIT, bool PTS>
__device__ __forceinline__ void psf_points_dispatch(const float* __restrict__ points, int N, int L,
                                                    const aadff_surface_t* __restrict__ surf_main,
                                                    const aadff_surface_t* __restrict__ surf_chief,
                                                    aadff_lens_const_t lc,
                                                    const aadff_lens_state_t* __restrict__ states,
                                                    const float* __restrict__ u_main, int spp, long main_ss,
                                                    long main_sl, const float* __restrict__ u_chief,
                                                    int spp_chief, long chief_ss, long chief_sl, SplatGeom g, int centre_mode, int map_grid, float* psf,
                                                    float* centre_out, int* flags, StageArgs stage, int trace_mode, const float* __restrict__ fit_c) {
    const PsfLds lds = psf_lds<false>();
    auto body = [&](auto seq) {
        psf_points_body<false, decltype(seq), FIT, PTS>(lds, points, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_ss, main_sl, u_chief, spp_chief, chief_ss,
                                              chief_sl, g, centre_mode, map_grid, psf, centre_out, flags, stage, EdgeArgs{}, fit_c);
    };
    [[maybe_unused]] const int path = psf_seq_path(surf_main + (size_t)blockIdx.y * lc.n_surf, centre_mode == 1 ? surf_chief : nullptr, lc.n_surf, trace_mode == 1);
#ifndef AADFF_PSF_NO_SEQ
    if (trace_mode == 2 && path && flags && threadIdx.x == 0) atomicOr(flags, kPsfSeqFlag << (path - 1));
    if (path == 1) body(seq::Rf50mm{});
    else if (path == 2) body(seq::F28{});
    else
#endif
        body(KindLoop{});
}

// TIMED: the same code under a second name for the launches that carry aadff_time_next_launch's events (see conv.hip)
template <bool TIMED, bool FIT, bool PTS = false>
__global__ __launch_bounds__(kPsfThreads, 6) void psf_points_kernel(const float* __restrict__ points, int N, int L,
                                                          const aadff_surface_t* __restrict__ surf_main,
                                                          const aadff_surface_t* __restrict__ surf_chief,
                                                          aadff_lens_const_t lc,
                                                          const aadff_lens_state_t* __restrict__ states,
                                                          const float* __restrict__ u_main, int spp, long main_ss,
                                                          long main_sl, const float* __restrict__ u_chief,
                                                          int spp_chief, long chief_ss, long chief_sl, SplatGeom g, int centre_mode, int map_grid, float* psf,
                                                          float* centre_out, int* flags, StageArgs stage, int trace_mode, const float* __restrict__ fit_c) {
    psf_points_dispatch<FIT, PTS>(points, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_ss, main_sl, u_chief, spp_chief, chief_ss, chief_sl, g,
                        centre_mode, map_grid, psf, centre_out, flags, stage, trace_mode, fit_c);
}

// the edge-exact form: band rays deferred to aadff_strict_edge_retrace, histograms left unnormalised in edge.raw.  It stays on the
// run-time loop for every lens: with a body per kind sequence its spills went up (scratch 32 -> 40 B, VGPR spills 9 -> 15, SGPR
// spills 58 -> 137) - over the budget the sequence trace was given, for a kernel outside the headline step.
__global__ __launch_bounds__(kPsfThreads, 6) void psf_points_edge_kernel(const float* __restrict__ points, int N, int L,
                                                          const aadff_surface_t* __restrict__ surf_main,
                                                          const aadff_surface_t* __restrict__ surf_chief,
                                                          aadff_lens_const_t lc,
                                                          const aadff_lens_state_t* __restrict__ states,
                                                          const float* __restrict__ u_main, int spp, long main_ss,
                                                          long main_sl, const float* __restrict__ u_chief,
                                                          int spp_chief, long chief_ss, long chief_sl, SplatGeom g, int centre_mode,
                                                          float* centre_out, int* flags, EdgeArgs edge) {
    psf_points_body<true, KindLoop>(psf_lds<true>(), points, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_ss, main_sl, u_chief, spp_chief, chief_ss,
                                    chief_sl, g, centre_mode, 0, nullptr, centre_out, flags, StageArgs{}, edge);
}

// raw [S*L][N][ks*ks] -> normalised PSFs in either layout of aadff_psf_points (grid: N x L x S)
__global__ __launch_bounds__(kPsfThreads) void psf_normalise_kernel(const float* __restrict__ raw, int N, int L, SplatGeom g, int map_grid, float* psf) {
    extern __shared__ float hist[];
    __shared__ float red[3 * kPsfWaves];
    const int n = blockIdx.x, l = blockIdx.y, s = blockIdx.z, kk = g.ks * g.ks;
    const float* src = raw + ((size_t)(s * L + l) * N + n) * kk;
    for (int e = threadIdx.x; e < kk; e += kPsfThreads) hist[e] = src[e];
    __syncthreads();
    normalise_and_write(hist, red, g, map_grid, psf, s, l, n, N, L);
}

// ------------------------------------------------------------------------------------
// Refocus + post_computation: workgroup per focus state.
//   deeplens/optics.py:1155-1180 (refocus), :1187-1217 (calc_fov), :178-187, :1097-1102
// ------------------------------------------------------------------------------------
#ifndef AADFF_STAGE_COPY_WGS
#define AADFF_STAGE_COPY_WGS 14
#endif
constexpr int kStageWorkgroups = 64;     // upload workgroups (x 1024 threads) riding on the refocus launch (aadff_refocus_staged)
constexpr int kRefocusThreads = 1024;     // plain entry: 16 waves per focus state
constexpr int kRefocusSplit = 4;          // staged entry: 4 workgroups x 256 threads per focus state, last arriver finishes
struct RefocusScratch {                   // per focus state, zero-initialised once by the caller; self-resetting
    float part[kRefocusSplit][2];         // (sum, count) of each quarter of the rays
    unsigned arrived;
    unsigned nan_seen;                    // NaN in a Newton residual of a quarter that did not finish the state
    unsigned loaded, passed;              // [state 0 only] gate of the upload workgroups (see refocus_kernel)
    unsigned pad[4];
};
static_assert(sizeof(RefocusScratch) == 64, "aadff.h documents 64 bytes per focus state");

template <int NT, int SPLIT>
__global__ __launch_bounds__(NT) void refocus_kernel(const float* __restrict__ depth, const float* __restrict__ u,
                                                       int spp, long u_ss, const aadff_surface_t* __restrict__ surf,
                                                       aadff_lens_const_t lc, aadff_lens_state_t* states,
                                                       int do_refocus, int S, const float* __restrict__ stage_src,
                                                       float* __restrict__ stage_dst, long stage_n, RefocusScratch* scratch) {
    if ((int)blockIdx.x >= S * SPLIT) {
        // Upload workgroups: copy the pinned-host uniform block to HBM for the PSF kernel while the
        // focus workgroups (which read their own draws straight from the host block) trace.
        // The bulk copy would queue ~20 us of PCIe reads in front of the focus workgroups' own 16 KB of draws:
        // wait until every focus workgroup holds its draws (they have lower block ids: dispatched first).
        if constexpr (SPLIT > 1) {
            if (threadIdx.x == 0) {
                int spins = 0;
                while (__hip_atomic_load(&scratch->loaded, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) < (unsigned)(S * SPLIT)) {
                    __builtin_amdgcn_s_sleep(8);
                    if (++spins > (1 << 20)) break;                       // never hang the queue; only the overlap is lost
                }
                const unsigned old = __hip_atomic_fetch_add(&scratch->passed, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                if (old == gridDim.x - S * SPLIT - 1) {                  // last one through resets the gate for the next launch
                    __hip_atomic_store(&scratch->loaded, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    __hip_atomic_store(&scratch->passed, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                }
            }
            __syncthreads();
        }
        const long n4 = stage_n >> 2;
        const int first = S * SPLIT;
        const long stride = (long)(gridDim.x - first) * NT;
        const float4* src4 = reinterpret_cast<const float4*>(stage_src);
        float4* dst4 = reinterpret_cast<float4*>(stage_dst);
        long i = (long)(blockIdx.x - first) * NT + threadIdx.x;
        for (; i + 3 * stride < n4; i += 4 * stride) {          // four loads in flight per lane: PCIe latency
            const float4 a = src4[i], b = src4[i + stride], c = src4[i + 2 * stride], d = src4[i + 3 * stride];
            dst4[i] = a; dst4[i + stride] = b; dst4[i + 2 * stride] = c; dst4[i + 3 * stride] = d;
        }
        for (; i < n4; i += stride) dst4[i] = src4[i];
        if ((int)blockIdx.x == first && threadIdx.x < (stage_n & 3)) stage_dst[(n4 << 2) + threadIdx.x] = stage_src[(n4 << 2) + threadIdx.x];
        return;
    }
    __shared__ float red[2 * (NT / 64)];
    __shared__ float s_dsensor;
    __shared__ int s_count;
    __shared__ int s_last, s_flags0;
    const int s = blockIdx.x / SPLIT, part = blockIdx.x - s * SPLIT, tid = threadIdx.x;
    int nan_flag = 0;
    int flags = 0;
    if (do_refocus) {
        const float* ut = u + (size_t)s * u_ss;
        const float* ur = ut + spp;
        const float dep = depth[s];
        // this workgroup's rays: [begin, end); two rays per lane (packed arithmetic)
        const int chunk = (spp + SPLIT - 1) / SPLIT;
        const int begin = part * chunk, end = min(spp, begin + chunk);
        float sum = 0.f, cnt = 0.f;
        // first pair of draws up front; with the staged entry they come over PCIe and open the upload gate
        float pt0 = 0.f, pt1 = 0.f, pr0 = 0.f, pr1 = 0.f;
        if (begin + tid < end) {
            const int i = begin + tid, j1 = i + NT < end ? i + NT : i;
            pt0 = ut[i]; pt1 = ut[j1]; pr0 = ur[i]; pr1 = ur[j1];
        }
        if constexpr (SPLIT > 1) {
            asm volatile("s_waitcnt vmcnt(0)" : "+v"(pt0), "+v"(pt1), "+v"(pr0), "+v"(pr1));
            __syncthreads();
            if (tid == 0) __hip_atomic_fetch_add(&scratch->loaded, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
        }
        for (int i = begin + tid; i < end; i += 2 * NT) {
            const int i1 = i + NT;
            const i2 act = {-1, i1 < end ? -1 : 0};
            const int j1 = act.y ? i1 : i;
            f2 x2, y2;
            const bool firstit = i == begin + tid;
            disc_sample2((f2){firstit ? pt0 : ut[i], firstit ? pt1 : ut[j1]}, (f2){firstit ? pr0 : ur[i], firstit ? pr1 : ur[j1]}, lc.first_r2, x2, y2);
            Ray2 r;
            r.ox = x2; r.oy = y2; r.oz = f2s(lc.first_d);
            r.dx = x2; r.dy = y2; r.dz = f2s(lc.first_d - dep);               // o - (0,0,depth)
            const f2 inv = vrsq(vmax(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz, f2s(1e-24f)));
            r.dx *= inv; r.dy *= inv; r.dz *= inv;
            r.alive = act;
            trace_forward2(surf, lc.n_surf, r, nan_flag);
            f2 t = (r.dx * r.ox + r.dy * r.oy) * vrcp(r.dx * r.dx + r.dy * r.dy);
            t = t * r.ra;
            const f2 fd = r.oz - r.dz * t;
            const i2 ok = (r.ra > 0.f) & (fd == fd) & (fd > 0.f);
            sum += (ok.x ? fd.x : 0.f) + (ok.y ? fd.y : 0.f);
            cnt += (ok.x ? 1.f : 0.f) + (ok.y ? 1.f : 0.f);
        }
        sum = wave_sum(sum); cnt = wave_sum(cnt);
        if ((tid & 63) == 0) { red[(tid >> 6) * 2] = sum; red[(tid >> 6) * 2 + 1] = cnt; }
        const int s_nan = __syncthreads_or(nan_flag);
        if (tid == 0) {
            float ts = 0.f, tc = 0.f;
            for (int w = 0; w < NT / 64; ++w) { ts += red[2 * w]; tc += red[2 * w + 1]; }
            int last = 1;
            s_flags0 = 0;
            if constexpr (SPLIT > 1) {
                // publish the partial, count arrivals (the counter wraps to 0 by itself), the last one reduces in
                // fixed order (deterministic) and goes on to the field-of-view trace
                RefocusScratch* sc = scratch + s;
                sc->part[part][0] = ts; sc->part[part][1] = tc;
                if (s_nan) atomicOr(&sc->nan_seen, 1u);
                const unsigned old = __hip_atomic_fetch_add(&sc->arrived, 1u, __ATOMIC_ACQ_REL, __HIP_MEMORY_SCOPE_AGENT);
                last = old == SPLIT - 1;
                if (last) {
                    __hip_atomic_store(&sc->arrived, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    if (atomicExch(&sc->nan_seen, 0u)) s_flags0 = 1;
                    ts = 0.f; tc = 0.f;
                    for (int p = 0; p < SPLIT; ++p) {
                        ts += __hip_atomic_load(&sc->part[p][0], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                        tc += __hip_atomic_load(&sc->part[p][1], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                    }
                }
            }
            s_last = last;
            s_dsensor = ts / tc;
            s_count = (int)tc;
        }
        __syncthreads();
        if (!s_last) return;
        flags = s_flags0;
    } else {
        if (tid == 0) { s_dsensor = states[s].d_sensor; s_count = states[s].n_focus_rays; }
        __syncthreads();
    }
    const float d_sensor = s_dsensor;

    // calc_fov: M=100 rays from the sensor corner through the shrunk exit pupil, traced backward
    constexpr int M = 100;
    float tsum = 0.f, wsum = 0.f;
    if (tid < M) {
        const float start = -lc.exp_r_shrunk, end = lc.exp_r_shrunk;
        const float step = (end - start) / (float)(M - 1);
        const float x2 = tid < M / 2 ? start + step * (float)tid : end - step * (float)(M - 1 - tid);   // torch.linspace
        Ray r = ray_to(lc.r_last, 0.f, d_sensor, x2, 0.f, lc.exp_z);
        trace_range<false>(surf, 0, lc.n_surf, false, r, nan_flag);
        tsum = (r.dx / r.dz) * r.ra;
        wsum = r.ra;
    }
    tsum = wave_sum(tsum); wsum = wave_sum(wsum);
    __syncthreads();
    if ((tid & 63) == 0) { red[(tid >> 6) * 2] = tsum; red[(tid >> 6) * 2 + 1] = wsum; }
    __syncthreads();
    const int any_nan = __syncthreads_or(nan_flag);
    if (tid == 0) {
        if (any_nan) flags |= 1;
        float ts = 0.f, tw = 0.f;
        for (int w = 0; w < NT / 64; ++w) { ts += red[2 * w]; tw += red[2 * w + 1]; }
        float hfov = atanf(ts / tw);
        if (hfov != hfov) { hfov = 0.5f; flags |= 2; }
        const double th = tan((double)hfov);
        const double foclen = (double)lc.r_last / th;
        aadff_lens_state_t o;
        o.d_sensor = d_sensor;
        o.hfov = hfov;
        o.tan_hfov = (float)th;
        o.foclen = (float)foclen;
        o.fnum = (float)(foclen / (double)lc.enp_r / 2.0);
        o.n_focus_rays = s_count;
        o.flags = flags;
        o.pad = 0;
        states[s] = o;
    }
}

}  // namespace aadff

using namespace aadff;

// The address at which the GPU sees a block of pinned host memory (hipHostMalloc / torch pin_memory), or the error "<who> not pinned ..."
static int mapped_host_pointer(const void* host, const char* who, void** out) {
    void* mapped = nullptr;
    if (hipHostGetDevicePointer(&mapped, const_cast<void*>(host), 0) != hipSuccess || !mapped) {
        (void)hipGetLastError();
        AADFF_CHECK_ARG(false, "%s not pinned (device-mapped) host memory", who);
    }
    *out = mapped;
    return 0;
}

extern "C" {

int aadff_trace_rays(const float* o_in, const float* d_in, const float* ra_in, float* o_out, float* d_out,
                     float* ra_out, int n, const aadff_surface_t* surf, int first, int last, int forward,
                     const aadff_lens_state_t* state_or_null, int* flags_or_null, aadff_stream_t stream) {
    AADFF_CHECK_ARG(o_in && d_in && o_out && d_out && ra_out && surf, "trace_rays: NULL pointer");
    AADFF_CHECK_ARG(n >= 0 && first >= 0 && first <= last && last <= AADFF_MAX_SURF, "trace_rays: bad range [%d,%d) or n=%d", first, last, n);
    if (n == 0) return 0;
    hipLaunchKernelGGL(trace_rays_kernel, dim3((n + 255) / 256), dim3(256), 0, (hipStream_t)stream, o_in, d_in, ra_in,
                       o_out, d_out, ra_out, n, surf, first, last, forward, state_or_null, flags_or_null);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_trace_points(const float* points_obj, int N, const float* u_theta, const float* u_r, int spp, float pupil_z,
                       float pupil_r, const aadff_surface_t* surf, int n_surf, const aadff_lens_state_t* state,
                       float* o_out, float* d_out, float* ra_out, aadff_stream_t stream) {
    AADFF_CHECK_ARG(points_obj && u_theta && u_r && surf && state && o_out && d_out && ra_out, "trace_points: NULL pointer");
    AADFF_CHECK_ARG(N > 0 && N <= 65535 && spp > 0 && n_surf > 0 && n_surf <= AADFF_MAX_SURF, "trace_points: bad sizes N=%d spp=%d n_surf=%d", N, spp, n_surf);
    const float r2 = (float)((double)pupil_r * (double)pupil_r);
    hipLaunchKernelGGL(trace_points_kernel, dim3((spp + 255) / 256, N), dim3(256), 0, (hipStream_t)stream, points_obj, N,
                       u_theta, u_r, spp, pupil_z, r2, surf, n_surf, state, o_out, d_out, ra_out);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_psf_splat(const float* o, const float* ra, const float* centre, int spp, int N, float pixel_size, int ks,
                    float* psf_raw_or_null, float* psf, aadff_stream_t stream) {
    AADFF_CHECK_ARG(o && ra && centre && psf, "psf_splat: NULL pointer");
    AADFF_CHECK_ARG(spp > 0 && N > 0 && ks >= 1 && ks <= AADFF_MAX_KS, "psf_splat: bad sizes spp=%d N=%d ks=%d", spp, N, ks);
    hipLaunchKernelGGL(psf_splat_kernel, dim3(N), dim3(256), (size_t)ks * ks * sizeof(float), (hipStream_t)stream, o, ra, centre, spp, N,
                       make_splat_geom(pixel_size, ks), psf_raw_or_null, psf);
    AADFF_CHECK_LAUNCH();
    return 0;
}

// AADFF_PSF_TRACE, read per launch (tests switch it): "loop" sends every lens through the run-time loop of trace_part2 (1);
// "mark" leaves the choice alone and has the workgroups that take a compiled sequence say so in the flags word (2: bit 8 the
// rf50mm sequence, bit 9 the 50mm_f2.8 one - for a caller that passes a flags word of its own, not one raise_psf_flags reads)
static int psf_trace_mode() {
    const char* e = getenv("AADFF_PSF_TRACE");
    return !e ? 0 : strcmp(e, "loop") == 0 ? 1 : strcmp(e, "mark") == 0 ? 2 : 0;
}

// AADFF_PSF_CHIEF, read per launch: "full" makes a fit launch a launch without weights - every chief centre from every draw
static bool psf_chief_full() {
    const char* e = getenv("AADFF_PSF_CHIEF");
    return e && strcmp(e, "full") == 0;
}

// The launches of before, for A/B runs and tests; all read per launch.  AADFF_PSF_POINTS=raw: the entries with pupil points map raw draws
// in every workgroup again (and stage them), the prologue computes the weights alone.  AADFF_CHIEF_CENTRES=per_wavelength: a node-ray
// wave per (point, wavelength, state).  AADFF_PSF_LAUNCHES=parent: both.
static bool psf_launches_parent() {
    const char* e = getenv("AADFF_PSF_LAUNCHES");
    return e && strcmp(e, "parent") == 0;
}
static bool psf_points_raw() {
    const char* e = getenv("AADFF_PSF_POINTS");
    return (e && strcmp(e, "raw") == 0) || psf_launches_parent();
}
static bool chief_centres_per_wavelength() {
    const char* e = getenv("AADFF_CHIEF_CENTRES");
    return (e && strcmp(e, "per_wavelength") == 0) || psf_launches_parent();
}

// pupil_xy: NULL, or the points aadff_chief_fit_prologue made of u_main / u_chief (same sizes and strides)
static int psf_points_launch(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                     const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                     int spp_chief, long chief_stride_s, long chief_stride_l, int ks, int centre_mode,
                     int map_layout, float* psf, float* centre_out_or_null, int* flags_or_null,
                     const aadff_stage_t* stage, const float* fit_weights, float* fit_centres, const float* pupil_xy, aadff_stream_t stream) {
    AADFF_CHECK_ARG(points && surf_main && states && u_main && psf, "psf_points: NULL pointer");
    AADFF_CHECK_ARG(centre_mode == 0 || (surf_chief && u_chief && spp_chief > 0), "psf_points: chief-ray centre needs surf_chief/u_chief");
    AADFF_CHECK_ARG(S > 0 && S <= 65535 && N > 0 && L > 0 && L <= 65535 && spp > 0, "psf_points: bad sizes S=%d N=%d L=%d spp=%d", S, N, L, spp);
    AADFF_CHECK_ARG(ks >= 1 && ks <= AADFF_MAX_KS, "psf_points: ks %d outside [1,%d]", ks, AADFF_MAX_KS);
    AADFF_CHECK_ARG(lc.n_surf > 0 && lc.n_surf <= AADFF_MAX_SURF, "psf_points: n_surf %d", lc.n_surf);
    int map_grid = 0;
    if (map_layout) {
        map_grid = (int)lround(std::sqrt((double)N));
        AADFF_CHECK_ARG(map_grid * map_grid == N, "psf_points: psf_map layout needs N = g*g, got %d", N);
    }
    StageArgs sa{};
    if (stage && stage->first_slice < S) {
        AADFF_CHECK_ARG(stage->src_host && stage->dst_dev && stage->counters, "psf_points_staged: NULL pointer in aadff_stage_t");
        AADFF_CHECK_ARG(stage->first_slice >= 0 && stage->slice_stride > 0 && (stage->slice_stride & 3) == 0,
                        "psf_points_staged: slice_stride %ld must be a positive multiple of 4", stage->slice_stride);
        AADFF_CHECK_ARG((((uintptr_t)stage->src_host | (uintptr_t)stage->dst_dev) & 15) == 0, "psf_points_staged: blocks must be 16-byte aligned");
        AADFF_CHECK_ARG(S < 65535, "psf_points_staged: S=%d", S);
        void* mapped;
        if (const int rc = mapped_host_pointer(stage->src_host, "psf_points_staged: src_host is", &mapped)) return rc;
        sa.src = reinterpret_cast<const float4*>(mapped);
        sa.dst = reinterpret_cast<float4*>(stage->dst_dev);
        sa.slice_n4 = stage->slice_stride >> 2;
        sa.first_slice = stage->first_slice;
        sa.copy_wgs = (int)std::min<long>(std::min<long>(AADFF_STAGE_COPY_WGS, (long)N * L), (sa.slice_n4 + kPsfThreads - 1) / kPsfThreads);
        sa.counters = stage->counters;
        sa.target = stage->generation * (unsigned)sa.copy_wgs;
        // the late path re-bases u_main / u_chief from dst_dev onto src_host: both must point into the staged block
        const float* lo = stage->dst_dev;
        const float* hi = stage->dst_dev + (long)S * stage->slice_stride;
        AADFF_CHECK_ARG(u_main >= lo && u_main < hi && (!u_chief || (u_chief >= lo && u_chief < hi)),
                        "psf_points_staged: u_main/u_chief must point into dst_dev[0 .. S*slice_stride)");
    }
    const int trace_mode = psf_trace_mode();
    const float* fit_c = nullptr;
    if (fit_weights && centre_mode == 1 && spp_chief >= 4 * kChiefRays && !psf_chief_full()) {
        AADFF_CHECK_ARG(fit_centres, "psf_points_fit: fit_weights without fit_centres");
        const int per_l = chief_centres_per_wavelength();
        hipLaunchKernelGGL(chief_fit_centres_kernel, dim3((N + kNodeWaves - 1) / kNodeWaves, per_l ? L : 1, S), dim3(kNodeWaves * 64), 0, (hipStream_t)stream,
                           points, N, L, surf_main, surf_chief, lc, states, fit_weights, trace_mode, per_l, fit_centres);
        AADFF_CHECK_LAUNCH();
        fit_c = fit_centres;
    }
    // points in place of draws: fit launches only (a launch that traces every chief ray is the launch of before, staging included)
    const bool pts = fit_c && pupil_xy && !psf_points_raw();
    if (pts) {
        main_stride_l = chief_stride_l = 2 * (long)spp + 2 * (long)spp_chief;
        main_stride_s = chief_stride_s = L * main_stride_l;
        u_main = pupil_xy;
        u_chief = pupil_xy + 2 * (long)spp;
        sa.src = nullptr;                                                // no copy plane, no wait: nothing reads the staged draws
        sa.dst = nullptr;
    }
    hipEvent_t ev0 = g_time_start, ev1 = g_time_stop;                    // aadff_time_next_launch
    g_time_start = g_time_stop = nullptr;
    // six instances of one kernel: with or without the events of aadff_time_next_launch; without fitted centres, with them, and with them
    // and pupil points
    const auto kern = pts   ? (ev0 ? psf_points_kernel<true, true, true> : psf_points_kernel<false, true, true>)
                    : fit_c ? (ev0 ? psf_points_kernel<true, true> : psf_points_kernel<false, true>)
                            : (ev0 ? psf_points_kernel<true, false> : psf_points_kernel<false, false>);
    if (ev0)
        hipExtLaunchKernelGGL(kern, dim3(N, L, sa.src ? S + 1 : S), dim3(kPsfThreads), (size_t)ks * ks * sizeof(float), (hipStream_t)stream,
                              ev0, ev1, 0, points, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l, u_chief,
                              spp_chief, chief_stride_s, chief_stride_l, make_splat_geom(lc.pixel_size, ks), centre_mode, map_grid, psf,
                              centre_out_or_null, flags_or_null, sa, trace_mode, fit_c);
    else
        hipLaunchKernelGGL(kern, dim3(N, L, sa.src ? S + 1 : S), dim3(kPsfThreads), (size_t)ks * ks * sizeof(float), (hipStream_t)stream, points, N, L, surf_main,
                           surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l, u_chief, spp_chief, chief_stride_s,
                           chief_stride_l, make_splat_geom(lc.pixel_size, ks),
                           centre_mode, map_grid, psf, centre_out_or_null, flags_or_null, sa, trace_mode, fit_c);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_psf_points(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                     const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                     int spp_chief, long chief_stride_s, long chief_stride_l, int ks, int centre_mode,
                     int map_layout, float* psf, float* centre_out_or_null, int* flags_or_null,
                     aadff_stream_t stream) {
    return psf_points_launch(points, S, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l,
                             u_chief, spp_chief, chief_stride_s, chief_stride_l, ks, centre_mode, map_layout, psf,
                             centre_out_or_null, flags_or_null, nullptr, nullptr, nullptr, nullptr, stream);
}

int aadff_psf_points_fit(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                         const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                         const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                         int spp_chief, long chief_stride_s, long chief_stride_l, int ks, int centre_mode,
                         int map_layout, float* psf, float* centre_out_or_null, int* flags_or_null,
                         const float* fit_weights_or_null, float* fit_centres, aadff_stream_t stream) {
    return psf_points_launch(points, S, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l,
                             u_chief, spp_chief, chief_stride_s, chief_stride_l, ks, centre_mode, map_layout, psf,
                             centre_out_or_null, flags_or_null, nullptr, fit_weights_or_null, fit_centres, nullptr, stream);
}

int aadff_psf_points_staged(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                            const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                            const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                            int spp_chief, long chief_stride_s, long chief_stride_l, int ks, int centre_mode,
                            int map_layout, float* psf, float* centre_out_or_null, int* flags_or_null,
                            const aadff_stage_t* stage, aadff_stream_t stream) {
    AADFF_CHECK_ARG(stage, "psf_points_staged: NULL stage");
    return psf_points_launch(points, S, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l,
                             u_chief, spp_chief, chief_stride_s, chief_stride_l, ks, centre_mode, map_layout, psf,
                             centre_out_or_null, flags_or_null, stage, nullptr, nullptr, nullptr, stream);
}

int aadff_psf_points_staged_fit(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                                const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                                const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                                int spp_chief, long chief_stride_s, long chief_stride_l, int ks, int centre_mode,
                                int map_layout, float* psf, float* centre_out_or_null, int* flags_or_null,
                                const aadff_stage_t* stage, const float* fit_weights_or_null, float* fit_centres, aadff_stream_t stream) {
    AADFF_CHECK_ARG(stage, "psf_points_staged_fit: NULL stage");
    return psf_points_launch(points, S, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l,
                             u_chief, spp_chief, chief_stride_s, chief_stride_l, ks, centre_mode, map_layout, psf,
                             centre_out_or_null, flags_or_null, stage, fit_weights_or_null, fit_centres, nullptr, stream);
}

int aadff_psf_points_fit_pts(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                             const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                             const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                             int spp_chief, long chief_stride_s, long chief_stride_l, int ks, int centre_mode,
                             int map_layout, float* psf, float* centre_out_or_null, int* flags_or_null,
                             const float* fit_weights_or_null, float* fit_centres, const float* pupil_xy_or_null, aadff_stream_t stream) {
    return psf_points_launch(points, S, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l,
                             u_chief, spp_chief, chief_stride_s, chief_stride_l, ks, centre_mode, map_layout, psf,
                             centre_out_or_null, flags_or_null, nullptr, fit_weights_or_null, fit_centres, pupil_xy_or_null, stream);
}

int aadff_psf_points_staged_fit_pts(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                                    const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                                    const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                                    int spp_chief, long chief_stride_s, long chief_stride_l, int ks, int centre_mode,
                                    int map_layout, float* psf, float* centre_out_or_null, int* flags_or_null,
                                    const aadff_stage_t* stage, const float* fit_weights_or_null, float* fit_centres,
                                    const float* pupil_xy_or_null, aadff_stream_t stream) {
    AADFF_CHECK_ARG(stage, "psf_points_staged_fit_pts: NULL stage");
    return psf_points_launch(points, S, N, L, surf_main, surf_chief, lc, states, u_main, spp, main_stride_s, main_stride_l,
                             u_chief, spp_chief, chief_stride_s, chief_stride_l, ks, centre_mode, map_layout, psf,
                             centre_out_or_null, flags_or_null, stage, fit_weights_or_null, fit_centres, pupil_xy_or_null, stream);
}

// the weights of a stack's chief draws and, with pa.xy, the pupil points of its main and chief draws: one launch
static int chief_fit_prologue_launch(const char* who, const float* u_chief, int S, int L, int spp_chief, long chief_stride_s, long chief_stride_l,
                                     const aadff_stage_t* stage_or_null, float* weights, PupilArgs pa, aadff_stream_t stream) {
    AADFF_CHECK_ARG(u_chief && weights, "%s: NULL pointer", who);
    AADFF_CHECK_ARG(S > 0 && S <= 65535 && L > 0 && L <= 65535 && spp_chief > 0, "%s: bad sizes S=%d L=%d spp_chief=%d", who, S, L, spp_chief);
    const float* u_late = u_chief;
    int late_from = S;
    pa.u_main_late = pa.u_main;
    if (stage_or_null && stage_or_null->first_slice < S) {
        // the draws of the states >= first_slice are still on the host when this kernel runs: read them where the late path of the
        // PSF launch does, at u_chief's (and u_main's) place in the mapped pinned block
        const aadff_stage_t* stage = stage_or_null;
        AADFF_CHECK_ARG(stage->src_host && stage->dst_dev && stage->first_slice >= 0 && stage->slice_stride > 0, "%s: bad aadff_stage_t", who);
        AADFF_CHECK_ARG(u_chief >= stage->dst_dev && u_chief < stage->dst_dev + (long)S * stage->slice_stride,
                        "%s: u_chief must point into dst_dev[0 .. S*slice_stride)", who);
        AADFF_CHECK_ARG(!pa.xy || (pa.u_main >= stage->dst_dev && pa.u_main < stage->dst_dev + (long)S * stage->slice_stride),
                        "%s: u_main must point into dst_dev[0 .. S*slice_stride)", who);
        void* mapped;
        if (const int rc = mapped_host_pointer(stage->src_host, "chief_fit_weights: src_host is", &mapped)) return rc;
        u_late = reinterpret_cast<const float*>(mapped) + (u_chief - stage->dst_dev);
        if (pa.xy) pa.u_main_late = reinterpret_cast<const float*>(mapped) + (pa.u_main - stage->dst_dev);
        late_from = stage->first_slice;
    }
    if (pa.xy)
        hipLaunchKernelGGL(chief_fit_weights_kernel<true>, dim3(L, S, 2), dim3(kFitThreads), 0, (hipStream_t)stream, u_chief, u_late, late_from, L, spp_chief,
                           chief_stride_s, chief_stride_l, weights, pa);
    else
        hipLaunchKernelGGL(chief_fit_weights_kernel<false>, dim3(L, S), dim3(kFitThreads), 0, (hipStream_t)stream, u_chief, u_late, late_from, L, spp_chief,
                           chief_stride_s, chief_stride_l, weights, pa);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_chief_fit_weights(const float* u_chief, int S, int L, int spp_chief, long chief_stride_s, long chief_stride_l,
                            const aadff_stage_t* stage_or_null, float* weights, aadff_stream_t stream) {
    return chief_fit_prologue_launch("chief_fit_weights", u_chief, S, L, spp_chief, chief_stride_s, chief_stride_l, stage_or_null, weights, PupilArgs{}, stream);
}

int aadff_chief_fit_prologue(const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief, int S, int L, int spp_chief,
                             long chief_stride_s, long chief_stride_l, aadff_lens_const_t lc, const aadff_stage_t* stage_or_null, float* weights,
                             float* pupil_xy, aadff_stream_t stream) {
    AADFF_CHECK_ARG(u_main && pupil_xy && spp > 0, "chief_fit_prologue: NULL pointer or spp=%d", spp);
    PupilArgs pa{};
    if (!psf_points_raw()) {                                             // (raw: the PSF launch will not read the points)
        pa.u_main = u_main; pa.main_ss = main_stride_s; pa.main_sl = main_stride_l; pa.spp = spp;
        pa.enp_r2 = lc.enp_r2; pa.enp_r2_shrunk = lc.enp_r2_shrunk; pa.xy = pupil_xy;
    }
    return chief_fit_prologue_launch("chief_fit_prologue", u_chief, S, L, spp_chief, chief_stride_s, chief_stride_l, stage_or_null, weights, pa, stream);
}

int aadff_chief_fit_tables(double* node_xy, double* fit, double* fit_low) {
    AADFF_CHECK_ARG(node_xy && fit && fit_low, "chief_fit_tables: NULL pointer");
    std::memcpy(node_xy, h_chief_node_xy, sizeof(h_chief_node_xy));
    std::memcpy(fit, h_chief_fit, sizeof(h_chief_fit));
    std::memcpy(fit_low, h_chief_fit_low, sizeof(h_chief_fit_low));
    return 0;
}

int aadff_psf_points_edge(const float* points, int S, int N, int L, const aadff_surface_t* surf_main,
                          const aadff_surface_t* surf_chief, aadff_lens_const_t lc, const aadff_lens_state_t* states,
                          const float* u_main, int spp, long main_stride_s, long main_stride_l, const float* u_chief,
                          int spp_chief, long chief_stride_s, long chief_stride_l, int ks, float delta_mm, float* raw,
                          float* centre_out, float* slope_out_or_null, unsigned* edge_count, unsigned* edge_list, int edge_cap,
                          int* flags_or_null, aadff_stream_t stream) {
#if defined(AADFF_PSF_SCALAR) || defined(AADFF_PSF_NO_COMPACT) || defined(AADFF_PSF_SWITCH_LOOP)
    set_error("psf_points_edge: not part of the measurement builds of the trace kernels");
    return AADFF_EUNSUPPORTED;
#else
    AADFF_CHECK_ARG(points && surf_main && surf_chief && states && u_main && u_chief && raw && centre_out && edge_count && edge_list,
                    "psf_points_edge: NULL pointer");
    AADFF_CHECK_ARG(S > 0 && S <= 65535 && N > 0 && N <= 65535 && L > 0 && L <= 65535 && spp > 0 && spp <= 65536 && spp_chief > 0,
                    "psf_points_edge: bad sizes S=%d N=%d L=%d spp=%d spp_chief=%d (point and sample ids are 16 bits each)", S, N, L, spp, spp_chief);
    AADFF_CHECK_ARG(ks >= 1 && ks <= AADFF_MAX_KS, "psf_points_edge: ks %d outside [1,%d]", ks, AADFF_MAX_KS);
    AADFF_CHECK_ARG(lc.n_surf > 0 && lc.n_surf <= AADFF_MAX_SURF, "psf_points_edge: n_surf %d", lc.n_surf);
    AADFF_CHECK_ARG(delta_mm >= 0.f && edge_cap >= 1, "psf_points_edge: delta %g mm, capacity %d", (double)delta_mm, edge_cap);
    hipStream_t st = (hipStream_t)stream;
    AADFF_CHECK_HIP(hipMemsetAsync(edge_count, 0, (size_t)S * L * sizeof(unsigned), st));
    EdgeArgs e{};
    e.delta = delta_mm; e.count = edge_count; e.list = edge_list; e.cap = edge_cap; e.raw = raw; e.slope = slope_out_or_null;
    hipLaunchKernelGGL(psf_points_edge_kernel, dim3(N, L, S), dim3(kPsfThreads), (size_t)ks * ks * sizeof(float), st, points, N, L, surf_main, surf_chief, lc,
                       states, u_main, spp, main_stride_s, main_stride_l, u_chief, spp_chief, chief_stride_s, chief_stride_l,
                       make_splat_geom(lc.pixel_size, ks), 1, centre_out, flags_or_null, e);
    AADFF_CHECK_LAUNCH();
    return 0;
#endif
}

int aadff_psf_normalise(const float* raw, int S, int N, int L, float pixel_size, int ks, int map_layout, float* psf, aadff_stream_t stream) {
    AADFF_CHECK_ARG(raw && psf, "psf_normalise: NULL pointer");
    AADFF_CHECK_ARG(S > 0 && S <= 65535 && N > 0 && L > 0 && L <= 65535 && ks >= 1 && ks <= AADFF_MAX_KS, "psf_normalise: bad sizes S=%d N=%d L=%d ks=%d", S, N, L, ks);
    int map_grid = 0;
    if (map_layout) {
        map_grid = (int)lround(std::sqrt((double)N));
        AADFF_CHECK_ARG(map_grid * map_grid == N, "psf_normalise: psf_map layout needs N = g*g, got %d", N);
    }
    hipLaunchKernelGGL(psf_normalise_kernel, dim3(N, L, S), dim3(kPsfThreads), (size_t)ks * ks * sizeof(float), (hipStream_t)stream, raw, N, L,
                       make_splat_geom(pixel_size, ks), map_grid, psf);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_refocus(const float* depth, int S, const float* u, int spp, long u_stride_s,
                  const aadff_surface_t* surf_green, aadff_lens_const_t lc, aadff_lens_state_t* states,
                  aadff_stream_t stream) {
    AADFF_CHECK_ARG(depth && u && surf_green && states, "refocus: NULL pointer");
    AADFF_CHECK_ARG(S > 0 && spp > 0 && lc.n_surf > 0 && lc.n_surf <= AADFF_MAX_SURF, "refocus: bad sizes S=%d spp=%d", S, spp);
    hipLaunchKernelGGL((refocus_kernel<kRefocusThreads, 1>), dim3(S), dim3(kRefocusThreads), 0, (hipStream_t)stream, depth, u, spp, u_stride_s, surf_green, lc, states, 1, S,
                       (const float*)nullptr, (float*)nullptr, 0L, (RefocusScratch*)nullptr);
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_refocus_staged(const float* depth, int S, const float* u_host, float* u_dev, long n_u, int spp,
                         long u_stride_s, const aadff_surface_t* surf_green, aadff_lens_const_t lc,
                         aadff_lens_state_t* states, void* scratch, aadff_stream_t stream) {
    AADFF_CHECK_ARG(depth && u_host && u_dev && surf_green && states && scratch, "refocus_staged: NULL pointer");
    AADFF_CHECK_ARG(S > 0 && spp > 0 && lc.n_surf > 0 && lc.n_surf <= AADFF_MAX_SURF, "refocus_staged: bad sizes S=%d spp=%d", S, spp);
    AADFF_CHECK_ARG(n_u >= 0, "refocus_staged: n_u %ld", n_u);
    AADFF_CHECK_ARG((((uintptr_t)u_host | (uintptr_t)u_dev) & 15) == 0, "refocus_staged: u_host/u_dev must be 16-byte aligned");
    void* mapped;
    if (const int rc = mapped_host_pointer(u_host, "refocus_staged: u_host is", &mapped)) return rc;
    constexpr int NT = 256;
    const long n4 = n_u >> 2;
    const int copy_wgs = (int)std::min<long>(kStageWorkgroups * (kRefocusThreads / NT), std::max<long>(1, (n4 + NT - 1) / NT));
    hipLaunchKernelGGL((refocus_kernel<NT, kRefocusSplit>), dim3(S * kRefocusSplit + copy_wgs), dim3(NT), 0, (hipStream_t)stream, depth,
                       (const float*)mapped, spp, u_stride_s, surf_green, lc, states, 1, S, (const float*)mapped, u_dev, n_u,
                       reinterpret_cast<RefocusScratch*>(scratch));
    AADFF_CHECK_LAUNCH();
    return 0;
}

int aadff_post_computation(int S, const aadff_surface_t* surf_green, aadff_lens_const_t lc, aadff_lens_state_t* states,
                           aadff_stream_t stream) {
    AADFF_CHECK_ARG(surf_green && states, "post_computation: NULL pointer");
    AADFF_CHECK_ARG(S > 0 && lc.n_surf > 0 && lc.n_surf <= AADFF_MAX_SURF, "post_computation: bad sizes S=%d", S);
    hipLaunchKernelGGL((refocus_kernel<kRefocusThreads, 1>), dim3(S), dim3(kRefocusThreads), 0, (hipStream_t)stream, (const float*)nullptr,
                       (const float*)nullptr, 0, 0L, surf_green, lc, states, 0, S, (const float*)nullptr, (float*)nullptr, 0L,
                       (RefocusScratch*)nullptr);
    AADFF_CHECK_LAUNCH();
    return 0;
}

// mapped_host_pointer for callers of the library: the per-call API hands such addresses to aadff_refocus (2 x 2048 draws and the
// depth read over PCIe by one workgroup) and as `points` to aadff_psf_points_staged instead of queueing a copy in front of every launch.
int aadff_host_device_pointer(const void* host, void** dev_out) {
    AADFF_CHECK_ARG(host && dev_out, "host_device_pointer: NULL pointer");
    return mapped_host_pointer(host, "host_device_pointer:", dev_out);
}

__global__ void publish_flags_kernel(const int* __restrict__ flags, int* mirror) {
    if (threadIdx.x == 0) __hip_atomic_store(mirror, __hip_atomic_load(flags, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT),
                                             __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_SYSTEM);
}

int aadff_publish_flags(const int* flags_dev, int* mirror_host, aadff_stream_t stream) {
    AADFF_CHECK_ARG(flags_dev && mirror_host, "publish_flags: NULL pointer");
    void* mapped;
    if (const int rc = mapped_host_pointer(mirror_host, "publish_flags: mirror_host is", &mapped)) return rc;
    hipLaunchKernelGGL(publish_flags_kernel, dim3(1), dim3(64), 0, (hipStream_t)stream, flags_dev, reinterpret_cast<int*>(mapped));
    AADFF_CHECK_LAUNCH();
    return 0;
}

}  // extern "C"
