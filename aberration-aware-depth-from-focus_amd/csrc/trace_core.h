// The ray trace that trace.hip (PSF grid, refocus, bulk trace), lens_analysis.hip (spot moments, MTF) and render_rt.hip (ray-traced
// rendering) share: scalar one-ray-per-lane, packed two-rays-per-lane, their measurement switches (the Makefile's variant builds).
// One thread per ray; the surface table is wave-uniform (scalar loads, SGPR operands), so every branch on the surface kind is uniform.
// Spheres are intersected in closed form (the reference keeps Newton's root but discards its convergence mask for them,
// deeplens/surfaces.py:466); even aspheres run the reference's Newton iteration, whose loop exits per WAVE (`__any`) where the
// reference's exits per batch (`while (...).any()`, deeplens/surfaces.py:547) - extra steps on converged rays are the same arithmetic the
// reference performs.  Semantics: SURVEY.md Appendix A.1/A.2, citations per function below (paths relative to the reference repo).
#pragma once
#include <cmath>
#include "common.h"

namespace aadff {

constexpr float kEps = 1e-9f;            // deeplens/basics.py:34
constexpr float kMaxT = 1e5f;            // deeplens/basics.py:32
constexpr int kNewtonMaxIter = 10;       // deeplens/surfaces.py:26
constexpr float kTolTight = 10e-6f;      // deeplens/surfaces.py:27
constexpr float kTolLoose = 50e-6f;      // deeplens/surfaces.py:28
constexpr float kStepBound = 5.f;        // deeplens/surfaces.py:29
// fused kernels: a Newton update shorter than aadff_surface_t::newton_step_tol (<= 10 um, set per surface by the host from
// the surface's largest profile curvature) ends the loop (see newton2)
[[maybe_unused]] constexpr float kTwoPiHi = 3.14159274101257324f;   // (float)np.pi (libm sin/cos builds)

struct Ray {
    float ox, oy, oz, dx, dy, dz, ra;
};

// ---- arithmetic primitives -------------------------------------------------------------
// Default: hardware reciprocal / sqrt / rsqrt (1 ulp) instead of the IEEE-exact sequences (11
// instructions per division, ~10 per sqrt).  Their error (~1e-7 relative on quantities of a few mm)
// is three orders below the fp32 noise the reference itself carries at the first surface (one ulp of
// t ~ 1500 mm is 1.2e-4 mm); -DAADFF_TRACE_IEEE restores the exact forms.
#ifdef AADFF_TRACE_IEEE
__device__ __forceinline__ float frcp(float x) { return 1.f / x; }
__device__ __forceinline__ float fsqrt(float x) { return sqrtf(x); }
__device__ __forceinline__ float frsq(float x) { return 1.f / sqrtf(x); }
__device__ __forceinline__ float fdiv(float a, float b) { return a / b; }
#else
__device__ __forceinline__ float frcp(float x) { return __builtin_amdgcn_rcpf(x); }
__device__ __forceinline__ float fsqrt(float x) { return __builtin_amdgcn_sqrtf(x); }
__device__ __forceinline__ float frsq(float x) { return __builtin_amdgcn_rsqf(x); }
__device__ __forceinline__ float fdiv(float a, float b) { return a * __builtin_amdgcn_rcpf(b); }
#endif

// ---- even-asphere sag and d(sag)/d(r^2): deeplens/surfaces.py:787-830 ----
// sag = c r^2 / (1 + sf) + sum a_j r^(2j),  sf = sqrt(1 - (1+k) c^2 r^2).  The reference's expression for
// the conic part of d(sag)/d(r^2), (1 + sf + (1+k) r^2 c^2 / (2 sf)) c / (1 + sf)^2, is identically
// c / (2 sf); the closed form is used here (one reciprocal instead of two divisions).
__device__ __forceinline__ void sag_and_slope(const aadff_surface_t& s, float r2, float& sag, float& slope) {
    const float a = (1.f + s.k) * r2 * (s.c * s.c);
    const float sf = fsqrt(1.f - a);
    sag = r2 * s.c * frcp(1.f + sf);
    slope = 0.5f * s.c * frcp(sf);
    if (s.n_ai > 0) {
        // sum a_j r2^j and its derivative by Horner (the reference's power form, surfaces.py:799,823, differs
        // by rounding of terms that are < 1e-3 of the sag); derivative coefficients (j+1) a_j come from the table
        float ps, pd;
        if (s.n_ai <= 6) {
            ps = s.ai[5]; pd = s.dai[5];
#pragma unroll
            for (int j = 4; j >= 0; --j) { ps = ps * r2 + s.ai[j]; pd = pd * r2 + s.dai[j]; }
        } else {
            ps = s.ai[AADFF_MAX_AI - 1]; pd = s.dai[AADFF_MAX_AI - 1];
#pragma unroll
            for (int j = AADFF_MAX_AI - 2; j >= 0; --j) { ps = ps * r2 + s.ai[j]; pd = pd * r2 + s.dai[j]; }
        }
        sag += ps * r2;
        slope += pd;
    }
}

__device__ __forceinline__ float dsag_dr2(const aadff_surface_t& s, float r2) {
    float sag, slope;
    sag_and_slope(s, r2, sag, slope);
    return slope;
}

// ---- validity masks: deeplens/surfaces.py:724-743 ----
__device__ __forceinline__ bool valid_strict(const aadff_surface_t& s, float r2) {
    return s.k_gt_m1 ? (r2 < s.r2 && r2 < s.r2_shape) : (r2 < s.r2);
}
__device__ __forceinline__ bool valid_loose(const aadff_surface_t& s, float r2) {
    return s.k_gt_m1 ? (r2 < s.r2_shape) : (r2 > 0.f);
}

// ---- Newton intersection: deeplens/surfaces.py:523-586.  Called by alive lanes only. ----
template <bool STRICT>
__device__ __forceinline__ float newton_step(const aadff_surface_t& s, const Ray& r, float dxy2, float od, float& t) {
    const float px = r.ox + r.dx * t, py = r.oy + r.dy * t, pz = r.oz + r.dz * t;
    float r2 = px * px + py * py;
    const bool m = STRICT ? valid_strict(s, r2) : valid_loose(s, r2);
    r2 = m ? r2 : 0.f;                                   // x*valid, y*valid
    float sag, slope;
    sag_and_slope(s, r2, sag, slope);
    const float ft = sag + s.d - pz;
    const float dr2dt = 2.f * (dxy2 * t + od);
    const float dfdt = slope * dr2dt - r.dz;
    float step = fdiv(ft, dfdt + kEps);
    step = fminf(fmaxf(step, -kStepBound), kStepBound);
    t -= step;
    return ft;
}

// Root of the ray with the CONIC part of the surface, measured from the vertex-plane point p0 = o + d t0:
//   c (1 + k dz^2) tau^2 + 2 beta tau + c rho^2 = 0,  beta = c (p0x dx + p0y dy) - dz,  rho^2 = p0x^2 + p0y^2
// (from c (1+k) z^2 - 2 z + c r^2 = 0 with z = dz tau); the root next to the vertex plane in cancellation-free
// form.  k = 0 is the sphere.  Returns false when the ray misses the conic.
__device__ __forceinline__ bool conic_root(const aadff_surface_t& s, const Ray& r, float t0, float& p0x, float& p0y, float& tau) {
    p0x = r.ox + r.dx * t0; p0y = r.oy + r.dy * t0;
    const float rho2 = p0x * p0x + p0y * p0y;
    const float beta = s.c * (p0x * r.dx + p0y * r.dy) - r.dz;
    const float A = s.c * (1.f + s.k * r.dz * r.dz);
    const float disc = beta * beta - A * (s.c * rho2);
    const float root = fsqrt(fmaxf(disc, 0.f));
    tau = fdiv(s.c * rho2, beta < 0.f ? (root - beta) : -(root + beta));
    return disc >= 0.f;
}

__device__ __forceinline__ void newton(const aadff_surface_t& s, const Ray& r, float& t_out, bool& valid_out, int& nan_flag) {
    const float dxy2 = r.dx * r.dx + r.dy * r.dy;
    const float od = r.dx * r.ox + r.dy * r.oy;
    const float t0 = fdiv(s.d - r.oz, r.dz);
    float t = t0;
#ifndef AADFF_NEWTON_PLANE_START
    // start from the conic root instead of the vertex plane (surfaces.py:543): Newton then only has to absorb
    // the polynomial departure (1-2 steps instead of 3-4) and reaches the same root within its tolerance
    {
        float p0x, p0y, tau;
        if (conic_root(s, r, t0, p0x, p0y, tau)) t = t0 + tau;
    }
#endif
    float ft = kMaxT;
    for (int it = 0; it < kNewtonMaxIter; ++it) {
        if (!__any(fabsf(ft) > kTolLoose)) break;
        ft = newton_step<false>(s, r, dxy2, od, t);
        if (ft != ft) nan_flag = 1;
    }
    const float t1 = t - t0;
    t = t0 + t1;                                         // surfaces.py:565-569 (not an fp32 identity)
    ft = newton_step<true>(s, r, dxy2, od, t);
    const float px = r.ox + r.dx * t, py = r.oy + r.dy * t;
    valid_out = valid_strict(s, px * px + py * py) && (fabsf(ft) < kTolTight) && (t > 0.f);
    t_out = t;
}

// ---- vector Snell refraction with the surface normal: deeplens/surfaces.py:589-679 ----
// KEEP = true: a ray that fails keeps its direction (the reference leaves dead rays untouched and the
// generic trace API exposes them); KEEP = false (fused PSF / refocus kernels): dead rays are never read
// again, so nothing is preserved.
// Sphere normal: the reference normalises +-2 (x, y, z - (d + R)); since |p - centre| = |R| on the sphere
// that unit vector is exactly (c x, c y, c (z - d) - 1) for either sign of c -> no normalisation needed.
// Refracted direction sr n + eta (d - cosi n) is evaluated as eta d + (sr - eta cosi) n.
template <bool KEEP>
__device__ __forceinline__ void refract(const aadff_surface_t& s, Ray& r, bool forward) {
    float nx, ny, nz;
    if (s.kind == AADFF_SURF_STOP) {
        nx = 0.f; ny = 0.f; nz = -1.f;
    } else if (s.kind == AADFF_SURF_SPHERIC) {
        nx = s.c * r.ox; ny = s.c * r.oy; nz = s.c * (r.oz - s.d) - 1.f;
    } else {
        const float g = dsag_dr2(s, r.ox * r.ox + r.oy * r.oy);
        nx = g * 2.f * r.ox; ny = g * 2.f * r.oy; nz = -1.f;
        const float inv = frsq(fmaxf(nx * nx + ny * ny + 1.f, 1e-24f));           // F.normalize
        nx *= inv; ny *= inv; nz = -inv;
    }
    // forward rays use -n (surfaces.py:654-655): fold the sign into cosi and the final combination
    const float sgn = forward ? -1.f : 1.f;
    const float eta = forward ? s.eta_fwd : s.eta_bwd;
    const float eta2 = forward ? s.eta_fwd2 : s.eta_bwd2;
    const float cosi = sgn * (r.dx * nx + r.dy * ny + r.dz * nz);
    const float sin2 = eta2 * (1.f - cosi * cosi);
    const bool valid = (cosi * cosi > 0.1f) && (sin2 < 1.f);
    const float g = sgn * (fsqrt(fmaxf(1.f - sin2, 0.f)) - eta * cosi);
    if (KEEP) {
        if (valid) {
            r.dx = eta * r.dx + g * nx; r.dy = eta * r.dy + g * ny; r.dz = eta * r.dz + g * nz;
        } else {
            r.ra = 0.f;
        }
    } else {
        r.dx = eta * r.dx + g * nx; r.dy = eta * r.dy + g * ny; r.dz = eta * r.dz + g * nz;
        r.ra = valid ? r.ra : 0.f;
    }
}

// ---- one surface interaction: deeplens/surfaces.py:391-520 (dead rays are skipped) ----
template <bool KEEP>
__device__ __forceinline__ void react(const aadff_surface_t& s, Ray& r, bool forward, int& nan_flag) {
    if (!(r.ra > 0.f)) return;
    float t, px, py, pz;
    bool valid;
    if (s.kind == AADFF_SURF_STOP) {
        t = fdiv(s.d - r.oz, r.dz);
        px = r.ox + t * r.dx; py = r.oy + t * r.dy; pz = r.oz + t * r.dz;
        valid = fsqrt(px * px + py * py) <= s.r;
#ifndef AADFF_SPHERE_NEWTON
    } else if (s.kind == AADFF_SURF_SPHERIC) {
        // Sphere (k = 0, no polynomial): closed-form root instead of the reference's Newton iteration
        // (deeplens/surfaces.py:456-487 keeps Newton's t but DISCARDS its convergence mask, so only the root
        // matters).  From the vertex-plane point p0 = o + d*t0 the sphere |p - (0,0,d+R)| = R reads
        //   tau^2 + 2 b tau + rho^2 = 0,  rho^2 = p0x^2 + p0y^2,  b = p0x dx + p0y dy - R dz,
        // whose root next to the vertex plane is, in cancellation-free form and scaled by c = 1/R,
        //   tau = c rho^2 / (-beta + sgn(-beta) sqrt(beta^2 - c^2 rho^2)),   beta = c (p0x dx + p0y dy) - dz.
        const float t0 = fdiv(s.d - r.oz, r.dz);
        float p0x, p0y, tau;
        const bool hit = conic_root(s, r, t0, p0x, p0y, tau);
        t = t0 + tau;
        px = p0x + r.dx * tau; py = p0y + r.dy * tau; pz = s.d + r.dz * tau;
        valid = hit && (px * px + py * py <= s.r2) && (t >= 0.f);
#endif
    } else {
        bool nvalid;
        newton(s, r, t, nvalid, nan_flag);
        px = r.ox + t * r.dx; py = r.oy + t * r.dy; pz = r.oz + t * r.dz;
        valid = s.kind == AADFF_SURF_SPHERIC ? ((px * px + py * py <= s.r2) && (t >= 0.f))   // Newton's own mask is discarded (:466)
                                             : nvalid;
    }
    if (KEEP) {
        if (!valid) { r.ra = 0.f; return; }
        r.ox = px; r.oy = py; r.oz = pz;
    } else {
        r.ox = px; r.oy = py; r.oz = pz;
        if (!valid) { r.ra = 0.f; return; }
    }
    if (s.kind != AADFF_SURF_STOP || (forward ? s.refract_fwd : s.refract_bwd)) refract<KEEP>(s, r, forward);
}

template <bool KEEP>
__device__ __forceinline__ void trace_range(const aadff_surface_t* __restrict__ surf, int first, int last, bool forward,
                                            Ray& r, int& nan_flag) {
    if (forward)
        for (int i = first; i < last; ++i) react<KEEP>(surf[i], r, true, nan_flag);
    else
        for (int i = last - 1; i >= first; --i) react<KEEP>(surf[i], r, false, nan_flag);
}

__device__ __forceinline__ void propagate_to(Ray& r, float z) {      // deeplens/basics.py:255-273 (all rays)
    const float t = fdiv(z - r.oz, r.dz);
    r.ox += r.dx * t; r.oy += r.dy * t; r.oz += r.dz * t;
}

__device__ __forceinline__ void normalize3(float& x, float& y, float& z) {
    const float inv = frsq(fmaxf(x * x + y * y + z * z, 1e-24f));
    x *= inv; y *= inv; z *= inv;
}

// pupil / disc sample from two raw uniforms: deeplens/optics.py:480-485, surfaces.py:192-195
__device__ __forceinline__ void disc_sample(float u_theta, float u_r, float R2, float& x, float& y) {
    const float rr = fsqrt(u_r * R2);
#ifndef AADFF_LIBM_SINCOS
    // v_sin_f32 / v_cos_f32 take their argument in revolutions: cos(2*pi*u) in one instruction each.  The
    // reference evaluates cos(fp32(u*2*pi)); both forms differ from the exact angle by ~4e-7 rad, i.e. < 1e-5 mm
    // at the pupil rim (measured: rendered-image parity unchanged); -DAADFF_LIBM_SINCOS restores cosf/sinf.
    x = rr * __builtin_amdgcn_cosf(u_theta);
    y = rr * __builtin_amdgcn_sinf(u_theta);
#else
    const float theta = u_theta * 2.f * kTwoPiHi;
    x = rr * cosf(theta);
    y = rr * sinf(theta);
#endif
}

__device__ __forceinline__ Ray ray_to(float px, float py, float pz, float tx, float ty, float tz) {
    Ray r;
    r.ox = px; r.oy = py; r.oz = pz;
    r.dx = tx - px; r.dy = ty - py; r.dz = tz - pz;
    normalize3(r.dx, r.dy, r.dz);
    r.ra = 1.f;
    return r;
}

// ------------------------------------------------------------------------------------
// Two rays per lane (fused PSF kernel only).  Every quantity is a float2 whose components belong to two
// independent rays, so nearly all arithmetic issues as packed fp32 (v_pk_fma/mul/add_f32: two rays per
// 4-cycle instruction instead of one ray per ~3-cycle instruction); only the transcendentals, compares
// and selects stay per component.  Same formulas as the scalar core above, KEEP = false semantics (a dead
// ray's state is never read again), masks are int2 (-1 / 0).
// ------------------------------------------------------------------------------------
typedef float f2 __attribute__((ext_vector_type(2)));
typedef int i2 __attribute__((ext_vector_type(2)));

struct Ray2 {
    f2 ox, oy, oz, dx, dy, dz, ra;
    i2 alive;          // validity while tracing (a lane mask: no per-surface compare/select); ra = alive ? 1 : 0 afterwards
};
__device__ __forceinline__ f2 f2s(float a) { return (f2){a, a}; }
__device__ __forceinline__ f2 vsqrt(f2 a) { return (f2){fsqrt(a.x), fsqrt(a.y)}; }
__device__ __forceinline__ f2 vrcp(f2 a) { return (f2){frcp(a.x), frcp(a.y)}; }
__device__ __forceinline__ f2 vrsq(f2 a) { return (f2){frsq(a.x), frsq(a.y)}; }
__device__ __forceinline__ f2 vmax(f2 a, f2 b) { return __builtin_elementwise_max(a, b); }
__device__ __forceinline__ f2 vmin(f2 a, f2 b) { return __builtin_elementwise_min(a, b); }
// max(x, 0) as ONE v_max_f32 per component (the generic form first canonicalises x: two instructions)
__device__ __forceinline__ f2 vmax0(f2 a) {
    float x, y;
    asm("v_max_f32 %0, 0, %1" : "=v"(x) : "v"(a.x));
    asm("v_max_f32 %0, 0, %1" : "=v"(y) : "v"(a.y));
    return (f2){x, y};
}
__device__ __forceinline__ f2 vabs(f2 a) { return __builtin_elementwise_abs(a); }
__device__ __forceinline__ f2 vsel(i2 m, f2 a, f2 b) { return (f2){m.x ? a.x : b.x, m.y ? a.y : b.y}; }
__device__ __forceinline__ bool any2(i2 m) { return (m.x | m.y) != 0; }

// sum a_j r2^j (to be multiplied by r2) and its r2-derivative, by Horner
__device__ __forceinline__ void poly2(const aadff_surface_t& s, f2 r2, f2& ps, f2& pd) {
    if (s.n_ai <= 6) {
        ps = f2s(s.ai[5]); pd = f2s(s.dai[5]);
#pragma unroll
        for (int j = 4; j >= 0; --j) { ps = ps * r2 + s.ai[j]; pd = pd * r2 + s.dai[j]; }
    } else {
        ps = f2s(s.ai[AADFF_MAX_AI - 1]); pd = f2s(s.dai[AADFF_MAX_AI - 1]);
#pragma unroll
        for (int j = AADFF_MAX_AI - 2; j >= 0; --j) { ps = ps * r2 + s.ai[j]; pd = pd * r2 + s.dai[j]; }
    }
}
__device__ __forceinline__ void sag_and_slope2(const aadff_surface_t& s, f2 r2, f2& sag, f2& slope) {
    const f2 a = (1.f + s.k) * r2 * (s.c * s.c);
#ifndef AADFF_NO_RSQ_SLOPE
    // 1/sf from one v_rsq and sf = (1 - a) / sf: one transcendental less per ray than sqrt + rcp (callers mask r2 so
    // that 1 - a >= 1e-9, valid_loose2 / valid_strict2)
    const f2 om = 1.f - a;
    const f2 isf = vrsq(om);
    const f2 sf = om * isf;
    sag = r2 * s.c * vrcp(1.f + sf);
    slope = (0.5f * s.c) * isf;
#else
    const f2 sf = vsqrt(1.f - a);
    sag = r2 * s.c * vrcp(1.f + sf);
    slope = (0.5f * s.c) * vrcp(sf);
#endif
    if (s.n_ai > 0) {
        f2 ps, pd;
        poly2(s, r2, ps, pd);
        sag += ps * r2;
        slope += pd;
    }
}
__device__ __forceinline__ i2 valid_strict2(const aadff_surface_t& s, f2 r2) {
    const i2 a = r2 < s.r2;
    return s.k_gt_m1 ? (a & (r2 < s.r2_shape)) : a;
}
__device__ __forceinline__ i2 valid_loose2(const aadff_surface_t& s, f2 r2) {
    return s.k_gt_m1 ? (r2 < s.r2_shape) : (r2 > 0.f);
}
// Paired core, vertex-plane form: every surface first moves the ray IN PLACE to the vertex plane z = d (origin p0,
// parameter tau from there: no cancellation for far objects), the kind-specific code only produces tau, a validity
// mask and the normal, and the common tail advances and refracts the ray in place -- the loop-carried ray state is
// never defined inside a branch, which saves the ~12 register copies per surface the branchy form cost.
template <bool STRICT>
__device__ __forceinline__ f2 newton_step2(const aadff_surface_t& s, const Ray2& r, f2 dxy2, f2 od, f2& tau, f2* slope_out = nullptr,
                                           f2* step_out = nullptr) {
    const f2 px = r.ox + r.dx * tau, py = r.oy + r.dy * tau;
    f2 r2 = px * px + py * py;
    const i2 m = STRICT ? valid_strict2(s, r2) : valid_loose2(s, r2);
    r2 = vsel(m, r2, f2s(0.f));
    f2 sag, slope;
    sag_and_slope2(s, r2, sag, slope);
    const f2 ft = sag - r.dz * tau;                      // sag + d - p_z with p_z = d + dz tau
    const f2 dr2dt = 2.f * (dxy2 * tau + od);
    const f2 dfdt = slope * dr2dt - r.dz;
    f2 step = ft * vrcp(dfdt + kEps);
    step = vmin(vmax(step, f2s(-kStepBound)), f2s(kStepBound));
    tau -= step;
    if (slope_out) *slope_out = slope;
    if (step_out) *step_out = step;
    return ft;
}
// conic root from the vertex-plane point (r.ox, r.oy, d)
template <bool SPHERE = false>                                  // SPHERE: kind SPHERIC implies k == 0 (Aspheric.kind())
__device__ __forceinline__ i2 conic_root2(const aadff_surface_t& s, const Ray2& r, f2& tau) {
    const f2 rho2 = r.ox * r.ox + r.oy * r.oy;
    const f2 beta = s.c * (r.ox * r.dx + r.oy * r.dy) - r.dz;
    const f2 A = SPHERE ? f2s(s.c) : s.c * (1.f + s.k * r.dz * r.dz);
    const f2 disc = beta * beta - A * (s.c * rho2);
    const f2 root = vsqrt(vmax0(disc));
#ifndef AADFF_NO_SIGNXFER
    // -(beta + sign(beta) root): the sign transfer is one v_bfi per ray where the two-sided form costs a compare and a
    // select each (beta = -0 exactly would pick the other root; beta is c (p0 . d) - dz with dz ~ 1)
    const f2 sroot = (f2){__builtin_copysignf(root.x, beta.x), __builtin_copysignf(root.y, beta.y)};
    tau = (s.c * rho2) * vrcp(-(beta + sroot));
#else
    tau = (s.c * rho2) * vrcp(vsel(beta < 0.f, root - beta, -(root + beta)));
#endif
    return disc >= 0.f;
}
// slope_out: d sag / d r^2 of the last (strict) step, i.e. one converged Newton update (<= 5e-5 mm, typically 1e-7)
// before the hit point; the fused kernels reuse it for the surface normal instead of evaluating the asphere again
// (relative change of the slope over that update <= 2e-6: below the fp32 noise of the trace; -DAADFF_NORMAL_REEVAL
// restores the literal evaluation at the hit point, surfaces.py:589-630).  r is at the vertex plane; t0 = distance
// travelled to get there (the reference's t > 0 test is on t0 + tau).
__device__ __forceinline__ void newton2(const aadff_surface_t& s, const Ray2& r, i2 alive, f2 t0, f2& tau_out, i2& valid_out, int& nan_flag,
                                        f2* slope_out = nullptr) {
    const f2 dxy2 = r.dx * r.dx + r.dy * r.dy;
    const f2 od = r.dx * r.ox + r.dy * r.oy;
    f2 tau = f2s(0.f);
#ifndef AADFF_NEWTON_PLANE_START
    i2 hit0;
    {
        f2 tc;
        hit0 = conic_root2(s, r, tc);
        tau = vsel(hit0, tc, f2s(0.f));
    }
#endif
    // The reference leaves its loop when the residual BEFORE the last update is below 5e-5 mm, i.e. it spends one
    // whole evaluation confirming a converged point, then takes its extra (strict) step.  A Newton update of length
    // `step` leaves a residual of f''/(2 f') x step^2 (f'' <= the largest curvature kappa of the surface profile, f' ~ -dz);
    // the host sets newton_step_tol = min(1e-2, sqrt(4e-6 / kappa)) mm per surface (deeplens/surfaces.py: pack), so that
    // this residual stays <= 3e-6 mm, 3x under the strict step's |residual| < 1e-5 test, for ANY lens file (kappa = 0.03/mm
    // gives the 10 um that the shipped 50 mm lenses run with); the strict step — a full Newton update like any other —
    // then takes the point to ~1e-12 mm: the confirming evaluation is skipped without moving the hit (with 1 um the rim
    // rays of nearly every wave forced one more whole evaluation).
    [[maybe_unused]] const float step_tol = s.newton_step_tol;
    f2 ft = f2s(kMaxT), step = f2s(kMaxT);
    i2 nanm = {0, 0};                                    // NaN seen in ANY residual (the reference exits on the first, surfaces.py:555)
#if !defined(AADFF_NEWTON_LITERAL_EXIT) && !defined(AADFF_NEWTON_CHECK_EVERY_STEP)
    // The first evaluation always runs (the reference enters its loop with ft = MAXT) and the second does whenever any
    // ray of the batch started more than 5e-5 mm off the surface, which from the conic root of an asphere is every
    // batch: run both without the wave-wide exit test, then continue under it.  (Steps on converged rays are no-ops
    // at the 1e-9 level, which is also what the reference's batch-wide loop does to them.)  A NaN residual does NOT
    // survive the updates (the step clamp is v_max/v_min: maxnum/minnum drop a NaN operand, where torch.clamp propagates
    // it), so every residual is tested as it is produced - one compare and a scalar OR each - and the flag is raised once.
#if !defined(AADFF_NEWTON_PLANE_START) && !defined(AADFF_NEWTON_GENERIC_FIRST)
    if (s.n_ai > 0 && !__any(any2(alive & ~hit0))) {
        // Every live ray of the wave starts ON the conic (tau = its conic root), where the residual is the polynomial
        // part alone, sag_conic = dz tau, and sf = sqrt(1 - (1+k) c^2 r^2) = 1 - (1+k) c dz tau: the first Newton step
        // needs no square root and no conic sag (30 instead of 74 instructions per lane); same update as the generic
        // evaluation up to rounding.
        const f2 px = r.ox + r.dx * tau, py = r.oy + r.dy * tau;
        const f2 r2 = px * px + py * py;
        f2 ps, pd;
        poly2(s, r2, ps, pd);
        ft = ps * r2;
        nanm |= ft != ft;
        const f2 sf = 1.f - ((1.f + s.k) * s.c) * (r.dz * tau);
        const f2 slope = (0.5f * s.c) * vrcp(sf) + pd;
        const f2 dfdt = slope * (2.f * (dxy2 * tau + od)) - r.dz;
        step = ft * vrcp(dfdt + kEps);
        step = vmin(vmax(step, f2s(-kStepBound)), f2s(kStepBound));
        tau -= step;
    } else
#endif
    {
        ft = newton_step2<false>(s, r, dxy2, od, tau, nullptr, &step);
        nanm |= ft != ft;
    }
    ft = newton_step2<false>(s, r, dxy2, od, tau, nullptr, &step);
    nanm |= ft != ft;
    for (int it = 2; it < kNewtonMaxIter; ++it) {
        if (!__any(any2(alive & (vabs(ft) > kTolLoose) & (vabs(step) > step_tol)))) break;
        ft = newton_step2<false>(s, r, dxy2, od, tau, nullptr, &step);
        nanm |= ft != ft;
    }
#else
    for (int it = 0; it < kNewtonMaxIter; ++it) {
#ifndef AADFF_NEWTON_LITERAL_EXIT
        if (!__any(any2(alive & (vabs(ft) > kTolLoose) & (vabs(step) > step_tol)))) break;
#else
        if (!__any(any2(alive & (vabs(ft) > kTolLoose)))) break;
#endif
        ft = newton_step2<false>(s, r, dxy2, od, tau, nullptr, &step);
        nanm |= ft != ft;
    }
#endif
    ft = newton_step2<true>(s, r, dxy2, od, tau, slope_out);
    nanm |= ft != ft;
    if (any2(alive & nanm)) nan_flag = 1;
    const f2 px = r.ox + r.dx * tau, py = r.oy + r.dy * tau;
    valid_out = valid_strict2(s, px * px + py * py) & (vabs(ft) < kTolTight) & (t0 + tau > 0.f);
    tau_out = tau;
}
// vector Snell refraction at a surface with unit normal (nx, ny, nz) (surfaces.py:633-679)
__device__ __forceinline__ i2 refract_dir2(const aadff_surface_t& s, Ray2& r, bool forward, f2 nx, f2 ny, f2 nz) {
    const float sgn = forward ? -1.f : 1.f;
    const float eta = forward ? s.eta_fwd : s.eta_bwd;
    const float eta2 = forward ? s.eta_fwd2 : s.eta_bwd2;
    const f2 cosi = sgn * (r.dx * nx + r.dy * ny + r.dz * nz);
    const f2 cos2 = cosi * cosi;
    // cos^2 i > 0.1 and eta^2 (1 - cos^2 i) < 1  <=>  cos^2 i > max(0.1, 1 - 1/eta^2)  (host-computed per surface)
    const i2 valid = cos2 > (forward ? s.cos2_min_fwd : s.cos2_min_bwd);
#ifndef AADFF_NO_FOLDED_SNELL
    const f2 k2 = eta2 * cos2 + (1.f - eta2);           // 1 - eta^2 (1 - cos^2 i) as one fma with wave-uniform constants
#else
    const f2 k2 = 1.f - eta2 * (1.f - cos2);
#endif
    const f2 g = sgn * (vsqrt(vmax0(k2)) - eta * cosi);
    r.dx = eta * r.dx + g * nx; r.dy = eta * r.dy + g * ny; r.dz = eta * r.dz + g * nz;
    return valid;
}
__device__ __forceinline__ void react2(const aadff_surface_t& s, Ray2& r, bool forward, int& nan_flag) {
    const i2 alive = r.alive;
#ifdef AADFF_SURFACE_SKIP
    // wave-uniform skip only: a per-lane early return turns the whole surface body into a divergent region whose
    // results are merged back with ~12 v_mov per surface (dead lanes just compute values nobody reads)
    if (!__any(any2(alive))) return;
#endif
    // (no skip at all by default: vignetted rays are scattered over the lanes, a wave with no live ray is a rarity
    // before the compaction and impossible after it, and the test costs two vector instructions per surface)
    // to the vertex plane, in place
    const f2 t0 = (s.d - r.oz) * vrcp(r.dz);
    r.ox += r.dx * t0; r.oy += r.dy * t0;
    f2 tau, nx, ny, nz;
    i2 valid;
    if (s.kind == AADFF_SURF_SPHERIC) {
        const i2 hit = conic_root2<true>(s, r, tau);
        valid = hit & (t0 + tau >= 0.f);
        r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + r.dz * tau;
        valid &= (r.ox * r.ox + r.oy * r.oy) <= s.r2;
        nx = s.c * r.ox; ny = s.c * r.oy; nz = (s.c * r.dz) * tau - 1.f;      // c (z - d) - 1 with z - d = dz tau
    } else if (s.kind == AADFF_SURF_STOP) {
        r.oz = f2s(s.d);
        valid = (r.ox * r.ox + r.oy * r.oy) <= s.r * s.r;           // sqrt(x^2+y^2) <= r (surfaces.py:418)
        nx = f2s(0.f); ny = f2s(0.f); nz = f2s(-1.f);
    } else {
        f2 g;
#ifndef AADFF_NORMAL_REEVAL
        newton2(s, r, alive, t0, tau, valid, nan_flag, &g);
        r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + r.dz * tau;
#else
        newton2(s, r, alive, t0, tau, valid, nan_flag);
        r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + r.dz * tau;
        f2 sag;
        sag_and_slope2(s, r.ox * r.ox + r.oy * r.oy, sag, g);
#endif
        nx = g * 2.f * r.ox; ny = g * 2.f * r.oy;
        const f2 inv = vrsq(vmax(nx * nx + ny * ny + 1.f, f2s(1e-24f)));
        nx *= inv; ny *= inv; nz = -inv;
    }
    valid &= alive;
    if (s.kind != AADFF_SURF_STOP || (forward ? s.refract_fwd : s.refract_bwd)) valid &= refract_dir2(s, r, forward, nx, ny, nz);
    r.alive = valid;
}
// ---- run-structured forward trace (default in the fused kernels) ---------------------------------------------------
// Validity is carried as a MARGIN vm (alive <=> vm >= 0) that every test lowers with v_min3_f32 instead of a compare,
// a mask AND and a select each: r^2 <= R^2 becomes R^2 - r^2, disc >= 0 the discriminant itself, cos^2 i > thr becomes
// cos^2 i - nextup(thr).  (v_min3 drops NaN operands; a NaN can only come from a ray that an earlier margin already
// marked dead, and the splat window test rejects NaN positions.)
__device__ __forceinline__ f2 vmin3(f2 a, f2 b, f2 c) {
    return (f2){__builtin_fminf(__builtin_fminf(a.x, b.x), c.x), __builtin_fminf(__builtin_fminf(a.y, b.y), c.y)};
}
// One spherical surface, forward, unit directions.  Consecutive spheres run in a loop of their own (trace_part2) so the
// ray lives in the same registers from one sphere to the next; with the three surface kinds behind one switch the
// compiler merged the branches with 4-7 register copies per surface.
// The refraction needs no normal vector: with n = (c x, c y, c dz tau - 1) on the sphere, d.n = beta + c tau
// (beta = c (p0.d) - dz from the root), and  d' = eta d + g n  with  g = -(sqrt(1 - eta^2 (1 - (d.n)^2)) + eta d.n)
// is  (eta dx + (g c) x,  eta dy + (g c) y,  eta dz + (g c)(dz tau) - g)   (surfaces.py:589-679 restated).
typedef const __attribute__((address_space(4))) aadff_surface_t* csurf_t;
struct SphereP {                          // the scalars one sphere step needs
    float d, c, r2, eta, eta2, thr;
};
// (Measured and rejected: issuing the next entry's scalar loads by hand ahead of the arithmetic, with the ray registers
// tied to the asm statements to pin the order: 376 us against 332 us for the compiler's own s_load / s_waitcnt placement.)
__device__ __forceinline__ void sphere_step2(const SphereP& s, Ray2& r, f2& vm) {
    const f2 t0 = (s.d - r.oz) * vrcp(r.dz);
    r.ox += r.dx * t0; r.oy += r.dy * t0;                               // vertex plane
    const f2 rho2 = r.ox * r.ox + r.oy * r.oy;
    const f2 beta = s.c * (r.ox * r.dx + r.oy * r.dy) - r.dz;
    const f2 crho = s.c * rho2;
    const f2 disc = beta * beta - s.c * crho;
    const f2 root = vsqrt(vmax0(disc));
    const f2 sroot = (f2){__builtin_copysignf(root.x, beta.x), __builtin_copysignf(root.y, beta.y)};
    const f2 tau = crho * vrcp(-(beta + sroot));
    const f2 dzt = r.dz * tau;
    r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + dzt;
    vm = vmin3(vm, disc, t0 + tau);                                     // hit the sphere, t >= 0 (surfaces.py:466-470)
    const f2 dn = beta + s.c * tau;
    const f2 cos2 = dn * dn;
    vm = vmin3(vm, s.r2 - (r.ox * r.ox + r.oy * r.oy), cos2 - s.thr);   // inside the aperture; refraction valid (surfaces.py:660-666)
    const f2 sq = vsqrt(vmax0(s.eta2 * cos2 + (1.f - s.eta2)));
    const f2 g = -(sq + s.eta * dn);
    const f2 gc = g * s.c;
    r.dx = s.eta * r.dx + gc * r.ox;
    r.dy = s.eta * r.dy + gc * r.oy;
    r.dz = s.eta * r.dz + (gc * dzt - g);
}
#ifdef AADFF_SPHERE_FROM_POINT
// The same sphere met from where the ray IS (a point of the previous surface, a few mm away) instead of from the vertex
// plane: with p = o - (0,0,d) the quadratic  c t^2 + 2 t (c p.d - dz) + (c |p|^2 - 2 pz) = 0  has the same near root
// t = C / -(B + sign(B) sqrt(B^2 - c C)); no division by dz to reach the plane first - one transcendental and two packed
// instructions fewer per ray pair.  Not for a ray that starts metres away (the object point): c |p|^2 and B^2 then cancel
// catastrophically in fp32, so the first surface of a trace keeps the vertex-plane form.
__device__ __forceinline__ void sphere_step2_from_point(const SphereP& s, Ray2& r, f2& vm) {
    const f2 pz = r.oz - s.d;
    const f2 p2 = r.ox * r.ox + r.oy * r.oy + pz * pz;
    const f2 beta = s.c * (r.ox * r.dx + r.oy * r.dy + pz * r.dz) - r.dz;
    const f2 cc = s.c * p2 - 2.f * pz;
    const f2 disc = beta * beta - s.c * cc;
    const f2 root = vsqrt(vmax0(disc));
    const f2 sroot = (f2){__builtin_copysignf(root.x, beta.x), __builtin_copysignf(root.y, beta.y)};
    const f2 tau = cc * vrcp(-(beta + sroot));
    const f2 zt = pz + r.dz * tau;                                      // height above the vertex at the hit
    r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + zt;
    vm = vmin3(vm, disc, tau);
    const f2 dn = beta + s.c * tau;
    const f2 cos2 = dn * dn;
    vm = vmin3(vm, s.r2 - (r.ox * r.ox + r.oy * r.oy), cos2 - s.thr);
    const f2 sq = vsqrt(vmax0(s.eta2 * cos2 + (1.f - s.eta2)));
    const f2 g = -(sq + s.eta * dn);
    const f2 gc = g * s.c;
    r.dx = s.eta * r.dx + gc * r.ox;
    r.dy = s.eta * r.dy + gc * r.oy;
    r.dz = s.eta * r.dz + (gc * zt - g);
}
#endif
// stop / asphere, forward (the general code of react2 with the margin form of validity)
__device__ __forceinline__ void stop_step2(const aadff_surface_t& s, Ray2& r, f2& vm) {
    const f2 t0 = (s.d - r.oz) * vrcp(r.dz);
    r.ox += r.dx * t0; r.oy += r.dy * t0;
    r.oz = f2s(s.d);
    vm = vmin3(vm, s.r * s.r - (r.ox * r.ox + r.oy * r.oy), vm);        // sqrt(x^2+y^2) <= r (surfaces.py:418)
    if (s.refract_fwd) {
        const i2 v = refract_dir2(s, r, true, f2s(0.f), f2s(0.f), f2s(-1.f));
        vm = vsel(v, vm, f2s(-1.f));
    }
}
__device__ __forceinline__ void asphere_step2(const aadff_surface_t& s, Ray2& r, f2& vm, int& nan_flag) {
    const f2 t0 = (s.d - r.oz) * vrcp(r.dz);
    r.ox += r.dx * t0; r.oy += r.dy * t0;
    f2 tau, g;
    i2 valid;
    const i2 alive = vm >= 0.f;
#ifndef AADFF_NORMAL_REEVAL
    newton2(s, r, alive, t0, tau, valid, nan_flag, &g);
    r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + r.dz * tau;
#else
    newton2(s, r, alive, t0, tau, valid, nan_flag);
    r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + r.dz * tau;
    f2 sag;
    sag_and_slope2(s, r.ox * r.ox + r.oy * r.oy, sag, g);
#endif
    f2 nx = g * 2.f * r.ox, ny = g * 2.f * r.oy;
    const f2 inv = vrsq(vmax(nx * nx + ny * ny + 1.f, f2s(1e-24f)));
    nx *= inv; ny *= inv;
    valid &= refract_dir2(s, r, true, nx, ny, -inv);
    vm = vsel(valid, vm, f2s(-1.f));
}
__device__ __forceinline__ void other_step2(const aadff_surface_t& s, Ray2& r, f2& vm, int& nan_flag) {
    if (s.kind == AADFF_SURF_STOP) {
        stop_step2(s, r, vm);
    } else if (s.kind == AADFF_SURF_SPHERIC) {                          // only with -DAADFF_SPHERE_NEWTON-style builds; kept general
        const f2 t0 = (s.d - r.oz) * vrcp(r.dz);
        r.ox += r.dx * t0; r.oy += r.dy * t0;
        f2 tau;
        const i2 hit = conic_root2<true>(s, r, tau);
        i2 valid = hit & (t0 + tau >= 0.f);
        r.ox += r.dx * tau; r.oy += r.dy * tau; r.oz = s.d + r.dz * tau;
        valid &= (r.ox * r.ox + r.oy * r.oy) <= s.r2;
        const i2 v = refract_dir2(s, r, true, s.c * r.ox, s.c * r.oy, (s.c * r.dz) * tau - 1.f);
        vm = vsel(valid & v, vm, f2s(-1.f));
    } else {
        asphere_step2(s, r, vm, nan_flag);
    }
}
__device__ __forceinline__ SphereP sphere_params(csurf_t cs, int i) {
    SphereP p;
    p.d = cs[i].d; p.c = cs[i].c; p.r2 = cs[i].r2; p.eta = cs[i].eta_fwd; p.eta2 = cs[i].eta_fwd2;
    p.thr = __builtin_bit_cast(float, __builtin_bit_cast(int, cs[i].cos2_min_fwd) + 1);
    return p;
}
// ---- the same trace with the surface kinds known at compile time ----------------------------------------------------
// In the loop of trace_part2 the ray is carried across a run-time dispatch on `kind`, and the compiler joins the code paths
// with blocks of register copies at every change of kind (7 into a sphere run, 22-31 out of a run, a stop or an asphere).
// With the kind sequence a template argument the steps follow each other as straight-line code and the ray stays in one
// set of registers from the first surface to the last; every number (c, d, r2, eta, k, ai, whether the stop refracts, ...)
// is still read from the table.  psf_points_dispatch picks the instantiation once per workgroup.
template <int... K>
struct KindSeq {
    static constexpr int n = sizeof...(K);
    static constexpr int kind(int i) { constexpr int k[] = {K...}; return k[i]; }
    static constexpr int stop() { for (int i = 0; i < n; ++i) if (kind(i) == AADFF_SURF_STOP) return i; return -1; }
    static constexpr int split = stop() < 0 ? n / 2 : (stop() + 2 < n ? stop() + 2 : n);     // as psf_points_body computes it
};
struct KindLoop { static constexpr int n = 0; };                        // kinds read at run time: trace_part2
#if defined(AADFF_PSF_GENERIC_LOOP) || defined(AADFF_PSF_SWITCH_LOOP) || defined(AADFF_PSF_SCALAR) || defined(AADFF_PSF_NO_COMPACT) || \
    defined(AADFF_SPHERE_FROM_POINT)
#define AADFF_PSF_NO_SEQ 1                                              // measurement builds keep the one loop
#endif
namespace seq {
constexpr int S = AADFF_SURF_SPHERIC, T = AADFF_SURF_STOP, A = AADFF_SURF_ASPHERIC;
typedef KindSeq<S, S, S, S, S, T, S, S, A, A, S, S> Rf50mm;             // rf50mm, rf50mm_ai4, rf50mm_named
typedef KindSeq<S, S, S, S, S, S, T, S, S, S, S> F28;                   // 50mm_f2.8
}
template <class SEQ, int I, int LAST>
__device__ __forceinline__ void seq_steps2(const aadff_surface_t* __restrict__ surf, Ray2& r, f2& vm, int& nan_flag) {
    if constexpr (I < LAST) {
        if constexpr (SEQ::kind(I) == AADFF_SURF_SPHERIC) sphere_step2(sphere_params((csurf_t)surf, I), r, vm);
        else if constexpr (SEQ::kind(I) == AADFF_SURF_STOP) stop_step2(surf[I], r, vm);
        else asphere_step2(surf[I], r, vm, nan_flag);
        seq_steps2<SEQ, I + 1, LAST>(surf, r, vm, nan_flag);
    }
}
template <class SEQ, int I = 0>
__device__ __forceinline__ bool seq_matches(csurf_t cs, int n_surf) {
    if constexpr (I == 0) { if (n_surf != SEQ::n) return false; }
    if constexpr (I < SEQ::n) return cs[I].kind == SEQ::kind(I) && seq_matches<SEQ, I + 1>(cs, n_surf);
    else return true;
}
// 0: the loop; 1, 2: the compiled sequences.  Wave-uniform: table reads only.
__device__ __forceinline__ int psf_seq_path(const aadff_surface_t* main_tab, const aadff_surface_t* chief_tab, int n_surf, int force_loop) {
#ifndef AADFF_PSF_NO_SEQ
    if (force_loop) return 0;
    const csurf_t m = (csurf_t)main_tab, c = (csurf_t)(chief_tab ? chief_tab : main_tab);
    if (seq_matches<seq::Rf50mm>(m, n_surf) && seq_matches<seq::Rf50mm>(c, n_surf)) return 1;
    if (seq_matches<seq::F28>(m, n_surf) && seq_matches<seq::F28>(c, n_surf)) return 2;
#endif
    return 0;
}
// surfaces [first, last) forward; r.alive in/out (r.ra not touched)
template <class SEQ, int FIRST, int LAST>
__device__ __forceinline__ void trace_seq2(const aadff_surface_t* __restrict__ surf, Ray2& r, int& nan_flag) {
    f2 vm = vsel(r.alive, f2s(3e38f), f2s(-1.f));
    seq_steps2<SEQ, FIRST, LAST>(surf, r, vm, nan_flag);
    r.alive = vm >= 0.f;
}
__device__ __forceinline__ void trace_part2(const aadff_surface_t* __restrict__ surf, int first, int last, Ray2& r, int& nan_flag) {
#ifdef AADFF_PSF_SWITCH_LOOP
    for (int i = first; i < last; ++i) react2(surf[i], r, true, nan_flag);
#else
    // the table is read through the constant address space: wave-uniform scalar loads (the kernel's own global stores
    // otherwise make the compiler fall back to per-lane vector loads inside the sphere loop)
    const csurf_t cs = (csurf_t)surf;
    f2 vm = vsel(r.alive, f2s(3e38f), f2s(-1.f));
    int i = first;
    while (i < last) {
        if (cs[i].kind == AADFF_SURF_SPHERIC) {
            do {
                const SphereP cur = sphere_params(cs, i);
#ifdef AADFF_SPHERE_FROM_POINT
                if (i == 0) sphere_step2(cur, r, vm);
                else sphere_step2_from_point(cur, r, vm);
#else
                sphere_step2(cur, r, vm);
#endif
                ++i;
            } while (i < last && cs[i].kind == AADFF_SURF_SPHERIC);
        } else {
            other_step2(surf[i], r, vm, nan_flag);
            ++i;
        }
    }
    r.alive = vm >= 0.f;
#endif
}
// in: r.alive; out: r.alive and r.ra = alive ? 1 : 0
template <class SEQ = KindLoop>
__device__ __forceinline__ void trace_forward2(const aadff_surface_t* __restrict__ surf, int n_surf, Ray2& r, int& nan_flag) {
    if constexpr (SEQ::n == 0) trace_part2(surf, 0, n_surf, r, nan_flag);
    else trace_seq2<SEQ, 0, SEQ::n>(surf, r, nan_flag);
    r.ra = vsel(r.alive, f2s(1.f), f2s(0.f));
}
__device__ __forceinline__ void disc_sample2(f2 u_theta, f2 u_r, float R2, f2& x, f2& y) {
    const f2 rr = vsqrt(u_r * R2);
#ifndef AADFF_LIBM_SINCOS
    x = rr * (f2){__builtin_amdgcn_cosf(u_theta.x), __builtin_amdgcn_cosf(u_theta.y)};
    y = rr * (f2){__builtin_amdgcn_sinf(u_theta.x), __builtin_amdgcn_sinf(u_theta.y)};
#else
    const f2 theta = u_theta * 2.f * kTwoPiHi;
    x = rr * (f2){cosf(theta.x), cosf(theta.y)};
    y = rr * (f2){sinf(theta.x), sinf(theta.y)};
#endif
}
// rays from one object point to two pupil samples, then through the lens to the sensor plane
template <class SEQ = KindLoop>
__device__ __forceinline__ Ray2 trace_pair_to_sensor(float px, float py, float pz, f2 tx, f2 ty, float tz, i2 active,
                                                     const aadff_surface_t* __restrict__ surf, int n_surf, float d_sensor,
                                                     int& nan_flag) {
    Ray2 r;
    r.ox = f2s(px); r.oy = f2s(py); r.oz = f2s(pz);
    r.dx = tx - px; r.dy = ty - py; r.dz = f2s(tz - pz);
    const f2 inv = vrsq(vmax(r.dx * r.dx + r.dy * r.dy + r.dz * r.dz, f2s(1e-24f)));
    r.dx *= inv; r.dy *= inv; r.dz *= inv;
    r.alive = active;
    trace_forward2<SEQ>(surf, n_surf, r, nan_flag);
    const f2 t = (d_sensor - r.oz) * vrcp(r.dz);
    r.ox += r.dx * t; r.oy += r.dy * t; r.oz += r.dz * t;
    return r;
}

// host: the r^2 stratum of the stratified pupil samples, pupilr**2 / spp * num_angle in float64 (sample_pupil, deeplens/optics.py:579)
inline float r2_step(float pupil_r, int spp, int num_angle) {
    return (float)((double)pupil_r * (double)pupil_r / spp * num_angle);
}

}  // namespace aadff
