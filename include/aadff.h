/*
 * aadff.h — C ABI of the MI355X-native focal-stack rendering hot path.
 *
 * The reference (singer-yang/Aberration-Aware-Depth-from-Focus) has no FFI: its hot
 * path is a chain of stock torch ops behind plain Python functions.
 * This header is the boundary a maintainer would bind from those Python functions
 * (ctypes stub: INTEGRATION.md).  Every entry point cites the reference code it
 * replaces (paths relative to the reference repo).
 *
 * Conventions
 *  - all pointers are DEVICE pointers to contiguous fp32 (or the struct types below)
 *    unless the name ends in `_host`;
 *  - `stream` is a hipStream_t passed as void*; work is enqueued, never synchronised;
 *  - inputs are never written, outputs are caller-allocated;
 *  - return 0 on success, a negative AADFF_E* for argument errors, a positive
 *    hipError_t for runtime errors; aadff_last_error() gives the message.
 */
#ifndef AADFF_H_
#define AADFF_H_

#include <stddef.h>   /* size_t */

#ifdef __cplusplus
extern "C" {
#endif

#define AADFF_ABI_VERSION 9

#define AADFF_EINVAL      (-1)   /* bad shape / size / NULL pointer                  */
#define AADFF_EUNSUPPORTED (-2)  /* parameter outside what the kernels were built for */

#define AADFF_MAX_GRID   64      /* PSF grid per side (reference uses 7..11)          */
#define AADFF_MAX_KS     51      /* PSF kernel size, odd (psf_map default: optics.py:1006) */
#define AADFF_MAX_SURF   32      /* surfaces per lens                                 */
#define AADFF_MAX_AI     8       /* even-asphere coefficients a2..a16                 */

typedef void* aadff_stream_t;

/* Surface kinds = the three branches of Aspheric.ray_reaction, deeplens/surfaces.py:409,456,491 */
enum { AADFF_SURF_STOP = 0, AADFF_SURF_SPHERIC = 1, AADFF_SURF_ASPHERIC = 2 };

/* One surface at ONE wavelength.  Host code fills it (deeplens/optics.py: LensTable);
 * values that the reference forms in float64 Python arithmetic and then feeds to fp32
 * tensor ops are rounded to fp32 exactly once, here.  136 bytes. */
typedef struct aadff_surface {
    float d;            /* vertex z [mm]                            surfaces.py:11-14 */
    float c;            /* curvature 1/roc                          surfaces.py:304   */
    float k;            /* conic                                    surfaces.py:305   */
    float r;            /* semi-diameter                            surfaces.py:16    */
    float r2;           /* (float)(r*r), r*r in double              surfaces.py:466,727 */
    float r2_shape;     /* fp32 (1-1e-9)/c^2/(1+k); +inf if unused  surfaces.py:727,738 */
    float eta_fwd;      /* n1/n2 (float64 -> fp32)                  surfaces.py:400-402 */
    float eta_fwd2;     /* (n1/n2)^2 squared in float64 -> fp32     surfaces.py:658   */
    float eta_bwd;      /* n2/n1                                    surfaces.py:403-405 */
    float eta_bwd2;
    int   kind;         /* AADFF_SURF_*                                               */
    int   n_ai;         /* number of even-asphere coefficients (0..AADFF_MAX_AI)      */
    int   refract_fwd;  /* 0 when kind==STOP and eta_fwd==1 (air-air stop skips it)   surfaces.py:449 */
    int   refract_bwd;
    int   k_gt_m1;      /* k > -1 selects the shape-domain test     surfaces.py:727,738 */
    float ai[AADFF_MAX_AI];   /* a2, a4, ... (coefficient of r^(2(j+1)))       surfaces.py:799 */
    float dai[AADFF_MAX_AI];  /* (j+1) * ai[j] in fp32: derivative coefficients surfaces.py:823 */
    float cos2_min_fwd; /* max(0.1, 1 - 1/eta_fwd^2): the two refraction validity tests of surfaces.py:660-663   */
    float cos2_min_bwd; /* (cos^2 i > 0.1 and eta^2 (1 - cos^2 i) < 1) as ONE threshold on cos^2 i (fused kernels) */
    float newton_step_tol; /* fused kernels: a Newton update shorter than this [mm] ends the loose loop before the strict step
                              (the reference spends one more evaluation confirming |residual| <= 5e-5, surfaces.py:547).
                              Must satisfy kappa * tol^2 <= 4e-6 with kappa the largest |d^2 sag / d r^2| over the aperture, so
                              that the residual the strict step sees stays 3x under its 1e-5 test; <= 1e-2.  0 = never skip. */
} aadff_surface_t;

/* Per-focus-setting lens state; lives on the device so a whole stack is rendered
 * without a host round trip.  Written by aadff_refocus / aadff_post_computation.
 * Mirrors the attributes Lensgroup.refocus mutates (deeplens/optics.py:1155-1187). */
typedef struct aadff_lens_state {
    float d_sensor;     /* sensor z [mm]                                              */
    float hfov;         /* half diagonal field of view [rad]   optics.py:1187-1217    */
    float tan_hfov;     /* (float)tan((double)hfov)            optics.py:1289         */
    float foclen;       /* r_last / tan(hfov)                  optics.py:1097-1102    */
    float fnum;         /* foclen / (2*entrance pupil radius)  optics.py:186-187      */
    int   n_focus_rays; /* rays that contributed to d_sensor (0 => refocus failed; optics.py:1176) */
    int   flags;        /* bit0: NaN seen in a Newton residual (reference would exit(0), surfaces.py:555);
                           bit1: hfov was NaN and replaced by 0.5 (optics.py:1210-1212) */
    int   pad;
} aadff_lens_state_t;

/* Lens-constant sensor/pupil description (host-side scalars, passed by value). */
typedef struct aadff_lens_const {
    int   n_surf;
    float r_last;          /* half sensor diagonal [mm]                   optics.py:2068 */
    float sensor_w, sensor_h;  /* sensor_size[1], sensor_size[0] [mm]     optics.py:169  */
    float pixel_size;      /* sensor_size[0]/H [mm]                       optics.py:175  */
    float enp_z, enp_r;    /* entrance pupil (z, radius)                  optics.py:1320-1403 */
    float enp_r2;          /* (float)(enp_r^2), squared in double         optics.py:481  */
    float enp_r2_shrunk;   /* (float)((0.5*enp_r)^2)                      optics.py:1400,481 */
    float exp_z;           /* exit pupil z                                               */
    float exp_r_shrunk;    /* 0.5 * exit pupil radius (calc_fov)          optics.py:1196 */
    float first_d;         /* first surface vertex z (refocus sampling)   surfaces.py:188-199 */
    float first_r2;        /* (float)(first surface r^2)                  surfaces.py:193 */
} aadff_lens_const_t;

int         aadff_abi_version(void);
const char* aadff_last_error(void);
/* number of CUs etc. of the current device, for host-side launch heuristics */
int         aadff_device_info(int* n_cu, int* lds_bytes, char* arch, int arch_len);

/* ------------------------------------------------------------------ image space */

/* Spatially-varying blur with a g x g PSF grid.  Replaces render_psf_map,
 * deeplens/render_psf.py:31-73.  img [B,C,H,W], psf_map [C,g*ks,g*ks], out [B,C,H,W].
 * Arithmetic contract of the three convolution entries (ks <= 11 on the matrix cores): every fp32 operand is carried as an
 * fp16 hi + lo pair after a power-of-two pre-scale (per image tile / per PSF), products hi*hi + hi*lo + lo*hi accumulate in
 * fp32: >= 21-22 significand bits per operand, <= 2e-6 abs from the reference's fp32 conv2d on every golden case (tested;
 * seven decades of dynamic range inside one tile stay within 1e-6 of the tile maximum).  Non-finite input: an inf / NaN pixel
 * makes the whole tile that staged it (<= 34 x 108 pixels with halo) NaN, where F.conv2d poisons only the ks x ks support;
 * everything the reference poisons is non-finite here too and nothing farther than 128 pixels from the bad pixel is affected
 * (tested).  A PSF patch that is NaN (no ray inside its window, optics.py:978) turns exactly its image patch into NaN, as in
 * the reference. */
int aadff_render_psf_map(const float* img, const float* psf_map, float* out,
                         int B, int C, int H, int W, int grid, int ks, aadff_stream_t stream);

/* Stack-fused form: one image tile staged once for S PSF maps.  Replaces the slice loop
 * of 2_aber_aware_dff_aif.py:104-114 over render_psf_map + torch.stack(dim=2).
 * img [B,C,H,W], psf_maps [S,C,g*ks,g*ks], out [B,C,S,H,W]. */
int aadff_render_psf_map_stack(const float* img, const float* psf_maps, float* out,
                               int B, int C, int S, int H, int W, int grid, int ks,
                               aadff_stream_t stream);
/* The same with the destination of every slice given by strides (elements): the plane of (b, c, s) starts at
 * out + (b*C + c)*stride_bc + s*stride_s.  stride_bc = S*H*W, stride_s = H*W is the contiguous stack above;
 * stride_bc = H*W, stride_s = C*H*W (B = 1) writes the slices as consecutive [C,H,W] units - the layout of a sharded
 * run's all-gather buffer (BASELINE.json config 3), so a rank renders straight into it.  Planes must not
 * overlap.  Same reference counterpart as aadff_render_psf_map_stack. */
int aadff_render_psf_map_stack_strided(const float* img, const float* psf_maps, float* out,
                                       long stride_bc, long stride_s,
                                       int B, int C, int S, int H, int W, int grid, int ks,
                                       aadff_stream_t stream);
/* M1-layered stack (SURVEY.md 8(d) "M1-layered": the depth MAP quantised into L layers, one ray-traced PSF map per (slice, layer)):
 * out[b][c][s][y][x] = render_psf_map(img, psf_maps[s * L + layer_idx[b][y][x]])[b][c][y][x], i.e. the per-pixel selection among the L
 * candidates of slice s, computed in ONE launch from one staged image band per pass and written once (the composition renders
 * S * L full slices and gathers: L x the output bytes plus a pass over them).  Composes render_psf_map, deeplens/render_psf.py:31-73,
 * over the slice loop of 2_aber_aware_dff_aif.py:104-114.  img [B,C,H,W], psf_maps [S*L,C,g*ks,g*ks], layer_idx [B,H,W] uint8 (values
 * < L), out [B,C,S,H,W]; ks 11 (other sizes: AADFF_EUNSUPPORTED, compose).  Arithmetic contract as aadff_render_psf_map. */
int aadff_render_psf_map_stack_layered(const float* img, const float* psf_maps, const unsigned char* layer_idx, float* out, int B, int C, int S,
                                       int L, int H, int W, int grid, int ks, aadff_stream_t stream);

/* Seam-free PSF-map rendering (no reference counterpart; the space-variant blur of Hirsch et al., "Efficient filter flow", 2010):
 * every pixel's PSF is the bilinear interpolation of the four grid PSFs whose nodes surround it.  img [B,C,H,W], psf_maps
 * [S,C,g*ks,g*ks] (tile (i,j) as aadff_render_psf_map reads it), out [B,C,S,H,W]; S = 1 is a single slice.  node_y, node_x: HOST
 * pointers to g floats each, strictly increasing: the position of grid row i / grid column j in pixel-index units (pixel centres
 * at integers; nodes may lie outside the image).  For row y: k = clamp(#{i : node_y[i] <= y} - 1, 0, g-2),
 * fy = clamp((y - node_y[k]) / (node_y[k+1] - node_y[k]), 0, 1) (g == 1: k = 0, fy = 0), so rows beyond the outer nodes take the
 * outer PSF; columns alike give l, fx.  With R(i,j) = aadff_render_psf(img, tile (i,j) of map s) (flip, reflect padding):
 *   out[b,c,s,y,x] = (1-fy) [(1-fx) R(k,l) + fx R(k,l+1)] + fy [(1-fx) R(k+1,l) + fx R(k+1,l+1)]
 * computed in one launch from the maps (no per-pixel PSF tensor).  Plain fp32 FMA chains over the taps, one per corner PSF, blended
 * last; no atomics, every output written once, bit-reproducible.  All arguments are validated before any HIP call: NULL pointers,
 * even ks, ks / grid out of range, H or W <= ks/2, sizes too large for one launch, non-finite nodes, and nodes that are not
 * strictly increasing (the message names the axis and the index) give AADFF_EINVAL.  Odd ks up to AADFF_MAX_KS; unlike the patch
 * entries, grid may exceed H or W (cells without a pixel launch nothing). */
int aadff_render_psf_map_blend_stack(const float* img, const float* psf_maps, float* out,
                                     const float* node_y, const float* node_x,
                                     int B, int C, int S, int H, int W, int grid, int ks, aadff_stream_t stream);

/* Occlusion-aware layered PSF-map rendering (no reference counterpart; the layered defocus composite, the pixel-level form of the
 * per-ray rule of aadff_render_raytraced_layered): every layer's premultiplied image and its mask are blurred with that layer's PSF and
 * the layers are composited front to back with a transmittance, in one launch per stack (csrc/conv_occl.hip).
 * img [B,C,H,W]; psf_maps [S*L,C,g*ks,g*ks], pair p = s*L + l, tile (i,j) as aadff_render_psf_map reads it; layer [B,H,W] uint8, layer 0
 * the nearest, a texel whose index is >= L lies on no layer (a hole); out [B,C,S,H,W]; coverage_or_null [B,C,S,H,W] or NULL.
 * Arithmetic contract, per output pixel (b,c,s,y,x) of patch (i,j) (patch bounds int(i/grid*n), as aadff_render_psf_map):
 *   1. w_l(u,v) = psf[ks-1-u][ks-1-v] of tile (i,j) of map s*L + l, channel c (the flipped tile).
 *   2. The image and the layer map are reflect-padded by ks/2 with the same index reflection; tap t = (u,v) reads texel
 *      (reflect(y - ks/2 + u), reflect(x - ks/2 + v)).
 *   3. m_l(t) = (layer[b,t] == l).
 *   4. a_l = sum_t w_l(t) (m_l(t) ? 1 : 0): the coverage, one fp32 fma chain a = fma(w, m, a) from 0 over the taps in row-major order
 *      (u = 0 .. ks-1, inside it v = 0 .. ks-1).
 *   5. q_l = sum_t w_l(t) (m_l(t) ? img[b,c,t] : 0): the radiance, a second chain of the same form in the same tap order.  The mask is
 *      a SELECT, not a product: a NaN or Inf on a texel of another layer or of a hole does not reach the output.
 *   6. T = 1, V = 0, A = 0; for l = 0 .. L-1 in this order: V = fma(T, q_l, V); A = fma(T, a_l, A); T = T * max(1 - a_l, 0)
 *      (each operation rounded once, fp32).
 *   7. normalize != 0: out = V / A (IEEE division) where A > 0, else 0; normalize == 0: out = V.  coverage = A.
 * Consequences that hold exactly: a layer none of whose window texels carries index l has a_l = q_l = 0 and leaves V, A, T unchanged
 * (the kernel skips the layers absent from the staged tile: no bit changes); if every window texel is on layer k, V = q_k and A = a_k;
 * scaling the image by a power of two scales V by the same factor bit for bit.  No atomics, every output written once, a repeat equals
 * itself bit for bit, a stack equals its slices and a batch its images.  Gradients: the _bwd entry below.  All arguments are validated before any HIP
 * call: NULL pointers (coverage may be NULL), even ks, ks outside 3 .. AADFF_MAX_KS, L outside 1 .. AADFF_RENDER_MAX_LAYERS (defined
 * below, 32), grid outside 1 .. AADFF_MAX_GRID or above min(H, W), H or W <= ks/2 and sizes too large for one launch give AADFF_EINVAL. */
int aadff_render_psf_map_stack_occluded(const float* img, const float* psf_maps, const unsigned char* layer, float* out,
                                        float* coverage_or_null, int B, int C, int S, int L, int H, int W, int grid, int ks,
                                        int normalize, aadff_stream_t stream);

/* Gradients of aadff_render_psf_map_stack_occluded to the image and the PSF maps (csrc/conv_occl_bwd.hip).  The layer
 * map is integral and gets none.  d_out_or_null = g and d_cov_or_null = h [B,C,S,H,W] are the upstream gradients to `out` and to the
 * coverage; either may be NULL and then counts as 0 (both NULL: AADFF_EINVAL).  d_img_or_null [B,C,H,W], d_maps_or_null
 * [S*L,C,g*ks,g*ks]: only the ones given are computed (both NULL: AADFF_EINVAL).  With q_l, a_l, T_l, V, A, out of the forward's
 * contract (recomputed with the forward's chains, bit for bit) and f_l = max(1 - a_l, 0), per element (b,c,s,pi):
 *   1. normalize and A > 0: gV = g / A, gA = fma(-gV, out, h) (= h - g out / A); normalize and A = 0: gV = 0, gA = h;
 *      normalize == 0: gV = g, gA = h.
 *   2. Back to front: R_L = 0, G_l = fma(gV, q_l, gA * a_l), R_l = fma(f_l, R_{l+1}, G_l); then front to back with T_0 = 1:
 *      alpha_l = dL/dq_l = gV * T_l,   beta_l = dL/da_l = gA * T_l - [1 - a_l > 0] T_l R_{l+1}  (fma(-T_l, R_{l+1}, gA * T_l)),
 *      T_{l+1} = T_l * f_l.  The indicator is the derivative of the clamp, 0 at equality.  T_l R_{l+1} is never formed as a quotient.
 *   3. With refl the forward's reflect padding, p = ks/2, and the PSF belonging to the SOURCE pixel's patch (as
 *      aadff_render_psf_map_stack_bwd):
 *        d_img[b,c,t] = sum_s sum_{pi, tap : refl(pi + tap - p) = t} alpha_{layer[b,t]}(b,c,s,pi) w^{s,layer[b,t]}_{patch(pi)}(tap)
 *      a SELECT by the texel's layer, not a sum over layers; a hole texel gets exactly 0; mirror folds as the patch route's d_img;
 *        d_maps[s L + l, c, i ks + a, j ks + e] = sum_b sum_{pi in patch(i,j)} alpha_l(pi) (m_l(t) ? img[b,c,t] : 0) + beta_l(pi) (m_l(t) ? 1 : 0),
 *      t = refl(pi + p - (a,e)): the image enters through a select, so a NaN on a hole or on another layer's texel reaches no
 *      gradient; the maps of a layer that occurs nowhere in the batch get exact zeros.
 * Plain fp32 fma, every sum in a fixed order, no float atomics, every output element written exactly once, bit-reproducible.  The
 * d_img sum over the slices runs in ascending s, each slice's whole contribution added as one value to a running sum that starts at 0.
 * Workspace: DEVICE memory of at least aadff_render_psf_map_stack_occluded_bwd_workspace(B, C, 1, L, H, W, grid, ks, d_maps != NULL)
 * bytes: alpha and beta per (b,c,s,l,pixel) plus, for d_maps, one partial per 32 x 32 tile.  The entry processes as many slices per
 * pass as fit; the query for the call's own S is the size at which one pass suffices; results are bit-equal for every admissible
 * size.  The workspace need not be initialised.  The argument domain and the messages are the forward's; everything is validated
 * before any HIP call.  The query returns 0 for a shape the call rejects. */
int aadff_render_psf_map_stack_occluded_bwd(const float* img, const float* psf_maps, const unsigned char* layer,
                                            const float* d_out_or_null, const float* d_cov_or_null, float* d_img_or_null,
                                            float* d_maps_or_null, void* workspace, size_t workspace_bytes, int B, int C, int S, int L,
                                            int H, int W, int grid, int ks, int normalize, aadff_stream_t stream);
size_t aadff_render_psf_map_stack_occluded_bwd_workspace(int B, int C, int S, int L, int H, int W, int grid, int ks, int need_maps);

/* Soft depth layers for the occlusion-aware layered render (csrc/conv_occl_soft.hip): the L maps of a slice are NODES
 * in depth, every texel carries a continuous layer coordinate and is blurred with the PSF interpolated linearly between the two nodes
 * around it; the slabs between nodes are composited front to back by the rule of aadff_render_psf_map_stack_occluded.
 * img [B,C,H,W]; psf_maps [S*L,C,g*ks,g*ks], node l of slice s is map s*L + l, node 0 the nearest, tiles as aadff_render_psf_map reads
 * them; pos [B,H,W] float32, the texel's layer coordinate; 1 <= L <= AADFF_RENDER_MAX_LAYERS; out, coverage_or_null [B,C,S,H,W].
 * Arithmetic contract.  Per texel t:
 *   1. !(pos >= 0) (NaN included): a hole, it covers nothing and shows nothing.  Otherwise p = min(pos, L-1), slab k = min((int)p, L-1),
 *      f = p - k: exact in float32, in [0,1).  Slab L-1 has node L-1 alone and is reached only at p = L-1, with f = 0.
 *   2. m0 = fl(1 - f), m1 = f, x0 = fl(m0 * img[b,c,t]), x1 = fl(m1 * img[b,c,t]).
 * Per output pixel (b,c,s,y,x) of patch (i,j), with w_k the flipped tile (i,j) of map s*L + k, channel c, and img and pos reflect-padded
 * by ks/2 alike (steps 1, 2 of the contract above):
 *   3. Per slab k four fp32 fma chains from 0 over the taps in row-major order, each term a SELECT on slab(t) == k:
 *        q0 = sum_t w_k(t) (slab(t)==k ? x0 : 0),      a0 = sum_t w_k(t) (slab(t)==k ? m0 : 0),
 *        q1 = sum_t w_{k+1}(t) (slab(t)==k ? x1 : 0),  a1 = sum_t w_{k+1}(t) (slab(t)==k ? m1 : 0)     (both exactly 0 for k = L-1),
 *      then q_k = fl(q0 + q1), a_k = fl(a0 + a1).  A NaN on a hole or on another slab's texel never reaches the output.
 *   4. Steps 6 and 7 of the contract above with q_k, a_k for q_l, a_l: T = 1, V = 0, A = 0; for k = 0 .. L-1: V = fma(T, q_k, V),
 *      A = fma(T, a_k, A), T = T * max(1 - a_k, 0); out = V / A where A > 0, else 0 (normalize == 0: out = V); coverage = A.
 * The image is expected finite on every texel that is not a hole (0 * Inf in x1 is not defined here).  Consequences that hold exactly:
 * integral coordinates (holes as NaN or < 0) give aadff_render_psf_map_stack_occluded on the same indices bit for bit (m0 = 1, x0 = x,
 * every term of q1, a1 an exact 0; the kernel skips that pass where no staged texel of the slab has f != 0); L = 1 gives the hard L = 1
 * render for every pos >= 0; pos > L-1 gives what pos = L-1 gives; a slab with no texel in the window changes nothing; a power-of-two
 * image scale scales V alike; a repeat equals itself, a stack its slices and a batch its images.  A uniform surface inside one slab
 * has a_k = 1 up to rounding and hides what lies behind it: only its PSF moves with f.  No atomics, every output written once.
 * Forward only.  The argument domain and the messages are aadff_render_psf_map_stack_occluded's; NULL pos gives AADFF_EINVAL;
 * everything is validated before any HIP call. */
int aadff_render_psf_map_stack_soft_occluded(const float* img, const float* psf_maps, const float* pos, float* out,
                                             float* coverage_or_null, int B, int C, int S, int L, int H, int W, int grid, int ks,
                                             int normalize, aadff_stream_t stream);

/* Measurement aid (no reference counterpart): arm the NEXT aadff_render_psf_map_stack (slice-batched kernel: ks 11, S >= 3)
 * or aadff_psf_points / aadff_psf_points_staged call made by this host thread so that its kernel is launched with the two
 * HIP events (hipEvent_t, timing enabled) attached to the dispatch (hipExtLaunchKernelGGL): hipEventElapsedTime then gives
 * the kernel's own begin-to-end time - what rocprofv3 reports - instead of the bracket of two stream events, which adds the
 * dispatch gaps (~2-4 us).  A stack call (plain, strided or layered) that launches any other convolution kernel records the two
 * events around its launch instead; a stack call that refuses its arguments disarms.  NULL, NULL disarms.  Other launches ignore it. */
int aadff_time_next_launch(void* start_event, void* stop_event);

/* One PSF for the whole image.  Replaces render_psf, deeplens/render_psf.py:12-28.
 * psf [C,ks,ks]. */
int aadff_render_psf(const float* img, const float* psf, float* out,
                     int B, int C, int H, int W, int ks, aadff_stream_t stream);

/* Diagnostics: what the patch-convolution entry `entry` ("map": aadff_render_psf_map, "psf": aadff_render_psf, "stack", "strided",
 * "layered": the aadff_render_psf_map_stack* entries) would launch for these arguments under the current environment (the
 * AADFF_CONV_* switches).  Host arithmetic only: the very plan the entry launches from, no device is touched.  S is ignored by
 * "map" / "psf" (one slice), grid by "psf" (1), L by all but "layered", the strides by all but "strided".
 * name [name_len]: the kernel instantiation as the library's symbol table spells it (nm -C), e.g. conv_psf_map_blkw_kernel<13, 32>;
 * info [5]: workgroups, threads per workgroup, dynamic LDS bytes, slices per workgroup of a wide Toeplitz launch (0 otherwise),
 * 1 if the launch takes aadff_time_next_launch's events on its own dispatch (0: they are recorded around it).
 * A shape the entry refuses returns the entry's own code and sets its message. */
int aadff_conv_plan_describe(const char* entry, int B, int C, int S, int L, int H, int W, int grid, int ks, long stride_bc,
                             long stride_s, char* name, int name_len, long long* info);

/* Per-pixel PSF gather (no flip, replicate padding, same PSF for every channel).
 * Replaces local_psf_render, deeplens/render_psf.py:76-107.  psf [B,H,W,ks,ks]. */
int aadff_local_psf_render(const float* img, const float* psf, float* out,
                           int B, int C, int H, int W, int ks, aadff_stream_t stream);

/* ---- backward of the image-space operators (csrc/conv_bwd.hip).  In the reference these functions are plain torch
 * (F.pad + F.conv2d, unfold / fold) and torch.autograd differentiates them; the entries below are those gradients as
 * closed forms.  Plain fp32 operands, fp32 accumulation, every sum in a fixed order (no float atomics): bitwise
 * reproducible from run to run.  A gradient whose output pointer is NULL is not computed; both NULL is an error.
 * The argument domain is the forward entry's: what it rejects is rejected here the same way, before any HIP call. */

/* Gradients of aadff_render_psf_map_stack (S = 1: aadff_render_psf_map; S = 1, grid = 1: aadff_render_psf), i.e. the
 * autograd of deeplens/render_psf.py:12-73 (reflect pad :57, flipped depthwise conv2d per patch :59-72), summed over the
 * slice loop of 2_aber_aware_dff_aif.py:104-114.  img [B,C,H,W], psf_maps [S,C,g*ks,g*ks], dy [B,C,S,H,W] contiguous,
 * d_img [B,C,H,W] (sum over the slices; PSF chosen by the patch of the dy pixel, halo folded back over the reflect
 * padding), d_psf [S,C,g*ks,g*ks] (sum over the batch).  d_psf needs `workspace`: device memory of at least
 * aadff_render_psf_map_stack_bwd_workspace bytes (partial sums per 32 x 32 tile, added in a fixed order by a second
 * kernel); it may be NULL / 0 when d_psf is NULL. */
int aadff_render_psf_map_stack_bwd(const float* img, const float* psf_maps, const float* dy,
                                   float* d_img_or_null, float* d_psf_or_null, void* workspace, size_t workspace_bytes,
                                   int B, int C, int S, int H, int W, int grid, int ks, aadff_stream_t stream);
/* Workspace bytes of the call above for the same shape (host arithmetic only, no device needed; monotone in B and S). */
int aadff_render_psf_map_stack_bwd_workspace(int B, int C, int S, int H, int W, int grid, int ks, size_t* bytes);

/* Gradients of aadff_render_psf_map_blend_stack (csrc/conv_blend_bwd.hip).  With the HAT of node i on row y,
 *   Hy_i(y) = [k(y) == i] (1 - fy(y)) + [min(k(y) + 1, g - 1) == i] fy(y)      (k, fy of the forward; g == 1: 1 everywhere)
 * and Hx_j(x) alike, the forward is out[b,c,s,y,x] = sum_{nodes (i,j)} Hy_i(y) Hx_j(x) sum_{u,v} xpad[b,c,y+u,x+v] w_ij[ks-1-u][ks-1-v]
 * (xpad the reflect-padded image, w_ij tile (i,j) of map s), and
 *   d_img[b,c,y',x']         = sum_s sum_{(i,j)} sum over the source pixels (y,x) and taps (u,v) whose reflected position is (y',x') of
 *                              dy[b,c,s,y,x] Hy_i(y) Hx_j(x) w_ij[ks-1-u][ks-1-v]          (the direct term plus the mirror folds)
 *   d_maps[s,c,i ks+a,j ks+e] = sum_b sum_{(y,x)} dy[b,c,s,y,x] Hy_i(y) Hx_j(x) xpad[b,c,y+ks-1-a,x+ks-1-e]
 * img [B,C,H,W], psf_maps [S,C,g*ks,g*ks], dy [B,C,S,H,W] contiguous, d_img [B,C,H,W] (sum over the slices), d_maps [S,C,g*ks,g*ks]
 * (sum over the batch; the tile of a node whose hat holds no pixel is exact zeros).  node_y, node_x: HOST pointers as in the forward;
 * they get no gradient.  Plain fp32 fmaf sums in a fixed order, the same fx, fy arithmetic as the forward, no float atomics, every
 * output element written exactly once: bit-reproducible.  A gradient whose pointer is NULL is not computed; both NULL is an error.
 * d_maps needs `workspace`: device memory of at least aadff_render_psf_map_blend_stack_bwd_workspace bytes (partial sums per 32 x 32
 * tile of a cell, added in a fixed order by a second kernel); it may be NULL / 0 when d_maps is NULL.  The argument domain and the
 * messages are the forward's (plus S*C <= 65535); everything is validated before any HIP call. */
int aadff_render_psf_map_blend_stack_bwd(const float* img, const float* psf_maps, const float* dy,
                                         float* d_img_or_null, float* d_maps_or_null, void* workspace, size_t workspace_bytes,
                                         const float* node_y, const float* node_x,
                                         int B, int C, int S, int H, int W, int grid, int ks, aadff_stream_t stream);
/* Workspace bytes of the call above: a bound that holds for any nodes (host arithmetic only; monotone in B and S); 0 for a shape the
 * call rejects (aadff_last_error says why). */
size_t aadff_render_psf_map_blend_stack_bwd_workspace(int B, int C, int S, int H, int W, int grid, int ks);

/* Gradients of aadff_local_psf_render, i.e. the autograd of deeplens/render_psf.py:76-107 (replicate pad :93, unfold :99,
 * product with the per-pixel kernels and sum :100-104, fold :105).  dy [B,C,H,W], d_img [B,C,H,W] (taps that clamp onto
 * a border pixel all land on it), d_psf [B,H,W,ks,ks] (sum over the channels). */
int aadff_local_psf_render_bwd(const float* img, const float* psf, const float* dy,
                               float* d_img_or_null, float* d_psf_or_null,
                               int B, int C, int H, int W, int ks, aadff_stream_t stream);

/* Thin-lens baseline renderer with the PSF evaluated in the kernel.  Replaces ThinLens.coc + ThinLens.render (4-D
 * branch), deeplens/psfnet.py:503-512,549-570: per pixel the circle of confusion of `depth` for focus distance
 * `foc_dist[b]`, a Gaussian of sigma = coc/2 pixels cut off at radius coc/2, L1-normalised, gathered over the
 * replicate-padded image (deeplens/render_psf.py:76-107).  No [N,H,W,ks,ks] tensor is materialised.
 *   img [B,C,H,W] (C <= 4), depth [B,1,H,W] (mm), foc_dist [B] (mm), out [B,C,H,W]; ks in {3,5,...,13}
 *   negate_or_null: device int, non-zero = negate depth and foc_dist first (the reference's whole-tensor test
 *                   `(depth < 0).any()`, psfnet.py:505, evaluated by the caller on the device: no host sync)
 *   foc_len_over_fnum, foc_len, inv_pixel_size = 1/ps, d_min, d_max: the lens constants of psfnet.py:491-500
 *   (depth is clamped to [d_min, d_max]; coc in pixels is clamped to >= 0.1). */
int aadff_thinlens_render(const float* img, const float* depth, const float* foc_dist, const int* negate_or_null,
                          float* out, int B, int C, int H, int W, int ks, float foc_len_over_fnum, float foc_len,
                          float inv_pixel_size, float d_min, float d_max, aadff_stream_t stream);

/* ---- differentiable thin-lens baseline (csrc/thinlens_bwd.hip).  In the reference ThinLens.render is plain torch without
 * @torch.no_grad(), differentiable in the image, the depth map and the focus distance; the entries below are its stack-fused
 * forward and those gradients as closed forms.  Lens constants and `negate_or_null` as in aadff_thinlens_render;
 * the argument domain is its domain (C <= 4, ks in {3,5,...,13}) with S >= 1, checked before any HIP call. */

/* aadff_thinlens_render for S focus distances per batch item with the image window staged once: foc_dists [B,S],
 * out [B,C,S,H,W]; slice s is bit-equal to aadff_thinlens_render with foc_dist = foc_dists[:, s]. */
int aadff_thinlens_render_stack(const float* img, const float* depth, const float* foc_dists, const int* negate_or_null,
                                float* out, int B, int C, int S, int H, int W, int ks, float foc_len_over_fnum, float foc_len,
                                float inv_pixel_size, float d_min, float d_max, aadff_stream_t stream);

/* Gradients of aadff_thinlens_render_stack: dy [B,C,S,H,W] -> d_img [B,C,H,W] (sum over the slices in slice order; taps that
 * clamp onto a border pixel all land on it), d_depth [B,1,H,W] (sum over the slices in slice order; exactly 0 where the
 * depth is outside [d_min, d_max] or the 0.1 px floor of the coc is active), d_foc [B,S].  The disc mask rho < r^2 is a
 * constant, r^2 is computed exactly as the forward computes it.  A gradient whose pointer is NULL is not computed; all
 * NULL is an error.  No float atomics: bitwise reproducible.  `workspace`: device memory of at least
 * aadff_thinlens_render_stack_bwd_workspace bytes (r^2 and 1/Z per (b, slice, pixel) for d_img, one partial per
 * workgroup for d_foc); may be NULL / 0 when only d_depth is wanted.  No [B,H,W,ks,ks] tensor is built. */
int aadff_thinlens_render_stack_bwd(const float* img, const float* depth, const float* foc_dists, const int* negate_or_null,
                                    const float* dy, float* d_img_or_null, float* d_depth_or_null, float* d_foc_or_null,
                                    void* workspace, size_t workspace_bytes, int B, int C, int S, int H, int W, int ks,
                                    float foc_len_over_fnum, float foc_len, float inv_pixel_size, float d_min, float d_max,
                                    aadff_stream_t stream);
/* Workspace bytes of the call above (host arithmetic only):
 * 4 * ((need_img ? 2 * B*S*H*W : 0) + (need_foc ? B*S*H*ceil(W/64) : 0)). */
int aadff_thinlens_render_stack_bwd_workspace(int B, int C, int S, int H, int W, int ks, int need_img, int need_foc,
                                              size_t* bytes);

/* ---- depth from a focal stack (csrc/dfocus.hip): the classical estimator, the counterpart of the renderers.
 * Not in the reference, which estimates depth with networks only (dff/AiFNet.py). */
enum { AADFF_DFOCUS_NONE = 0, AADFF_DFOCUS_PARABOLA = 1, AADFF_DFOCUS_GAUSSIAN = 2 };

/* Focus measure, argmax over the slices and three-point peak fit in one launch and one pass over the stack.
 *   stack [N,C,S,H,W] (C in 1..4, the layout every stack renderer here writes), coords [N,S]: the abscissa of every slice,
 *   strictly monotone per row in either direction (not checked: device data), spacing free.
 *   gray g = ((c0 + c1) + c2 ...) * float32(1/C); modified Laplacian ML = |(2g - g_left) - g_right| + |(2g - g_up) - g_down| with
 *   replicate padding (exactly rounded: bit-reproducible); F_s = sum of ML over window x window (replicate padding of the ML map,
 *   non-negative terms, rows then columns); s* = the first slice with the largest F_s; f0 = F_s*, u0 = coords[s*].
 *   Fit, only for 0 < s* < S-1 and interp != NONE: h- = u0 - u[s*-1], h+ = u[s*+1] - u0; PARABOLA a = f0 - F[s*-1], b = f0 - F[s*+1];
 *   GAUSSIAN a = log1p((f0 - F[s*-1]) / (F[s*-1] + eps)), b likewise; x = (a h+^2 - b h-^2) / (2 (b h- + a h+)), 0 for a zero
 *   denominator, clamped to the interval between -h- and h+; otherwise x = 0.
 *   depth [N,1,H,W] = u0 + x, index [N,1,H,W] int32 = s*, peak [N,1,H,W] = f0, aif [N,C,H,W] = stack[n,:,s*,y,x] (a copy),
 *   volume [N,S,H,W] = F.  aif and volume are written only when their pointers are non-NULL; the other outputs do not depend on
 *   that.  window in {1,3,5,7,9}, interp one of AADFF_DFOCUS_*, eps > 0.  No atomics, no workspace: bitwise reproducible.
 *   Inputs are expected to be finite; a constant image gives F = 0, index 0, depth = coords[:,0], peak 0.
 * Arguments are checked before any HIP call; the message names the offending one. */
int aadff_depth_from_stack(const float* stack, const float* coords, float* depth, int* index, float* peak, float* aif_or_null,
                           float* volume_or_null, int N, int C, int S, int H, int W, int window, int interp, float eps,
                           aadff_stream_t stream);

/* ---- differentiable depth head and its loss (csrc/focus_head.hip): stage 2 ("attention") of the reference's
 * AiFDepthNet.fit and AiFDepthNet.compute_loss (dff/AiFNet.py:376-434, 450-584) as fused kernels.
 *
 * The head.  scores [N,K,S,H,W] (K in {1,2}), stack [N,Ct,S,H,W] (Ct in 1..4) of which the first Ca channels are read in place,
 * foc_dists [N,S] (any values, any order).  zd = scores[:,0], za = scores[:,K-1].
 *   normalize == 0: pd = softmax_S(zd), pa = softmax_S(za) (the maximum is subtracted before exp).
 *   normalize != 0: pd = softplus(zd) / sum_S softplus(zd) with torch's softplus (beta 1, threshold 20); pa likewise of za for
 *                   K == 2, but pa = softmax_S(za) for K == 1 (the reference's asymmetry).
 *   depth [N,1,H,W] = sum_s pd_s foc_dists[n,s]; aif [N,Ca,H,W] = sum_s pa_s stack[n,c,s].
 * One launch, offsets in 64 bits, 16-byte accesses when W % 4 == 0 and the pointers are 16-byte aligned. */
int aadff_attention_depth(const float* scores, const float* stack, const float* foc_dists, float* depth, float* aif, int N, int K,
                          int Ct, int Ca, int S, int H, int W, int normalize, aadff_stream_t stream);

/* Gradients of the call above for the cotangents g_depth [N,1,H,W] and g_aif [N,Ca,H,W]: d_scores [N,K,S,H,W], d_stack
 * [N,Ct,S,H,W] (exact zeros in the channels from Ca on), d_foc [N,S].  The attention is recomputed from the scores; nothing of
 * the forward is needed.  A gradient whose pointer is NULL is not computed (all NULL is an error); the others do not depend on
 * that.  d_foc is reduced in two stages of fixed order, no atomics: bitwise reproducible.  `workspace`: device memory of at
 * least 4 * N * S * 4 * ceil(H * ceil(W / 4) / 256) bytes (one partial per wave and slice) when d_foc is asked for, else it may be
 * NULL / 0. */
int aadff_attention_depth_bwd(const float* scores, const float* stack, const float* foc_dists, const float* g_depth, const float* g_aif,
                              float* d_scores_or_null, float* d_stack_or_null, float* d_foc_or_null, void* workspace,
                              size_t workspace_bytes, int N, int K, int Ct, int Ca, int S, int H, int W, int normalize,
                              aadff_stream_t stream);

/* The six sums of the loss over the common top-left window h x w of the tensors that are given: depth [N,1,Hd,Wd] (always),
 * gt_depth [N,1,Hg,Wg], and aif [N,Ca,Ha,Wa] with gt_aif [N,Ca,Hi,Wi] (Ca in 1..4); at least one of gt_depth and gt_aif.
 *   mask = gt_depth > 0, or range[0] <= gt_depth <= range[1] when `range_or_null` (two floats on the device) is given.
 *   sums[0] = sum_mask |depth - gt_depth|, sums[1] = |mask|, sums[2] = sum_mask (depth - gt_depth)^2      (0 without gt_depth)
 *   sums[3] = sum |aif - gt_aif|                                                                           (0 without gt_aif)
 *   sums[4] = sum wx r(depth[y+1,x] - depth[y,x]), sums[5] = sum wy r(depth[y,x+1] - depth[y,x]), r(t) = sqrt(t^2 + 1e-6),
 *             w = exp(-mean_c (150 (gt_aif' - gt_aif))^2) over the same pixel pair                        (0 without gt_aif)
 * Terms are formed in float32 and added in float64: per-workgroup partials, then one fixed-order final sum (no atomics).
 * `workspace`: at least 48 * ceil(N * h * w / 1024) bytes of device memory. */
int aadff_dff_loss_sums(const float* depth, const float* aif_or_null, const float* gt_depth_or_null, const float* gt_aif_or_null,
                        const float* range_or_null, double* sums, void* workspace, size_t workspace_bytes, int N, int Ca, int Hd,
                        int Wd, int Ha, int Wa, int Hg, int Wg, int Hi, int Wi, aadff_stream_t stream);

/* Gradients of the sums above for their cotangents g_sums (six doubles on the device; those of sums[1] and sums[2] are not used:
 * the count and the mean square carry no gradient): d_depth [N,1,Hd,Wd], d_aif [N,Ca,Ha,Wa], zero outside the window, sign(0) = 0.
 * A cotangent multiplies only terms that exist, so an infinite or nan cotangent of an empty sum leaves zeros.  A gradient whose
 * pointer is NULL is not computed (both NULL is an error). */
int aadff_dff_loss_bwd(const float* depth, const float* aif_or_null, const float* gt_depth_or_null, const float* gt_aif_or_null,
                       const float* range_or_null, const double* g_sums, float* d_depth_or_null, float* d_aif_or_null, int N, int Ca,
                       int Hd, int Wd, int Ha, int Wa, int Hg, int Wg, int Hi, int Wi, aadff_stream_t stream);

/* ---- cost-volume depth head (csrc/dfv_head.hip): what the reference's DFVNet puts between a decoder level's cost
 * volume and its loss (DFV_models/DFFNet.py:94-95, 102-115; disparityregression of DFV_models/submodule.py:63-77) as fused kernels.
 *
 * cost [B,S,h,w], foc_dists [B,S] (any values, any order) -> for every pixel of the H x W output (H >= h, W >= w, any ratio):
 *   z_s  = the bilinear interpolation of cost[b,s] with ATen's rule for align_corners = False, in float32: scale = float(in) / out,
 *          src = max(scale * (dst + 0.5) - 0.5, 0), i0 = int(src), i1 = min(i0 + 1, in - 1), lambda = src - i0,
 *          z = (1 - ly) ((1 - lx) c[y0,x0] + lx c[y0,x1]) + ly ((1 - lx) c[y1,x0] + lx c[y1,x1]);
 *   p    = softmax_S(z) (the maximum is subtracted before exp: finite for costs of any size);
 *   pred [B,1,H,W] = sum_s p_s foc_dists[b,s];   std [B,1,H,W] = sqrt(sum_s p_s (pred - foc_dists[b,s])^2);
 *   prob [B,S,H,W] = p, written only when the pointer is non-NULL; the other outputs do not depend on that.
 * The reference's trilinear call (levels 3 and 4) has the same depth in and out and is this operation slice by slice.
 * One launch, offsets in 64 bits; no tensor of the output's resolution with S slices exists unless prob is asked for.
 * Arguments are checked before any HIP call; H < h or W < w (shrinking) is an argument error. */
int aadff_dfv_head_fwd(const float* cost, const float* foc_dists, float* pred, float* std, float* prob_or_null, int B, int S, int h,
                       int w, int H, int W, aadff_stream_t stream);

/* Gradients of pred above for the cotangent g_pred [B,1,H,W] (std and prob carry none): with dz_s = p_s (foc_dists[b,s] - pred) g,
 *   d_cost [B,S,h,w] = sum over the output pixels that read a cell of their weight times dz_s;   d_foc [B,S] = sum_pixels p_s g.
 * The softmax is recomputed from the cost; nothing of the forward is needed.  Gather form, no atomics: the pixels of a cell come from
 * the forward's own float32 index function, d_cost is summed along x into a scratch [B,S,H,w] and then along y, d_foc in two stages
 * of fixed order - bitwise reproducible.  A gradient whose pointer is NULL is not computed (both NULL is an error); the other does
 * not depend on that.  `workspace`: device memory of at least
 *   4 * B * S * ((d_cost ? H * w : 0) + (d_foc ? ceil(H / R) * ceil(w / TC) : 0)) bytes, with
 *   ratio = ceil(W / w), TC = clamp(240 / ratio - 1, 1, 8), R = clamp(256 / ((TC + 1) * ratio + 1), 1, 8) in integer arithmetic:
 *   the cells of a row and the output rows one workgroup of the first stage owns. */
int aadff_dfv_head_bwd(const float* cost, const float* foc_dists, const float* g_pred, float* d_cost_or_null, float* d_foc_or_null,
                       void* workspace, size_t workspace_bytes, int B, int S, int h, int w, int H, int W, aadff_stream_t stream);

/* ---- confidence-guided depth refinement (csrc/depth_refine.hip): one iteration of a confidence-weighted joint
 * bilateral filter.  u [N,1,H,W] the quantity to filter (in practice 1 / depth), c [N,1,H,W] its confidence (c < 2^-30, negative or nan
 * counts as 0), g [N,C,H,W] the guide, C in 1..4; radius r in 1..8.  For a pixel p and every pixel q of the (2r+1)^2 window clipped to
 * the image (no padding: a tap outside does not exist), in float32:
 *   w(p,q) = expf(max(-((dy^2 + dx^2) ks + sum_ch (g(p) - g(q))^2 kr), -64)),   ks = 1 / (2 sigma_space^2), kr = 1 / (2 sigma_range^2 C);
 *   A = sum w c(q) u(q),  D = sum w c(q), both without the taps whose c(q) is 0 (a u there may be anything, nan included),  Wn = sum w;
 *   u_out(p) = A / D where D > 0, else u(p) bit for bit;   c_out(p) = D / Wn.
 * D = 0 means that every confidence of the window is 0: the clamp keeps every weight a normal number.  One launch, offsets in 64 bits.
 * No output may be one of the inputs or the other output.  Arguments are checked before any HIP call. */
int aadff_depth_refine_fwd(const float* u, const float* c, const float* g, float* u_out, float* c_out, int N, int C, int H, int W,
                           int radius, float ks, float kr, aadff_stream_t stream);

/* Gradients of the above for the cotangents g_u_out, g_c_out [N,1,H,W] of u_out and c_out, the guide held constant, u finite:
 *   alpha(p) = g_u_out(p) / D(p) (0 where D = 0),   beta(p) = g_c_out(p) / Wn(p),
 *   d_u(q) = c(q) sum_p w(p,q) alpha(p) + [D(q) = 0] g_u_out(q),
 *   d_c(q) = sum_p w(p,q) (alpha(p) (u(q) - u_out(p)) + beta(p)),   p over the clipped window of q.
 * The threshold on c is transparent to d_c (the formula holds at every q, also where c(q) counts as 0).  Two gather passes, no
 * atomics, bitwise reproducible: the first recomputes D, Wn and u_out (nothing of the forward is kept) and writes alpha, u_out, beta
 * and the pass-through term into `work`, the second gathers them with the same weights.  A gradient whose pointer is NULL is not
 * written (both NULL is an error); the other does not depend on that.  `work`: device memory of at least 16 * N * H * W bytes. */
int aadff_depth_refine_bwd(const float* u, const float* c, const float* g, const float* g_u_out, const float* g_c_out, float* d_u_or_null,
                           float* d_c_or_null, void* work, size_t work_bytes, int N, int C, int H, int W, int radius, float ks, float kr,
                           aadff_stream_t stream);

/* ---- evaluation metrics (csrc/metrics.hip): the depth scores of the reference's dff/metrics.py and the PSNR / SSIM of
 * its batch_PSNR / batch_SSIM as per-image float64 sums that stay on the device.  No atomics: two fixed-order stages through the
 * caller's workspace, bitwise reproducible. */
enum { AADFF_VALID_MASK = 0, AADFF_VALID_FINITE = 1 };
#define AADFF_DEPTH_METRIC_COLS 16
#define AADFF_SSIM_TILE_H 32   /* 7 x 7 windows per workgroup of aadff_image_metric_sums: rows ... */
#define AADFF_SSIM_TILE_W 64   /* ... and columns */

/* One pass over est, gt [N,1,H,W] float32, mask_or_null [N,1,H,W] bytes (torch.bool's storage; non-zero = valid) and conf_or_null
 * [N,1,H,W] float32 -> sums [N,16] float64, one row per image.  Per pixel, in float64 from the exactly converted float32 values e, g, c
 * (IEEE division, the device's float64 log): d = g - e, rel = |d| / g, sq = d^2 / g, l2 = (log g - log e)^2, q = max(e / g, g / e) with
 * a nan handed on as numpy.maximum does.  Columns:
 *    0 count   1 sum |d|   2 sum d^2   3 sum rel   4 sum sq   5 sum l2   6, 7, 8 count of q < 1.25, 1.5625, 1.953125
 *    9 sum c   10 sum c |d|   11 sum c d^2 (zero without conf)   12..15 the counts of FINITE mode, zero in MASK mode
 * AADFF_VALID_MASK: over the pixels with mask != 0 (all pixels when the mask is NULL): the reference's mask_*, AIF_DepthNEt_*, mae, mse,
 *   rmse and *_w_conf* functions are quotients of these columns.
 * AADFF_VALID_FINITE (mask must be NULL): every pixel takes part, as in the reference's unmasked abs_rel, sq_rel, rmse_log and
 *   accuracy_k (dff/metrics.py:10-43): an infinite rel, sq or l2 is left out of its sum, a nan is kept; column 12 counts the pixels
 *   whose rel is not infinite, 13 those whose sq is not infinite, 14 those where neither log g nor log e is infinite (rmse_log divides
 *   by that, not by the number of terms it kept), 15 those whose q is not infinite.  Columns 0-2 and 6-11 run over all pixels.
 * An empty valid set leaves a row of zeros.  `workspace`: device memory of at least 128 * N * ceil(ceil(H * W / 4) / 256) bytes.
 * 16-byte accesses when H * W % 4 == 0 (so with W % 4 == 0) and est, gt, conf are 16-byte and mask 4-byte aligned.
 * Arguments are checked before any HIP call; the message names the offending one. */
int aadff_depth_metric_sums(const float* est, const float* gt, const unsigned char* mask_or_null, const float* conf_or_null,
                            double* sums, void* workspace, size_t workspace_bytes, int N, int H, int W, int valid_mode,
                            aadff_stream_t stream);

/* pred, target [N,C,H,W] float32, C in 1..4 -> sums [N,2] float64.  x, y = the images quantised as torch's
 * img.mul(255).add_(0.5).clamp_(0, 255).to(uint8) does, every step rounded separately in float32 (a nan gives 0).
 *   sums[n][0] = sum over channels and pixels of (x - y)^2, accumulated in 64-bit integers: exact.
 *   sums[n][1] = sum over channels and over the (H-6)(W-6) full 7 x 7 windows of
 *                S = (2 ux uy + C1)(2 vxy + C2) / ((ux^2 + uy^2 + C1)(vx + vy + C2)),  C1 = (0.01 * 255)^2, C2 = (0.03 * 255)^2,
 *                u = window mean, v = sample (co)variance (n - 1 = 48): scikit-image's structural_similarity with its defaults on uint8
 *                images, whose mean over the image cropped by 3 is this sum / ((H-6)(W-6)).  The five window sums are exact
 *                integers; the (co)variance numerators 49 Sxx - Sx^2, 49 Syy - Sy^2, 49 Sxy - Sx Sy are formed in 64-bit integers and
 *                only the last step is float64.  Computed only when want_ssim != 0 (else 0); H >= 7 and W >= 7 are then required.
 * `workspace`: 8-byte aligned device memory of at least 16 * N * B bytes, B = C * ceil((H-6) / 32) * ceil((W-6) / 64) with want_ssim,
 * else ceil(ceil(C * H * W / 4) / 256).  16-byte accesses when W % 4 == 0 (without want_ssim: C * H * W % 4 == 0) and both pointers
 * are 16-byte aligned. */
int aadff_image_metric_sums(const float* pred, const float* target, double* sums, void* workspace, size_t workspace_bytes, int N,
                            int C, int H, int W, int want_ssim, aadff_stream_t stream);

/* The quantisation rule of the kernel above, the same function compiled for the host: out[i] = byte of values[i], n >= 0 values in
 * host memory.  For tests of the rule against torch; needs no GPU. */
int aadff_quantise_u8_host(const float* values, unsigned char* out, long n);

/* ------------------------------------------------------------------ ray tracing */

/* Generic trace of n rays through surfaces [first,last) in travel order (reverse when
 * !forward), optionally followed by propagation to z = state->d_sensor.  Replaces
 * Lensgroup.trace / trace2sensor, deeplens/optics.py:598-714 + Ray.propagate_to,
 * deeplens/basics.py:255-273.  o,d [n,3], ra [n]; in and out may alias. */
int aadff_trace_rays(const float* o_in, const float* d_in, const float* ra_in,
                     float* o_out, float* d_out, float* ra_out, int n,
                     const aadff_surface_t* surf, int first, int last, int forward,
                     const aadff_lens_state_t* state_or_null, int* flags_or_null,
                     aadff_stream_t stream);

/* parity="strict": the same trace in the reference's own operation order, one IEEE float32 operation at a time (no fma
 * contraction, IEEE division / sqrt, F.normalize's fused norm, the BATCH-WIDE Newton iteration count of
 * deeplens/surfaces.py:547: all n rays of the call are one batch, as in one reference call), one launch pair per
 * surface; csrc/strict.hip, specification oracle/scalar_trace.py.  In place on o,d [n,3], ra [n] (device).  `surf_host` is
 * the HOST copy of the packed table of ONE wavelength (n_surf records).  propagate != 0 adds Ray.propagate_to(z_sensor).
 * scratch: 2*AADFF_MAX_SURF + 1 device words (zeroed by the call).  flags_or_null (device): set to 1 on a NaN residual
 * in an iteration the reference would have run.  Replaces Aspheric.ray_reaction / Lensgroup.trace,
 * deeplens/surfaces.py:391-830, deeplens/optics.py:598-714, for Lensgroup(parity="strict").  A verification path: what it
 * can and cannot reproduce is in DESIGN.md section 2. */
int aadff_trace_rays_strict(float* o, float* d, float* ra, int n, const aadff_surface_t* surf_host, int first, int last,
                            int forward, int propagate, float z_sensor, unsigned* scratch, int* flags_or_null,
                            aadff_stream_t stream);

/* The same strict trace for B independent Newton batches of n rays each in ONE launch per surface (ABI v6): what a whole focal
 * stack of Lensgroup(parity="strict") runs on - the S refocus traces (deeplens/optics.py:1155-1180), the S field-of-view traces
 * (:1187-1217) and the S x 3 x 2 traces of psf_map (main + chief rays per wavelength, :888-1026) are three calls instead of
 * 72 S.  o, d [B,n,3], ra [B,n] (device), in place.  tables_host: n_tables (<= 4) packed tables of n_surf records (HOST);
 * batch_table [B] (device): which table (wavelength) batch b traces with.  Every batch keeps its own iteration counts
 * (`while (|ft| > 5e-5).any()` is per reference call, deeplens/surfaces.py:547).
 * points_or_null != NULL: the rays are BUILT first, as sample_from_points + Ray.__init__ do (deeplens/optics.py:482-491,
 * deeplens/basics.py:216-244): ray i of batch b = (sample i / N, point i % N): o = points[point_set[b]][i % N] ([P,N,3] object
 * points, device), d = F.normalize(pupil[b][i / N] - o) (pupil [B, n / N, 3], device), ra = 1; o / d / ra are outputs then.
 * z_sensor_or_null [B] (device): Ray.propagate_to(z_sensor[b]) behind the last surface (trace2sensor).
 * scratch: 2*B*AADFF_MAX_SURF + 1 device words (zeroed by the call); flags_or_null as aadff_trace_rays_strict (any batch).
 * tbuf_or_null: 2*B*n floats (device, scratch): the Newton iterates handed from the counting pass of a surface to the launch that
 * applies it, which then does not iterate again when the batch's count is 3, 4 or 10 (same function, same state: same bits); NULL
 * recomputes. */
int aadff_trace_rays_strict_batched(float* o, float* d, float* ra, int n, int B, const aadff_surface_t* tables_host, int n_tables,
                                    int n_surf, const int* batch_table, const float* points_or_null, const int* point_set,
                                    const float* pupil, int N, int first, int last, int forward, const float* z_sensor_or_null,
                                    unsigned* scratch, float* tbuf_or_null, int* flags_or_null, aadff_stream_t stream);

/* The strict trace of B batches in ONE launch for ALL surfaces, with SPECULATED batch-wide Newton counts (ABI v7; csrc/strict_fused.hip).
 * Same rays, same per-ray arithmetic and same result as aadff_trace_rays_strict_batched WHEN pred[b][i] - the number of loose
 * iterations the reference's `while (|ft| > 5e-5).any() and it < 10` loop (deeplens/surfaces.py:547) runs for batch b at surface i -
 * is right for every curved surface the batch crosses.  The call cannot know that; it reports what it saw:
 *   bits [B][2][AADFF_MAX_SURF] (device, zeroed by the call): [b][0][i] bit j = some ray of batch b had |ft| > 5e-5 in loose
 *   iteration j + 1 at surface i (j < pred[b][i]); [b][1][i] the same for a NaN residual (the reference exits, surfaces.py:555-558).
 * The caller checks, in the order the surfaces are crossed: n = pred[b][i] is the reference's count <=> bits 0..n-2 are set and
 * (bit n-1 is clear or n == 10).  At the first surface where that fails the batch's result (and its later bits) are meaningless:
 * replay the batch through aadff_trace_rays_strict_batched, whose any-bits give the true counts (aadff/strict_stack.py keeps the
 * table).  Rays whose Newton iterate becomes periodic (a fixed point or a two-cycle of the float32 map t -> t - clamp(ft / dfdt))
 * are not iterated further: the remaining iterates and any-bits follow from the cycle, bit for bit.
 * tables_dev: n_tables packed tables of n_surf records on the DEVICE; pred [B][AADFF_MAX_SURF] int32 (device), values 1..10 (flat
 * surfaces ignored); other arguments as aadff_trace_rays_strict_batched.  With points: origin_at_pupil != 0 starts the rays AT the
 * pupil points (refocus: rays leave the first surface's aperture away from the axis point, deeplens/optics.py:1166-1170).
 * out_mode 0: o / d / ra in place.  out_mode 1 (needs points; o, d, ra may be NULL): out0[b][i] = the z at which the ray crosses
 * the axis in the least-squares sense, o.z - d.z * ((d.x o.x + d.y o.y) / (d.x^2 + d.y^2)) * ra, out1[b][i] = ra - refocus's per-ray
 * arithmetic (optics.py:1171-1174, element-wise IEEE float32).  out_mode 2: out0 = d.x / d.z (calc_fov, optics.py:1205), out1 = ra.
 * pupil_set_or_null [B]: batch b takes its pupil points from row pupil_set[b] of `pupil` (NULL: row b) - the same rays traced
 * under several candidate count rows are several batches sharing one row.
 * Replaces Lensgroup.trace / trace2sensor,
 * deeplens/optics.py:598-714, for Lensgroup(parity="strict"). */
int aadff_trace_rays_strict_fused(float* o, float* d, float* ra, int n, int B, const aadff_surface_t* tables_dev, int n_tables, int n_surf,
                                  const int* batch_table, const float* points_or_null, const int* point_set, const float* pupil, int N,
                                  int first, int last, int forward, const float* z_sensor_or_null, const int* pred, unsigned* bits,
                                  int origin_at_pupil, int out_mode, float* out0, float* out1, const int* pupil_set_or_null,
                                  aadff_stream_t stream);

/* psf_map of a strict-parity lens for B = S x L (focus state, wavelength) batches in ONE launch (ABI v7): per batch and object point
 * the chief rays (shrunk pupil) -> centre in ATen's summation order (as aadff_strict_centroid), the main rays -> bilinear histogram
 * (forward_integral, deeplens/monte_carlo.py:9-121, IEEE float32 divisions) -> normalised PSF; no ray state goes through memory.
 * Replaces Lensgroup.psf_diff / psf_rgb / psf_map, deeplens/optics.py:888-1026, for Lensgroup(parity="strict"), with the batch-wide
 * Newton counts speculated as in aadff_trace_rays_strict_fused:
 *   points [P][N][3] object points (optics.py:945-950), point_set [B]; tables_dev [n_tables][n_surf] (device); table_main / table_chief
 *   [B]: the table each batch's main / chief rays trace with; z_sensor [B]; pupil_main [B][spp][3], pupil_chief [B][spp_chief][3]:
 *   pupil points (optics.py:480-486, computed by the caller with the reference's own host calls);
 *   pred [B][2][AADFF_MAX_SURF] int32: predicted counts of the chief ([b][0]) and main ([b][1]) batch;
 *   psf: map_grid = 0: [B][N][ks][ks]; map_grid = g (N = g*g): [B][g*ks][g*ks] in the psf_map tiling (optics.py:1025);
 *   centre [B][N][2]; bits [B][2][2][AADFF_MAX_SURF] ([b][phase][any | nan][surface], zeroed by the call); any_valid [B]: 1 where a chief
 *   ray of the batch is valid (the assert of optics.py:901).  All pointers are device pointers.
 * job_batch_or_null [B]: the call renders the B JOBS j = 0..B-1, job j being batch job_batch[j] of the arrays above (NULL: batch j):
 *   inputs, psf and centre are indexed by the batch, pred / bits / any_valid by the job - a caller replays the few batches whose
 *   prediction failed with corrected counts, overwriting exactly their PSFs. */
int aadff_strict_psf_points(const float* points, int N, int B, const int* job_batch_or_null, const int* point_set, const aadff_surface_t* tables_dev, int n_tables,
                            int n_surf, const int* table_main, const int* table_chief, const float* z_sensor, const float* pupil_main,
                            int spp, const float* pupil_chief, int spp_chief, const int* pred, float pixel_size, int ks, int map_grid,
                            float* psf, float* centre, unsigned* bits, int* any_valid, aadff_stream_t stream);

/* aadff_strict_psf_points with TWO-VARIANT jobs (ABI v9): a batch whose chief-ray count at ONE surface is known to flip between n and
 * n + 1 from draw to draw (whether the slowest ray of the batch is still above 5e-5 after n iterations, deeplens/surfaces.py:547) is
 * rendered under both counts in the same launch instead of being re-launched when the guess was wrong.
 *   alt_or_null [B] int32 (device): per job, surface | n << 8 with pred[j][0][surface] = n + 1, or -1 (an ordinary job).
 *   The job's ordinary outputs (psf, centre, bits, any_valid) are those of the row as given (count n + 1); the bits of that run show
 *   which count the reference's loop would have stopped at.  The variant under n: psf_alt [B] x the per-batch layout of psf and
 *   centre_alt [B][N][2], indexed by the JOB; bits_alt [B][2][AADFF_MAX_SURF] (any | nan) the chief bits a launch under that row
 *   would have reported (its last any-word, never a surface's: the largest number of re-traced chief rays among the job's object
 *   points); any_valid_alt [B]: > 0 a chief ray of that variant is valid, 0 none, < 0 the variant is not available.  All zeroed by
 *   the call.  Only the chief rays whose iterate after n iterations differs from the one after n + 1 are traced twice (rf50mm at its
 *   4 / 5 flip: up to a third of an off-axis point's 2048); the main rays are traced once and binned against both centres.
 * alt_or_null = NULL is aadff_strict_psf_points. */
int aadff_strict_psf_points_alt(const float* points, int N, int B, const int* job_batch_or_null, const int* point_set, const aadff_surface_t* tables_dev,
                                int n_tables, int n_surf, const int* table_main, const int* table_chief, const float* z_sensor,
                                const float* pupil_main, int spp, const float* pupil_chief, int spp_chief, const int* pred, float pixel_size,
                                int ks, int map_grid, float* psf, float* centre, unsigned* bits, int* any_valid, const int* alt_or_null,
                                float* psf_alt, float* centre_alt, unsigned* bits_alt, int* any_valid_alt, aadff_stream_t stream);

/* Self test (no reference counterpart) of the packed float32 primitives the two-rays-per-lane strict kernels use (csrc/strict_math2.h)
 * against the compiler's IEEE forms, bit for bit: op 0: num[i] / den[i] (reciprocal refinement with packed FMAs + v_div_fixup_f32,
 * no v_div_scale_f32 pre-scaling); op 1: sqrt(num[i]) (v_sqrt_f32 + two-neighbour correction, no pre-scaling of arguments below
 * 2^-96); op 2: num[i] / (den[i] * den[i]) with the reciprocal of the squared denominator grown from the refined reciprocal of
 * den[i] (how sag / d sag share 1 / (1 + sf), deeplens/surfaces.py:787-830) against the compiler's division by the rounded square.
 * n values (device).  mismatches: 17 device words = count, then (index, bits of the packed result) of the first 8. */
int aadff_selftest_strict_ops(const float* num, const float* den, int n, int op, unsigned* mismatches, aadff_stream_t stream);

/* Chief-ray PSF centres of B batches: centre[b][p] = -(sum_s o_xy[b,s,p] ra[b,s,p]) / (sum_s ra[b,s,p] + 1e-9), o [B,spp,N,3],
 * ra [B,spp,N] (device) -> centre [B,N,2]; any_valid [B] = 1 where some ray of the batch has ra == 1 (the reference asserts it:
 * "No sampled rays is valid.", deeplens/optics.py:901).  The sums run in the ORDER of ATen's CPU `tensor.sum(0)` (cascade
 * summation of an outer reduction), so the centre has the bits the reference's psf_center (deeplens/optics.py:888-913) computes
 * on the host; oracle/aten_sum.py is the specification.  For Lensgroup(parity="strict"). */
int aadff_strict_centroid(const float* o, const float* ra, int spp, int N, int B, float* centre, int* any_valid, aadff_stream_t stream);

/* Rays from object points through the entrance pupil to the sensor.  Replaces
 * sample_from_points + trace2sensor, deeplens/optics.py:457-491,635-661.
 * points_obj [N,3] (object space, mm); u_theta,u_r [spp] raw uniform draws
 * (theta = u*2*pi, r = sqrt(u*R^2)); outputs o,d [spp,N,3], ra [spp,N]. */
int aadff_trace_points(const float* points_obj, int N, const float* u_theta, const float* u_r, int spp,
                       float pupil_z, float pupil_r, const aadff_surface_t* surf, int n_surf,
                       const aadff_lens_state_t* state, float* o_out, float* d_out, float* ra_out,
                       aadff_stream_t stream);

/* Ray-traced lens analysis: per-field spot moments in one launch, the rays are never stored.  Stratified pupil samples
 * (sample_pupil, deeplens/optics.py:539-591: sector i, ring j, theta = (u + i) 2 pi / A, r^2 = (u + j) R^2 A / spp) from
 * the object points of sample_point_source (:400-454), traced through the lens and projected to the state's d_sensor
 * (analysis_rms :1975-2012, calc_magnification3 :1221-1256).  points [P,3] (mm); u [n_pass][spp][2][P] raw uniform draws in
 * the reference's order (per sample a theta block of P, then an r^2 block of P); surf [n_pass][n_surf] (one table per pass);
 * pupil_z / pupil_r the entrance pupil; spp a multiple of num_angle, at most 2048.  One workgroup per field point runs the
 * passes in order.  Out: moments [n_pass][P][4] = (valid count, sum x, sum y, S2 = sum ra |p - c|^2), c = sum / (count +
 * 1e-4) of pass 0 (ref_mode 1) or of the pass itself (ref_mode 0); S2 = 0 when want_s2 = 0.  Fixed-order reductions (no
 * float atomics): bit-reproducible.  flags bit 0: NaN in a Newton residual. */
int aadff_spot_moments(const float* points, int P, const float* u, int spp, int num_angle, int n_pass,
                       const aadff_surface_t* surf, int n_surf, float pupil_z, float pupil_r,
                       const aadff_lens_state_t* state, int ref_mode, int want_s2, float* moments,
                       int* flags_or_null, aadff_stream_t stream);

/* Ray-traced MTF: the geometric OTF of every object point, colour, sensor plane, axis and frequency in one launch.
 * Stands for psf2mtf and draw_mtf (deeplens/optics.py:1028-1065, 1914-1941), which cut one row and one column out of a 256 x 256
 * psf_diff histogram and FFT them; here the transform is taken of the traced hits themselves.  points, u, spp, num_angle, n_pass,
 * surf, pupil and state are aadff_spot_moments': the same rays on the same draws.  Per pass q and point p, the n valid rays land at
 * (x_k, y_k) on z = d_sensor with slopes a_k = dx/dz, b_k = dy/dz; on the plane d_sensor + defocus[z] (HOST array, mm, Z <= 16) they
 * land at h_k = (x_k + a_k delta, y_k + b_k delta) around c = (mean x + mean a delta, mean y + mean b delta), plain means over the
 * valid rays.  Axes: axes_mode 0 (radial) e_T = (p_x, p_y) / hypot(p_x, p_y) of the object point ((1, 0) when both are exactly 0),
 * e_S = (-e_T.y, e_T.x); axes_mode 1 (xy) e_T = (1, 0), e_S = (0, 1).  For freqs[f] (HOST array, cycles/mm, finite and >= 0,
 * F <= 128): OTF = (1/n) sum_k exp(-2 pi i nu e.(h_k - c)), zeros when n = 0.  Both host arrays are copied into the kernel
 * arguments by the call.  Out: otf [n_pass][P][Z][2 (T, S)][F][2 (re, im)]; moments [n_pass][P][8] = (n, sum x, sum y, sum a,
 * sum b, 0, 0, 0), the first three summed in aadff_spot_moments' order.  One workgroup per point, rays kept in LDS (spp <= 2048), one
 * lane per output entry, no atomics: bit-reproducible.  flags bit 0: NaN in a Newton residual. */
int aadff_mtf_points(const float* points, int P, const float* u, int spp, int num_angle, int n_pass,
                     const aadff_surface_t* surf, int n_surf, float pupil_z, float pupil_r,
                     const aadff_lens_state_t* state, const float* freqs, int F, const float* defocus, int Z,
                     int axes_mode, float* otf, float* moments, int* flags_or_null, aadff_stream_t stream);

/* Ray-traced image rendering (no counterpart in the reference snapshot, whose 'raytracing' branch of
 * render_single_img calls methods it does not define).  For every pixel (i, j) of an H x W sensor and every channel c (surf_rgb
 * [3][n_surf]: the tables of WAVE_RGB), spp rays leave the sensor point (-sensor_w/2 + (j+1) ps, sensor_h/2 - (i+1) ps, d_sensor)
 * (sample_sensor, deeplens/optics.py:494-535; d_sensor is read from `state` on the device) towards stratified points of the exit
 * pupil (pupil_z, pupil_r; sample_pupil with 8 sectors: sample s has sector s / (spp/8), ring s % (spp/8), theta = (u[c,s,0,i,j] +
 * sector) 2 pi / 8, r^2 = (u[c,s,1,i,j] + ring) pupil_r^2 8 / spp), are traced backwards through all surfaces and propagated to
 * z = depth (< 0), where they land at (px, py).  Scene coordinates uj = W/2 - 1 - px / (scale ps), vi = H/2 - 1 + py / (scale ps); a
 * ray counts if it survived every surface and -1 <= uj <= W, -1 <= vi <= H; its value is the bilinear sample of img[b, c] at (vi, uj)
 * (texel centres at integers, indices clamped to the image).  out [B,3,H,W] = sum value / count, 0 where count = 0; with vignetting
 * != 0 sum value / spp.  count_or_null [3,H,W] the valid rays per pixel (float), valid_or_null [3,spp,H,W] the per-ray validity
 * (bytes; diagnostics).  u_or_null [3,spp,2,H,W] raw uniforms, or NULL: the kernel then draws uniform number idx (the flat index
 * into that array) as aadff_sensor_uniforms(seed) defines it.  spp a multiple of 8.  One lane per (pixel, channel), no atomics:
 * bit-reproducible; B > 4 runs as launches of 4 images over the same rays.  flags bit 0: NaN in a Newton residual. */
int aadff_render_raytraced(const float* img, int B, int H, int W, const float* u_or_null, unsigned long long seed, int spp,
                           const aadff_surface_t* surf_rgb, int n_surf, float pupil_z, float pupil_r, float sensor_w, float sensor_h,
                           float pixel_size, float depth, float scale, int vignetting, const aadff_lens_state_t* state, float* out,
                           float* count_or_null, unsigned char* valid_or_null, int* flags_or_null, aadff_stream_t stream);

/* Ray-traced rendering of a layered RGB-D scene.  Sensor points, pupil samples, uniforms / seed, trace and scene
 * coordinates are aadff_render_raytraced's.  The scene is L planes (1 <= L <= AADFF_RENDER_MAX_LAYERS) at layer_depths[l] (HOST
 * array, mm: 0 > z_0 > z_1 > ... nearest first) with scales[l] (HOST array, object mm per sensor mm at plane l), and layer [B,H,W]
 * (bytes, device): the plane each texel of image b lies on; an index >= L lies on none (a hole).  Both host arrays are copied into the
 * kernel arguments by the call.  Every ray that survived the lens starts with T = 1, A = 0, V = 0 per image and visits l = 0 .. L-1:
 * propagated from its last surface to z_l it meets the plane if -1 <= uj <= W, -1 <= vi <= H (coordinates with scales[l]); with the
 * four texels and bilinear weights of aadff_render_raytraced, a = the bilinear form of m_t = (layer[b,t] == l), q = the same form of
 * (m_t ? img[b,c,t] : 0); then V += T q, A += T a, T *= 1 - a.  out [B,3,H,W] = sum V / sum A over the pixel's rays, 0 where sum A = 0;
 * with vignetting != 0 sum V / spp.  coverage_or_null [B,3,H,W] = sum A; alive_or_null [3,H,W] the rays that survived the lens (float);
 * alive_rays_or_null [3,spp,H,W] bytes, per ray (diagnostics).  With L = 1 and layer == 0 the output equals aadff_render_raytraced's bit
 * for bit and coverage its count.  No atomics: bit-reproducible; B > 4 runs as launches of 4 images over the same rays, an image
 * renders to the same bits in any of them.  flags bit 0: NaN in a Newton residual. */
#define AADFF_RENDER_MAX_LAYERS 32
int aadff_render_raytraced_layered(const float* img, const unsigned char* layer, int B, int H, int W, const float* u_or_null,
                                   unsigned long long seed, int spp, const aadff_surface_t* surf_rgb, int n_surf, float pupil_z,
                                   float pupil_r, float sensor_w, float sensor_h, float pixel_size, int L, const float* layer_depths,
                                   const float* scales, int vignetting, const aadff_lens_state_t* state, float* out,
                                   float* coverage_or_null, float* alive_or_null, unsigned char* alive_rays_or_null, int* flags_or_null,
                                   aadff_stream_t stream);

/* The uniforms aadff_render_raytraced draws when it is given none: out [3,spp,2,H,W], element idx = output idx of the SplitMix64
 * sequence seeded with `seed` (z = seed + (idx+1) 0x9E3779B97F4A7C15; z = (z ^ z>>30) 0xBF58476D1CE4E5B9; z = (z ^ z>>27)
 * 0x94D049BB133111EB; z ^= z>>31), its top 24 bits times 2^-24: values in [0, 1). */
int aadff_sensor_uniforms(unsigned long long seed, int spp, int H, int W, float* out, aadff_stream_t stream);

/* Bilinear splat of sensor hits into ks x ks histograms + normalisation.  Replaces
 * forward_integral / assign_points_to_pixels, deeplens/monte_carlo.py:9-121 and the
 * division of deeplens/optics.py:978.  o [spp,N,3], ra [spp,N], centre [N,2];
 * psf_raw_or_null / psf [N,ks,ks].  ra is a weight (0: a dead ray): as in the reference (monte_carlo.py:38) a hit inside
 * the window is scaled by it about the centre before it is binned; one that a weight above 1 carries out of the window is dropped. */
int aadff_psf_splat(const float* o, const float* ra, const float* centre, int spp, int N,
                    float pixel_size, int ks, float* psf_raw_or_null, float* psf,
                    aadff_stream_t stream);

/* Fused PSF of N normalised points for S focus states and L wavelengths in ONE launch:
 * object-space mapping, chief-ray centre pass (shrunk pupil, `surf_chief` table), main
 * pass, splat, normalise.  Replaces Lensgroup.psf_diff / psf_rgb / psf_map,
 * deeplens/optics.py:888-1026.
 *   points      [S,N,3]  normalised (x,y in [-1,1], z = depth mm < 0)
 *   surf_main   [L][n_surf], surf_chief [n_surf]
 *   states      [S]
 *   u_main      raw uniforms: theta row at u_main + s*main_stride_s + l*main_stride_l, r row spp
 *               floats after it (dense [S,L,2,spp] has strides 2*L*spp, 2*spp)
 *   u_chief     same with spp_chief and its own strides (any layout that keeps the host
 *               generator's draw order can be consumed without a re-layout copy)
 *   centre_mode 1: chief-ray centre (center=True); 0: ideal perspective centre (optics.py:970-975)
 *   map_layout  0: psf [S,N,L,ks,ks] ; 1: psf_map layout [S,L,g*ks,g*ks] with N = g*g (optics.py:1025)
 *   centre_out_or_null [S,L,N,2]
 *   flags_or_null: see aadff_publish_flags.  A point whose rays all miss the ks x ks window gets a 0/0 = NaN PSF, as in
 *   the reference (optics.py:978, monte_carlo.py:37).
 */
int aadff_psf_points(const float* points, int S, int N, int L,
                     const aadff_surface_t* surf_main, const aadff_surface_t* surf_chief,
                     aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l,
                     const float* u_chief, int spp_chief, long chief_stride_s, long chief_stride_l,
                     int ks, int centre_mode, int map_layout, float* psf, float* centre_out_or_null,
                     int* flags_or_null, aadff_stream_t stream);

/* Upload of the uniform blocks of focus states [first_slice, S) folded into an
 * aadff_psf_points launch: a few leading workgroups copy src_host (PINNED host memory,
 * [S][slice_stride] floats, the layout u_main/u_chief index into) to dst_dev and bump
 * counters[s]; the PSF workgroups of those states wait for counters[s] to reach
 * generation * (number of copy workgroups); HIP guarantees no dispatch order, so the wait is bounded and a
 * workgroup whose block is late reads its draws from src_host directly (flag bit 3 reports the lost overlap).  Blocks of states < first_slice must already be
 * in dst_dev (aadff_refocus_staged with n_u = first_slice*slice_stride puts them there, hidden
 * behind the focus traces).  counters: [S] device words zeroed once; generation = 1, 2, 3 ...
 * for successive launches on the same counters (same S, N, L, slice_stride each time). */
typedef struct aadff_stage {
    const float* src_host;
    float*       dst_dev;
    long         slice_stride;
    int          first_slice;
    unsigned     generation;
    unsigned*    counters;
} aadff_stage_t;

int aadff_psf_points_staged(const float* points, int S, int N, int L,
                     const aadff_surface_t* surf_main, const aadff_surface_t* surf_chief,
                     aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l,
                     const float* u_chief, int spp_chief, long chief_stride_s, long chief_stride_l,
                     int ks, int centre_mode, int map_layout, float* psf, float* centre_out_or_null,
                     int* flags_or_null, const aadff_stage_t* stage, aadff_stream_t stream);

/* Chief-centre fit.  Where no chief ray of a point is vignetted, the sensor hit is a smooth function of the pupil position, and the
 * chief centre - its mean over the spp_chief draws - equals sum_k w_k hit(node_k) over AADFF_CHIEF_NODES fixed nodes of the shrunk
 * pupil, with weights that follow from the monomial moments of the SAME draws (not the continuous pupil integral: the result is this
 * draw's sample mean up to the truncation of a degree-AADFF_CHIEF_DEGREE fit).  The draws are shared by all points of a (state,
 * wavelength), so the weights are computed once per launch:
 *   aadff_chief_fit_weights: weights [S][L][2][AADFF_CHIEF_NODES] (degree d, then degree d - 2) from the u_chief block the PSF launch
 *     will read (same pointer and strides).  stage_or_null: the aadff_stage_t of the staged PSF launch that follows on the same
 *     stream - the draws of states >= first_slice are then read from the pinned host block, where they still are.
 *   aadff_psf_points_fit / aadff_psf_points_staged_fit: aadff_psf_points / _staged with that buffer and fit_centres, scratch of
 *     [S][L][N][4] floats (16-byte aligned).  With centre_mode 1 and spp_chief >= 4 * AADFF_CHIEF_RAYS, a launch of one wave per
 *     (point, state) in front of the PSF launch traces the nodes and a guard ring at 1.05 x the shrunk-pupil radius
 *     (AADFF_CHIEF_RAYS rays in all); the fitted centre stands if every one of those rays is alive and the degree-d and
 *     degree-(d - 2) centres agree; otherwise the PSF workgroup traces every draw, as without weights and with the same bits.
 *     fit_weights_or_null = NULL, or AADFF_PSF_CHIEF=full in the environment (read per launch), is aadff_psf_points / _staged.
 *   aadff_chief_fit_tables (host only, for tests): node_xy [AADFF_CHIEF_RAYS][2] in the unit disc (nodes, centre first, then the
 *     ring); fit [66][AADFF_CHIEF_NODES] and fit_low [45][AADFF_CHIEF_NODES]: pinv(V)^T of the monomial bases of total degree d and
 *     d - 2 (x^(t-b) y^b, ordered by t then b), transposed.  tools/gen_chief_fit_tables.py generates them. */
#define AADFF_CHIEF_NODES 85
#define AADFF_CHIEF_RAYS 128
#define AADFF_CHIEF_DEGREE 10
#define AADFF_CHIEF_FIT_TOL 1e-6f     /* mm, either axis: the largest |centre_d - centre_(d-2)| a fitted centre may have */
int aadff_chief_fit_weights(const float* u_chief, int S, int L, int spp_chief, long chief_stride_s, long chief_stride_l,
                            const aadff_stage_t* stage_or_null, float* weights, aadff_stream_t stream);
int aadff_psf_points_fit(const float* points, int S, int N, int L,
                     const aadff_surface_t* surf_main, const aadff_surface_t* surf_chief,
                     aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l,
                     const float* u_chief, int spp_chief, long chief_stride_s, long chief_stride_l,
                     int ks, int centre_mode, int map_layout, float* psf, float* centre_out_or_null,
                     int* flags_or_null, const float* fit_weights_or_null, float* fit_centres, aadff_stream_t stream);
int aadff_psf_points_staged_fit(const float* points, int S, int N, int L,
                     const aadff_surface_t* surf_main, const aadff_surface_t* surf_chief,
                     aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l,
                     const float* u_chief, int spp_chief, long chief_stride_s, long chief_stride_l,
                     int ks, int centre_mode, int map_layout, float* psf, float* centre_out_or_null,
                     int* flags_or_null, const aadff_stage_t* stage, const float* fit_weights_or_null, float* fit_centres, aadff_stream_t stream);
int aadff_chief_fit_tables(double* node_xy, double* fit, double* fit_low);

/* Pupil points once per stack.  The pupil point of a draw depends on (state, wavelength, draw) alone, and every one of the N point
 * workgroups of a (state, wavelength) used to map the same draws again.  A fit launch can read the points instead:
 *   aadff_chief_fit_prologue: aadff_chief_fit_weights (same weights, to the bit) which also maps the main draws (lc.enp_r2) and the
 *     chief draws (lc.enp_r2_shrunk) of every (state, wavelength) with the PSF kernel's own mapping and writes them to pupil_xy:
 *     [S][L] blocks of {main x [spp], main y [spp], chief x [spp_chief], chief y [spp_chief]} floats - the block of draws with x in
 *     place of theta and y in place of r.  u_main / u_chief and their strides are what the PSF launch gets; with a stage, both must
 *     point into dst_dev and the draws of states >= first_slice are read from the pinned host block.
 *   aadff_psf_points_fit_pts / aadff_psf_points_staged_fit_pts: aadff_psf_points_fit / _staged_fit with those points.  Where the launch
 *     carries fitted centres (see above) its workgroups load points instead of draws; nothing reads the device copy of the draws then,
 *     so the staged entry copies nothing, waits for nothing and only keeps stage->counters in step with stage->generation (a later
 *     launch on the same counters may stage again).  A launch without fitted centres (no weights, centre_mode 0, few chief draws,
 *     AADFF_PSF_CHIEF=full), pupil_xy_or_null = NULL, or AADFF_PSF_POINTS=raw in the environment is aadff_psf_points_fit / _staged_fit.
 * Environment, read per launch, for A/B runs and tests: AADFF_PSF_POINTS=raw (above; the prologue then writes no points),
 * AADFF_CHIEF_CENTRES=per_wavelength (the node rays traced by a wave per (point, wavelength, state) instead of once per (point,
 * state): the same centres, to the bit), AADFF_PSF_LAUNCHES=parent (both). */
int aadff_chief_fit_prologue(const float* u_main, int spp, long main_stride_s, long main_stride_l,
                             const float* u_chief, int S, int L, int spp_chief, long chief_stride_s, long chief_stride_l,
                             aadff_lens_const_t lc, const aadff_stage_t* stage_or_null, float* weights, float* pupil_xy,
                             aadff_stream_t stream);
int aadff_psf_points_fit_pts(const float* points, int S, int N, int L,
                     const aadff_surface_t* surf_main, const aadff_surface_t* surf_chief,
                     aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l,
                     const float* u_chief, int spp_chief, long chief_stride_s, long chief_stride_l,
                     int ks, int centre_mode, int map_layout, float* psf, float* centre_out_or_null,
                     int* flags_or_null, const float* fit_weights_or_null, float* fit_centres, const float* pupil_xy_or_null,
                     aadff_stream_t stream);
int aadff_psf_points_staged_fit_pts(const float* points, int S, int N, int L,
                     const aadff_surface_t* surf_main, const aadff_surface_t* surf_chief,
                     aadff_lens_const_t lc, const aadff_lens_state_t* states,
                     const float* u_main, int spp, long main_stride_s, long main_stride_l,
                     const float* u_chief, int spp_chief, long chief_stride_s, long chief_stride_l,
                     int ks, int centre_mode, int map_layout, float* psf, float* centre_out_or_null,
                     int* flags_or_null, const aadff_stage_t* stage, const float* fit_weights_or_null, float* fit_centres,
                     const float* pupil_xy_or_null, aadff_stream_t stream);

/* "Edge-exact" PSF grid (ABI v8; Lensgroup(parity="edge")): aadff_psf_points with the one decision the float32 noise of a trace
 * can flip taken out of the fast kernel.  The histogram's only discontinuity is the window test of deeplens/monte_carlo.py:37
 * (`|s| < R - 0.01 ps`): a hit within the noise of that edge lands inside or outside depending on the last bit of the trace
 * (deeplens/surfaces.py:523-586: the batch-wide Newton loop), and a flipped border ray changes a cropped PSF by 1 / (rays inside).
 * Three calls on one stream replace Lensgroup.psf_map, deeplens/optics.py:888-1026, for S focus states whose d_sensor / hfov the
 * caller computed in the reference's arithmetic (aadff_trace_rays_strict_fused levels, aadff/strict_stack.py):
 *   1. aadff_psf_points_edge: arguments as aadff_psf_points (chief-ray centres, centre_mode 1).  A live ray whose hit lies within
 *      delta_mm of the window edge is NOT splatted but appended as (point << 16 | sample) to edge_list[s*L + l][edge_cap], its job's
 *      edge_count[s*L + l] incremented (zeroed by the call; a count above edge_cap means rays were dropped).  raw [S*L][N][ks*ks]
 *      receives the UNNORMALISED histograms of all other rays, centre_out [S,L,N,2] the centres.
 *   2. aadff_strict_edge_retrace (csrc/strict_fused.hip): re-traces the listed rays of the B = S*L batches in the reference's float32
 *      operation order - arguments as aadff_strict_psf_points (object points and pupil points from the reference's host arithmetic,
 *      pred[b][1] = the main batch's Newton counts) - applies forward_integral's window test and bilinear taps to that hit with
 *      `centre` = step 1's centres, and adds the taps to raw.  flags bit 4: a list overflowed.
 *      PROVISIONAL STATES: step 1 may run on lens states that are only close to the exact ones (the fast refocus kernel's, a few
 *      ulps off) so that it overlaps the strict refocus / calc_fov round trips; it then also writes slope_out [S,L,N,2], the mean
 *      direction tangents of the valid chief rays, and step 2 - given states_prov [P] (what step 1 ran on), tan_exact [P] =
 *      float(tan(hfov)) and z_sensor of the exact states - moves each centre into the exact world before the window test:
 *      c = (c - slope * (d_exact - d_prov)) * tan_exact / tan_prov.  states_prov_or_null = NULL: step 1 ran on the exact states.
 *   3. aadff_psf_normalise: raw -> psf in either layout of aadff_psf_points (the division of optics.py:978; same summation order as
 *      aadff_psf_points: a PSF none of whose rays was deferred is what aadff_psf_points writes for the same states, up to the
 *      order of the float atomics of its LDS histogram, which no two launches share). */
int aadff_psf_points_edge(const float* points, int S, int N, int L,
                          const aadff_surface_t* surf_main, const aadff_surface_t* surf_chief,
                          aadff_lens_const_t lc, const aadff_lens_state_t* states,
                          const float* u_main, int spp, long main_stride_s, long main_stride_l,
                          const float* u_chief, int spp_chief, long chief_stride_s, long chief_stride_l,
                          int ks, float delta_mm, float* raw, float* centre_out, float* slope_out_or_null,
                          unsigned* edge_count, unsigned* edge_list, int edge_cap,
                          int* flags_or_null, aadff_stream_t stream);
int aadff_strict_edge_retrace(const float* points, int N, int B, const int* point_set, const aadff_surface_t* tables_dev, int n_tables,
                              int n_surf, const int* table_main, const float* z_sensor, const float* pupil_main, int spp,
                              const int* pred, float pixel_size, int ks, const float* centre, const unsigned* edge_count,
                              const unsigned* edge_list, int edge_cap, float* raw, int* flags_or_null,
                              const aadff_lens_state_t* states_prov_or_null, const float* tan_exact, const float* slope,
                              aadff_stream_t stream);
int aadff_psf_normalise(const float* raw, int S, int N, int L, float pixel_size, int ks, int map_layout, float* psf,
                        aadff_stream_t stream);

/* Fused PSF-surrogate network: P rows of (x, y, z, foc_z) -> MLP (Linear+ReLU ..., Linear+Sigmoid) -> L1-normalise
 * -> mode 0: psf_out[P][n_out] (PSFNet.pred, deeplens/psfnet.py:375-390, psfnet_arch.py:24-47), or
 *    mode 1: out[N][C][H][W] = per-pixel PSF gather over img (PSFNet.render + local_psf_render,
 *            deeplens/psfnet.py:393-441, deeplens/render_psf.py:76-107; P = N*H*W, ks*ks = n_out).
 *            out_slices = S > 0: a whole focal stack in one launch (2_aber_aware_dff_aif.py:104-114): inp holds
 *            P = B*S*H*W rows ordered [b][slice][y][x], img is [B][C][H][W], out is [B][C][S][H][W].
 * Layer l maps in_features[l] -> out_features[l] (widths <= 256, in_features[0] == 4, n_out <= 128).
 * wpack: the weights as exact fp16 (hi, lo) pairs in MFMA fragment order, per layer
 *   [out tile 16][k-step 32][plane hi|lo][lane 64][8 halves]: lane (m = lane&15, kg = lane>>4) holds
 *   weight[16*tile + m][32*step + 8*kg + 0..7], hi = fp16(w), lo = fp16(w - hi), zero-padded;
 * bias: per layer out_features padded to 16, concatenated.  (aadff/psfnet_pack.py builds both.) */
#define AADFF_PSFNET_MAX_LAYERS 16
int aadff_psfnet_forward(const float* inp, long P, const void* wpack, const float* bias, int n_layers,
                         const int* in_features, const int* out_features, int mode, float* psf_out,
                         const float* img, float* out, int C, int H, int W, int ks, int out_slices, int precision,
                         int* flags_or_null, aadff_stream_t stream);
/* precision (both psfnet entries): 0 = fp32-equivalent (fp16 hi/lo operand split, three MFMAs per product: <= 2e-7 from
 * torch fp32); 1 = fp16 single pass (opt-in: operands rounded to fp16, one MFMA per product, PSFs ~5e-4 relative).
 * flags_or_null (both psfnet entries): bit 4 is ORed in when a hidden activation exceeded 65504, the largest value the
 * fp16 hi half of the split operand can carry — the affected outputs are then inf/NaN garbage and the caller must not
 * use them (the shipped rf50mm checkpoint peaks at 41, tests/golden/g11_ckpt_activation_range.json). */

/* PSFNet.render for a whole RGB-D focal stack with the network input generated in the kernel
 * (deeplens/psfnet.py:393-441 per slice, 2_aber_aware_dff_aif.py:104-114 for the stack): row (n, s, y, x) =
 * (xs[x], ys[y], clamp((depth[n][y][x] - d_min) * inv_range, 0, 1), foc_z[n][s]); out [N,C,S,H,W] (S = 1: [N,C,H,W]).
 * xs = linspace(-1, 1, W), ys = linspace(1, -1, H) (psfnet.py:427-431), foc_z = depth2z(foc_dist) (psfnet.py:447-450),
 * inv_range = 1 / (d_max - d_min) in fp32. */
int aadff_psfnet_render_rgbd(const float* depth, const float* xs, const float* ys, const float* foc_z, float d_min,
                             float inv_range, long N, int S, const void* wpack, const float* bias, int n_layers,
                             const int* in_features, const int* out_features, const float* img, float* out, int C, int H,
                             int W, int ks, int precision, int* flags_or_null, aadff_stream_t stream);

/* Gradients of aadff_psfnet_render_rgbd (precision 0) to the image, the depth map and foc_z (csrc/psfnet_bwd.hip), i.e. the
 * autograd of PSFNet.render over the slice loop: deeplens/psfnet.py:393-450 (coordinate rows, depth2z = torch.clamp :447-450),
 * deeplens/psfnet_arch.py:24-47 (Linear + ReLU ..., Linear + Sigmoid, F.normalize p=1) and deeplens/render_psf.py:76-107
 * (per-pixel gather, replicate padding).  The network weights get no gradient.  Nothing is kept from the forward: the
 * kernel recomputes it with the forward's arithmetic, keeps one ReLU mask bit per hidden unit on the CU and runs the
 * transposed chain on the matrix cores with the forward's fp16 hi/lo operand split, every row scaled by a power of two.
 *   dy [N,C,S,H,W] contiguous; wtpack: the TRANSPOSED weights in the fragment order of wpack, per layer
 *   [in tile 16][k-step 32 over out_features][plane hi|lo][lane 64][8 halves] of W_l^T * 2^wt_exp[l], |wt_exp[l]| <= 64: a power
 *   of two per layer that keeps the lo halves of small weights out of fp16's subnormal range; the kernel undoes the product of
 *   the scales at the end (aadff/psfnet_pack.py: pack_transposed).  Both may be NULL when only d_img is asked for.
 *   d_depth [N,H,W]: sum over the slices in slice order of d_z * inv_range where 0 <= (depth - d_min) * inv_range <= 1,
 *     exactly 0 outside (the autograd of torch.clamp);  d_foc_z [N,S];  d_img [N,C,H,W]: sum over the slices in slice order.
 * An output whose pointer is NULL is not computed (all NULL is an error).  workspace: device memory of at least
 * aadff_psfnet_render_rgbd_bwd_workspace bytes: 4 bytes per row (n, s, y, x) and 4 per 64 rows when d_depth or d_foc_z is
 * asked for (need_input), the network input and the PSFs of ONE slice (H*W*(4 + ks*ks) floats) when d_img is (need_img).
 * Every sum has a fixed order (no float atomics): bitwise reproducible.  Arguments are checked before any HIP call. */
int aadff_psfnet_render_rgbd_bwd(const float* depth, const float* xs, const float* ys, const float* foc_z, float d_min,
                                 float inv_range, long N, int S, const void* wpack, const float* bias, const void* wtpack,
                                 const int* wt_exp, int n_layers, const int* in_features, const int* out_features, const float* img,
                                 const float* dy, int C, int H, int W, int ks, float* d_img_or_null, float* d_depth_or_null,
                                 float* d_foc_z_or_null, void* workspace, size_t workspace_bytes, aadff_stream_t stream);
/* Workspace bytes of the call above (host arithmetic only, no device needed). */
int aadff_psfnet_render_rgbd_bwd_workspace(long N, int S, int C, int H, int W, int ks, int need_input, int need_img,
                                           size_t* bytes);

/* Refocus S lens states in one launch: trace spp rays from (0,0,depth[s]) (green table),
 * least-squares axis crossing -> d_sensor, then hfov/foclen/fnum.  Replaces
 * Lensgroup.refocus + post_computation + calc_fov + calc_efl,
 * deeplens/optics.py:1155-1217,178-187,1097-1102.  depth [S] (mm, <0); u: theta row at
 * u + s*u_stride_s, r row spp floats after it (dense [S,2,spp]: stride 2*spp). */
int aadff_refocus(const float* depth, int S, const float* u, int spp, long u_stride_s,
                  const aadff_surface_t* surf_green, aadff_lens_const_t lc,
                  aadff_lens_state_t* states, aadff_stream_t stream);

/* aadff_refocus with the host->device upload of the step's uniform block folded into the same
 * launch: u_host is PINNED host memory (hipHostMalloc / torch pin_memory) in the layout
 * aadff_psf_points will read; the S focus workgroups read their 2*spp draws
 * (u_host + s*u_stride_s) over PCIe while extra workgroups copy its first n_u floats to u_dev
 * (the rest can ride on the PSF launch, aadff_psf_points_staged).
 * Saves the separate hipMemcpyAsync and its queue gap in front of a focal stack
 * (the torch.rand draws of deeplens/optics.py:480-481,1166 stay on the host, Appendix B).
 * Both pointers 16-byte aligned.  The host block may be reused once this launch completed.
 * The rays of a focus state are traced by 4 workgroups; `scratch` (64 bytes per focus state,
 * device memory, zeroed once by the caller, not shared by concurrent launches) carries their
 * partial sums to the one that finishes the state (fixed summation order: deterministic). */
int aadff_refocus_staged(const float* depth, int S, const float* u_host, float* u_dev, long n_u, int spp,
                         long u_stride_s, const aadff_surface_t* surf_green, aadff_lens_const_t lc,
                         aadff_lens_state_t* states, void* scratch, aadff_stream_t stream);

/* The device-visible address of a block of PINNED host memory (error when it is not device-mapped).  The per-call mirror of
 * Lensgroup.refocus / psf_map (deeplens/optics.py:1155-1180, :888-1026) passes such addresses to aadff_refocus (draws and depth
 * read over PCIe by the one workgroup) and as `points` of aadff_psf_points_staged, so that no copy is queued in front of a launch. */
int aadff_host_device_pointer(const void* host, void** dev_out);

/* hfov/foclen/fnum for states whose d_sensor is already set (lens load, or a caller
 * that assigns d_sensor).  Replaces post_computation, deeplens/optics.py:178-187. */
int aadff_post_computation(int S, const aadff_surface_t* surf_green, aadff_lens_const_t lc,
                           aadff_lens_state_t* states, aadff_stream_t stream);

/* Copy the flags word the PSF / refocus kernels OR into (bit 0: NaN in a Newton residual — the reference exits,
 * deeplens/surfaces.py:555-558; bit 1: no valid chief ray, the assert of deeplens/optics.py:901; bit 2: a focus state
 * without a positive sensor position, i.e. a refocus that found no valid ray - "sensor position is negative.",
 * deeplens/optics.py:1176; bit 3: a staged upload arrived late and the samples were read over PCIe instead) to a PINNED host word from inside the stream:
 * the host can then poll the reference's error conditions of pipelined stacks without a device synchronisation
 * (it reads the mirror after an event it waits on anyway).  One 64-thread launch. */
int aadff_publish_flags(const int* flags_dev, int* mirror_host, aadff_stream_t stream);

/* One optimisation step of the PSF-network fit on a FLAT fp32 parameter buffer: torch.optim.AdamW (betas, eps, decoupled
 * weight decay) with the learning rate of CosineAnnealingLR(T_max = t_max, eta_min = 0) evaluated in the kernel from the
 * device step counter (`*step_dev` = completed steps; incremented by this call), so the launch pair is HIP-graph
 * capturable with no host-side scalar.  Replaces the optimiser half of deeplens/psfnet.py:85-108 (AdamW + scheduler.step()).
 *   grad: fp32 [n], or bf16 [n] with grad_is_bf16 != 0 (gradients of the bf16 parameter copy)
 *   param_bf16_or_null: bf16 [n] copy of the updated parameters (round to nearest even) for the bf16 leg
 *   scratch4: 4 device floats (the step's scalars, written by a one-thread launch in front of the update) */
int aadff_adamw_step(float* param, const void* grad, int grad_is_bf16, float* exp_avg, float* exp_avg_sq,
                     void* param_bf16_or_null, long n, int* step_dev, float* scratch4, float lr0, int t_max, float beta1,
                     float beta2, float eps, float weight_decay, aadff_stream_t stream);

/* Two fused pieces of the fit step's backward (HIP-graph capturable, fp32 or bf16 tensors):
 * aadff_relu_bwd_bias: dz = dy * (y > 0) and db = column sums of dz for one hidden layer ([M,N] row-major) — the
 *   ReLU backward + bias gradient of deeplens/psfnet_arch.py:24-41 under autograd;
 * aadff_psfnet_head_loss_grad: pred = L1-normalised sigmoid(z) (psfnet_arch.py:41-47), and dz = d/dz of
 *   nn.MSELoss()(pred, target) (deeplens/psfnet.py:94-106) for z [B,N], N <= 128; pred and target are fp32. */
int aadff_relu_bwd_bias(const void* dy, const void* y, void* dz, void* db, int M, int N, int is_bf16, aadff_stream_t stream);
int aadff_psfnet_head_loss_grad(const void* z, const float* target, float* pred, void* dz, int B, int N, int is_bf16,
                                aadff_stream_t stream);

/* The fit step of the PSF network as hand-written bf16 MFMA kernels (csrc/mlp_train.hip; used by aadff/mlp_fit.py), i.e. the
 * autograd graph of deeplens/psfnet.py:94-106 over deeplens/psfnet_arch.py:24-47 without torch autograd:
 * aadff_fit_gemm_nt: out[b][a] = sum_c A[a][c] B[b][c] for bf16 A [na][lda], B [nb][ldb], contraction nc <= 256, with
 *   epilogue 0 forward (+ bias[a], bf16 out [nb][ld_out] and optional transposed copy outT [na][ld_outT]),
 *            1 forward + ReLU,
 *            2 dX (multiply by mask[b][a] > 0 — the forward output —, bf16 out / outT, dbias[a] += column sums, fp32 atomics),
 *            3 dW (fp32 out [nb][ld_out]);
 *   leading dimensions multiples of 8 (operands) / 4 (outputs), padding zero, na a multiple of 4;
 * aadff_fit_layer_bwd: the backward of one layer in ONE launch: dW [n][k] fp32 = dzT [n][:batch] . xT_prev [k][:batch], and,
 *   when wT != NULL, the dX epilogue for the layer below: dz_prev [batch][k] = (dz [batch][:n] . wT [k][:n]) masked by
 *   x_prev > 0, its transposed copy dzT_prev and dbias_prev[k] += column sums;
 * aadff_fit_input: fp32 batch [B][K] -> bf16 x [B][ld_x] and xT [K][ld_xT];
 * aadff_fit_head: sigmoid + L1 normalise + MSE gradient for logits z [B][ld_z] bf16 -> pred fp32 [B][N], dz / dzT bf16,
 *   dbias += column sums; when step_dev != NULL it also prepares the optimiser step (scalars into scratch4 as in
 *   aadff_adamw_step, step counter += 1) for the aadff_fit_adamw that follows in the same stream;
 * aadff_fit_adamw: AdamW on flat fp32 parameters with fp32 gradients (zeroed after use), refreshing the bf16 operand
 *   copies param_bf16[dst[i]] and, where dst_t[i] >= 0, param_bf16[dst_t[i]] (the transposed weights). */
/* The same step in THREE launches (aadff_fit_chain = 2, then aadff_fit_adamw): a workgroup takes 16 rows of the batch through
 * input cast, every Linear(+ReLU), the head and the whole dX chain with the activations in LDS (rows only meet in dW), then
 * one launch computes dW of all layers.  `aadff_fit_net` describes the network and its buffers:
 *   param_bf16:   W_l at off_w and W_l^T at off_wt in MFMA FRAGMENT ORDER - a matrix M [rows][cols] (W: n x k, W^T: k x n) is stored as
 *                 [row / 16][col / 32][lane = ((col % 32) / 8) * 16 + row % 16][col % 8], zero padded to whole 16-row tiles and
 *                 32-column steps, so that a wave-instruction reads 1 KiB contiguously; bias_l [up4(n)] at off_b (bf16; offsets in
 *                 elements, multiples of 8; refreshed by aadff_fit_adamw through its destination maps; ld_k / ld_n are not used
 *                 by this entry);
 *   scratch_bf16: X_l^T [k_l][ld_batch] at off_xt[l] (l = 0..L-1) and dZ_l^T [n_{l-1}][ld_batch] at off_dzt[l] (l = 1..L), written
 *                 by the chain kernel, read by the dW kernel (zero padded columns batch..ld_batch);
 *   grad (fp32):  dW_l [n][k] at off_gw (stored), db_l [n] at off_gb (ADDED by atomics: must be zero on entry; aadff_fit_adamw
 *                 leaves it zero);
 *   inp [B][k_0], target / pred [B][n_last] fp32.   Widths <= 256, input widths multiples of 4, n_last <= 128, B <= 256.
 * When step_dev != NULL the chain also prepares the optimiser step as aadff_fit_head does. */
#define AADFF_FIT_MAX_LAYERS 16
typedef struct aadff_fit_net {
    int n_layers, batch, ld_batch;
    int k[AADFF_FIT_MAX_LAYERS], n[AADFF_FIT_MAX_LAYERS];
    int ld_k[AADFF_FIT_MAX_LAYERS], ld_n[AADFF_FIT_MAX_LAYERS];
    int off_w[AADFF_FIT_MAX_LAYERS], off_wt[AADFF_FIT_MAX_LAYERS], off_b[AADFF_FIT_MAX_LAYERS];
    int off_xt[AADFF_FIT_MAX_LAYERS + 1], off_dzt[AADFF_FIT_MAX_LAYERS + 1];
    int off_gw[AADFF_FIT_MAX_LAYERS], off_gb[AADFF_FIT_MAX_LAYERS];
    const void* param_bf16;
    void* scratch_bf16;
    float* grad;
    const float* inp;
    const float* target;
    float* pred;
} aadff_fit_net;
int aadff_fit_chain(const aadff_fit_net* net, int* step_dev, float* scratch4, float lr0, int t_max, float beta1, float beta2,
                    float weight_decay, aadff_stream_t stream);
int aadff_fit_gemm_nt(const void* A, int lda, int na, const void* B, int ldb, int nb, int nc, int epilogue, void* out,
                      int ld_out, void* outT, int ld_outT, const void* bias, const void* mask, int ld_mask, float* dbias,
                      aadff_stream_t stream);
int aadff_fit_layer_bwd(const void* xT_prev, int ld_xT, int k, const void* dzT, int ld_dzT, int n, int batch, float* dW,
                        const void* wT, int ld_wT, const void* dz, int ld_dz, const void* x_prev, int ld_x, void* dz_prev,
                        int ld_dzp, void* dzT_prev, int ld_dzTp, float* dbias_prev, aadff_stream_t stream);
int aadff_fit_input(const float* inp, void* x, int ld_x, void* xT, int ld_xT, int B, int K, aadff_stream_t stream);
int aadff_fit_head(const void* z, int ld_z, const float* target, float* pred, void* dz, int ld_dz, void* dzT, int ld_dzT,
                   float* dbias, int B, int N, int* step_dev, float* scratch4, float lr0, int t_max, float beta1, float beta2,
                   float weight_decay, aadff_stream_t stream);
int aadff_fit_adamw(float* param, float* grad, float* exp_avg, float* exp_avg_sq, void* param_bf16, const int* dst,
                    const int* dst_t, long n, const float* scal4, float beta1, float beta2, float eps, aadff_stream_t stream);

/* ------------------------------------------------------------------ host helper */

/* HOST routine (no GPU work): the next n float32 uniforms of torch's CPU generator, bit-identical
 * to torch.rand(n), produced from / written back to the byte state of torch.get_rng_state()
 * (5056 bytes).  Replaces the host draws torch.rand(spp) of deeplens/optics.py:480-481 and
 * deeplens/surfaces.py:192-193 at ~7x the speed while leaving torch's generator exactly where the
 * reference's call sequence would.  out_host may be pinned memory. */
int aadff_host_mt19937_uniform_f32(unsigned char* torch_state_host, long state_bytes, long n, float* out_host);

/* HOST routine: advance the same byte state past n float32 draws without producing them (the generator's regenerations
 * only) - the state torch.rand(n) would leave behind.  A rank of the sharded configuration that owns some
 * slices of a scene skips the other slices' draws of the reference's per-scene stream (deeplens/optics.py:480-481 in the
 * call order of a stack) instead of producing and dropping them. */
int aadff_host_mt19937_discard(unsigned char* torch_state_host, long state_bytes, long n);

/* HOST routine: the [n_rows][row_len] block of draws that starts at the generator's position, produced in TWO passes - phase 0: the
 * first `head` draws of every row (the rest skipped, a 2504-byte generator snapshot per row kept in `snapshots`), the state left
 * behind the whole block as torch.rand(n_rows * row_len) would; phase 1: the remaining row_len - head draws of every row from the
 * snapshots.  Same block as one pass, bit for bit.  For a focal stack the heads are the focus draws (torch.rand(2048) twice per
 * slice, deeplens/surfaces.py:192-193 via optics.py:1166): the refocus launch can start after phase 0 while phase 1 fills the PSF
 * rows (deeplens/optics.py:480-481) behind it. */
int aadff_host_mt19937_rows(unsigned char* torch_state_host, long state_bytes, int n_rows, long row_len, long head, float* out_host,
                            unsigned char* snapshots_host, int phase);

/* HOST routine (strict / edge parity): out[k] = np.mean of the values of row k whose weight is > 0 and which are > 0 (and not NaN) -
 * refocus's `focus_d[ra > 0]`, `focus_d[~isnan & (focus_d > 0)]`, `np.mean` (deeplens/optics.py:1175-1178) for all slices of a stack in
 * numpy's own arithmetic: pairwise float32 summation in numpy's blocking, the division in float64, rounded to float32; NaN for a row
 * without a countable value.  values / weights [rows][n], scratch [n], out [rows]; all host memory. */
int aadff_host_masked_mean_f32(const float* values, const float* weights, long rows, long n, float* scratch, float* out);

/* HOST DRIVER of a strict / edge focal stack (ABI v8, csrc/stack_host.cpp): the per-stack host work between two GPU waits as one call
 * each.  A strict / edge stack is host-bound (0.6 ms of GPU work, 1.2 ms of Python between its waits); these calls do exactly what
 * aadff/strict_stack.py does there - same parameter blocks, same launches (the entry points above), same count check, same host
 * arithmetic - and return a status instead of deciding anything new: 0 = done; 1 = some batch was confirmed by none of its
 * candidate count rows; 2 = a NaN residual in a run the reference makes (the caller repeats the level the slow way, which corrects the
 * table / raises the reference's error).  Replaces the host side of Lensgroup.refocus + calc_fov (deeplens/optics.py:1155-1217) for S
 * slices and of Lensgroup.psf_map (:888-1026) of an edge-parity lens.
 * aadff_levels_t: blocks in the layout of aadff/strict_stack.py (_Stage): level 1 parameters [S*3 axis points | jobs_max job -> batch |
 * J*MAX_SURF predicted rows], results [J*2048 crossing z | J*2048 ra | J*2*MAX_SURF any / nan bits]; level 2 parameters [S*3 sensor
 * corners | M*3 pupil points | job -> batch | rows], results [J*M tan | J*M ra | bits].  The caller has written job -> batch, the rows
 * and the M pupil points; pinned host blocks (h_*) and their device twins (d_*). */
typedef struct aadff_levels {
    int S, n_surf, n_tables, jobs_max, fov_rays, J1, J2, pad;
    const aadff_surface_t* tables_dev;
    const int* bt_green;                 /* [>= jobs_max] table index of the focus wavelength */
    const int* zeros;                    /* [>= jobs_max] */
    int *h_par1, *d_par1, *h_res1, *d_res1;
    int *h_par2, *d_par2, *h_res2, *d_res2;
    float *h_pupil, *d_pupil;            /* [S][2048][3] aperture points of the focus rays */
    unsigned char curved[AADFF_MAX_SURF];
} aadff_levels_t;
/* level 1: aperture points of the first surface from the stack's uniforms (as aadff_host_pupil_points: theta row of slice k at
 * u_host + off_focus[k], radius row 2048 floats behind), upload, launch, download, event (a hipEvent_t, or NULL) */
int aadff_levels_focus_submit(const aadff_levels_t* p, const float* u_host, const long* off_focus, float pi_f, float R2, float z_first,
                              const float* focus, const void* cos_fn, const void* sin_fn, const void* sqrt_fn, int width,
                              aadff_stream_t stream, void* event_or_null);
/* after the event: chosen[S] = the confirmed job of every slice, d_sensor[S] = np.mean of its countable crossing distances
 * (aadff_host_masked_mean_f32; NaN for a slice without one: the reference's "sensor position is negative."); scratch [2048] */
int aadff_levels_focus_finish(const aadff_levels_t* p, int* chosen, float* d_sensor, float* scratch);
/* level 2: the sensor corners (r_last, 0, d_sensor[k]) into the block, upload, launch (forward = 0: the usual backward trace), download, event */
int aadff_levels_fov_submit(const aadff_levels_t* p, const float* d_sensor, float r_last, int forward, aadff_stream_t stream, void* event_or_null);
/* after the event: chosen[S], tan_fov [S][M] and ra [S][M] of the confirmed jobs (the caller takes torch's own sum and atan of them) */
int aadff_levels_fov_finish(const aadff_levels_t* p, int* chosen, float* tan_fov, float* ra);

/* the edge-exact psf_map level of a stack (see aadff_psf_points_edge): everything the three launches need, owned by the caller */
typedef struct aadff_edge_stack {
    int S, L, N, spp, ks, n_surf, n_tables, t_green, cap, pad;
    long per, per_l, o_main, n_pm;       /* floats per slice / per wavelength of the uniform block, offset of the main rows, floats of main pupil points */
    float delta, pixel_size;
    aadff_lens_const_t lc;
    const aadff_surface_t* tables_dev;
    float *h_u, *d_u;                    /* [S*per] the stack's uniforms */
    float *h_focus, *d_focus;            /* [2 S]: focus distances | float(tan(hfov)) of the exact states */
    const float* d_pts;                  /* [S][N][3] normalised field points */
    void* states_prov;                   /* aadff_lens_state_t[S] (device): written by the provisional refocus */
    float *raw, *slope;
    unsigned *count, *list;              /* [S*L + 1] (last word: flags), [S*L][cap] */
    int* h_back;                         /* [S*L + 1] pinned: counts and flags come back here */
    int *h_par3, *d_par3;                /* [S*L z_sensor | S*N*3 object points | S*L*2*MAX_SURF count rows (written by the caller)] */
    const int *pset, *bt_main;           /* [S*L] */
    float *h_pupil_main, *d_pupil_main;  /* [S*L][spp][3] */
} aadff_edge_stack_t;
/* provisional pass: uniforms and focus distances up, fast refocus -> states_prov, aadff_psf_points_edge on them (centre [S*L][N][2]) */
int aadff_edge_provisional(const aadff_edge_stack_t* e, const float* focus, float* centre, aadff_stream_t stream);
/* after levels 1 and 2: object points of the exact states (psf_diff's float32 arithmetic, deeplens/optics.py:945-950) from pts_norm
 * [N][3], hfov [S] (float64, as the reference's Python floats) and d_sensor [S]; uploads (event_uploaded: the pinned blocks may be
 * reused), re-trace with the centres moved into the exact world, normalise into maps [S][L][g ks][g ks], counts / flags to h_back,
 * event_done */
int aadff_edge_finish(const aadff_edge_stack_t* e, const float* pts_norm, const double* hfov, const float* d_sensor, float r_last,
                      float sensor_w, float sensor_h, const float* centre, float* maps, aadff_stream_t stream, void* event_uploaded,
                      void* event_done);

/* Workgroup size (256 or 1024, default 1024) of an aadff_strict_psf_points launch with fewer than 1024 workgroups, i.e. a re-launch
 * of the few batches whose speculated Newton counts (deeplens/surfaces.py:547) were off: 1024 threads shorten it on an idle GPU,
 * 256 get scheduled beside another stack's full launch (aadff.strict_stack.StrictPipeline).  Process-wide. */
int aadff_strict_replay_threads(int threads);

/* HOST routine (strict-parity mode): rows of pupil / aperture points from host uniforms in the reference's float32 operations -
 * theta = (u * 2) * pi, r = sqrt(u' * R^2), (r cos theta, r sin theta, z): deeplens/optics.py:480-486 (sample_point_source's pupil
 * sampling) and deeplens/surfaces.py:188-199 (the aperture points of refocus).  cos_fn / sin_fn / sqrt_fn: addresses of the vector routines
 * torch's CPU kernels use, resolved by the caller in the libtorch_cpu.so of its process - kind 1: MKL's vmsCos / vmsSin / vmsSqrt
 * (torch built with MKL: ATen/cpu/vml.h), kind 16: Sleef_cosf16_u10 / Sleef_sinf16_u10, kind 8: Sleef_cosf8_u10 / Sleef_sinf8_u10
 * (sqrt_fn unused: IEEE root) - same routines, same bits, without the ~70 small tensor operations per stack.  Row i: n theta uniforms at u + theta_off[i], n radius uniforms at u + r_off[i] -> out[i][n][3]. */
int aadff_host_pupil_points(const float* u_host, long n_rows, const long* theta_off, const long* r_off, long n, float pi_f, float R2,
                            float z, float* out_host, const void* cos_fn, const void* sin_fn, const void* sqrt_fn, int kind);

#ifdef __cplusplus
}
#endif
#endif /* AADFF_H_ */
