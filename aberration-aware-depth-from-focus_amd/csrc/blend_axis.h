// The cell decomposition and the blend-fraction arithmetic of the blended PSF-map render, shared by its forward (conv_blend.hip) and
// its backward (conv_blend_bwd.hip): both units cut the axes the same way and compute fx, fy with the same three roundings.
// Semantics: include/aadff.h (aadff_render_psf_map_blend_stack); design: DESIGN.md 4.18, 4.19.
#pragma once
#include <cmath>
#include <cstdlib>
#include "common.h"

namespace aadff {

// One axis of the cell decomposition, by value in the kernel arguments (scalar loads), as PatchBounds is.
//   cell c (0 <= c < ncell, ncell = max(g - 1, 1)) covers the pixels b[c] <= p < b[c + 1] and blends nodes c and min(c + 1, g - 1);
//   its tiles are ts[c] <= t < ts[c + 1] of the axis' tile enumeration: an empty cell has no tile, so nothing is launched for it.
struct BlendAxis {
    int b[AADFF_MAX_GRID];
    int ts[AADFF_MAX_GRID];
    float node[AADFF_MAX_GRID];
};
struct BlendCells { BlendAxis y, x; };

constexpr int BT = 32;                        // tile edge: BT x BT pixels of one cell

// the cell of tile t: at most 62 scalar steps in front of ks^2 * 64 FMAs per lane
__device__ __forceinline__ int cell_of_tile(const BlendAxis& a, int ncell, int t) {
    int c = 0;
    while (c + 1 < ncell && t >= a.ts[c + 1]) ++c;
    return c;
}
// the cell of pixel p (0 <= p < n): the last c with b[c] <= p; the empty cells in front of it are stepped over
__device__ __forceinline__ int cell_of_pixel(const BlendAxis& a, int ncell, int p) {
    int c = 0;
    while (c + 1 < ncell && p >= a.b[c + 1]) ++c;
    return c;
}

// fx of pixel p in the cell between nodes n0 and n1: three roundings (difference, difference, quotient), then the clamp
__device__ __forceinline__ float blend_frac(int p, float n0, float n1, bool single) {
    const float f = __fdiv_rn(__fsub_rn((float)p, n0), __fsub_rn(n1, n0));
    return single ? 0.f : fminf(fmaxf(f, 0.f), 1.f);
}

// cells of one axis: b[c] = the first pixel at or right of node c (c = 1 .. g-2; integers p with node[c] <= p), 0 and n at the ends
static inline int fill_axis(BlendAxis& a, const float* node, int g, int n) {
    const int ncell = g > 1 ? g - 1 : 1;
    for (int i = 0; i < g; ++i) a.node[i] = node[i];
    a.b[0] = 0;
    for (int c = 1; c < ncell; ++c) {
        const double e = std::ceil((double)node[c]);
        a.b[c] = e <= 0.0 ? 0 : (e >= (double)n ? n : (int)e);
    }
    a.b[ncell] = n;
    a.ts[0] = 0;
    for (int c = 0; c < ncell; ++c) a.ts[c + 1] = a.ts[c] + (a.b[c + 1] - a.b[c] + BT - 1) / BT;
    return a.ts[ncell];
}

static inline int check_nodes(const float* node, int g, const char* axis) {
    for (int i = 0; i < g; ++i) AADFF_CHECK_ARG(std::isfinite(node[i]), "render_psf_map_blend: %s[%d] is not finite", axis, i);
    for (int i = 1; i < g; ++i)
        AADFF_CHECK_ARG(node[i] > node[i - 1], "render_psf_map_blend: %s is not strictly increasing at index %d (%g after %g)", axis, i,
                        (double)node[i], (double)node[i - 1]);
    return 0;
}

// the argument domain of the forward entry, checked the same way by the backward entries
static inline int blend_check_shape(int B, int C, int S, int H, int W, int grid, int ks) {
    AADFF_CHECK_ARG(B > 0 && C > 0 && S > 0 && H > 0 && W > 0, "render_psf_map_blend: empty tensor (B=%d C=%d S=%d H=%d W=%d)", B, C, S, H, W);
    AADFF_CHECK_ARG(grid >= 1 && grid <= AADFF_MAX_GRID, "render_psf_map_blend: grid %d outside [1,%d]", grid, AADFF_MAX_GRID);
    AADFF_CHECK_ARG(ks % 2 == 1, "PSF kernel size should be odd");
    AADFF_CHECK_ARG(ks >= 1 && ks <= AADFF_MAX_KS, "render_psf_map_blend: ks %d outside [1,%d]", ks, AADFF_MAX_KS);
    AADFF_CHECK_ARG(ks / 2 < H && ks / 2 < W, "render_psf_map_blend: reflect padding %d needs H,W > pad", ks / 2);
    AADFF_CHECK_ARG((size_t)B * C <= 65535, "render_psf_map_blend: B*C too large");
    AADFF_CHECK_ARG((size_t)H + (size_t)BT * grid <= (size_t)65535 * BT && (size_t)W + (size_t)BT * grid <= ((size_t)1 << 30),
                    "render_psf_map_blend: H=%d W=%d too large for the launch grid", H, W);
    return 0;
}

}  // namespace aadff
