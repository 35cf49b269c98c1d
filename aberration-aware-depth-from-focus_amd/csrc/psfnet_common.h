// What the fused PSF-surrogate renderer (psfnet.hip) and its backward (psfnet_bwd.hip) share: the workgroup shape, the LDS layout
// of the activations and the exact fp16 hi/lo operand split.  The backward recomputes the forward and has to reproduce its bits.
#pragma once
#include "common.h"

namespace aadff {
namespace pn {

constexpr int NWV = 8, NTH = 64 * NWV;
constexpr int AP = 256;                 // activation row pitch in halves; 16-byte slots XOR-swizzled by the pixel (swz)
constexpr int MAXL = AADFF_PSFNET_MAX_LAYERS;

typedef _Float16 half8v __attribute__((ext_vector_type(8)));
typedef _Float16 half4v __attribute__((ext_vector_type(4)));
typedef float float4v __attribute__((ext_vector_type(4)));
typedef unsigned uint4v __attribute__((ext_vector_type(4)));

// In-kernel layer-0 input (PSFNet.render, deeplens/psfnet.py:424-437): row (n, slice, y, x) of the network input is
// (xs[x], ys[y], clamp((depth[n][y][x] - d_min) * inv_range, 0, 1), foc_z[n][slice]) -- the [N,S,H,W,4] coordinate tensor
// of the reference (168 MB for a 1024^2 x 10 stack) is never written.  depth == nullptr: rows come from `inp`.
struct Coord {
    const float* depth;     // [N][H][W] mm (< 0)
    const float* xs;        // [W]  torch.linspace(-1, 1, W)
    const float* ys;        // [H]  torch.linspace(1, -1, H)
    const float* foc_z;     // [N][S]  depth2z(foc_dist)
    float d_min, inv_range; // depth2z: (depth - d_min) * (1 / (d_max - d_min)), the form ATen evaluates tensor / scalar in
};

// LDS offset (halves) of feature `f` of pixel `px`: the 16-byte slot index is XORed with px & 15.  The MFMA B-fragment
// read (lane = pixel px & 15, k-group kg: slot 4 s + kg) then touches every bank once per ds_read_b128 lane group
// (unswizzled with a padded pitch it is 2-way: SQ_LDS_BANK_CONFLICT was 49 % of the LDS cycles), and the write-back
// (lane = pixel, 4 features = half a slot) is 2-way instead of 4-way.
__device__ __forceinline__ int swz(int px, int f) { return px * AP + ((((f >> 3) ^ px) & 15) << 3 | (f & ~127) | (f & 7)); }

// x = hi + lo with hi = fp16(x) (RNE) and lo = fp16(x - hi): v_cvt_pk_f16_f32 for two hi halves, then one
// v_fma_mix{lo,hi}_f16 per lo half (fp16 hi * -1 + fp32 x, rounded once to fp16) -- the compiler emits convert-back,
// subtract and convert instead (20 instead of 10 VALU per four values of the layer write-back).
__device__ __forceinline__ void split4(float4v v, half4v& h, half4v& l) {
    typedef _Float16 half2v __attribute__((ext_vector_type(2)));
    const half2v h01 = {(_Float16)v[0], (_Float16)v[1]}, h23 = {(_Float16)v[2], (_Float16)v[3]};
    unsigned l01, l23;
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\tv_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(l01) : "v"(__builtin_bit_cast(unsigned, h01)), "v"(v[0]), "v"(v[1]));
    asm("v_fma_mixlo_f16 %0, %1, -1.0, %2 op_sel_hi:[1,0,0]\n\tv_fma_mixhi_f16 %0, %1, -1.0, %3 op_sel:[1,0,0] op_sel_hi:[1,0,0]"
        : "=&v"(l23) : "v"(__builtin_bit_cast(unsigned, h23)), "v"(v[2]), "v"(v[3]));
    const half2v q01 = __builtin_bit_cast(half2v, l01), q23 = __builtin_bit_cast(half2v, l23);
    h = (half4v){h01[0], h01[1], h23[0], h23[1]};
    l = (half4v){q01[0], q01[1], q23[0], q23[1]};
}

}  // namespace pn
}  // namespace aadff
