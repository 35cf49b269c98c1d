// The launch plan of the patch convolution: which conv_psf_map_* instantiation (conv.hip) an entry launches for a shape under the
// current environment, with what grid and arguments.  conv_plan (conv_plan.cpp) decides it once per call, on the host, without a HIP
// call; conv_launch (conv.hip) switches on it.  Plain C++: no HIP header.
#pragma once
#include <cstddef>
#include "patch_bounds.h"

#ifndef AADFF_MFMA_SPW
#define AADFF_MFMA_SPW 1          // slices per wave from one staged tile (2 measured slower: 118 vs 74 us)
#endif

namespace aadff {

void set_error(const char* fmt, ...);                                       // runtime.cpp (as in common.h)

// output tiles of the kernel families; conv.hip asserts them against the kernels' own constants
constexpr int kConvTile = 32;                                               // packed-FMA, generic, Toeplitz forms: 32 x 32
constexpr int kConvBandCols = 96;                                           // slice-batched and block-GEMM forms: bands of RB rows x 96 columns
constexpr int kConvSbRows = 24, kConvBlkRows = 24, kConvBlkWaves = 3;

// the entries of include/aadff.h that render through the plan
enum class ConvEntry { map, psf, stack, strided, layered };
enum class ConvFamily { valu, generic, mfma, toeplitz_wide, sbatch, blk, blkw };

struct ConvPlan {
    ConvFamily family;
    // template arguments as the symbol spells them (bool as 0 / 1): valu KS, NW | mfma KS, NW, SPW | toeplitz_wide NK, KSPLIT, MAXR, MAXT |
    // sbatch RB, NC, PAIR, TIMED, LAYERED (TIMED 0 here: conv_launch takes the TIMED twin when it is given events) | blk KS, TIMED | blkw KS, RB
    int targ[5];
    unsigned gx, gy, gz, block;                                             // launch grid, threads per workgroup
    size_t lds;                                                             // dynamic LDS bytes
    // scalar launch arguments: slices the kernel renders (S; S * L maps for the layered entry), layers, tiles or bands per patch,
    // chunks (nchunk or npass), and what only one family takes (spw, P: toeplitz_wide; stagger, pair_mod: sbatch)
    int C, S, L, H, W, grid, ks, ntx, nty, nchunk, spw, P, stagger, pair_mod;
    PatchBounds pb;
    bool attach;        // the launch takes aadff_time_next_launch's events on its own dispatch; false: the caller records them around it
};

// Fills pl for entry(B, C, S, L, H, W, grid, ks) with output strides sbc / ss (elements) under the current environment, or refuses:
// return code and error text of the entry itself.  ptrs_ok: the caller's pointers are all non-NULL (checked where the entry checks it).
int conv_plan(ConvPlan& pl, ConvEntry entry, bool ptrs_ok, int B, int C, int S, int L, int H, int W, int grid, int ks, long sbc, long ss);
// the instantiation's name as the symbol table spells it (nm -C), without namespace and parameter list
void conv_plan_name(const ConvPlan& pl, char* buf, size_t len);

}  // namespace aadff
