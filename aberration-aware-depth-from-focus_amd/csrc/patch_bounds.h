// Patch bounds of the patch convolution and their host-side fill: plain C++, no HIP header, so that the host unit that plans the
// launches (conv_plan.cpp) builds without one.  Included by common.h for every other unit.
#pragma once
#include "aadff.h"

#ifdef __HIPCC__
#define AADFF_HOST_DEVICE __host__ __device__
#else
#define AADFF_HOST_DEVICE
#endif

namespace aadff {

// ------------------------------------------------------------------------------------
// Patch bounds: Python `int(i / grid * n)` in float64 (deeplens/render_psf.py:65-66).
// Passed by value in the kernarg segment -> read with scalar loads.
// ------------------------------------------------------------------------------------
struct PatchBounds {
    int hb[AADFF_MAX_GRID + 1];
    int wb[AADFF_MAX_GRID + 1];
    // ceil(2^32 / d) for the uniform block-index decompositions: n / d == __umulhi(n, magic) for
    // n < 65536 (integer division has no scalar form on gfx950 and costs ~15 VALU slots each)
    unsigned m_ntx, m_nty, m_nchunk, m_c;
    // XCD-aware block order (xcd_remap): 1-D launches only.  gx, gy = logical grid extents; N = 8 xcd_q + xcd_r blocks (xcd_q = 0: plain order)
    unsigned gx, gy, xcd_q, xcd_r, m_gx, m_gy;      // m_gx / m_gy != 0: magic multipliers, valid while the launch has < 65536 blocks
};

AADFF_HOST_DEVICE inline unsigned magic_of(unsigned d) { return (unsigned)((0x100000000ull + d - 1) / d); }

inline void fill_bounds(int* b, int grid, int n) {
    for (int i = 0; i <= grid; ++i) b[i] = (int)((double)i / (double)grid * (double)n);
}

}  // namespace aadff
