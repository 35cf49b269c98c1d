// Stand-alone walk of the patch convolution's launch plan (csrc/conv_plan.cpp) over the corners of its domain, compiled with
// -fsanitize=address,undefined and run by tests/test_conv_paths_host.py.  Supplies its own set_error, so nothing of HIP is linked.
// Every plan that is not refused is checked for a launch the hardware accepts; a sanitizer report aborts the program.
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <initializer_list>
#include "conv_plan.h"

namespace aadff {
static char g_err[512];
void set_error(const char* fmt, ...) {
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(g_err, sizeof(g_err), fmt, ap);
    va_end(ap);
}
}  // namespace aadff

using namespace aadff;

static long n_plans = 0, n_refused = 0;

static void fail(const char* what, const char* name, int B, int C, int S, int L, int H, int W, int grid, int ks) {
    fprintf(stderr, "conv_plan_walk: %s (%s; B=%d C=%d S=%d L=%d H=%d W=%d grid=%d ks=%d)\n", what, name, B, C, S, L, H, W, grid, ks);
    exit(1);
}

static void walk(ConvEntry entry, int B, int C, int S, int L, int H, int W, int grid, int ks) {
    ConvPlan pl;
    const long ss = (long)H * W, sbc = (long)S * ss;
    g_err[0] = 0;
    const int rc = conv_plan(pl, entry, true, B, C, S, L, H, W, grid, ks, sbc, ss);
    ++n_plans;
    if (rc != 0) {
        ++n_refused;
        if ((rc != AADFF_EINVAL && rc != AADFF_EUNSUPPORTED) || !g_err[0]) fail("refusal without code or message", "-", B, C, S, L, H, W, grid, ks);
        return;
    }
    char name[96];
    conv_plan_name(pl, name, sizeof(name));
    if (std::strncmp(name, "conv_psf_map_", 13) != 0) fail("no name", name, B, C, S, L, H, W, grid, ks);
    if (pl.gx < 1 || pl.gy < 1 || pl.gz < 1 || pl.gx > 0x7fffffffu || pl.gz > 65535u) fail("launch grid out of range", name, B, C, S, L, H, W, grid, ks);
    if (pl.block < 64 || pl.block > 320 || pl.block % 64) fail("block size", name, B, C, S, L, H, W, grid, ks);
    if (pl.lds > 64 * 1024 - 64) fail("LDS bytes", name, B, C, S, L, H, W, grid, ks);
    if (pl.pb.hb[0] != 0 || pl.pb.hb[grid] != H || pl.pb.wb[0] != 0 || pl.pb.wb[grid] != W) fail("patch bounds", name, B, C, S, L, H, W, grid, ks);
    if (pl.attach != (pl.family == ConvFamily::sbatch && entry != ConvEntry::layered)) fail("attach flag", name, B, C, S, L, H, W, grid, ks);
}

int main() {
    static const char* const envs[][2] = {{nullptr, nullptr}, {"AADFF_CONV_PATH", "valu"}, {"AADFF_CONV_PATH", "toeplitz"}, {"AADFF_CONV_BLKW", "0"},
                                          {"AADFF_CONV_BLKW", "1"}, {"AADFF_CONV_BLKW_RB", "48"}, {"AADFF_CONV_PAIR", "1"}, {"AADFF_CONV_NW", "5"},
                                          {"AADFF_CONV_NW", "-2147483648"}, {"AADFF_CONV_PAIR", "2147483647"}};
    // H x W: tiny, H = W = grid (below), odd, and planes at and just past 2^27 and 2^30 pixels
    static const int shapes[][2] = {{26, 27}, {77, 70}, {1024, 1024}, {8192, 16384}, {8192, 16385}, {16385, 8192}, {32768, 32768}, {32768, 32769}, {32769, 32768},
                                    {1, 1 << 30}, {(1 << 30) + 1, 1}, {46341, 46341}};
    static const int bcs[][2] = {{1, 1}, {1, 3}, {5, 13}, {65535, 1}, {1, 65535}, {255, 257}, {256, 256}, {65536, 1}, {0x7fffffff, 0x7fffffff}};
    static const int grids[] = {1, 2, 7, 11, 32, AADFF_MAX_GRID, AADFF_MAX_GRID + 1, 0};
    static const int kss[] = {1, 3, 5, 9, 11, 13, 17, 21, 23, 31, 33, 49, AADFF_MAX_KS, AADFF_MAX_KS + 2, 4, -1};
    static const int slices[] = {1, 2, 3, 4, 5, 8, 9, 12, 13, 16, 17, 63, 64};
    for (const auto& e : envs) {
        for (const char* k : {"AADFF_CONV_PATH", "AADFF_CONV_BLKW", "AADFF_CONV_BLKW_RB", "AADFF_CONV_NW", "AADFF_CONV_PAIR"}) unsetenv(k);
        if (e[0]) setenv(e[0], e[1], 1);
        for (const int ks : kss)
            for (const int grid : grids)
                for (const auto& bc : bcs) {
                    for (const auto& hw : shapes)
                        for (const int S : slices) {
                            walk(S == 1 ? ConvEntry::map : ConvEntry::stack, bc[0], bc[1], S, 1, hw[0], hw[1], grid, ks);
                            if (S <= 5) walk(ConvEntry::layered, bc[0], bc[1], S, S == 1 ? 254 : (S == 5 ? 255 : 13), hw[0], hw[1], grid, ks);
                        }
                    walk(ConvEntry::psf, bc[0], bc[1], 1, 1, 77, 70, 1, ks);
                    if (grid >= 1) walk(ConvEntry::stack, bc[0], bc[1], 64, 1, grid, grid, grid, ks);           // H = W = grid: one-pixel patches
                }
    }
    // the strided entry: strides below one plane, overlapping, and the two accepted orders
    for (const long sbc : {100L, 5389L, 5390L, 5390L * 10, 5390L * 30})
        for (const long ss : {100L, 5390L, 5390L * 3, 5390L * 10}) {
            ConvPlan pl;
            ++n_plans;
            n_refused += conv_plan(pl, ConvEntry::strided, true, 1, 3, 10, 1, 77, 70, 2, 11, sbc, ss) != 0;
        }
    printf("conv_plan_walk: %ld plans, %ld refused\n", n_plans, n_refused);
    return n_refused > 0 && n_refused < n_plans ? 0 : 1;
}
