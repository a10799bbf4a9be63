// Ensemble products (include/fluid_amd.h "ensemble products"): what fluid_solver.hip needs of fluid_quantile.hip.
#pragma once
#include <cmath>

#include "fluid_kernels.h"

namespace fluid {

constexpr int kQuantileMaxLevels = 16;

// The position of a level among `members` sorted values, numpy's default ("linear", Hyndman-Fan type 7): h = level *
// (members - 1) in double -- exact: a float's 24 bits times at most 7 --, lo = floor(h), frac = h - lo, also exact; at the top,
// lo = members - 1 and frac = 0.  members >= 1, level finite and in [0, 1].  The ONE body: fluid_quantile_position returns it
// and fluid_member_quantiles fills the kernel's table with it.
inline void quantile_position(int members, float level, int* lo, double* frac)
{
    const double h = (double)level * (double)(members - 1);
    const double f = std::floor(h);
    *lo = (int)f;
    *frac = h - f;
    if (*lo >= members - 1) {
        *lo = members - 1;
        *frac = 0.0;
    }
}

// The kernel-argument tables: wave-uniform, read with scalar loads.
struct QuantileLevels {
    double frac[kQuantileMaxLevels];
    int lo[kQuantileMaxLevels];
    int count;
};
struct ExceedLevels {
    float threshold[kQuantileMaxLevels];
    int count;
};

// One field, all mb.count members, every cell of the (n + 2)^2 array, lv.count levels: array l of `out` starts l * stride
// floats behind it.  `inv`: as for the pack.  ONE launch each, one lane per cell, no cap on the grid.  Pad columns are not
// read.  Quantiles: mb.count in [1, kTransformMaxMembers].  Exceedance: any mb.count >= 1.
void launch_member_quantiles(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, const QuantileLevels& lv, float* out,
                             size_t stride);
void launch_member_exceedance(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, const ExceedLevels& lv, bool below,
                              float* out, size_t stride);

}  // namespace fluid
