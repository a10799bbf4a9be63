// The one sorting network of the tree: fluid_verify.hip (the CRPS's order statistics) and fluid_quantile.hip (the quantile
// fields) sort a cell's members with it.  Device code only.
#pragma once
#include <hip/hip_runtime.h>

namespace fluid {

// A bitonic sorting network over MP registers, ascending: every index is a compile-time constant once the three loops are
// unrolled, so the values never leave the registers and an exchange is one v_min_f32 and one v_max_f32.  log2(MP) * (log2(MP)
// + 1) / 2 stages of MP / 2 exchanges each: 1, 6, 24, 80, 240, 672 exchanges at MP = 2 .. 64.  The inputs hold no NaN and no
// -0 where the result is used (rule 3, rule 5).
template <int MP>
__device__ __forceinline__ void verify_sort(float (&v)[MP])
{
    constexpr int LOG = MP == 2 ? 1 : MP == 4 ? 2 : MP == 8 ? 3 : MP == 16 ? 4 : MP == 32 ? 5 : 6;
    static_assert((1 << LOG) == MP, "MP is one of 2, 4, 8, 16, 32, 64");
#pragma unroll
    for (int lk = 1; lk <= LOG; ++lk) {
#pragma unroll
        for (int lj = lk - 1; lj >= 0; --lj) {
#pragma unroll
            for (int i = 0; i < MP; ++i) {
                const int k = 1 << lk, j = 1 << lj, l = i ^ j;
                if (l > i) {
                    const float lo = fminf(v[i], v[l]), hi = fmaxf(v[i], v[l]);
                    const bool up = (i & k) == 0;
                    v[i] = up ? lo : hi;
                    v[l] = up ? hi : lo;
                }
            }
        }
    }
}

}  // namespace fluid
