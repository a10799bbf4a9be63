// Ensemble products (include/fluid_amd.h "ensemble products"): the quantile fields and the exceedance probabilities of an
// ensemble, their kernels and launch wrappers, in a translation unit of their own.  Declarations: fluid_quantile.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fluid_quantile.h"
#include "fluid_sort.h"

namespace fluid {

// (fluid_kernels.hip has the reason: the empty asm keeps a widening conversion from folding into a mixed-precision
// instruction that rounds once where the contract rounds twice)
__device__ __forceinline__ float quantile_keep_f32(float v) { asm("" : "+v"(v)); return v; }

// the float the pack shows
__device__ __forceinline__ float quantile_value(const float* p, float) { return *p; }
__device__ __forceinline__ float quantile_value(const half_t* p, float inv) { return quantile_keep_f32((float)*p) * inv; }

// Both kernels: ONE LANE PER CELL, NO CAP ON THE GRID -- cdiv(W * W, 256) blocks of 256 lanes, lane t = blockIdx.x * 256 +
// threadIdx.x takes cell t = row * W + col of the W x W array and no other, lanes past the last cell leave at once.  No lane
// strides over several cells, so there is no wrap of the grid.  W * W <= 65535^2 < 2^32 - 256: t fits an unsigned in every
// block.  Consecutive lanes take consecutive columns, so a member's load is a coalesced row segment.  A cell's place in a
// dense array is t itself.

// ---------------------------------------------------------------------------
// k_member_quantiles: MP = the member count padded to a power of two; the values live in MP registers, pads are +inf and sort
// last.  Members 0 .. HAVE - 1 always exist (HAVE = MP / 2 + 1 <= members for MP >= 4; MP = 2 serves members = 1 and 2:
// HAVE = 1); the others are loaded under a wave-uniform branch, and a member that does not exist is not read.  The
// finiteness of the cell is taken from the values as loaded -- the network's v_min / v_max drop NaNs --, then every value
// gets + 0.0f (rule 1) and the network sorts in place.  Registers cannot be indexed by a run-time position: per level, a
// run-time loop reads (lo, frac) from the kernel-argument table (scalar loads, wave-uniform) and an unrolled
// compare-and-select chain over the MP registers picks s_lo and s_{lo + 1}: 2 MP selects per level.  A pad is never USED:
// it can only be picked as s_{lo + 1} when frac == 0, where the result is s_lo alone.  No LDS, no atomics, no matrix
// instructions.
// ---------------------------------------------------------------------------
template <typename S, int MP>
__global__ __launch_bounds__(256) void k_member_quantiles(const S* __restrict__ x, int pitch, int w, size_t ms, int members, float inv,
                                                          QuantileLevels lv, float* __restrict__ out, size_t stride)
{
#pragma clang fp contract(off)
    constexpr int HAVE = MP == 2 ? 1 : MP / 2 + 1;
    const unsigned cells = (unsigned)w * (unsigned)w, t = blockIdx.x * 256u + threadIdx.x;
    if (t >= cells) return;
    const unsigned row = t / (unsigned)w, col = t - row * (unsigned)w;
    size_t off = (size_t)row * (size_t)pitch + (size_t)(XOFF + (int)col);
    float v[MP];
#pragma unroll
    for (int k = 0; k < MP; ++k) {
        if (k < HAVE || k < members) v[k] = quantile_value(x + off, inv);
        else v[k] = INFINITY;
        off += ms;
    }
    bool finite = true;
#pragma unroll
    for (int k = 0; k < MP; ++k)
        if (k < HAVE || k < members) finite = finite && fabsf(v[k]) < INFINITY;
#pragma unroll
    for (int k = 0; k < MP; ++k) v[k] = v[k] + 0.0f;
    verify_sort<MP>(v);
    float* o = out + t;
    for (int l = 0; l < lv.count; ++l) {
        const int lo = lv.lo[l];
        const double frac = lv.frac[l];
        float a = v[0], b = v[1];
#pragma unroll
        for (int i = 1; i < MP; ++i) a = lo == i ? v[i] : a;
#pragma unroll
        for (int i = 2; i < MP; ++i) b = lo + 1 == i ? v[i] : b;
        float q = a;
        if (frac != 0.0) {
            const double d = (double)b - (double)a;
            const double p = __dmul_rn(frac, d);
            q = (float)__dadd_rn((double)a, p);
        }
        *o = finite ? q : __builtin_nanf("");
        o += stride;
    }
}

// ---------------------------------------------------------------------------
// k_member_exceedance: the members in a run-time loop, any count, kExceedUnroll at a time -- that many loads in flight
// together --, each read once for all thresholds; 64-bit row and member offsets.  Up to kQuantileMaxLevels integer counters
// with compile-time indices: the threshold loop is unrolled and guarded by the wave-uniform count, the thresholds sit in
// scalar registers.  Float comparisons: -0 equals +0, a NaN member counts as neither above nor below.  out =
// (float)((double)count / (double)members).  No LDS, no atomics, no matrix instructions.
// ---------------------------------------------------------------------------
constexpr int kExceedUnroll = 4;

template <bool BELOW, int R>
__device__ __forceinline__ void exceed_tally(const float (&xv)[R], const ExceedLevels& lv, int (&count)[kQuantileMaxLevels])
{
#pragma unroll
    for (int l = 0; l < kQuantileMaxLevels; ++l)
        if (l < lv.count) {
#pragma unroll
            for (int r = 0; r < R; ++r) count[l] += (BELOW ? xv[r] < lv.threshold[l] : xv[r] > lv.threshold[l]) ? 1 : 0;
        }
}

template <typename S, bool BELOW>
__global__ __launch_bounds__(256) void k_member_exceedance(const S* __restrict__ x, int pitch, int w, size_t ms, int members, float inv,
                                                           ExceedLevels lv, float* __restrict__ out, size_t stride)
{
    constexpr int L = kQuantileMaxLevels;
    const unsigned cells = (unsigned)w * (unsigned)w, t = blockIdx.x * 256u + threadIdx.x;
    if (t >= cells) return;
    const unsigned row = t / (unsigned)w, col = t - row * (unsigned)w;
    const S* p = x + ((size_t)row * (size_t)pitch + (size_t)(XOFF + (int)col));
    int count[L];
#pragma unroll
    for (int l = 0; l < L; ++l) count[l] = 0;
    int m = 0;
    for (; m + kExceedUnroll <= members; m += kExceedUnroll) {
        float xv[kExceedUnroll];
#pragma unroll
        for (int r = 0; r < kExceedUnroll; ++r) {
            xv[r] = quantile_value(p, inv);
            p += ms;
        }
        exceed_tally<BELOW>(xv, lv, count);
    }
    for (; m < members; ++m) {
        const float xv[1] = {quantile_value(p, inv)};
        p += ms;
        exceed_tally<BELOW>(xv, lv, count);
    }
    const double dm = (double)members;
    float* o = out + t;
#pragma unroll
    for (int l = 0; l < L; ++l)
        if (l < lv.count) {
            *o = (float)((double)count[l] / dm);
            o += stride;
        }
}

static unsigned product_blocks(int n) { return (unsigned)(((size_t)(n + 2) * (size_t)(n + 2) + 255) / 256); }

void launch_member_quantiles(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, const QuantileLevels& lv, float* out,
                             size_t stride)
{
    const int M = mb.count;
#define FLUID_QUANTILE_LAUNCH(S, MP)                                                                                                     \
    hipLaunchKernelGGL((k_member_quantiles<S, MP>), dim3(product_blocks(n)), dim3(256), 0, s, (const S*)x, pitch, n + 2, mb.stride, M, inv, lv, \
                       out, stride)
#define FLUID_QUANTILE_BY_MP(S)                         \
    do {                                                \
        if (M <= 2) FLUID_QUANTILE_LAUNCH(S, 2);        \
        else if (M <= 4) FLUID_QUANTILE_LAUNCH(S, 4);   \
        else if (M <= 8) FLUID_QUANTILE_LAUNCH(S, 8);   \
        else if (M <= 16) FLUID_QUANTILE_LAUNCH(S, 16); \
        else if (M <= 32) FLUID_QUANTILE_LAUNCH(S, 32); \
        else FLUID_QUANTILE_LAUNCH(S, 64);              \
    } while (0)
    if (st == STORAGE_F16) FLUID_QUANTILE_BY_MP(half_t);
    else FLUID_QUANTILE_BY_MP(float);
#undef FLUID_QUANTILE_BY_MP
#undef FLUID_QUANTILE_LAUNCH
}

void launch_member_exceedance(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, const ExceedLevels& lv, bool below,
                              float* out, size_t stride)
{
#define FLUID_EXCEED_LAUNCH(S, B)                                                                                                             \
    hipLaunchKernelGGL((k_member_exceedance<S, B>), dim3(product_blocks(n)), dim3(256), 0, s, (const S*)x, pitch, n + 2, mb.stride, mb.count, \
                       inv, lv, out, stride)
    if (st == STORAGE_F16) {
        if (below) FLUID_EXCEED_LAUNCH(half_t, true);
        else FLUID_EXCEED_LAUNCH(half_t, false);
    } else {
        if (below) FLUID_EXCEED_LAUNCH(float, true);
        else FLUID_EXCEED_LAUNCH(float, false);
    }
#undef FLUID_EXCEED_LAUNCH
}

}  // namespace fluid
