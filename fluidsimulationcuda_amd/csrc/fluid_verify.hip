// Verifying ensembles (include/fluid_amd.h "verifying ensembles"): the scoring kernel, its fold and their launch wrapper, in a
// translation unit of their own.  Declarations: fluid_verify.h.
#include <hip/hip_runtime.h>

#include <cmath>

#include "fluid_sort.h"
#include "fluid_verify.h"

namespace fluid {

// (fluid_kernels.hip has the reason: the empty asm keeps a widening conversion from folding into a mixed-precision
// instruction that rounds once where the contract rounds twice)
__device__ __forceinline__ float verify_keep_f32(float v) { asm("" : "+v"(v)); return v; }

// the float the pack shows: rule 1
__device__ __forceinline__ float verify_value(const float* p, float) { return *p; }
__device__ __forceinline__ float verify_value(const half_t* p, float inv) { return verify_keep_f32((float)*p) * inv; }

// The chains below are long and every term of one is independent work: the build's scheduler (max-ilp) would widen all MP terms
// to double ahead of the chain and hold them, 2 registers each.  A scheduling barrier every 8 terms bounds what is live.
__device__ __forceinline__ void verify_fence(int k)
{
    if ((k & 7) == 7) __builtin_amdgcn_sched_barrier(0);
}

__device__ __forceinline__ double verify_wave_sum(double s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
    return s;
}

// verify_sort, the bitonic network over MP registers: fluid_sort.h, shared with the quantile fields.

// ---------------------------------------------------------------------------
// k_verify_members: one lane per cell of the box.  Cell t = (row - row_lo) * cols + (col - col_lo), t < cells; lane L =
// blockIdx.x * 256 + threadIdx.x of the gridDim.x * 256 lanes takes the cells L, L + gridDim.x * 256, .. -- consecutive lanes
// on consecutive columns, so a member's load is a coalesced row segment, and a cell's `members` loads are independent and in
// flight together.  MP = the member count padded to a power of two: the values live in MP registers, pads are +inf and sort
// last.  Members 0 .. MP / 2 always exist (MP / 2 < members <= MP); the others are loaded under a wave-uniform branch.
// The mean and q chains and the rank run on the values as loaded, in member order; then every value gets + 0.0f (rule 3)
// and the network sorts them in place; the two CRPS chains walk the sorted registers.  Per lane four double accumulators
// from -0.0 (a sum starts from its first term, and a lane without a cell adds nothing), the 64-lane butterfly, the four
// waves through LDS in wave order, ONE plain store per block and sum: psums[sum * gridDim.x + block].  The rank counts go
// to per-block LDS words with integer atomics and from there to pbins[rank * gridDim.x + block], ranks 0 .. members.  No
// floating-point atomics, no matrix instructions.  No lane leaves early: every lane reaches the butterfly.
// ---------------------------------------------------------------------------
template <typename S, int MP>
__global__ __launch_bounds__(256) void k_verify_members(const S* __restrict__ x, int pitch, int w, size_t ms, int members, float inv,
                                                        const float* __restrict__ truth, CellBox box, unsigned cells, double dpair,
                                                        float* __restrict__ crps_map, double* __restrict__ psums, unsigned* __restrict__ pbins)
{
#pragma clang fp contract(off)
    __shared__ unsigned bins[kVerifyBins];
    __shared__ double part[4][4];
    if (threadIdx.x < kVerifyBins) bins[threadIdx.x] = 0u;
    __syncthreads();

    const unsigned cols = (unsigned)(box.col_hi - box.col_lo);
    const double dm = (double)members, dm1 = (double)(members - 1), coef0 = (double)(1 - members);
    double acc_e = -0.0, acc_se = -0.0, acc_var = -0.0, acc_crps = -0.0;
    // cells <= 65535^2 fits an unsigned, but the lane's last t + stride need not: the lane counts its cells, it does not
    // compare a t that may have wrapped
    const unsigned stride = gridDim.x * 256u, first = blockIdx.x * 256u + threadIdx.x;
    const unsigned mine = first < cells ? (cells - first - 1u) / stride + 1u : 0u;
    unsigned t = first;
    for (unsigned it = 0; it < mine; ++it, t += stride) {
        const unsigned r = t / cols;
        const int row = box.row_lo + (int)r, col = box.col_lo + (int)(t - r * cols);
        const size_t at = (size_t)row * (size_t)pitch + (size_t)(XOFF + col);
        const size_t dat = (size_t)row * (size_t)w + (size_t)col;
        asm("" : "+s"(members));                   // (the MP comparisons with it are made where they are used, not kept)
        float v[MP];
        const float y = truth[dat];
        size_t off = at;
#pragma unroll
        for (int k = 0; k < MP; ++k) {
            if (k <= MP / 2 || k < members) v[k] = verify_value(x + off, inv);
            else v[k] = INFINITY;
            off += ms;
            asm("" : "+v"(off));                     // one address walking the members: MP bases hoisted out of the cell loop spill
            verify_fence(k);
        }
        // rule 2: the chains of fluid_ensemble_stats; rule 4: the rank
        double s = (double)v[0];
        int rank = v[0] < y ? 1 : 0;
#pragma unroll
        for (int k = 1; k < MP; ++k)
            if (k <= MP / 2 || k < members) {
                s = s + (double)v[k];
                rank += v[k] < y ? 1 : 0;
                verify_fence(k);
            }
        const double mean = s / dm;
        double q;
        {
            const double d = (double)verify_keep_f32(v[0]) - mean;
            q = d * d;
        }
#pragma unroll
        for (int k = 1; k < MP; ++k)
            if (k <= MP / 2 || k < members) {
                const double d = (double)verify_keep_f32(v[k]) - mean;
                q = q + d * d;
                verify_fence(k);
            }
        const double var = q / dm1;
        const double e = mean - (double)y;
        const double se = e * e;
        // 64 finite floats cannot overflow a double: s is finite exactly when every member is (rule 5)
        const bool finite = fabs(s) < (double)INFINITY && fabsf(y) < INFINITY;
        // rule 3
#pragma unroll
        for (int k = 0; k < MP; ++k) v[k] = v[k] + 0.0f;
        const double yc = (double)(y + 0.0f);
        __builtin_amdgcn_sched_barrier(0);
        verify_sort<MP>(v);
        __builtin_amdgcn_sched_barrier(0);
        double a = fabs((double)v[0] - yc);
        double coef = coef0;                       // 2 i - M - 1 at i = 1, then + 2.0 per step: exact.  (Opaque per cell: MP
        asm("" : "+v"(coef));                      // coefficients hoisted out of the cell loop are 2 MP registers held)
        double g = coef * (double)v[0];
#pragma unroll
        for (int i = 1; i < MP; ++i)
            if (i <= MP / 2 || i < members) {
                const double si = (double)v[i];
                a = a + fabs(si - yc);
                coef = coef + 2.0;
                g = g + coef * si;
                verify_fence(i);
            }
        const double t1 = a / dm;
        const double t2 = g / dpair;
        double crps = t1 - t2;
        if (!finite) crps = __builtin_nan("");
        if (crps_map) crps_map[dat] = (float)crps;
        acc_e = acc_e + e;
        acc_se = acc_se + se;
        acc_var = acc_var + var;
        acc_crps = acc_crps + crps;
        atomicAdd(&bins[rank], 1u);
    }
    acc_e = verify_wave_sum(acc_e);
    acc_se = verify_wave_sum(acc_se);
    acc_var = verify_wave_sum(acc_var);
    acc_crps = verify_wave_sum(acc_crps);
    if ((threadIdx.x & 63) == 0) {
        const int wv = threadIdx.x >> 6;
        part[wv][0] = acc_e; part[wv][1] = acc_se; part[wv][2] = acc_var; part[wv][3] = acc_crps;
    }
    __syncthreads();
    if (threadIdx.x < 4)
        psums[(size_t)threadIdx.x * gridDim.x + blockIdx.x] =
            ((part[0][threadIdx.x] + part[1][threadIdx.x]) + part[2][threadIdx.x]) + part[3][threadIdx.x];
    if ((int)threadIdx.x <= members) pbins[(size_t)threadIdx.x * gridDim.x + blockIdx.x] = bins[threadIdx.x];
}

// One wave per entry of the row (grid kVerifyRow).  Entry 0: the cell count.  Entries 1 .. 4: lane l chains the blocks'
// partials l, l + 64, .. of that sum from -0.0 in index order, then the butterfly.  Entries 5 + r: r <= members, the integer
// sum of the blocks' counts; beyond, +0.0.  blocks == 0 (an empty box): zero sums and zero bins.
__global__ __launch_bounds__(64) void k_verify_fold(const double* __restrict__ psums, const unsigned* __restrict__ pbins, int blocks, int members,
                                                    double count, double* __restrict__ row)
{
    const int entry = blockIdx.x;
    if (entry == 0) {
        if (threadIdx.x == 0) row[0] = count;
    } else if (entry < kVerifySums) {
        const double* p = psums + (size_t)(entry - 1) * blocks;
        double s = -0.0;
        for (int k = threadIdx.x; k < blocks; k += 64) s = s + p[k];
        s = verify_wave_sum(s);
        if (threadIdx.x == 0) row[entry] = s;
    } else {
        const int r = entry - kVerifySums;
        unsigned long long c = 0;
        if (r <= members) {
            const unsigned* p = pbins + (size_t)r * blocks;
            for (int k = threadIdx.x; k < blocks; k += 64) c += p[k];
        }
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) c += __shfl_xor(c, off, 64);
        if (threadIdx.x == 0) row[entry] = (double)c;
    }
}

void launch_verify_members(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, const float* truth, CellBox box,
                           bool fair, float* crps_map, void* partials, double* row)
{
    const int blocks = verify_blocks(box), M = mb.count;
    const unsigned cells = box.empty() ? 0u : (unsigned)(box.row_hi - box.row_lo) * (unsigned)(box.col_hi - box.col_lo);
    double* psums = static_cast<double*>(partials);
    unsigned* pbins = reinterpret_cast<unsigned*>(psums + (size_t)4 * blocks);
    const double dpair = (double)(fair ? M * (M - 1) : M * M);
    if (blocks > 0) {
#define FLUID_VERIFY_LAUNCH(S, MP)                                                                                                           \
    hipLaunchKernelGGL((k_verify_members<S, MP>), dim3(blocks), dim3(256), 0, s, (const S*)x, pitch, n + 2, mb.stride, M, inv, truth, box, cells, \
                       dpair, crps_map, psums, pbins)
#define FLUID_VERIFY_BY_MP(S)                      \
    do {                                           \
        if (M <= 2) FLUID_VERIFY_LAUNCH(S, 2);     \
        else if (M <= 4) FLUID_VERIFY_LAUNCH(S, 4);   \
        else if (M <= 8) FLUID_VERIFY_LAUNCH(S, 8);   \
        else if (M <= 16) FLUID_VERIFY_LAUNCH(S, 16); \
        else if (M <= 32) FLUID_VERIFY_LAUNCH(S, 32); \
        else FLUID_VERIFY_LAUNCH(S, 64);           \
    } while (0)
        if (st == STORAGE_F16) FLUID_VERIFY_BY_MP(half_t);
        else FLUID_VERIFY_BY_MP(float);
#undef FLUID_VERIFY_BY_MP
#undef FLUID_VERIFY_LAUNCH
    }
    hipLaunchKernelGGL(k_verify_fold, dim3(kVerifyRow), dim3(64), 0, s, psums, pbins, blocks, M, (double)cells, row);
}

}  // namespace fluid
