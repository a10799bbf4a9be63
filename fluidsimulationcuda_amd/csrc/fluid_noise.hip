// Ensemble noise (include/fluid_amd.h "ensemble noise"): two kernels and their launch wrappers, in a translation unit of
// their own.  Declarations and the generator's one body: fluid_noise.h.
#include <hip/hip_runtime.h>

#include "fluid_noise.h"

namespace fluid {

// (fluid_kernels.hip has the reason: the empty asm keeps widening / narrowing conversions from folding into mixed-precision
// instructions that round once where the contract rounds twice)
__device__ __forceinline__ float noise_keep_f32(float v) { asm("" : "+v"(v)); return v; }

// ---------------------------------------------------------------------------
// k_noise_members: the lane and vector shape of k_relax_spread -- one lane per vector of 4 columns of a row in both storage
// types (16-byte accesses of float fields, 8-byte ones of half fields), vector 0 ghost column 0 alone, vector v >= 1 columns
// 1 + 4 * (v - 1) .. 4 * v, a row's edge vectors touching their valid columns one by one so that pad columns are neither
// read nor written.  The member rides in the grid (blockIdx.y); its base is 64-bit scalar arithmetic per block, and so is
// its amplitude, one wave-uniform load.  A lane's four cells are four independent Philox chains: ten rounds of two 32 x 32
// -> 64 multiplies each, nothing shared between them but the key schedule.  SET stores without reading; ADD reads the
// vector first, and a member whose amplitude is +-0 leaves at once -- the whole block, the amplitude being the block's.
// No LDS, no atomics, plain vector stores.
// ---------------------------------------------------------------------------
constexpr int kNoiseVW = 4;

template <typename S, bool ADD>
__global__ __launch_bounds__(256) void k_noise_members(S* __restrict__ x, int pitch, int n, size_t ms, int vecs, float inv, float scale,
                                                       float amp, const float* __restrict__ mamp, NoiseKey key, unsigned tag, unsigned first_id)
{
#pragma clang fp contract(off)
    constexpr int VW = kNoiseVW;
    typedef S vec_t __attribute__((ext_vector_type(VW)));
    if (mamp) amp = mamp[blockIdx.y];                              // this member's own amplitude (wave-uniform)
    if (ADD && amp == 0.0f) return;                                // rule: a member with a_m == +-0 keeps every bit
    const unsigned t = blockIdx.x * 256u + threadIdx.x;           // (n + 2) * vecs < 2^32 for every N the library accepts
    if (t >= (unsigned)(n + 2) * (unsigned)vecs) return;
    const int row = (int)(t / (unsigned)vecs), v = (int)(t % (unsigned)vecs);
    const int c0 = 1 + VW * (v - 1);                               // first column of this lane's vector (vector 0: 1 - VW)
    int valid = 0;
#pragma unroll
    for (int e = 0; e < VW; ++e)
        if (c0 + e >= 0 && c0 + e <= n + 1) valid |= 1 << e;
    const bool whole = valid == (1 << VW) - 1;
    // element 0 of the vector; for vector 0 that lies in the left pad (only element VW - 1 is touched)
    S* __restrict__ p = x + blockIdx.y * ms + ((size_t)row * (size_t)pitch + (size_t)(XOFF + c0));
    const unsigned word2 = tag | (first_id + blockIdx.y);
    const double a = (double)amp;

    S old[VW];
    if constexpr (ADD) {
        if (whole) {
            const vec_t o = *reinterpret_cast<const vec_t*>(p);
#pragma unroll
            for (int e = 0; e < VW; ++e) old[e] = o[e];
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) old[e] = ((valid >> e) & 1) ? p[e] : (S)0;
        }
    }
    S y[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) {
        const double z = noise_z(key.k0, key.k1, (unsigned)(c0 + e), (unsigned)row, word2, key.sequence);
        const double prod = __dmul_rn(a, z);
        if constexpr (!ADD) {
            const float f = (float)prod;
            if constexpr (sizeof(S) == 4) y[e] = f;
            else y[e] = (S)noise_keep_f32(f);
        } else {
            double xd;
            if constexpr (sizeof(S) == 4) xd = (double)old[e];
            else xd = (double)(noise_keep_f32((float)old[e]) * inv);
            const float f = (float)__dadd_rn(xd, prod);
            if constexpr (sizeof(S) == 4) y[e] = f;
            else y[e] = (S)noise_keep_f32(noise_keep_f32((float)(S)noise_keep_f32(f)) * scale);      // narrow(y), then the field's scale
        }
    }
    if (whole) {
        vec_t o;
#pragma unroll
        for (int e = 0; e < VW; ++e) o[e] = y[e];
        *reinterpret_cast<vec_t*>(p) = o;
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
            if ((valid >> e) & 1) p[e] = y[e];
    }
}

// one lane per float, blocks striding over the array: q may pass 2^32, its two halves are the counter's first two words
constexpr unsigned kNoiseDenseBlocks = 1u << 20;

__global__ __launch_bounds__(256) void k_noise_dense(float* __restrict__ out, size_t count, float amp, NoiseKey key, unsigned word2)
{
#pragma clang fp contract(off)
    const double a = (double)amp;
    for (size_t q = (size_t)blockIdx.x * 256u + threadIdx.x; q < count; q += (size_t)gridDim.x * 256u) {
        const double z = noise_z(key.k0, key.k1, (unsigned)q, (unsigned)(q >> 32), word2, key.sequence);
        out[q] = (float)__dmul_rn(a, z);
    }
}

static inline unsigned cdiv(unsigned a, unsigned b) { return (a + b - 1) / b; }

void launch_noise_members(hipStream_t s, int st, void* x, int pitch, int n, Members mb, bool add, float inv, float scale, float amp,
                          const float* mamp, NoiseKey key, int field, int first_id)
{
    const int vecs = 1 + (n + 1 + kNoiseVW - 1) / kNoiseVW;         // ghost column 0, then columns 1 .. n + 1 in vectors of 4
    const dim3 grid(cdiv((unsigned)(n + 2) * (unsigned)vecs, 256), mb.count);
    const unsigned tag = (unsigned)field << 16, id = (unsigned)first_id;
#define FLUID_NOISE_LAUNCH(S, ADD)                                                                                                        \
    hipLaunchKernelGGL((k_noise_members<S, ADD>), grid, dim3(256), 0, s, (S*)x, pitch, n, mb.stride, vecs, inv, scale, amp, mamp, key, tag, id)
    if (st == STORAGE_F16) {
        if (add) FLUID_NOISE_LAUNCH(half_t, true);
        else FLUID_NOISE_LAUNCH(half_t, false);
    } else {
        if (add) FLUID_NOISE_LAUNCH(float, true);
        else FLUID_NOISE_LAUNCH(float, false);
    }
#undef FLUID_NOISE_LAUNCH
}

void launch_noise_dense(hipStream_t s, float* out, size_t count, float amp, NoiseKey key, int stream_id)
{
    const size_t blocks = (count + 255) / 256;
    const unsigned grid = (unsigned)(blocks < kNoiseDenseBlocks ? blocks : kNoiseDenseBlocks);
    hipLaunchKernelGGL(k_noise_dense, dim3(grid), dim3(256), 0, s, out, count, amp, key, noise_word2(kNoiseDenseTag, stream_id));
}

}  // namespace fluid
