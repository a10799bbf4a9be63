// Ensemble noise (include/fluid_amd.h "ensemble noise"): the generator -- one body for the host and for the kernels -- and
// what fluid_solver.hip needs of fluid_noise.hip.
#pragma once
#include "fluid_kernels.h"

namespace fluid {

// Philox4x32-10 (Salmon, Moraes, Dror & Shaw 2011): ten rounds, the key bumped between them.  c: the counter in, the four
// random words out.
constexpr unsigned kPhiloxM0 = 0xD2511F53u, kPhiloxM1 = 0xCD9E8D57u, kPhiloxW0 = 0x9E3779B9u, kPhiloxW1 = 0xBB67AE85u;
constexpr int kPhiloxRounds = 10;
__host__ __device__ inline void philox4x32_10(unsigned (&c)[4], unsigned k0, unsigned k1)
{
#pragma unroll
    for (int r = 0; r < kPhiloxRounds; ++r) {
        const unsigned long long p0 = (unsigned long long)kPhiloxM0 * c[0], p1 = (unsigned long long)kPhiloxM1 * c[2];
        const unsigned n0 = (unsigned)(p1 >> 32) ^ c[1] ^ k0, n2 = (unsigned)(p0 >> 32) ^ c[3] ^ k1;
        c[0] = n0;
        c[1] = (unsigned)p1;
        c[2] = n2;
        c[3] = (unsigned)p0;
        k0 += kPhiloxW0;
        k1 += kPhiloxW1;
    }
}

// The counter words 2 of the header: (tag << 16) | id.  Tags 0 .. FLUID_NFIELDS - 1 are field ids (id: the member),
// kNoiseDenseTag is fluid_noise_dense's (id: the stream).
constexpr int kNoiseDenseTag = 15, kNoiseIds = 65536;
__host__ __device__ inline unsigned noise_word2(int tag, int id) { return ((unsigned)tag << 16) | (unsigned)id; }

// z of one counter: S = the sum of the eight 16-bit halves of the four words, an integer in [0, 524280]; z = (double)(S -
// 262140) * C, C = 1 / sqrt(8 * (2^32 - 1) / 12) rounded once: the integer is exact in double, so z is ONE rounding.
// Irwin-Hall with n = 8: mean 0, variance 1, |z| <= 4.899.
constexpr double kNoiseC = 0x1.3988e1412ed76p-16;
__host__ __device__ inline double noise_z(unsigned k0, unsigned k1, unsigned c0, unsigned c1, unsigned c2, unsigned c3)
{
    unsigned c[4] = {c0, c1, c2, c3};
    philox4x32_10(c, k0, k1);
    int sum = 0;
#pragma unroll
    for (int w = 0; w < 4; ++w) sum += (int)(c[w] & 0xffffu) + (int)(c[w] >> 16);
    return (double)(sum - 262140) * kNoiseC;
}

// fluid_noise_members on one field, all mb.count members: cell (row i, column j) of member m gets the z of counter (j, i,
// noise_word2(field, first_id + m), sequence) under the key (k0, k1) times the member's amplitude -- mamp[m], or `amp` for
// everybody where mamp is null.  add == false: x = narrow((float)(a * z)) in every cell of the (n + 2)^2 array.  add ==
// true: x = narrow((float)(widen(x) * inv + a * z)) * scale, product and sum rounded one after the other, in double; a
// member whose amplitude is +-0 is neither read nor stored.  `inv`, `scale`: as for launch_transform_members_local.  One
// launch, the member in the grid; pad columns are neither read nor written.
struct NoiseKey {
    unsigned k0, k1, sequence;
};
void launch_noise_members(hipStream_t s, int st, void* x, int pitch, int n, Members mb, bool add, float inv, float scale, float amp,
                          const float* mamp, NoiseKey key, int field, int first_id);
// fluid_noise_dense: out[q] = (float)((double)amp * z of counter (low 32 bits of q, high 32 bits of q, noise_word2(kNoiseDenseTag,
// stream_id), sequence)), q < count.  One launch; count > 0.
void launch_noise_dense(hipStream_t s, float* out, size_t count, float amp, NoiseKey key, int stream_id);

}  // namespace fluid
