// The ETKF solve of the one-call analysis (include/fluid_amd.h "one-call analysis"): one kernel and its launch wrapper, in a
// translation unit of their own.  Declarations: fluid_etkf.h.
#include <hip/hip_runtime.h>

#include "fluid_etkf.h"

namespace fluid {

// ---------------------------------------------------------------------------
// The ETKF solve of one lattice node per block (include/fluid_amd.h "one-call analysis"; DESIGN.md has the layout).
// S = mirror(C) + shift * I and V = I live in LDS, rows padded to MP + 1 doubles: a row walk (lane = column) is unit
// stride and a column walk (lane = row) has the odd stride MP + 1, so neither phase of a rotation meets a bank twice.
// Cyclic Jacobi in the round-robin ordering: n = M rounded up to even, n - 1 steps per sweep, in step s the pairs
// {n - 1, s} and {(s + i) mod (n - 1), (s - i) mod (n - 1)}, i = 1 .. n / 2 - 1 -- disjoint, so they rotate together; a
// pair with the bye index M (odd M) does nothing.  Per step: lane i < n / 2 works out pair i's rotation once, barrier,
// rows p and q of S for every pair (J^T S), barrier, columns p and q of S and of V (S J, V J) with the pair's own 2 x 2
// block set to its closed form, barrier.  Every loop is bounded by M or kEtkfMaxSweeps alone; what ends the sweeps or
// fails the node is a word in LDS every thread reads after a barrier, so all 256 threads reach every barrier.  A node
// that fails or is empty stores +0 everywhere.  No atomics, no matrix instructions: each entry of the result is one
// thread's sum in index order.
// ---------------------------------------------------------------------------
__device__ __forceinline__ bool etkf_finite(double x) { return fabs(x) <= 1.7976931348623157e308; }

template <int MP>
__global__ __launch_bounds__(256) void k_etkf_solve(EtkfOperands in, EtkfResults out, int M, double shift)
{
#pragma clang fp contract(off)
    constexpr int LD = MP + 1, HP = MP / 2;
    __shared__ double S[MP * LD], V[MP * LD];
    __shared__ double rot_c[HP], rot_s[HP], rot_pp[HP], rot_qq[HP], lam[MP], scale[MP], proj[MP], wv[MP], rh[MP];
    __shared__ unsigned long long rowbits[MP];
    __shared__ int rot_p[HP], rot_q[HP], rot_on[HP], rotated, failed;
    const int tid = (int)threadIdx.x, MM = M * M;
    const size_t node = blockIdx.x;
    const int count = !in.counts ? 1 : in.starts ? in.counts[node + 1] - in.counts[node] : in.counts[node];      // block-uniform
    if (tid == 0) rotated = failed = 0;
    __syncthreads();
    const bool empty = count == 0;
    if (!empty) {
        const double* __restrict__ g = in.gram + node * in.gram_node;
        for (int e = tid; e < MM; e += 256) {
            const int k = e / M, m = e - k * M;
            const double a = k <= m ? g[(size_t)k * in.gram_row + m] : g[(size_t)m * in.gram_row + k];
            if (!etkf_finite(a)) failed = 1;
            S[k * LD + m] = k == m ? shift + a : a;
            V[k * LD + m] = k == m ? 1.0 : 0.0;
        }
        if (tid < M) {
            const double r = in.rhs[node * in.rhs_node + tid];
            if (!etkf_finite(r)) failed = 1;
            rh[tid] = r;
        }
    }
    __syncthreads();
    bool bad = failed != 0;                                           // block-uniform from here on: read behind a barrier
    const int n = (M + 1) & ~1, half = n >> 1, ring = n - 1;
    bool converged = false;
    for (int sweep = 0; sweep < kEtkfMaxSweeps && !empty && !bad && !converged; ++sweep) {
        for (int step = 0; step < ring; ++step) {
            if (tid < half) {
                const int a = tid == 0 ? ring : (step + tid) % ring, b = tid == 0 ? step : (step - tid + ring) % ring;
                const int p = a < b ? a : b, q = a < b ? b : a;
                int on = 0;
                double c = 1.0, s = 0.0, npp = 0.0, nqq = 0.0;
                if (q < M) {
                    const double app = S[p * LD + p], aqq = S[q * LD + q], apq = S[p * LD + q];
                    if (!(fabs(apq) <= 0x1p-53 * (sqrt(app) * sqrt(aqq)))) {      // (a NaN anywhere rotates: it runs into the cap)
                        const double theta = (aqq - app) / (2.0 * apq), at = fabs(theta);
                        double t = at > 0x1p500 ? 0.5 / at : 1.0 / (at + sqrt(theta * theta + 1.0));      // theta^2 would overflow
                        if (theta < 0.0) t = -t;
                        c = 1.0 / sqrt(t * t + 1.0);
                        s = t * c;
                        npp = app - t * apq;
                        nqq = aqq + t * apq;
                        on = 1;
                        rotated = 1;
                    }
                }
                rot_p[tid] = p;
                rot_q[tid] = q;
                rot_on[tid] = on;
                rot_c[tid] = c;
                rot_s[tid] = s;
                rot_pp[tid] = npp;
                rot_qq[tid] = nqq;
            }
            __syncthreads();
            for (int e = tid; e < half * M; e += 256) {              // J^T S: rows p and q, lane = column
                const int i = e / M, j = e - i * M;
                if (!rot_on[i]) continue;
                const int p = rot_p[i], q = rot_q[i];
                const double c = rot_c[i], s = rot_s[i], x = S[p * LD + j], y = S[q * LD + j];
                S[p * LD + j] = c * x - s * y;
                S[q * LD + j] = s * x + c * y;
            }
            __syncthreads();
            for (int e = tid; e < half * M; e += 256) {              // S J and V J: columns p and q, lane = row
                const int i = e / M, r = e - i * M;
                if (!rot_on[i]) continue;
                const int p = rot_p[i], q = rot_q[i];
                const double c = rot_c[i], s = rot_s[i], x = S[r * LD + p], y = S[r * LD + q];
                double nx = c * x - s * y, ny = s * x + c * y;
                if (r == p) {
                    nx = rot_pp[i];
                    ny = 0.0;
                } else if (r == q) {
                    nx = 0.0;
                    ny = rot_qq[i];
                }
                S[r * LD + p] = nx;
                S[r * LD + q] = ny;
                const double vx = V[r * LD + p], vy = V[r * LD + q];
                V[r * LD + p] = c * vx - s * vy;
                V[r * LD + q] = s * vx + c * vy;
            }
            __syncthreads();
        }
        converged = rotated == 0;                                     // a sweep without a rotation ends the solve
        __syncthreads();
        if (tid == 0) rotated = 0;
        __syncthreads();
    }
    const bool solve = !empty && !bad && converged;                   // (the cap reached: failed)
    if (solve && tid < M) {
        const double l = S[tid * LD + tid];
        if (!(etkf_finite(l) && l > 0.0)) failed = 1;
        lam[tid] = l;
    }
    __syncthreads();
    const bool fold = solve && failed == 0;
    if (fold && tid < M) {                                            // (V^T rhs)_i / lambda_i and sqrt((M - 1) / lambda_i)
        double t = 0.0;
        for (int k = 0; k < M; ++k) t = t + V[k * LD + tid] * rh[k];
        proj[tid] = t / lam[tid];
        scale[tid] = sqrt((double)(M - 1) / lam[tid]);
    }
    __syncthreads();
    if (fold && tid < M) {
        double t = 0.0;
        for (int i = 0; i < M; ++i) t = t + V[tid * LD + i] * proj[i];
        wv[tid] = t;
    }
    __syncthreads();
    if (fold)
        for (int e = tid; e < MM; e += 256) {                        // D = W - I + w 1^T, kept as the float it is stored as
            const int k = e / M, m = e - k * M;
            double t = 0.0;
            for (int i = 0; i < M; ++i) t = t + (V[k * LD + i] * V[m * LD + i]) * scale[i];
            const float d = (float)((t - (k == m ? 1.0 : 0.0)) + wv[k]);
            if (!(fabsf(d) <= 3.402823466e38f)) failed = 1;
            S[k * LD + m] = (double)d;
        }
    __syncthreads();
    const bool keep = fold && failed == 0;
    const int status = empty ? 1 : keep ? 0 : 2;
    if (out.increments) {
        float* __restrict__ o = out.increments + node * (size_t)MM;
        for (int e = tid; e < MM; e += 256) {
            const int k = e / M, m = e - k * M;
            o[e] = keep ? (float)S[k * LD + m] : 0.0f;
        }
    } else {
        int tp = 1;
        while (tp < M) tp <<= 1;                                      // transform_padded(M)
        double* __restrict__ o = out.table + node * (size_t)M * (size_t)tp;
        for (int e = tid; e < M * tp; e += 256) {
            const int k = e / tp, m = e - k * tp;
            o[e] = keep && m < M ? S[k * LD + m] : 0.0;
        }
        if (tid < M) {
            unsigned long long word = 0;
            if (keep)
                for (int m = 0; m < M; ++m)
                    if (S[tid * LD + m] != 0.0) word |= 1ull << m;
            out.bits[node * (size_t)M + tid] = word;
            rowbits[tid] = word;
        }
        __syncthreads();
        if (tid == 0) {
            unsigned long long all = 0;
            for (int k = 0; k < M; ++k) all |= rowbits[k];
            out.cols[node] = all;
        }
    }
    if (out.status && tid == 0) out.status[node] = status;
}

// the LDS arrays are sized by the padding of the Gram kernels: a small ensemble does not pay for 64 members
void launch_etkf_solve(hipStream_t s, int members, double shift, const EtkfOperands& in, const EtkfResults& out, int nodes)
{
#define FLUID_ETKF_CASE(MP)                                                                                           \
    case MP:                                                                                                          \
        hipLaunchKernelGGL((k_etkf_solve<MP>), dim3((unsigned)nodes), dim3(256), 0, s, in, out, members, shift);      \
        break
    switch (gram_padded(members)) {
        FLUID_ETKF_CASE(8);
        FLUID_ETKF_CASE(16);
        FLUID_ETKF_CASE(32);
        FLUID_ETKF_CASE(64);
    }
#undef FLUID_ETKF_CASE
}

}  // namespace fluid
