// fluid_kernels.hip -- hand-written gfx950 (CDNA4) kernels for the
// Stable-Fluids step: boundary, sources, Jacobi sweep, advection, divergence,
// pressure-gradient subtraction, plus two wavefront reductions.
//
// Arithmetic contract (bit parity with the reference's
// project/sequential/FluidSequential.c): every expression keeps the reference's
// operand order, division is true IEEE division, and this file is compiled with
// -ffp-contract=off so no multiply-add is fused.
//
// Device field layout (see DESIGN.md "Data layout in HBM"): a field is W=n+2
// rows of `pitch` floats; column c of a row sits at float index c+XOFF with
// XOFF=63, so interior column 1 starts a 256-byte line and a wave's 64 float4
// accesses cover whole 128-byte lines.  Pad floats (index <63 and >n+64) are
// zero-initialised and never read as data.
//
// Every stencil kernel takes a global interior row range [row_lo,row_hi) so the
// same code serves one GPU (1..n) and a row slab of a multi-GPU run, and every
// kernel applies the reference's set_bnd (FluidSequential.c:62-75) itself: the
// thread that produces an interior cell next to a wall also writes the ghost
// cell(s) derived from it, so no separate boundary launch is needed.
//
// Ensembles: every kernel that touches a field takes the member stride `ms` (elements between two members of a field) and
// finds its member in the grid -- blockIdx.z where y is the row, blockIdx.y in the one-dimensional kernels, blockIdx.z /
// (solves per launch) in the fused Jacobi kernel -- and adds member * ms to its field pointers first thing: scalar
// arithmetic on the kernel arguments, after which the kernel is the one-simulation kernel.
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <array>
#include <cstdlib>
#include <utility>

#include "fluid_kernels.h"

namespace fluid {

// ---------------------------------------------------------------------------
// helpers
// ---------------------------------------------------------------------------
__device__ __forceinline__ float flip_if(bool c, float v) { return c ? -v : v; }

// Field storage type S: float (the reference's arithmetic, bit for bit) or
// _Float16 (BASELINE config 4: fp16 fields, every operation still in fp32 on the
// widened values, one round-to-nearest when a kernel stores).
// With fp16 storage hipcc likes to fold the widening / narrowing conversions into
// mixed-precision instructions (observed: fmul + fptrunc -> v_fma_mixlo_f16 x, y, 0),
// which rounds the exact product straight to fp16 and adds a +0 that flips -0
// results: neither is "the fp32 operation, then one rounding on store".  An empty
// asm on the value (no instruction) keeps the conversions separate.
__device__ __forceinline__ float keep_f32(float v) { asm("" : "+v"(v)); return v; }
__device__ __forceinline__ float ld1(const float* p) { return *p; }
__device__ __forceinline__ float ld1(const half_t* p) { return keep_f32((float)*p); }
__device__ __forceinline__ void st1(float* p, float v) { *p = v; }
__device__ __forceinline__ void st1(half_t* p, float v) { *p = (half_t)keep_f32(v); }
// a value as it reads back after a store in the storage type (fp16 storage: rounded once; fp32: itself)
template <typename S>
__device__ __forceinline__ float as_stored(float v)
{
    if constexpr (sizeof(S) == 2) return keep_f32((float)(S)keep_f32(v));
    else return v;
}
typedef half_t half4_t __attribute__((ext_vector_type(4)));
__device__ __forceinline__ float4 ld4(const float* p) { return *reinterpret_cast<const float4*>(p); }
__device__ __forceinline__ float4 ld4(const half_t* p)
{
    const half4_t h = *reinterpret_cast<const half4_t*>(p);
    return make_float4(keep_f32((float)h.x), keep_f32((float)h.y), keep_f32((float)h.z), keep_f32((float)h.w));
}
__device__ __forceinline__ void st4(float* p, const float4& v) { *reinterpret_cast<float4*>(p) = v; }
__device__ __forceinline__ void st4(half_t* p, const float4& v)
{
    half4_t h;
    h.x = (half_t)keep_f32(v.x); h.y = (half_t)keep_f32(v.y); h.z = (half_t)keep_f32(v.z); h.w = (half_t)keep_f32(v.w);
    *reinterpret_cast<half4_t*>(p) = h;
}

// Range-checked buffer loads/stores (buf_ldv / buf_stv below) for the fused kernel's steady state: the
// hardware range check (offset >= num_records: loads return 0, stores are
// dropped) replaces every `if` around a memory operation, so the loop body has a
// fixed number of them and hipcc can emit counted s_waitcnt vmcnt(N) instead of
// draining the queue (vmcnt(0)) once per iteration -- which is what keeps three
// rows of loads in flight.  kBufOff disables a lane: added to any in-field
// offset it stays below 2^32 and above num_records (fields are < 2 GiB).
constexpr unsigned kBufOff = 0x80000000u;
typedef unsigned uint4_t __attribute__((ext_vector_type(4)));
typedef unsigned uint2_t __attribute__((ext_vector_type(2)));

// value of lane-1 / lane+1 across the whole 64-wide wave (DPP wave shifts; one
// VALU op each, no LDS).  Lane 0 / 63 receive `edge`.
__device__ __forceinline__ float from_lane_below(float v, float edge)
{
    int r = __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v),
                                        0x138 /*wave_shr:1*/, 0xf, 0xf, false);
    return __int_as_float(r);
}
__device__ __forceinline__ float from_lane_above(float v, float edge)
{
    int r = __builtin_amdgcn_update_dpp(__float_as_int(edge), __float_as_int(v),
                                        0x130 /*wave_shl:1*/, 0xf, 0xf, false);
    return __int_as_float(r);
}

// Same shifts with bound_ctrl: lane 0 / 63 read 0.  No `old` operand to set up,
// so the compiler folds the shift into the consuming add (v_add_f32_dpp).
__device__ __forceinline__ float lane_below0(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x138, 0xf, 0xf, true));
}
__device__ __forceinline__ float lane_above0(float v)
{
    return __int_as_float(__builtin_amdgcn_update_dpp(0, __float_as_int(v), 0x130, 0xf, 0xf, true));
}

// Ghost cells that derive from interior cell (j,i) holding `val`
// (FluidSequential.c:65-74): across a vertical wall the ghost is -val when
// b==1, across a horizontal wall -val when b==2, else a copy; a corner is
// 0.5f*(horizontal neighbour + vertical neighbour), both of which are ghosts of
// the same corner-most interior cell.  Handles n==1 (a cell on several walls).
template <typename S>
__device__ __forceinline__ void emit_ghosts(S* __restrict__ f, size_t pitch, int n, int b, int j, int i, float val)
{
    const bool nx = (b == 1), ny = (b == 2);
    const bool left = (j == 1), right = (j == n), top = (i == 1), bot = (i == n);
    if (!(left | right | top | bot)) return;
    const float gx = flip_if(nx, val);
    const float gy = flip_if(ny, val);
    const float corner = 0.5f * (gy + gx);   // 0.5f*(x[horizontal nbr] + x[vertical nbr])
    S* r0 = f + XOFF;
    S* ri = f + (size_t)i * pitch + XOFF;
    S* rn = f + (size_t)(n + 1) * pitch + XOFF;
    if (left) st1(ri, gx);
    if (right) st1(ri + n + 1, gx);
    if (top) st1(r0 + j, gy);
    if (bot) st1(rn + j, gy);
    if (top & left) st1(r0, corner);
    if (top & right) st1(r0 + n + 1, corner);
    if (bot & left) st1(rn, corner);
    if (bot & right) st1(rn + n + 1, corner);
}

// ---------------------------------------------------------------------------
// a2  set_bnd as its own kernel (C-ABI operator + tests; the step itself uses
// the fused form).  One thread per edge index k in 1..n; thread k==1 / k==n
// also writes the corners from the values it just produced.
// ---------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(256) void k_set_bnd(S* __restrict__ f, int pitch, int n, int b, size_t ms)
{
    const int k = 1 + blockIdx.x * 256 + threadIdx.x;
    if (k > n) return;
    f += blockIdx.y * ms;
    const size_t P = (size_t)pitch;
    const bool nx = (b == 1), ny = (b == 2);
    S* r0 = f + XOFF;
    S* rk = f + (size_t)k * P + XOFF;
    S* r1 = f + P + XOFF;
    S* rN = f + (size_t)n * P + XOFF;
    S* rn = f + (size_t)(n + 1) * P + XOFF;
    const float gl = flip_if(nx, ld1(rk + 1));      // x[0,k]
    const float gr = flip_if(nx, ld1(rk + n));      // x[n+1,k]
    const float gt = flip_if(ny, ld1(r1 + k));      // x[k,0]
    const float gb = flip_if(ny, ld1(rN + k));      // x[k,n+1]
    st1(rk, gl);
    st1(rk + n + 1, gr);
    st1(r0 + k, gt);
    st1(rn + k, gb);
    if (k == 1) {
        st1(r0, 0.5f * (gt + gl));                                  // x[1,0] + x[0,1]
        st1(rn, 0.5f * (gb + flip_if(nx, ld1(rN + 1))));            // x[1,n+1] + x[0,n]
    }
    if (k == n) {
        st1(r0 + n + 1, 0.5f * (gt + flip_if(nx, ld1(r1 + n))));    // x[n,0] + x[n+1,1]
        st1(rn + n + 1, 0.5f * (gb + gr));                          // x[n,n+1] + x[n+1,n]
    }
}

// ---------------------------------------------------------------------------
// a3  add_source: x += dt*s on every cell of rows [row_lo,row_hi), ghosts
// included (FluidSequential.c:78-82).  Streams whole padded rows as float4
// (pads are 0 and stay 0).
// ---------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(256) void k_add_source(S* __restrict__ x, const S* __restrict__ s, int pitch, int row_lo,
                                                    int row_hi, float dt, size_t ms, const float* __restrict__ mdt)
{
    if (mdt) dt = mdt[blockIdx.y];          // this member's own dt (wave-uniform)
    const int nvec = pitch >> 2;
    const size_t total = (size_t)(row_hi - row_lo) * nvec;
    S* xv = x + blockIdx.y * ms + (size_t)row_lo * pitch;
    const S* sv = s + blockIdx.y * ms + (size_t)row_lo * pitch;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        float4 a = ld4(xv + 4 * t);
        const float4 c = ld4(sv + 4 * t);
        a.x = a.x + dt * c.x;
        a.y = a.y + dt * c.y;
        a.z = a.z + dt * c.z;
        a.w = a.w + dt * c.w;
        st4(xv + 4 * t, a);
    }
}

// add_source when the source field is known to be all +0: x += inc with inc = dt*(+0)
// formed on the host (so x = -0 still becomes +0 for dt >= 0, exactly as x + dt*0 does).
template <typename S>
__global__ __launch_bounds__(256) void k_add_zero_source(S* __restrict__ x, int pitch, int row_lo, int row_hi, float inc, size_t ms,
                                                         const float* __restrict__ minc)
{
    if (minc) inc = minc[blockIdx.y];       // this member's own increment (wave-uniform)
    const int nvec = pitch >> 2;
    const size_t total = (size_t)(row_hi - row_lo) * nvec;
    S* xv = x + blockIdx.y * ms + (size_t)row_lo * pitch;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        float4 a = ld4(xv + 4 * t);
        a.x = a.x + inc;
        a.y = a.y + inc;
        a.z = a.z + inc;
        a.w = a.w + inc;
        st4(xv + 4 * t, a);
    }
}

// x *= factor on rows [row_lo, row_hi) (factor a power of two: how a field kept scaled -- the pressure and its right-hand
// side with fp16 storage, see fluid_solver.hip: project -- goes back to its plain values for a reader that does not know)
template <typename S>
__global__ __launch_bounds__(256) void k_scale(S* __restrict__ x, int pitch, int row_lo, int row_hi, float factor, size_t ms)
{
    const int nvec = pitch >> 2;
    const size_t total = (size_t)(row_hi - row_lo) * nvec;
    S* xv = x + blockIdx.y * ms + (size_t)row_lo * pitch;
    for (size_t t = (size_t)blockIdx.x * 256 + threadIdx.x; t < total; t += (size_t)gridDim.x * 256) {
        float4 a = ld4(xv + 4 * t);
        a.x = a.x * factor;
        a.y = a.y * factor;
        a.z = a.z * factor;
        a.w = a.w * factor;
        st4(xv + 4 * t, a);
    }
}

// ---------------------------------------------------------------------------
// a4  Jacobi sweep, three variants.  All compute, for interior rows
// [row_lo,row_hi) and columns 1..n,
//     out = (x0 + alpha*(((L + R) + U) + D)) / beta     (FluidSequential.c:95-96)
// and the ghosts of `out` that derive from those cells.
// ---------------------------------------------------------------------------

// (i) naive-global: one thread per cell, five global loads.
template <typename S>
__global__ __launch_bounds__(256) void k_jacobi_naive(const S* __restrict__ x, const S* __restrict__ x0,
                                                      S* __restrict__ out, int pitch, int n, int row_lo,
                                                      int row_hi, float alpha, float beta, int b, size_t ms, const float2* __restrict__ mab)
{
    if (mab) {                              // this member's own coefficients (wave-uniform)
        const float2 ab = mab[blockIdx.z];
        alpha = ab.x;
        beta = ab.y;
    }
    const int j = 1 + blockIdx.x * 64 + (threadIdx.x & 63);
    const int i = row_lo + blockIdx.y * 4 + (threadIdx.x >> 6);
    if (j > n || i >= row_hi) return;
    x += blockIdx.z * ms; x0 += blockIdx.z * ms; out += blockIdx.z * ms;
    const size_t P = (size_t)pitch;
    const S* c = x + (size_t)i * P + XOFF + j;
    float nb = ld1(c - 1) + ld1(c + 1);
    nb = nb + ld1(c - (ptrdiff_t)P);
    nb = nb + ld1(c + P);
    const float val = (ld1(x0 + (size_t)i * P + XOFF + j) + alpha * nb) / beta;
    st1(out + (size_t)i * P + XOFF + j, val);
    emit_ghosts(out, P, n, b, j, i, val);
}

// (ii) LDS-tiled: a (TY+2)x(TX+2) halo tile of x staged in LDS per workgroup
// (TX=64, TY=16, 256 threads, each thread 4 rows of one column).  Tile corners
// are not needed by a 5-point stencil and are not loaded.
constexpr int LT_X = 64, LT_Y = 16;
template <typename S>
__global__ __launch_bounds__(256) void k_jacobi_lds(const S* __restrict__ x, const S* __restrict__ x0,
                                                    S* __restrict__ out, int pitch, int n, int row_lo,
                                                    int row_hi, float alpha, float beta, int b, size_t ms, const float2* __restrict__ mab)
{
    if (mab) {                              // this member's own coefficients (wave-uniform)
        const float2 ab = mab[blockIdx.z];
        alpha = ab.x;
        beta = ab.y;
    }
    __shared__ float tile[LT_Y + 2][LT_X + 2 + 1];
    x += blockIdx.z * ms; x0 += blockIdx.z * ms; out += blockIdx.z * ms;
    const int tx = threadIdx.x & 63, ty = threadIdx.x >> 6;      // ty in 0..3
    const int j0 = 1 + blockIdx.x * LT_X, i0 = row_lo + blockIdx.y * LT_Y;
    const int j = j0 + tx;
    const size_t P = (size_t)pitch;
    const int rows = min(LT_Y, row_hi - i0);
    const int cols = min(LT_X, n - j0 + 1);
    // body + top/bottom halo rows: rows i0-1 .. i0+rows, 64 columns each
    for (int r = ty; r < rows + 2; r += 4)
        if (tx < cols) tile[r][tx + 1] = ld1(x + (size_t)(i0 - 1 + r) * P + XOFF + j);
    // left/right halo columns
    if (threadIdx.x < 2 * LT_Y) {
        const int r = threadIdx.x >> 1, side = threadIdx.x & 1;
        if (r < rows) {
            const int jj = side ? j0 + cols : j0 - 1;
            tile[r + 1][side ? cols + 1 : 0] = ld1(x + (size_t)(i0 + r) * P + XOFF + jj);
        }
    }
    __syncthreads();
    if (tx >= cols) return;
#pragma unroll
    for (int k = 0; k < LT_Y / 4; ++k) {
        const int r = ty + 4 * k;
        if (r >= rows) break;
        const int i = i0 + r;
        float nb = tile[r + 1][tx] + tile[r + 1][tx + 2];
        nb = nb + tile[r][tx + 1];
        nb = nb + tile[r + 2][tx + 1];
        const float val = (ld1(x0 + (size_t)i * P + XOFF + j) + alpha * nb) / beta;
        st1(out + (size_t)i * P + XOFF + j, val);
        emit_ghosts(out, P, n, b, j, i, val);
    }
}

// (iii) streaming: each lane owns one float4 (4 columns) and walks RB rows
// with a three-row register window, so every x row is fetched once per strip
// (+2 halo rows per RB); left/right neighbours come from the adjacent lanes by
// DPP wave shift, and only the wave's two edge lanes issue an extra dword load.
// 16 bytes per lane, 1 KiB per wave-instruction, 256-byte aligned.
template <int RB, typename S>
__global__ __launch_bounds__(256) void k_jacobi_stream(const S* __restrict__ x, const S* __restrict__ x0,
                                                       S* __restrict__ out, int pitch, int n, int row_lo,
                                                       int row_hi, float alpha, float beta, int b, size_t ms, const float2* __restrict__ mab)
{
    if (mab) {                              // this member's own coefficients (wave-uniform)
        const float2 ab = mab[blockIdx.z];
        alpha = ab.x;
        beta = ab.y;
    }
    x += blockIdx.z * ms; x0 += blockIdx.z * ms; out += blockIdx.z * ms;
    const int lane = threadIdx.x & 63;
    const int vec = blockIdx.x * 256 + threadIdx.x;     // float4 index along the row
    const int nvec = (n + 3) >> 2;
    const int i0 = row_lo + blockIdx.y * RB;
    const int i1 = min(i0 + RB, row_hi);
    const bool active = vec < nvec;
    const int v = active ? vec : nvec - 1;              // clamp: inactive lanes load valid memory
    const int j = 1 + 4 * v;                            // first column of this lane
    const size_t P = (size_t)pitch;
    const S* xc = x + XOFF + j;
    const S* rc = x0 + XOFF + j;
    S* oc = out + XOFF + j;
    const bool edge_lo = (lane == 0), edge_hi = (lane == 63) | (vec >= nvec - 1);
    const bool nx = (b == 1), ny = (b == 2);

    float4 up = ld4(xc + (size_t)(i0 - 1) * P);
    float4 me = ld4(xc + (size_t)i0 * P);
    for (int i = i0; i < i1; ++i) {
        const float4 dn = ld4(xc + (size_t)(i + 1) * P);
        const float4 r = ld4(rc + (size_t)i * P);
        float le = 0.f, re = 0.f;
        if (edge_lo) le = ld1(xc + (size_t)i * P - 1);
        if (edge_hi) re = ld1(xc + (size_t)i * P + 4);
        float L = from_lane_below(me.w, le);
        float R = from_lane_above(me.x, re);
        if (edge_lo) L = le;
        if (edge_hi) R = re;
        float4 o;
        float nb;
        nb = L + me.y;     nb = nb + up.x; nb = nb + dn.x; o.x = (r.x + alpha * nb) / beta;
        nb = me.x + me.z;  nb = nb + up.y; nb = nb + dn.y; o.y = (r.y + alpha * nb) / beta;
        nb = me.y + me.w;  nb = nb + up.z; nb = nb + dn.z; o.z = (r.z + alpha * nb) / beta;
        nb = me.z + R;     nb = nb + up.w; nb = nb + dn.w; o.w = (r.w + alpha * nb) / beta;
        if (active) {
            S* orow = oc + (size_t)i * P;
            const int last = n - j;            // component index of column n (>=0)
            if (last >= 3) {
                st4(orow, o);
            } else {                           // ragged right end: columns j..n only
                st1(orow, o.x);
                if (last >= 1) st1(orow + 1, o.y);
                if (last >= 2) st1(orow + 2, o.z);
            }
            // ---- fused set_bnd (selects only: no runtime-indexed arrays) ----
            const float vn = last == 0 ? o.x : last == 1 ? o.y : last == 2 ? o.z : o.w;  // column n
            if (j == 1) st1(orow - 1, flip_if(nx, o.x));                   // x[0,i]
            if (last <= 3) st1(orow + last + 1, flip_if(nx, vn));          // x[n+1,i]
            if (i == 1 || i == n) {
                float4 g4;
                g4.x = flip_if(ny, o.x); g4.y = flip_if(ny, o.y);
                g4.z = flip_if(ny, o.z); g4.w = flip_if(ny, o.w);
                const float cl = 0.5f * (g4.x + flip_if(nx, o.x));          // corner next to column 1
                const float cr = 0.5f * (flip_if(ny, vn) + flip_if(nx, vn)); // corner next to column n
#pragma unroll
                for (int side = 0; side < 2; ++side) {
                    if (side == 0 ? i != 1 : i != n) continue;
                    S* g = oc + (side == 0 ? (size_t)0 : (size_t)(n + 1) * P);
                    if (last >= 3) {
                        st4(g, g4);
                    } else {
                        st1(g, g4.x);
                        if (last >= 1) st1(g + 1, g4.y);
                        if (last >= 2) st1(g + 2, g4.z);
                    }
                    if (j == 1) st1(g - 1, cl);
                    if (last <= 3) st1(g + last + 1, cr);
                }
            }
        }
        up = me;
        me = dn;
    }
}

// (iv) temporally blocked: T sweeps per launch, results identical to T launches
// of any variant above (the only way past 12 B/cell/sweep).
//
// One wave = one window of 64 lanes x NV columns (NV = 2: 128 columns, the
// default; NV = 4: 256) x one strip of `rb` output rows, marching down the rows
// with all T sweeps in flight: at step t it loads row t of x and x0 and, for
// s = 1..T, produces row t-s of "x after s sweeps" from the three rows of stage
// s-1 it still holds.  Everything lives in registers: per stage a three-row ring
// of its input, a queue of the last T x0 rows, and three rows of x/x0 prefetched
// ahead of use.  The time loop is unrolled by three so the rings rotate by
// renaming, not by moving.  Left/right neighbours come from the adjacent lanes
// by DPP; a wave has no one to ask at its two ends, so windows overlap by
// HL = ceil(T/NV) lanes per side and only the inner 64-2*HL lanes store (the
// wrong values creep inwards one column per sweep and never reach them).  Strips
// overlap by T rows per side the same way.  No LDS, no barriers.
//
// set_bnd is replayed inside the pipeline (it must be: sweep s+1 reads the
// ghosts of sweep s): the lanes holding ghost column 0 / n+1 overwrite that
// component from the neighbouring interior column after every stage (EDGE
// windows only), and ghost rows 0 / n+1 of a stage are the flipped rows 1 / n
// of the same stage (steps near a wall take the `general` path; all others a
// branch-free body).  Domain walls do not shrink the valid region.  Corner
// ghosts are never read by a 5-point stencil, so they are only formed in the
// final store.  Negation is a sign-bit XOR (bit-identical to the reference's
// unary minus, zeros and NaNs included).
//
// The division by the per-solve constant beta comes in three forms (DIVMODE):
// 0: (..)/beta, true division (about 20 VALU-op times on gfx950).
// 4: beta is a power of two and alpha == 1.0f (the pressure solve: 1, 4):
//   `beta` carries the exact reciprocal, (..)*rbeta is the same correctly rounded
//   result for every input, and x * 1.0f is x, so alpha is not applied at all.
// 2: (float)((double)(..) * yd) with yd = RN64(1/beta).  The double product is
//   within 2^-52 relative of the true quotient, while a quotient of two floats is
//   never that close to a float rounding boundary (the boundary would need an odd
//   25-bit significand times beta's to fit 24 bits), so the final conversion
//   rounds exactly as IEEE division does; zeros, denormals, inf and NaN need no
//   special case.  The one exception class -- quotients that land exactly on a
//   denormal midpoint, possible for a few even-integer-like beta -- is why the
//   solver proves each beta on the device before using modes 2 and 4:
//   k_validate_div compares them with a/beta for all 2^32 inputs.
// 3: the two-term reciprocal q = fma(x, hi, x*lo) with hi = RD32(1/beta), lo = RN32(1/beta - hi) > 0 -- two
//   PACKED instructions per pair of cells where mode 2 takes six scalar ones.  hi + lo carries 1/beta to
//   ~2^-48 relative, which rounds like the true quotient for every x that is zero or at least beta * 2^-98 in
//   magnitude (k_validate_div proves it for all such x; lo > 0 keeps -0 / beta = -0); below that x*lo loses bits
//   to underflow and q can be one ulp off.  The dividends here are x0 + alpha*nb, and a float sum is either
//   zero or no smaller than 2^-24 of its smaller operand, or than half its larger one: wherever the right-hand
//   side x0 is at least m in magnitude, EVERY dividend of EVERY sweep is 0 or >= 2^-25 * m, whatever the
//   neighbours hold.  So no per-value guard is needed, only a fact about x0: k_tile_min_abs reduces |x0| over
//   tiles of kTileRows x kTileCols cells once per solve (x0 does not change during a solve), and a wave takes
//   the two-term path if every tile its strip and window touch (overlaps included) is >= beta * 2^-72;
//   otherwise, and in the windows and strips on the domain's edge, it divides as mode 2 does.  Velocities
//   pass unless they have died out; a density with exact zeros outside its support falls back there.

// 5: Markstein's residual correction with the residual kept out of the underflow range by a power of two (round 3).
//   With r = RN32(1/beta) and S = 2^24:
//       q0 = D * r;   e = fma(q0, beta*S, D*(-S));   q = fma(e, -(r/S), q0)
//   -- four PACKED instructions per pair of cells where mode 2 takes six scalar ones.  e = -S*(D - q0*beta) is exact
//   (q0 is within an ulp of D/beta, so the residual has at most 24 significant bits, and the scale keeps its last bit
//   at or above 2^-148 even for denormal D: unscaled, it underflows for |D| < 2^-102 and the quotient comes out an ulp
//   off -- what DESIGN.md section 3 records of the unscaled form), and the last fma rounds q0 + (D - q0*beta)*r once,
//   which is RN(D/beta) by Markstein's theorem.  The signs are arranged so that -0 / beta = -0.  k_validate_div proves
//   it per beta for every |D| < 2^104.  Beyond that D*S overflows -- and then e, and q, are inf or NaN, never a finite
//   wrong number; every later sweep turns anything it computes from a non-finite value into a non-finite value, down
//   to the rows the wave stores.  So the wave keeps ONE sticky test on what it stores (fma(value, 0, acc): NaN as soon
//   as a value is inf or NaN), one packed instruction per time step, and a wave that stored anything non-finite runs
//   its strip again in mode 2 (stores are out of place, so a second pass simply overwrites the first).  Fields that
//   hold inf or NaN to begin with take that second pass too; nothing else ever does (|D| >= 2^104 ~ 2e31).
//   Unlike mode 3 this needs no fact about the data: the tiny and denormal ranges a decaying field crosses are exact.

// One lane's share of a row: NV consecutive columns (NV = 2 or 4).
template <int NV>
struct Vec {
    float c[NV];
};
typedef float v2f __attribute__((ext_vector_type(2)));
typedef half_t half2_t __attribute__((ext_vector_type(2)));

template <int NV>
__device__ __forceinline__ Vec<NV> buf_ldv(const float*, __amdgpu_buffer_rsrc_t r, unsigned off)
{
    Vec<NV> v;
    if constexpr (NV == 4) {
        const uint4_t u = __builtin_amdgcn_raw_buffer_load_b128(r, off, 0, 0);
        v.c[0] = __uint_as_float(u.x); v.c[1] = __uint_as_float(u.y); v.c[2] = __uint_as_float(u.z); v.c[3] = __uint_as_float(u.w);
    } else {
        const uint2_t u = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
        v.c[0] = __uint_as_float(u.x); v.c[1] = __uint_as_float(u.y);
    }
    return v;
}
template <int NV>
__device__ __forceinline__ Vec<NV> buf_ldv(const half_t*, __amdgpu_buffer_rsrc_t r, unsigned off)
{
    Vec<NV> v;
    if constexpr (NV == 4) {
        const uint2_t u = __builtin_amdgcn_raw_buffer_load_b64(r, off, 0, 0);
        half4_t h;
        __builtin_memcpy(&h, &u, 8);
        v.c[0] = keep_f32((float)h.x); v.c[1] = keep_f32((float)h.y); v.c[2] = keep_f32((float)h.z); v.c[3] = keep_f32((float)h.w);
    } else {
        const unsigned u = __builtin_amdgcn_raw_buffer_load_b32(r, off, 0, 0);
        half2_t h;
        __builtin_memcpy(&h, &u, 4);
        v.c[0] = keep_f32((float)h.x); v.c[1] = keep_f32((float)h.y);
    }
    return v;
}
template <int NV>
__device__ __forceinline__ void buf_stv(float*, __amdgpu_buffer_rsrc_t r, unsigned off, const Vec<NV>& v)
{
    if constexpr (NV == 4) {
        uint4_t u;
        u.x = __float_as_uint(v.c[0]); u.y = __float_as_uint(v.c[1]); u.z = __float_as_uint(v.c[2]); u.w = __float_as_uint(v.c[3]);
        __builtin_amdgcn_raw_buffer_store_b128(u, r, off, 0, 0);
    } else {
        uint2_t u;
        u.x = __float_as_uint(v.c[0]); u.y = __float_as_uint(v.c[1]);
        __builtin_amdgcn_raw_buffer_store_b64(u, r, off, 0, 0);
    }
}
template <int NV>
__device__ __forceinline__ void buf_stv(half_t*, __amdgpu_buffer_rsrc_t r, unsigned off, const Vec<NV>& v)
{
    if constexpr (NV == 4) {
        half4_t h;
        h.x = (half_t)keep_f32(v.c[0]); h.y = (half_t)keep_f32(v.c[1]); h.z = (half_t)keep_f32(v.c[2]); h.w = (half_t)keep_f32(v.c[3]);
        uint2_t u;
        __builtin_memcpy(&u, &h, 8);
        __builtin_amdgcn_raw_buffer_store_b64(u, r, off, 0, 0);
    } else {
        half2_t h;
        h.x = (half_t)keep_f32(v.c[0]); h.y = (half_t)keep_f32(v.c[1]);
        unsigned u;
        __builtin_memcpy(&u, &h, 4);
        __builtin_amdgcn_raw_buffer_store_b32(u, r, off, 0, 0);
    }
}

// the per-solve constants of the division (DIVMODE above): what each mode reads
struct DivK {
    float beta;           // 0: beta; 4: the exact reciprocal; 5: r = RN32(1/beta); 2, 3: unused
    double yd;            // 2 (and 3's fallback): RN64(1/beta)
    float hi, lo;         // 3: hi = RD32(1/beta), lo = RN32(1/beta - hi); 5: hi = beta * 2^24, lo = -(r * 2^-24)
};
constexpr float kDiv5NegScale = -0x1p24f;

template <typename S, int NV>
struct TbArgs {
    const S* xc;          // x   + column offset of this lane
    const S* rc;          // x0  + column offset
    S* oc;                // out + column offset
    __amdgpu_buffer_rsrc_t bx, br, bo;   // the three fields as range-checked buffers
    unsigned ld_off;      // byte offset of this lane's vector in row 0 (kBufOff: lane loads nothing)
    unsigned st_off;      // same for the store (kBufOff unless the lane owns interior or ghost columns)
    unsigned row_bytes;
    unsigned m_lg;        // all ones in the lane whose last component is ghost column 0, else 0
    unsigned m_r[NV];     // all ones in the lane AND component that is ghost column n+1
    int n, q_lo, q_hi, cg;
    float alpha;
    DivK k;               // the division's constants
    S* dc;                // DIVSRC: the divergence field + column offset, its buffer, and -0.5f * h
    __amdgpu_buffer_rsrc_t bd;   // (ADDSRC: the field that receives x0 + dt * source, and dt in div_scale)
    float div_scale;
    int s_lo, s_hi;       // ADDSRC: rows of it this wave stores (its strip, plus the wall row next to it)
    unsigned sx, sy;      // sign masks: flip across vertical / horizontal walls
    float x0_inc;         // pending add_source increment of the right-hand side (-0.0f: none)
    bool st_rg_lane, is_lg;
    bool fill;            // skip the stage evaluations of the pipeline fill and drain that nothing reads (tb_march)
};

__device__ __forceinline__ float fxor(float v, unsigned m) { return __uint_as_float(__float_as_uint(v) ^ m); }
template <int NV>
__device__ __forceinline__ Vec<NV> fxorv(const Vec<NV>& v, unsigned m)
{
    Vec<NV> o;
#pragma unroll
    for (int c = 0; c < NV; ++c) o.c[c] = fxor(v.c[c], m);
    return o;
}

// (r + alpha*nb) / beta for one cell (the validator) and for a pair of cells (the kernel; same
// operations, the compiler emits the packed form of each).
template <int DIVMODE>
__device__ __forceinline__ float tb_div(float num, const DivK& k)
{
    if (DIVMODE == 0) return num / k.beta;
    if (DIVMODE == 4) return num * k.beta;         // beta holds the exact reciprocal
    if (DIVMODE == 3) return __builtin_fmaf(num, k.hi, num * k.lo);
    if (DIVMODE == 5) {
        const float q0 = num * k.beta;
        const float e = __builtin_fmaf(q0, k.hi, num * kDiv5NegScale);
        return __builtin_fmaf(e, k.lo, q0);
    }
    return (float)((double)num * k.yd);
}
template <int DIVMODE>
__device__ __forceinline__ v2f tb_div2(v2f num, const DivK& k)
{
    if constexpr (DIVMODE == 4) return num * k.beta;
    else if constexpr (DIVMODE == 3) {             // v_pk_mul_f32 + v_pk_fma_f32 (four plain v_mul / v_fmac: measured no better)
        const v2f p = num * k.lo;
        return __builtin_elementwise_fma(num, (v2f){k.hi, k.hi}, p);
    } else if constexpr (DIVMODE == 5) {           // 2 x v_pk_mul_f32 + 2 x v_pk_fma_f32
        const v2f ds = num * kDiv5NegScale;
        const v2f q0 = num * k.beta;
        const v2f e = __builtin_elementwise_fma(q0, (v2f){k.hi, k.hi}, ds);
        return __builtin_elementwise_fma(e, (v2f){k.lo, k.lo}, q0);
    } else return (v2f){tb_div<DIVMODE>(num.x, k), tb_div<DIVMODE>(num.y, k)};
}

// One lane's vector of one stage.  Its columns are worked on in pairs (0,1), (2,3), which is how every
// row already sits in registers (a load fills aligned registers, each result is written as aligned
// pairs): the horizontal sum l+r is one scalar add per column -- the two at the ends of the vector
// reach into the neighbouring lane through DPP -- whose results land in adjacent registers, and
// everything after it is one packed instruction per pair (v_pk_add_f32 x3, v_pk_mul_f32 x1..2).
// 3 to 3.5 VALU instructions per cell instead of 6.5: a wave issues about one instruction per 4.6
// cycles whatever its kind (tools/ubench/valu_cost.hip), so instructions are what to save.
// Operand order and roundings are those of FluidSequential.c:93-94.
template <int DIVMODE, int NV>
__device__ __forceinline__ Vec<NV> tb_stencil(const Vec<NV>& up, const Vec<NV>& me, const Vec<NV>& dn, const Vec<NV>& r,
                                              float alpha, const DivK& k)
{
    float h[NV];
    h[0] = lane_below0(me.c[NV - 1]) + me.c[1];
#pragma unroll
    for (int c = 1; c < NV - 1; ++c) h[c] = me.c[c - 1] + me.c[c + 1];
    h[NV - 1] = me.c[NV - 2] + lane_above0(me.c[0]);
    Vec<NV> G;
#pragma unroll
    for (int p = 0; p < NV; p += 2) {
        v2f s = {h[p], h[p + 1]};
        s = s + (v2f){up.c[p], up.c[p + 1]};
        s = s + (v2f){dn.c[p], dn.c[p + 1]};
        if constexpr (DIVMODE != 4) s = s * alpha;       // mode 4: alpha == 1.0f, x * 1.0f is x
        s = (v2f){r.c[p], r.c[p + 1]} + s;
        s = tb_div2<DIVMODE>(s, k);
        G.c[p] = s.x;
        G.c[p + 1] = s.y;
    }
    return G;
}

// All 2^32 float bit patterns a: does tb_div<DIVMODE>(a) equal a / beta bit for bit
// (any NaN matches any NaN)?  Counts mismatches; the solver requires zero.
// Mode 3 (arg = hi): its fallback, mode 2, must be exact for every a, and the two-term quotient for every a
// that is zero or at least beta * 2^-98 in magnitude (the dividends the tile test lets through are zero or
// at least beta * 2^-97, see DIVMODE 3).
// Mode 5: exact for every a that the quotient of is finite ... or else NOT FINITE (inf / NaN, which the wave's sticky test
// on its stored rows catches, see DIVMODE 5) -- never a finite value that differs from a / beta.  In practice: exact for
// |a| < 2^104, non-finite beyond.
template <int DIVMODE>
__global__ __launch_bounds__(256) void k_validate_div(float beta, DivK k, unsigned long long* __restrict__ bad)
{
    unsigned long long n = 0;
    const unsigned long long stride = (unsigned long long)gridDim.x * 256;
    auto differs = [](float got, float ref) { return (ref != ref) ? !(got != got) : (__float_as_uint(got) != __float_as_uint(ref)); };
    DivK k2 = k;
    for (unsigned long long i = (unsigned long long)blockIdx.x * 256 + threadIdx.x; i < (1ull << 32); i += stride) {
        const float a = __uint_as_float((unsigned)i);
        const float ref = a / beta;
        if constexpr (DIVMODE == 3) {
            const bool in_range = a == 0.0f || !(__builtin_fabsf(a) < beta * 0x1p-98f);
            n += differs(tb_div<2>(a, k2), ref) || (in_range && differs(tb_div<3>(a, k), ref));
        } else if constexpr (DIVMODE == 5) {
            const float got = tb_div<5>(a, k);
            const bool finite = __builtin_fabsf(got) < __builtin_inff();
            const bool must_be_exact = __builtin_fabsf(a) < 0x1p100f;       // (the claim is 2^104; what matters is: far beyond any field)
            n += differs(got, ref) && (finite || must_be_exact);
        } else {
            n += differs(tb_div<DIVMODE>(a, k), ref);
        }
    }
    if (n) atomicAdd(bad, n);
}

// ghost columns of one freshly computed row (set_bnd, FluidSequential.c:65-66), edge windows only.
// Branch-free: per-lane bit masks pick the one lane/component that is a ghost column and replace it
// by its (sign-flipped) interior neighbour; every other lane and component passes through unchanged.
// (Uniform branches here cost an edge-window wave ~2.7x an interior wave per step and made the two
// edge windows the tail of every launch.)  v1 / vn return column 1 / column n of the row, which the
// final stage needs for the corner cells.
__device__ __forceinline__ float bitsel(unsigned mask, float a, float b)      // mask ? a : b, per bit
{
    return __uint_as_float((__float_as_uint(a) & mask) | (__float_as_uint(b) & ~mask));
}

template <typename S, int NV>
__device__ __forceinline__ void tb_fix_columns(Vec<NV>& G, const TbArgs<S, NV>& a, float& v1, float& vn, bool need_corners)
{
    float o[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) o[c] = G.c[c];
    const float from_right = lane_above0(o[0]);          // column 1 as seen from the lane holding column 0
    const float from_left = lane_below0(o[NV - 1]);      // column n as seen from the next lane (n % NV == 0)
    G.c[0] = bitsel(a.m_r[0], fxor(from_left, a.sx), o[0]);
#pragma unroll
    for (int c = 1; c < NV - 1; ++c) G.c[c] = bitsel(a.m_r[c], fxor(o[c - 1], a.sx), o[c]);
    G.c[NV - 1] = bitsel(a.m_lg, fxor(from_right, a.sx), bitsel(a.m_r[NV - 1], fxor(o[NV - 2], a.sx), o[NV - 1]));
    if (need_corners) {          // folds to a constant once the stage loop is unrolled
        v1 = from_right;
        unsigned bits = __float_as_uint(from_left) & a.m_r[0];
#pragma unroll
        for (int c = 1; c < NV; ++c) bits |= __float_as_uint(o[c - 1]) & a.m_r[c];
        vn = __uint_as_float(bits);
    }
}

// final stage: store row q, its ghost columns, and ghost rows / corners -- WITHOUT branches.
// Every lane that holds anything to be stored writes its whole vector through the range-checked
// buffer: the ragged last vector and the two ghost-column lanes spill their surplus components
// into pad floats (never read as data), so edge windows issue the same single store per step as
// interior ones; wall strips add the two ghost rows, enabled by a select on the offset.  A fixed
// number of memory operations per step is what lets hipcc count them (see kBufOff).
template <bool EDGE, bool WALL, typename S, int NV>
__device__ __forceinline__ void tb_store_to(S* oc, __amdgpu_buffer_rsrc_t bo, const Vec<NV>& G, int q, bool mine, const TbArgs<S, NV>& a,
                                            float v1, float vn)
{
    auto on = [](bool c, unsigned off) { return c ? off : kBufOff; };
    buf_stv<NV>(oc, bo, on(mine, a.st_off) + (unsigned)q * a.row_bytes, G);
    if (WALL) {
        Vec<NV> g = fxorv<NV>(G, a.sy);                  // ghost row = flipped wall row ...
        if (EDGE) {                                      // ... except its two corner cells
            const float cl = 0.5f * (fxor(v1, a.sy) + fxor(v1, a.sx));
            const float cr = 0.5f * (fxor(vn, a.sy) + fxor(vn, a.sx));
            if (a.is_lg) g.c[NV - 1] = cl;
#pragma unroll
            for (int c = 0; c < NV; ++c)
                if (a.st_rg_lane && a.cg == c) g.c[c] = cr;
        }
        buf_stv<NV>(oc, bo, on(mine & (q == 1), a.st_off), g);                                        // row 0
        buf_stv<NV>(oc, bo, on(mine & (q == a.n), a.st_off) + (unsigned)(a.n + 1) * a.row_bytes, g);  // row n+1
    }
}
template <bool EDGE, bool WALL, typename S, int NV>
__device__ __forceinline__ void tb_store(const Vec<NV>& G, int q, bool mine, const TbArgs<S, NV>& a, float v1, float vn)
{
    tb_store_to<EDGE, WALL, S, NV>(a.oc, a.bo, G, q, mine, a, v1, vn);
}

// DIVSRC: the divergence of (u, v) on row t-1 (FluidSequential.c:151-152: (-0.5f*h) * (((uR - uL) + vD) - vU)) from the
// rows the wave holds -- u row t-1, v rows t-2 and t -- for the first launch of a pressure solve, which then needs
// no divergence kernel before it: the row becomes the launch's right-hand side and is stored for the later launches.
template <int NV>
__device__ __forceinline__ Vec<NV> tb_divergence(const Vec<NV>& u, const Vec<NV>& v_up, const Vec<NV>& v_dn, float scale)
{
    float g[NV];
#pragma unroll
    for (int c = 0; c < NV; ++c) {
        const float ur = c < NV - 1 ? u.c[c + 1] : lane_above0(u.c[0]);
        const float ul = c > 0 ? u.c[c - 1] : lane_below0(u.c[NV - 1]);
        g[c] = ur - ul;
    }
    Vec<NV> d;
#pragma unroll
    for (int p = 0; p < NV; p += 2) {
        v2f s = {g[p], g[p + 1]};
        s = s + (v2f){v_dn.c[p], v_dn.c[p + 1]};
        s = s - (v2f){v_up.c[p], v_up.c[p + 1]};
        s = s * scale;
        d.c[p] = s.x;
        d.c[p + 1] = s.y;
    }
    return d;
}

// the hand-over of a prefetched row into the pipeline, as register moves the compiler cannot see
// through (tb_step says why)
template <int NV>
__device__ __forceinline__ Vec<NV> take(const Vec<NV>& v)
{
    Vec<NV> o;
#pragma unroll
    for (int p = 0; p < NV; p += 2) {
        v2f in = {v.c[p], v.c[p + 1]}, out;
        asm("v_mov_b64 %0, %1" : "=v"(out) : "v"(in));
        o.c[p] = out.x;
        o.c[p + 1] = out.y;
    }
    return o;
}

// x0 queue shift as straight-line code (a loop here is recognised as memmove,
// which pins the whole queue in scratch memory).
template <int K, int N, int NV>
__device__ __forceinline__ void tb_qshift(Vec<NV> (&Q)[N])
{
    if constexpr (K >= 1) {
        Q[K] = Q[K - 1];
        tb_qshift<K - 1, N, NV>(Q);
    }
}

// DIVMODE 5's sticky test on a row of the last stage: nf turns NaN -- and stays NaN -- once a value is inf or NaN
// (x * 0 is +-0 for every finite x).  One packed instruction per pair and time step.
template <int DIVMODE, int NV>
__device__ __forceinline__ void tb_sticky(const Vec<NV>& G, v2f& nf)
{
    if constexpr (DIVMODE == 5) {
#pragma unroll
        for (int p = 0; p < NV; p += 2) nf = __builtin_elementwise_fma((v2f){G.c[p], G.c[p + 1]}, (v2f){0.f, 0.f}, nf);
    }
}

// One time step.  Ring s (s = 0..T-1) holds three consecutive rows of "x after
// s sweeps"; at phase PH its slots are up = PH, me = PH+1, fresh = PH+2 (mod 3).
// GEN = false: every row any stage touches at this step is interior -- a
// branch-free body.  GEN = true (the few steps of a wall strip that sit on rows
// 0 / n+1): per-stage checks, ghost rows of each stage regenerated from its rows 1 / n.
// PART (interior body only): stages 1 .. smax run and the rest are skipped -- a wave-uniform branch per stage.  A skipped
// stage stores nothing and leaves its ring slot undefined: only evaluations that are skipped as well read it (tb_march).
template <int T, int DIVMODE, bool EDGE, bool WALL, bool GEN, int PH, typename S, int NV, bool DIVSRC = false, bool ADDSRC = false,
          bool PART = false>
__device__ __forceinline__ void tb_step(int t, Vec<NV> (&W)[T][3], Vec<NV> (&Q)[T + 1], Vec<NV> (&PX)[3], Vec<NV> (&PQ)[3],
                                        const TbArgs<S, NV>& a, Vec<NV> (&UR)[3], Vec<NV> (&VR)[3], v2f& nf, int smax = T)
{
    static_assert(!(PART && GEN), "the general body runs every stage");
    constexpr int UP = PH % 3, ME = (PH + 1) % 3, FR = (PH + 2) % 3;
    // stage 0: row t of x and x0, loaded three steps ago.  The hand-over is an opaque register move on
    // purpose: a plain assignment lets the allocator rename the prefetch slot into the ring and pay
    // for it with copies at the loop's back edge -- copies of rows still in flight, i.e. a wait for
    // every outstanding load once per iteration.
    __builtin_amdgcn_sched_barrier(0);                   // (and not hoisted into the previous step either)
    if constexpr (DIVSRC) {
        // the two prefetch slots carry u and v (the first guess is all +0 and is not read): rings of their last three rows
        UR[FR] = take<NV>(PX[PH]);
        VR[FR] = take<NV>(PQ[PH]);
    } else {
        W[0][FR] = take<NV>(PX[PH]);
        Q[0] = take<NV>(PQ[PH]);
        if constexpr (ADDSRC) {
            // add_source inside the solve's first launch (FluidSequential.c:78-82 with the SWAP of :181 / :201 / :209 behind
            // it): the first guess x IS the source field s and the right-hand side is x0 + dt * s -- formed here row by row,
            // in the reference's order (the product rounded, then the sum), handed to the stages and stored OUT OF PLACE for
            // the solve's later launches (neighbouring waves still read the raw rows of x0, so it cannot go back in place;
            // the solver swaps the two buffers afterwards).  Ghost cells included, as add_source touches every cell.
#pragma unroll
            for (int p = 0; p < NV; p += 2) {
                const v2f ds = (v2f){W[0][FR].c[p], W[0][FR].c[p + 1]} * a.div_scale;
                const v2f q = (v2f){Q[0].c[p], Q[0].c[p + 1]} + ds;
                Q[0].c[p] = as_stored<S>(q.x);           // fp16 storage: what a separate add_source pass would hand on
                Q[0].c[p + 1] = as_stored<S>(q.y);
            }
            buf_stv<NV>(a.dc, a.bd, (((t >= a.s_lo) & (t < a.s_hi)) ? a.st_off : kBufOff) + (unsigned)t * a.row_bytes, Q[0]);
        } else {
#pragma unroll
            for (int p = 0; p < NV; p += 2) {            // x0 + dt*0 where an add_source was deferred, else x0 + (-0) = x0
                const v2f q = (v2f){Q[0].c[p], Q[0].c[p + 1]} + a.x0_inc;
                Q[0].c[p] = q.x;
                Q[0].c[p + 1] = q.y;
            }
        }
    }
    {   // refill the slot with row t+3: three steps of arithmetic cover the memory latency.  Rows past
        // the field's end and lanes past its width fall outside the buffer and read as 0.
        const unsigned off = a.ld_off + (unsigned)(t + 3) * a.row_bytes;
        PX[PH] = buf_ldv<NV>(a.xc, a.bx, off);
        PQ[PH] = buf_ldv<NV>(a.rc, a.br, off);
    }
    // the loads must ISSUE here, three steps before their use: left to itself the scheduler sinks
    // them to the end of the unrolled iteration (shorter live ranges) and the wave then waits out a
    // full memory latency per iteration
    __builtin_amdgcn_sched_barrier(0);
    if constexpr (DIVSRC) {
        // right-hand side row t-1 = divergence there; it is what stage 1 consumes at this step (Q[1]), and it is stored
        // (with the ghost cells set_bnd(0, div) would give it) for the solve's later launches and as the step's v_prev
        const int q = t - 1;
        Vec<NV> D = tb_divergence<NV>(UR[ME], VR[UP], VR[FR], a.div_scale);
#pragma unroll
        for (int c = 0; c < NV; ++c) D.c[c] = as_stored<S>(D.c[c]);     // fp16 storage: what a separate divergence pass would hand on
        Q[1] = D;
        float v1 = 0.f, vn = 0.f;
        if (EDGE) tb_fix_columns<S, NV>(D, a, v1, vn, WALL);
        tb_store_to<EDGE, (WALL || GEN), S, NV>(a.dc, a.bd, D, q, (q >= 1) & (q <= a.n) & (q >= a.q_lo) & (q < a.q_hi), a, v1, vn);
    }
    if constexpr (!GEN) {
#pragma unroll
        for (int s = 1; s <= T; ++s) {
            // PART: the stage's arithmetic behind a scalar branch; its ring write and store are not (a skipped stage writes
            // an undefined row, which costs nothing, and stores through a disabled offset), so that every step issues the
            // same memory operations outside any branch and the loop after the partial steps keeps waiting for each row
            // three steps after its load (hipcc counts the operations in flight per path: see the prologue of tb_march)
            const bool run = !PART || s <= smax;
            const int q = t - s;                         // row this stage produces now (wave-uniform)
            Vec<NV> G;
            float v1 = 0.f, vn = 0.f;
            if (run) {
                G = tb_stencil<DIVMODE, NV>(W[s - 1][UP], W[s - 1][ME], W[s - 1][FR], Q[s], a.alpha, a.k);
                if (EDGE) tb_fix_columns<S, NV>(G, a, v1, vn, WALL && s == T);
                if (s == T) tb_sticky<DIVMODE, NV>(G, nf);
            } else {
#pragma unroll
                for (int c = 0; c < NV; ++c) G.c[c] = __builtin_nondeterministic_value(W[s - 1][FR].c[c]);
            }
            if (s < T) W[s][FR] = G;
            else tb_store<EDGE, WALL, S, NV>(G, q, run & (q >= a.q_lo) & (q < a.q_hi), a, v1, vn);
        }
    } else {
        // ring writes stay unconditional (selected values), so the rings stay in registers
#pragma unroll
        for (int s = 1; s <= T; ++s) {
            const int q = t - s;
            const bool interior = (q >= 1 && q <= a.n);
            Vec<NV> G = tb_stencil<DIVMODE, NV>(W[s - 1][UP], W[s - 1][ME], W[s - 1][FR], Q[s], a.alpha, a.k);
            float v1 = 0.f, vn = 0.f;
            if (EDGE) tb_fix_columns<S, NV>(G, a, v1, vn, s == T);
            if (s < T) {
                const Vec<NV> me = W[s][ME];
                const Vec<NV> flipped_me = fxorv<NV>(me, a.sy);  // ghost row n+1 of this stage = flipped row n
                const Vec<NV> flipped_g = fxorv<NV>(G, a.sy);    // ghost row 0 of this stage = flipped row 1
                const bool bot_ghost = (q == a.n + 1), top_ghost = (q == 1);
#pragma unroll
                for (int c = 0; c < NV; ++c) {
                    W[s][FR].c[c] = bot_ghost ? flipped_me.c[c] : G.c[c];
                    W[s][ME].c[c] = top_ghost ? flipped_g.c[c] : me.c[c];
                }
            } else {
                tb_sticky<DIVMODE, NV>(G, nf);
                tb_store<EDGE, true, S, NV>(G, q, interior & (q >= a.q_lo) & (q < a.q_hi), a, v1, vn);
            }
        }
    }
    tb_qshift<T, T + 1, NV>(Q);
}

// returns (wave-uniform): did the last stage produce anything that is not finite (DIVMODE 5 only; false otherwise)
template <int T, int DIVMODE, bool EDGE, bool WALL, typename S, int NV, bool DIVSRC = false, bool ADDSRC = false>
__device__ __forceinline__ bool tb_march(int t0, int t1, const TbArgs<S, NV>& a)
{
    Vec<NV> W[T][3], Q[T + 1], PX[3], PQ[3], UR[3], VR[3];
    v2f nf = {0.f, 0.f};
    Vec<NV> zero;
#pragma unroll
    for (int c = 0; c < NV; ++c) zero.c[c] = 0.f;
#pragma unroll
    for (int s = 0; s < T; ++s) { W[s][0] = zero; W[s][1] = zero; W[s][2] = zero; }
#pragma unroll
    for (int s = 0; s <= T; ++s) Q[s] = zero;
#pragma unroll
    for (int d = 0; d < 3; ++d) { UR[d] = zero; VR[d] = zero; }
#pragma unroll
    for (int d = 0; d < 3; ++d) {                        // rows t0, t0+1, t0+2 in flight before the first step
        const unsigned off = a.ld_off + (unsigned)(t0 + d) * a.row_bytes;
        PX[d] = buf_ldv<NV>(a.xc, a.bx, off);
        PQ[d] = buf_ldv<NV>(a.rc, a.br, off);
        // a store that stores nothing (offset out of range): the loop is entered with the same
        // load, load, store sequence in flight that one of its iterations leaves behind, so the wait
        // for a row at the top of the loop counts 7 younger operations on both paths into it instead
        // of draining the queue
        buf_stv<NV>(a.oc, a.bo, kBufOff, zero);
        if constexpr (DIVSRC || ADDSRC) buf_stv<NV>(a.dc, a.bd, kBufOff, zero);      // (a step of these variants stores a second row)
        __builtin_amdgcn_sched_barrier(0);               // in this order
    }
    // whole triples only: up to two surplus steps load nothing (rows past the field) and store nothing
    // (q >= q_hi).  A step is "interior" when the rows its stages produce, t-T .. t-1, all lie in 1..n
    // and no stage below the last is on row 1 (whose ghost row it would have to regenerate):
    // T+1 <= t <= n+1.  Wall strips run the general body only for the triples that contain another
    // kind of step -- about T/3 of them per wall -- as three loops, so neither body pays for the
    // other's registers.
    // Pipeline fill (a.fill): stage s at step t produces row t-s from rows t-s-1 .. t-s+1 of stage s-1.  When the strip's
    // top is not the wall (t0 = q_lo-T), stage 0 holds rows t0 .. only, so stage s is right from row t0+s on, which it
    // produces at step t0+2s; what it produces before that feeds only earlier evaluations of the later stages, and
    // through them rows of stage T above q_lo, which are not stored.  So the first ceil(2T/3) triples run stages
    // 1 .. (t-t0)/2 only: T(T+1) of a strip's T(rb+2T) stage evaluations.  The same way the steps of the last triple
    // past t1 run none.  Both are partial steps of the interior body; the general one always runs every stage.
    int t = t0;
    if constexpr (WALL) {
        for (; t <= t1 && t < T + 1; t += 3) {
            tb_step<T, DIVMODE, EDGE, WALL, true, 0, S, NV, DIVSRC, ADDSRC>(t, W, Q, PX, PQ, a, UR, VR, nf);
            tb_step<T, DIVMODE, EDGE, WALL, true, 1, S, NV, DIVSRC, ADDSRC>(t + 1, W, Q, PX, PQ, a, UR, VR, nf);
            tb_step<T, DIVMODE, EDGE, WALL, true, 2, S, NV, DIVSRC, ADDSRC>(t + 2, W, Q, PX, PQ, a, UR, VR, nf);
        }
    }
    const int fill_end = (a.fill && t0 == a.q_lo - T) ? t0 + 3 * ((2 * T + 2) / 3) : t0;   // partial steps before it
    const int full_end = a.fill ? t1 - 2 : t1;           // ... and in triples that start after it
    auto stages = [&](int u) { return u > t1 ? 0 : u < fill_end ? (u - t0) >> 1 : T; };
    for (; t <= t1 && t < fill_end && (!WALL || t + 1 <= a.n); t += 3) {
        tb_step<T, DIVMODE, EDGE, WALL, false, 0, S, NV, DIVSRC, ADDSRC, true>(t, W, Q, PX, PQ, a, UR, VR, nf, stages(t));
        tb_step<T, DIVMODE, EDGE, WALL, false, 1, S, NV, DIVSRC, ADDSRC, true>(t + 1, W, Q, PX, PQ, a, UR, VR, nf, stages(t + 1));
        tb_step<T, DIVMODE, EDGE, WALL, false, 2, S, NV, DIVSRC, ADDSRC, true>(t + 2, W, Q, PX, PQ, a, UR, VR, nf, stages(t + 2));
    }
    for (; t <= full_end && (!WALL || t + 1 <= a.n); t += 3) {
        tb_step<T, DIVMODE, EDGE, WALL, false, 0, S, NV, DIVSRC, ADDSRC>(t, W, Q, PX, PQ, a, UR, VR, nf);
        tb_step<T, DIVMODE, EDGE, WALL, false, 1, S, NV, DIVSRC, ADDSRC>(t + 1, W, Q, PX, PQ, a, UR, VR, nf);
        tb_step<T, DIVMODE, EDGE, WALL, false, 2, S, NV, DIVSRC, ADDSRC>(t + 2, W, Q, PX, PQ, a, UR, VR, nf);
    }
    for (; t <= t1 && (!WALL || t + 1 <= a.n); t += 3) {
        tb_step<T, DIVMODE, EDGE, WALL, false, 0, S, NV, DIVSRC, ADDSRC, true>(t, W, Q, PX, PQ, a, UR, VR, nf, stages(t));
        tb_step<T, DIVMODE, EDGE, WALL, false, 1, S, NV, DIVSRC, ADDSRC, true>(t + 1, W, Q, PX, PQ, a, UR, VR, nf, stages(t + 1));
        tb_step<T, DIVMODE, EDGE, WALL, false, 2, S, NV, DIVSRC, ADDSRC, true>(t + 2, W, Q, PX, PQ, a, UR, VR, nf, stages(t + 2));
    }
    if constexpr (WALL) {
        for (; t <= t1; t += 3) {
            tb_step<T, DIVMODE, EDGE, WALL, true, 0, S, NV, DIVSRC, ADDSRC>(t, W, Q, PX, PQ, a, UR, VR, nf);
            tb_step<T, DIVMODE, EDGE, WALL, true, 1, S, NV, DIVSRC, ADDSRC>(t + 1, W, Q, PX, PQ, a, UR, VR, nf);
            tb_step<T, DIVMODE, EDGE, WALL, true, 2, S, NV, DIVSRC, ADDSRC>(t + 2, W, Q, PX, PQ, a, UR, VR, nf);
        }
    }
    if constexpr (DIVMODE == 5) return __builtin_amdgcn_ballot_w64((nf.x != nf.x) | (nf.y != nf.y)) != 0ull;
    else return false;
}

// the four bodies of a march: edge windows replay the ghost columns, wall strips the ghost rows (both wave-uniform)
template <int T, int DIVMODE, typename S, int NV, bool DIVSRC = false, bool ADDSRC = false>
__device__ __forceinline__ bool tb_march_any(bool edge, bool wall, int t0, int t1, const TbArgs<S, NV>& a)
{
    if (edge) {
        if (wall) return tb_march<T, DIVMODE, true, true, S, NV, DIVSRC, ADDSRC>(t0, t1, a);
        return tb_march<T, DIVMODE, true, false, S, NV, DIVSRC, ADDSRC>(t0, t1, a);
    }
    if (wall) return tb_march<T, DIVMODE, false, true, S, NV, DIVSRC, ADDSRC>(t0, t1, a);
    return tb_march<T, DIVMODE, false, false, S, NV, DIVSRC, ADDSRC>(t0, t1, a);
}

// which (window, strip group) pairs exist (launch_jacobi_tb)
struct TbGrid {
    int inner_wins, inner_blocks, edge_wins, edge_blocks, first_right;
    int hole_lo, hole_hi;     // rows [hole_lo, hole_hi) inside [row_lo, row_hi) are left out (hole_lo >= hole_hi: none): the two
                              // edge parts of a launch split around a halo exchange run as ONE launch (launch_jacobi_tb)
};

// waves per SIMD the register allocator must leave room for (second launch-bound argument): the
// kernel hides its latencies (memory, dependent packed operations) only by running other waves
constexpr int tb_waves_per_simd(int T, int NV) { return NV == 2 ? (T <= 8 ? 4 : T <= 12 ? 3 : 2) : (T <= 4 ? 3 : 2); }

// blockIdx.z picks one of up to three independent solves of the same shape (u, v and density
// diffusion): more waves per launch, hence taller strips and less pipeline-fill redundancy -- and, in an ensemble, one
// member: z = solve + count * member.  gridDim.x is a multiple of 8, so the XCD renumbering sees the same thing in every
// z-slice.  The member's offset goes into the field pointers before the buffer descriptors are made (scalar arithmetic);
// nothing in the march knows of it.
template <int T, int DIVMODE, int NV, typename S, bool DIVSRC = false, bool ADDSRC = false>
__global__ __launch_bounds__(256, tb_waves_per_simd(T, NV)) void k_jacobi_tb(TbBatch batch, int pitch, int n, int row_lo,
                                                                             int row_hi, int rb, int rb_edge, TbGrid g, int fill)
{
    static_assert(!DIVSRC || DIVMODE == 4, "the divergence-sourced launch is the first launch of a pressure solve");
    static_assert(!(DIVSRC && ADDSRC) && (!ADDSRC || DIVMODE != 3), "one second store per launch; mode 3's tiles are taken from the summed field");
    // Workgroups are handed to the 8 XCDs round-robin by linear id, and each XCD has its own L2.  The
    // grid is one-dimensional, a multiple of 8 long, and renumbered so that XCD k works through the
    // k-th contiguous eighth of the (window, strip group) list, windows fastest: the blocks an XCD
    // runs at the same time are neighbouring windows of the same rows, and the columns they both
    // read (2*HL lanes per window, a third of the reads at T = 16) are served by that XCD's L2
    // instead of crossing the fabric twice.
    // Only blocks that have rows are enumerated: interior windows x their strip groups first, then the
    // edge windows (window 0 and the last one or two), which have more, shorter strips.
    const unsigned per_xcd = gridDim.x >> 3;
    unsigned vid = (blockIdx.x & 7u) * per_xcd + (blockIdx.x >> 3);
    if (vid >= (unsigned)(g.inner_blocks + g.edge_blocks)) return;
    int win, strip_group;
    if (vid < (unsigned)g.inner_blocks) {
        win = 1 + (int)(vid % (unsigned)g.inner_wins);
        strip_group = (int)(vid / (unsigned)g.inner_wins);
    } else {
        vid -= (unsigned)g.inner_blocks;
        const int e = (int)(vid % (unsigned)g.edge_wins);
        strip_group = (int)(vid / (unsigned)g.edge_wins);
        win = e == 0 ? 0 : g.first_right + e - 1;
    }
    // (count is 1, 2 or 3: divisions by constants, not by a run-time value)
    const unsigned member = batch.count == 3 ? blockIdx.z / 3u : batch.count == 2 ? blockIdx.z >> 1 : blockIdx.z;
    const unsigned sv = blockIdx.z - member * (unsigned)batch.count;
    const size_t mofs = (size_t)member * batch.mstride;
    const S* __restrict__ x = static_cast<const S*>(batch.x[sv]) + mofs;
    const S* __restrict__ x0 = static_cast<const S*>(batch.x0[sv]) + mofs;
    S* __restrict__ out = static_cast<S*>(batch.out[sv]) + mofs;
    // the solve's constants: the launch's own, or this member's record of the table (fluid_*_members) -- wave-uniform loads
    // either way, and nothing below this prologue knows which
    float alpha = batch.alpha[sv], beta = batch.beta[sv];
    double yd = batch.yd[sv];
    float k_hi = batch.hi[sv], k_lo = batch.lo[sv], x0_inc = batch.x0_inc[sv], div_scale = batch.div_scale;
    unsigned tile_thr = batch.tile_thr[sv];
    if (batch.mk != nullptr) {
        // (through the constant address space -- nothing on the device writes the table -- so that a wave-uniform address
        // gives scalar loads into SGPRs: a generic pointer here made the compiler select between the two ADDRESSES and
        // load per lane, eleven more VGPRs for the whole march)
        typedef const TbMemberK __attribute__((address_space(4))) * MemberKPtr;
        const MemberKPtr mk = (MemberKPtr)(uintptr_t)batch.mk + ((size_t)sv * (unsigned)batch.members + member);
        alpha = mk->alpha;
        beta = mk->beta;
        yd = mk->yd;
        k_hi = mk->hi;
        k_lo = mk->lo;
        x0_inc = mk->x0_inc;
        if (ADDSRC) div_scale = mk->div_scale;
        if (DIVMODE == 3) tile_thr = mk->tile_thr;
    }
    const int b = batch.b[sv];
    constexpr int HL = (T + NV - 1) / NV;                // lanes of overlap per side: T columns
    constexpr int VS = 64 - 2 * HL;
    constexpr int C0 = (XOFF + 1) / NV;                  // vector index of column 1 within a row
    static_assert((XOFF + 1) % NV == 0 && HL <= C0, "window overlap must fit the row's left pad");
    const int lane = threadIdx.x & 63;
    // the wave index is uniform, but anything derived from threadIdx is divergent to hipcc: readfirstlane
    // makes the strip bounds (and with them the loop control and the store conditions) scalar
    const int strip = strip_group * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    // the two windows that carry the ghost columns do extra work per stage; they get shorter strips
    // (rb_edge < rb, more of them) so that they do not finish long after everybody else
    const int kg = n / NV;                               // ghost column n+1 = component cg of vector kg
    const bool left_edge = (win == 0);                                                  // wave-uniform
    const bool right_edge = (kg >= win * VS - HL) && (kg < win * VS - HL + 64);         // wave-uniform
    const bool edge = left_edge || right_edge;
    const int rbw = edge ? rb_edge : rb;
    TbArgs<S, NV> a;
    a.k.yd = yd;
    a.k.lo = k_lo;
    a.k.hi = k_hi;
    a.x0_inc = x0_inc;
    int seg_hi = row_hi;                                 // this wave's output rows [q_lo, q_hi): strips do not straddle the hole
    a.q_lo = row_lo + strip * rbw;
    if (g.hole_lo < g.hole_hi) {
        const int top = (g.hole_lo - row_lo + rbw - 1) / rbw;      // strips above the hole
        if (strip < top) seg_hi = g.hole_lo;
        else a.q_lo = g.hole_hi + (strip - top) * rbw;
    }
    if (a.q_lo >= seg_hi) return;                        // wave-uniform
    a.q_hi = min(a.q_lo + rbw, seg_hi);
    a.s_lo = a.q_lo == 1 ? 0 : a.q_lo;                   // (ADDSRC) the strips next to a wall store the wall row too
    a.s_hi = a.q_hi == n + 1 ? n + 2 : a.q_hi;
    const int k = win * VS - HL + lane;                  // vector index: columns 1+NV*k .. NV+NV*k
    const int nvec = (n + NV - 1) / NV;
    const bool ld_ok = k <= pitch / NV - C0 - 1;         // the whole vector lies inside the row (k >= -HL >= -C0 always)
    const ptrdiff_t cofs = (ptrdiff_t)(XOFF + 1) + NV * (ptrdiff_t)(ld_ok ? k : 0);
    a.xc = x + cofs;
    a.rc = x0 + cofs;
    a.oc = out + cofs;
    {
        const unsigned field_bytes = (unsigned)((size_t)(n + 2) * (size_t)pitch * sizeof(S));    // < 2 GiB (launch_jacobi_tb)
        // a first guess known to be all +0 (sources after step 0, the pressure) is never read: an
        // empty descriptor makes every load of it return 0
        // (DIVSRC: x and x0 are u and v, both read; the first guess is +0 by definition and lives nowhere)
        a.bx = __builtin_amdgcn_make_buffer_rsrc(const_cast<S*>(x), 0, (batch.x_zero[sv] && !DIVSRC) ? 0u : field_bytes, 0x00020000);
        a.br = __builtin_amdgcn_make_buffer_rsrc(const_cast<S*>(x0), 0, field_bytes, 0x00020000);
        a.bo = __builtin_amdgcn_make_buffer_rsrc(out, 0, field_bytes, 0x00020000);
        S* dv = (DIVSRC || ADDSRC) ? static_cast<S*>(batch.div[sv]) + mofs : out;
        a.dc = dv + cofs;
        a.bd = __builtin_amdgcn_make_buffer_rsrc(dv, 0, field_bytes, 0x00020000);
        a.div_scale = div_scale;
        a.row_bytes = (unsigned)((size_t)pitch * sizeof(S));
        const unsigned col = (unsigned)((XOFF + 1 + NV * (ptrdiff_t)k) * (ptrdiff_t)sizeof(S));
        a.ld_off = ld_ok ? col : kBufOff;
    }
    a.n = n;
    a.cg = n % NV;
    a.is_lg = (k == -1);
    const bool is_rg = (k == kg);
    const bool own = (lane >= HL) && (lane < 64 - HL);
    const bool st_int = own && k >= 0 && k < nvec;       // stores interior columns
    a.st_rg_lane = is_rg && (own || k == nvec);          // stores ghost column n+1 (exactly one lane grid-wide)
    a.m_lg = a.is_lg ? 0xFFFFFFFFu : 0u;
#pragma unroll
    for (int c = 0; c < NV; ++c) a.m_r[c] = (is_rg && a.cg == c) ? 0xFFFFFFFFu : 0u;
    // lanes that store: owners of interior columns (the ragged last vector included), the lane whose
    // last component is ghost column 0 and the lane holding ghost column n+1; surplus components go to pads
    a.st_off = (ld_ok && (st_int || a.is_lg || a.st_rg_lane)) ? a.ld_off : kBufOff;
    a.sx = (b == 1) ? 0x80000000u : 0u;
    a.sy = (b == 2) ? 0x80000000u : 0u;
    a.alpha = alpha;
    a.k.beta = beta;
    a.fill = fill != 0;
    const int t0 = max(0, a.q_lo - T), t1 = a.q_hi - 1 + T;
    // a strip whose input rows [q_lo-T, q_hi-1+T] all exist never needs a regenerated ghost row
    const bool wall = (a.q_lo < T) || (a.q_hi - 1 + T > n + 1);      // wave-uniform
    constexpr int DM = DIVMODE == 3 ? 2 : DIVMODE;                   // what mode 3 falls back to
    bool two_term = false;
    if constexpr (DIVMODE == 3) {
        // the two-term division if |x0| >= thr on every tile that this wave's part of the grid touches (DIVMODE 3
        // above): the x0 rows q_lo-T+1 .. q_hi+T-2 are the ones that reach a cell this wave stores, the columns are
        // those of its 64 * NV lanes; both clipped to the interior (ghost cells repeat interior values, and what
        // lanes past the row's ends compute is never stored)
        // this member's own minima: a wave never takes the two-term path on the strength of another member's
        const unsigned* __restrict__ tiles = batch.tiles[sv] ? batch.tiles[sv] + (size_t)member * batch.tile_mstride : nullptr;
        const unsigned thr = tile_thr;
        const int tr0 = (max(1, a.q_lo - T + 1) - 1) / kTileRows, tr1 = (min(n, a.q_hi + T - 2) - 1) / kTileRows;
        const int c0 = max(1, 1 + NV * (win * VS - HL)), c1 = min(n, NV * (win * VS - HL + 64));
        const int tc0 = (c0 - 1) / kTileCols, tc1 = (c1 - 1) / kTileCols, ntc = tc1 - tc0 + 1;
        const int count = (tr1 - tr0 + 1) * ntc;
        bool low = false;
        if (tiles != nullptr)
            for (int i = lane; i < count; i += 64)
                low |= tiles[(size_t)(tr0 + i / ntc) * batch.tile_pitch + (tc0 + i % ntc)] < thr;
        two_term = tiles != nullptr && __builtin_amdgcn_ballot_w64(low) == 0ull;
    }
    if (two_term) {
        tb_march_any<T, DIVMODE, S, NV>(edge, wall, t0, t1, a);
    } else {
        const bool again = tb_march_any<T, DM, S, NV, DIVSRC, ADDSRC>(edge, wall, t0, t1, a);
        // mode 5: something this wave stored is inf or NaN -- a dividend beyond 2^104, or a field that holds such values
        // to begin with.  The strip once more, dividing as mode 2 does; its stores replace the first pass's.
        if constexpr (DIVMODE == 5) {
            if (again) tb_march_any<T, 2, S, NV, false, ADDSRC>(edge, wall, t0, t1, a);
        }
    }
}

// |x0| minima over tiles of kTileRows x kTileCols interior cells (tile (r, c): rows 1 + r*kTileRows ..., columns
// 1 + c*kTileCols ...), as the bit pattern of a non-negative float (they order like unsigned integers), over the
// rows [row_lo, row_hi) only.  One wave per 32 rows x 256 columns: 16 lanes x 4 columns make one tile.
template <typename S>
__global__ __launch_bounds__(256) void k_tile_min_abs(TileBatch tb, int pitch, int n, int row_lo, int row_hi, int tile_row0, int tile_pitch)
{
    const unsigned member = blockIdx.z / (unsigned)tb.count, sv = blockIdx.z - member * (unsigned)tb.count;
    const S* __restrict__ f = static_cast<const S*>(tb.field[sv]) + (size_t)member * tb.mstride;
    unsigned* __restrict__ out = tb.tiles[sv] + (size_t)member * tb.tile_mstride;
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int tr = tile_row0 + blockIdx.y;
    const int j = 1 + 4 * (lane + 64 * (blockIdx.x * 4 + wave));         // first of this lane's four columns
    const int i0 = max(row_lo, 1 + tr * kTileRows), i1 = min(row_hi, 1 + (tr + 1) * kTileRows);   // 1 <= row_lo, row_hi <= n+1
    const size_t P = (size_t)pitch;
    float m = __builtin_inff();
    if (j <= n)
        for (int i = i0; i < i1; ++i) {
            const float4 v = ld4(f + (size_t)i * P + XOFF + j);           // columns past n read ghost / pad floats: masked below
            m = fminf(m, fabsf(v.x));
            if (j + 1 <= n) m = fminf(m, fabsf(v.y));
            if (j + 2 <= n) m = fminf(m, fabsf(v.z));
            if (j + 3 <= n) m = fminf(m, fabsf(v.w));
        }
    // fminf drops NaNs: a NaN in x0 makes every dividend it enters NaN, which any division mode returns as NaN
#pragma unroll
    for (int off = 8; off > 0; off >>= 1) m = fminf(m, __shfl_xor(m, off, 16));
    // (the 16 lanes of a tile agree on i0 < i1; lane 0 of the group holds the tile's first column)
    // A tile only partly inside [row_lo, row_hi) (a slab's ghost zone ends inside it) reads 0 = "divide the long way": rows
    // of it that become valid later -- an exchange inside the solve -- were never looked at, and a wave working on them must
    // not take the two-term path on the strength of the rows that were.
    const bool whole = row_lo <= 1 + tr * kTileRows && row_hi >= min(n + 1, 1 + (tr + 1) * kTileRows);
    if ((lane & 15) == 0 && j <= n) out[(size_t)tr * tile_pitch + (j - 1) / kTileCols] = whole ? __float_as_uint(m) : 0u;
}

// ---------------------------------------------------------------------------
// a5  advect (FluidSequential.c:107-141): the velocity streams in coalesced, the
// four bilinear taps of d0 per cell are gathered (served by L2 / Infinity Cache).
// ---------------------------------------------------------------------------
// What bounds these kernels is the gather, not HBM: a wave-wide load whose lanes are 16 bytes apart touches eight
// 128-byte lines to use a quarter of each, and a cell needs four taps per advected field.  So a wave works on 256
// consecutive cells of a row in four rounds of 64 -- lane l takes cells l, 64+l, 128+l, 192+l -- which makes every
// gather of every round lane-contiguous: the two horizontally adjacent taps of a cell are ONE 8-byte load (they are
// contiguous in memory; 4-byte aligned, which global loads allow), so a round's taps touch three lines per instruction,
// not eight.  The wave's own cells -- velocities in, results out -- travel as one 16-byte access per lane and change
// into that order through LDS (wave_cells_in / wave_cells_out; k_gradient_advect keeps one dword per lane and round,
// see there).  Four independent back-traces per thread keep 8 or 16 loads in flight.  Per cell the arithmetic is the
// reference's, in its order.
// Offsets are BYTE offsets of type IDX: unsigned for fields below 2^32 bytes (every size up to ~32700^2 fp32), so an
// access is a scalar base plus a 32-bit vector offset and no 64-bit vector arithmetic is spent on addresses; size_t beyond.
template <typename S, typename IDX>
__device__ __forceinline__ const S* at(const S* base, IDX byte_off) { return reinterpret_cast<const S*>(reinterpret_cast<const char*>(base) + byte_off); }
template <typename S, typename IDX>
__device__ __forceinline__ S* at(S* base, IDX byte_off) { return reinterpret_cast<S*>(reinterpret_cast<char*>(base) + byte_off); }

template <typename IDX>
struct AdvectTap {
    IDX o;                // byte offset of the top-left tap
    float s0, s1, t0, t1;
};

// P: row pitch in bytes, E: element size in bytes
template <typename IDX>
__device__ __forceinline__ AdvectTap<IDX> advect_trace(int j, int i, float uu, float vv, float dt0, int n, IDX P, IDX E)
{
    float px = (float)j - dt0 * uu;
    float py = (float)i - dt0 * vv;
    const float hi = (float)n + 0.5f;
    // FluidSequential.c:117-127: if (x < 0.5) x = 0.5; if (x > N + 0.5) x = N + 0.5 -- as max / min (the same value
    // for every x that is not NaN; a NaN velocity, which sends the reference's (int) cast into undefined behaviour,
    // lands on the lower bound here)
    px = __builtin_fminf(__builtin_fmaxf(px, 0.5f), hi);
    py = __builtin_fminf(__builtin_fmaxf(py, 0.5f), hi);
    const int j0 = (int)px, i0 = (int)py;
    AdvectTap<IDX> t;
    t.s1 = px - (float)j0;
    t.s0 = 1.0f - t.s1;
    t.t1 = py - (float)i0;
    t.t0 = 1.0f - t.t1;
    t.o = (IDX)i0 * P + (IDX)(XOFF + j0) * E;
    return t;
}

// two horizontally adjacent cells in one access
struct __attribute__((packed, aligned(4))) FloatPair { float a, b; };
__device__ __forceinline__ void ld_pair(const float* p, float& a, float& b)
{
    const FloatPair v = *reinterpret_cast<const FloatPair*>(p);
    a = v.a;
    b = v.b;
}
__device__ __forceinline__ void ld_pair(const half_t* p, float& a, float& b)
{
    a = ld1(p);
    b = ld1(p + 1);
}

template <typename S, typename IDX>
__device__ __forceinline__ float advect_sample(const S* __restrict__ d0, IDX P, const AdvectTap<IDX>& t)
{
    float q00, q10, q01, q11;            // q[col][row]
    ld_pair(at(d0, t.o), q00, q10);
    ld_pair(at(d0, t.o + P), q01, q11);
    const float a = t.t0 * q00 + t.t1 * q01;
    const float e = t.t0 * q10 + t.t1 * q11;
    return t.s0 * a + t.s1 * e;
}

constexpr int kAdvectRounds = 4;         // cells per thread, 64 apart
// first column of a thread's round-0 cell: a block covers 256 threads x 4 rounds = 1024 consecutive columns
__device__ __forceinline__ int advect_col0() { return 1 + (int)blockIdx.x * 1024 + (int)(threadIdx.x >> 6) * 256 + (int)(threadIdx.x & 63); }
// does this block hold a cell next to a wall (wave-uniform)?  Only those run the ghost-cell code at all.
__device__ __forceinline__ bool advect_wall_block(int i, int n) { return i == 1 || i == n || blockIdx.x == 0 || blockIdx.x == gridDim.x - 1; }

// A wave's own 256 cells of a row, in and out, as ONE 16-byte access per lane instead of four 4-byte ones: the memory
// side wants lane l to hold cells 4l .. 4l+3, the gathers want it to hold cells l, 64+l, 128+l, 192+l (above), and a
// wave-private 1 KiB tile of LDS turns one into the other.  What these kernels wait for is the number of vector-memory
// instructions the texture addresser has to take apart, about 21 cycles each per CU whatever their width: the
// velocity loads and the result stores were half of them.  LDS executes a wave's instructions in order, so no barrier.
// `p` points at the wave's first cell (16-byte aligned: column 1 sits on a 256-byte line and waves start 256 cells apart);
// `cells` of the 256 exist (the rest of the row's last vector is pad; lanes past it repeat the last vector).
template <typename S>
__device__ __forceinline__ void wave_cells_in(const S* __restrict__ p, int cells, float* __restrict__ tile, float (&out)[4])
{
    const int lane = threadIdx.x & 63;
    const int vec = min(lane, (cells - 1) >> 2);
    *reinterpret_cast<float4*>(tile + 4 * lane) = ld4(p + 4 * vec);
    __builtin_amdgcn_wave_barrier();
#pragma unroll
    for (int k = 0; k < 4; ++k) out[k] = tile[lane + 64 * k];
    __builtin_amdgcn_wave_barrier();
}
template <typename S>
__device__ __forceinline__ void wave_cells_out(S* __restrict__ p, int cells, float* __restrict__ tile, const float (&val)[4])
{
    const int lane = threadIdx.x & 63;
#pragma unroll
    for (int k = 0; k < 4; ++k) tile[lane + 64 * k] = val[k];
    __builtin_amdgcn_wave_barrier();
    const float4 y = *reinterpret_cast<const float4*>(tile + 4 * lane);
    __builtin_amdgcn_wave_barrier();
    const int left = cells - 4 * lane;                   // cells of this lane's vector that exist
    if (left >= 4) {
        st4(p + 4 * lane, y);
    } else if (left > 0) {
        st1(p + 4 * lane, y.x);
        if (left > 1) st1(p + 4 * lane + 1, y.y);
        if (left > 2) st1(p + 4 * lane + 2, y.z);
    }
}

// (Round 3 built the version DESIGN.md had sketched -- the taps staged in LDS: a block takes a tile of 8 or 16 rows x 256
// columns, computes all its back-traces, reduces their bounding box, loads the box with coalesced 16-byte accesses when it
// fits 12-24 rows x 272 columns per field and reads every tap from LDS, else gathers as here.  Bit-identical, 1.6 instead of 5
// vector-memory instructions per cell -- and slower wherever the back-traces are short or smooth, which is the workload:
// 8192^2, one field, smooth velocity: 196-210 us against 178-196 here (16-row tiles: 243-264); two fields inside a step: 329 us
// against 275 (decaying data), 546 against 555 (ordinary data).  It only won on large AND noisy velocities (13-cell
// back-traces of white noise: 366 against 490 us).  Two block-wide barriers, the staging burst and 34-60 KB of LDS per block
// (2-4 blocks per CU) cost more than the gathers they replace; the single-field kernel here already moves its 1074 MB at
// 6.0 TB/s.  Not kept.)
// (A block that walks eight rows and loads the next row's velocity ahead of the current row's taps was measured slower:
// 324 against 294 us at 8192^2.  The texture addresser is busy 94 % of k_advect2's time -- rocprofv3 TA_BUSY_avr --
// so what these kernels wait for is the address path of their gathers, neither HBM nor latency.)
template <typename S, typename IDX>
__global__ __launch_bounds__(256) void k_advect(S* __restrict__ d, const S* __restrict__ d0, const S* __restrict__ u,
                                                const S* __restrict__ v, int pitch, int n, int row_lo, int row_hi,
                                                float dt0, int b, size_t ms, const float* __restrict__ mdt0)
{
    __shared__ __attribute__((aligned(16))) float tiles[4][2][256];
    if (mdt0) dt0 = mdt0[blockIdx.z];       // this member's own dt * N (wave-uniform)
    // the member's offset goes into the scalar bases: the offsets' width (IDX) depends on one field's size only
    d += blockIdx.z * ms; d0 += blockIdx.z * ms; u += blockIdx.z * ms; v += blockIdx.z * ms;
    const int j0 = advect_col0();
    const int i = row_lo + blockIdx.y;
    if (i >= row_hi) return;
    const IDX E = (IDX)sizeof(S), P = (IDX)pitch * E;
    const IDX r = (IDX)i * P + (IDX)XOFF * E;
    const bool wall = advect_wall_block(i, n);
    const int wave = threadIdx.x >> 6;
    const int c0 = j0 - (int)(threadIdx.x & 63);         // the wave's first column (wave-uniform)
    const int cells = min(256, n + 1 - c0);              // how many of its 256 columns exist
    if (cells <= 0) return;
    float uu[kAdvectRounds], vv[kAdvectRounds], val[kAdvectRounds];
    wave_cells_in(at(u, r + (IDX)c0 * E), cells, tiles[wave][0], uu);
    wave_cells_in(at(v, r + (IDX)c0 * E), cells, tiles[wave][1], vv);
#pragma unroll
    for (int k = 0; k < kAdvectRounds; ++k) val[k] = advect_sample(d0, P, advect_trace<IDX>(min(j0 + 64 * k, n), i, uu[k], vv[k], dt0, n, P, E));
    wave_cells_out(at(d, r + (IDX)c0 * E), cells, tiles[wave][0], val);
    if (wall) {
#pragma unroll
        for (int k = 0; k < kAdvectRounds; ++k) {
            const int j = j0 + 64 * k;
            if (j <= n) emit_ghosts(d, (size_t)pitch, n, b, j, i, val[k]);
        }
    }
}

// Two advections along the same velocity field in one pass (vel_step advects u and v, both along
// (u0, v0), FluidSequential.c:213-214): the velocity is read and the back-trace computed once, and
// the eight taps of the two sources sit at the same offsets.
template <typename S, typename IDX>
__global__ __launch_bounds__(256) void k_advect2(S* __restrict__ da, const S* __restrict__ d0a, int ba, S* __restrict__ db,
                                                 const S* __restrict__ d0b, int bb, const S* __restrict__ u,
                                                 const S* __restrict__ v, int pitch, int n, int row_lo, int row_hi, float dt0, size_t ms,
                                                 const float* __restrict__ mdt0)
{
    __shared__ __attribute__((aligned(16))) float tiles[4][2][256];
    if (mdt0) dt0 = mdt0[blockIdx.z];       // this member's own dt * N (wave-uniform)
    da += blockIdx.z * ms; d0a += blockIdx.z * ms; db += blockIdx.z * ms; d0b += blockIdx.z * ms; u += blockIdx.z * ms; v += blockIdx.z * ms;
    const int j0 = advect_col0();
    const int i = row_lo + blockIdx.y;
    if (i >= row_hi) return;
    const IDX E = (IDX)sizeof(S), P = (IDX)pitch * E;
    const IDX r = (IDX)i * P + (IDX)XOFF * E;
    const bool wall = advect_wall_block(i, n);
    const int wave = threadIdx.x >> 6;
    const int c0 = j0 - (int)(threadIdx.x & 63);         // the wave's first column (wave-uniform)
    const int cells = min(256, n + 1 - c0);              // how many of its 256 columns exist
    if (cells <= 0) return;
    float uu[kAdvectRounds], vv[kAdvectRounds], va[kAdvectRounds], vb[kAdvectRounds];
    wave_cells_in(at(u, r + (IDX)c0 * E), cells, tiles[wave][0], uu);
    wave_cells_in(at(v, r + (IDX)c0 * E), cells, tiles[wave][1], vv);
#pragma unroll
    for (int k = 0; k < kAdvectRounds; ++k) {
        const AdvectTap<IDX> t = advect_trace<IDX>(min(j0 + 64 * k, n), i, uu[k], vv[k], dt0, n, P, E);
        va[k] = advect_sample(d0a, P, t);
        vb[k] = advect_sample(d0b, P, t);
    }
    wave_cells_out(at(da, r + (IDX)c0 * E), cells, tiles[wave][0], va);
    wave_cells_out(at(db, r + (IDX)c0 * E), cells, tiles[wave][1], vb);
    if (wall) {
#pragma unroll
        for (int k = 0; k < kAdvectRounds; ++k) {
            const int j = j0 + 64 * k;
            if (j <= n) {
                emit_ghosts(da, (size_t)pitch, n, ba, j, i, va[k]);
                emit_ghosts(db, (size_t)pitch, n, bb, j, i, vb[k]);
            }
        }
    }
}

// ---------------------------------------------------------------------------
// a6  divergence + pressure clear (FluidSequential.c:143-158).
// div = (-0.5f*h) * (((uR - uL) + vD) - vU), p = 0, set_bnd(0) on both: the
// ghosts of p are 0 as well, so p is zeroed on whole rows incl. ghost rows.
// ---------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(256) void k_divergence(const S* __restrict__ u, const S* __restrict__ v, S* __restrict__ p,
                                                    S* __restrict__ div, int pitch, int n, int row_lo, int row_hi,
                                                    float h, int write_p, float pscale, size_t ms)
{
    const int j = 1 + blockIdx.x * 256 + threadIdx.x;
    const int i = row_lo + blockIdx.y;
    if (j > n || i >= row_hi) return;
    u += blockIdx.z * ms; v += blockIdx.z * ms; p += blockIdx.z * ms; div += blockIdx.z * ms;
    const size_t P = (size_t)pitch;
    const size_t c = (size_t)i * P + XOFF + j;
    const float scale = (-0.5f * h) * pscale;            // pscale: a power of two (1 unless the solver keeps a scaled pressure, fp16 storage)
    float g = ld1(u + c + 1) - ld1(u + c - 1);
    g = g + ld1(v + c + P);
    g = g - ld1(v + c - P);
    const float val = scale * g;
    st1(div + c, val);
    emit_ghosts(div, P, n, 0, j, i, val);
    if (write_p) {          // the solver usually just marks p as "all zero" instead
        st1(p + c, 0.0f);
        emit_ghosts(p, P, n, 0, j, i, 0.0f);
    }
}

// 64-lane butterfly maximum (the reductions further down, and k_subtract_gradient_max)
__device__ __forceinline__ float wave_max(float m)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off, 64));
    return m;
}

// ---------------------------------------------------------------------------
// a7  pressure-gradient subtraction (FluidSequential.c:161-173):
// u -= (0.5f*(pR-pL))/h ; v -= (0.5f*(pD-pU))/h ; set_bnd(1,u), set_bnd(2,v).
// ---------------------------------------------------------------------------
template <typename S>
__global__ __launch_bounds__(256) void k_subtract_gradient(S* __restrict__ u, S* __restrict__ v, const S* __restrict__ p,
                                                           int pitch, int n, int row_lo, int row_hi, float h, float pinv, size_t ms)
{
    const int j = 1 + blockIdx.x * 256 + threadIdx.x;
    const int i = row_lo + blockIdx.y;
    if (j > n || i >= row_hi) return;
    u += blockIdx.z * ms; v += blockIdx.z * ms; p += blockIdx.z * ms;
    const size_t P = (size_t)pitch;
    const size_t c = (size_t)i * P + XOFF + j;
    const float gx = 0.5f * (ld1(p + c + 1) - ld1(p + c - 1));
    const float gy = 0.5f * (ld1(p + c + P) - ld1(p + c - P));
    // pinv: 1 / (the power of two the pressure field is scaled by): (2^k x) / h * 2^-k is x / h, bit for bit
    const float nu = ld1(u + c) - (gx / h) * pinv;
    const float nv = ld1(v + c) - (gy / h) * pinv;
    st1(u + c, nu);
    st1(v + c, nv);
    emit_ghosts(u, P, n, 1, j, i, nu);
    emit_ghosts(v, P, n, 2, j, i, nv);
}

// The same with max(|u|, |v|) of what it stores (k_absmax2's result over the same rows, interior cells) reduced on the
// way: on row slabs the advection that follows needs that bound on the host before it can start, and a reduction pass of
// its own costs as much as this whole kernel.  Every block leaves its maximum in partials[]; k_max_partials (one block)
// folds them into the result word.  No atomics (thousands of them on one word serialise at ~12 ns each) and no memset.
template <typename S>
__global__ __launch_bounds__(256) void k_subtract_gradient_max(S* __restrict__ u, S* __restrict__ v, const S* __restrict__ p,
                                                               int pitch, int n, int row_lo, int row_hi, float h,
                                                               float* __restrict__ partials, float pinv)
{
    const int j = 1 + blockIdx.x * 256 + threadIdx.x;
    const size_t P = (size_t)pitch;
    float m = 0.0f;
    if (j <= n)
        for (int i = row_lo + blockIdx.y; i < row_hi; i += gridDim.y) {
            const size_t c = (size_t)i * P + XOFF + j;
            const float gx = 0.5f * (ld1(p + c + 1) - ld1(p + c - 1));
            const float gy = 0.5f * (ld1(p + c + P) - ld1(p + c - P));
            const float nu = ld1(u + c) - (gx / h) * pinv;
            const float nv = ld1(v + c) - (gy / h) * pinv;
            st1(u + c, nu);
            st1(v + c, nv);
            emit_ghosts(u, P, n, 1, j, i, nu);
            emit_ghosts(v, P, n, 2, j, i, nv);
            m = fmaxf(m, fmaxf(fabsf(as_stored<S>(nu)), fabsf(as_stored<S>(nv))));
        }
    __shared__ float part[4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) partials[blockIdx.y * gridDim.x + blockIdx.x] = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
}

__global__ __launch_bounds__(256) void k_max_partials(const float* __restrict__ partials, int count, unsigned int* __restrict__ result)
{
    float m = 0.0f;
    for (int k = threadIdx.x; k < count; k += 256) m = fmaxf(m, partials[k]);
    __shared__ float part[4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) *result = __float_as_uint(fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3])));
}

// The last two operators of a step in one pass (FluidSequential.c:240 + :185): the gradient subtraction
// of the second projection, then the density advection along the velocity it has just produced.  The
// back-trace of cell (i, j) needs u and v at (i, j) only -- the values this thread holds in registers
// (as stored: rounded to the storage type first) -- so the advection need not read the two fields back.
// Four cells per thread (64 apart, as in k_advect), per cell the arithmetic of k_subtract_gradient and k_advect.
// (Its own cells move as one dword per lane and round: the 16-byte accesses through LDS that pay in k_advect2 -- 44 -> 18
// memory instructions per wave and row here -- were built and measured for this kernel too, and gained nothing.)
template <typename S, typename IDX>
__global__ __launch_bounds__(256) void k_gradient_advect(S* __restrict__ u, S* __restrict__ v, const S* __restrict__ p,
                                                         S* __restrict__ d, const S* __restrict__ d0, int pitch, int n,
                                                         int row_lo, int row_hi, float h, float dt0, int b, float pinv, size_t ms,
                                                         const float* __restrict__ mdt0)
{
    if (mdt0) dt0 = mdt0[blockIdx.z];       // this member's own dt * N (wave-uniform)
    u += blockIdx.z * ms; v += blockIdx.z * ms; p += blockIdx.z * ms; d += blockIdx.z * ms; d0 += blockIdx.z * ms;
    const int j0 = advect_col0();
    const int i = row_lo + blockIdx.y;
    if (i >= row_hi) return;
    const IDX E = (IDX)sizeof(S), P = (IDX)pitch * E;
    const IDX r = (IDX)i * P + (IDX)XOFF * E;
    const bool wall = advect_wall_block(i, n);
    float nu[kAdvectRounds], nv[kAdvectRounds], val[kAdvectRounds];
#pragma unroll
    for (int k = 0; k < kAdvectRounds; ++k) {            // lane-contiguous dwords; the row's left/right neighbours are L1 hits
        const IDX c = r + (IDX)min(j0 + 64 * k, n) * E;
        const float gx = 0.5f * (ld1(at(p, c + E)) - ld1(at(p, c - E)));
        const float gy = 0.5f * (ld1(at(p, c + P)) - ld1(at(p, c - P)));
        nu[k] = ld1(at(u, c)) - (gx / h) * pinv;
        nv[k] = ld1(at(v, c)) - (gy / h) * pinv;
    }
#pragma unroll
    for (int k = 0; k < kAdvectRounds; ++k) {
        const int j = j0 + 64 * k;
        if (j <= n) {
            st1(at(u, r + (IDX)j * E), nu[k]);
            st1(at(v, r + (IDX)j * E), nv[k]);
            if (wall) {
                emit_ghosts(u, (size_t)pitch, n, 1, j, i, nu[k]);
                emit_ghosts(v, (size_t)pitch, n, 2, j, i, nv[k]);
            }
        }
    }
#pragma unroll
    for (int k = 0; k < kAdvectRounds; ++k)
        val[k] = advect_sample(d0, P, advect_trace<IDX>(min(j0 + 64 * k, n), i, as_stored<S>(nu[k]), as_stored<S>(nv[k]), dt0, n, P, E));
#pragma unroll
    for (int k = 0; k < kAdvectRounds; ++k) {
        const int j = j0 + 64 * k;
        if (j <= n) {
            st1(at(d, r + (IDX)j * E), val[k]);
            if (wall) emit_ghosts(d, (size_t)pitch, n, b, j, i, val[k]);
        }
    }
}

// ---------------------------------------------------------------------------
// wavefront reductions (diagnostics + the advect halo bound of the slab path).
// 64-lane __shfl_xor butterflies, one atomic per wave.  Neither feeds back
// into the fields, so they cannot change results.
//   k_absmax2 : max(|u|,|v|) over interior cells of rows [row_lo,row_hi)
//               (non-negative floats order like their bit patterns => atomicMax
//               on the uint view is exact and order independent).
//   k_residual: max |beta*x - alpha*(L+R+U+D) - x0| over the same cells.
// ---------------------------------------------------------------------------
// wave maxima -> block maximum (LDS) -> ONE atomic per block: contended atomics on a single word
// serialise at ~12 ns each, so one per wave from thousands of waves costs more than the reduction.
__device__ __forceinline__ void block_max_to(unsigned int* __restrict__ result, float m)
{
    __shared__ float part[4];
    m = wave_max(m);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0) {
        m = fmaxf(fmaxf(part[0], part[1]), fmaxf(part[2], part[3]));
        atomicMax(result, __float_as_uint(m));
    }
}

// one workgroup per group of rows, whole float4 vectors (columns beyond 1..n masked out)
// rstride (here and in k_residual): words between two members' results -- 0: every member into the one word (the maximum
// over the ensemble), 1: member m into word m
template <typename S>
__global__ __launch_bounds__(256) void k_absmax2(const S* __restrict__ u, const S* __restrict__ v, int pitch, int n,
                                                 int row_lo, int row_hi, unsigned int* __restrict__ result, size_t ms, int rstride)
{
    u += blockIdx.y * ms; v += blockIdx.y * ms;
    result += blockIdx.y * (unsigned)rstride;
    const size_t P = (size_t)pitch;
    const int nvec = (n + 3) >> 2;
    float m = 0.0f;
    for (int i = row_lo + blockIdx.x; i < row_hi; i += gridDim.x)
        for (int k = threadIdx.x; k < nvec; k += 256) {
            const size_t c = (size_t)i * P + XOFF + 1 + 4 * (size_t)k;
            const float4 a = ld4(u + c), b = ld4(v + c);
            const int last = n - (1 + 4 * k);            // components 0..last are columns <= n
            float t = fmaxf(fabsf(a.x), fabsf(b.x));
            if (last >= 1) t = fmaxf(t, fmaxf(fabsf(a.y), fabsf(b.y)));
            if (last >= 2) t = fmaxf(t, fmaxf(fabsf(a.z), fabsf(b.z)));
            if (last >= 3) t = fmaxf(t, fmaxf(fabsf(a.w), fabsf(b.w)));
            m = fmaxf(m, t);
        }
    block_max_to(result, m);
}

template <typename S>
__global__ __launch_bounds__(256) void k_residual(const S* __restrict__ x, const S* __restrict__ x0, int pitch, int n,
                                                  int row_lo, int row_hi, float alpha, float beta,
                                                  unsigned int* __restrict__ result, size_t ms, int rstride,
                                                  const float2* __restrict__ mab)
{
    if (mab) { alpha = mab[blockIdx.y].x; beta = mab[blockIdx.y].y; }      // this member's own coefficients (wave-uniform)
    x += blockIdx.y * ms; x0 += blockIdx.y * ms;
    result += blockIdx.y * (unsigned)rstride;
    const size_t P = (size_t)pitch;
    float m = 0.0f;
    for (int i = row_lo + blockIdx.x; i < row_hi; i += gridDim.x)
        // (kept rolled, as hipcc had it before the coefficient table existed: with the table's load ahead of the loop it unrolls
        // it for fp32 storage to 193 registers and 2 waves per SIMD, where the kernel used to have 33 and 8)
#pragma unroll 1
        for (int j = 1 + threadIdx.x; j <= n; j += 256) {
            const size_t c = (size_t)i * P + XOFF + j;
            const float nb = ld1(x + c - 1) + ld1(x + c + 1) + ld1(x + c - P) + ld1(x + c + P);
            m = fmaxf(m, fabsf(beta * ld1(x + c) - alpha * nb - ld1(x0 + c)));
        }
    block_max_to(result, m);
}

// ---------------------------------------------------------------------------
// ensemble reductions (diagnostics; include/fluid_amd.h "ensemble diagnostics").  Nothing here feeds back into a field.
// ---------------------------------------------------------------------------
// Per member, over the interior cells: the sum of x and of x*x in double (a stored value widens exactly, and the square
// of a float or half is exact in double).  Grid (blocks, members); a block strides over the rows as k_absmax2 does, whole
// 4-element vectors with the columns beyond n masked.  Two accumulators per lane, a 64-lane butterfly on doubles, the
// four waves combined through LDS, and ONE plain store of the block's pair into partials[member * gridDim.x + block]:
// no floating-point atomics, so the order of every addition is fixed by (n, members, grid) alone and the result is the
// same bits run after run.  k_fold_moments adds a member's partials.
__device__ __forceinline__ double wave_sum(double s)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) s = s + __shfl_xor(s, off, 64);
    return s;
}

template <typename S>
__global__ __launch_bounds__(256) void k_member_moments(const S* __restrict__ x, int pitch, int n, size_t ms,
                                                        double2* __restrict__ partials)
{
    x += blockIdx.y * ms;
    const size_t P = (size_t)pitch;
    const int nvec = (n + 3) >> 2;
    double s = 0.0, q = 0.0;
    for (int i = 1 + blockIdx.x; i <= n; i += gridDim.x)
        for (int k = threadIdx.x; k < nvec; k += 256) {
            const float4 a = ld4(x + (size_t)i * P + XOFF + 1 + 4 * (size_t)k);
            const int last = n - (1 + 4 * k);            // components 0..last are columns <= n
            const double d0 = (double)a.x, d1 = (double)a.y, d2 = (double)a.z, d3 = (double)a.w;
            s = s + d0; q = q + d0 * d0;
            if (last >= 1) { s = s + d1; q = q + d1 * d1; }
            if (last >= 2) { s = s + d2; q = q + d2 * d2; }
            if (last >= 3) { s = s + d3; q = q + d3 * d3; }
        }
    __shared__ double part[4][2];
    s = wave_sum(s);
    q = wave_sum(q);
    if ((threadIdx.x & 63) == 0) { part[threadIdx.x >> 6][0] = s; part[threadIdx.x >> 6][1] = q; }
    __syncthreads();
    if (threadIdx.x == 0)
        partials[(size_t)blockIdx.y * gridDim.x + blockIdx.x] =
            make_double2(((part[0][0] + part[1][0]) + part[2][0]) + part[3][0], ((part[0][1] + part[1][1]) + part[2][1]) + part[3][1]);
}

// one wave per member: lane l adds partials l, l + 64, ... in index order, then the butterfly
__global__ __launch_bounds__(64) void k_fold_moments(const double2* __restrict__ partials, int count, double2* __restrict__ out)
{
    const double2* p = partials + (size_t)blockIdx.x * count;
    double s = 0.0, q = 0.0;
    for (int k = threadIdx.x; k < count; k += 64) { s = s + p[k].x; q = q + p[k].y; }
    s = wave_sum(s);
    q = wave_sum(q);
    if (threadIdx.x == 0) out[blockIdx.x] = make_double2(s, q);
}

// The M x M matrix of inner products between the members of a field, or between their anomalies about the ensemble mean
// (include/fluid_amd.h "ensemble diagnostics", fluid_member_gram): a tall-skinny A^T A, interior cells x members, where
// every stored value is read from memory ONCE.  MP = the member count padded to 8, 16, 32 or 64 (padding members are
// zeros; their rows and columns are never read back).  A block stages a chunk of CH = 4096 / MP consecutive interior
// cells of one row in all members into LDS as doubles, [cell][member], R = MP + 2 doubles per cell: a lane loads one value
// (ld1: consecutive lanes, consecutive columns), widens it as the pack does and stores it; the two doubles of padding
// keep a cell 16-byte aligned and spread the lanes of a store over the banks.  CENTRE: one lane per cell then forms the
// mean chain of fluid_ensemble_stats in member order (IEEE double, no contraction) and subtracts it in place -- M adds per
// cell against MP^2 fmas.
// Each WAVE keeps the whole matrix in registers: lane (ta, tb) of the 8 x 8 lane grid owns the T x T tile of members
// T * ta .., T * tb .., T = MP / 8 -- 64 double accumulators at MP = 64 -- and the four waves of a block take the cells
// wave, wave + 4, .. of the chunk.  Per cell a lane reads its T + T operands from LDS (ds_read_b128; all lanes read the same
// cell, so equal ta or tb broadcast) and issues T * T v_fma_f64.  (ta, tb) is laid over the lanes so that each of the four
// 16-lane groups a ds_read_b128 is served in holds 4 values of ta and 4 of tb: their addresses lie in distinct banks.
// The lower triangle's lanes (ta > tb) compute their tiles like the others and drop them: a wave runs no faster with them
// masked.  The next chunk's 16 values per lane are loaded before the fmas of the current one.
// An accumulator starts at -0.0, so a sum starts from its first term.  At the end the four waves' matrices are added through
// LDS in wave order and the block's matrix (tiles with ta <= tb) goes to partials[block][MP * MP] with plain stores;
// k_fold_gram adds the blocks' partials per entry in a fixed order.  No floating-point atomics, no matrix instructions:
// the order of every addition is fixed by (n, members, storage, centre) alone.  Blocks stride over the chunks; row and
// member bases are 64-bit arithmetic, so fields past 4 GiB need nothing of their own.
constexpr int kGramChunkValues = 4096;       // cells x padded members of one staged chunk: 32 KiB of doubles
constexpr int kGramLoads = kGramChunkValues / 256;

template <int T>
__device__ __forceinline__ void gram_operands(const double* __restrict__ p, double (&o)[T])
{
    if constexpr (T == 1) o[0] = p[0];
    else {
#pragma unroll
        for (int i = 0; i < T; i += 2) {
            const double2 v = *reinterpret_cast<const double2*>(p + i);
            o[i] = v.x; o[i + 1] = v.y;
        }
    }
}

template <typename S, int MP, bool CENTRE>
__global__ __launch_bounds__(256) void k_member_gram(const S* __restrict__ x, int pitch, int n, size_t ms, int members, float inv,
                                                     int cpr, unsigned chunks, double* __restrict__ partials)
{
    constexpr int T = MP / 8, CH = kGramChunkValues / MP, R = MP + 2;
    static_assert(MP * MP <= CH * R, "the block's matrix is folded in the staging memory");
    __shared__ __attribute__((aligned(16))) double stage[CH * R];
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l5 = lane & 31, q = l5 >> 2;
    const int ta = 4 * (lane >> 5) + (q >> 1), tb = 4 * ((0x96 >> q) & 1) + (l5 & 3);
    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = -0.0;

    float f[kGramLoads];
    // chunk c: cells col0 .. col0 + nc - 1 of interior row 1 + c / cpr; value v = t + 256 * r of it: cell v % CH, member v / CH
    auto cells_of = [&](unsigned c) { return min(CH, n - (int)(c % (unsigned)cpr) * CH); };
    auto load = [&](unsigned c) {
        const int nc = cells_of(c);
        const S* row = x + (size_t)(1 + c / (unsigned)cpr) * (size_t)pitch + (size_t)(XOFF + 1) + (size_t)(c % (unsigned)cpr) * CH;
#pragma unroll
        for (int r = 0; r < kGramLoads; ++r) {
            const int v = t + 256 * r, cell = v % CH, k = v / CH;
            float a = 0.0f;
            if (cell < nc && k < members) {
                a = ld1(row + (size_t)k * ms + cell);
                if constexpr (sizeof(S) != 4) a = a * inv;
            }
            f[r] = a;
        }
    };

    unsigned chunk = blockIdx.x;              // (gridDim.x <= chunks: every block has a chunk)
    load(chunk);
    for (; chunk < chunks; chunk += gridDim.x) {
        const int nc = cells_of(chunk);
#pragma unroll
        for (int r = 0; r < kGramLoads; ++r) {
            const int v = t + 256 * r;
            stage[(v % CH) * R + v / CH] = (double)f[r];
        }
        __syncthreads();
        if constexpr (CENTRE) {
            const double dm = (double)members;
            for (int c = t; c < nc; c += 256) {
                double* p = stage + c * R;
                double s = p[0];
                for (int m = 1; m < members; ++m) s = s + p[m];
                const double mu = s / dm;
                for (int m = 0; m < members; ++m) p[m] = p[m] - mu;
            }
            __syncthreads();
        }
        if (chunk + gridDim.x < chunks) load(chunk + gridDim.x);
        for (int c = wave; c < nc; c += 4) {
            double a[T], b[T];
            gram_operands<T>(stage + c * R + ta * T, a);
            gram_operands<T>(stage + c * R + tb * T, b);
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }

    // ((wave 0 + wave 1) + wave 2) + wave 3, every lane its own entries; the last wave stores the block's matrix
    double* out = partials + (size_t)blockIdx.x * (MP * MP);
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const int at = (ta * T + i) * MP + tb * T + j;
                    if (w > 0) acc[i][j] = stage[at] + acc[i][j];
                    if (w < 3) stage[at] = acc[i][j];
                    else if (ta <= tb) out[at] = acc[i][j];
                }
        }
        if (w < 3) __syncthreads();
    }
}

// Entry e of the padded matrix: the sum over the blocks' partials in a fixed order -- 16 entries per block, 16 lanes per
// entry: lane p adds partials p, p + 16, .. in index order from -0.0, then the 16 sums are added in index order.  Entries
// of tiles below the diagonal (tile side T) were not stored and are not read; out[e] of them is left alone.
__global__ __launch_bounds__(256) void k_fold_gram(const double* __restrict__ partials, int count, int mp, int tile, double* __restrict__ out)
{
    __shared__ double part[16][16];
    const int e = blockIdx.x * 16 + (threadIdx.x & 15), p0 = threadIdx.x >> 4;
    const bool live = (e / mp) / tile <= (e % mp) / tile;
    double s = -0.0;
    if (live)
        for (int p = p0; p < count; p += 16) s = s + partials[(size_t)p * (size_t)(mp * mp) + e];
    part[p0][threadIdx.x & 15] = s;
    __syncthreads();
    if (threadIdx.x < 16 && live) {
        s = part[0][threadIdx.x];
#pragma unroll
        for (int p = 1; p < 16; ++p) s = s + part[p][threadIdx.x];
        out[e] = s;
    }
}

// ---- observing ensembles (include/fluid_amd.h "observing ensembles") -------------------------------------------------------
// One observation: the bilinear point sample of advect_sample, in float, operation by operation -- the taps as the pack
// shows them (fp16 storage: widened, the scale divided back in float), two lerps along the rows, one along the columns.
// `tap`: element offset of x[i0][j0] in a member; w = {s0, s1, t0, t1}.  All four taps are read whatever the weights: a
// non-finite tap under a zero weight makes the observation non-finite, as in the reference's advect.
template <typename S>
__device__ __forceinline__ float observe_point(const S* __restrict__ x, int pitch, unsigned long long tap, const float4& w, float inv)
{
    const S* p = x + tap;
    float q00 = ld1(p), q10 = ld1(p + 1), q01 = ld1(p + pitch), q11 = ld1(p + pitch + 1);            // q[col][row]
    if constexpr (sizeof(S) != 4) {
        q00 = q00 * inv; q10 = q10 * inv; q01 = q01 * inv; q11 = q11 * inv;
    }
    const float a = w.z * q00 + w.w * q01;
    const float e = w.z * q10 + w.w * q11;
    return w.x * a + w.y * e;
}

// Where the taps of a point come from (include/fluid_amd.h "typed networks"), the last template argument of the three kernels
// that read a field through the network.  OneField: every point observes x -- the kernels as they were, no per-point lookup.
// FieldOfPoint: point p observes field index[p]; `table` arrives by value with the kernel's arguments and goes into LDS at
// block start (twelve lanes, one 16-byte entry each, then a barrier), where a lane looks its point's entry up once per chunk,
// next to its tap and weights: the index is per lane, so the lookup is a vector one, and LDS serves 64 lanes on at most twelve
// addresses in one broadcast read.  observe_point is the same for both: it gets a base and an inv.
template <typename S>
struct OneField {
    static constexpr bool typed = false, recorded = false;
    const S* x;                            // member 0 of the launch
    float inv;
};
struct FieldOfPoint {
    static constexpr bool typed = true, recorded = false;
    const unsigned char* index;            // [points] field ids < kObservedFields
    FieldSources table;
    unsigned first;                        // member 0 of the launch is member `first` of every field
};

// Recorded (include/fluid_amd.h "asynchronous observations"): nothing is observed, h_k[p] is the float an earlier launch left
// in a record.  The two Gram kernels' gather is then one load per member: lane = point, so a wave reads 64 consecutive floats;
// no taps, no weights, no table and no barrier for it.  It does not depend on the storage type: instantiated with S = float.
struct Recorded {
    static constexpr bool typed = false, recorded = true;
    const float* h;                        // h[member * stride + point]
    size_t stride;
};

template <typename SRC>
__device__ __forceinline__ void stage_sources(const SRC& src, FieldSource* lds)
{
    if constexpr (SRC::typed) {
        if (threadIdx.x < kObservedFields) lds[threadIdx.x] = src.table.of[threadIdx.x];
        __syncthreads();
    }
}

// member 0 of the launch in the field point `pt` observes, and that field's 1 / scale
template <typename S, typename SRC>
__device__ __forceinline__ const S* source_of(const SRC& src, const FieldSource* lds, size_t ms, unsigned pt, float* inv)
{
    if constexpr (SRC::typed) {
        const FieldSource e = lds[src.index[pt]];
        *inv = e.inv;
        return reinterpret_cast<const S*>(e.base) + (size_t)src.first * ms;
    } else {
        *inv = src.inv;
        return src.x;
    }
}

// fluid_observe_members: one lane per point, the member in the grid (blockIdx.y); four gathered taps, one coalesced store.
// Points [p0, p0 + np) of the table; out[member * ostride + (point - p0)].
template <typename S, typename SRC>
__global__ __launch_bounds__(256) void k_observe_members(SRC src, int pitch, size_t ms, const unsigned long long* __restrict__ tap,
                                                         const float4* __restrict__ weight, int p0, int np, float* __restrict__ out,
                                                         size_t ostride)
{
    __shared__ FieldSource sources[kObservedFields];
    stage_sources(src, sources);
    const unsigned i = blockIdx.x * 256u + threadIdx.x;
    if (i >= (unsigned)np) return;
    const unsigned p = (unsigned)p0 + i;
    float inv;
    const S* x = source_of<S>(src, sources, ms, p, &inv);
    out[(size_t)blockIdx.y * ostride + i] = observe_point<S>(x + (size_t)blockIdx.y * ms, pitch, tap[p], weight[p], inv);
}

// fluid_observation_gram: k_member_gram with the observations of the members in place of their cells.  A chunk is CH = 64
// points in all MP padded members (padding members are zeros), staged in LDS as doubles [point][member], R = MP + 2 doubles
// per point; wave w gathers and interpolates members w, w + 4, .. of the chunk, lane l its point l, so a lane reads its
// point's offset and weights once per chunk.  One lane per point (wave 0) then does the operand chain of the header: the
// mean chain in member order and its subtraction (CENTRE), the multiplication by 1 / sigma (`sigma` non-null), and -- OBS --
// the innovation d = (y - mean) / sigma, which goes into the point's first padding double, stage[point][MP].
// The products are k_member_gram's: lane (ta, tb) of the 8 x 8 lane grid owns a T x T tile, the four waves take the points
// wave, wave + 4, .., and are added in wave order at the end.  The innovation column needs no accumulator of its own: the
// lanes below the diagonal, whose tiles are dropped anyway, take d for one of their operands --
//   lane (tb + 1, tb), tb = 0 .. 6: a[0] := d, so acc[0][j] = sum d * a_m, m = T * tb + j: rhs of tile row tb;
//   lane (7, 0):                   b[0] := d, so acc[i][0] = sum a_k * d, k = 7 T + i:     rhs of tile row 7;
//   lane (6, 0):                   both,      so acc[0][0] = sum d * d.
// A block's partial is E = MP * MP + MP + 1 doubles: the matrix (tiles with ta <= tb), rhs[MP], dd; plain stores, no
// atomics, no matrix instructions.  Blocks stride over the chunks: the order of every addition is fixed by (points,
// members, CENTRE, OBS).
constexpr int kObsChunk = 64;

template <typename S, int MP, bool CENTRE, bool OBS, typename SRC>
__global__ __launch_bounds__(256) void k_observation_gram(SRC src, int pitch, size_t ms, int members,
                                                          const unsigned long long* __restrict__ tap, const float4* __restrict__ weight,
                                                          const float* __restrict__ obs, const float* __restrict__ sigma, int points,
                                                          unsigned chunks, double* __restrict__ partials)
{
    constexpr int T = MP / 8, CH = kObsChunk, R = MP + 2, L = CH * MP / 256, E = MP * MP + MP + 1;
    static_assert(MP * MP <= CH * R, "the block's matrix is folded in the staging memory");
    __shared__ __attribute__((aligned(16))) double stage[CH * R];
    __shared__ FieldSource sources[kObservedFields];
    stage_sources(src, sources);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l5 = lane & 31, q = l5 >> 2;
    const int ta = 4 * (lane >> 5) + (q >> 1), tb = 4 * ((0x96 >> q) & 1) + (l5 & 3);
    const bool d_for_a = OBS && (ta == tb + 1 || (ta == 6 && tb == 0)), d_for_b = OBS && tb == 0 && ta >= 6;
    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = -0.0;

    float f[L];
    auto points_of = [&](unsigned c) { return min(CH, points - (int)c * CH); };
    auto load = [&](unsigned c) {
        const int pt = (int)c * CH + lane;
        const bool live = pt < points;
        if constexpr (SRC::recorded) {
#pragma unroll
            for (int r = 0; r < L; ++r) {
                const int k = wave + 4 * r;
                f[r] = live && k < members ? src.h[(size_t)k * src.stride + (size_t)pt] : 0.0f;
            }
        } else {
            const unsigned long long o = live ? tap[pt] : 0ull;
            const float4 w = live ? weight[pt] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float inv = 0.0f;
            const S* x = live ? source_of<S>(src, sources, ms, (unsigned)pt, &inv) : nullptr;
#pragma unroll
            for (int r = 0; r < L; ++r) {
                const int k = wave + 4 * r;
                float a = 0.0f;
                if (live && k < members) a = observe_point<S>(x + (size_t)k * ms, pitch, o, w, inv);
                f[r] = a;
            }
        }
    };

    unsigned chunk = blockIdx.x;              // (gridDim.x <= chunks: every block has a chunk)
    load(chunk);
    for (; chunk < chunks; chunk += gridDim.x) {
        const int nc = points_of(chunk);
#pragma unroll
        for (int r = 0; r < L; ++r) stage[lane * R + wave + 4 * r] = (double)f[r];
        __syncthreads();
        if (CENTRE || OBS || sigma) {
            if (t < nc) {
                const int pt = (int)chunk * CH + t;
                double* p = stage + t * R;
                double mu = 0.0;
                if constexpr (CENTRE) {
                    double s = p[0];
                    for (int m = 1; m < members; ++m) s = s + p[m];
                    mu = s / (double)members;
                }
                const double sg = sigma ? (double)sigma[pt] : 1.0;
                if (CENTRE || sigma)
                    for (int m = 0; m < members; ++m) {
                        double v = p[m];
                        if constexpr (CENTRE) v = v - mu;
                        if (sigma) v = v * sg;
                        p[m] = v;
                    }
                if constexpr (OBS) {
                    double dv = (double)obs[pt];
                    if constexpr (CENTRE) dv = dv - mu;
                    if (sigma) dv = dv * sg;
                    p[MP] = dv;
                }
            }
            __syncthreads();
        }
        if (chunk + gridDim.x < chunks) load(chunk + gridDim.x);
        for (int c = wave; c < nc; c += 4) {
            double a[T], b[T];
            gram_operands<T>(stage + c * R + ta * T, a);
            gram_operands<T>(stage + c * R + tb * T, b);
            if constexpr (OBS) {
                const double dv = stage[c * R + MP];
                if (d_for_a) a[0] = dv;
                if (d_for_b) b[0] = dv;
            }
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }

    // ((wave 0 + wave 1) + wave 2) + wave 3, every lane its own entries; the last wave stores the block's partial
    double* out = partials + (size_t)blockIdx.x * E;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const int at = (ta * T + i) * MP + tb * T + j;
                    if (w > 0) acc[i][j] = stage[at] + acc[i][j];
                    if (w < 3) stage[at] = acc[i][j];
                    else if (ta <= tb) out[at] = acc[i][j];
                    else if constexpr (OBS) {
                        if (ta == tb + 1 && i == 0) out[MP * MP + tb * T + j] = acc[i][j];
                        if (ta == 7 && tb == 0 && j == 0) out[MP * MP + 7 * T + i] = acc[i][j];
                        if (ta == 6 && tb == 0 && i == 0 && j == 0) out[MP * MP + MP] = acc[i][j];
                    }
                }
        }
        if (w < 3) __syncthreads();
    }
}

// k_fold_gram for the partials of k_observation_gram: entry e of the E = mp * mp + mp + 1 doubles of a partial (matrix,
// rhs, dd), the same fixed order -- 16 lanes per entry, lane p adds partials p, p + 16, .. from -0.0, then the 16 sums in
// index order.  Matrix entries of tiles below the diagonal were not stored and are not read; rhs and dd only with `obs`.
__global__ __launch_bounds__(256) void k_fold_observation_gram(const double* __restrict__ partials, int count, int mp, int tile, int obs,
                                                               double* __restrict__ out)
{
    __shared__ double part[16][16];
    const int entries = mp * mp + mp + 1;
    const int e = blockIdx.x * 16 + (threadIdx.x & 15), p0 = threadIdx.x >> 4;
    const bool live = e < mp * mp ? (e / mp) / tile <= (e % mp) / tile : (obs && e < entries);
    double s = -0.0;
    if (live)
        for (int p = p0; p < count; p += 16) s = s + partials[(size_t)p * (size_t)entries + e];
    part[p0][threadIdx.x & 15] = s;
    __syncthreads();
    if (threadIdx.x < 16 && live) {
        s = part[0][threadIdx.x];
#pragma unroll
        for (int p = 1; p < 16; ++p) s = s + part[p][threadIdx.x];
        out[e] = s;
    }
}

// ---- lattice observations (include/fluid_amd.h "lattice observations") ----------------------------------------------------
// fluid_observation_gram_lattice, first launch: the operands of every point of the network, observed ONCE whatever the
// number of nodes.  The first half of k_observation_gram, chunk by chunk: a block takes the CH = 64 points of its chunk,
// wave w gathers and interpolates members w, w + 4, .., one lane per point then does the operand chain of the header (mean
// chain in member order and its subtraction with CENTRE, the multiplication by 1 / sigma, the innovation with OBS) -- the
// same operations in the same order, so a_k and d have k_observation_gram's bits.  The rows go to out[point][R], R = MP + 2
// doubles: a_k for the MP padded members (padding members 0), then d (0 without OBS), then 0 -- the layout k_lattice_gram
// stages, written with consecutive lanes on consecutive doubles.
template <typename S, int MP, bool CENTRE, bool OBS, typename SRC>
__global__ __launch_bounds__(256) void k_observation_operands(SRC src, int pitch, size_t ms, int members,
                                                              const unsigned long long* __restrict__ tap, const float4* __restrict__ weight,
                                                              const float* __restrict__ obs, const float* __restrict__ sigma, int points,
                                                              double* __restrict__ out)
{
    constexpr int CH = kObsChunk, R = MP + 2, L = CH * MP / 256;
    __shared__ __attribute__((aligned(16))) double stage[CH * R];
    __shared__ FieldSource sources[kObservedFields];
    stage_sources(src, sources);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int first = (int)blockIdx.x * CH, nc = min(CH, points - first);
    {
        const int pt = first + lane;
        const bool live = pt < points;
        if constexpr (SRC::recorded) {
#pragma unroll
            for (int r = 0; r < L; ++r) {
                const int k = wave + 4 * r;
                stage[lane * R + k] = (double)(live && k < members ? src.h[(size_t)k * src.stride + (size_t)pt] : 0.0f);
            }
        } else {
            const unsigned long long o = live ? tap[pt] : 0ull;
            const float4 w = live ? weight[pt] : make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            float inv = 0.0f;
            const S* x = live ? source_of<S>(src, sources, ms, (unsigned)pt, &inv) : nullptr;
#pragma unroll
            for (int r = 0; r < L; ++r) {
                const int k = wave + 4 * r;
                float a = 0.0f;
                if (live && k < members) a = observe_point<S>(x + (size_t)k * ms, pitch, o, w, inv);
                stage[lane * R + k] = (double)a;
            }
        }
    }
    __syncthreads();
    if (t < nc) {
        const int pt = first + t;
        double* p = stage + t * R;
        double mu = 0.0;
        if constexpr (CENTRE) {
            double s = p[0];
            for (int m = 1; m < members; ++m) s = s + p[m];
            mu = s / (double)members;
        }
        const double sg = sigma ? (double)sigma[pt] : 1.0;
        if (CENTRE || sigma)
            for (int m = 0; m < members; ++m) {
                double v = p[m];
                if constexpr (CENTRE) v = v - mu;
                if (sigma) v = v * sg;
                p[m] = v;
            }
        double dv = 0.0;
        if constexpr (OBS) {
            dv = (double)obs[pt];
            if constexpr (CENTRE) dv = dv - mu;
            if (sigma) dv = dv * sg;
        }
        p[MP] = dv;
        p[MP + 1] = 0.0;
    }
    __syncthreads();
    double* rows = out + (size_t)first * R;
    for (int v = t; v < nc * R; v += 256) rows[v] = stage[v];
}

// ---- screening observations (include/fluid_amd.h "screening observations") ------------------------------------------------
// fluid_observation_departures and the gate of the six Gram and analysis calls: one body.  The first half of
// k_observation_operands with the members walked at run time -- a block takes the CH = 64 points of its chunk, wave w gathers
// and interpolates members w, w + 4, .., staged as doubles [point][member], kScreenRow = 65 doubles per point (an odd row:
// the lanes of the second half, one per point, walk their rows on different banks).  One lane per point then runs rules 2 - 5
// of the header, every operation rounded once: the mean chain and the chain of squared anomalies of k_ensemble_stats, the
// departure of k_observation_gram with CENTRE, the decision, the rank.  Every output pointer may be null:
//   mean, spread, departure [points] floats, rank, flag [points] bytes: the per-point results;
//   sigma_out [points] floats: +0 at a rejected point, what the point came with elsewhere (sigma_in, or 1 for a null one) --
//     the buffer the Gram launch behind this one reads; it may be sigma_in itself: a lane reads its own float, then writes it;
//   chunk_sums [chunks][3] doubles: the count, the sum of d * d and the sum of vs over the chunk's points that are not
//     rejected, each added in increasing point index from -0.0 (which is "from the first term": -0.0 + x has the bits of x).
// `obs` null: nothing beyond mean and spread is defined, and the host passes none of the other outputs.
constexpr int kScreenRow = 65;

template <typename S, typename SRC>
__global__ __launch_bounds__(256) void k_observation_screen(SRC src, int pitch, size_t ms, int members,
                                                            const unsigned long long* __restrict__ tap, const float4* __restrict__ weight,
                                                            const float* __restrict__ obs, const float* sigma_in, float threshold, int points,
                                                            float* sigma_out, float* __restrict__ mean, float* __restrict__ spread,
                                                            float* __restrict__ departure, unsigned char* __restrict__ rank,
                                                            unsigned char* __restrict__ flag, double* __restrict__ chunk_sums)
{
#pragma clang fp contract(off)
    constexpr int CH = kObsChunk, R = kScreenRow;
    __shared__ double stage[CH * R];
    __shared__ double term[3][CH];
    __shared__ FieldSource sources[kObservedFields];
    stage_sources(src, sources);
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int first = (int)blockIdx.x * CH, nc = min(CH, points - first);
    {
        const int pt = first + lane;
        const bool live = pt < points;
        if constexpr (SRC::recorded) {
            if (live)
                for (int k = wave; k < members; k += 4) stage[lane * R + k] = (double)src.h[(size_t)k * src.stride + (size_t)pt];
        } else {
            if (live) {
                const unsigned long long o = tap[pt];
                const float4 w = weight[pt];
                float inv = 0.0f;
                const S* x = source_of<S>(src, sources, ms, (unsigned)pt, &inv);
                for (int k = wave; k < members; k += 4) stage[lane * R + k] = (double)observe_point<S>(x + (size_t)k * ms, pitch, o, w, inv);
            }
        }
    }
    __syncthreads();
    if (t < nc) {
        const int pt = first + t;
        const double* p = stage + t * R;
        double s = p[0];
        for (int m = 1; m < members; ++m) s = s + p[m];
        const double mu = s / (double)members;
        double e = p[0] - mu;
        double q = e * e;
        for (int m = 1; m < members; ++m) {
            e = p[m] - mu;
            const double ee = e * e;
            q = q + ee;
        }
        const double var = q / (double)(members - 1);
        if (mean) mean[pt] = (float)mu;
        if (spread) spread[pt] = (float)sqrt(var);
        const float sf = sigma_in ? sigma_in[pt] : 1.0f;
        bool rejected = false;
        double lhs = 0.0, vs = 0.0;
        if (obs) {
            const double y = (double)obs[pt], sg = (double)sf;
            const double dep = y - mu;
            const double d = dep * sg;
            lhs = d * d;
            vs = var * sg;
            vs = vs * sg;
            const double bound = 1.0 + vs;
            const double t2 = (double)threshold * (double)threshold;
            const double lim = t2 * bound;
            rejected = threshold != 0.0f && lhs > lim;
            if (departure) departure[pt] = (float)dep;
            if (rank) {
                int below = 0;
                for (int m = 0; m < members; ++m) below += p[m] < y ? 1 : 0;      // (floats widened exactly: the floats' own order)
                rank[pt] = (unsigned char)below;
            }
            if (flag) flag[pt] = rejected ? 1 : 0;
        }
        if (sigma_out) sigma_out[pt] = rejected ? 0.0f : sf;
        if (chunk_sums) {
            term[0][t] = rejected ? -0.0 : 1.0;                                   // (-0.0: adding it changes no bit of any sum)
            term[1][t] = rejected ? -0.0 : lhs;
            term[2][t] = rejected ? -0.0 : vs;
        }
    }
    if (chunk_sums) {
        __syncthreads();
        if (t < 3) {
            double a = -0.0;
            for (int i = 0; i < nc; ++i) a = a + term[t][i];
            chunk_sums[(size_t)blockIdx.x * 3 + t] = a;
        }
    }
}

// the three sums of k_observation_screen's chunks, folded as k_fold_observation_gram folds partials: 16 lanes per sum, lane j
// chains the chunks j, j + 16, .. from -0.0, then the 16 sums are added in index order.  One block of 64 lanes.
__global__ __launch_bounds__(64) void k_fold_screen_sums(const double* __restrict__ chunk_sums, int chunks, double* __restrict__ out)
{
    __shared__ double part[16][4];
    const int e = threadIdx.x & 3, j = threadIdx.x >> 2;
    double s = -0.0;
    if (e < 3)
        for (int c = j; c < chunks; c += 16) s = s + chunk_sums[(size_t)c * 3 + e];
    part[j][e] = s;
    __syncthreads();
    if (threadIdx.x < 3) {
        s = part[0][threadIdx.x];
#pragma unroll
        for (int p = 1; p < 16; ++p) s = s + part[p][threadIdx.x];
        out[threadIdx.x] = s;
    }
}

// fluid_observation_gram_lattice, second launch: the second half of k_observation_gram, one block per node, the node index
// in the grid.  start[node] .. start[node + 1] are the node's entries {point index, bits of the float weight w}, in
// increasing point index, built and bounds-checked on the host; a block walks them in chunks of CH = 64: the entries go to
// LDS, then the points' rows of `operands` (k_observation_operands: R = MP + 2 doubles, read with consecutive lanes on
// consecutive doubles) are gathered into the staging layout of k_observation_gram.  Lane (ta, tb) of the 8 x 8 lane grid owns
// a T x T tile: per point it rounds w * a_k once for its T row operands and issues T * T v_fma_f64 with the unweighted
// column operands, (w * a_k) * a_m as the header defines it -- so within a diagonal tile only k <= m is the header's entry,
// and the host mirrors element by element.  The four waves take the points wave, wave + 4, .. of a chunk and are added in
// wave order at the end.  The innovation sums ride in lanes below the diagonal, whose tiles are dropped, with d for the
// COLUMN operand (the row operand is the one that carries w):
//   lane (ta, 0), ta = 1 .. 7: b[0] := d, so acc[i][0] = sum (w * a_k) * d, k = T * ta + i: rhs of tile row ta;
//   lane (2, 1):               row operands of tile row 0 and b[0] := d:                    rhs of tile row 0;
//   lane (3, 1):               a[0] := d, b[0] := d, so acc[0][0] = sum (w * d) * d.
// A node's result is a partial of k_observation_gram, E = MP * MP + MP + 1 doubles: the matrix (tiles with ta <= tb), rhs[MP],
// dd; a node without entries stores nothing (the host writes its zeros).  Plain stores, no atomics, no matrix instructions;
// the order of every addition is fixed by the node's list.
template <int MP, bool OBS>
__global__ __launch_bounds__(256) void k_lattice_gram(const double* __restrict__ operands, const int* __restrict__ start,
                                                      const int2* __restrict__ entry, double* __restrict__ out)
{
    constexpr int T = MP / 8, CH = kObsChunk, R = MP + 2, E = MP * MP + MP + 1;
    static_assert(MP * MP <= CH * R, "the node's matrix is folded in the staging memory");
    __shared__ __attribute__((aligned(16))) double stage[CH * R];
    __shared__ int2 ent[CH];
    const int first = start[blockIdx.x], last = start[blockIdx.x + 1];
    if (first >= last) return;
    const int t = threadIdx.x, lane = t & 63, wave = t >> 6;
    const int l5 = lane & 31, q = l5 >> 2;
    const int ta = 4 * (lane >> 5) + (q >> 1), tb = 4 * ((0x96 >> q) & 1) + (l5 & 3);
    const bool rhs0 = OBS && ta == 2 && tb == 1, dd_lane = OBS && ta == 3 && tb == 1;
    const bool d_for_b = OBS && ((tb == 0 && ta >= 1) || rhs0 || dd_lane);
    const int arow = rhs0 ? 0 : ta;
    double acc[T][T];
#pragma unroll
    for (int i = 0; i < T; ++i)
#pragma unroll
        for (int j = 0; j < T; ++j) acc[i][j] = -0.0;

    for (int base = first; base < last; base += CH) {
        const int nc = min(CH, last - base);
        if (t < nc) ent[t] = entry[base + t];
        __syncthreads();
        for (int v = t; v < nc * R; v += 256) {
            const int pt = v / R;
            stage[v] = operands[(size_t)ent[pt].x * R + (v - pt * R)];
        }
        __syncthreads();
        for (int c = wave; c < nc; c += 4) {
            const double w = (double)__int_as_float(ent[c].y);
            double a[T], b[T];
            gram_operands<T>(stage + c * R + arow * T, a);
            gram_operands<T>(stage + c * R + tb * T, b);
            if constexpr (OBS) {
                const double dv = stage[c * R + MP];
                if (dd_lane) a[0] = dv;
                if (d_for_b) b[0] = dv;
            }
#pragma unroll
            for (int i = 0; i < T; ++i) a[i] = w * a[i];
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) acc[i][j] = __builtin_fma(a[i], b[j], acc[i][j]);
        }
        __syncthreads();
    }

    // ((wave 0 + wave 1) + wave 2) + wave 3, every lane its own entries; the last wave stores the node's result
    double* res = out + (size_t)blockIdx.x * E;
#pragma unroll
    for (int w = 0; w < 4; ++w) {
        if (wave == w) {
#pragma unroll
            for (int i = 0; i < T; ++i)
#pragma unroll
                for (int j = 0; j < T; ++j) {
                    const int at = (ta * T + i) * MP + tb * T + j;
                    if (w > 0) acc[i][j] = stage[at] + acc[i][j];
                    if (w < 3) stage[at] = acc[i][j];
                    else if (ta <= tb) res[at] = acc[i][j];
                    else if constexpr (OBS) {
                        if (tb == 0 && j == 0) res[MP * MP + ta * T + i] = acc[i][j];
                        if (rhs0 && j == 0) res[MP * MP + i] = acc[i][j];
                        if (dd_lane && i == 0 && j == 0) res[MP * MP + MP] = acc[i][j];
                    }
                }
        }
        if (w < 3) __syncthreads();
    }
}

// Across the members, per cell (ghost cells included): mean and population variance as float fields in the layout of a
// field, by the two-pass definition of include/fluid_amd.h -- all in double, member order, the first member's value (not
// 0.0) as the start of both chains.  One lane per VW = 4 (fp16: 8) consecutive columns of a row, vector v of a row covering
// columns 1 + VW * (v - 1) .. VW * v: vector 0 holds ghost column 0 alone, the last one may end at ghost column n + 1.  A
// vector that lies within columns 1 .. n + 1 moves as whole 16-byte accesses; the (at most two) others of a row touch
// their valid columns one by one, so pads are neither read nor written.  The accumulators are dependent chains, the
// loads are not: kStatsUnroll members' vectors are loaded before they are added.
constexpr int kStatsUnroll = 4;

template <typename S> struct StatsVec { static constexpr int VW = 16 / (int)sizeof(S); };

template <typename S, bool FULL>
__device__ __forceinline__ void stats_load(const S* __restrict__ p, int valid, double (&d)[StatsVec<S>::VW])
{
    constexpr int VW = StatsVec<S>::VW;
    if constexpr (FULL) {
        if constexpr (sizeof(S) == 4) {
            const float4 a = *reinterpret_cast<const float4*>(p);
            d[0] = (double)a.x; d[1] = (double)a.y; d[2] = (double)a.z; d[3] = (double)a.w;
        } else {
            typedef half_t half8_t __attribute__((ext_vector_type(8)));
            const half8_t h = *reinterpret_cast<const half8_t*>(p);
#pragma unroll
            for (int e = 0; e < VW; ++e) d[e] = (double)(float)h[e];
        }
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) d[e] = ((valid >> e) & 1) ? (double)(float)p[e] : 0.0;
    }
}

template <typename S, bool FULL>
__device__ __forceinline__ void stats_cell(const S* __restrict__ x, size_t ms, int members, size_t at, int valid,
                                           float* __restrict__ mean, float* __restrict__ var)
{
    constexpr int VW = StatsVec<S>::VW;
    const double dm = (double)members;
    double s[VW], q[VW], mu[VW], d[kStatsUnroll][VW];
    stats_load<S, FULL>(x + at, valid, s);
    int m = 1;
    for (; m + kStatsUnroll <= members; m += kStatsUnroll) {
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r) stats_load<S, FULL>(x + (size_t)(m + r) * ms + at, valid, d[r]);
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r)
#pragma unroll
            for (int e = 0; e < VW; ++e) s[e] = s[e] + d[r][e];
    }
    for (; m < members; ++m) {
        stats_load<S, FULL>(x + (size_t)m * ms + at, valid, d[0]);
#pragma unroll
        for (int e = 0; e < VW; ++e) s[e] = s[e] + d[0][e];
    }
#pragma unroll
    for (int e = 0; e < VW; ++e) mu[e] = s[e] / dm;
    stats_load<S, FULL>(x + at, valid, d[0]);
#pragma unroll
    for (int e = 0; e < VW; ++e) { const double t = d[0][e] - mu[e]; q[e] = t * t; }
    m = 1;
    for (; m + kStatsUnroll <= members; m += kStatsUnroll) {
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r) stats_load<S, FULL>(x + (size_t)(m + r) * ms + at, valid, d[r]);
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r)
#pragma unroll
            for (int e = 0; e < VW; ++e) { const double t = d[r][e] - mu[e]; q[e] = q[e] + t * t; }
    }
    for (; m < members; ++m) {
        stats_load<S, FULL>(x + (size_t)m * ms + at, valid, d[0]);
#pragma unroll
        for (int e = 0; e < VW; ++e) { const double t = d[0][e] - mu[e]; q[e] = q[e] + t * t; }
    }
    if constexpr (FULL) {
#pragma unroll
        for (int e = 0; e < VW; e += 4) {
            *reinterpret_cast<float4*>(mean + at + e) = make_float4((float)mu[e], (float)mu[e + 1], (float)mu[e + 2], (float)mu[e + 3]);
            *reinterpret_cast<float4*>(var + at + e) =
                make_float4((float)(q[e] / dm), (float)(q[e + 1] / dm), (float)(q[e + 2] / dm), (float)(q[e + 3] / dm));
        }
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
            if ((valid >> e) & 1) {
                mean[at + e] = (float)mu[e];
                var[at + e] = (float)(q[e] / dm);
            }
    }
}

// total = (n + 2) * vecs work items, vecs = vectors per row (launch_ensemble_stats)
template <typename S>
__global__ __launch_bounds__(256) void k_ensemble_stats(const S* __restrict__ x, int pitch, int n, size_t ms, int members, int vecs,
                                                        float* __restrict__ mean, float* __restrict__ var)
{
    constexpr int VW = StatsVec<S>::VW;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;          // (n + 2) * vecs < 2^32 for every N the library accepts
    if (t >= (unsigned)(n + 2) * (unsigned)vecs) return;
    const int row = (int)(t / (unsigned)vecs), v = (int)(t % (unsigned)vecs);
    const int c0 = 1 + VW * (v - 1);                     // first column of this lane's vector (vector 0: 1 - VW)
    int valid = 0;
#pragma unroll
    for (int e = 0; e < VW; ++e)
        if (c0 + e >= 0 && c0 + e <= n + 1) valid |= 1 << e;
    // XOFF + c0 = 64 + VW * (v - 1) is a multiple of VW and never negative: vector 0 starts in the left pad, which it skips
    const size_t at = (size_t)row * (size_t)pitch + (size_t)(XOFF + c0);
    if (valid == (1 << VW) - 1) stats_cell<S, true>(x, ms, members, at, valid, mean, var);
    else stats_cell<S, false>(x, ms, members, at, valid, mean, var);
}

// ---------------------------------------------------------------------------
// relaxation to prior spread (include/fluid_amd.h "relaxation to prior spread"): the per-cell sample standard deviation of a
// field over the members as a dense float array, and the in-place rescaling of a field's anomalies towards such an array.
// Both are k_ensemble_stats with another end: lanes cut the same way (one lane per vector of columns, vector 0 the ghost
// column 0 alone, edge vectors masked, member bases in 64-bit scalar arithmetic, kStatsUnroll members' loads in flight),
// the same two chains s and q in double and member order, for any member count.  Two differences in shape, both measured
// (DESIGN.md section 9).  A vector is 4 columns in both storage types -- 16-byte accesses of float fields, 8-byte ones of
// half fields.  And there is ONE arithmetic path: a wave nearly always holds whole vectors and a row's two edge vectors,
// and two instantiations of the walk, as in k_ensemble_stats, make every such wave run the members twice; here only the
// accesses branch on `whole`, an edge vector loading its valid columns one by one and computing zeros in the others.
// The dense side is a member of a dense pack: row `row` starts row * (n + 2) floats behind the array, aligned to 4 bytes
// only (dense4_t).  Values are read as the pack shows them, widen(x) * inv for an fp16 field held at a scale.  The
// relaxation walks the members a third time to re-read, rescale and store them, and stores narrow(y) times the scale, as
// k_transform_members_local does.  A cell with q == 0 or f == 1 keeps its bits: an edge vector does not store it, a whole
// vector stores back the words it loaded for it; a lane without any other cell leaves before the third walk, and so does
// a wave of such lanes.  No LDS, no atomics.
// ---------------------------------------------------------------------------
typedef float dense4_t __attribute__((ext_vector_type(4), aligned(4)));

// columns per lane: 4 for both storage types (fp16: 8-byte accesses).  The 8 of k_ensemble_stats doubles the double
// arithmetic and the registers of a lane and halves the lanes: measured, never faster
template <typename S> struct SpreadVec { static constexpr int VW = 4; };

// one member's vector as stored (16 bytes, fp16: 8; an edge vector: its valid columns one by one, the others 0)
template <typename S> struct SpreadRaw { S c[SpreadVec<S>::VW]; };

template <typename S>
__device__ __forceinline__ SpreadRaw<S> spread_load(const S* __restrict__ p, int valid, bool whole)
{
    constexpr int VW = SpreadVec<S>::VW;
    typedef S vec_t __attribute__((ext_vector_type(VW)));
    SpreadRaw<S> r;
    if (whole) {
        const vec_t a = *reinterpret_cast<const vec_t*>(p);
#pragma unroll
        for (int e = 0; e < VW; ++e) r.c[e] = a[e];
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) r.c[e] = ((valid >> e) & 1) ? p[e] : (S)0;
    }
    return r;
}

// the value the pack shows
template <typename S>
__device__ __forceinline__ double spread_value(S c, float inv)
{
    if constexpr (sizeof(S) == 4) return (double)c;
    else return (double)(keep_f32((float)c) * inv);
}

// s, then mu = s / members and q, per column of the lane's vector: the chains of stats_cell
template <typename S>
__device__ __forceinline__ void spread_moments(const S* __restrict__ x, size_t ms, int members, size_t at, int valid, bool whole, float inv,
                                               double (&mu)[SpreadVec<S>::VW], double (&q)[SpreadVec<S>::VW])
{
    constexpr int VW = SpreadVec<S>::VW;
    const double dm = (double)members;
    double s[VW];
    SpreadRaw<S> d[kStatsUnroll];
    d[0] = spread_load<S>(x + at, valid, whole);
#pragma unroll
    for (int e = 0; e < VW; ++e) s[e] = spread_value<S>(d[0].c[e], inv);
    int m = 1;
    for (; m + kStatsUnroll <= members; m += kStatsUnroll) {
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r) d[r] = spread_load<S>(x + (size_t)(m + r) * ms + at, valid, whole);
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r)
#pragma unroll
            for (int e = 0; e < VW; ++e) s[e] = s[e] + spread_value<S>(d[r].c[e], inv);
    }
    for (; m < members; ++m) {
        d[0] = spread_load<S>(x + (size_t)m * ms + at, valid, whole);
#pragma unroll
        for (int e = 0; e < VW; ++e) s[e] = s[e] + spread_value<S>(d[0].c[e], inv);
    }
#pragma unroll
    for (int e = 0; e < VW; ++e) mu[e] = s[e] / dm;
    d[0] = spread_load<S>(x + at, valid, whole);
#pragma unroll
    for (int e = 0; e < VW; ++e) { const double t = spread_value<S>(d[0].c[e], inv) - mu[e]; q[e] = t * t; }
    m = 1;
    for (; m + kStatsUnroll <= members; m += kStatsUnroll) {
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r) d[r] = spread_load<S>(x + (size_t)(m + r) * ms + at, valid, whole);
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r)
#pragma unroll
            for (int e = 0; e < VW; ++e) { const double t = spread_value<S>(d[r].c[e], inv) - mu[e]; q[e] = q[e] + t * t; }
    }
    for (; m < members; ++m) {
        d[0] = spread_load<S>(x + (size_t)m * ms + at, valid, whole);
#pragma unroll
        for (int e = 0; e < VW; ++e) { const double t = spread_value<S>(d[0].c[e], inv) - mu[e]; q[e] = q[e] + t * t; }
    }
}

// this lane's vector: false past the last one.  `at`: element 0 of the vector in a member (for vector 0 in the left pad,
// which it skips: only element VW - 1 is valid); `dat`: the same element in a dense (n + 2)^2 array, negative for vector 0
// of row 0 (adding a valid e brings it back)
template <typename S>
__device__ __forceinline__ bool spread_vector(int pitch, int n, int vecs, size_t* at, ptrdiff_t* dat, int* valid)
{
    constexpr int VW = SpreadVec<S>::VW;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;          // (n + 2) * vecs < 2^32 for every N the library accepts
    if (t >= (unsigned)(n + 2) * (unsigned)vecs) return false;
    const int row = (int)(t / (unsigned)vecs), v = (int)(t % (unsigned)vecs);
    const int c0 = 1 + VW * (v - 1);
    int ok = 0;
#pragma unroll
    for (int e = 0; e < VW; ++e)
        if (c0 + e >= 0 && c0 + e <= n + 1) ok |= 1 << e;
    *valid = ok;
    *at = (size_t)row * (size_t)pitch + (size_t)(XOFF + c0);
    *dat = (ptrdiff_t)row * (ptrdiff_t)(n + 2) + (ptrdiff_t)c0;
    return true;
}

template <typename S>
__device__ __forceinline__ void spread_cell(const S* __restrict__ x, size_t ms, int members, size_t at, ptrdiff_t dat, int valid, bool whole, float inv,
                                            float* __restrict__ out)
{
    constexpr int VW = SpreadVec<S>::VW;
    const double dm1 = (double)(members - 1);
    double mu[VW], q[VW];
    spread_moments<S>(x, ms, members, at, valid, whole, inv, mu, q);
    float sd[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) sd[e] = (float)sqrt(q[e] / dm1);
    if (whole) {
#pragma unroll
        for (int e = 0; e < VW; e += 4) {
            dense4_t d;
            d.x = sd[e]; d.y = sd[e + 1]; d.z = sd[e + 2]; d.w = sd[e + 3];
            *reinterpret_cast<dense4_t*>(out + (dat + e)) = d;
        }
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
            if ((valid >> e) & 1) out[dat + e] = sd[e];
    }
}

// total = (n + 2) * vecs work items, as k_ensemble_stats; members >= 2
template <typename S>
__global__ __launch_bounds__(256) void k_member_spread(const S* __restrict__ x, int pitch, int n, size_t ms, int members, int vecs, float inv,
                                                       float* __restrict__ out)
{
    constexpr int VW = SpreadVec<S>::VW;
    size_t at;
    ptrdiff_t dat;
    int valid;
    if (!spread_vector<S>(pitch, n, vecs, &at, &dat, &valid)) return;
    spread_cell<S>(x, ms, members, at, dat, valid, valid == (1 << VW) - 1, inv, out);
}

// rule 6 of the header: product and sum each rounded once, then to float, then narrowed and back at the field's scale
template <typename S>
__device__ __forceinline__ S relaxed(S old, float inv, float scale, double mu, double f)
{
#pragma clang fp contract(off)
    const double d = spread_value<S>(old, inv) - mu;
    const double p = __dmul_rn(f, d);
    const float y = (float)__dadd_rn(mu, p);
    if constexpr (sizeof(S) == 4) return y;
    else return (S)keep_f32(as_stored<S>(y) * scale);
}

// one member's vector re-read, rescaled in the columns of `act` and stored; `act` is not 0
template <typename S>
__device__ __forceinline__ void relax_store(S* __restrict__ p, const SpreadRaw<S>& old, int act, bool whole, float inv, float scale,
                                            const double (&mu)[SpreadVec<S>::VW], const double (&f)[SpreadVec<S>::VW])
{
    constexpr int VW = SpreadVec<S>::VW;
    typedef S vec_t __attribute__((ext_vector_type(VW)));
    S y[VW];
#pragma unroll
    for (int e = 0; e < VW; ++e) y[e] = relaxed<S>(old.c[e], inv, scale, mu[e], f[e]);
    if (whole) {
        vec_t v;
#pragma unroll
        for (int e = 0; e < VW; ++e) v[e] = ((act >> e) & 1) ? y[e] : old.c[e];
        *reinterpret_cast<vec_t*>(p) = v;
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
            if ((act >> e) & 1) p[e] = y[e];
    }
}

template <typename S>
__device__ __forceinline__ void relax_cell(S* __restrict__ x, size_t ms, int members, size_t at, ptrdiff_t dat, int valid, bool whole, float inv,
                                           float scale, const float* __restrict__ prior, double alpha)
{
#pragma clang fp contract(off)
    constexpr int VW = SpreadVec<S>::VW;
    const double dm1 = (double)(members - 1);
    double mu[VW], q[VW], f[VW];
    float sb[VW];
    if (whole) {
#pragma unroll
        for (int e = 0; e < VW; e += 4) {
            const dense4_t d = *reinterpret_cast<const dense4_t*>(prior + (dat + e));
            sb[e] = d.x; sb[e + 1] = d.y; sb[e + 2] = d.z; sb[e + 3] = d.w;
        }
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e) sb[e] = ((valid >> e) & 1) ? prior[dat + e] : 0.0f;
    }
    spread_moments<S>(x, ms, members, at, valid, whole, inv, mu, q);
    int act = 0;
#pragma unroll
    for (int e = 0; e < VW; ++e) {
        const double sa = sqrt(q[e] / dm1);
        double t = (double)sb[e] - sa;
        t = __dmul_rn(alpha, t);
        t = t / sa;
        f[e] = __dadd_rn(1.0, t);
        if (((valid >> e) & 1) && q[e] != 0.0 && f[e] != 1.0) act |= 1 << e;      // (a NaN q or f is live: its cell becomes NaN)
    }
    if (act == 0) return;
    int m = 0;
    for (; m + kStatsUnroll <= members; m += kStatsUnroll) {
        SpreadRaw<S> d[kStatsUnroll];
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r) d[r] = spread_load<S>(x + (size_t)(m + r) * ms + at, valid, whole);
#pragma unroll
        for (int r = 0; r < kStatsUnroll; ++r) relax_store<S>(x + (size_t)(m + r) * ms + at, d[r], act, whole, inv, scale, mu, f);
    }
    for (; m < members; ++m) {
        const SpreadRaw<S> d = spread_load<S>(x + (size_t)m * ms + at, valid, whole);
        relax_store<S>(x + (size_t)m * ms + at, d, act, whole, inv, scale, mu, f);
    }
}

template <typename S>
__global__ __launch_bounds__(256) void k_relax_spread(S* __restrict__ x, int pitch, int n, size_t ms, int members, int vecs, float inv,
                                                      float scale, const float* __restrict__ prior, double alpha)
{
    constexpr int VW = SpreadVec<S>::VW;
    size_t at;
    ptrdiff_t dat;
    int valid;
    if (!spread_vector<S>(pitch, n, vecs, &at, &dat, &valid)) return;
    relax_cell<S>(x, ms, members, at, dat, valid, valid == (1 << VW) - 1, inv, scale, prior, alpha);
}

// ---------------------------------------------------------------------------
// moving whole ensembles: all members of a field <-> a dense float array (include/fluid_amd.h "moving ensembles").
// The dense side is one member after the other, each the reference's (n + 2)^2 row-major array, member m starting
// m * dstride floats behind `dense`: always float, aligned to 4 bytes only, and the offset of a row within 16 bytes
// changes from row to row when (n + 2) % 4 != 0.  The field side is cut into the vectors of k_ensemble_stats: one lane
// per VW = 4 (fp16: 8) columns, vector v of a row covering columns 1 + VW * (v - 1) .. VW * v, so a field-side access is
// 16 aligned bytes; vector 0 is ghost column 0 alone, and it and the last vector(s) of a row touch their valid columns
// one by one on both sides: pad columns are neither read as data nor written.  On the dense side a whole vector is VW / 4
// accesses of 16 bytes that promise 4-byte alignment only (global memory takes them; consecutive lanes, consecutive
// bytes of the row).  Grid (blocks over the (n + 2) * vecs vectors of a member, members): the member base on both sides
// is 64-bit scalar arithmetic per block -- members * dstride * 4 may pass 4 GiB -- and the offsets within a member have
// the index type I (narrow_index).  No LDS, no atomics.
// pack: dense = widen(x) * inv for fp16 storage (inv = 1 / FieldState::fscale, a power of two: the multiplication a
// download does on the host, exact); fp32 storage moves the words as they are.  unpack: x = narrow(dense), one
// round-to-nearest-even behind the empty-asm fence (st1).
// ---------------------------------------------------------------------------
template <typename S, typename I>
__device__ __forceinline__ bool member_vector(int pitch, int n, int vecs, I* at, I* dat, int* valid)
{
    constexpr int VW = StatsVec<S>::VW;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;          // (n + 2) * vecs < 2^32 for every N the library accepts
    if (t >= (unsigned)(n + 2) * (unsigned)vecs) return false;
    const int row = (int)(t / (unsigned)vecs), v = (int)(t % (unsigned)vecs);
    const int c0 = 1 + VW * (v - 1);                     // first column of this lane's vector (vector 0: 1 - VW)
    int ok = 0;
#pragma unroll
    for (int e = 0; e < VW; ++e)
        if (c0 + e >= 0 && c0 + e <= n + 1) ok |= 1 << e;
    *valid = ok;
    // element 0 of the vector on either side; for vector 0 that lies before the row (only element VW - 1 is touched)
    *at = (I)row * (I)pitch + (I)(XOFF + c0);
    *dat = (I)row * (I)(n + 2) + (I)c0;        // (wraps for vector 0 of row 0: c0 < 0; adding e = VW - 1 wraps it back)
    return true;
}

template <typename S, typename I>
__global__ __launch_bounds__(256) void k_pack_members(const S* __restrict__ x, int pitch, int n, size_t ms, int vecs, float inv,
                                                      float* __restrict__ dense, size_t dstride)
{
    constexpr int VW = StatsVec<S>::VW;
    I at, dat;
    int valid;
    if (!member_vector<S, I>(pitch, n, vecs, &at, &dat, &valid)) return;
    x += blockIdx.y * ms;
    dense += blockIdx.y * dstride;
    if (valid == (1 << VW) - 1) {
        float f[VW];
        if constexpr (sizeof(S) == 4) {
            const float4 a = *reinterpret_cast<const float4*>(x + at);
            f[0] = a.x; f[1] = a.y; f[2] = a.z; f[3] = a.w;
        } else {
            typedef half_t half8_t __attribute__((ext_vector_type(8)));
            const half8_t h = *reinterpret_cast<const half8_t*>(x + at);
#pragma unroll
            for (int e = 0; e < VW; ++e) f[e] = keep_f32((float)h[e]) * inv;
        }
#pragma unroll
        for (int e = 0; e < VW; e += 4) {
            dense4_t d;
            d.x = f[e]; d.y = f[e + 1]; d.z = f[e + 2]; d.w = f[e + 3];
            *reinterpret_cast<dense4_t*>(dense + (I)(dat + (I)e)) = d;
        }
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
            if ((valid >> e) & 1) {
                if constexpr (sizeof(S) == 4) dense[(I)(dat + (I)e)] = x[(I)(at + (I)e)];
                else dense[(I)(dat + (I)e)] = ld1(x + (I)(at + (I)e)) * inv;
            }
    }
}

template <typename S, typename I>
__global__ __launch_bounds__(256) void k_unpack_members(S* __restrict__ x, int pitch, int n, size_t ms, int vecs,
                                                        const float* __restrict__ dense, size_t dstride)
{
    constexpr int VW = StatsVec<S>::VW;
    I at, dat;
    int valid;
    if (!member_vector<S, I>(pitch, n, vecs, &at, &dat, &valid)) return;
    x += blockIdx.y * ms;
    dense += blockIdx.y * dstride;
    if (valid == (1 << VW) - 1) {
        float f[VW];
#pragma unroll
        for (int e = 0; e < VW; e += 4) {
            const dense4_t d = *reinterpret_cast<const dense4_t*>(dense + (I)(dat + (I)e));
            f[e] = d.x; f[e + 1] = d.y; f[e + 2] = d.z; f[e + 3] = d.w;
        }
        if constexpr (sizeof(S) == 4) {
            *reinterpret_cast<float4*>(x + at) = make_float4(f[0], f[1], f[2], f[3]);
        } else {
            typedef half_t half8_t __attribute__((ext_vector_type(8)));
            half8_t h;
#pragma unroll
            for (int e = 0; e < VW; ++e) h[e] = (half_t)keep_f32(f[e]);
            *reinterpret_cast<half8_t*>(x + at) = h;
        }
    } else {
#pragma unroll
        for (int e = 0; e < VW; ++e)
            if ((valid >> e) & 1) st1(x + (I)(at + (I)e), dense[(I)(dat + (I)e)]);
    }
}

// ---------------------------------------------------------------------------
// block-averaged pack (include/fluid_amd.h "coarse snapshots"): the (n + 2)^2 array of a member, ghost ring included, cut
// into R x R blocks, R = 2^LR, each written as one float.  The order of the sum is part of the contract: per row of a block
// a pairwise tree over adjacent columns in double, then the rows added one after the other, one exact scaling, one
// rounding.  The kernel is one read of the field: a lane takes the VW = 4 (fp16: 8) columns VW * g .. VW * g + VW - 1 of
// a row -- a group, block-aligned -- and walks down the R rows of its block, 8 rows' loads in flight at a time, with the
// running sum(s) in registers.  Column 0
// sits one element before an aligned line, so a group is the last element of one aligned 16-byte vector and the first
// VW - 1 of the next: the lane loads the aligned vector at column VW * g + 1 and takes column VW * g from the lane below
// it, which holds it as the last element of its own vector (one lane exchange per load); lane 0 of a wave and the first
// group of a row load that one element themselves.  The last element of a row's last vector is a pad column (inside the
// pitch: pitch_for), loaded and not used.  R > VW: the R / VW lanes of a block finish each row's tree with xor exchanges,
// lower lane + upper lane at every level in the block's first lane, which writes the cell.  R < VW: a lane owns VW / R
// cells.  Grid (blocks over the side * groups lanes of a member, members), member bases in 64-bit scalar arithmetic, field
// offsets of type I (narrow_index), as in k_pack_members.  No LDS, no atomics; the stores are 1 / R^2 of the traffic.
// ---------------------------------------------------------------------------
// ROWS rows of a lane's group, from row `at` on, all their loads in flight together: s[0 .. OUTS) takes (FIRST: starts from) each
// row's tree over the columns of each of the lane's blocks (R > VW: of the whole block), row after row
template <typename S, typename I, int LR, int ROWS, bool FIRST>
__device__ __forceinline__ void coarse_rows(const S* __restrict__ x, I at, int pitch, float inv, bool own, double* s)
{
    constexpr int VW = StatsVec<S>::VW, R = 1 << LR;
    constexpr int LANES = R > VW ? R / VW : 1, OUTS = R < VW ? VW / R : 1;
    typedef S vec_t __attribute__((ext_vector_type(VW)));
    vec_t v[ROWS];                                      // columns VW * g + 1 .. VW * g + VW
    S lone[ROWS];                                       // column VW * g, where no lane below holds it
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        v[i] = *reinterpret_cast<const vec_t*>(x + (I)(at + (I)i * (I)pitch));
        lone[i] = (S)0;
    }
    if (own) {
#pragma unroll
        for (int i = 0; i < ROWS; ++i) lone[i] = x[(I)(at + (I)i * (I)pitch - (I)1)];
    }
#pragma unroll
    for (int i = 0; i < ROWS; ++i) {
        float f[VW], mine;
        if constexpr (sizeof(S) == 4) {
#pragma unroll
            for (int e = 0; e < VW; ++e) f[e] = v[i][e];
            mine = lone[i];
        } else {
#pragma unroll
            for (int e = 0; e < VW; ++e) f[e] = keep_f32((float)v[i][e]) * inv;
            mine = keep_f32((float)lone[i]) * inv;
        }
        const float below = __shfl_up(f[VW - 1], 1);
        double d[VW];
        d[0] = (double)(own ? mine : below);
#pragma unroll
        for (int e = 1; e < VW; ++e) d[e] = (double)f[e - 1];
#pragma unroll
        for (int width = VW >> 1; width >= OUTS; width >>= 1)      // the levels of the tree inside the group
#pragma unroll
            for (int k = 0; k < width; ++k) d[k] = d[2 * k] + d[2 * k + 1];
#pragma unroll
        for (int m = 1; m < LANES; m <<= 1) d[0] = d[0] + __shfl_xor(d[0], m);      // ... and across the block's lanes
#pragma unroll
        for (int k = 0; k < OUTS; ++k) s[k] = FIRST && i == 0 ? d[k] : s[k] + d[k];      // the sum starts from row 0, not from 0.0
    }
}

template <typename S, typename I, int LR>
__global__ __launch_bounds__(256) void k_pack_members_coarse(const S* __restrict__ x, int pitch, int n, size_t ms, int groups, float inv,
                                                             float* __restrict__ coarse, size_t cstride)
{
    constexpr int VW = StatsVec<S>::VW, R = 1 << LR;
    constexpr int LANES = R > VW ? R / VW : 1;          // lanes that share a coarse cell
    constexpr int OUTS = R < VW ? VW / R : 1;           // coarse cells of one lane
    constexpr int ROWS = R < 8 ? R : 8;                 // rows whose loads are in flight together
    constexpr double SCALE = 1.0 / (double)(1 << (2 * LR));
    const int side = (n + 2) >> LR;
    const unsigned t = blockIdx.x * 256u + threadIdx.x;           // side * groups < 2^32 for every N the library accepts
    // (n + 2) % R == 0: groups % LANES == 0, so the lanes of a block are LANES aligned lanes of one wave, all here or all gone
    if (t >= (unsigned)side * (unsigned)groups) return;
    const int bi = (int)(t / (unsigned)groups), g = (int)(t % (unsigned)groups);
    x += blockIdx.y * ms;
    coarse += blockIdx.y * cstride;
    const bool own = (threadIdx.x & 63u) == 0 || g == 0;          // no lane below that holds column VW * g
    I at = (I)(bi << LR) * (I)pitch + (I)(XOFF + 1 + VW * g);      // XOFF + 1 = 64: 16 aligned bytes
    double s[OUTS];
    coarse_rows<S, I, LR, ROWS, true>(x, at, pitch, inv, own, s);
#pragma unroll 1
    for (int i = ROWS; i < R; i += ROWS) {
        at += (I)ROWS * (I)pitch;
        coarse_rows<S, I, LR, ROWS, false>(x, at, pitch, inv, own, s);
    }
    const size_t out = (size_t)bi * (size_t)side;
    if constexpr (R >= VW) {
        if ((g & (LANES - 1)) == 0) coarse[out + (size_t)(g / LANES)] = (float)(s[0] * SCALE);
    } else {
#pragma unroll
        for (int k = 0; k < OUTS; ++k)
            if (g * OUTS + k < side) coarse[out + (size_t)(g * OUTS + k)] = (float)(s[k] * SCALE);
    }
}

// ---------------------------------------------------------------------------
// recombining ensembles (include/fluid_amd.h "recombining ensembles"): every new member of a field a linear combination of
// the old ones, in place, X' = X T.  A lane owns ONE cell of one row in all members -- with fp16 storage too: two bytes per
// lane, consecutive lanes consecutive bytes -- and keeps MP double accumulators in registers, MP = the member count rounded
// up to a power of two: 2 * MP VGPRs, 128 at MP = 64, which is why a lane owns no 16-byte vector here.  It walks the old
// members in order, kTransformAhead of their loads in flight at a time, widens each value once (as the pack does: fp16
// widened exactly, times inv = 1 / FieldState::fscale) and adds its product with each weight of row k of the table to that
// column's accumulator: one v_fma_f64 per term -- the product of two widened floats is exact in double, so the fused form
// rounds exactly where mul + add would.  An accumulator starts at -0.0: -0.0 + p == p for every p, +-0, inf and NaN
// included, so the sum starts from its first term without a flag.  All loads of a cell precede its first store by data
// dependence: the call is in place.
// The table: [members][MP] doubles (padding columns 0), read by every lane at the same address -- scalar loads, the weight
// an SGPR operand of the fma.  DENSE: no weight of the members x members matrix is zero, every term is taken (a padding
// column's accumulator may then hold anything; it is never stored).  Otherwise bits[k] holds a set bit for every column m
// with a non-zero weight of old member k and a term is skipped by a uniform branch -- scalar work only: first per k, then
// per group of 8 columns, then per column, so a selection costs M * (MP / 8 + 8) scalar tests and M fmas per cell.
// `empty`: the columns with no term at all (known on the host), stored as +0.
// Grid (blocks over the n + 2 columns, rows): row and member bases are 64-bit scalar arithmetic, a lane's own offset is
// its column -- no index-width template, nothing of its own for fields past 4 GiB.  No LDS, no atomics.
// ---------------------------------------------------------------------------
constexpr int kTransformAhead = 4;

template <int MP, bool DENSE>
__device__ __forceinline__ void transform_term(double (&acc)[MP], double xd, const double* __restrict__ w, unsigned long long bits)
{
    if constexpr (DENSE) {
        // 32 weights -- 64 SGPRs -- at a time: without the barrier the scheduler hoists the scalar loads of all the rows in
        // flight to the top and spills SGPRs into VGPR lanes, a v_readlane per weight
#pragma unroll
        for (int g = 0; g < MP; g += 32) {
#pragma unroll
            for (int m = g; m < g + 32 && m < MP; ++m) acc[m] = __builtin_fma(xd, w[m], acc[m]);
            __builtin_amdgcn_sched_barrier(0);
        }
    } else {
        if (bits == 0) return;
#pragma unroll
        for (int g = 0; g < MP; g += 8) {
            if (MP > 8 && ((bits >> g) & 0xffull) == 0) continue;
#pragma unroll
            for (int m = g; m < g + 8 && m < MP; ++m)
                if ((bits >> m) & 1ull) acc[m] = __builtin_fma(xd, w[m], acc[m]);
        }
    }
}

template <typename S, int MP, bool DENSE>
__global__ __launch_bounds__(256) void k_transform_members(S* __restrict__ x, int pitch, int n, size_t ms, int members, float inv,
                                                           const double* __restrict__ table, const unsigned long long* __restrict__ bits,
                                                           unsigned long long empty)
{
    const unsigned col = blockIdx.x * 256u + threadIdx.x;
    if (col > (unsigned)(n + 1)) return;
    x += (size_t)blockIdx.y * (size_t)pitch + (size_t)XOFF;      // this row of member 0, scalar; the lane adds its column
    double acc[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) acc[m] = -0.0;
    int k = 0;
    for (; k + kTransformAhead <= members; k += kTransformAhead) {
        float f[kTransformAhead];
#pragma unroll
        for (int r = 0; r < kTransformAhead; ++r) f[r] = ld1(x + (size_t)(k + r) * ms + col);
#pragma unroll
        for (int r = 0; r < kTransformAhead; ++r) {
            if constexpr (sizeof(S) != 4) f[r] = f[r] * inv;
            transform_term<MP, DENSE>(acc, (double)f[r], table + (size_t)(k + r) * MP, DENSE ? 0ull : bits[k + r]);
        }
    }
    for (; k < members; ++k) {
        float f = ld1(x + (size_t)k * ms + col);
        if constexpr (sizeof(S) != 4) f = f * inv;
        transform_term<MP, DENSE>(acc, (double)f, table + (size_t)k * MP, DENSE ? 0ull : bits[k]);
    }
#pragma unroll
    for (int m = 0; m < MP; ++m)
        if (m < members) st1(x + (size_t)m * ms + col, (empty >> m) & 1ull ? 0.0f : (float)acc[m]);
}

// ---------------------------------------------------------------------------
// localised updates (include/fluid_amd.h "localised updates"): the increment of a transform under a per-cell taper, in
// place, X' = X + g o (X D), over a box of cells only.  The kernel of k_transform_members with three differences.  The grid
// covers the box: blockIdx.y counts rows from row_lo, a block's 256 columns start at col_lo.  The taper is loaded first: a
// lane whose g is zero has nothing to store, and a wave whose lanes all find zero leaves after that one load -- a taper's
// bounding box is mostly such waves near its corners, a null box nearly all of them.  And the accumulators hold the
// increment s_m, not the new value: after the walk over the old members each member with a term (`used`, known on the
// host) is read once more -- its own cell, which no other lane stores and this lane has not stored yet -- and stored as
// x_m + g * s_m, product and sum rounded one after the other in double, then to float, then to the storage type.  The
// re-read costs a load that hits the cache; a second register set would cost 64 VGPRs at MP = 64.  Members without a term
// are not stored.  An fp16 field held at a scale (FieldState::fscale, a power of two) keeps it, because the cells this
// launch does not visit keep it: a value is read as widen(x) * inv, as the pack shows it, and narrow(y) goes back times
// `scale` -- exact, both being halves and powers of two apart, unless the product leaves the range of a half.
// ---------------------------------------------------------------------------
__device__ __forceinline__ float tapered(float xm, double g, double s)
{
#pragma clang fp contract(off)
    const double p = __dmul_rn(g, s);
    return (float)__dadd_rn((double)xm, p);
}

template <typename S, int MP, bool DENSE>
__global__ __launch_bounds__(256) void k_transform_members_local(S* __restrict__ x, int pitch, int w, size_t ms, int members,
                                                                 float inv, float scale, const double* __restrict__ table,
                                                                 const unsigned long long* __restrict__ bits, unsigned long long used,
                                                                 const float* __restrict__ taper, int row_lo, int col_lo, int col_hi)
{
    const unsigned col = (unsigned)col_lo + blockIdx.x * 256u + threadIdx.x;
    const size_t row = (size_t)row_lo + blockIdx.y;
    const bool inside = col < (unsigned)col_hi;
    float gf = 1.0f;
    if (taper && inside) gf = taper[row * (size_t)w + col];
    const bool live = inside && gf != 0.0f;                        // (a NaN taper is live: its cell becomes NaN)
    if (__builtin_amdgcn_ballot_w64(live) == 0) return;            // the whole wave: uniform
    if (!live) return;
    x += row * (size_t)pitch + (size_t)XOFF;                       // this row of member 0, scalar; the lane adds its column
    double acc[MP];
#pragma unroll
    for (int m = 0; m < MP; ++m) acc[m] = -0.0;
    int k = 0;
    for (; k + kTransformAhead <= members; k += kTransformAhead) {
        float f[kTransformAhead];
#pragma unroll
        for (int r = 0; r < kTransformAhead; ++r) f[r] = ld1(x + (size_t)(k + r) * ms + col);
#pragma unroll
        for (int r = 0; r < kTransformAhead; ++r) {
            if constexpr (sizeof(S) != 4) f[r] = f[r] * inv;
            transform_term<MP, DENSE>(acc, (double)f[r], table + (size_t)(k + r) * MP, DENSE ? 0ull : bits[k + r]);
        }
    }
    for (; k < members; ++k) {
        float f = ld1(x + (size_t)k * ms + col);
        if constexpr (sizeof(S) != 4) f = f * inv;
        transform_term<MP, DENSE>(acc, (double)f, table + (size_t)k * MP, DENSE ? 0ull : bits[k]);
    }
    const double g = (double)gf;
    constexpr int GROUP = MP < kTransformAhead ? MP : kTransformAhead;      // the loads of a group precede its stores
#pragma unroll
    for (int m0 = 0; m0 < MP; m0 += GROUP) {
        float xm[GROUP];
        bool take[GROUP];                                                   // uniform: scalar tests
#pragma unroll
        for (int r = 0; r < GROUP; ++r) {
            take[r] = m0 + r < members && ((used >> (m0 + r)) & 1ull);
            xm[r] = take[r] ? ld1(x + (size_t)(m0 + r) * ms + col) : 0.0f;
            if constexpr (sizeof(S) != 4) xm[r] = xm[r] * inv;
        }
#pragma unroll
        for (int r = 0; r < GROUP; ++r) {
            if (!take[r]) continue;
            float y = tapered(xm[r], g, acc[m0 + r]);
            if constexpr (sizeof(S) != 4) y = as_stored<S>(y) * scale;      // narrow(y), then the field's scale
            st1(x + (size_t)(m0 + r) * ms + col, y);
        }
    }
}

// ---------------------------------------------------------------------------
// lattice updates (include/fluid_amd.h "lattice updates"): X' = X + sum_b phi_b o (X D_b), the increment matrices D given at
// the nodes of a coarse lattice and blended bilinearly to every cell, every product on the OLD X, in place, one launch.
// A wave owns a patch of 64 cells, 2^lpc columns by 64 >> lpc rows, aligned to the lattice's origin; the spacing is a
// multiple of both sides, so a patch lies inside one lattice cell: its (up to) four corner nodes -- hence the four tables,
// their words of non-zero bits and which corners exist -- are wave-uniform and the weights stay scalar-load operands of
// v_fma_f64 as in k_transform_members (transform_term).  Only phi is per lane.  The widest patch the spacing allows is
// taken (one row of 64 columns at a multiple of 64): the bits do not depend on it.
// Two full accumulator sets (node sum and blend) would be 256 VGPRs at MP = 64.  Instead the new members are taken in
// chunks of 16: per chunk 16 blend sums, and per corner 16 node sums that are folded into them -- 64 VGPRs -- and each
// chunk and corner walks the old members again as k_transform_members does, kTransformAhead loads in flight, from the
// cache (a patch is members x 256 bytes).  Since a later chunk reads what an earlier one would have stored, nothing is
// stored before the last walk: a chunk's results wait as floats, MP VGPRs more.  (Keeping the OLD values in registers
// and walking them by an unrolled loop instead reads each once, but the scalar loads of 64 unrolled rows spill 60 to 170
// SGPRs into VGPR lanes at MP >= 16 and leave two waves per SIMD at MP = 64.)  A node sum starts at -0.0 like every sum of
// transform_term; so does the blend: -0.0 + p == p for every p, and a corner that takes no part in a lane (phi == 0 there,
// or no term in that column) adds -0.0 by select, so its inf or NaN never meets the sum.  Corners with phi == 0 in the whole
// wave, or without a term in the chunk, are skipped by uniform branches: that is every corner but one outside the hull and
// on a 1 x 1 lattice.  A (lane, member) no corner takes part in is not stored; the others store narrow((float)(x_m + s))
// times the field's scale.  Row and member bases are 64-bit scalar arithmetic; a lane adds a 32-bit offset inside its
// patch.  Lanes of an edge patch that fall outside the array are masked.  No LDS, no atomics.
// ---------------------------------------------------------------------------
struct LatticeAxis {
    int a;           // the lower node of the lattice cell: wave-uniform
    double t0, t1;   // this lane's weights of nodes a and a + 1
};

// rule 2 of the header; q0 = the patch's first index less the origin (a multiple of the patch side), q = the lane's
__device__ __forceinline__ LatticeAxis lattice_axis(int nodes, int step, long long q0, long long q)
{
    const long long last = (long long)(nodes - 1) * (long long)step;
    LatticeAxis ax;
    ax.a = (nodes == 1 || q0 <= 0) ? 0 : q0 >= last ? nodes - 2 : (int)(q0 / step);
    if (nodes == 1 || q <= 0) ax.t1 = 0.0;
    else if (q >= last) ax.t1 = 1.0;
    else ax.t1 = (double)(q - (long long)ax.a * (long long)step) / (double)step;
    ax.t0 = 1.0 - ax.t1;
    return ax;
}

template <typename S, int MP, bool DENSE>
__global__ __launch_bounds__(256) void k_transform_members_lattice(S* __restrict__ x, int pitch, int w, size_t ms, int members, float inv,
                                                                   float scale, const double* __restrict__ table,
                                                                   const unsigned long long* __restrict__ bits,
                                                                   const unsigned long long* __restrict__ cols, int nodes_row,
                                                                   int nodes_col, long long row0, long long col0, int step, int lpc,
                                                                   int row_off, int col_off)
{
#pragma clang fp contract(off)
    constexpr int CH = MP < 16 ? MP : 16;
    constexpr unsigned long long CMASK = (1ull << CH) - 1ull;
    const int wave = __builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6)), lane = (int)(threadIdx.x & 63u);
    const int pj = ((int)blockIdx.x * 4 + wave) * (1 << lpc) - col_off;      // the patch's first column and row: scalar,
    const int pi = (int)blockIdx.y * (64 >> lpc) - row_off;                   // negative where the origin's phase says so
    if (pj >= w) return;                                                       // (the whole wave)
    const int lr = lane >> lpc, lc = lane & ((1 << lpc) - 1);
    const int i = pi + lr, j = pj + lc;
    const bool live = (unsigned)i < (unsigned)w && (unsigned)j < (unsigned)w;
    const LatticeAxis ar = lattice_axis(nodes_row, step, (long long)pi - row0, (long long)i - row0);
    const LatticeAxis ac = lattice_axis(nodes_col, step, (long long)pj - col0, (long long)j - col0);
    // the corners in row-major node order: (a, b), (a, b + 1), (a + 1, b), (a + 1, b + 1)
    const double phi0 = live ? __dmul_rn(ar.t0, ac.t0) : 0.0, phi1 = live ? __dmul_rn(ar.t0, ac.t1) : 0.0;
    const double phi2 = live ? __dmul_rn(ar.t1, ac.t0) : 0.0, phi3 = live ? __dmul_rn(ar.t1, ac.t1) : 0.0;
    unsigned long long ccols[4];      // per corner the columns with a term, 0 where the corner takes no part in this wave
    size_t cnode[4];
    unsigned long long any = 0, mine = 0;      // columns some corner of the wave has; columns this lane stores
#pragma unroll
    for (int c = 0; c < 4; ++c) {
        const int ca = ar.a + (c >> 1), cb = ac.a + (c & 1);
        const double phi = c == 0 ? phi0 : c == 1 ? phi1 : c == 2 ? phi2 : phi3;
        const bool exists = ca < nodes_row && cb < nodes_col;
        cnode[c] = exists ? (size_t)ca * (size_t)nodes_col + (size_t)cb : 0;
        ccols[c] = exists && __builtin_amdgcn_ballot_w64(phi != 0.0) != 0 ? cols[cnode[c]] : 0ull;
        any |= ccols[c];
        if (phi != 0.0) mine |= ccols[c];
    }
    if (any == 0) return;                                                      // uniform: nothing to store in this patch
    const ptrdiff_t base = (ptrdiff_t)pi * (ptrdiff_t)pitch + (ptrdiff_t)pj + (ptrdiff_t)XOFF;      // scalar
    const int at = lr * pitch + lc;                                            // the lane's offset inside the patch
    const auto cell = [&](int m) { return x + (base + (ptrdiff_t)((size_t)m * ms)) + (unsigned)at; };      // scalar base + the lane's offset
    float y[MP];
#pragma unroll
    for (int m0 = 0; m0 < MP; m0 += CH) {
        if (m0 >= members || ((any >> m0) & CMASK) == 0) continue;             // uniform
        double s[CH];
#pragma unroll
        for (int r = 0; r < CH; ++r) s[r] = -0.0;
#pragma unroll 1
        for (int c = 0; c < 4; ++c) {
            const unsigned long long cc = (c == 0 ? ccols[0] : c == 1 ? ccols[1] : c == 2 ? ccols[2] : ccols[3]) >> m0;
            if ((cc & CMASK) == 0) continue;
            const size_t node = c == 0 ? cnode[0] : c == 1 ? cnode[1] : c == 2 ? cnode[2] : cnode[3];
            const double phi = c == 0 ? phi0 : c == 1 ? phi1 : c == 2 ? phi2 : phi3;
            const double* __restrict__ tab = table + node * (size_t)members * (size_t)MP + (size_t)m0;
            const unsigned long long* __restrict__ nb = bits + node * (size_t)members;
            double t[CH];
#pragma unroll
            for (int r = 0; r < CH; ++r) t[r] = -0.0;
            int k = 0;
            for (; k + kTransformAhead <= members; k += kTransformAhead) {
                float f[kTransformAhead];
#pragma unroll
                for (int r = 0; r < kTransformAhead; ++r) f[r] = live ? ld1(cell(k + r)) : 0.0f;
#pragma unroll
                for (int r = 0; r < kTransformAhead; ++r) {
                    if constexpr (sizeof(S) != 4) f[r] = f[r] * inv;
                    transform_term<CH, DENSE>(t, (double)f[r], tab + (size_t)(k + r) * MP, DENSE ? 0ull : (nb[k + r] >> m0) & CMASK);
                }
            }
            for (; k < members; ++k) {
                float f = live ? ld1(cell(k)) : 0.0f;
                if constexpr (sizeof(S) != 4) f = f * inv;
                transform_term<CH, DENSE>(t, (double)f, tab + (size_t)k * MP, DENSE ? 0ull : (nb[k] >> m0) & CMASK);
            }
            const bool lane_in = phi != 0.0;
#pragma unroll
            for (int r = 0; r < CH; ++r) {
                const double p = __dmul_rn(phi, t[r]);
                s[r] = __dadd_rn(s[r], lane_in && ((cc >> r) & 1ull) ? p : -0.0);
            }
        }
#pragma unroll
        for (int r = 0; r < CH; ++r) {
            const bool put = m0 + r < members && ((mine >> (m0 + r)) & 1ull);
            float xm = put ? ld1(cell(m0 + r)) : 0.0f;
            if constexpr (sizeof(S) != 4) xm = xm * inv;
            y[m0 + r] = (float)__dadd_rn((double)xm, s[r]);
        }
    }
#pragma unroll
    for (int m = 0; m < MP; ++m) {
        if (!(m < members && ((any >> m) & 1ull))) continue;                   // uniform; `mine` is the lane's own
        if (!((mine >> m) & 1ull)) continue;
        float v = y[m];
        if constexpr (sizeof(S) != 4) v = as_stored<S>(v) * scale;             // narrow(y), then the field's scale
        st1(cell(m), v);
    }
}

// one thread per cell of the dense (w x w) taper; the definition is fluid_kernels.h's, shared with the host's bounding box
__global__ __launch_bounds__(256) void k_taper_gaspari_cohn(float* __restrict__ out, int w, double col, double row, double c)
{
    const unsigned j = blockIdx.x * 256u + threadIdx.x;
    if (j >= (unsigned)w) return;
    const unsigned i = blockIdx.y;
    out[(size_t)i * (size_t)w + j] = (float)taper_value(taper_radius((double)j - col, (double)i - row, c));
}

// ---------------------------------------------------------------------------
// launch wrappers (host).  Shapes are validated by the caller (fluid_solver).
// `st` selects the field storage type the untyped pointers refer to.
// ---------------------------------------------------------------------------
static inline unsigned cdiv(unsigned a, unsigned b) { return (a + b - 1) / b; }

// element offsets into a field fit 32 bits (with a byte offset below 2^32 for the hardware's address add)
static inline bool narrow_index(int st, int pitch, int n) { return (size_t)(n + 2) * (size_t)pitch * storage_bytes(st) < (1ull << 32); }

#define FLUID_BY_STORAGE(st, ...)             \
    do {                                      \
        if ((st) == STORAGE_F16) {            \
            using S = half_t;                 \
            __VA_ARGS__;                      \
        } else {                              \
            using S = float;                  \
            __VA_ARGS__;                      \
        }                                     \
    } while (0)
// ... and of the kernels that take the index type of their field offsets: 32-bit where they fit (narrow_index)
#define FLUID_BY_STORAGE_INDEX(st, pitch, n, ...)                                                  \
    do {                                                                                           \
        if (narrow_index(st, pitch, n)) { using I = unsigned; FLUID_BY_STORAGE(st, __VA_ARGS__); } \
        else { using I = size_t; FLUID_BY_STORAGE(st, __VA_ARGS__); }                              \
    } while (0)

// grid-stride kernels over rows [row_lo, row_hi): one thread per 4 elements, 1 .. 8192 blocks
static inline unsigned stride_blocks(int pitch, int row_lo, int row_hi)
{
    return (unsigned)std::clamp<size_t>(((size_t)(row_hi - row_lo) * (pitch >> 2) + 255) / 256, 1, 8192);
}

void launch_set_bnd(hipStream_t s, int st, void* f, int pitch, int n, int b, Members mb)
{
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_set_bnd<S>, dim3(cdiv(n, 256), mb.count), dim3(256), 0, s, (S*)f, pitch, n, b, mb.stride));
}

// src == nullptr: the source is known to be all +0 (dt is then the pre-multiplied increment dt*0)
void launch_add_source(hipStream_t s, int st, void* x, const void* src, int pitch, int row_lo, int row_hi, float dt, Members mb,
                       const float* mdt)
{
    const dim3 grid(stride_blocks(pitch, row_lo, row_hi), mb.count);
    if (!src) {
        FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_add_zero_source<S>, grid, dim3(256), 0, s, (S*)x, pitch, row_lo, row_hi, dt, mb.stride, mdt));
        return;
    }
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_add_source<S>, grid, dim3(256), 0, s, (S*)x, (const S*)src, pitch, row_lo, row_hi, dt, mb.stride,
                                            mdt));
}

void launch_scale(hipStream_t s, int st, void* x, int pitch, int row_lo, int row_hi, float factor, Members mb)
{
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_scale<S>, dim3(stride_blocks(pitch, row_lo, row_hi), mb.count), dim3(256), 0, s, (S*)x, pitch,
                                            row_lo, row_hi, factor, mb.stride));
}

void launch_jacobi(hipStream_t s, int st, int variant, const void* x, const void* x0, void* out, int pitch, int n,
                   int row_lo, int row_hi, float alpha, float beta, int b, Members mb, const float2* mab)
{
    const int rows = row_hi - row_lo;
    if (rows <= 0) return;
    switch (variant) {
    case JACOBI_NAIVE:
        FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_jacobi_naive<S>, dim3(cdiv(n, 64), cdiv(rows, 4), mb.count), dim3(256), 0, s,
                                                (const S*)x, (const S*)x0, (S*)out, pitch, n, row_lo, row_hi, alpha,
                                                beta, b, mb.stride, mab));
        break;
    case JACOBI_LDS:
        FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_jacobi_lds<S>, dim3(cdiv(n, LT_X), cdiv(rows, LT_Y), mb.count), dim3(256), 0, s,
                                                (const S*)x, (const S*)x0, (S*)out, pitch, n, row_lo, row_hi, alpha,
                                                beta, b, mb.stride, mab));
        break;
    default: {
        constexpr int RB = 8;
        const unsigned nvec = (n + 3) / 4;
        FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_jacobi_stream<RB, S>), dim3(cdiv(nvec, 256), cdiv(rows, RB), mb.count), dim3(256),
                                                0, s, (const S*)x, (const S*)x0, (S*)out, pitch, n, row_lo, row_hi,
                                                alpha, beta, b, mb.stride, mab));
    }
    }
}

// one kernel per shape of kTbShapes (taking its address is what instantiates it), in the table's order
using TbKernel = void (*)(TbBatch, int, int, int, int, int, int, TbGrid, int);
template <typename S, size_t... I>
static std::array<TbKernel, kTbShapeCount> tb_kernels(std::index_sequence<I...>)
{
    return {&k_jacobi_tb<kTbShapes[I].T, kTbShapes[I].divmode, kTbShapes[I].nv, S, kTbShapes[I].form == TB_DIVSRC,
                         kTbShapes[I].form == TB_ADDSRC>...};
}

// batch.count solves per launch of the shape (T, divmode, nv, form).
// divmode 0: beta; 2: beta unused, yd = RN64(1/beta); 4: beta = exact reciprocal of a power of two and alpha == 1;
// 3: hi, lo = the two-term reciprocal where the tiles of |x0| minima allow it, yd elsewhere;
// 5: beta = RN32(1/beta), hi = beta * 2^24, lo = -(RN32(1/beta) * 2^-24), yd for the second pass of a wave that met inf / NaN.
bool launch_jacobi_tb(hipStream_t s, int st, int T, int divmode, int nv, int form, const TbBatch& batch, int pitch, int n, int row_lo,
                      int row_hi, int rb, int rb_edge, int hole_lo, int hole_hi, bool fill)
{
    static const auto f32 = tb_kernels<float>(std::make_index_sequence<kTbShapeCount>());
    static const auto f16 = tb_kernels<half_t>(std::make_index_sequence<kTbShapeCount>());
    const int shape = jacobi_tb_index(T, divmode, nv, form);
    if (shape < 0) return false;
    const int rows = row_hi - row_lo;
    if (rows <= 0 || batch.count <= 0 || batch.members <= 0) return true;
    if (hole_lo < row_lo) hole_lo = row_lo;
    if (hole_hi > row_hi) hole_hi = row_hi;
    const bool hole = hole_lo < hole_hi;
    if (hole && hole_lo == row_lo && hole_hi == row_hi) return true;
    const int HL = (T + nv - 1) / nv, VS = 64 - 2 * HL;
    const unsigned nvec = (n + nv - 1) / nv;
    rb_edge = rb_edge < 1 ? rb : (rb_edge > rb ? rb : rb_edge);
    // edge windows: those whose 64 lanes include vector -1 (window 0) or vector kg = n / nv (the last one or two)
    const int nwin = (int)cdiv(nvec, VS), kg = n / nv;
    int first_right = nwin - 1;
    while (first_right > 1 && kg < (first_right - 1) * VS - HL + 64) --first_right;
    if (first_right < 1) first_right = 1;                // a single window is window 0
    TbGrid g;
    g.first_right = first_right;
    g.inner_wins = first_right - 1;
    g.edge_wins = 1 + (nwin - first_right);
    // strips of a window: over the rows, or over the part above the hole and the part below it (none straddles it)
    auto strips = [&](int r) { return hole ? cdiv(hole_lo - row_lo, r) + cdiv(row_hi - hole_hi, r) : cdiv(rows, r); };
    g.hole_lo = hole ? hole_lo : 0;
    g.hole_hi = hole ? hole_hi : 0;
    g.inner_blocks = g.inner_wins * (int)cdiv(strips(rb), 4);
    g.edge_blocks = g.edge_wins * (int)cdiv(strips(rb_edge), 4);
    const dim3 grid(8 * cdiv(g.inner_blocks + g.edge_blocks, 8), 1, batch.count * batch.members), block(256);
    const TbKernel k = (st == STORAGE_F16 ? f16 : f32)[shape];
    hipLaunchKernelGGL(k, grid, block, 0, s, batch, pitch, n, row_lo, row_hi, rb, rb_edge, g, fill ? 1 : 0);
    return true;
}

// tiles of |x0| minima for division mode 3, rows [row_lo, row_hi) within 1..n+1; tb.tiles[k] holds tile_rows(n) x tile_pitch words
// per member: member m's minima lie m * tile_mstride words behind them
void launch_tile_min_abs(hipStream_t s, int st, const TileBatch& tiles, int count, int pitch, int n, int row_lo, int row_hi, int tile_pitch,
                         Members mb, size_t tile_mstride)
{
    if (row_lo < 1) row_lo = 1;
    if (row_hi > n + 1) row_hi = n + 1;
    if (row_hi <= row_lo || count <= 0) return;
    const int tr0 = (row_lo - 1) / kTileRows, tr1 = (row_hi - 2) / kTileRows;
    const dim3 grid(cdiv(cdiv(n, 4), 256), tr1 - tr0 + 1, count * mb.count);
    TileBatch tb = tiles;
    tb.count = count;
    tb.mstride = mb.stride;
    tb.tile_mstride = tile_mstride;
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_tile_min_abs<S>, grid, dim3(256), 0, s, tb, pitch, n, row_lo, row_hi, tr0, tile_pitch));
}

// mismatches of division mode `divmode` against a/beta over all 2^32 inputs are added to *bad; kbeta / yd / hi / lo: the
// constants the mode reads (DivK)
void launch_validate_div(hipStream_t s, int divmode, float beta, float kbeta, double yd, float hi, float lo, unsigned long long* bad)
{
    DivK k;
    k.beta = kbeta;
    k.yd = yd;
    k.hi = hi;
    k.lo = lo;
    const auto f = divmode == 4 ? k_validate_div<4> : divmode == 5 ? k_validate_div<5> : divmode == 3 ? k_validate_div<3> : k_validate_div<2>;
    hipLaunchKernelGGL(f, dim3(8192), dim3(256), 0, s, beta, k, bad);
}

void launch_advect(hipStream_t s, int st, void* d, const void* d0, const void* u, const void* v, int pitch, int n,
                   int row_lo, int row_hi, float dt0, int b, Members mb, const float* mdt0)
{
    if (row_hi <= row_lo) return;
    const dim3 grid(cdiv(n, 1024), row_hi - row_lo, mb.count);
    FLUID_BY_STORAGE_INDEX(st, pitch, n, hipLaunchKernelGGL((k_advect<S, I>), grid, dim3(256), 0, s, (S*)d, (const S*)d0, (const S*)u,
                                                            (const S*)v, pitch, n, row_lo, row_hi, dt0, b, mb.stride, mdt0));
}

void launch_advect2(hipStream_t s, int st, void* da, const void* d0a, int ba, void* db, const void* d0b, int bb, const void* u,
                    const void* v, int pitch, int n, int row_lo, int row_hi, float dt0, Members mb, const float* mdt0)
{
    if (row_hi <= row_lo) return;
    const dim3 grid(cdiv(n, 1024), row_hi - row_lo, mb.count);
    FLUID_BY_STORAGE_INDEX(st, pitch, n, hipLaunchKernelGGL((k_advect2<S, I>), grid, dim3(256), 0, s, (S*)da, (const S*)d0a, ba, (S*)db,
                                                            (const S*)d0b, bb, (const S*)u, (const S*)v, pitch, n, row_lo, row_hi, dt0, mb.stride,
                                                            mdt0));
}

void launch_divergence(hipStream_t s, int st, const void* u, const void* v, void* p, void* div, int pitch, int n,
                       int row_lo, int row_hi, float h, int write_p, float pscale, Members mb)
{
    if (row_hi <= row_lo) return;
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_divergence<S>, dim3(cdiv(n, 256), row_hi - row_lo, mb.count), dim3(256), 0, s,
                                            (const S*)u, (const S*)v, (S*)p, (S*)div, pitch, n, row_lo, row_hi, h,
                                            write_p, pscale, mb.stride));
}

void launch_subtract_gradient(hipStream_t s, int st, void* u, void* v, const void* p, int pitch, int n, int row_lo,
                              int row_hi, float h, float* partials, unsigned int* max_out, float pinv, Members mb)
{
    if (row_hi <= row_lo) return;
    if (max_out && mb.count == 1) {          // (slabs: one member)
        const unsigned per_col = cdiv(n, 256), rows = (unsigned)(row_hi - row_lo);
        const unsigned gy = std::max(1u, std::min(rows, (unsigned)kMaxPartials / per_col));     // a few rows per block
        FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_subtract_gradient_max<S>, dim3(per_col, gy), dim3(256), 0, s, (S*)u, (S*)v,
                                                (const S*)p, pitch, n, row_lo, row_hi, h, partials, pinv));
        hipLaunchKernelGGL(k_max_partials, dim3(1), dim3(256), 0, s, partials, (int)(per_col * gy), max_out);
        return;
    }
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_subtract_gradient<S>, dim3(cdiv(n, 256), row_hi - row_lo, mb.count), dim3(256), 0, s,
                                            (S*)u, (S*)v, (const S*)p, pitch, n, row_lo, row_hi, h, pinv, mb.stride));
}

void launch_gradient_advect(hipStream_t s, int st, void* u, void* v, const void* p, void* d, const void* d0, int pitch, int n,
                            int row_lo, int row_hi, float h, float dt0, int b, float pinv, Members mb, const float* mdt0)
{
    if (row_hi <= row_lo) return;
    const dim3 grid(cdiv(n, 1024), row_hi - row_lo, mb.count);
    FLUID_BY_STORAGE_INDEX(st, pitch, n, hipLaunchKernelGGL((k_gradient_advect<S, I>), grid, dim3(256), 0, s, (S*)u, (S*)v, (const S*)p,
                                                            (S*)d, (const S*)d0, pitch, n, row_lo, row_hi, h, dt0, b, pinv, mb.stride,
                                                            mdt0));
}

void launch_absmax2(hipStream_t s, int st, const void* u, const void* v, int pitch, int n, int row_lo, int row_hi,
                    unsigned int* result, Members mb, int rstride)
{
    if (row_hi <= row_lo) return;
    const unsigned blocks = (unsigned)(row_hi - row_lo) < 1024u ? (unsigned)(row_hi - row_lo) : 1024u;
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_absmax2<S>, dim3(blocks, mb.count), dim3(256), 0, s, (const S*)u, (const S*)v, pitch,
                                            n, row_lo, row_hi, result, mb.stride, rstride));
}

void launch_residual(hipStream_t s, int st, const void* x, const void* x0, int pitch, int n, int row_lo, int row_hi,
                     float alpha, float beta, unsigned int* result, Members mb, int rstride, const float2* mab)
{
    if (row_hi <= row_lo) return;
    const unsigned blocks = (unsigned)(row_hi - row_lo) < 1024u ? (unsigned)(row_hi - row_lo) : 1024u;
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_residual<S>, dim3(blocks, mb.count), dim3(256), 0, s, (const S*)x, (const S*)x0, pitch,
                                            n, row_lo, row_hi, alpha, beta, result, mb.stride, rstride, mab));
}

// sized from the whole launch: blocks x members is a few rounds of the chip whatever the split between the two, so an
// ensemble of small grids fills the GPU as one large grid does; at least one block per member, at most one per row
int moment_blocks(int n, int members)
{
    return std::max(1, std::min(n, kMomentBlocks / std::max(1, members)));
}

void launch_member_moments(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, double2* partials, double2* out)
{
    const int blocks = moment_blocks(n, mb.count);
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_member_moments<S>, dim3(blocks, mb.count), dim3(256), 0, s, (const S*)x, pitch, n, mb.stride,
                                            partials));
    hipLaunchKernelGGL(k_fold_moments, dim3(mb.count), dim3(64), 0, s, partials, blocks, out);
}

// chunks of one member's interior: gram_padded / 4096 fix the cells per chunk, a row is cut into whole chunks and a last
// shorter one
static inline unsigned gram_chunks(int n, int mp)
{
    const int ch = kGramChunkValues / mp;
    return (unsigned)n * (unsigned)((n + ch - 1) / ch);
}

// at most two (MP = 64: 128 VGPRs of accumulators) or four resident blocks per CU, at least one chunk per block
int gram_blocks(int n, int members)
{
    const int mp = gram_padded(members);
    return (int)std::min<unsigned>(gram_chunks(n, mp), mp == 64 ? 512u : 1024u);
}

void launch_member_gram(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, bool centre, double* partials,
                        double* out)
{
    const int mp = gram_padded(mb.count), blocks = gram_blocks(n, mb.count);
    const int cpr = (n + kGramChunkValues / mp - 1) / (kGramChunkValues / mp);
    const unsigned chunks = gram_chunks(n, mp);
#define FLUID_GRAM_CASE(MP)                                                                                                               \
    case MP:                                                                                                                              \
        if (centre)                                                                                                                       \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_member_gram<S, MP, true>), dim3(blocks), dim3(256), 0, s, (const S*)x, pitch, n,   \
                                                    mb.stride, mb.count, inv, cpr, chunks, partials));                                    \
        else                                                                                                                              \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_member_gram<S, MP, false>), dim3(blocks), dim3(256), 0, s, (const S*)x, pitch, n,  \
                                                    mb.stride, mb.count, inv, cpr, chunks, partials));                                    \
        break
    switch (mp) {
        FLUID_GRAM_CASE(8);
        FLUID_GRAM_CASE(16);
        FLUID_GRAM_CASE(32);
        FLUID_GRAM_CASE(64);
    }
#undef FLUID_GRAM_CASE
    hipLaunchKernelGGL(k_fold_gram, dim3(mp * mp / 16), dim3(256), 0, s, partials, blocks, mp, mp / 8, out);
}

// The observing kernels' source argument, inside FLUID_BY_STORAGE: `typed` non-null is the table pts.field indexes, the launch's
// member 0 being member `first_member` of every field; otherwise (x, inv).  LAUNCH names the type SRC and the value src.
#define FLUID_BY_SOURCE(typed, first_member, ...)                                 \
    do {                                                                          \
        if (typed) {                                                              \
            using SRC = FieldOfPoint;                                             \
            const SRC src = {pts.field, *(typed), (unsigned)(first_member)};      \
            __VA_ARGS__;                                                          \
        } else {                                                                  \
            using SRC = OneField<S>;                                              \
            const SRC src = {(const S*)x, inv};                                   \
            __VA_ARGS__;                                                          \
        }                                                                         \
    } while (0)
// ... and of the two Gram launches, which also read a record (`recorded` non-null: st, x, inv and typed are not looked at)
#define FLUID_BY_OBSERVED(st, typed, recorded, ...)                               \
    do {                                                                          \
        if (recorded) {                                                           \
            using S = float;                                                      \
            using SRC = Recorded;                                                 \
            const SRC src = {(recorded)->h, (recorded)->stride};                  \
            __VA_ARGS__;                                                          \
        } else {                                                                  \
            FLUID_BY_STORAGE(st, FLUID_BY_SOURCE(typed, 0, __VA_ARGS__));         \
        }                                                                         \
    } while (0)

void launch_observe_members(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed, int first_member,
                            const ObservationPoints& pts, int first_point, int npoints, float* out, size_t ostride)
{
    const dim3 grid(cdiv((unsigned)npoints, 256), mb.count);
    FLUID_BY_STORAGE(st, FLUID_BY_SOURCE(typed, first_member,
                                         hipLaunchKernelGGL((k_observe_members<S, SRC>), grid, dim3(256), 0, s, src, pitch, mb.stride, pts.tap,
                                                            (const float4*)pts.weight, first_point, npoints, out, ostride)));
}

// as gram_blocks: at most two (MP = 64) or four resident blocks per CU, at least one chunk of 64 points per block
int observation_gram_blocks(int points, int members)
{
    return (int)std::min<unsigned>(cdiv((unsigned)points, kObsChunk), gram_padded(members) == 64 ? 512u : 1024u);
}

void launch_observation_gram(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed,
                             const ObservationPoints& pts, bool centre, const float* obs, const float* sigma, double* partials, double* out,
                             const RecordedValues* recorded)
{
    const int mp = gram_padded(mb.count), blocks = observation_gram_blocks(pts.count, mb.count);
    const unsigned chunks = cdiv((unsigned)pts.count, kObsChunk);
#define FLUID_OBS_GRAM_LAUNCH(MP, CENTRE, OBS)                                                                                             \
    FLUID_BY_OBSERVED(st, typed, recorded,                                                                                                 \
                      hipLaunchKernelGGL((k_observation_gram<S, MP, CENTRE, OBS, SRC>), dim3(blocks), dim3(256), 0, s, src, pitch, mb.stride,      \
                                         mb.count, pts.tap, (const float4*)pts.weight, obs, sigma, pts.count, chunks, partials))
#define FLUID_OBS_GRAM_CASE(MP)                                     \
    case MP:                                                        \
        if (centre && obs) FLUID_OBS_GRAM_LAUNCH(MP, true, true);   \
        else if (centre) FLUID_OBS_GRAM_LAUNCH(MP, true, false);    \
        else if (obs) FLUID_OBS_GRAM_LAUNCH(MP, false, true);       \
        else FLUID_OBS_GRAM_LAUNCH(MP, false, false);               \
        break
    switch (mp) {
        FLUID_OBS_GRAM_CASE(8);
        FLUID_OBS_GRAM_CASE(16);
        FLUID_OBS_GRAM_CASE(32);
        FLUID_OBS_GRAM_CASE(64);
    }
#undef FLUID_OBS_GRAM_CASE
#undef FLUID_OBS_GRAM_LAUNCH
    hipLaunchKernelGGL(k_fold_observation_gram, dim3(cdiv((unsigned)observation_gram_entries(mb.count), 16)), dim3(256), 0, s, partials,
                       blocks, mp, mp / 8, obs ? 1 : 0, out);
}

void launch_observation_gram_lattice(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed,
                                     const ObservationPoints& pts, bool centre, const float* obs, const float* sigma, double* operands, const LatticeLists& lists,
                                     double* out, const RecordedValues* recorded)
{
    const int mp = gram_padded(mb.count);
    const unsigned chunks = cdiv((unsigned)pts.count, kObsChunk);
#define FLUID_OBS_OPERANDS_LAUNCH(MP, CENTRE, OBS)                                                                                         \
    FLUID_BY_OBSERVED(st, typed, recorded,                                                                                                 \
                      hipLaunchKernelGGL((k_observation_operands<S, MP, CENTRE, OBS, SRC>), dim3(chunks), dim3(256), 0, s, src, pitch, mb.stride,  \
                                         mb.count, pts.tap, (const float4*)pts.weight, obs, sigma, pts.count, operands))
#define FLUID_LATTICE_GRAM_CASE(MP)                                                                                                        \
    case MP:                                                                                                                               \
        if (centre && obs) FLUID_OBS_OPERANDS_LAUNCH(MP, true, true);                                                                      \
        else if (centre) FLUID_OBS_OPERANDS_LAUNCH(MP, true, false);                                                                       \
        else if (obs) FLUID_OBS_OPERANDS_LAUNCH(MP, false, true);                                                                          \
        else FLUID_OBS_OPERANDS_LAUNCH(MP, false, false);                                                                                  \
        if (obs) hipLaunchKernelGGL((k_lattice_gram<MP, true>), dim3(lists.nodes), dim3(256), 0, s, operands, lists.start, lists.entry, out);  \
        else hipLaunchKernelGGL((k_lattice_gram<MP, false>), dim3(lists.nodes), dim3(256), 0, s, operands, lists.start, lists.entry, out);     \
        break
    switch (mp) {
        FLUID_LATTICE_GRAM_CASE(8);
        FLUID_LATTICE_GRAM_CASE(16);
        FLUID_LATTICE_GRAM_CASE(32);
        FLUID_LATTICE_GRAM_CASE(64);
    }
#undef FLUID_LATTICE_GRAM_CASE
#undef FLUID_OBS_OPERANDS_LAUNCH
}

void launch_observation_screen(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed,
                               const ObservationPoints& pts, const float* obs, const float* sigma, float threshold, const ScreenOutputs& out,
                               const RecordedValues* recorded)
{
    const unsigned chunks = cdiv((unsigned)pts.count, kObsChunk);
    FLUID_BY_OBSERVED(st, typed, recorded,
                      hipLaunchKernelGGL((k_observation_screen<S, SRC>), dim3(chunks), dim3(256), 0, s, src, pitch, mb.stride, mb.count, pts.tap,
                                         (const float4*)pts.weight, obs, sigma, threshold, pts.count, out.sigma, out.mean, out.spread,
                                         out.departure, out.rank, out.flag, out.sums ? out.chunk_sums : nullptr));
    if (out.sums) hipLaunchKernelGGL(k_fold_screen_sums, dim3(1), dim3(64), 0, s, out.chunk_sums, (int)chunks, out.sums);
}

void launch_ensemble_stats(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float* mean, float* var)
{
    const int vw = 16 / (int)storage_bytes(st);
    const int vecs = 1 + (n + 1 + vw - 1) / vw;          // vector 0: ghost column 0; the others: columns 1 .. n + 1
    const unsigned total = (unsigned)(n + 2) * (unsigned)vecs;
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_ensemble_stats<S>, dim3(cdiv(total, 256)), dim3(256), 0, s, (const S*)x, pitch, n, mb.stride,
                                            mb.count, vecs, mean, var));
}

// vectors per row of the scheme of k_ensemble_stats / k_pack_members: ghost column 0, then columns 1 .. n + 1 in whole vectors
static inline int row_vectors(int st, int n)
{
    const int vw = 16 / (int)storage_bytes(st);
    return 1 + (n + 1 + vw - 1) / vw;
}

// vectors per row of k_member_spread / k_relax_spread: ghost column 0, then columns 1 .. n + 1 in vectors of 4 (SpreadVec)
static inline int spread_vectors(int n) { return 1 + (n + 1 + 3) / 4; }

void launch_member_spread(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, float* out)
{
    const int vecs = spread_vectors(n);
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_member_spread<S>, dim3(cdiv((unsigned)(n + 2) * (unsigned)vecs, 256)), dim3(256), 0, s,
                                            (const S*)x, pitch, n, mb.stride, mb.count, vecs, inv, out));
}

void launch_relax_spread(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, float scale, const float* prior,
                         float alpha)
{
    const int vecs = spread_vectors(n);
    FLUID_BY_STORAGE(st, hipLaunchKernelGGL(k_relax_spread<S>, dim3(cdiv((unsigned)(n + 2) * (unsigned)vecs, 256)), dim3(256), 0, s, (S*)x,
                                            pitch, n, mb.stride, mb.count, vecs, inv, scale, prior, (double)alpha));
}

void launch_pack_members(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, float* dense, size_t dstride)
{
    const int vecs = row_vectors(st, n);
    const dim3 grid(cdiv((unsigned)(n + 2) * (unsigned)vecs, 256), mb.count);
    FLUID_BY_STORAGE_INDEX(st, pitch, n, hipLaunchKernelGGL((k_pack_members<S, I>), grid, dim3(256), 0, s, (const S*)x, pitch, n, mb.stride,
                                                            vecs, inv, dense, dstride));
}

void launch_unpack_members(hipStream_t s, int st, void* x, int pitch, int n, Members mb, const float* dense, size_t dstride)
{
    const int vecs = row_vectors(st, n);
    const dim3 grid(cdiv((unsigned)(n + 2) * (unsigned)vecs, 256), mb.count);
    FLUID_BY_STORAGE_INDEX(st, pitch, n, hipLaunchKernelGGL((k_unpack_members<S, I>), grid, dim3(256), 0, s, (S*)x, pitch, n, mb.stride, vecs,
                                                            dense, dstride));
}

// factor: 2, 4, .. 64 and a divisor of n + 2 (fluid_solver checks it; factor 1 is launch_pack_members)
void launch_pack_members_coarse(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, int factor, float* coarse,
                                size_t cstride)
{
    const int vw = 16 / (int)storage_bytes(st);
    const int groups = (n + 2 + vw - 1) / vw;           // block-aligned groups of vw columns per row, column 0 included
    const int lr = __builtin_ctz((unsigned)factor);
    const dim3 grid(cdiv((unsigned)((n + 2) >> lr) * (unsigned)groups, 256), mb.count);
#define FLUID_COARSE_CASE(LR)                                                                                                             \
    case LR:                                                                                                                              \
        FLUID_BY_STORAGE_INDEX(st, pitch, n, hipLaunchKernelGGL((k_pack_members_coarse<S, I, LR>), grid, dim3(256), 0, s, (const S*)x,    \
                                                                pitch, n, mb.stride, groups, inv, coarse, cstride));                      \
        break
    switch (lr) {
        FLUID_COARSE_CASE(1);
        FLUID_COARSE_CASE(2);
        FLUID_COARSE_CASE(3);
        FLUID_COARSE_CASE(4);
        FLUID_COARSE_CASE(5);
        FLUID_COARSE_CASE(6);
    }
#undef FLUID_COARSE_CASE
}

// mb.count in [1, 64] (fluid_solver checks it); `table`: transform_padded(mb.count) doubles per old member; `bits` may be
// null when `dense`
void launch_transform_members(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, const double* table,
                              const unsigned long long* bits, unsigned long long empty, bool dense)
{
    const dim3 grid(cdiv((unsigned)(n + 2), 256), (unsigned)(n + 2));
#define FLUID_TRANSFORM_CASE(MP)                                                                                                           \
    case MP:                                                                                                                               \
        if (dense)                                                                                                                         \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_transform_members<S, MP, true>), grid, dim3(256), 0, s, (S*)x, pitch, n, mb.stride, \
                                                    mb.count, inv, table, bits, empty));                                                   \
        else                                                                                                                               \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_transform_members<S, MP, false>), grid, dim3(256), 0, s, (S*)x, pitch, n, mb.stride, \
                                                    mb.count, inv, table, bits, empty));                                                   \
        break
    switch (transform_padded(mb.count)) {
        FLUID_TRANSFORM_CASE(1);
        FLUID_TRANSFORM_CASE(2);
        FLUID_TRANSFORM_CASE(4);
        FLUID_TRANSFORM_CASE(8);
        FLUID_TRANSFORM_CASE(16);
        FLUID_TRANSFORM_CASE(32);
        FLUID_TRANSFORM_CASE(64);
    }
#undef FLUID_TRANSFORM_CASE
}

// as launch_transform_members; the box is not empty and lies inside the (n + 2)^2 array (fluid_solver checks both)
void launch_transform_members_local(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, float scale,
                                    const double* table, const unsigned long long* bits, unsigned long long used, bool dense,
                                    const float* taper, CellBox box)
{
    const dim3 grid(cdiv((unsigned)(box.col_hi - box.col_lo), 256), (unsigned)(box.row_hi - box.row_lo));
#define FLUID_LOCAL_CASE(MP)                                                                                                             \
    case MP:                                                                                                                             \
        if (dense)                                                                                                                       \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_transform_members_local<S, MP, true>), grid, dim3(256), 0, s, (S*)x, pitch, n + 2, \
                                                    mb.stride, mb.count, inv, scale, table, bits, used, taper, box.row_lo, box.col_lo,   \
                                                    box.col_hi));                                                                        \
        else                                                                                                                             \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_transform_members_local<S, MP, false>), grid, dim3(256), 0, s, (S*)x, pitch,      \
                                                    n + 2, mb.stride, mb.count, inv, scale, table, bits, used, taper, box.row_lo,        \
                                                    box.col_lo, box.col_hi));                                                            \
        break
    switch (transform_padded(mb.count)) {
        FLUID_LOCAL_CASE(1);
        FLUID_LOCAL_CASE(2);
        FLUID_LOCAL_CASE(4);
        FLUID_LOCAL_CASE(8);
        FLUID_LOCAL_CASE(16);
        FLUID_LOCAL_CASE(32);
        FLUID_LOCAL_CASE(64);
    }
#undef FLUID_LOCAL_CASE
}

// as launch_transform_members_local without taper and box; the lattice is valid (fluid_solver checks it): step a positive
// multiple of 8, at least one node each way.  A patch is the widest power of two of columns, up to 64, that divides step.
void launch_transform_members_lattice(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, float scale,
                                      const LatticeTables& t, bool dense, const Lattice& lat)
{
    const int w = n + 2;
    int lpc = 3;
    while (lpc < 6 && lat.step % (2 << lpc) == 0) ++lpc;
    const int pc = 1 << lpc, pr = 64 >> lpc;
    // the first patch starts at or before cell 0, on the origin's phase
    const int col_off = (int)((((long long)lat.col0 % pc) + pc) % pc), row_off = (int)((((long long)lat.row0 % pr) + pr) % pr);
    const int cshift = (pc - col_off) % pc, rshift = (pr - row_off) % pr;
    const dim3 grid(cdiv(cdiv((unsigned)(w + cshift), (unsigned)pc), 4), cdiv((unsigned)(w + rshift), (unsigned)pr));
#define FLUID_LATTICE_CASE(MP)                                                                                                            \
    case MP:                                                                                                                              \
        if (dense)                                                                                                                        \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_transform_members_lattice<S, MP, true>), grid, dim3(256), 0, s, (S*)x, pitch, w,   \
                                                    mb.stride, mb.count, inv, scale, t.table, t.bits, t.cols, lat.nodes_row,              \
                                                    lat.nodes_col, (long long)lat.row0, (long long)lat.col0, lat.step, lpc, rshift,       \
                                                    cshift));                                                                             \
        else                                                                                                                              \
            FLUID_BY_STORAGE(st, hipLaunchKernelGGL((k_transform_members_lattice<S, MP, false>), grid, dim3(256), 0, s, (S*)x, pitch, w,  \
                                                    mb.stride, mb.count, inv, scale, t.table, t.bits, t.cols, lat.nodes_row,              \
                                                    lat.nodes_col, (long long)lat.row0, (long long)lat.col0, lat.step, lpc, rshift,       \
                                                    cshift));                                                                             \
        break
    switch (transform_padded(mb.count)) {
        FLUID_LATTICE_CASE(1);
        FLUID_LATTICE_CASE(2);
        FLUID_LATTICE_CASE(4);
        FLUID_LATTICE_CASE(8);
        FLUID_LATTICE_CASE(16);
        FLUID_LATTICE_CASE(32);
        FLUID_LATTICE_CASE(64);
    }
#undef FLUID_LATTICE_CASE
}

void launch_taper_gaspari_cohn(hipStream_t s, float* out, int n, float col, float row, float c)
{
    const dim3 grid(cdiv((unsigned)(n + 2), 256), (unsigned)(n + 2));
    hipLaunchKernelGGL(k_taper_gaspari_cohn, grid, dim3(256), 0, s, out, n + 2, (double)col, (double)row, (double)c);
}

}  // namespace fluid
