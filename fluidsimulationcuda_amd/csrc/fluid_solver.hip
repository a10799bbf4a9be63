// fluid_solver.hip -- C++ host orchestrator + the extern "C" shim of
// include/fluid_amd.h.  Owns device memory, sequences the kernels of
// fluid_kernels.hip exactly as the reference's vel_step / dens_step do
// (project/sequential/FluidSequential.c:176-241), and drives the row-slab halo
// exchange through a callback when the grid is split over several GPUs.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <mutex>
#include <new>
#include <string>
#include <unordered_map>
#include <vector>

#include "fluid_ctx.h"
#include "fluid_etkf.h"
#include "fluid_noise.h"
#include "fluid_verify.h"
#include "fluid_quantile.h"

namespace fluid_detail {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

// see "fields that are zero by definition" (the RCCL exchange's too: rows travel as they are in memory)
int materialize_zero(fluid_ctx* c, int f)
{
    if (!c->field[f].zero) return FLUID_OK;
    HIP_TRY(hipMemsetAsync(c->ptr(f), 0, c->all_bytes(), c->stream));     // every member: they lie back to back
    c->field[f].zero = false;
    return FLUID_OK;
}

int refuse_ensemble(const fluid_ctx* c, const char* what)
{
    if (c && c->members > 1) return fail(FLUID_E_INVALID, "%s: not available on an ensemble (this context has %d members)", what, c->members);
    return FLUID_OK;
}

}  // namespace fluid_detail

namespace {

using fluid_detail::fail;
using fluid_detail::g_err;
using fluid_detail::materialize_zero;

constexpr size_t kControlBytes = 256;   // tail of the arena: reduction scalar (+0), division-proof counter (+8)
constexpr int kMaxMembers = 21845;   // 3 solves x members blocks in z of the fused Jacobi kernel (HIP: gridDim.z <= 65535)
constexpr int kMaxN = 65533;     // one grid row per blockIdx.y in the pointwise kernels (HIP: gridDim.y <= 65535 = N + 2);
                                 // 65535^2 x 9 fields is 155 GB of the 288 GB, so nothing practical is cut off

}  // namespace

namespace {

using fluid::XOFF;

int check_ctx(const fluid_ctx* c)
{
    if (!c) return fail(FLUID_E_INVALID, "null context");
    return FLUID_OK;
}

int check_fields(const fluid_ctx* c, std::initializer_list<int> ids)
{
    for (int id : ids)
        if (!c->valid_field(id)) return fail(FLUID_E_INVALID, "bad field id %d", id);
    return FLUID_OK;
}

int check_iters(int iters)
{
    if (iters < 0 || (iters & 1)) return fail(FLUID_E_INVALID, "sweep count must be even and >= 0 (got %d)", iters);
    return FLUID_OK;
}

int check_b(int b)
{
    if (b < 0 || b > 2) return fail(FLUID_E_INVALID, "b must be 0, 1 or 2");
    return FLUID_OK;
}

// ---- library-owned scratch (fluid_ctx.h: Scratch) -------------------------------------------------------------------------
// `s` has room for `bytes`, with a pinned twin if one is wanted; *grew: it was allocated anew, and holds nothing.  The one
// place where such memory is allocated, grown and -- short of the context's end -- freed; the contract is in fluid_ctx.h.
int reserve(fluid_ctx* c, Scratch& s, size_t bytes, bool twin, const char* call, const char* what, bool* grew = nullptr)
{
    if (grew) *grew = false;
    if (s.bytes >= bytes && (s.host || !twin)) return FLUID_OK;
    char *dev = nullptr, *host = nullptr;
    hipError_t e = hipMalloc((void**)&dev, bytes);
    if (e == hipSuccess && twin) e = hipHostMalloc((void**)&host, bytes, hipHostMallocDefault);
    if (e == hipSuccess && s.dev) e = hipStreamSynchronize(c->stream);     // launches enqueued so far may still read the old pair
    if (e != hipSuccess) {
        (void)hipGetLastError();
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        return fail(e == hipErrorOutOfMemory ? FLUID_E_NOMEM : FLUID_E_HIP, "%s: allocating %zu bytes of %s: %s", call, bytes, what,
                    hipGetErrorString(e));
    }
    s.release();
    s.dev = dev;
    s.host = host;
    s.bytes = bytes;
    if (grew) *grew = true;
    return FLUID_OK;
}

// an event a buffer's owner records behind the copies out of its twin, made when first needed (fluid_destroy destroys it)
int ensure_event(hipEvent_t* ev)
{
    if (!*ev) HIP_TRY(hipEventCreateWithFlags(ev, hipEventDisableTiming));
    return FLUID_OK;
}

// ---- tables of per-member constants (fluid_ctx.h: ConstRing) -------------------------------------------------------
constexpr size_t kConstAlign = 256, kConstSlots = 8, kConstBlobs = 64;
size_t const_pad(size_t len) { return (len + kConstAlign - 1) / kConstAlign * kConstAlign; }

// the ring and its events, complete after the first fluid_*_members call of a context with more than one member: a call
// that failed part-way leaves what it made to the next one, which makes what is missing
int ensure_consts(fluid_ctx* c)
{
    ConstRing& r = c->consts;
    // the largest table is a batch's: 3 solves x members records; room for kConstSlots of them
    const size_t bytes = std::max<size_t>(64u << 10, kConstSlots * const_pad(3 * (size_t)c->members * sizeof(fluid::TbMemberK)));
    TRY(reserve(c, r.ring, bytes, true, "per-member constants", "tables"));
    while (r.live.size() + r.free_events.size() < kConstBlobs) {
        hipEvent_t ev = nullptr;
        TRY(ensure_event(&ev));
        r.free_events.push_back(ev);
    }
    return FLUID_OK;
}

// *dev: device memory that holds `len` bytes equal to `data` for every launch enqueued on the context's stream from now
// until the next call of this function
int member_consts(fluid_ctx* c, const void* data, size_t len, const void** dev)
{
    ConstRing& r = c->consts;
    if (!r.ring.dev || const_pad(len) * kConstSlots > r.ring.bytes) return fail(FLUID_E_INVALID, "per-member constants: no table (internal)");
    unsigned long long hash = 1469598103934665603ull;
    for (size_t k = 0; k < len; ++k) hash = (hash ^ static_cast<const unsigned char*>(data)[k]) * 1099511628211ull;
    for (const ConstRing::Blob& b : r.live)
        if (b.len == len && b.hash == hash && std::memcmp(r.ring.host + b.off, data, len) == 0) {
            *dev = r.ring.dev + b.off;
            return FLUID_OK;
        }
    if (r.head + const_pad(len) > r.ring.bytes) r.head = 0;
    const size_t lo = r.head, hi = lo + const_pad(len);
    // The tables this one overwrites (and the oldest, if all events are out) leave the ring.  Their device bytes are safe
    // without a wait: the copy below runs behind every launch enqueued so far.  Their host bytes must have been read:
    // that copy was enqueued kConstSlots tables ago, so the wait is a formality unless the queue is that deep.
    for (size_t k = 0; k < r.live.size();) {
        const ConstRing::Blob b = r.live[k];
        const bool overlap = b.off < hi && lo < b.off + const_pad(b.len);
        if (!overlap && !(k == 0 && r.free_events.empty())) {
            ++k;
            continue;
        }
        HIP_TRY(hipEventSynchronize(b.copied));
        r.free_events.push_back(b.copied);
        r.live.erase(r.live.begin() + (ptrdiff_t)k);
    }
    std::memcpy(r.ring.host + lo, data, len);
    HIP_TRY(hipMemcpyAsync(r.ring.dev + lo, r.ring.host + lo, len, hipMemcpyHostToDevice, c->stream));
    hipEvent_t ev = r.free_events.back();
    r.free_events.pop_back();
    HIP_TRY(hipEventRecord(ev, c->stream));
    r.live.push_back({lo, len, hash, ev});
    r.head = hi;
    *dev = r.ring.dev + lo;
    return FLUID_OK;
}

// the single-sweep kernels' {alpha, beta} per member (nullptr: both uniform, the values the launch passes hold)
int member_pairs(fluid_ctx* c, const MemberVal& alpha, const MemberVal& beta, const float2** dev)
{
    *dev = nullptr;
    if (alpha.uniform() && beta.uniform()) return FLUID_OK;
    std::vector<float2> ab(c->members);
    for (int m = 0; m < c->members; ++m) ab[m] = make_float2(alpha.at(m), beta.at(m));
    const void* p = nullptr;
    TRY(member_consts(c, ab.data(), ab.size() * sizeof ab[0], &p));
    *dev = static_cast<const float2*>(p);
    return FLUID_OK;
}

// a device array with one float per member, or nullptr when `v` is uniform (the value the launch passes holds)
int member_floats(fluid_ctx* c, const MemberVal& v, const float** dev)
{
    *dev = nullptr;
    if (v.uniform()) return FLUID_OK;
    const void* p = nullptr;
    TRY(member_consts(c, v.values().data(), v.values().size() * sizeof(float), &p));
    *dev = static_cast<const float*>(p);
    return FLUID_OK;
}

// the bit of fluid_ctx::xowed of the compute stream work is enqueued on now
unsigned stream_bit(const fluid_ctx* c) { return c->stream2 && c->stream == c->stream2 ? 2u : 1u; }

// the current compute stream waits for the exchange in flight, if it still owes that wait; another stream's debt stays
int xchg_join(fluid_ctx* c)
{
    if (!(c->xowed & stream_bit(c))) return FLUID_OK;
    HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_xdone, 0));
    c->xowed &= ~stream_bit(c);
    return FLUID_OK;
}

// Every exchange goes through here.  One issued `async` (slabs, FLUID_PARAM_XCHG_OVERLAP) runs with the exchange stream as
// "the context's stream": behind everything enqueued on the compute stream so far (event), and every compute stream behind
// it again only when that stream calls xchg_join() before it consumes the rows.  A callback that enqueues elsewhere or waits
// on the host (the tests' in-process fabric) is merely not overlapped.  The ranks issue their collectives in one order
// whichever stream each goes to (RCCL serialises a communicator's operations in issue order across streams).
int call_exchange(fluid_ctx* c, int kind, const int* ids, int count, int depth, float* scalar, bool async = false)
{
    // one exchange in flight at a time: this stream joins the earlier one (a debt left on the other waits on the later record)
    TRY(xchg_join(c));
    // An exchange the caller waits for at once stays in line on the compute stream: a hop to another stream and back
    // costs ~10 us each way on this platform (measured: a no-op exchange routed through the second stream leaves the GPU
    // idle for 20 us), which only an exchange that runs beside a launch can pay for.
    if (!async || !c->xstream || !c->xchg_overlap) return c->xchg(c->xchg_user, kind, ids, count, depth, scalar);
    HIP_TRY(hipEventRecord(c->ev_xbegin, c->stream));
    HIP_TRY(hipStreamWaitEvent(c->xstream, c->ev_xbegin, 0));
    hipStream_t compute = c->stream;
    c->stream = c->xstream;
    const int rc = c->xchg(c->xchg_user, kind, ids, count, depth, scalar);
    c->stream = compute;
    if (rc != 0) return rc;
    HIP_TRY(hipEventRecord(c->ev_xdone, c->xstream));
    c->xowed = 3u;                                       // every compute stream: main and stream2
    return 0;
}

int exchange(fluid_ctx* c, int kind, std::initializer_list<int> fields, int depth, float* scalar = nullptr)
{
    if (c->nranks == 1 && !c->rccl) return FLUID_OK;      // (a one-rank communicator may be attached: it is then exercised)
    if (!c->xchg) return fail(FLUID_E_COMM, "multi-GPU context without an exchange callback");
    std::vector<int> ids(fields);
    // the same field listed twice (self-advection) is exchanged once
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    const int rc = call_exchange(c, kind, ids.data(), (int)ids.size(), depth, scalar);
    if (rc != 0) return fail(FLUID_E_COMM, "exchange callback failed (kind %d, rc %d)", kind, rc);
    return FLUID_OK;
}

int reduce_to_host(fluid_ctx* c, float* out)
{
    HIP_TRY(hipMemcpyAsync(c->h_scalar, c->d_scalar, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    float v;
    std::memcpy(&v, c->h_scalar, sizeof v);
    *out = v;
    return FLUID_OK;
}

// ---- timing ---------------------------------------------------------------
int timing_begin(fluid_ctx* c, int cat, hipEvent_t* stop_out)
{
    *stop_out = nullptr;
    if (!c->timing) return FLUID_OK;
    if (c->ev_used == c->ev_pool.size()) {
        fluid_ctx::Ev e{};
        HIP_TRY(hipEventCreate(&e.a));
        HIP_TRY(hipEventCreate(&e.b));
        c->ev_pool.push_back(e);
    }
    auto& p = c->ev_pool[c->ev_used++];
    p.cat = cat;
    p.pressure = cat == FLUID_TIME_DIFFUSION && c->in_pressure_solve;
    HIP_TRY(hipEventRecord(p.a, c->stream));
    *stop_out = p.b;
    return FLUID_OK;
}

int timing_end(fluid_ctx* c, hipEvent_t stop, int sweeps)
{
    if (!stop) return FLUID_OK;
    HIP_TRY(hipEventRecord(stop, c->stream));
    c->pending_sweeps += sweeps;
    if (c->in_pressure_solve) c->pending_pressure_sweeps += sweeps;
    return FLUID_OK;
}

int timing_collect(fluid_ctx* c)
{
    if (c->ev_used == 0) return FLUID_OK;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (c->stream2) HIP_TRY(hipStreamSynchronize(c->stream2));
    for (size_t k = 0; k < c->ev_used; ++k) {
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, c->ev_pool[k].a, c->ev_pool[k].b));
        c->cat_ms[c->ev_pool[k].cat] += ms;
        c->cat_calls[c->ev_pool[k].cat] += 1;
        if (c->ev_pool[k].pressure) c->pressure_ms += ms;
    }
    c->sweeps += c->pending_sweeps;
    c->pending_sweeps = 0;
    c->pressure_sweeps += c->pending_pressure_sweeps;
    c->pending_pressure_sweeps = 0;
    c->ev_used = 0;
    return FLUID_OK;
}

// RAII-free helper: time one operator launch under category `cat`
#define TIMED(c, cat, stmt)                      \
    do {                                         \
        hipEvent_t stop_;                        \
        TRY(timing_begin((c), (cat), &stop_));   \
        stmt;                                    \
        TRY(timing_end((c), stop_, 0));          \
    } while (0)

// Division mode for `beta` in the temporally blocked kernel (fluid_kernels.hip, DIVMODE): 0 = true division,
// 4 = multiply by the exact reciprocal (beta a power of two, alpha 1), 5 = scaled residual correction (four packed
// instructions per pair of cells, any data), 3 = two-term reciprocal where |x0| allows it (hi, lo; two packed
// instructions), 2 = f64 reciprocal multiply (six scalar ones).  Modes 2, 3, 4 and 5 are only
// used after k_validate_div has proven them against a/beta for every one of the 2^32 float inputs on this
// device -- a few ms, once per (mode, beta) and PROCESS: the proof is about the arithmetic of the device
// type, so contexts share it (a fresh context used to spend 3 x 2.5 ms re-proving the step's three betas).
struct DivProofs {
    std::mutex mu;
    std::unordered_map<unsigned long long, int> proven;     // (device, wanted mode, beta bits) -> mode to use
};
DivProofs& div_proofs()
{
    static DivProofs p;
    return p;
}

struct DivPlan {
    int mode = 0;
    float arg = 0.f;      // what the kernel receives as `beta`: beta (0, 2, 3), 1/beta (4)
    float hi = 0.f, lo = 0.f;   // mode 3: the two-term reciprocal; mode 5: beta * 2^24 and -(RN32(1/beta) * 2^-24)
    unsigned tile_thr = 0;      // mode 3: bits of beta * 2^-72, what |x0| must reach on a tile (fluid_kernels.hip, DIVMODE 3)
    double yd = 0.0;      // modes 2, 3
};

float round_down_to_float(double v)
{
    float f = (float)v;
    if ((double)f > v) f = std::nextafterf(f, -INFINITY);
    return f;
}

// `force` (2): the mode to try instead of the best one for this beta -- what a solve whose members disagree settles on
DivPlan division_mode(fluid_ctx* c, float beta, float alpha, int force = 0)
{
    DivPlan plan;
    plan.arg = beta;
    plan.yd = 1.0 / (double)beta;
    if (c->fast_div == 0 || !(beta > 0.f) || !std::isfinite(beta)) return plan;
    int e2 = 0;
    const float rbeta = 1.0f / beta;
    const bool pow2 = std::frexp(beta, &e2) == 0.5f && std::isnormal(rbeta) && rbeta * beta == 1.0f;
    const float hi = round_down_to_float(plan.yd), lo = (float)(plan.yd - (double)hi);
    // mode 4 (pressure solve: alpha 1, beta 4): multiply by the exact reciprocal, and x * 1.0f is x so
    // alpha is not applied at all; else mode 3 when 1/beta splits into two normal floats with lo > 0
    // (not for powers of two: lo = 0 turns inf * lo into NaN); else mode 2, the double-precision reciprocal.
    // A mode that fails its proof hands over to the next: 3 -> 2 -> 0, 4 -> 2 -> 0, 5 -> 2 -> 0.
    const bool two_term = c->fast_div == 1 && c->tiles && beta >= 1.0f && beta <= 0x1p24f && std::isnormal(hi) && std::isnormal(lo) && lo > 0.f;
    // mode 5 (the default for every other beta): r = RN32(1/beta), beta * 2^24 and r * 2^-24 must be ordinary numbers
    const bool residual = c->fast_div == 2 && beta >= 0x1p-60f && beta <= 0x1p60f;
    const float r5_hi = beta * 0x1p24f, r5_lo = -(rbeta * 0x1p-24f);
    int want = force ? force : (pow2 && alpha == 1.0f) ? 4 : two_term ? 3 : residual ? 5 : 2;
    unsigned bits;
    std::memcpy(&bits, &beta, sizeof bits);
    int dev = 0;
    (void)hipGetDevice(&dev);
    DivProofs& proofs = div_proofs();
    std::lock_guard<std::mutex> lock(proofs.mu);
    int mode = 0;
    while (want != 0) {
        const unsigned long long key = ((unsigned long long)(dev & 0xFF) << 40) | ((unsigned long long)want << 32) | bits;
        auto it = proofs.proven.find(key);
        if (it != proofs.proven.end()) {
            mode = it->second;
        } else {
            unsigned long long* bad = reinterpret_cast<unsigned long long*>(c->d_scalar) + 1;   // 8-byte slot of the 256-B block
            unsigned long long* hbad = reinterpret_cast<unsigned long long*>(c->h_scalar) + 1;
            if (hipMemsetAsync(bad, 0, sizeof *bad, c->stream) != hipSuccess) return plan;
            fluid::launch_validate_div(c->stream, want, beta, (want == 4 || want == 5) ? rbeta : beta, plan.yd, want == 5 ? r5_hi : hi,
                                       want == 5 ? r5_lo : lo, bad);
            if (hipMemcpyAsync(hbad, bad, sizeof *bad, hipMemcpyDeviceToHost, c->stream) != hipSuccess ||
                hipStreamSynchronize(c->stream) != hipSuccess)
                return plan;
            mode = *hbad == 0 ? want : 0;
            proofs.proven.emplace(key, mode);
        }
        if (mode != 0) break;
        want = want == 2 ? 0 : 2;
    }
    plan.mode = mode;
    if (mode == 4 || mode == 5) plan.arg = rbeta;
    if (mode == 5) {
        plan.hi = r5_hi;
        plan.lo = r5_lo;
    }
    if (mode == 3) {
        plan.hi = hi;
        plan.lo = lo;
        const float thr = beta * 0x1p-72f;
        std::memcpy(&plan.tile_thr, &thr, sizeof thr);
    }
    return plan;
}

// ---- row-slab bookkeeping ------------------------------------------------------
// FieldState::reach = how many rows beyond each INNER edge of this slab currently hold
// the same values as their owner's copy (kEverywhere: the field is known identical
// on all ranks, e.g. freshly zeroed).  Writers set it (an operator that computes
// `r` rows past the slab leaves reach r), need() raises it with ONE exchange for
// all the fields that fall short.  With one slab everything is a no-op.
constexpr int kEverywhere = 1 << 28;

int exchange_cap(const fluid_ctx* c) { return c->min_slab - 1; }     // rows a neighbour can always supply

void wrote(fluid_ctx* c, int f, int reach)
{
    c->field[f].reach = c->nranks > 1 ? reach : kEverywhere;
    c->field[f].zero = false;
    c->field[f].pend = false;                        // overwritten: whatever the old contents still owed is moot
    c->field[f].src_of = 0;
    c->field[f].fscale = 1.0f;                       // (a writer that keeps a scale sets it again afterwards)
}

// fields a and b trade buffers -- and with them everything recorded about the buffers' contents
void trade(fluid_ctx* c, int a, int b) { std::swap(c->field[a], c->field[b]); }

// `async`: the compute stream does not wait for the rows (call_exchange); the caller's next solve joins them (xchg_join)
int need_list(fluid_ctx* c, const std::vector<int>& fields, int reach, bool async = false)
{
    if (c->nranks == 1 || reach <= 0) return FLUID_OK;
    if (reach > exchange_cap(c)) return fail(FLUID_E_COMM, "halo of %d rows exceeds the slab height", reach);
    std::vector<int> ids;
    for (int f : fields)
        if (c->field[f].reach < reach) ids.push_back(f);
    if (ids.empty()) return FLUID_OK;
    if (!c->xchg) return fail(FLUID_E_COMM, "multi-GPU context without an exchange callback");
    std::sort(ids.begin(), ids.end());
    ids.erase(std::unique(ids.begin(), ids.end()), ids.end());
    c->in_halo_exchange = true;            // rows travel as they are in memory; a pending increment stays pending on every rank alike
    const int rc = call_exchange(c, FLUID_XCHG_HALO, ids.data(), (int)ids.size(), reach, nullptr, async);
    c->in_halo_exchange = false;
    if (rc != 0) return fail(FLUID_E_COMM, "halo exchange failed (rc %d)", rc);
    for (int f : ids) c->field[f].reach = reach;
    return FLUID_OK;
}

int need(fluid_ctx* c, std::initializer_list<int> fields, int reach, bool async = false)
{
    return need_list(c, std::vector<int>(fields), reach, async);
}

// interior rows [lo,hi) this slab computes when it works `reach` rows past its inner edges
void rows(const fluid_ctx* c, int reach, int* lo, int* hi)
{
    *lo = std::max(1, c->own0 - reach);
    *hi = std::min(c->n + 1, c->own1 + reach);
}

// rows(), plus the wall rows where the range reaches them (pointwise kernels treat them as cells, FluidSequential.c:78-82)
void rows_with_walls(const fluid_ctx* c, int reach, int* lo, int* hi)
{
    rows(c, reach, lo, hi);
    if (*lo == 1) *lo = 0;
    if (*hi == c->n + 1) *hi = c->n + 2;
}

// ---- fields that are zero by definition ---------------------------------------------
// The sources of every step after the first and the pressure's first guess are all +0.  Writing those zeros and reading
// them back is pure traffic, so such a field is only MARKED zero (FieldState::zero, mark_zero); the three consumers that
// matter take the mark (add_source adds the constant dt*0, the fused Jacobi kernel reads nothing, the divergence kernel
// skips its p stores) and everything else materialises the zeros first.
// add_source of such a source adds dt*0 to every cell: nothing but the sign of -0 (and NaN/inf rules for a non-finite
// dt), for a read and a write of the whole field.  With the fused Jacobi kernel the increment stays PENDING instead
// (FieldState::pend): the solve that consumes the field as its right-hand side adds it to each row as it loads it, any
// other reader settles it with the real kernel first (here) -- a solve that takes it as its first guess included
// (batch_prepare) -- and a writer that replaces the field drops it (wrote).
int settle_source(fluid_ctx* c, int f);

// a field kept scaled (fscale) goes back to plain values: every row of it, one multiplication by a power of two
int unscale(fluid_ctx* c, int f)
{
    if (c->field[f].fscale == 1.0f) return FLUID_OK;
    const float inv = 1.0f / c->field[f].fscale;
    c->field[f].fscale = 1.0f;
    if (c->field[f].zero) return FLUID_OK;
    fluid::launch_scale(c->stream, c->st, c->ptr(f), c->pitch, 0, c->n + 2, inv, c->mb());
    return FLUID_OK;
}

// x += amount * src on rows [lo, hi) (src null: x += amount), each member by its own amount
int add_source_now(fluid_ctx* c, int x, const void* src, int lo, int hi, const MemberVal& amount)
{
    const float* per_member = nullptr;
    TRY(member_floats(c, amount, &per_member));
    TIMED(c, FLUID_TIME_SOURCE,
          fluid::launch_add_source(c->stream, c->st, c->ptr(x), src, c->pitch, lo, hi, amount.at(0), c->mb(), per_member));
    return FLUID_OK;
}

int settle(fluid_ctx* c, int f, bool keep_scale = false)
{
    if (!keep_scale) TRY(unscale(c, f));
    if (c->field[f].src_of) return settle_source(c, f);
    if (!c->field[f].pend) return FLUID_OK;
    const int reach = c->nranks > 1 ? std::min(c->field[f].reach, exchange_cap(c)) : 0;
    int lo, hi;
    rows_with_walls(c, reach, &lo, &hi);
    TRY(add_source_now(c, f, nullptr, lo, hi, c->field[f].pend_inc));
    c->field[f].pend = false;
    return FLUID_OK;
}

// the deferred add_source of a real source field only (a pending constant increment stays pending: the fused kernel
// applies it on load)
int settle_source(fluid_ctx* c, int f)
{
    if (!c->field[f].src_of) return FLUID_OK;
    // an add_source of a real source field that no diffusion launch took over (see op_add_source): the kernel of its own
    const int s = c->field[f].src_of - 1;
    const int reach = c->nranks > 1 ? std::min({c->field[f].reach, c->field[s].reach, exchange_cap(c)}) : 0;
    int lo, hi;
    rows_with_walls(c, reach, &lo, &hi);
    TRY(add_source_now(c, f, c->ptr(s), lo, hi, c->field[f].src_dt));
    wrote(c, f, reach);                // (src_of = 0)
    return FLUID_OK;
}

int materialize(fluid_ctx* c, int f, bool keep_scale = false)
{
    TRY(materialize_zero(c, f));
    return settle(c, f, keep_scale);
}

int materialize(fluid_ctx* c, std::initializer_list<int> fs)
{
    for (int f : fs) TRY(materialize(c, f));
    return FLUID_OK;
}

void mark_zero(fluid_ctx* c, int f) { wrote(c, f, kEverywhere); c->field[f].zero = true; }

// ---- operators -------------------------------------------------------------------
// `defer` (only the step functions pass it: nothing can touch x or s between this call and the diffusion that follows it
// there): with the fused Jacobi kernel a real source is not added now -- the first launch of the solve whose right-hand
// side x is and whose first guess s is (FluidSequential.c:181, :201, :209: SWAP, then diffuse) reads both fields anyway,
// forms x + dt*s as it loads them and stores the sum out of place (op_diffuse_batch).  Any other reader settles it first.
int op_add_source(fluid_ctx* c, int x, int s, const MemberVal& dt, bool defer = false)
{
    // pointwise: valid as far out as both operands are
    const int reach = c->nranks > 1 ? std::min({c->field[x].reach, c->field[s].reach, exchange_cap(c)}) : 0;
    int lo, hi;
    rows_with_walls(c, reach, &lo, &hi);
    TRY(materialize(c, x));
    if (c->field[s].zero) {
        volatile float z = 0.0f;
        // the reference's dt * s[i] with s[i] = +0 (sign and NaN rules included): +0 or -0 as each member's dt has it
        const MemberVal inc = dt.map([&](float d) { return d * z; });
        if (c->variant == fluid::JACOBI_TB && c->defer_zero_source) {
            c->field[x].pend = true;             // (x was settled just above: one pending increment at a time)
            c->field[x].pend_inc = inc;
            return FLUID_OK;               // x's reach unchanged: nothing was written
        }
        TRY(add_source_now(c, x, nullptr, lo, hi, inc));
    } else {
        TRY(settle(c, s));                 // (a source that is itself owed something: never inside a step)
        if (defer && c->fuse_add_source && c->variant == fluid::JACOBI_TB && fluid::jacobi_tb_exists(-1, -1, c->tb_nv, fluid::TB_ADDSRC)) {
            c->field[x].src_of = 1 + s;
            c->field[x].src_dt = dt;
            return FLUID_OK;               // x's reach unchanged: nothing was written
        }
        TRY(add_source_now(c, x, c->ptr(s), lo, hi, dt));
    }
    wrote(c, x, reach);
    return FLUID_OK;
}

// ---- strip-height tuner -----------------------------------------------------------------------------------
// The fused Jacobi kernel's speed depends on the strip height `rb` in ways no closed form captured (how the
// (window, strip) blocks fall into rounds on the 256 CUs and 8 XCDs, how much pipeline fill they repeat): over a sweep
// of heights the closed-form pick was 10-23 % off the best on most shapes (tools/slab_rb_sweep.py).  Results do not
// depend on rb, so the library measures instead: for each launch shape -- sweeps per launch, fields per launch, form,
// rows, N, lane width, storage -- the first launches cycle through a handful of heights with an event pair around
// each, and once every candidate has two samples the fastest is kept.  The table is shared by all contexts of the
// process (a benchmark can tune in a throw-away context); harvesting is by hipEventQuery, never a wait.
struct RbTuner {
    struct Entry {
        std::vector<int> cand;
        std::vector<float> best_ms;
        std::vector<int> samples, issued;
        int fixed = 0;
        std::string what;             // the launch shape in words (FLUID_TUNE_LOG)
    };
    std::mutex mu;
    std::unordered_map<unsigned long long, Entry> table;
};
RbTuner& rb_tuner()
{
    static RbTuner t;
    return t;
}
constexpr int kTuneSamples = 2;

unsigned long long tune_key(const fluid_ctx* c, int T, int m, int divmode, long long rows_n)
{
    int dev = 0;
    (void)hipGetDevice(&dev);
    unsigned long long h = 1469598103934665603ull;
    for (unsigned long long v : {(unsigned long long)dev, (unsigned long long)c->n, (unsigned long long)rows_n, (unsigned long long)T,
                                 (unsigned long long)m, (unsigned long long)divmode, (unsigned long long)c->tb_nv, (unsigned long long)c->st,
                                 (unsigned long long)c->tb_edge_pct, (unsigned long long)c->tb_fill,
                                 (unsigned long long)c->members}) {      // an ensemble fills the chip: not the heights of one small grid
        h ^= v;
        h *= 1099511628211ull;
    }
    return h;
}

// finished trials -> the table (never waits)
void tune_harvest(fluid_ctx* c)
{
    if (c->trials.empty()) return;
    RbTuner& t = rb_tuner();
    std::lock_guard<std::mutex> lock(t.mu);
    size_t keep = 0;
    for (size_t k = 0; k < c->trials.size(); ++k) {
        fluid_ctx::Trial& tr = c->trials[k];
        if (hipEventQuery(tr.b) != hipSuccess) {
            c->trials[keep++] = tr;
            continue;
        }
        float ms = 0.f;
        auto it = t.table.find(tr.key);
        if (hipEventElapsedTime(&ms, tr.a, tr.b) == hipSuccess && it != t.table.end() && !it->second.fixed) {
            RbTuner::Entry& e = it->second;
            e.best_ms[tr.cand] = e.samples[tr.cand] ? std::min(e.best_ms[tr.cand], ms) : ms;
            e.samples[tr.cand] += 1;
            bool done = true;
            for (int sdone : e.samples) done = done && sdone >= kTuneSamples;
            if (done) {
                e.fixed = e.cand[std::min_element(e.best_ms.begin(), e.best_ms.end()) - e.best_ms.begin()];
                if (std::getenv("FLUID_TUNE_LOG")) {
                    std::string msg;
                    for (size_t q = 0; q < e.cand.size(); ++q) msg += " " + std::to_string(e.cand[q]) + ":" + std::to_string((int)(e.best_ms[q] * 1e3f));
                    fprintf(stderr, "[fluid tune] key %016llx [%s] -> %d rows  (height:us%s)\n", tr.key, e.what.c_str(), e.fixed, msg.c_str());
                }
            }
        }
        c->free_events.push_back(tr.a);
        c->free_events.push_back(tr.b);
    }
    c->trials.resize(keep);
}

// the height to use for this launch; *trial >= 0: it is a measurement of candidate *trial (tune_begin / tune_end bracket the launch)
// (solves, form, divmode: for the shape's name in the log only)
int tune_pick(fluid_ctx* c, unsigned long long key, int heuristic, int T, long long rows_n, int* trial, int solves = 0, int form = 0, int divmode = 0)
{
    *trial = -1;
    tune_harvest(c);
    RbTuner& t = rb_tuner();
    std::lock_guard<std::mutex> lock(t.mu);
    RbTuner::Entry& e = t.table[key];
    if (e.fixed) return e.fixed;
    if (e.cand.empty()) {
        char what[96];
        snprintf(what, sizeof what, "N=%d T=%d solves=%d members=%d form=%d divmode=%d rows=%lld", c->n, T, solves, c->members, form, divmode, rows_n);
        e.what = what;
        e.cand.push_back(heuristic);
        for (int r : {48, 56, 64, 80, 96, 112, 128, 160, 192}) {
            if (r < T || r >= rows_n + 2 * T) continue;         // (a height past the rows is one strip: the tallest candidate covers it)
            if (std::find(e.cand.begin(), e.cand.end(), r) == e.cand.end()) e.cand.push_back(r);
        }
        // a strip repeats about T rows of pipeline fill (FLUID_PARAM_TB_FILL; 2T without it): large grids may gain
        // waves from shorter strips too
        if (rows_n > 2200)
            for (int r : {32, 40})
                if (r >= T && std::find(e.cand.begin(), e.cand.end(), r) == e.cand.end()) e.cand.push_back(r);
        // small grids are bound by the latency of one wave's march, rb + 2T steps: strips shorter than the pipeline is
        // deep pay there (256^2, 8 sweeps per launch: 0.21 ms per step at 4 rows against 0.26 at 16)
        if (rows_n <= 2200)
            for (int r : {2, 4, 8, 12, 24, 32, 40})
                if (r < rows_n && std::find(e.cand.begin(), e.cand.end(), r) == e.cand.end()) e.cand.push_back(r);
        if (e.cand.size() == 1) {                                // nothing to choose from (tiny grids)
            e.fixed = heuristic;
            return heuristic;
        }
        e.best_ms.assign(e.cand.size(), 0.f);
        e.samples.assign(e.cand.size(), 0);
        e.issued.assign(e.cand.size(), 0);
    }
    // the candidate with the fewest trials issued so far (finished or still in flight)
    const int pick = (int)(std::min_element(e.issued.begin(), e.issued.end()) - e.issued.begin());
    if (e.issued[pick] >= kTuneSamples + 2) return e.cand[0];   // all issued, results still in flight: the closed-form pick meanwhile
    e.issued[pick] += 1;
    *trial = pick;
    return e.cand[pick];
}

int tune_begin(fluid_ctx* c, unsigned long long key, int trial)
{
    fluid_ctx::Trial tr{};
    tr.key = key;
    tr.cand = trial;
    for (hipEvent_t* ev : {&tr.a, &tr.b}) {
        if (!c->free_events.empty()) {
            *ev = c->free_events.back();
            c->free_events.pop_back();
        } else {
            HIP_TRY(hipEventCreate(ev));
        }
    }
    HIP_TRY(hipEventRecord(tr.a, c->stream));
    c->trials.push_back(tr);
    return FLUID_OK;
}

int tune_end(fluid_ctx* c)
{
    HIP_TRY(hipEventRecord(c->trials.back().b, c->stream));
    return FLUID_OK;
}

// what pick_sweeps() needs to know of the problem, the same on every rank: `canonical` (fp16 storage: the schedule is part
// of the result, so it derives from the global problem alone and a short reach exchanges early instead of shortening a
// launch; fp32 results do not depend on it), `small` (below FLUID_PARAM_TB_MIN_CELLS: one launch per sweep; default 0,
// the fused kernel wins at every size measured) and `slab_cells` (what a rank sweeps: from the base slab height, not this
// rank's own, so that ranks of an uneven split take the same size-dependent decisions)
struct SweepShape {
    bool canonical, small;
    long long slab_cells;
};

// for `count` solves per launch: fp32 weighs a batch's cells against TB_MIN_CELLS (plans made ahead of a batch pass 1)
// Ensembles: every size here is ONE member's.  fp16 storage must (the schedule is part of the result, and member m has to
// equal a one-member context); for fp32 it is a choice, speed only: the depth rules ("12 and 16 pay from 8 M cells") were
// measured on single grids, where they mark the point at which a field's rows fall out of cache between a strip's stages --
// a property of one member's rows, not of how many members share the launch.  No ensemble measurement backs either choice.
SweepShape sweep_shape(const fluid_ctx* c, int count)
{
    const bool canonical = c->st == fluid::STORAGE_F16;
    const long long slab_cells = (long long)(c->nranks > 1 ? c->min_slab : c->n) * c->n;
    return {canonical, (canonical ? (long long)c->n * c->n : slab_cells * count) < c->tb_min_cells, slab_cells};
}

// Sweeps fused into the next launch of a solve with `remaining` sweeps to go, of which `room` can run before rows must be
// exchanged (slabs; = remaining on one GPU).  Depths 16 / 12 / 8 / 4 / 2 where kTbShapes has them in any division mode
// (16 and 12: 2-column lanes), fp32 storage for 16 and 12.  Per sweep the deep launches are the cheap ones where they pay
// at all, and a shallow remainder is dear (measured, us per sweep of a pressure solve at 4096^2: 4.26 at 16, 4.05 at 12,
// 5.02 at 8; at 8192^2 13.6 / 16.3 / 23.5), so the depths of a solve are PLANNED: the multiset of allowed depths that adds
// up to `remaining` at the least estimated cost, deepest first -- 40 sweeps run as 16 + 12 + 12 rather than 16 + 16 + 8.
//   - 12 pays on grids (or slabs) of 8 M cells and more.  16 too, but for the general form (a double-precision multiply
//     per cell: bound by arithmetic, which deeper blocking only adds to) only once a field outgrows the Infinity Cache
//     (96 MiB rule), and it wants rows: on a 1024-row slab 12 beats it (3.3 against 3.8 us per sweep).
//   - FLUID_PARAM_TB_T16_MIN_CELLS replaces the size rules by one floor (0: always), so that tests can run the deep
//     kernels of either form on grids the oracle finishes in milliseconds.
//   - fp16 storage rounds once per launch, so its schedule is part of the result and stays the greedy 8 / 4 / 2 one.
int pick_sweeps(const fluid_ctx* c, int remaining, int room, const SweepShape& shape, bool all_mode4)
{
    const long long slab_cells = shape.slab_cells;
    // the fused kernel addresses a field through 32-bit buffer offsets: fields of 2 GiB and more
    // (beyond ~23000^2 in fp32) take single-sweep launches
    if (c->variant != fluid::JACOBI_TB || shape.small || c->field_bytes >= 0x7F000000ull) return 1;
    room = std::min(room, remaining);
    const int greedy = (room >= 8 && c->tb_max_t >= 8) ? 8 : (room >= 4 && c->tb_max_t >= 4) ? 4 : room >= 2 ? 2 : 1;
    if (shape.canonical || !fluid::jacobi_tb_exists(12, -1, c->tb_nv, fluid::TB_PLAIN) || c->tb_max_t < 12 || room < 12 || (remaining & 1)) return greedy;
    const bool forced = c->tb_t16_min_cells >= 0;
    const bool big = forced ? slab_cells >= c->tb_t16_min_cells : slab_cells >= (8ll << 20);
    if (!big) return greedy;
    const long long slab_rows = slab_cells / std::max(c->n, 1);
    // 16: the pressure form always; the general form once a field outgrows the Infinity Cache; never on short slabs
    const bool pays16 = forced || ((all_mode4 || (unsigned long long)slab_cells * c->esz > (96ull << 20)) && slab_rows >= 3000);
    const int* depth = fluid::kTbDepths;
    constexpr int nd = (int)std::size(fluid::kTbDepths);
    static const double per_sweep[] = {1.00, 1.04, 1.30, 2.6, 5.0};      // relative cost of one sweep at that depth
    static_assert(std::size(per_sweep) == nd, "one cost per depth");
    const double per_launch = 0.5;
    bool allowed[nd];
    for (int k = 0; k < nd; ++k)
        allowed[k] = depth[k] <= c->tb_max_t && (depth[k] != 16 || pays16) && fluid::jacobi_tb_exists(depth[k], -1, c->tb_nv, fluid::TB_PLAIN);
    // least cost to run exactly r sweeps (r even)
    std::vector<double> cost(remaining + 1, 1e300);
    cost[0] = 0.0;
    for (int r = 2; r <= remaining; r += 2)
        for (int k = 0; k < nd; ++k) {
            if (!allowed[k] || depth[k] > r) continue;
            const double v = cost[r - depth[k]] + depth[k] * per_sweep[k] + per_launch;
            if (v < cost[r] - 1e-9) cost[r] = v;
        }
    // the plan's launches, deepest first; take the deepest one that fits the room
    int best = 0;
    for (int r = remaining; r > 0;) {
        int pickd = 0;
        for (int k = 0; k < nd && !pickd; ++k)
            if (allowed[k] && depth[k] <= r && std::fabs(cost[r - depth[k]] + depth[k] * per_sweep[k] + per_launch - cost[r]) < 1e-9)
                pickd = depth[k];
        if (!pickd) break;
        if (pickd <= room) best = std::max(best, pickd);
        r -= pickd;
    }
    return best ? best : greedy;
}

// One Jacobi solve of the step: field x (first guess in, result out), right-hand
// side x0, wall rule b.  Up to three such solves of the same length run as one
// batch (u, v and density diffusion are independent of one another).
// Its coefficients belong to the caller (a step function, op_diffuse) and outlive the batch; u and v of a step share one
// object, which is how batch_plan knows that they share their division plans too.
struct Coeffs {
    MemberVal alpha, beta;
};

struct Solve {
    int b, x, x0;
    const Coeffs* k;
};

// FluidSequential.c:85-104.  Results land in the fields `x`.  A sweep that writes
// `r` rows past the slab needs x valid r+1 rows out and x0 r rows out, so a solve
// that starts with reach R runs R sweeps before it must exchange again -- on
// ranges that shrink one row per sweep per inner edge, the same arithmetic per
// cell as the 1-GPU run (bit-identical).  `final_reach`: rows past the slab the
// caller would like valid afterwards (the gradient wants 1).  The temporally
// blocked kernel runs T of the sweeps per launch, all solves of the batch in the
// same launch.  Sweeps ping-pong between x's buffer and a scratch field's; if a
// result ends in the scratch buffer the two fields trade buffers (trade(): the
// records swap, no copy) -- field ids, not addresses, are stable.
// `ds` (one GPU, a single pressure solve): the right-hand side sv[0].x0 is the divergence of (ds->u, ds->v), not yet
// computed -- the first launch computes it row by row as it goes and stores it (fluid_kernels.hip, DIVSRC).
struct DivSource {
    int u, v;
    float scale;          // -0.5f * h
};

// One op_diffuse_batch call: its solves, and what its steps -- prepare, plan, the sweep loop, commit -- hand on
struct Batch {
    const Solve* sv;
    int count, iters, final_reach;
    const DivSource* ds;
    int scratch_base;          // a batch beside another on the second stream (full_step) takes the last slots
    const int* scratch;        // each solve's ping-pong partner
    const int* sum;            // where x0 + dt*s of a deferred add_source lands
    int cur[3], nxt[3];        // the fields each solve's next launch reads its guess from / writes to
    std::vector<DivPlan> plan[3];    // per solve: one entry, or with per-member coefficients one per member, all of one mode
    bool same_mode, all_mode4, add_src;   // add_src: the right-hand sides' deferred add_source rides in the first launch
    float out_scale[3];
    SweepShape shape;
};

// a solve's |x0| minima per tile (division mode 3) go with its scratch field: a batch on the second stream has slots of its own
// (per solve AND member: slot s holds `members` tables back to back)
size_t tile_words(const fluid_ctx* c) { return (size_t)fluid::tile_rows(c->n) * fluid::tile_pitch(c->n); }
unsigned* solve_tiles(const fluid_ctx* c, int slot) { return c->tiles + (size_t)slot * c->members * tile_words(c); }

// Division modes across the members of one solve.  The mode is a template parameter of the kernel, so one launch runs one
// mode, and the members of a solve cannot be launched apart (every member goes through the same launches): each member's
// beta is planned as a solve of its own would be (division_mode: proof per distinct beta, cached per process), and the solve
// takes the members' common mode if they agree -- the ordinary case -- and otherwise the most general one proven for every
// member's beta: 2, else 0.  Every mode is exact, so only speed depends on the choice.
void plan_members(fluid_ctx* c, const Coeffs& k, std::vector<DivPlan>& out)
{
    const int M = c->members;
    const MemberVal &alpha = k.alpha, &beta = k.beta;
    out.resize(M);
    bool same = true;
    for (int m = 0; m < M; ++m) {
        out[m] = (m > 0 && beta.at(m) == beta.at(m - 1) && alpha.at(m) == alpha.at(m - 1)) ? out[m - 1] : division_mode(c, beta.at(m), alpha.at(m));
        same = same && out[m].mode == out[0].mode;
    }
    if (same) return;
    bool all2 = true;
    for (int m = 0; m < M; ++m) {
        out[m] = division_mode(c, beta.at(m), alpha.at(m), /*force=*/2);
        all2 = all2 && out[m].mode == 2;
    }
    if (all2) return;
    for (int m = 0; m < M; ++m) {
        out[m] = DivPlan{};
        out[m].arg = beta.at(m);
        out[m].yd = 1.0 / (double)beta.at(m);
    }
}

// argument checks, the scales of the solves reconciled, right-hand sides that are zero by definition materialised
int batch_prepare(fluid_ctx* c, Batch& B)
{
    static const int kScratch[3] = {FLUID_TMP0, FLUID_TMP1, FLUID_TMP2};
    static const int kSum[3] = {FLUID_TMP3, FLUID_TMP4, FLUID_TMP5};
    const Solve* sv = B.sv;
    if (B.scratch_base < 0 || B.scratch_base + B.count > 3) return fail(FLUID_E_INVALID, "a batch holds 1 to 3 solves");
    B.scratch = kScratch + B.scratch_base;
    B.sum = kSum + B.scratch_base;
    TRY(check_iters(B.iters));
    if (B.count < 1 || B.count > 3) return fail(FLUID_E_INVALID, "a batch holds 1 to 3 solves");
    for (int k = 0; k < B.count; ++k) {
        if (sv[k].x == sv[k].x0 || sv[k].x >= FLUID_TMP0 || sv[k].x0 >= FLUID_TMP0)
            return fail(FLUID_E_INVALID, "diffuse: x and x0 must be distinct non-scratch fields");
        for (int j = 0; j < k; ++j)
            if (sv[j].x == sv[k].x || sv[j].x == sv[k].x0 || sv[j].x0 == sv[k].x)
                return fail(FLUID_E_INVALID, "diffuse: the solves of a batch must not share fields");
    }
    // The solve is linear in (x, x0): a right-hand side kept scaled (fp16 storage: the divergence, project()) gives a
    // solution with the same factor, provided the first guess carries it too (a guess that is zero by definition does)
    for (int k = 0; k < B.count; ++k) {
        const FieldState &x = c->field[sv[k].x], &x0 = c->field[sv[k].x0];
        if ((x.zero ? x0.fscale : x.fscale) != x0.fscale || x0.src_of) {
            if (x.fscale != 1.0f || x0.fscale != 1.0f) TRY(xchg_join(c));
            TRY(unscale(c, sv[k].x));
            TRY(unscale(c, sv[k].x0));
        }
        B.out_scale[k] = x0.fscale;
    }
    if (B.iters == 0) {
        TRY(xchg_join(c));
        for (int k = 0; k < B.count; ++k) TRY(settle_source(c, sv[k].x0));    // (no launch to take a deferred source over)
        return FLUID_OK;
    }
    for (int k = 0; k < B.count; ++k) TRY(materialize_zero(c, sv[k].x0));     // a pending increment rides along (TbBatch::x0_inc)
    // A first guess has no such path: the fused kernel reads x as it is in memory.  It is pending only after
    // fluid_op_add_source of a zero source (in a step the pending field is always the right-hand side), so settle it here
    for (int k = 0; k < B.count; ++k)
        if (c->field[sv[k].x].pend) {
            TRY(xchg_join(c));                    // (its kernel touches rows that may be on their way)
            TRY(settle(c, sv[k].x, /*keep_scale=*/true));
        }
    return FLUID_OK;
}

// division modes, whether a deferred add_source rides in the first launch (else it is settled now), mode 3's tile minima
int batch_plan(fluid_ctx* c, Batch& B)
{
    const Solve* sv = B.sv;
    B.same_mode = B.all_mode4 = true;
    for (int k = 0; k < B.count; ++k) {
        B.cur[k] = sv[k].x;
        B.nxt[k] = B.scratch[k];
        const Coeffs& co = *sv[k].k;
        if (k > 0 && sv[k].k == sv[k - 1].k) {
            B.plan[k] = B.plan[k - 1];                               // (u and v)
        } else if (c->variant != fluid::JACOBI_TB) {
            B.plan[k].assign(1, DivPlan{});                          // (true division, by the kernels of one sweep)
            B.plan[k][0].arg = co.beta.at(0);
        } else if (co.alpha.uniform() && co.beta.uniform()) {
            B.plan[k].assign(1, division_mode(c, co.beta.at(0), co.alpha.at(0)));
        } else {
            plan_members(c, co, B.plan[k]);
        }
        B.same_mode = B.same_mode && B.plan[k][0].mode == B.plan[0][0].mode;
        B.all_mode4 = B.all_mode4 && B.plan[k][0].mode == 4;
    }
    B.shape = sweep_shape(c, B.count);
    // a deferred add_source (op_add_source) rides in the first launch if that is a fused one of a shape that exists with the
    // second store, the source is this solve's first guess and all solves agree.  That depth: what the loop picks when
    // nothing is short (a short reach there exchanges first, or shortens the launch and the source is settled there)
    const FieldState& x00 = c->field[sv[0].x0];
    bool add_src = x00.src_of != 0 && B.ds == nullptr && B.same_mode;
    for (int k = 0; k < B.count; ++k) {
        const FieldState &x = c->field[sv[k].x], &x0 = c->field[sv[k].x0];
        add_src = add_src && x0.src_of == 1 + sv[k].x && x0.src_dt == x00.src_dt && !x.zero && !x.pend && !x.src_of;
    }
    B.add_src = add_src && fluid::jacobi_tb_exists(pick_sweeps(c, B.iters, B.iters, B.shape, B.all_mode4), B.plan[0][0].mode, c->tb_nv, fluid::TB_ADDSRC);
    if (!B.add_src)
        for (int k = 0; k < B.count; ++k)
            if (c->field[sv[k].x0].src_of) {
                TRY(xchg_join(c));                        // (its kernel touches rows that may be on their way)
                TRY(settle_source(c, sv[k].x0));
            }
    // division mode 3 needs |x0| >= beta * 2^-72 wherever it is used: minima of |x0| per tile, once per solve (x0 does not
    // change during it), over the rows of x0 that are valid here; tiles beyond them read 0 = "divide the long way"
    fluid::TileBatch tb{};
    int m = 0, valid = kEverywhere;
    for (int k = 0; k < B.count; ++k)
        if (B.plan[k][0].mode == 3) {
            tb.field[m] = c->ptr(sv[k].x0);
            tb.tiles[m] = solve_tiles(c, B.scratch_base + k);
            valid = std::min(valid, c->nranks > 1 ? c->field[sv[k].x0].reach : kEverywhere);
            ++m;
        }
    if (m == 0) return FLUID_OK;
    TRY(xchg_join(c));
    if (c->nranks > 1)
        HIP_TRY(hipMemsetAsync(solve_tiles(c, B.scratch_base), 0, (size_t)B.count * c->members * tile_words(c) * sizeof(unsigned), c->stream));
    int lo, hi;
    rows(c, std::min(valid, c->n), &lo, &hi);
    fluid::launch_tile_min_abs(c->stream, c->st, tb, m, c->pitch, c->n, lo, hi, fluid::tile_pitch(c->n), c->mb(), tile_words(c));
    return FLUID_OK;
}

// sweeps the batch can run right now: x is read one row further out than x0
int batch_reach(const fluid_ctx* c, const Batch& B)
{
    int r = kEverywhere;
    for (int k = 0; k < B.count; ++k) r = std::min(r, std::min(c->field[B.cur[k]].reach, c->field[B.sv[k].x0].reach + 1));
    return r;
}

// The constants of (solve j, member m) in one fused launch.  x0_inc: what the launch adds to the right-hand side as it loads
// it; div_scale: the scale of what the launch itself forms (fill_batch).
fluid::TbMemberK solve_constants(const Batch& B, int j, int m, const MemberVal& x0_inc, const MemberVal& div_scale)
{
    const DivPlan& p = B.plan[j][B.plan[j].size() > 1 ? (size_t)m : 0];
    return {p.yd, B.sv[j].k->alpha.at(m), p.arg, p.hi, p.lo, x0_inc.at(m), div_scale.at(m), p.tile_thr, /*pad=*/0};
}

// the fused kernel's arguments for solves [first, last); divsrc / addsrc: the launch forms (and stores) the right-hand sides
int fill_batch(fluid_ctx* c, const Batch& B, int first, int last, bool divsrc, bool addsrc, fluid::TbBatch* out)
{
    static const MemberVal nothing_pending(-0.0f);                   // x + (-0) is x for every x
    // ADDSRC: each member's dt (batch_plan: the same for all solves); DIVSRC: the divergence's factor
    const MemberVal own_scale(divsrc ? B.ds->scale : 0.0f);
    const MemberVal& div_scale = addsrc ? c->field[B.sv[first].x0].src_dt : own_scale;
    const MemberVal* x0_inc[3];
    fluid::TbBatch bt{};
    bool per_member = !div_scale.uniform();
    for (int j = first; j < last; ++j) {
        const int q = j - first;
        const FieldState& x0 = c->field[B.sv[j].x0];
        // a pending increment rides in every launch of the solve but one that forms the right-hand side itself
        x0_inc[q] = x0.pend && !addsrc && !divsrc ? &x0.pend_inc : &nothing_pending;
        per_member = per_member || B.plan[j].size() > 1 || !x0_inc[q]->uniform();
        const fluid::TbMemberK k0 = solve_constants(B, j, 0, *x0_inc[q], div_scale);
        bt.x[q] = c->ptr(B.cur[j]);
        bt.x0[q] = x0.ptr;
        bt.out[q] = c->ptr(B.nxt[j]);
        bt.alpha[q] = k0.alpha;
        bt.beta[q] = k0.beta;
        bt.yd[q] = k0.yd;
        bt.hi[q] = k0.hi;
        bt.lo[q] = k0.lo;
        bt.tiles[q] = B.plan[j][0].mode == 3 ? solve_tiles(c, B.scratch_base + j) : nullptr;
        bt.tile_thr[q] = k0.tile_thr;
        bt.b[q] = B.sv[j].b;
        bt.x_zero[q] = c->field[B.cur[j]].zero ? 1 : 0;
        bt.x0_inc[q] = k0.x0_inc;
        if (addsrc) bt.div[q] = c->ptr(B.sum[j]);
    }
    bt.count = last - first;
    bt.members = c->members;
    bt.mstride = c->field_floats;
    bt.tile_mstride = tile_words(c);
    bt.tile_pitch = fluid::tile_pitch(c->n);
    bt.div_scale = div_scale.at(0);
    if (divsrc) {
        bt.x[0] = c->ptr(B.ds->u);
        bt.x0[0] = c->ptr(B.ds->v);
        bt.div[0] = c->ptr(B.sv[0].x0);
    }
    // something differs from member to member (fluid_*_members): the constants above, once per (solve, member), in a table
    if (per_member && c->members > 1) {
        const int M = c->members;
        std::vector<fluid::TbMemberK> rec((size_t)bt.count * M);
        for (int j = first; j < last; ++j)
            for (int m = 0; m < M; ++m) rec[(size_t)(j - first) * M + m] = solve_constants(B, j, m, *x0_inc[j - first], div_scale);
        const void* dev = nullptr;
        TRY(member_consts(c, rec.data(), rec.size() * sizeof rec[0], &dev));
        bt.mk = static_cast<const fluid::TbMemberK*>(dev);
    }
    *out = bt;
    return FLUID_OK;
}

// strip height of the two edge windows (ghost columns cost ~1.6x per row: shorter strips there keep the launch balanced)
int edge_rows(const fluid_ctx* c, int T, int rb) { return std::max(2 * T, rb * (c->tb_edge_pct > 0 ? c->tb_edge_pct : 100) / 100); }

// Closed-form strip height of a fused launch of m solves, T sweeps, rows_n output rows (tools/tb_sweep.py on MI355X): the
// kernel hides its latencies only behind other waves, so every block should be resident at once (a 256-thread block is one
// wave per SIMD), in the tallest strips that allow (a strip of rb rows marches rb + T - 1 rows of stages with
// FLUID_PARAM_TB_FILL, rb + 2T without): the smallest height from T (2T without) whose blocks fit 92 % of one round;
// grids too large for one round stop at 80 rows (160 for a batch; 192 at T = 16).
int strip_rows(const fluid_ctx* c, int T, int m, long long rows_n)
{
    const int nv = c->tb_nv;
    const int HL = (T + nv - 1) / nv, VS = 64 - 2 * HL;
    const long long windows = ((c->n + nv - 1) / nv + VS - 1) / VS;
    const long long inner = windows > 2 ? windows - 2 : 0, outer = windows - inner;
    const int resident = nv == 2 ? (T >= 16 ? 2 : 4) : (T >= 8 ? 2 : 3);
    const long long room = (long long)c->num_cu * resident * 92 / 100;
    const int cap = T >= 16 ? 192 : (T >= 8 ? 80 : 96) * (m > 1 ? 2 : 1);
    int rb = c->tb_fill ? T : 2 * T;
    auto fits = [&](int r) {
        const long long si = (rows_n + r - 1) / r, se = (rows_n + edge_rows(c, T, r) - 1) / edge_rows(c, T, r);
        return (inner * ((si + 3) / 4) + outer * ((se + 3) / 4)) * m <= room;
    };
    for (; rb < cap; rb += 2)
        if (fits(rb)) break;
    // small grids: a launch lasts as long as one wave's march of rb + T - 1 rows (rb + 2T), and the best height
    // measured is about rows / 64 (2 at 128^2, 4 at 256^2, 8 at 512^2, 16 and more from 1024^2).
    // An ensemble (m = solves x members) whose blocks no longer fit one round at that height is not waiting for one wave's
    // march any more: it keeps the tall strips of the loop above, which repeat less pipeline fill.  (Closed form only: the
    // tuner measures short and tall candidates alike)
    if (rows_n <= 1100) {
        const int low = std::max(2, std::min(rb, (int)(rows_n / 64) & ~1));
        if (c->members == 1 || fits(low)) rb = low;
        else rb = (int)std::min<long long>(rb, std::max<long long>(low, (rows_n + 1) & ~1ll));      // (no taller than the rows there are)
    }
    return rb;
}

// A fused launch of the sweep loop; strip height TB_ROWS, else the closed form as the run-time tuner's first candidate
// (RbTuner).  While this stream owes the wait on an exchange in flight, the strips whose inputs are this slab's own rows --
// output rows [own0 + T, own1 - T): T sweeps reach T rows -- go first and run while the halo rows travel; the strips next to
// the inner edges wait for the exchange's event, in one launch.  Same arithmetic per cell whichever launch it falls into.
int launch_fused(fluid_ctx* c, const fluid::TbBatch& bt, int T, int divmode, bool divsrc, bool addsrc, int lo, int hi)
{
    const bool owed = c->nranks > 1 && (c->xowed & stream_bit(c));
    const int in_lo = owed && c->rank > 0 ? std::max(lo, c->own0 + T) : lo;
    const int in_hi = owed && c->rank < c->nranks - 1 ? std::min(hi, c->own1 - T) : hi;
    const bool split = owed && in_hi - in_lo >= 2 * T && (in_lo > lo || in_hi < hi);
    const int form = divsrc ? fluid::TB_DIVSRC : addsrc ? fluid::TB_ADDSRC : fluid::TB_PLAIN;
    for (int part = split ? 0 : 1; part < 2; ++part) {     // 0: the interior of a split launch; 1: the rest (or all)
        const int plo = part ? lo : in_lo, phi = part ? hi : in_hi;
        const int hole_lo = part && split ? in_lo : 0, hole_hi = part && split ? in_hi : 0;
        if (part) TRY(xchg_join(c));
        const long long rows_n = (phi - plo) - std::max(0, hole_hi - hole_lo);
        int rb = c->tb_rows > 0 ? c->tb_rows : strip_rows(c, T, bt.count * c->members, rows_n);   // solves per launch: every member's
        int trial = -1;
        unsigned long long key = 0;
        if (c->tb_rows <= 0 && c->autotune) {
            // (the two edge parts of a split launch: keyed by their rows, and as a shape of their own)
            key = tune_key(c, T, bt.count + (divsrc ? 8 : 0) + (addsrc ? 16 : 0) + (hole_hi > hole_lo ? 32 : 0), divmode, rows_n);
            rb = tune_pick(c, key, rb, T, rows_n, &trial, bt.count, form, divmode);
        }
        if (trial >= 0) TRY(tune_begin(c, key, trial));
        if (!fluid::launch_jacobi_tb(c->stream, c->st, T, divmode, c->tb_nv, form, bt, c->pitch, c->n, plo, phi, rb,
                                     std::min(rb, edge_rows(c, T, rb)), hole_lo, hole_hi, c->tb_fill))
            return fail(FLUID_E_INVALID, "no fused Jacobi kernel: %d sweeps, division mode %d, %d-column lanes, form %d", T, divmode, c->tb_nv, form);
        if (trial >= 0) TRY(tune_end(c));
    }
    if (split) c->split_launches += 1;
    return FLUID_OK;
}

// the state a launch of the sweep loop leaves: `r` rows past the slab valid (kEverywhere: one GPU); `first`: the solves' first
void commit_launch(fluid_ctx* c, Batch& B, bool first, int r)
{
    if (B.ds && first && c->nranks > 1)             // the divergence exists where this launch stored it
        c->field[B.sv[0].x0].reach = std::max(0, std::min(c->field[B.sv[0].x0].reach, r));
    if (B.add_src && first) {
        // the sums were stored out of place, on the rows this launch computed (+ the wall rows next to them): the
        // right-hand side takes that buffer, the sum field the old one
        for (int j = 0; j < B.count; ++j) {
            trade(c, B.sv[j].x0, B.sum[j]);
            wrote(c, B.sum[j], 0);
            wrote(c, B.sv[j].x0, std::max(0, r));
        }
        B.add_src = false;
    }
    for (int j = 0; j < B.count; ++j) {
        c->field[B.cur[j]].zero = false;             // from now on this buffer is just the other half of the ping-pong
        wrote(c, B.nxt[j], r);
        std::swap(B.cur[j], B.nxt[j]);
    }
}

// the sweep loop: launches of T sweeps each, an exchange first whenever the valid rows run short
int batch_sweep(fluid_ctx* c, Batch& B)
{
    const Solve* sv = B.sv;
    const bool multi = c->nranks > 1, canonical = B.shape.canonical;
    int r = multi ? batch_reach(c, B) : kEverywhere;
    for (int k = 0; k < B.iters;) {
        const int remaining = B.iters - k;
        const int wantT = canonical ? pick_sweeps(c, remaining, remaining, B.shape, B.all_mode4) : 1;   // slabs with fp16 storage keep halo >= 8 (fluid_create_ex)
        if (r < wantT) {
            const int depth = std::max(wantT, std::min(c->halo, remaining + B.final_reach));
            std::vector<int> ids;
            for (int j = 0; j < B.count; ++j) {
                ids.push_back(B.cur[j]);
                if (c->field[sv[j].x0].reach < depth - 1) ids.push_back(sv[j].x0);
            }
            TRY(xchg_join(c));                                // (the caller's exchange first, if it is still out)
            TRY(need_list(c, ids, depth, /*async=*/true));    // the launch below is split around it
            r = batch_reach(c, B);
        }
        const int T = canonical ? wantT : pick_sweeps(c, remaining, std::min(r, remaining), B.shape, B.all_mode4);
        if (B.add_src && k == 0 && !fluid::jacobi_tb_exists(T, B.plan[0][0].mode, c->tb_nv, fluid::TB_ADDSRC)) {
            B.add_src = false;                   // a shallower first launch than planned (short reach): the kernel of its own after all
            TRY(xchg_join(c));
            for (int j = 0; j < B.count; ++j) TRY(settle_source(c, sv[j].x0));
        }
        int lo, hi;
        rows(c, multi ? std::min(r - T, exchange_cap(c)) : 0, &lo, &hi);
        if (T == 1) {
            // the single-sweep kernels, one launch per solve, read x and x0 as they are in memory
            const int v = c->variant == fluid::JACOBI_TB ? (B.shape.small ? fluid::JACOBI_NAIVE : fluid::JACOBI_STREAM) : c->variant;
            TRY(xchg_join(c));
            for (int j = 0; j < B.count; ++j) TRY(materialize(c, B.cur[j], /*keep_scale=*/true));
            for (int j = 0; j < B.count; ++j) TRY(settle(c, sv[j].x0, /*keep_scale=*/true));
            for (int j = 0; j < B.count; ++j) {
                const float2* mab = nullptr;
                TRY(member_pairs(c, sv[j].k->alpha, sv[j].k->beta, &mab));
                fluid::launch_jacobi(c->stream, c->st, v, c->ptr(B.cur[j]), c->ptr(sv[j].x0), c->ptr(B.nxt[j]), c->pitch, c->n, lo, hi,
                                     sv[j].k->alpha.at(0), sv[j].k->beta.at(0), sv[j].b, c->mb(), mab);
            }
            if (c->timing) {
                c->launches += B.count;
                c->field_launches += (long long)B.count * c->members;
            }
        } else {
            // one launch per group of solves that share a division mode (normally: all of them)
            for (int first = 0, last; first < B.count; first = last) {
                last = B.same_mode ? B.count : first + 1;
                const bool divsrc = B.ds != nullptr && k == 0, addsrc = B.add_src && k == 0;
                fluid::TbBatch bt;
                TRY(fill_batch(c, B, first, last, divsrc, addsrc, &bt));
                TRY(launch_fused(c, bt, T, B.plan[first][0].mode, divsrc, addsrc, lo, hi));
                if (c->timing) {
                    c->launches += 1;
                    c->field_launches += (long long)(last - first) * c->members;
                }
            }
        }
        r = multi ? std::min(r - T, exchange_cap(c)) : kEverywhere;
        commit_launch(c, B, k == 0, r);
        k += T;
    }
    return FLUID_OK;
}

int op_diffuse_batch(fluid_ctx* c, const Solve* sv, int count, int iters, int final_reach = 0, const DivSource* ds = nullptr,
                     int scratch_base = 0)
{
    Batch B{sv, count, iters, final_reach, ds, scratch_base};
    TRY(batch_prepare(c, B));
    if (iters == 0) return FLUID_OK;
    hipEvent_t stop;
    TRY(timing_begin(c, FLUID_TIME_DIFFUSION, &stop));
    TRY(batch_plan(c, B));
    TRY(batch_sweep(c, B));
    HIP_TRY(hipGetLastError());
    // commit: a result that ended in the scratch buffer takes it over (its record with it)
    for (int j = 0; j < count; ++j) {
        if (B.cur[j] != sv[j].x) trade(c, sv[j].x, B.scratch[j]);
        wrote(c, B.scratch[j], 0);
        c->field[sv[j].x].fscale = B.out_scale[j];
    }
    return timing_end(c, stop, iters * count * c->members);
}

int op_diffuse(fluid_ctx* c, int b, int x, int x0, const Coeffs& k, int iters, int final_reach = 0, const DivSource* ds = nullptr)
{
    const Solve one{b, x, x0, &k};
    return op_diffuse_batch(c, &one, 1, iters, final_reach, ds);
}

// FluidSequential.c:107-141.  The back-trace reaches dt0*max|vel| cells, so a
// slab first learns the global bound (wavefront reduction + MAX exchange) and
// makes sure that many rows of the advected field(s) are valid past its edges;
// when the reach exceeds what a neighbour can supply it gathers whole fields.
// The bound is a host decision, i.e. a pipeline drain: vmax_begin() only
// enqueues (reduction kernel, device-side all-reduce, copy to pinned memory),
// so the caller can put independent work behind it before advect_rows() waits.
// `have_max`: the gradient subtraction that has just produced (u, v) left their maximum in the device word already
// (op_subtract_gradient with_max)
int vmax_begin(fluid_ctx* c, int u, int v, bool have_max = false)
{
    if (c->nranks == 1) return FLUID_OK;
    if (!have_max) {
        TRY(materialize(c, {u, v}));
        HIP_TRY(hipMemsetAsync(c->d_scalar, 0, sizeof(unsigned), c->stream));
        fluid::launch_absmax2(c->stream, c->st, c->ptr(u), c->ptr(v), c->pitch, c->n, c->own0, c->own1, c->d_scalar, c->mb());
    }
    TRY(exchange(c, FLUID_XCHG_MAX_BEGIN, {}, 0));       // in-place MAX over ranks on the device scalar
    HIP_TRY(hipMemcpyAsync(c->h_scalar, c->d_scalar, sizeof(unsigned), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipEventRecord(c->scalar_ready, c->stream));
    return FLUID_OK;
}

// slabs: waits for the bound vmax_begin() enqueued (*vmax) and brings in the rows of `sources` an advection along it reads
// (whole fields beyond a neighbour's reach) unless the `have` rows already there cover them -- *fetched: rows came in here
int advect_rows(fluid_ctx* c, std::initializer_list<int> sources, float dt0, int have, float* vmax, bool* fetched)
{
    HIP_TRY(hipEventSynchronize(c->scalar_ready));
    std::memcpy(vmax, c->h_scalar, sizeof *vmax);
    TRY(exchange(c, FLUID_XCHG_MAX_END, {}, 0, vmax));  // transports that reduce on the host finish here
    const double reach = std::ceil((double)std::fabs(dt0) * (double)*vmax) + 2.0;
    *fetched = !(have > 0 && reach <= (double)have);
    if (!*fetched) return FLUID_OK;
    if (reach <= (double)exchange_cap(c)) return need(c, sources, (int)reach);
    TRY(exchange(c, FLUID_XCHG_GATHER, sources, 0));     // (also NaN / inf)
    for (int f : sources) c->field[f].reach = kEverywhere;
    return FLUID_OK;
}

// vmax_begin() has been enqueued; `run` enqueues the advection of `sources` (FluidSequential.c:107-141) along that velocity.
// The classic order -- wait for the bound, bring in that many rows, advect -- leaves the GPU idle while the host reads the
// bound and enqueues the rest.  Velocities change little from step to step, so with a bound from the previous step at
// hand (slot 0: the velocity's own advection, 1: the density's) the exchange and the advection are enqueued FIRST, on
// that bound plus a quarter, and the host then checks the new bound against it: the same on every rank (both are
// all-reduced values), so all ranks agree on whether to do it over.  Doing it over is safe: an advection writes fields
// it does not read, and nothing that overwrites its inputs is enqueued before this function returns.
int advect_bounded(fluid_ctx* c, int slot, std::initializer_list<int> sources, float dt0, const std::function<int()>& run)
{
    if (c->nranks == 1) return run();
    int guess = 0;
    const float prev = c->vmax_prev[slot];
    if (c->early_advect && prev >= 0.0f) {
        const double g = std::ceil((double)std::fabs(dt0) * (double)prev * 1.25) + 2.0;
        if (g <= (double)exchange_cap(c)) {
            guess = (int)g;
            TRY(need(c, sources, guess));
            TRY(run());
        }
    }
    float vmax = 0.f;
    bool fetched = false;
    TRY(advect_rows(c, sources, dt0, guess, &vmax, &fetched));
    c->vmax_prev[slot] = std::isfinite(vmax) ? vmax : -1.0f;
    return fetched ? run() : FLUID_OK;
}

// dt0 = dt * N of every member (nullptr: a uniform dt)
int member_dt0(fluid_ctx* c, const MemberVal& dt, const float** dev)
{
    return member_floats(c, dt.map([&](float d) { return d * (float)c->n; }), dev);
}

int op_advect(fluid_ctx* c, int b, int d, int d0, int u, int v, const MemberVal& dt)
{
    if (d == d0 || d == u || d == v) return fail(FLUID_E_INVALID, "advect: output must not alias an input");
    const float dt0 = dt.at(0) * (float)c->n;
    TRY(materialize(c, {d0, u, v}));
    const float* mdt0 = nullptr;
    TRY(member_dt0(c, dt, &mdt0));
    TIMED(c, FLUID_TIME_ADVECTION,
          fluid::launch_advect(c->stream, c->st, c->ptr(d), c->ptr(d0), c->ptr(u), c->ptr(v), c->pitch, c->n, c->own0, c->own1, dt0, b, c->mb(),
                               mdt0));
    wrote(c, d, 0);
    return FLUID_OK;
}

// two advections along the same velocity (u, v) in one launch; results identical to two op_advect calls
int op_advect2(fluid_ctx* c, int ba, int da, int d0a, int bb, int db, int d0b, int u, int v, const MemberVal& dt)
{
    for (int d : {da, db})
        if (d == d0a || d == d0b || d == u || d == v) return fail(FLUID_E_INVALID, "advect: output must not alias an input");
    if (da == db) return fail(FLUID_E_INVALID, "advect: outputs must be distinct");
    const float dt0 = dt.at(0) * (float)c->n;
    TRY(materialize(c, {d0a, d0b, u, v}));
    const float* mdt0 = nullptr;
    TRY(member_dt0(c, dt, &mdt0));
    TIMED(c, FLUID_TIME_ADVECTION,
          fluid::launch_advect2(c->stream, c->st, c->ptr(da), c->ptr(d0a), ba, c->ptr(db), c->ptr(d0b), bb, c->ptr(u), c->ptr(v), c->pitch,
                                c->n, c->own0, c->own1, dt0, c->mb(), mdt0));
    wrote(c, da, 0);
    wrote(c, db, 0);
    return FLUID_OK;
}

// FluidSequential.c:143-158.  `want`: rows past the slab on which the caller
// would like the divergence (so that the pressure solve that follows needs no
// exchange of its own); u and v are brought in one row further than that.
// `pscale`: the divergence is stored multiplied by this power of two (project() with fp16 storage; 1 from the operator API)
int op_divergence(fluid_ctx* c, int u, int v, int p, int div, int want = 0, float pscale = 1.0f)
{
    if (p == u || p == v || div == u || div == v || p == div)
        return fail(FLUID_E_INVALID, "divergence: outputs must not alias inputs");
    const float h = 1.0f / (float)c->n;
    int reach = 0;
    TRY(materialize(c, {u, v}));
    if (c->nranks > 1) {
        reach = std::max(0, std::min(want, exchange_cap(c) - 1));
        TRY(need(c, {u, v}, reach + 1));
    }
    int lo, hi;
    rows(c, reach, &lo, &hi);
    // p = 0 everywhere (FluidSequential.c:153 + set_bnd(0,p)): marked, not written
    TIMED(c, FLUID_TIME_DIVERGENCE,
          fluid::launch_divergence(c->stream, c->st, c->ptr(u), c->ptr(v), c->ptr(p), c->ptr(div), c->pitch, c->n, lo, hi, h,
                                   /*write_p=*/0, pscale, c->mb()));
    wrote(c, div, reach);
    c->field[div].fscale = pscale;
    mark_zero(c, p);
    return FLUID_OK;
}

// `with_max` (slabs): max(|u|, |v|) of the result, over the slab's own rows, is left in the device word for the
// vmax_begin(.., have_max) that follows -- the bound of the advection along (u, v), without a pass of its own
int op_subtract_gradient(fluid_ctx* c, int u, int v, int p, bool with_max = false)
{
    if (p == u || p == v || u == v) return fail(FLUID_E_INVALID, "subtract_gradient: fields must be distinct");
    const float h = 1.0f / (float)c->n;
    TRY(materialize(c, {u, v}));
    TRY(materialize(c, p, /*keep_scale=*/true));           // a scaled pressure is divided back inside the kernel, exactly
    TRY(need(c, {p}, 1));
    with_max = with_max && c->nranks > 1 && c->d_partials;
    TIMED(c, FLUID_TIME_PROJECTION,
          fluid::launch_subtract_gradient(c->stream, c->st, c->ptr(u), c->ptr(v), c->ptr(p), c->pitch, c->n, c->own0, c->own1, h,
                                          c->d_partials, with_max ? c->d_scalar : nullptr, 1.0f / c->field[p].fscale, c->mb()));
    wrote(c, u, 0);
    wrote(c, v, 0);
    return FLUID_OK;
}

// the gradient subtraction of a projection and the advection of `d` (from d0, wall rule b) along the projected velocity,
// in one launch: results identical to op_subtract_gradient followed by op_advect.  One GPU only (on slabs the advection
// waits for a reduction over the velocity it follows).
int op_gradient_advect(fluid_ctx* c, int u, int v, int p, int b, int d, int d0, const MemberVal& dt)
{
    if (p == u || p == v || u == v) return fail(FLUID_E_INVALID, "subtract_gradient: fields must be distinct");
    if (d == d0 || d == u || d == v || d == p || d0 == u || d0 == v)
        return fail(FLUID_E_INVALID, "advect: output must not alias an input");
    if (c->nranks != 1) return fail(FLUID_E_INVALID, "op_gradient_advect is a one-GPU operator");
    const float h = 1.0f / (float)c->n;
    TRY(materialize(c, {u, v, d0}));
    TRY(materialize(c, p, /*keep_scale=*/true));
    const float* mdt0 = nullptr;
    TRY(member_dt0(c, dt, &mdt0));
    TIMED(c, FLUID_TIME_PROJECTION,
          fluid::launch_gradient_advect(c->stream, c->st, c->ptr(u), c->ptr(v), c->ptr(p), c->ptr(d), c->ptr(d0), c->pitch, c->n, c->own0,
                                        c->own1, h, dt.at(0) * (float)c->n, b, 1.0f / c->field[p].fscale, c->mb(), mdt0));
    wrote(c, u, 0);
    wrote(c, v, 0);
    wrote(c, d, 0);
    return FLUID_OK;
}

void coefficients(int n, float dt, float coef, float* alpha, float* beta)
{
    // ((dt*coef)*n)*n in float, then 1 + 4*alpha (FluidSequential.c:179-180,199-200)
    volatile float a = dt * coef;
    a = a * (float)n;
    a = a * (float)n;
    volatile float four_a = 4.0f * a;
    *alpha = a;
    *beta = 1.0f + four_a;
}

// alpha, beta of a diffusion with a uniform or per-member dt and coefficient: coefficients() per member, the same function
Coeffs diffusion_coeffs(const fluid_ctx* c, const MemberVal& dt, const MemberVal& coef)
{
    auto part = [&](bool want_beta) {
        return dt.map(coef, [&](float d, float k) {
            float alpha, beta;
            coefficients(c->n, d, k, &alpha, &beta);
            return want_beta ? beta : alpha;
        });
    };
    return {part(false), part(true)};
}

// divergence -> pressure solve -> gradient subtraction (FluidSequential.c:213-223
// and :238-240).  On slabs: ONE exchange (u, v, iters+2 rows) covers the divergence,
// every sweep of the solve and the gradient's one-row halo of p.
// `then_advect` (one GPU): d, d0, b, dt of an advection along (u, v) to run in the same launch as the gradient subtraction
struct AdvectAfter {
    int b, d, d0;
    const MemberVal& dt;
};

// can the divergence be computed inside the first launch of the pressure solve that follows it?  The fused kernel, a first
// launch of a shape that has a DIVSRC kernel (kTbShapes), the exact-reciprocal division of (alpha 1, beta 4)
bool divergence_fuses(fluid_ctx* c, int iters, int reach)
{
    if (c->variant != fluid::JACOBI_TB || !c->fuse_divergence) return false;
    const SweepShape shape = sweep_shape(c, 1);
    if (shape.small) return false;
    const int room = c->nranks > 1 ? std::min(reach + 1, iters) : iters;        // sweeps the first launch may fuse (op_diffuse_batch)
    if (!fluid::jacobi_tb_exists(pick_sweeps(c, iters, room, shape, true), 4, c->tb_nv, fluid::TB_DIVSRC)) return false;
    return division_mode(c, 4.0f, 1.0f).mode == 4;
}

// `with_max` (slabs): see op_subtract_gradient
int project(fluid_ctx* c, int u, int v, int p, int div, int iters, const AdvectAfter* then_advect = nullptr, bool with_max = false)
{
    // rows past the slab on which the divergence is wanted (so that the solve needs no exchange of its own), as op_divergence
    const int reach = c->nranks > 1 ? std::max(0, std::min(std::min(iters, c->halo - 1), exchange_cap(c) - 1)) : 0;
    // fused: computeDivergenceAndPressure (FluidSequential.c:143-158) inside the solve's first launch: p = 0 is a mark, the
    // divergence is produced row by row as that launch's right-hand side and stored, ghost cells included
    const bool fused = divergence_fuses(c, iters, reach);
    const DivSource ds{u, v, (-0.5f * (1.0f / (float)c->n)) * c->pscale};
    if (fused) {
        if (p == u || p == v || div == u || div == v || p == div)
            return fail(FLUID_E_INVALID, "divergence: outputs must not alias inputs");
        TRY(materialize(c, {u, v}));
        if (c->nranks > 1) TRY(need(c, {u, v}, reach + 1, /*async=*/true));      // joined by the solve's first launch
        mark_zero(c, p);
        wrote(c, div, reach);                 // about to be overwritten: as far as the first launch can form it from (u, v)
        c->field[div].fscale = c->pscale;     // (what the first launch stores; the solve is linear: p comes out with the same factor)
    } else {
        TRY(op_divergence(c, u, v, p, div, std::min(iters, c->halo - 1), c->pscale));
    }
    c->in_pressure_solve = true;            // timing only: reported separately (fluid_timing::pressure_ms)
    const Coeffs pressure{1.0f, 4.0f};
    const int rc_solve = op_diffuse(c, 0, p, div, pressure, iters, /*final_reach=*/1, fused ? &ds : nullptr);
    c->in_pressure_solve = false;
    TRY(rc_solve);
    if (fused) {                            // (the first launch recorded the rows it stored)
        TRY(xchg_join(c));
        wrote(c, div, 0);
        c->field[div].fscale = c->pscale;
    }
    if (then_advect) return op_gradient_advect(c, u, v, p, then_advect->b, then_advect->d, then_advect->d0, then_advect->dt);
    return op_subtract_gradient(c, u, v, p, with_max);
}

// FluidSequential.c:189-241 with the SWAPs resolved into field roles:
// after :201/:209 the diffused velocity lives in the *_prev buffers.
int vel_step(fluid_ctx* c, const MemberVal& dt, const MemberVal& visc, int iters)
{
    const int U = FLUID_U, V = FLUID_V, U0 = FLUID_U_PREV, V0 = FLUID_V_PREV;
    TRY(op_add_source(c, U, U0, dt, /*defer=*/true));
    TRY(op_add_source(c, V, V0, dt, /*defer=*/true));
    const Coeffs cv = diffusion_coeffs(c, dt, visc);
    // one exchange feeds both solves: right-hand sides iters-1 rows out, first guesses iters rows
    const int h = std::min(iters, c->halo);
    TRY(need(c, {U, V, U0, V0}, h, /*async=*/true));
    const Solve uv[2] = {{1, U0, U, &cv}, {2, V0, V, &cv}};
    TRY(op_diffuse_batch(c, uv, 2, iters));
    TRY(xchg_join(c));
    TRY(project(c, U0, V0, /*p=*/U, /*div=*/V, iters, nullptr, /*with_max=*/true));
    const float dt0 = dt.at(0) * (float)c->n;      // (slabs only: one member)
    TRY(vmax_begin(c, U0, V0, /*have_max=*/true));
    TRY(advect_bounded(c, 0, {U0, V0}, dt0, [&] { return op_advect2(c, 1, U, U0, 2, V, V0, U0, V0, dt); }));
    return project(c, U, V, /*p=*/U0, /*div=*/V0, iters);
}

// FluidSequential.c:176-186
int dens_step(fluid_ctx* c, const MemberVal& dt, const MemberVal& diff, int iters)
{
    const int X = FLUID_DENS, X0 = FLUID_DENS_PREV;
    TRY(op_add_source(c, X, X0, dt, /*defer=*/true));
    const Coeffs cd = diffusion_coeffs(c, dt, diff);
    const Solve one{0, X0, X, &cd};
    TRY(op_diffuse_batch(c, &one, 1, iters));
    TRY(vmax_begin(c, FLUID_U, FLUID_V));
    return advect_bounded(c, 1, {X0}, dt.at(0) * (float)c->n, [&] { return op_advect(c, 0, X, X0, FLUID_U, FLUID_V, dt); });
}

// One loop body of the reference's main (FluidSequential.c:305-306).  The density's
// source term and diffusion are brought forward next to the velocity's: the three
// diffusions are independent of one another and of everything in between, so they
// run as ONE batch (one exchange on slabs, three times the waves per launch); the
// arithmetic per cell and the final contents of all six fields are unchanged.
int full_step(fluid_ctx* c, const MemberVal& dt, const MemberVal& diff, const MemberVal& visc, int iters)
{
    const int U = FLUID_U, V = FLUID_V, D = FLUID_DENS, U0 = FLUID_U_PREV, V0 = FLUID_V_PREV, D0 = FLUID_DENS_PREV;
    TRY(op_add_source(c, U, U0, dt, /*defer=*/true));
    TRY(op_add_source(c, V, V0, dt, /*defer=*/true));
    TRY(op_add_source(c, D, D0, dt, /*defer=*/true));
    // right-hand sides and first guesses together (zeroed sources are valid everywhere and skipped); async: the first launch
    // of the diffusion runs its interior strips while the rows travel (op_diffuse_batch)
    TRY(need(c, {U, V, D, U0, V0, D0}, std::min(iters, c->halo), /*async=*/true));
    const Coeffs cv = diffusion_coeffs(c, dt, visc), cd = diffusion_coeffs(c, dt, diff);
    const float dt0 = dt.at(0) * (float)c->n;      // (slabs only: one member)
    const Solve all[3] = {{1, U0, U, &cv}, {2, V0, V, &cv}, {0, D0, D, &cd}};
    if (c->nranks == 1) {
        TRY(op_diffuse_batch(c, all, 3, iters));
        TRY(project(c, U0, V0, /*p=*/U, /*div=*/V, iters));
        TRY(op_advect2(c, 1, U, U0, 2, V, V0, U0, V0, dt));
        const AdvectAfter dens{0, D, D0, dt};
        return project(c, U, V, /*p=*/U0, /*div=*/V0, iters, &dens);
    }
    // Slabs: each advect needs the global max |velocity| on the host -- a pipeline drain.  The
    // density diffusion depends on nothing in between, so most of it rides in the same launches as
    // u and v (the fused kernel is latency-bound: a third field per launch is nearly free) and its
    // last sweeps are held back, one launch behind each reduction, so the GPU stays busy while the
    // host waits and talks to its peers.
    // The split falls on launch boundaries of the solve's own schedule (the last two launches are the ones
    // held back): with fp16 storage every launch rounds once, so cutting a launch in two would change the
    // result (iters = 20 runs as 8 + 8 + 4 on one GPU and must do so here).
    int fill1 = 0, fill2 = 0;
    {
        const SweepShape shape = sweep_shape(c, 1);
        std::vector<int> launches;
        for (int left = iters; left > 0;) {
            launches.push_back(pick_sweeps(c, left, left, shape, /*all_mode4=*/false));
            left -= launches.back();
        }
        // about eight sweeps behind each reduction (whole launches; single-sweep kernels: eight launches)
        for (int* fill : {&fill2, &fill1})
            while (*fill < 8 && !launches.empty()) {
                *fill += launches.back();
                launches.pop_back();
            }
        if (fill1 == 0) std::swap(fill1, fill2);
    }
    if (c->stream2 && c->slab_overlap && std::min(iters, c->halo) >= iters) {
        // A slab is a small problem: its launches leave most of the chip idle (one rank's share of 8192^2 / 8 keeps a
        // quarter of the wave slots busy), and the density diffusion depends on nothing in the velocity path.  So it
        // runs beside that path on a second stream -- from the moment its rows have arrived until the density advect at
        // the end -- and also fills the two stretches in which the host waits for the advect bounds.  Only when the ghost
        // zones cover the whole solve: an exchange inside it would put collectives on two streams in an order the ranks
        // could not agree on.  It ping-pongs with TMP2, the velocity path with TMP0 / TMP1.
        HIP_TRY(hipEventRecord(c->ev_fork, c->stream));
        HIP_TRY(hipStreamWaitEvent(c->stream2, c->ev_fork, 0));
        c->xowed = (c->xowed & 1u) ? 3u : 0u;       // stream2 now runs behind every wait of the main stream: it owes what that owes
        hipStream_t main_stream = c->stream;
        c->stream = c->stream2;
        const int rc_dens = op_diffuse_batch(c, all + 2, 1, iters, 0, nullptr, /*scratch_base=*/2);
        hipError_t e_join = rc_dens == FLUID_OK ? hipEventRecord(c->ev_join, c->stream2) : hipSuccess;
        c->stream = main_stream;
        TRY(rc_dens);
        HIP_TRY(e_join);
        TRY(op_diffuse_batch(c, all, 2, iters));
        TRY(project(c, U0, V0, /*p=*/U, /*div=*/V, iters, nullptr, /*with_max=*/true));
        TRY(vmax_begin(c, U0, V0, /*have_max=*/true));
        TRY(advect_bounded(c, 0, {U0, V0}, dt0, [&] { return op_advect2(c, 1, U, U0, 2, V, V0, U0, V0, dt); }));
        TRY(project(c, U, V, /*p=*/U0, /*div=*/V0, iters, nullptr, /*with_max=*/true));
        TRY(vmax_begin(c, U, V, /*have_max=*/true));
        HIP_TRY(hipStreamWaitEvent(c->stream, c->ev_join, 0));
        return advect_bounded(c, 1, {D0}, dt0, [&] { return op_advect(c, 0, D, D0, U, V, dt); });
    }
    const int rest = fill1 + fill2, head = iters - rest;
    if (head > 0) TRY(op_diffuse_batch(c, all, 3, head));
    if (rest > 0) TRY(op_diffuse_batch(c, all, 2, rest));
    TRY(xchg_join(c));
    TRY(project(c, U0, V0, /*p=*/U, /*div=*/V, iters, nullptr, /*with_max=*/true));
    TRY(vmax_begin(c, U0, V0, /*have_max=*/true));
    if (fill1 > 0) TRY(op_diffuse_batch(c, all + 2, 1, fill1));
    TRY(advect_bounded(c, 0, {U0, V0}, dt0, [&] { return op_advect2(c, 1, U, U0, 2, V, V0, U0, V0, dt); }));
    TRY(project(c, U, V, /*p=*/U0, /*div=*/V0, iters, nullptr, /*with_max=*/true));
    TRY(vmax_begin(c, U, V, /*have_max=*/true));
    if (fill2 > 0) TRY(op_diffuse_batch(c, all + 2, 1, fill2));
    return advect_bounded(c, 1, {D0}, dt0, [&] { return op_advect(c, 0, D, D0, U, V, dt); });
}

int zero_sources(fluid_ctx* c)
{
    // the reference's zeroing loop (FluidSequential.c:298-302): marked, see "fields that are zero by definition"
    for (int id : {FLUID_U_PREV, FLUID_V_PREV, FLUID_DENS_PREV}) mark_zero(c, id);
    return FLUID_OK;
}

// `wait` = false only enqueues (fp32 storage): step() / step_src() queue all their fields and wait once
// `member`: whose copy of the field.  An upload settles the field for ALL members first (materialize: the marks are shared,
// and the members that are not uploaded must end up holding what the marks stood for), then overwrites that member's rows.
int copy_rows(fluid_ctx* c, int field, float* host, const float* chost, int row_lo, int row_hi, bool to_device, bool wait = true,
              int member = 0)
{
    if (row_lo < 0 || row_hi > c->w || row_lo > row_hi) return fail(FLUID_E_INVALID, "bad row range");
    if (row_lo == row_hi) return FLUID_OK;
    // a download of a field kept scaled (fp16 storage: pressure, divergence) divides on the host, in float: exact, where a
    // pass over the fp16 field would round the plain values into fp16's subnormals again
    const float host_scale = (!to_device && c->st != fluid::STORAGE_F32) ? 1.0f / c->field[field].fscale : 1.0f;
    TRY(materialize(c, field, /*keep_scale=*/host_scale != 1.0f));
    char* dev = static_cast<char*>(c->row(field, row_lo)) + (size_t)member * c->field_bytes + (size_t)XOFF * c->esz;
    const size_t rows = (size_t)(row_hi - row_lo), w = (size_t)c->w;
    const size_t dp = (size_t)c->pitch * c->esz;
    if (to_device) c->field[field].reach = 0;     // the caller vouches only for its own rows
    if (c->st == fluid::STORAGE_F32) {
        const size_t hp = w * sizeof(float);
        if (to_device)
            HIP_TRY(hipMemcpy2DAsync(dev, dp, chost + (size_t)row_lo * w, hp, hp, rows, hipMemcpyHostToDevice, c->stream));
        else
            HIP_TRY(hipMemcpy2DAsync(host + (size_t)row_lo * w, hp, dev, dp, hp, rows, hipMemcpyDeviceToHost, c->stream));
        if (wait) HIP_TRY(hipStreamSynchronize(c->stream));
        return FLUID_OK;
    }
    // fp16 storage: the ABI's host arrays stay float; convert through a host staging buffer
    // (round to nearest even on the way in, exact on the way out)
    std::vector<fluid::half_t> stage(rows * w);
    const size_t hp = w * sizeof(fluid::half_t);
    if (to_device) {
        const float* src = chost + (size_t)row_lo * w;
        for (size_t k = 0; k < rows * w; ++k) stage[k] = (fluid::half_t)src[k];
        HIP_TRY(hipMemcpy2DAsync(dev, dp, stage.data(), hp, hp, rows, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    } else {
        HIP_TRY(hipMemcpy2DAsync(stage.data(), hp, dev, dp, hp, rows, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
        float* dst = host + (size_t)row_lo * w;
        for (size_t k = 0; k < rows * w; ++k) dst[k] = (float)stage[k] * host_scale;
    }
    return FLUID_OK;
}

// the context step() / step_src() keep between calls, one per calling thread; destroyed when the thread ends
// (for the main thread that is before the HIP runtime's own static destructors run)
struct CachedCtx {
    fluid_ctx* c = nullptr;
    ~CachedCtx();
};
thread_local CachedCtx g_cached_holder;
#define g_cached (g_cached_holder.c)

}  // namespace

// ===========================================================================
// extern "C" shim
// ===========================================================================
extern "C" {

const char* fluid_last_error(void) { return g_err.c_str(); }

int fluid_coefficients(int N, float dt, float coef, float* alpha, float* beta)
{
    if (N < 1 || !alpha || !beta) return fail(FLUID_E_INVALID, "fluid_coefficients: bad argument");
    coefficients(N, dt, coef, alpha, beta);
    return FLUID_OK;
}

int fluid_layout(int N, int* pitch, int* xoff, size_t* field_floats)
{
    if (N < 1 || N > kMaxN) return fail(FLUID_E_INVALID, "N must be in [1, %d] (got %d)", kMaxN, N);
    const int p = fluid::pitch_for(N);
    if (pitch) *pitch = p;
    if (xoff) *xoff = XOFF;
    if (field_floats) *field_floats = (size_t)(N + 2) * p;
    return FLUID_OK;
}

size_t fluid_arena_bytes_ensemble(int N, int storage, int members)
{
    size_t ff = 0;
    if (fluid_layout(N, nullptr, nullptr, &ff) != FLUID_OK) return 0;
    if (storage != FLUID_STORAGE_F32 && storage != FLUID_STORAGE_F16) return 0;
    if (members < 1 || members > kMaxMembers) return 0;
    return ff * FLUID_NFIELDS * fluid::storage_bytes(storage) * (size_t)members + kControlBytes;
}

size_t fluid_arena_bytes_ex(int N, int storage) { return fluid_arena_bytes_ensemble(N, storage, 1); }

size_t fluid_arena_bytes(int N) { return fluid_arena_bytes_ex(N, FLUID_STORAGE_F32); }

int fluid_create_ex(const fluid_config* cfg, fluid_ctx** out) { return fluid_create_ensemble(cfg, 1, out); }

// Every argument is checked before the device is touched.  Fields are laid out [field][member]: member m of field f starts
// (f * members + m) * field_bytes into the arena, the control block behind the last one.
int fluid_create_ensemble(const fluid_config* cfg, int members, fluid_ctx** out)
{
    if (!cfg || !out) return fail(FLUID_E_INVALID, "fluid_create_ex / fluid_create_ensemble: null argument");
    *out = nullptr;
    if (members < 1 || members > kMaxMembers) return fail(FLUID_E_INVALID, "members must be in [1, %d] (got %d)", kMaxMembers, members);
    if (members > 1 && cfg->nranks > 1) return fail(FLUID_E_INVALID, "an ensemble runs on one GPU: nranks must be 1 (got %d)", cfg->nranks);
    const int n = cfg->n;
    if (n < 1 || n > kMaxN) return fail(FLUID_E_INVALID, "N must be in [1, %d] (got %d)", kMaxN, n);
    const int P = cfg->nranks < 1 ? 1 : cfg->nranks;
    if (cfg->rank < 0 || cfg->rank >= P) return fail(FLUID_E_INVALID, "rank %d outside [0,%d)", cfg->rank, P);
    if (cfg->jacobi_variant < 0 || cfg->jacobi_variant >= fluid::JACOBI_VARIANTS)
        return fail(FLUID_E_INVALID, "unknown Jacobi variant %d", cfg->jacobi_variant);
    if (cfg->storage != FLUID_STORAGE_F32 && cfg->storage != FLUID_STORAGE_F16)
        return fail(FLUID_E_INVALID, "unknown storage type %d", cfg->storage);
    if (P > 1 && n / P < 2) return fail(FLUID_E_INVALID, "N=%d is too small for %d row slabs (need >= 2 rows each)", n, P);
    fluid_ctx* c = new (std::nothrow) fluid_ctx;
    if (!c) return fail(FLUID_E_NOMEM, "out of host memory");
    c->n = n;
    c->w = n + 2;
    c->pitch = fluid::pitch_for(n);
    c->field_floats = (size_t)c->w * c->pitch;
    c->members = members;
    c->st = cfg->storage;
    c->esz = fluid::storage_bytes(c->st);
    c->field_bytes = c->field_floats * c->esz;
    c->variant = cfg->jacobi_variant;
    if (c->st == fluid::STORAGE_F16 && n >= 16) {
        // 2^(floor(log2 N) - 2): h * pscale lies in (1/8, 1/4], so a scaled divergence is at most a quarter of the velocity
        // differences it is formed from -- no fp16 overflow that the plain field would not have had 2^12 earlier -- and the
        // pressure of ordinary velocities sits in fp16's normal range instead of its subnormals
        int e = 0;
        (void)std::frexp((float)n, &e);                 // n = m * 2^e, m in [0.5, 1): floor(log2 n) = e - 1
        c->pscale = std::ldexp(1.0f, e - 3);
    }
    c->rank = cfg->rank;
    c->nranks = P;
    const int base = n / P, rem = n % P;
    c->own0 = 1 + cfg->rank * base + std::min(cfg->rank, rem);
    c->own1 = c->own0 + base + (cfg->rank < rem ? 1 : 0);
    c->min_slab = base;
    // ghost-zone depth: never reaches a neighbour's wall rows (depth <= slab-1)
    // default: deep enough that a 40-sweep solve (+ the gradient's row) needs one exchange -- halo
    // rows are latency-bound on xGMI (32 KiB per row at 8192^2) -- at ~4 % redundant rows on a
    // 1024-row slab; shallower on short slabs
    const int want = cfg->halo > 0 ? cfg->halo : std::max(4, std::min(42, base / 8));
    c->halo = P > 1 ? std::max(1, std::min(want, base - 1)) : 1;
    if (P > 1 && cfg->storage == FLUID_STORAGE_F16) {
        // fp16 results depend on the launch schedule (one rounding per launch); keeping it identical to the
        // one-GPU schedule needs ghost zones at least as deep as the longest fused launch
        if (base - 1 < 8) {
            delete c;
            return fail(FLUID_E_INVALID, "fp16 storage needs row slabs of at least 9 rows (N=%d over %d slabs gives %d)", n, P, base);
        }
        c->halo = std::max(c->halo, 8);
    }
    const size_t bytes = c->all_bytes() * FLUID_NFIELDS + kControlBytes;
    int rc = FLUID_OK;
    auto bail = [&](int code) { fluid_destroy(c); return code; };
    if (cfg->arena) {
        if (cfg->arena_bytes < bytes) return bail(fail(FLUID_E_INVALID, "arena too small: %zu < %zu", cfg->arena_bytes, bytes));
        if (((uintptr_t)cfg->arena & 255u) != 0) return bail(fail(FLUID_E_INVALID, "arena must be 256-byte aligned"));
        c->arena = (char*)cfg->arena;
    } else {
        hipError_t e = hipMalloc((void**)&c->arena, bytes);
        if (e != hipSuccess) return bail(fail(e == hipErrorOutOfMemory ? FLUID_E_NOMEM : FLUID_E_HIP, "hipMalloc(%zu): %s", bytes, hipGetErrorString(e)));
        c->own_arena = true;
    }
    if (cfg->stream) {
        c->stream = (hipStream_t)cfg->stream;
    } else {
        hipError_t e = hipStreamCreateWithFlags(&c->stream, hipStreamNonBlocking);
        if (e != hipSuccess) return bail(fail(FLUID_E_HIP, "hipStreamCreate: %s", hipGetErrorString(e)));
        c->own_stream = true;
    }
    for (int k = 0; k < FLUID_NFIELDS; ++k) c->field[k].ptr = c->arena + (size_t)k * c->all_bytes();
    auto hip_ok = [&](hipError_t e, const char* what) {
        if (e == hipSuccess) return true;
        rc = fail(e == hipErrorOutOfMemory ? FLUID_E_NOMEM : FLUID_E_HIP, "%s: %s", what, hipGetErrorString(e));
        return false;
    };
    {
        int dev = 0, cus = 0;
        if (hipGetDevice(&dev) == hipSuccess &&
            hipDeviceGetAttribute(&cus, hipDeviceAttributeMultiprocessorCount, dev) == hipSuccess && cus > 0)
            c->num_cu = cus;
    }
    if (P > 1) {
        if (!hip_ok(hipStreamCreateWithFlags(&c->stream2, hipStreamNonBlocking), "hipStreamCreate(second stream)")) return bail(rc);
        if (!hip_ok(hipEventCreateWithFlags(&c->ev_fork, hipEventDisableTiming), "hipEventCreate")) return bail(rc);
        if (!hip_ok(hipEventCreateWithFlags(&c->ev_join, hipEventDisableTiming), "hipEventCreate")) return bail(rc);
        if (!hip_ok(hipStreamCreateWithFlags(&c->xstream, hipStreamNonBlocking), "hipStreamCreate(exchange stream)")) return bail(rc);
        if (!hip_ok(hipEventCreateWithFlags(&c->ev_xbegin, hipEventDisableTiming), "hipEventCreate")) return bail(rc);
        if (!hip_ok(hipEventCreateWithFlags(&c->ev_xdone, hipEventDisableTiming), "hipEventCreate")) return bail(rc);
    }
    if (!hip_ok(hipMemsetAsync(c->arena, 0, bytes, c->stream), "hipMemsetAsync(arena)")) return bail(rc);
    c->d_scalar = reinterpret_cast<unsigned int*>(c->arena + c->all_bytes() * FLUID_NFIELDS);   // RCCL-addressable
    {
        const size_t words = 3 * (size_t)members * tile_words(c);
        if (!hip_ok(hipMalloc((void**)&c->tiles, words * sizeof(unsigned)), "hipMalloc(tiles)")) return bail(rc);
        if (!hip_ok(hipMemsetAsync(c->tiles, 0, words * sizeof(unsigned), c->stream), "hipMemsetAsync(tiles)")) return bail(rc);
    }
    if (P > 1 && !hip_ok(hipMalloc((void**)&c->d_partials, fluid::kMaxPartials * sizeof(float)), "hipMalloc(partials)")) return bail(rc);
    if (!hip_ok(hipHostMalloc((void**)&c->h_scalar, 256, hipHostMallocDefault), "hipHostMalloc")) return bail(rc);
    if (!hip_ok(hipEventCreateWithFlags(&c->scalar_ready, hipEventDisableTiming), "hipEventCreate")) return bail(rc);
    if (!hip_ok(hipStreamSynchronize(c->stream), "hipStreamSynchronize")) return bail(rc);
    *out = c;
    return FLUID_OK;
}

int fluid_create(int N, fluid_ctx** out)
{
    fluid_config cfg;
    std::memset(&cfg, 0, sizeof cfg);
    cfg.n = N;
    cfg.nranks = 1;
    cfg.jacobi_variant = FLUID_JACOBI_TB;
    return fluid_create_ex(&cfg, out);
}

int fluid_destroy(fluid_ctx* c)
{
    if (!c) return FLUID_OK;
    if (c->stream) (void)hipStreamSynchronize(c->stream);
    if (c->stream2) (void)hipStreamSynchronize(c->stream2);
    if (c->xstream) (void)hipStreamSynchronize(c->xstream);
    for (auto& p : c->ev_pool) {
        (void)hipEventDestroy(p.a);
        (void)hipEventDestroy(p.b);
    }
    if (!c->trials.empty()) {                    // measurements that die with the context are handed back to the tuner
        RbTuner& t = rb_tuner();
        std::lock_guard<std::mutex> lock(t.mu);
        for (auto& tr : c->trials) {
            auto it = t.table.find(tr.key);
            if (it != t.table.end() && !it->second.fixed && it->second.issued[tr.cand] > 0) it->second.issued[tr.cand] -= 1;
            (void)hipEventDestroy(tr.a);
            (void)hipEventDestroy(tr.b);
        }
    }
    for (hipEvent_t ev : c->free_events) (void)hipEventDestroy(ev);
    fluid_detail::rccl_release(c->rccl);
    c->rccl = nullptr;
    if (c->h_scalar) (void)hipHostFree(c->h_scalar);
    if (c->tiles) (void)hipFree(c->tiles);
    for (auto& b : c->consts.live) (void)hipEventDestroy(b.copied);
    for (hipEvent_t ev : c->consts.free_events) (void)hipEventDestroy(ev);
    if (c->observe.table) (void)hipFree(c->observe.table);
    for (hipEvent_t ev : c->xform.copied)
        if (ev) (void)hipEventDestroy(ev);
    if (c->lattice.copied) (void)hipEventDestroy(c->lattice.copied);
    if (c->d_partials) (void)hipFree(c->d_partials);
    if (c->scalar_ready) (void)hipEventDestroy(c->scalar_ready);
    if (c->own_arena && c->arena) (void)hipFree(c->arena);
    if (c->stream2) (void)hipStreamDestroy(c->stream2);
    if (c->xstream) (void)hipStreamDestroy(c->xstream);
    if (c->ev_xbegin) (void)hipEventDestroy(c->ev_xbegin);
    if (c->ev_xdone) (void)hipEventDestroy(c->ev_xdone);
    if (c->ev_fork) (void)hipEventDestroy(c->ev_fork);
    if (c->ev_join) (void)hipEventDestroy(c->ev_join);
    if (c->own_stream && c->stream) (void)hipStreamDestroy(c->stream);
    if (g_cached == c) g_cached = nullptr;
    delete c;                                    // (frees every Scratch: nothing runs any more, see the waits above)
    return FLUID_OK;
}

int fluid_synchronize(fluid_ctx* c)
{
    TRY(check_ctx(c));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FLUID_OK;
}

int fluid_exchange_stream(fluid_ctx* c, void** stream)
{
    TRY(check_ctx(c));
    if (!stream) return fail(FLUID_E_INVALID, "null pointer");
    *stream = c->stream;                    // inside an exchange callback: the exchange stream (call_exchange)
    return FLUID_OK;
}

int fluid_split_launches(fluid_ctx* c, long long* count)
{
    TRY(check_ctx(c));
    if (!count) return fail(FLUID_E_INVALID, "null pointer");
    *count = c->split_launches;
    return FLUID_OK;
}

int fluid_owned_rows(fluid_ctx* c, int* row_lo, int* row_hi)
{
    TRY(check_ctx(c));
    if (row_lo) *row_lo = c->own0;
    if (row_hi) *row_hi = c->own1;
    return FLUID_OK;
}

int fluid_field_ptr(fluid_ctx* c, int field, void** dev_ptr)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {field}));
    if (!dev_ptr) return fail(FLUID_E_INVALID, "null pointer");
    if (c->in_halo_exchange) TRY(materialize_zero(c, field));
    else TRY(materialize(c, field));       // whoever asks for the address may read the memory
    *dev_ptr = c->ptr(field);
    return FLUID_OK;
}

int fluid_scalar_ptr(fluid_ctx* c, void** dev_ptr)
{
    TRY(check_ctx(c));
    if (!dev_ptr) return fail(FLUID_E_INVALID, "null pointer");
    *dev_ptr = c->d_scalar;
    return FLUID_OK;
}

int fluid_members(fluid_ctx* c, int* members)
{
    TRY(check_ctx(c));
    if (!members) return fail(FLUID_E_INVALID, "null pointer");
    *members = c->members;
    return FLUID_OK;
}

// the whole-field copies of a one-member context would have to pick a member or broadcast: either would be a trap
static int refuse_plain_copy(const fluid_ctx* c, const char* what)
{
    if (c->members > 1)
        return fail(FLUID_E_INVALID, "%s: this context has %d members -- use fluid_upload_member / fluid_download_member", what, c->members);
    return FLUID_OK;
}

static int check_member(const fluid_ctx* c, int member)
{
    if (member < 0 || member >= c->members) return fail(FLUID_E_INVALID, "member %d outside [0, %d)", member, c->members);
    return FLUID_OK;
}

int fluid_upload_member(fluid_ctx* c, int member, int field, const float* host)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {field}));
    TRY(check_member(c, member));
    if (!host) return fail(FLUID_E_INVALID, "null host pointer");
    return copy_rows(c, field, nullptr, host, 0, c->w, true, true, member);
}

int fluid_download_member(fluid_ctx* c, int member, int field, float* host)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {field}));
    TRY(check_member(c, member));
    if (!host) return fail(FLUID_E_INVALID, "null host pointer");
    return copy_rows(c, field, host, nullptr, 0, c->w, false, true, member);
}

int fluid_upload_rows(fluid_ctx* c, int field, const float* host, int row_lo, int row_hi)
{
    TRY(check_ctx(c));
    TRY(refuse_plain_copy(c, "fluid_upload_rows"));
    TRY(check_fields(c, {field}));
    if (!host) return fail(FLUID_E_INVALID, "null host pointer");
    return copy_rows(c, field, nullptr, host, row_lo, row_hi, true);
}

int fluid_download_rows(fluid_ctx* c, int field, float* host, int row_lo, int row_hi)
{
    TRY(check_ctx(c));
    TRY(refuse_plain_copy(c, "fluid_download_rows"));
    TRY(check_fields(c, {field}));
    if (!host) return fail(FLUID_E_INVALID, "null host pointer");
    return copy_rows(c, field, host, nullptr, row_lo, row_hi, false);
}

int fluid_upload(fluid_ctx* c, int field, const float* host)
{
    TRY(check_ctx(c));
    TRY(refuse_plain_copy(c, "fluid_upload"));
    return fluid_upload_rows(c, field, host, 0, c->w);
}

int fluid_download(fluid_ctx* c, int field, float* host)
{
    TRY(check_ctx(c));
    TRY(refuse_plain_copy(c, "fluid_download"));
    return fluid_download_rows(c, field, host, 0, c->w);
}

int fluid_fill(fluid_ctx* c, int field, float value)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {field}));
    if (value == 0.0f && !std::signbit(value)) {
        HIP_TRY(hipMemsetAsync(c->ptr(field), 0, c->all_bytes(), c->stream));
        wrote(c, field, kEverywhere);
        return FLUID_OK;
    }
    std::vector<float> row((size_t)c->w * c->w, value);
    for (int m = 0; m < c->members; ++m) TRY(fluid_upload_member(c, m, field, row.data()));     // every member
    wrote(c, field, kEverywhere);
    return FLUID_OK;
}

int fluid_set_jacobi_variant(fluid_ctx* c, int variant)
{
    TRY(check_ctx(c));
    if (variant < 0 || variant >= fluid::JACOBI_VARIANTS) return fail(FLUID_E_INVALID, "unknown Jacobi variant %d", variant);
    c->variant = variant;
    return FLUID_OK;
}

int fluid_set_param(fluid_ctx* c, int key, int value)
{
    TRY(check_ctx(c));
    switch (key) {
    case FLUID_PARAM_TB_MAX_SWEEPS:
        if (!fluid::is_tb_depth(value)) return fail(FLUID_E_INVALID, "TB_MAX_SWEEPS must be 16, 12, 8, 4 or 2");
        c->tb_max_t = value;
        return FLUID_OK;
    case FLUID_PARAM_TB_ROWS:
        if (value < 0) return fail(FLUID_E_INVALID, "TB_ROWS must be >= 0");
        c->tb_rows = value;
        return FLUID_OK;
    case FLUID_PARAM_TB_EDGE_ROWS_PCT:
        if (value < 0 || value > 100) return fail(FLUID_E_INVALID, "TB_EDGE_ROWS_PCT must be in [0,100]");
        c->tb_edge_pct = value;
        return FLUID_OK;
    case FLUID_PARAM_TB_MIN_CELLS:
        if (value < 0) return fail(FLUID_E_INVALID, "TB_MIN_CELLS must be >= 0");
        c->tb_min_cells = value;
        return FLUID_OK;
    case FLUID_PARAM_TB_FAST_DIVISION:
        if (value < 0 || value > 3) return fail(FLUID_E_INVALID, "TB_FAST_DIVISION must be 0, 1, 2 or 3");
        c->fast_div = value;
        return FLUID_OK;
    case FLUID_PARAM_TB_AUTOTUNE:
        c->autotune = value != 0;
        return FLUID_OK;
    case FLUID_PARAM_TB_FILL:
        c->tb_fill = value != 0;
        return FLUID_OK;
    case FLUID_PARAM_SLAB_OVERLAP:
        c->slab_overlap = value != 0;
        return FLUID_OK;
    case FLUID_PARAM_FUSE_DIVERGENCE:
        c->fuse_divergence = value != 0;
        return FLUID_OK;
    case FLUID_PARAM_EARLY_ADVECT:
        c->early_advect = value != 0;
        return FLUID_OK;
    case FLUID_PARAM_FUSE_ADD_SOURCE:
        c->fuse_add_source = value != 0;
        return FLUID_OK;
    case FLUID_PARAM_F16_PRESSURE_SCALE: {
        for (int f = 0; f < FLUID_NFIELDS; ++f) TRY(unscale(c, f));
        int e = 0;
        (void)std::frexp((float)c->n, &e);
        c->pscale = (value != 0 && c->st == fluid::STORAGE_F16 && c->n >= 16) ? std::ldexp(1.0f, e - 3) : 1.0f;
        return FLUID_OK;
    }
    case FLUID_PARAM_XCHG_OVERLAP:
        TRY(xchg_join(c));
        c->xchg_overlap = value != 0;
        return FLUID_OK;
    case FLUID_PARAM_TB_T16_MIN_CELLS:
        if (value < -1) return fail(FLUID_E_INVALID, "TB_T16_MIN_CELLS must be >= 0, or -1 for the default rule");
        c->tb_t16_min_cells = value;
        return FLUID_OK;
    case FLUID_PARAM_TB_LANE_COLUMNS:
        if (value != 2 && value != 4) return fail(FLUID_E_INVALID, "TB_LANE_COLUMNS must be 2 or 4");
        c->tb_nv = value;
        return FLUID_OK;
    case FLUID_PARAM_HALO:
        if (value < 1) return fail(FLUID_E_INVALID, "HALO must be >= 1");
        c->halo = c->nranks > 1 ? std::max(c->st == fluid::STORAGE_F16 ? 8 : 1, std::min(value, c->min_slab - 1)) : 1;
        return FLUID_OK;
    default:
        return fail(FLUID_E_INVALID, "unknown parameter %d", key);
    }
}

int fluid_plan_sweeps(int N, int rows, int storage, int pressure_form, int iters, int max_sweeps, int t16_min_cells, int* depths,
                      int capacity, int* count)
{
    if (N < 1 || N > kMaxN || rows < 1 || rows > N || iters < 0 || (iters & 1) || !depths || !count || capacity < 0)
        return fail(FLUID_E_INVALID, "fluid_plan_sweeps: bad argument");
    if (storage != FLUID_STORAGE_F32 && storage != FLUID_STORAGE_F16) return fail(FLUID_E_INVALID, "unknown storage type %d", storage);
    if (!fluid::is_tb_depth(max_sweeps)) return fail(FLUID_E_INVALID, "max_sweeps must be 16, 12, 8, 4 or 2");
    fluid_ctx c;                            // host-side description only: no device, no stream
    c.n = N;
    c.st = storage;
    c.esz = fluid::storage_bytes(storage);
    c.field_bytes = (size_t)(N + 2) * fluid::pitch_for(N) * c.esz;
    c.tb_max_t = max_sweeps;
    c.tb_t16_min_cells = t16_min_cells;
    const SweepShape shape{storage == FLUID_STORAGE_F16, false, (long long)rows * N};
    int k = 0;
    for (int left = iters; left > 0;) {
        const int t = pick_sweeps(&c, left, left, shape, pressure_form != 0);
        if (k < capacity) depths[k] = t;
        ++k;
        left -= t;
    }
    *count = k;
    return FLUID_OK;
}

int fluid_autotune_pending(fluid_ctx* c, int* shapes_open)
{
    TRY(check_ctx(c));
    if (!shapes_open) return fail(FLUID_E_INVALID, "null pointer");
    tune_harvest(c);
    RbTuner& t = rb_tuner();
    std::lock_guard<std::mutex> lock(t.mu);
    int open = 0;
    for (auto& kv : t.table) open += kv.second.fixed ? 0 : 1;
    *shapes_open = open;
    return FLUID_OK;
}

int fluid_division_mode(fluid_ctx* c, float alpha, float beta, int* mode)
{
    TRY(check_ctx(c));
    if (!mode) return fail(FLUID_E_INVALID, "null pointer");
    *mode = c->variant == fluid::JACOBI_TB ? division_mode(c, beta, alpha).mode : 0;
    return FLUID_OK;
}

int fluid_set_exchange(fluid_ctx* c, fluid_exchange_fn fn, void* user)
{
    TRY(check_ctx(c));
    TRY(fluid_detail::refuse_ensemble(c, "fluid_set_exchange"));
    c->xchg = fn;
    c->xchg_user = user;
    return FLUID_OK;
}

int fluid_exchange_now(fluid_ctx* c, int kind, const int* fields, int nfields, int depth)
{
    TRY(check_ctx(c));
    TRY(fluid_detail::refuse_ensemble(c, "fluid_exchange_now"));
    if (!c->xchg) return fail(FLUID_E_COMM, "no exchange installed");
    if (kind != FLUID_XCHG_HALO && kind != FLUID_XCHG_GATHER) return fail(FLUID_E_INVALID, "fluid_exchange_now moves rows: HALO or GATHER");
    if (nfields < 0 || (nfields > 0 && !fields)) return fail(FLUID_E_INVALID, "bad field list");
    // the depth is checked against the SHORTEST slab, which every rank knows: a check against this rank's own height
    // would let the tall ranks of an uneven split into the collective while the short ones return
    if (kind == FLUID_XCHG_HALO && c->nranks > 1 && (depth < 1 || depth > c->min_slab))
        return fail(FLUID_E_INVALID, "halo depth %d outside [1, %d] (the shortest slab)", depth, c->min_slab);
    for (int k = 0; k < nfields; ++k) {
        TRY(check_fields(c, {fields[k]}));
        TRY(settle(c, fields[k], /*keep_scale=*/true));   // the caller is about to look at the rows: no increment may stay pending
                                                          // (a scale stays: it is the same on every rank, and a download undoes it)
    }
    c->in_halo_exchange = true;
    const int rc = call_exchange(c, kind, fields, nfields, depth, nullptr);
    c->in_halo_exchange = false;
    if (rc != 0) return fail(FLUID_E_COMM, "exchange failed (kind %d, rc %d)", kind, rc);
    for (int k = 0; k < nfields; ++k)
        c->field[fields[k]].reach = kind == FLUID_XCHG_GATHER ? kEverywhere : std::max(c->field[fields[k]].reach, depth);
    return FLUID_OK;
}

// ---- calls whose physical parameters are one value for everybody or one per member (ensembles) ---------------------
// One body per call, on MemberVal: it checks the context and the call's other arguments and does the work.  The scalar
// entry point is that body.  The _members one first finds null arrays, a null context and non-finite entries, before
// anything else happens (nothing is launched and neither a field nor what the library still owes one changes), hands
// element 0 to the scalar entry point on a context with one member (row slabs included), and has the table ring in place
// before the body runs.
struct MemberArg {
    const char* name;
    const float* v;
};

static int check_member_args(const fluid_ctx* c, const char* call, std::initializer_list<MemberArg> args)
{
    for (const MemberArg& a : args)
        if (!a.v) return fail(FLUID_E_INVALID, "%s: null array `%s`", call, a.name);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    for (const MemberArg& a : args)
        for (int m = 0; m < c->members; ++m)
            if (!std::isfinite(a.v[m])) return fail(FLUID_E_INVALID, "%s: member %d: %s is not finite (%g)", call, m, a.name, (double)a.v[m]);
    return FLUID_OK;
}

static int vel_step_body(fluid_ctx* c, const MemberVal& dt, const MemberVal& visc, int iters)
{
    TRY(check_ctx(c));
    TRY(check_iters(iters));
    TRY(vel_step(c, dt, visc, iters));
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_vel_step(fluid_ctx* c, float dt, float visc, int iters) { return vel_step_body(c, dt, visc, iters); }

int fluid_vel_step_members(fluid_ctx* c, const float* dt, const float* visc, int iters)
{
    TRY(check_member_args(c, "fluid_vel_step_members", {{"dt", dt}, {"visc", visc}}));
    if (c->members == 1) return fluid_vel_step(c, dt[0], visc[0], iters);
    TRY(ensure_consts(c));
    return vel_step_body(c, {dt, c->members}, {visc, c->members}, iters);
}

static int dens_step_body(fluid_ctx* c, const MemberVal& dt, const MemberVal& diff, int iters)
{
    TRY(check_ctx(c));
    TRY(check_iters(iters));
    TRY(dens_step(c, dt, diff, iters));
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_dens_step(fluid_ctx* c, float dt, float diff, int iters) { return dens_step_body(c, dt, diff, iters); }

int fluid_dens_step_members(fluid_ctx* c, const float* dt, const float* diff, int iters)
{
    TRY(check_member_args(c, "fluid_dens_step_members", {{"dt", dt}, {"diff", diff}}));
    if (c->members == 1) return fluid_dens_step(c, dt[0], diff[0], iters);
    TRY(ensure_consts(c));
    return dens_step_body(c, {dt, c->members}, {diff, c->members}, iters);
}

static int step_body(fluid_ctx* c, const MemberVal& dt, const MemberVal& diff, const MemberVal& visc, int iters, int nsteps, int use_sources)
{
    TRY(check_ctx(c));
    TRY(check_iters(iters));
    if (nsteps < 0) return fail(FLUID_E_INVALID, "nsteps < 0");
    for (int z = 0; z < nsteps; ++z) {
        if (!(use_sources && z == 0)) TRY(zero_sources(c));
        TRY(full_step(c, dt, diff, visc, iters));
    }
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_step(fluid_ctx* c, float dt, float diff, float visc, int iters, int nsteps, int use_sources) { return step_body(c, dt, diff, visc, iters, nsteps, use_sources); }

int fluid_step_members(fluid_ctx* c, const float* dt, const float* diff, const float* visc, int iters, int nsteps, int use_sources)
{
    TRY(check_member_args(c, "fluid_step_members", {{"dt", dt}, {"diff", diff}, {"visc", visc}}));
    if (c->members == 1) return fluid_step(c, dt[0], diff[0], visc[0], iters, nsteps, use_sources);
    TRY(ensure_consts(c));
    return step_body(c, {dt, c->members}, {diff, c->members}, {visc, c->members}, iters, nsteps, use_sources);
}

static int add_source_body(fluid_ctx* c, int x, int s, const MemberVal& dt)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {x, s}));
    if (x == s) return fail(FLUID_E_INVALID, "add_source: x and s must differ");
    TRY(op_add_source(c, x, s, dt));
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_op_add_source(fluid_ctx* c, int x, int s, float dt) { return add_source_body(c, x, s, dt); }

int fluid_op_add_source_members(fluid_ctx* c, int x, int s, const float* dt)
{
    TRY(check_member_args(c, "fluid_op_add_source_members", {{"dt", dt}}));
    if (c->members == 1) return fluid_op_add_source(c, x, s, dt[0]);
    TRY(ensure_consts(c));
    return add_source_body(c, x, s, {dt, c->members});
}

static int jacobi_sweep_body(fluid_ctx* c, int b, int x, int x0, int out, const MemberVal& alpha, const MemberVal& beta)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {x, x0, out}));
    TRY(check_b(b));
    if (out == x || out == x0) return fail(FLUID_E_INVALID, "jacobi_sweep: out must not alias an input");
    TRY(materialize(c, {x, x0}));
    TRY(need(c, {x}, 1));
    const float2* mab = nullptr;
    TRY(member_pairs(c, alpha, beta, &mab));
    const int v1 = c->variant == fluid::JACOBI_TB ? fluid::JACOBI_STREAM : c->variant;   // one sweep: nothing to block
    fluid::launch_jacobi(c->stream, c->st, v1, c->ptr(x), c->ptr(x0), c->ptr(out), c->pitch, c->n, c->own0, c->own1, alpha.at(0), beta.at(0),
                         b, c->mb(), mab);
    wrote(c, out, 0);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_op_jacobi_sweep(fluid_ctx* c, int b, int x, int x0, int out, float alpha, float beta) { return jacobi_sweep_body(c, b, x, x0, out, alpha, beta); }

int fluid_op_jacobi_sweep_members(fluid_ctx* c, int b, int x, int x0, int out, const float* alpha, const float* beta)
{
    TRY(check_member_args(c, "fluid_op_jacobi_sweep_members", {{"alpha", alpha}, {"beta", beta}}));
    if (c->members == 1) return fluid_op_jacobi_sweep(c, b, x, x0, out, alpha[0], beta[0]);
    TRY(ensure_consts(c));
    return jacobi_sweep_body(c, b, x, x0, out, {alpha, c->members}, {beta, c->members});
}

static int diffuse_body(fluid_ctx* c, int b, int x, int x0, const Coeffs& k, int iters)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {x, x0}));
    TRY(check_b(b));
    return op_diffuse(c, b, x, x0, k, iters);
}

int fluid_op_diffuse(fluid_ctx* c, int b, int x, int x0, float alpha, float beta, int iters) { return diffuse_body(c, b, x, x0, {alpha, beta}, iters); }

int fluid_op_diffuse_members(fluid_ctx* c, int b, int x, int x0, const float* alpha, const float* beta, int iters)
{
    TRY(check_member_args(c, "fluid_op_diffuse_members", {{"alpha", alpha}, {"beta", beta}}));
    if (c->members == 1) return fluid_op_diffuse(c, b, x, x0, alpha[0], beta[0], iters);
    TRY(ensure_consts(c));
    return diffuse_body(c, b, x, x0, {{alpha, c->members}, {beta, c->members}}, iters);
}

static int advect_body(fluid_ctx* c, int b, int d, int d0, int u, int v, const MemberVal& dt)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {d, d0, u, v}));
    TRY(check_b(b));
    if (d == d0 || d == u || d == v) return fail(FLUID_E_INVALID, "advect: output must not alias an input");
    if (c->nranks > 1) {                  // on this call's bound alone (no early guess: it would change the exchanges issued)
        float vmax = 0.f;
        bool fetched = false;
        TRY(vmax_begin(c, u, v));
        TRY(advect_rows(c, {d0}, dt.at(0) * (float)c->n, 0, &vmax, &fetched));     // (slabs: one member)
    }
    TRY(op_advect(c, b, d, d0, u, v, dt));
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_op_advect(fluid_ctx* c, int b, int d, int d0, int u, int v, float dt) { return advect_body(c, b, d, d0, u, v, dt); }

int fluid_op_advect_members(fluid_ctx* c, int b, int d, int d0, int u, int v, const float* dt)
{
    TRY(check_member_args(c, "fluid_op_advect_members", {{"dt", dt}}));
    if (c->members == 1) return fluid_op_advect(c, b, d, d0, u, v, dt[0]);
    TRY(ensure_consts(c));
    return advect_body(c, b, d, d0, u, v, {dt, c->members});
}

// ---- operators ---------------------------------------------------------------
int fluid_op_set_bnd(fluid_ctx* c, int b, int x)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {x}));
    TRY(check_b(b));
    if (c->nranks != 1) return fail(FLUID_E_INVALID, "fluid_op_set_bnd is a whole-grid operator (1 GPU)");
    TRY(materialize(c, x));
    fluid::launch_set_bnd(c->stream, c->st, c->ptr(x), c->pitch, c->n, b, c->mb());
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_op_divergence(fluid_ctx* c, int u, int v, int p, int div)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {u, v, p, div}));
    TRY(op_divergence(c, u, v, p, div));
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_op_subtract_gradient(fluid_ctx* c, int u, int v, int p)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {u, v, p}));
    TRY(op_subtract_gradient(c, u, v, p));
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

// ---- diagnostics --------------------------------------------------------------
int fluid_residual(fluid_ctx* c, int x, int x0, float alpha, float beta, float* out)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {x, x0}));
    if (!out) return fail(FLUID_E_INVALID, "null pointer");
    TRY(materialize(c, {x, x0}));
    TRY(need(c, {x}, 1));
    HIP_TRY(hipMemsetAsync(c->d_scalar, 0, sizeof(unsigned), c->stream));
    fluid::launch_residual(c->stream, c->st, c->ptr(x), c->ptr(x0), c->pitch, c->n, c->own0, c->own1, alpha, beta, c->d_scalar,
                           c->mb());      // (an ensemble: the maximum over all members)
    TRY(reduce_to_host(c, out));
    return exchange(c, FLUID_XCHG_MAX, {}, 0, out);
}

int fluid_absmax_velocity(fluid_ctx* c, int u, int v, float* out)
{
    TRY(check_ctx(c));
    TRY(check_fields(c, {u, v}));
    if (!out) return fail(FLUID_E_INVALID, "null pointer");
    TRY(materialize(c, {u, v}));
    HIP_TRY(hipMemsetAsync(c->d_scalar, 0, sizeof(unsigned), c->stream));
    fluid::launch_absmax2(c->stream, c->st, c->ptr(u), c->ptr(v), c->pitch, c->n, c->own0, c->own1, c->d_scalar, c->mb());
    TRY(reduce_to_host(c, out));
    return exchange(c, FLUID_XCHG_MAX, {}, 0, out);
}

// ---- ensemble diagnostics -----------------------------------------------------
// Results and scratch are Scratch buffers (fluid_ctx.h: EnsembleReduce), reserved by the first call that needs them.
static int ensure_member_results(fluid_ctx* c)
{
    EnsembleReduce& r = c->red;
    const size_t m = (size_t)c->members;
    const char* call = "ensemble diagnostics";
    TRY(reserve(c, r.max, m * sizeof(unsigned), false, call, "result words"));
    TRY(reserve(c, r.moments, m * sizeof(double2), true, call, "moments"));
    return reserve(c, r.partials, m * (size_t)fluid::moment_blocks(c->n, c->members) * sizeof(double2), false, call, "partial moments");
}

// the two statistics fields: zeroed once, so their pad columns (which no kernel writes) stay zero
static int ensure_stats(fluid_ctx* c)
{
    const size_t bytes = c->field_floats * sizeof(float);
    for (Scratch* s : {&c->red.mean, &c->red.var}) {
        bool grew = false;
        TRY(reserve(c, *s, bytes, false, "fluid_ensemble_stats", "a statistics field", &grew));
        if (!grew) continue;
        if (const hipError_t e = hipMemsetAsync(s->dev, 0, bytes, c->stream); e != hipSuccess) {
            s->release();                          // nothing was enqueued on it; never kept with pads that are not zero
            return fail(FLUID_E_HIP, "fluid_ensemble_stats: hipMemsetAsync: %s", hipGetErrorString(e));
        }
    }
    return FLUID_OK;
}

// the members' result words (non-negative floats) to the caller's array
static int member_words_to_host(fluid_ctx* c, float* out)
{
    const size_t bytes = (size_t)c->members * sizeof(unsigned);
    HIP_TRY(hipMemcpyAsync(c->red.moments.host, c->red.max.dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    std::memcpy(out, c->red.moments.host, bytes);
    return FLUID_OK;
}

int fluid_residual_members(fluid_ctx* c, int x, int x0, const float* alpha, const float* beta, float* out)
{
    TRY(check_member_args(c, "fluid_residual_members", {{"alpha", alpha}, {"beta", beta}}));
    if (!out) return fail(FLUID_E_INVALID, "fluid_residual_members: null array `out`");
    if (!c->valid_field(x) || !c->valid_field(x0)) return fail(FLUID_E_INVALID, "fluid_residual_members: bad field id %d", c->valid_field(x) ? x0 : x);
    if (c->members == 1) return fluid_residual(c, x, x0, alpha[0], beta[0], out);
    TRY(ensure_consts(c));
    TRY(ensure_member_results(c));
    TRY(materialize(c, {x, x0}));
    const float2* mab = nullptr;
    TRY(member_pairs(c, {alpha, c->members}, {beta, c->members}, &mab));
    HIP_TRY(hipMemsetAsync(c->red.max.d<unsigned>(), 0, (size_t)c->members * sizeof(unsigned), c->stream));
    fluid::launch_residual(c->stream, c->st, c->ptr(x), c->ptr(x0), c->pitch, c->n, c->own0, c->own1, alpha[0], beta[0], c->red.max.d<unsigned>(),
                           c->mb(), /*rstride=*/1, mab);
    HIP_TRY(hipGetLastError());
    return member_words_to_host(c, out);
}

int fluid_absmax_velocity_members(fluid_ctx* c, int u, int v, float* out)
{
    if (!c) return fail(FLUID_E_INVALID, "fluid_absmax_velocity_members: null context");
    if (!out) return fail(FLUID_E_INVALID, "fluid_absmax_velocity_members: null array `out`");
    if (!c->valid_field(u) || !c->valid_field(v)) return fail(FLUID_E_INVALID, "fluid_absmax_velocity_members: bad field id %d", c->valid_field(u) ? v : u);
    if (c->members == 1) return fluid_absmax_velocity(c, u, v, out);
    TRY(ensure_member_results(c));
    TRY(materialize(c, {u, v}));
    HIP_TRY(hipMemsetAsync(c->red.max.d<unsigned>(), 0, (size_t)c->members * sizeof(unsigned), c->stream));
    fluid::launch_absmax2(c->stream, c->st, c->ptr(u), c->ptr(v), c->pitch, c->n, c->own0, c->own1, c->red.max.d<unsigned>(), c->mb(), /*rstride=*/1);
    HIP_TRY(hipGetLastError());
    return member_words_to_host(c, out);
}

// a sum over the rows of other ranks would need an exchange kind the callback contract does not have
static int refuse_slabs(const fluid_ctx* c, const char* call)
{
    if (c->nranks > 1) return fail(FLUID_E_INVALID, "%s: not available on row slabs (this context is rank %d of %d)", call, c->rank, c->nranks);
    return FLUID_OK;
}

int fluid_member_moments(fluid_ctx* c, int field, double* sum, double* sumsq)
{
    if (!c) return fail(FLUID_E_INVALID, "fluid_member_moments: null context");
    if (!sum && !sumsq) return fail(FLUID_E_INVALID, "fluid_member_moments: `sum` and `sumsq` are both null");
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "fluid_member_moments: bad field id %d", field);
    TRY(refuse_slabs(c, "fluid_member_moments"));
    TRY(ensure_member_results(c));
    TRY(materialize(c, field));
    fluid::launch_member_moments(c->stream, c->st, c->ptr(field), c->pitch, c->n, c->mb(), c->red.partials.d<double2>(),
                                 c->red.moments.d<double2>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(c->red.moments.host, c->red.moments.dev, (size_t)c->members * sizeof(double2), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double2* h = c->red.moments.h<double2>();
    for (int m = 0; m < c->members; ++m) {
        if (sum) sum[m] = h[m].x;
        if (sumsq) sumsq[m] = h[m].y;
    }
    return FLUID_OK;
}

int fluid_member_gram(fluid_ctx* c, int field, int centre, double* gram)
{
    if (!gram) return fail(FLUID_E_INVALID, "fluid_member_gram: null array `gram`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_member_gram: null context");
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "fluid_member_gram: bad field id %d", field);
    if (c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "fluid_member_gram: this context has %d members, above FLUID_TRANSFORM_MAX_MEMBERS = %d", c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    TRY(refuse_slabs(c, "fluid_member_gram"));
    const int M = c->members, mp = fluid::gram_padded(M);
    const size_t matrix = (size_t)mp * mp * sizeof(double);
    EnsembleReduce& r = c->red;                    // sized for this context's N and M: reserved once
    TRY(reserve(c, r.gram_partials, matrix * (size_t)fluid::gram_blocks(c->n, M), false, "fluid_member_gram", "partial matrices"));
    TRY(reserve(c, r.gram, matrix, true, "fluid_member_gram", "the result"));
    const float inv = c->st != fluid::STORAGE_F32 ? 1.0f / c->field[field].fscale : 1.0f;      // as pack_range sees the field
    TRY(materialize(c, field, /*keep_scale=*/inv != 1.0f));
    fluid::launch_member_gram(c->stream, c->st, c->ptr(field), c->pitch, c->n, c->mb(), inv, centre != 0, r.gram_partials.d<double>(),
                              r.gram.d<double>());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(r.gram.host, r.gram.dev, matrix, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (int k = 0; k < M; ++k)                    // the upper triangle was computed; the lower one is its mirror
        for (int m = k; m < M; ++m) gram[(size_t)k * M + m] = gram[(size_t)m * M + k] = r.gram.h<double>()[(size_t)k * mp + m];
    return FLUID_OK;
}

int fluid_ensemble_stats(fluid_ctx* c, int field, float* mean, float* variance)
{
    if (!c) return fail(FLUID_E_INVALID, "fluid_ensemble_stats: null context");
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "fluid_ensemble_stats: bad field id %d", field);
    TRY(refuse_slabs(c, "fluid_ensemble_stats"));
    TRY(ensure_stats(c));
    TRY(materialize(c, field));
    fluid::launch_ensemble_stats(c->stream, c->st, c->ptr(field), c->pitch, c->n, c->mb(), c->red.mean.d<float>(),
                                 c->red.var.d<float>());
    HIP_TRY(hipGetLastError());
    c->red.have_stats = true;
    if (!mean && !variance) return FLUID_OK;       // computed only: the results stay on the device (fluid_ensemble_stats_ptr)
    const size_t hp = (size_t)c->w * sizeof(float), dp = (size_t)c->pitch * sizeof(float);
    if (mean) HIP_TRY(hipMemcpy2DAsync(mean, hp, c->red.mean.d<float>() + XOFF, dp, hp, (size_t)c->w, hipMemcpyDeviceToHost, c->stream));
    if (variance) HIP_TRY(hipMemcpy2DAsync(variance, hp, c->red.var.d<float>() + XOFF, dp, hp, (size_t)c->w, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FLUID_OK;
}

int fluid_ensemble_stats_ptr(fluid_ctx* c, void** mean_dev, void** variance_dev)
{
    if (!c) return fail(FLUID_E_INVALID, "fluid_ensemble_stats_ptr: null context");
    TRY(refuse_slabs(c, "fluid_ensemble_stats_ptr"));
    if (!c->red.have_stats) return fail(FLUID_E_INVALID, "fluid_ensemble_stats_ptr: no fluid_ensemble_stats has run on this context yet");
    if (mean_dev) *mean_dev = c->red.mean.dev;
    if (variance_dev) *variance_dev = c->red.var.dev;
    return FLUID_OK;
}

// ---- moving whole ensembles: device pack / unpack, bulk host copies, recorded runs ----------------------------
// (include/fluid_amd.h "moving ensembles".)  One launch moves all members of a field -- or a range of them -- between the
// library's layout and a dense float array on the device; the bulk host copies and fluid_run are built on it.  The
// launches belong to none of the timing categories.  Every refusal is found before anything is launched or changed.
// factor 0: a dense call; otherwise the cells of a member of a coarse dense array (the factor has passed check_factor)
static size_t member_cells(const fluid_ctx* c, int factor = 0)
{
    const size_t side = (size_t)(factor ? c->w / factor : c->w);
    return side * side;
}

// Inside this file factor 0 stands for the dense calls, which share their bodies with the coarse ones: an entry point that
// takes a factor from the caller refuses 0 here, before anything else, and every body checks a non-zero factor (check_factor).
static int refuse_factor_zero(const char* call, int factor)
{
    if (factor == 0) return fail(FLUID_E_INVALID, "%s: factor 0: the factor must be one of 1, 2, 4, 8, 16, 32, 64", call);
    return FLUID_OK;
}

// a coarse factor for a grid of N: one of 1, 2, 4 .. 64 that divides N + 2
static int check_factor(const char* call, int N, int factor)
{
    if (N < 1) return fail(FLUID_E_INVALID, "%s: N = %d, factor %d: N must be at least 1", call, N, factor);
    if (factor < 1 || factor > 64 || (factor & (factor - 1)) != 0)
        return fail(FLUID_E_INVALID, "%s: N = %d, factor %d: the factor must be one of 1, 2, 4, 8, 16, 32, 64", call, N, factor);
    if ((N + 2) % factor != 0)
        return fail(FLUID_E_INVALID, "%s: N = %d, factor %d: the factor must divide N + 2 = %d", call, N, factor, N + 2);
    return FLUID_OK;
}

// bytes from the first float of member 0 to the end of member count - 1 in a dense array; false: not representable
static bool dense_span(size_t cells, int count, size_t stride, size_t* bytes)
{
    size_t b = 0;
    if (count < 1) { *bytes = 0; return true; }
    if (__builtin_mul_overflow((size_t)(count - 1), stride, &b) || __builtin_add_overflow(b, cells, &b) ||
        __builtin_mul_overflow(b, sizeof(float), &b))
        return false;
    *bytes = b;
    return true;
}

// `p` is device memory of the context's device and the `bytes` behind it lie inside one allocation: asked on the host,
// so that a wrong pointer never reaches a kernel
static int check_device_span(const fluid_ctx* c, const char* call, const char* name, const void* p, size_t bytes)
{
    hipPointerAttribute_t a, own;
    std::memset(&a, 0, sizeof a);
    std::memset(&own, 0, sizeof own);
    hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess || a.type != hipMemoryTypeDevice) {
        (void)hipGetLastError();
        return fail(FLUID_E_INVALID, "%s: `%s` (%p) is not device memory", call, name, p);
    }
    e = hipPointerGetAttributes(&own, c->arena);
    if (e != hipSuccess) {
        (void)hipGetLastError();
        return fail(FLUID_E_HIP, "%s: hipPointerGetAttributes(arena): %s", call, hipGetErrorString(e));
    }
    if (a.device != own.device)
        return fail(FLUID_E_INVALID, "%s: `%s` (%p) is memory of device %d, this context's fields are on device %d", call, name, p, a.device,
                    own.device);
    void* base = nullptr;
    size_t size = 0;
    e = hipMemGetAddressRange(reinterpret_cast<hipDeviceptr_t*>(&base), &size, reinterpret_cast<hipDeviceptr_t>(const_cast<void*>(p)));
    if (e != hipSuccess || !base) {
        (void)hipGetLastError();
        return fail(FLUID_E_INVALID, "%s: `%s` (%p): no device allocation found around it", call, name, p);
    }
    const size_t off = (size_t)(static_cast<const char*>(p) - static_cast<const char*>(base));
    if (off > size || bytes > size - off)
        return fail(FLUID_E_INVALID, "%s: `%s` (%p) needs %zu bytes, its allocation ends %zu bytes behind it", call, name, p, bytes,
                    off > size ? (size_t)0 : size - off);
    if (((uintptr_t)p & 3u) != 0) return fail(FLUID_E_INVALID, "%s: `%s` (%p) is not aligned to 4 bytes", call, name, p);
    return FLUID_OK;
}

// first / count / member_stride as a pack or unpack call means them (0: to the end; 0: dense), and the device array behind them
// (factor: 0 for the dense calls; a coarse pack's array has ((N + 2) / factor)^2 cells per member)
static int check_member_move(const fluid_ctx* c, const char* call, int field, int first, int* count, const void* dev, size_t* stride,
                             int factor = 0)
{
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "%s: bad field id %d", call, field);
    TRY(refuse_slabs(c, call));
    if (factor) TRY(check_factor(call, c->n, factor));
    if (first < 0 || first > c->members || *count < 0 || *count > c->members - first)
        return fail(FLUID_E_INVALID, "%s: first %d, count %d outside the %d members of this context", call, first, *count, c->members);
    if (*count == 0) *count = c->members - first;
    const size_t cells = member_cells(c, factor);
    if (*stride == 0) *stride = cells;
    if (*stride < cells) {
        if (factor) return fail(FLUID_E_INVALID, "%s: member_stride %zu is below ((N + 2) / %d)^2 = %zu", call, *stride, factor, cells);
        return fail(FLUID_E_INVALID, "%s: member_stride %zu is below (N + 2)^2 = %zu", call, *stride, cells);
    }
    size_t bytes = 0;
    if (!dense_span(cells, *count, *stride, &bytes)) return fail(FLUID_E_INVALID, "%s: member_stride %zu is too large", call, *stride);
    return check_device_span(c, call, "the dense array", dev, bytes);
}

// as fluid_download_member sees the field: the lazy state settled, a scale kept and divided back on the way out.
// factor 0: the dense pack; a coarse factor: the block-averaged one -- factor 1 is the dense pack, bit for bit, and runs it.
static int pack_range(fluid_ctx* c, int field, int first, int count, float* dst, size_t stride, int factor = 0)
{
    if (count == 0) return FLUID_OK;
    const float inv = c->st != fluid::STORAGE_F32 ? 1.0f / c->field[field].fscale : 1.0f;
    TRY(materialize(c, field, /*keep_scale=*/inv != 1.0f));
    const char* x = static_cast<const char*>(c->ptr(field)) + (size_t)first * c->field_bytes;
    if (factor > 1) fluid::launch_pack_members_coarse(c->stream, c->st, x, c->pitch, c->n, {count, c->field_floats}, inv, factor, dst, stride);
    else fluid::launch_pack_members(c->stream, c->st, x, c->pitch, c->n, {count, c->field_floats}, inv, dst, stride);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

// the launch alone: what it means for the field's record is the caller's business (unpack_range, fluid_upload_members)
static int unpack_launch(fluid_ctx* c, int field, int first, int count, const float* src, size_t stride)
{
    char* x = static_cast<char*>(c->ptr(field)) + (size_t)first * c->field_bytes;
    fluid::launch_unpack_members(c->stream, c->st, x, c->pitch, c->n, {count, c->field_floats}, src, stride);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

// All members: the field is replaced -- nothing is settled first, whatever it owed itself is dropped (wrote).  A proper
// sub-range: the field is settled for all members first, as by fluid_upload_member (the marks are shared, and the members
// outside the range must end up holding what the marks stood for), then the range is overwritten.
static int unpack_range(fluid_ctx* c, int field, int first, int count, const float* src, size_t stride)
{
    if (count == 0) return FLUID_OK;
    const bool all = first == 0 && count == c->members;
    if (!all) TRY(materialize(c, field));
    TRY(unpack_launch(c, field, first, count, src, stride));
    if (all) wrote(c, field, kEverywhere);
    return FLUID_OK;
}

int fluid_pack_members(fluid_ctx* c, int field, int first, int count, void* dst_dev, size_t member_stride)
{
    if (!dst_dev) return fail(FLUID_E_INVALID, "fluid_pack_members: null device pointer `dst_dev`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_pack_members: null context");
    TRY(check_member_move(c, "fluid_pack_members", field, first, &count, dst_dev, &member_stride));
    return pack_range(c, field, first, count, static_cast<float*>(dst_dev), member_stride);
}

int fluid_coarse_size(int N, int factor, int* side)
{
    if (!side) return fail(FLUID_E_INVALID, "fluid_coarse_size: null pointer `side`");
    TRY(check_factor("fluid_coarse_size", N, factor));
    *side = (N + 2) / factor;
    return FLUID_OK;
}

int fluid_pack_members_coarse(fluid_ctx* c, int field, int first, int count, int factor, void* dst_dev, size_t member_stride)
{
    TRY(refuse_factor_zero("fluid_pack_members_coarse", factor));
    if (!dst_dev) return fail(FLUID_E_INVALID, "fluid_pack_members_coarse: null device pointer `dst_dev`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_pack_members_coarse: null context");
    TRY(check_member_move(c, "fluid_pack_members_coarse", field, first, &count, dst_dev, &member_stride, factor));
    return pack_range(c, field, first, count, static_cast<float*>(dst_dev), member_stride, factor);
}

int fluid_unpack_members(fluid_ctx* c, int field, int first, int count, const void* src_dev, size_t member_stride)
{
    if (!src_dev) return fail(FLUID_E_INVALID, "fluid_unpack_members: null device pointer `src_dev`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_unpack_members: null context");
    TRY(check_member_move(c, "fluid_unpack_members", field, first, &count, src_dev, &member_stride));
    return unpack_range(c, field, first, count, static_cast<const float*>(src_dev), member_stride);
}

// ---- recombining ensembles: fluid_transform_members / fluid_select_members -------------------------------------------
// (include/fluid_amd.h "recombining ensembles".)  One body: a selection is the transform with its one-hot matrix.  Per
// call one table -- the weights widened to double (exact), [M][MP], then one word per old member with a bit for every
// non-zero weight -- copied on the context's stream from pinned memory (fluid_ctx.h: TransformTables); per listed field
// one launch.  No wait anywhere; the launches belong to none of the timing categories.
static size_t transform_table_bytes(int members)
{
    return (size_t)members * (size_t)fluid::transform_padded(members) * sizeof(double) + (size_t)members * sizeof(unsigned long long);
}

// One call's table on its way to the device: `weights` -- M * M floats, weights[k * M + m] the weight of OLD member k in
// (the increment of) NEW member m, all finite (the entry points check) -- widened into the next slot of the ring and
// copied on the context's stream.  What the kernels take of it: the device addresses, `used` (a bit for every column with
// a term) and whether every weight of the M x M matrix is non-zero.
struct StagedTable {
    const double* table = nullptr;
    const unsigned long long* bits = nullptr;
    unsigned long long used = 0;
    bool dense = true;
};

static int stage_transform_table(fluid_ctx* c, const char* call, const float* weights, StagedTable* out)
{
    const int M = c->members, MP = fluid::transform_padded(M);
    TransformTables& t = c->xform;
    const size_t slot = const_pad(transform_table_bytes(M));
    TRY(reserve(c, t.tables, slot * TransformTables::kSlots, true, call, "weight tables"));
    for (hipEvent_t& ev : t.copied) TRY(ensure_event(&ev));
    const int s = t.next;
    if (t.in_use[s]) HIP_TRY(hipEventSynchronize(t.copied[s]));      // a formality unless kSlots calls are still queued
    double* table = t.tables.h<double>((size_t)s * slot);
    unsigned long long* bits = reinterpret_cast<unsigned long long*>(table + (size_t)M * MP);
    StagedTable st;
    for (int k = 0; k < M; ++k) {
        unsigned long long row = 0;
        for (int m = 0; m < MP; ++m) {
            const float w = m < M ? weights[(size_t)k * M + m] : 0.0f;
            table[(size_t)k * MP + m] = (double)w;
            if (w != 0.0f) row |= 1ull << m;
            else if (m < M) st.dense = false;
        }
        bits[k] = row;
        st.used |= row;
    }
    st.table = t.tables.d<double>((size_t)s * slot);
    HIP_TRY(hipMemcpyAsync(t.tables.d<char>((size_t)s * slot), table, transform_table_bytes(M), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipEventRecord(t.copied[s], c->stream));
    t.in_use[s] = true;
    t.next = (s + 1) % TransformTables::kSlots;
    st.bits = reinterpret_cast<const unsigned long long*>(st.table + (size_t)M * MP);
    *out = st;
    return FLUID_OK;
}

static int transform_body(fluid_ctx* c, const char* call, const int* fields, int nfields, const float* weights)
{
    StagedTable t;
    TRY(stage_transform_table(c, call, weights, &t));
    const unsigned long long empty = ~t.used;                        // (bits past M are never looked at)
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        const float inv = c->st != fluid::STORAGE_F32 ? 1.0f / c->field[f].fscale : 1.0f;      // as pack_range sees the field
        TRY(materialize(c, f, /*keep_scale=*/inv != 1.0f));
        fluid::launch_transform_members(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), inv, t.table, t.bits, empty, t.dense);
        HIP_TRY(hipGetLastError());
        wrote(c, f, kEverywhere);                                    // plain values (scale 1), nothing owed
    }
    return FLUID_OK;
}

// what both calls refuse beyond their own array, before anything is launched or changed
static int check_transform(const fluid_ctx* c, const char* call, const int* fields, int nfields)
{
    if (nfields < 1 || nfields > FLUID_NFIELDS) return fail(FLUID_E_INVALID, "%s: nfields %d outside [1, %d]", call, nfields, FLUID_NFIELDS);
    for (int k = 0; k < nfields; ++k) {
        if (!c->valid_field(fields[k])) return fail(FLUID_E_INVALID, "%s: bad field id %d (fields[%d])", call, fields[k], k);
        for (int j = 0; j < k; ++j)
            if (fields[j] == fields[k]) return fail(FLUID_E_INVALID, "%s: field %d is listed twice (fields[%d] and fields[%d])", call, fields[k], j, k);
    }
    if (c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: this context has %d members, above FLUID_TRANSFORM_MAX_MEMBERS = %d", call, c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    return refuse_slabs(c, call);
}

int fluid_transform_members(fluid_ctx* c, const int* fields, int nfields, const float* weights)
{
    static_assert(FLUID_TRANSFORM_MAX_MEMBERS == fluid::kTransformMaxMembers, "the header's cap is the kernel's");
    if (!fields) return fail(FLUID_E_INVALID, "fluid_transform_members: null array `fields`");
    if (!weights) return fail(FLUID_E_INVALID, "fluid_transform_members: null array `weights`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_transform_members: null context");
    TRY(check_transform(c, "fluid_transform_members", fields, nfields));
    const int M = c->members;
    for (int k = 0; k < M; ++k)
        for (int m = 0; m < M; ++m)
            if (!std::isfinite(weights[(size_t)k * M + m]))
                return fail(FLUID_E_INVALID, "fluid_transform_members: weights[%d * M + %d] (old member k = %d, new member m = %d) is not finite",
                            k, m, k, m);
    return transform_body(c, "fluid_transform_members", fields, nfields, weights);
}

int fluid_select_members(fluid_ctx* c, const int* fields, int nfields, const int* source)
{
    if (!fields) return fail(FLUID_E_INVALID, "fluid_select_members: null array `fields`");
    if (!source) return fail(FLUID_E_INVALID, "fluid_select_members: null array `source`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_select_members: null context");
    TRY(check_transform(c, "fluid_select_members", fields, nfields));
    const int M = c->members;
    std::vector<float> onehot((size_t)M * M, 0.0f);
    for (int m = 0; m < M; ++m) {
        if (source[m] < 0 || source[m] >= M)
            return fail(FLUID_E_INVALID, "fluid_select_members: source[%d] = %d (new member m = %d) outside [0, %d)", m, source[m], m, M);
        onehot[(size_t)source[m] * M + m] = 1.0f;
    }
    return transform_body(c, "fluid_select_members", fields, nfields, onehot.data());
}

// ---- localised updates: fluid_transform_members_local / fluid_taper_gaspari_cohn ------------------------------------------
// (include/fluid_amd.h "localised updates".)  The increment of a transform under a per-cell taper, over a box of cells: the
// table of increments goes through the ring of the transform (stage_transform_table), every listed field is settled as
// pack_range settles it -- what it owes itself is added, a scale is KEPT: the launch stores some cells only, and a pass
// over the others to divide a scale back would cost the grid, not the box, and round the half denormals -- and one launch
// per field covers the box.  No wait; the launches belong to none of the timing categories.
static const char* const kBoxEntry[4] = {"row_lo", "row_hi", "col_lo", "col_hi"};

int fluid_transform_members_local(fluid_ctx* c, const int* fields, int nfields, const float* increments, const void* taper_dev,
                                  const int* box)
{
    const char* call = "fluid_transform_members_local";
    if (!fields) return fail(FLUID_E_INVALID, "%s: null array `fields`", call);
    if (!increments) return fail(FLUID_E_INVALID, "%s: null array `increments`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(check_transform(c, call, fields, nfields));
    const int M = c->members;
    for (int k = 0; k < M; ++k)
        for (int m = 0; m < M; ++m)
            if (!std::isfinite(increments[(size_t)k * M + m]))
                return fail(FLUID_E_INVALID, "%s: increments[%d * M + %d] (old member k = %d, new member m = %d) is not finite", call, k, m, k, m);
    fluid::CellBox b = {0, c->w, 0, c->w};
    if (box) {
        for (int e = 0; e < 4; ++e)
            if (box[e] < 0 || box[e] > c->w)
                return fail(FLUID_E_INVALID, "%s: box[%d] = %d (%s) outside [0, %d]", call, e, box[e], kBoxEntry[e], c->w);
        for (int e = 0; e < 4; e += 2)
            if (box[e] > box[e + 1])
                return fail(FLUID_E_INVALID, "%s: box[%d] = %d (%s) is above box[%d] = %d (%s)", call, e, box[e], kBoxEntry[e], e + 1, box[e + 1],
                            kBoxEntry[e + 1]);
        b = {box[0], box[1], box[2], box[3]};
    }
    if (taper_dev) TRY(check_device_span(c, call, "taper_dev", taper_dev, member_cells(c) * sizeof(float)));
    StagedTable t;
    if (!b.empty()) TRY(stage_transform_table(c, call, increments, &t));
    const bool launch = !b.empty() && (t.used & (M < 64 ? (1ull << M) - 1 : ~0ull)) != 0;      // (no term anywhere: nothing is stored)
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        const float scale = c->st != fluid::STORAGE_F32 ? c->field[f].fscale : 1.0f;           // as pack_range sees the field
        TRY(materialize(c, f, /*keep_scale=*/scale != 1.0f));
        if (!launch) continue;
        fluid::launch_transform_members_local(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), 1.0f / scale, scale, t.table, t.bits,
                                              t.used, t.dense, static_cast<const float*>(taper_dev), b);
        HIP_TRY(hipGetLastError());
        wrote(c, f, kEverywhere);                                    // nothing owed ...
        c->field[f].fscale = scale;                                  // ... and the scale it had: the launch stored at it
    }
    return FLUID_OK;
}

// The cells a taper can be non-zero in, on the host: along each axis the indices whose cell on the nearest row (column) of
// the other axis has r < 2 -- r falls with the other axis' distance, rounding included, so no other row can add a column
// -- by the kernel's own function, then one cell more on each side: what a rounding that differs between the host and the
// device could move.  No such index: the empty box {0, 0, 0, 0}.
static void taper_box(const fluid_ctx* c, float col, float row, float hw, int* box)
{
    const double centre[2] = {(double)row, (double)col}, hwd = (double)hw;
    int first[2], last[2], nearest[2];
    for (int a = 0; a < 2; ++a) nearest[a] = std::min(c->w - 1, std::max(0, (int)std::lround(centre[a])));
    for (int a = 0; a < 2; ++a) {
        const double other = (double)nearest[1 - a] - centre[1 - a];
        const double reach = std::min(2.0 * hwd, (double)c->w) + 1.0;
        const int lo = (int)std::max(0.0, std::floor(centre[a] - reach)), hi = (int)std::min((double)(c->w - 1), std::ceil(centre[a] + reach));
        first[a] = c->w;
        last[a] = -1;
        for (int i = lo; i <= hi; ++i)
            if (fluid::taper_radius((double)i - centre[a], other, hwd) < 2.0) {
                first[a] = std::min(first[a], i);
                last[a] = i;
            }
    }
    if (last[0] < 0 || last[1] < 0) {
        box[0] = box[1] = box[2] = box[3] = 0;
        return;
    }
    for (int a = 0; a < 2; ++a) {
        box[2 * a] = std::max(0, first[a] - 1);
        box[2 * a + 1] = std::min(c->w, last[a] + 2);
    }
}

int fluid_taper_gaspari_cohn(fluid_ctx* c, float col, float row, float hw, void* out_dev, int* box)
{
    const char* call = "fluid_taper_gaspari_cohn";
    if (!out_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `out_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(refuse_slabs(c, call));
    const float top = (float)c->n + 0.5f;
    if (!std::isfinite(col) || col < 0.5f || col > top) return fail(FLUID_E_INVALID, "%s: col = %g is not finite or outside [0.5, %g]", call, (double)col, (double)top);
    if (!std::isfinite(row) || row < 0.5f || row > top) return fail(FLUID_E_INVALID, "%s: row = %g is not finite or outside [0.5, %g]", call, (double)row, (double)top);
    if (!std::isfinite(hw) || !(hw > 0.0f)) return fail(FLUID_E_INVALID, "%s: c = %g is not finite or not above 0", call, (double)hw);
    TRY(check_device_span(c, call, "out_dev", out_dev, member_cells(c) * sizeof(float)));
    fluid::launch_taper_gaspari_cohn(c->stream, static_cast<float*>(out_dev), c->n, col, row, hw);
    HIP_TRY(hipGetLastError());
    if (box) taper_box(c, col, row, hw, box);
    return FLUID_OK;
}

// ---- lattice updates: fluid_transform_members_lattice ---------------------------------------------------------------------
// (include/fluid_amd.h "lattice updates".)  The increments of every node go into ONE table buffer (fluid_ctx.h:
// LatticeNodeTables) and travel on the context's stream; every listed field is settled as the local call settles it, scale
// kept, and one launch per field covers the whole array.  No wait unless the call before this one has not finished copying
// its tables out of the pinned twin; the launches belong to none of the timing categories.
static int ensure_lattice(fluid_ctx* c, const char* call, size_t bytes)
{
    LatticeNodeTables& t = c->lattice;
    bool grew = false;
    TRY(reserve(c, t.tables, bytes, true, call, "node tables", &grew));
    if (grew) t.in_use = false;     // (the stream has been waited for: nothing copies out of a twin any more)
    return ensure_event(&t.copied);
}

int fluid_transform_members_lattice(fluid_ctx* c, const int* fields, int nfields, const float* increments, int nodes_row, int nodes_col,
                                    int row0, int col0, int step)
{
    const char* call = "fluid_transform_members_lattice";
    if (!fields) return fail(FLUID_E_INVALID, "%s: null array `fields`", call);
    if (!increments) return fail(FLUID_E_INVALID, "%s: null array `increments`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(check_transform(c, call, fields, nfields));
    if (nodes_row < 1) return fail(FLUID_E_INVALID, "%s: nodes_row = %d is below 1", call, nodes_row);
    if (nodes_col < 1) return fail(FLUID_E_INVALID, "%s: nodes_col = %d is below 1", call, nodes_col);
    if ((long long)nodes_row * (long long)nodes_col > FLUID_LATTICE_MAX_NODES)
        return fail(FLUID_E_INVALID, "%s: %d x %d = %lld nodes, above FLUID_LATTICE_MAX_NODES = %d", call, nodes_row, nodes_col,
                    (long long)nodes_row * (long long)nodes_col, FLUID_LATTICE_MAX_NODES);
    if (step < 8 || step % 8 != 0) return fail(FLUID_E_INVALID, "%s: step = %d is not a positive multiple of 8", call, step);
    const int M = c->members, MP = fluid::transform_padded(M), nodes = nodes_row * nodes_col;
    bool any = false;
    for (int node = 0; node < nodes; ++node)
        for (int k = 0; k < M; ++k)
            for (int m = 0; m < M; ++m) {
                const float d = increments[((size_t)node * M + k) * M + m];
                if (!std::isfinite(d))
                    return fail(FLUID_E_INVALID, "%s: the increment of node (a = %d, b = %d), old member k = %d, new member m = %d is not finite",
                                call, node / nodes_col, node % nodes_col, k, m);
                any = any || d != 0.0f;
            }
    fluid::LatticeTables dev;
    bool dense = true;
    if (any) {                                                       // (no term anywhere: nothing is stored, nothing staged)
        const size_t table_bytes = (size_t)nodes * M * MP * sizeof(double), bits_bytes = (size_t)nodes * M * sizeof(unsigned long long);
        const size_t bytes = table_bytes + bits_bytes + (size_t)nodes * sizeof(unsigned long long);
        TRY(ensure_lattice(c, call, bytes));
        LatticeNodeTables& t = c->lattice;
        if (t.in_use) HIP_TRY(hipEventSynchronize(t.copied));       // the call before may still be copying out of the twin
        double* table = t.tables.h<double>();
        unsigned long long* bits = t.tables.h<unsigned long long>(table_bytes);
        unsigned long long* cols = bits + (size_t)nodes * M;
        for (int node = 0; node < nodes; ++node) {
            unsigned long long all = 0;
            for (int k = 0; k < M; ++k) {
                unsigned long long row = 0;
                for (int m = 0; m < MP; ++m) {
                    const float d = m < M ? increments[((size_t)node * M + k) * M + m] : 0.0f;
                    table[((size_t)node * M + k) * MP + m] = (double)d;
                    if (d != 0.0f) row |= 1ull << m;
                    else if (m < M) dense = false;
                }
                bits[(size_t)node * M + k] = row;
                all |= row;
            }
            cols[node] = all;
        }
        HIP_TRY(hipMemcpyAsync(t.tables.dev, t.tables.host, bytes, hipMemcpyHostToDevice, c->stream));
        HIP_TRY(hipEventRecord(t.copied, c->stream));
        t.in_use = true;
        dev.table = t.tables.d<double>();
        dev.bits = t.tables.d<unsigned long long>(table_bytes);
        dev.cols = dev.bits + (size_t)nodes * M;
    }
    const fluid::Lattice lat = {nodes_row, nodes_col, row0, col0, step};
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        const float scale = c->st != fluid::STORAGE_F32 ? c->field[f].fscale : 1.0f;           // as pack_range sees the field
        TRY(materialize(c, f, /*keep_scale=*/scale != 1.0f));
        if (!any) continue;
        fluid::launch_transform_members_lattice(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), 1.0f / scale, scale, dev, dense, lat);
        HIP_TRY(hipGetLastError());
        wrote(c, f, kEverywhere);                                    // nothing owed ...
        c->field[f].fscale = scale;                                  // ... and the scale it had: the launch stored at it
    }
    return FLUID_OK;
}

// ---- relaxation to prior spread: fluid_member_spread / fluid_relax_spread ------------------------------------------------
// (include/fluid_amd.h "relaxation to prior spread".)  The list is checked as a transform's is, without its member cap: the
// kernels walk the members in a loop.  Every listed field is settled as pack_range settles it, a scale KEPT: the spread
// alters nothing, and the relaxation stores at the scale, as the lattice update does.  One launch per field, no wait; the
// launches belong to none of the timing categories.
static int check_spread(const fluid_ctx* c, const char* call, const int* fields, int nfields, const char* name, const void* dev,
                        size_t* stride)
{
    if (nfields < 1 || nfields > FLUID_NFIELDS) return fail(FLUID_E_INVALID, "%s: nfields %d outside [1, %d]", call, nfields, FLUID_NFIELDS);
    for (int k = 0; k < nfields; ++k) {
        if (!c->valid_field(fields[k])) return fail(FLUID_E_INVALID, "%s: bad field id %d (fields[%d])", call, fields[k], k);
        for (int j = 0; j < k; ++j)
            if (fields[j] == fields[k]) return fail(FLUID_E_INVALID, "%s: field %d is listed twice (fields[%d] and fields[%d])", call, fields[k], j, k);
    }
    TRY(refuse_slabs(c, call));                                          // (a slab context has one member: say what it is first)
    if (c->members < 2) return fail(FLUID_E_INVALID, "%s: this context has %d member(s); a spread needs at least 2", call, c->members);
    const size_t cells = member_cells(c);
    if (*stride == 0) *stride = cells;
    if (*stride < cells) return fail(FLUID_E_INVALID, "%s: field_stride %zu is below (N + 2)^2 = %zu", call, *stride, cells);
    size_t bytes = 0;
    if (!dense_span(cells, nfields, *stride, &bytes)) return fail(FLUID_E_INVALID, "%s: field_stride %zu is too large", call, *stride);
    return check_device_span(c, call, name, dev, bytes);
}

int fluid_member_spread(fluid_ctx* c, const int* fields, int nfields, void* out_dev, size_t field_stride)
{
    const char* call = "fluid_member_spread";
    if (!fields) return fail(FLUID_E_INVALID, "%s: null array `fields`", call);
    if (!out_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `out_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(check_spread(c, call, fields, nfields, "out_dev", out_dev, &field_stride));
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        const float inv = c->st != fluid::STORAGE_F32 ? 1.0f / c->field[f].fscale : 1.0f;      // as pack_range sees the field
        TRY(materialize(c, f, /*keep_scale=*/inv != 1.0f));
        fluid::launch_member_spread(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), inv, static_cast<float*>(out_dev) + (size_t)k * field_stride);
        HIP_TRY(hipGetLastError());
    }
    return FLUID_OK;
}

int fluid_relax_spread(fluid_ctx* c, const int* fields, int nfields, const void* prior_dev, size_t field_stride, float alpha)
{
    const char* call = "fluid_relax_spread";
    if (!fields) return fail(FLUID_E_INVALID, "%s: null array `fields`", call);
    if (!prior_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `prior_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (!std::isfinite(alpha) || alpha < 0.0f) return fail(FLUID_E_INVALID, "%s: alpha = %g is not finite or is negative", call, (double)alpha);
    TRY(check_spread(c, call, fields, nfields, "prior_dev", prior_dev, &field_stride));
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        const float scale = c->st != fluid::STORAGE_F32 ? c->field[f].fscale : 1.0f;           // as pack_range sees the field
        TRY(materialize(c, f, /*keep_scale=*/scale != 1.0f));
        fluid::launch_relax_spread(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), 1.0f / scale, scale,
                                   static_cast<const float*>(prior_dev) + (size_t)k * field_stride, alpha);
        HIP_TRY(hipGetLastError());
        wrote(c, f, kEverywhere);                                    // nothing owed ...
        c->field[f].fscale = scale;                                  // ... and the scale it had: the launch stored at it
    }
    return FLUID_OK;
}

// ---- verifying ensembles: fluid_verify_members ------------------------------------------------------------------------------
// (include/fluid_amd.h "verifying ensembles".)  The list and `truth_dev` are checked as a spread's are, then the member cap,
// the box as fluid_transform_members_local takes one, the flags and the other two device extents.  Every listed field is
// settled as pack_range settles it, a scale KEPT: scoring alters nothing.  At most two launches per field, no wait; the
// launches belong to none of the timing categories.
static_assert(FLUID_VERIFY_SUMS == fluid::kVerifySums && FLUID_VERIFY_ROW == fluid::kVerifyRow, "the header's row is the kernels' row");
static_assert((unsigned long long)(kMaxN + 2) * (kMaxN + 2) <= 0xffffffffull, "the cells of the largest box are counted in an unsigned");

int fluid_verify_members(fluid_ctx* c, const int* fields, int nfields, const void* truth_dev, size_t field_stride, const int* box, int flags,
                         void* crps_dev, void* scores_dev)
{
    const char* call = "fluid_verify_members";
    if (!fields) return fail(FLUID_E_INVALID, "%s: null array `fields`", call);
    if (!truth_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `truth_dev`", call);
    if (!scores_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `scores_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(check_spread(c, call, fields, nfields, "truth_dev", truth_dev, &field_stride));
    if (c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: this context has %d members, above FLUID_TRANSFORM_MAX_MEMBERS = %d", call, c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    fluid::CellBox b = {1, c->n + 1, 1, c->n + 1};
    if (box) {
        for (int e = 0; e < 4; ++e)
            if (box[e] < 0 || box[e] > c->w)
                return fail(FLUID_E_INVALID, "%s: box[%d] = %d (%s) outside [0, %d]", call, e, box[e], kBoxEntry[e], c->w);
        for (int e = 0; e < 4; e += 2)
            if (box[e] > box[e + 1])
                return fail(FLUID_E_INVALID, "%s: box[%d] = %d (%s) is above box[%d] = %d (%s)", call, e, box[e], kBoxEntry[e], e + 1, box[e + 1],
                            kBoxEntry[e + 1]);
        b = {box[0], box[1], box[2], box[3]};
    }
    if (flags & ~FLUID_VERIFY_FAIR) return fail(FLUID_E_INVALID, "%s: unknown flag bits 0x%x (FLUID_VERIFY_FAIR is the only flag)", call, (unsigned)flags);
    if (((uintptr_t)scores_dev & 7u) != 0) return fail(FLUID_E_INVALID, "%s: `scores_dev` (%p) is not aligned to 8 bytes", call, scores_dev);
    TRY(check_device_span(c, call, "scores_dev", scores_dev, (size_t)nfields * FLUID_VERIFY_ROW * sizeof(double)));
    if (crps_dev) {
        size_t bytes = 0;
        (void)dense_span(member_cells(c), nfields, field_stride, &bytes);      // (check_spread has found it representable)
        TRY(check_device_span(c, call, "crps_dev", crps_dev, bytes));
    }
    const int blocks = fluid::verify_blocks(b);
    if (blocks > 0) TRY(reserve(c, c->verify.partials, fluid::verify_partial_bytes(blocks), false, call, "partial scores"));
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        const float inv = c->st != fluid::STORAGE_F32 ? 1.0f / c->field[f].fscale : 1.0f;      // as pack_range sees the field
        TRY(materialize(c, f, /*keep_scale=*/inv != 1.0f));
        fluid::launch_verify_members(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), inv,
                                     static_cast<const float*>(truth_dev) + (size_t)k * field_stride, b, (flags & FLUID_VERIFY_FAIR) != 0,
                                     crps_dev ? static_cast<float*>(crps_dev) + (size_t)k * field_stride : nullptr, c->verify.partials.dev,
                                     static_cast<double*>(scores_dev) + (size_t)k * FLUID_VERIFY_ROW);
        HIP_TRY(hipGetLastError());
    }
    return FLUID_OK;
}

// ---- ensemble products: fluid_quantile_position / fluid_member_quantiles / fluid_member_exceedance --------------------------
// (include/fluid_amd.h "ensemble products".)  One field per call.  The null pointers, then the context, the count, the field,
// the list's values, then the slabs, the stride and the device extent, as a spread's are checked.  The field is settled as
// pack_range settles it, a scale KEPT: the products alter nothing.  ONE launch per call, no wait; the launches belong to
// none of the timing categories.
static_assert(FLUID_QUANTILE_MAX_LEVELS == fluid::kQuantileMaxLevels, "the header's level count is the kernels'");

static int check_products(const fluid_ctx* c, const char* call, const char* name, const void* dev, int count, size_t* stride)
{
    TRY(refuse_slabs(c, call));
    const size_t cells = member_cells(c);
    if (*stride == 0) *stride = cells;
    if (*stride < cells) return fail(FLUID_E_INVALID, "%s: level_stride %zu is below (N + 2)^2 = %zu", call, *stride, cells);
    size_t bytes = 0;
    if (!dense_span(cells, count, *stride, &bytes)) return fail(FLUID_E_INVALID, "%s: level_stride %zu is too large", call, *stride);
    return check_device_span(c, call, name, dev, bytes);
}

int fluid_quantile_position(int members, float level, int* lo, double* frac)
{
    const char* call = "fluid_quantile_position";
    if (!lo) return fail(FLUID_E_INVALID, "%s: null pointer `lo`", call);
    if (!frac) return fail(FLUID_E_INVALID, "%s: null pointer `frac`", call);
    if (members < 1 || members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: members %d outside [1, %d]", call, members, FLUID_TRANSFORM_MAX_MEMBERS);
    if (!std::isfinite(level) || level < 0.0f || level > 1.0f)
        return fail(FLUID_E_INVALID, "%s: level %g is not finite or lies outside [0, 1]", call, (double)level);
    fluid::quantile_position(members, level, lo, frac);
    return FLUID_OK;
}

int fluid_member_quantiles(fluid_ctx* c, int field, const float* levels, int nlevels, void* out_dev, size_t level_stride)
{
    const char* call = "fluid_member_quantiles";
    if (!levels) return fail(FLUID_E_INVALID, "%s: null array `levels`", call);
    if (!out_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `out_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (nlevels < 1 || nlevels > FLUID_QUANTILE_MAX_LEVELS)
        return fail(FLUID_E_INVALID, "%s: nlevels %d outside [1, %d]", call, nlevels, FLUID_QUANTILE_MAX_LEVELS);
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "%s: bad field id %d", call, field);
    for (int l = 0; l < nlevels; ++l)
        if (!std::isfinite(levels[l]) || levels[l] < 0.0f || levels[l] > 1.0f)
            return fail(FLUID_E_INVALID, "%s: levels[%d] = %g is not finite or lies outside [0, 1]", call, l, (double)levels[l]);
    if (c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: this context has %d members, above FLUID_TRANSFORM_MAX_MEMBERS = %d", call, c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    TRY(check_products(c, call, "out_dev", out_dev, nlevels, &level_stride));
    fluid::QuantileLevels lv = {};
    lv.count = nlevels;
    for (int l = 0; l < nlevels; ++l) fluid::quantile_position(c->members, levels[l], &lv.lo[l], &lv.frac[l]);
    const float inv = c->st != fluid::STORAGE_F32 ? 1.0f / c->field[field].fscale : 1.0f;      // as pack_range sees the field
    TRY(materialize(c, field, /*keep_scale=*/inv != 1.0f));
    fluid::launch_member_quantiles(c->stream, c->st, c->ptr(field), c->pitch, c->n, c->mb(), inv, lv, static_cast<float*>(out_dev), level_stride);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_member_exceedance(fluid_ctx* c, int field, const float* thresholds, int nthresholds, int mode, void* out_dev, size_t level_stride)
{
    const char* call = "fluid_member_exceedance";
    if (!thresholds) return fail(FLUID_E_INVALID, "%s: null array `thresholds`", call);
    if (!out_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `out_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (nthresholds < 1 || nthresholds > FLUID_QUANTILE_MAX_LEVELS)
        return fail(FLUID_E_INVALID, "%s: nthresholds %d outside [1, %d]", call, nthresholds, FLUID_QUANTILE_MAX_LEVELS);
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "%s: bad field id %d", call, field);
    for (int l = 0; l < nthresholds; ++l)
        if (!std::isfinite(thresholds[l])) return fail(FLUID_E_INVALID, "%s: thresholds[%d] = %g is not finite", call, l, (double)thresholds[l]);
    if (mode != FLUID_EXCEED_ABOVE && mode != FLUID_EXCEED_BELOW)
        return fail(FLUID_E_INVALID, "%s: mode %d is neither FLUID_EXCEED_ABOVE nor FLUID_EXCEED_BELOW", call, mode);
    TRY(check_products(c, call, "out_dev", out_dev, nthresholds, &level_stride));
    fluid::ExceedLevels lv = {};
    lv.count = nthresholds;
    for (int l = 0; l < nthresholds; ++l) lv.threshold[l] = thresholds[l];
    const float inv = c->st != fluid::STORAGE_F32 ? 1.0f / c->field[field].fscale : 1.0f;      // as pack_range sees the field
    TRY(materialize(c, field, /*keep_scale=*/inv != 1.0f));
    fluid::launch_member_exceedance(c->stream, c->st, c->ptr(field), c->pitch, c->n, c->mb(), inv, lv, mode == FLUID_EXCEED_BELOW,
                                    static_cast<float*>(out_dev), level_stride);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

// ---- ensemble noise: fluid_noise_members / fluid_noise_dense / fluid_noise_value -------------------------------------------
// (include/fluid_amd.h "ensemble noise".)  The list is checked as a spread's is, without its M >= 2 rule.  SET replaces the
// field in all members, as an unpack of all members does: nothing is settled, what the field owed itself is dropped, the
// scale becomes 1.  ADD settles the field as fluid_relax_spread does, a scale KEPT, and stores at it.  The amplitudes go
// through the ring of per-member constants (one member: by value).  One launch per field, no wait; the launches belong to
// none of the timing categories.
int fluid_noise_members(fluid_ctx* c, const int* fields, int nfields, int mode, const float* amplitude, unsigned long long seed,
                        unsigned int sequence, int member_offset)
{
    const char* call = "fluid_noise_members";
    if (!fields) return fail(FLUID_E_INVALID, "%s: null array `fields`", call);
    if (!amplitude) return fail(FLUID_E_INVALID, "%s: null array `amplitude`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (nfields < 1 || nfields > FLUID_NFIELDS) return fail(FLUID_E_INVALID, "%s: nfields %d outside [1, %d]", call, nfields, FLUID_NFIELDS);
    for (int k = 0; k < nfields; ++k) {
        if (!c->valid_field(fields[k])) return fail(FLUID_E_INVALID, "%s: bad field id %d (fields[%d])", call, fields[k], k);
        for (int j = 0; j < k; ++j)
            if (fields[j] == fields[k]) return fail(FLUID_E_INVALID, "%s: field %d is listed twice (fields[%d] and fields[%d])", call, fields[k], j, k);
    }
    if (mode != FLUID_NOISE_SET && mode != FLUID_NOISE_ADD)
        return fail(FLUID_E_INVALID, "%s: mode %d is neither FLUID_NOISE_SET nor FLUID_NOISE_ADD", call, mode);
    for (int m = 0; m < c->members; ++m)
        if (!std::isfinite(amplitude[m])) return fail(FLUID_E_INVALID, "%s: member %d: amplitude is not finite (%g)", call, m, (double)amplitude[m]);
    if (member_offset < 0 || member_offset > fluid::kNoiseIds - c->members)
        return fail(FLUID_E_INVALID, "%s: member_offset %d with %d member(s): member ids must lie in [0, %d]", call, member_offset, c->members,
                    fluid::kNoiseIds - 1);
    TRY(refuse_slabs(c, call));
    const bool add = mode == FLUID_NOISE_ADD;
    const fluid::NoiseKey key = {(unsigned)seed, (unsigned)(seed >> 32), sequence};
    const float* per_member = nullptr;
    if (c->members > 1) {
        TRY(ensure_consts(c));
        TRY(member_floats(c, MemberVal(amplitude, c->members), &per_member));
    }
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        float scale = 1.0f;
        if (add) {
            scale = c->st != fluid::STORAGE_F32 ? c->field[f].fscale : 1.0f;                  // as pack_range sees the field
            TRY(materialize(c, f, /*keep_scale=*/scale != 1.0f));
        }
        fluid::launch_noise_members(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), add, 1.0f / scale, scale, amplitude[0], per_member,
                                    key, f, member_offset);
        HIP_TRY(hipGetLastError());
        wrote(c, f, kEverywhere);                                    // nothing owed, plain values ...
        c->field[f].fscale = scale;                                  // ... or, ADD, the scale it had: the launch stored at it
    }
    return FLUID_OK;
}

int fluid_noise_dense(fluid_ctx* c, void* out_dev, size_t count, float amplitude, unsigned long long seed, unsigned int sequence, int stream_id)
{
    const char* call = "fluid_noise_dense";
    if (!out_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `out_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (!std::isfinite(amplitude)) return fail(FLUID_E_INVALID, "%s: amplitude is not finite (%g)", call, (double)amplitude);
    if (stream_id < 0 || stream_id >= fluid::kNoiseIds)
        return fail(FLUID_E_INVALID, "%s: stream_id %d outside [0, %d]", call, stream_id, fluid::kNoiseIds - 1);
    TRY(refuse_slabs(c, call));
    size_t bytes = 0;
    if (__builtin_mul_overflow(count, sizeof(float), &bytes)) return fail(FLUID_E_INVALID, "%s: count %zu is too large", call, count);
    TRY(check_device_span(c, call, "out_dev", out_dev, bytes));
    if (count == 0) return FLUID_OK;
    fluid::launch_noise_dense(c->stream, static_cast<float*>(out_dev), count, amplitude, {(unsigned)seed, (unsigned)(seed >> 32), sequence}, stream_id);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_noise_value(unsigned long long seed, unsigned int sequence, int tag, int member_id, unsigned int c0, unsigned int c1, double* z)
{
    const char* call = "fluid_noise_value";
    if (!z) return fail(FLUID_E_INVALID, "%s: null pointer `z`", call);
    if (tag < 0 || tag > fluid::kNoiseDenseTag) return fail(FLUID_E_INVALID, "%s: tag %d outside [0, %d]", call, tag, fluid::kNoiseDenseTag);
    if (member_id < 0 || member_id >= fluid::kNoiseIds)
        return fail(FLUID_E_INVALID, "%s: member_id %d outside [0, %d]", call, member_id, fluid::kNoiseIds - 1);
    *z = fluid::noise_z((unsigned)seed, (unsigned)(seed >> 32), c0, c1, fluid::noise_word2(tag, member_id), sequence);
    return FLUID_OK;
}

// The staging buffer of the bulk host copies: g = max(1, min(M, 64 MiB / member bytes)) dense members.  The 64 MiB is a
// choice, not a measurement -- a buffer that fits the Infinity Cache beside the fields a group is packed from;
// tools/ensemble_io_timing.py records what the bulk copies cost with it.
static int ensure_stage(fluid_ctx* c, const char* call)
{
    const size_t member_bytes = member_cells(c) * sizeof(float);
    c->stage.members = (int)std::max<size_t>(1, std::min<size_t>((size_t)c->members, ((size_t)64 << 20) / member_bytes));
    return reserve(c, c->stage.buf, (size_t)c->stage.members * member_bytes, false, call, "staging buffer");
}

// fluid_download_members (factor 0) / fluid_download_members_coarse: the same staging buffer, in groups of as many (coarse)
// members as fit in it
static int download_body(fluid_ctx* c, const char* call, int field, int factor, float* host)
{
    if (!host) return fail(FLUID_E_INVALID, "%s: null host pointer", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "%s: bad field id %d", call, field);
    TRY(refuse_slabs(c, call));
    if (factor) TRY(check_factor(call, c->n, factor));
    TRY(ensure_stage(c, call));
    const size_t cells = member_cells(c, factor);
    const int group = (int)std::min<size_t>((size_t)c->members, (size_t)c->stage.members * (member_cells(c) / cells));
    for (int first = 0; first < c->members; first += group) {      // groups in stream order: the buffer is reused
        const int count = std::min(group, c->members - first);
        TRY(pack_range(c, field, first, count, c->stage.dev(), cells, factor));
        HIP_TRY(hipMemcpyAsync(host + (size_t)first * cells, c->stage.dev(), (size_t)count * cells * sizeof(float), hipMemcpyDeviceToHost, c->stream));
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FLUID_OK;
}

int fluid_download_members(fluid_ctx* c, int field, float* host) { return download_body(c, "fluid_download_members", field, 0, host); }

int fluid_download_members_coarse(fluid_ctx* c, int field, int factor, float* host)
{
    TRY(refuse_factor_zero("fluid_download_members_coarse", factor));
    return download_body(c, "fluid_download_members_coarse", field, factor, host);
}

int fluid_upload_members(fluid_ctx* c, int field, const float* host)
{
    if (!host) return fail(FLUID_E_INVALID, "fluid_upload_members: null host pointer");
    if (!c) return fail(FLUID_E_INVALID, "fluid_upload_members: null context");
    if (!c->valid_field(field)) return fail(FLUID_E_INVALID, "fluid_upload_members: bad field id %d", field);
    TRY(refuse_slabs(c, "fluid_upload_members"));
    TRY(ensure_stage(c, "fluid_upload_members"));
    const size_t cells = member_cells(c);
    for (int first = 0; first < c->members; first += c->stage.members) {
        const int count = std::min(c->stage.members, c->members - first);
        HIP_TRY(hipMemcpyAsync(c->stage.dev(), host + (size_t)first * cells, (size_t)count * cells * sizeof(float), hipMemcpyHostToDevice, c->stream));
        TRY(unpack_launch(c, field, first, count, c->stage.dev(), cells));
    }
    wrote(c, field, kEverywhere);              // every member was replaced: an unpack of all members, in groups
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FLUID_OK;
}

// ---- observing ensembles: a resident network of points, the members' values at it, their Gram matrix --------------------
// (include/fluid_amd.h "observing ensembles".)  The network is a table in library-owned device memory outside the arena
// (fluid_ctx.h: Observation), built and validated on the host; the observing calls settle the field as a pack does and
// launch on the context's stream.  The launches belong to none of the timing categories.  Every refusal is found before
// anything is launched or changed.
// fluid_set_observation_points and fluid_set_observation_network (include/fluid_amd.h "typed networks"), under the caller's
// name: a null `field` is the untyped network, a table of 32 bytes per point; per-point fields add one byte per point.
static int set_network(fluid_ctx* c, const char* call, const float* col, const float* row, const int* field, int npoints)
{
    if (npoints != 0 && !col) return fail(FLUID_E_INVALID, "%s: null array `col`", call);
    if (npoints != 0 && !row) return fail(FLUID_E_INVALID, "%s: null array `row`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (npoints < 0 || npoints > FLUID_OBSERVE_MAX_POINTS)
        return fail(FLUID_E_INVALID, "%s: npoints %d outside [0, FLUID_OBSERVE_MAX_POINTS = %d]", call, npoints, FLUID_OBSERVE_MAX_POINTS);
    TRY(refuse_slabs(c, call));
    const double hi = (double)c->n + 0.5;
    for (int p = 0; p < npoints; ++p) {
        const float xy[2] = {col[p], row[p]};
        for (int a = 0; a < 2; ++a)
            if (!std::isfinite(xy[a]) || (double)xy[a] < 0.5 || (double)xy[a] > hi)
                return fail(FLUID_E_INVALID, "%s: point %d: %s = %g is not a finite value in [0.5, N + 0.5 = %g]", call, p, a ? "row" : "col",
                            (double)xy[a], hi);
    }
    static_assert(FLUID_NFIELDS == fluid::kObservedFields, "a point's field id indexes fluid::FieldSources");
    const bool typed = field && npoints > 0;
    unsigned mask = 0;
    if (typed)
        for (int p = 0; p < npoints; ++p) {
            if (field[p] < 0 || field[p] >= FLUID_NFIELDS)
                return fail(FLUID_E_INVALID, "%s: point %d: field = %d is outside [0, FLUID_NFIELDS = %d)", call, p, field[p], (int)FLUID_NFIELDS);
            mask |= 1u << field[p];
        }
    Observation& o = c->observe;
    char* table = nullptr;
    std::vector<unsigned char> ids;                                     // the points' field ids, typed only
    const size_t table_bytes = (size_t)npoints * (typed ? 33 : 32);
    if (npoints > 0) {
        const size_t P = (size_t)npoints;
        std::vector<char> host(P * 24);
        float* weight = reinterpret_cast<float*>(host.data());
        unsigned long long* tap = reinterpret_cast<unsigned long long*>(host.data() + P * 16);
        for (size_t p = 0; p < P; ++p) {
            const int j0 = (int)col[p], i0 = (int)row[p];             // at most N: every tap of the 2 x 2 stencil exists
            const float s1 = col[p] - (float)j0, t1 = row[p] - (float)i0;
            weight[4 * p + 0] = 1.0f - s1;
            weight[4 * p + 1] = s1;
            weight[4 * p + 2] = 1.0f - t1;
            weight[4 * p + 3] = t1;
            tap[p] = (unsigned long long)i0 * (unsigned long long)c->pitch + (unsigned long long)(fluid::XOFF + j0);
        }
        if (typed) {
            ids.resize(P);
            for (size_t p = 0; p < P; ++p) ids[p] = (unsigned char)field[p];
        }
        hipError_t e = hipMalloc((void**)&table, table_bytes);
        if (e == hipSuccess) e = hipMemcpyAsync(table, host.data(), host.size(), hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess && typed) e = hipMemcpyAsync(table + P * 32, ids.data(), P, hipMemcpyHostToDevice, c->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(c->stream);
        if (e != hipSuccess) {                                          // the old network stays in place
            if (table) (void)hipFree(table);
            (void)hipGetLastError();
            return fail(e == hipErrorOutOfMemory ? FLUID_E_NOMEM : FLUID_E_HIP, "%s: a table of %zu bytes: %s", call, table_bytes,
                        hipGetErrorString(e));
        }
    } else if (o.table) HIP_TRY(hipStreamSynchronize(c->stream));      // launches that still read the old table
    if (o.table) (void)hipFree(o.table);
    o.table = table;
    o.points = npoints;
    o.typed = typed;
    o.mask = mask;
    o.fields.swap(ids);
    o.qc_checked = false;                                               // (the threshold stays: fluid_set_observation_qc)
    LatticeGram& g = c->lgram;                                          // the positions fluid_observation_gram_lattice builds its lists from
    g.valid = false;
    g.coords.resize((size_t)npoints * 2);
    for (int p = 0; p < npoints; ++p) {
        g.coords[2 * (size_t)p] = col[p];
        g.coords[2 * (size_t)p + 1] = row[p];
    }
    return FLUID_OK;
}

int fluid_set_observation_points(fluid_ctx* c, const float* col, const float* row, int npoints)
{
    return set_network(c, "fluid_set_observation_points", col, row, nullptr, npoints);
}

int fluid_set_observation_network(fluid_ctx* c, const float* col, const float* row, const int* field, int npoints)
{
    return set_network(c, "fluid_set_observation_network", col, row, field, npoints);
}

int fluid_observation_network_fields(fluid_ctx* c, unsigned* mask)
{
    if (!mask) return fail(FLUID_E_INVALID, "fluid_observation_network_fields: null pointer `mask`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_observation_network_fields: null context");
    TRY(refuse_slabs(c, "fluid_observation_network_fields"));
    *mask = c->observe.mask;
    return FLUID_OK;
}

int fluid_observation_points(fluid_ctx* c, int* npoints)
{
    if (!npoints) return fail(FLUID_E_INVALID, "fluid_observation_points: null pointer `npoints`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_observation_points: null context");
    TRY(refuse_slabs(c, "fluid_observation_points"));
    *npoints = c->observe.points;
    return FLUID_OK;
}

// what the three observing calls refuse beyond their own pointers
static int check_observe(const fluid_ctx* c, const char* call, int field)
{
    if (field != FLUID_FIELD_OF_POINT && !c->valid_field(field)) return fail(FLUID_E_INVALID, "%s: bad field id %d", call, field);
    TRY(refuse_slabs(c, call));
    if (c->observe.points == 0) return fail(FLUID_E_INVALID, "%s: no observation network is set (fluid_set_observation_points)", call);
    if (field == FLUID_FIELD_OF_POINT && !c->observe.typed)
        return fail(FLUID_E_INVALID, "%s: field = FLUID_FIELD_OF_POINT needs a typed network (fluid_set_observation_network with per-point fields)",
                    call);
    return FLUID_OK;
}

static fluid::ObservationPoints observation_points(const fluid_ctx* c)
{
    return {c->observe.tap(), c->observe.weight(), c->observe.points, c->observe.field_of_point()};
}

// A record (include/fluid_amd.h "asynchronous observations") under the caller's name: member_stride 0 is P, anything else at
// least P, and the (M - 1) * stride + P floats lie inside one device allocation.  The network is set (check_observe).
static int check_record(const fluid_ctx* c, const char* call, const void* record_dev, size_t* member_stride)
{
    const size_t P = (size_t)c->observe.points;
    if (*member_stride == 0) *member_stride = P;
    if (*member_stride < P) return fail(FLUID_E_INVALID, "%s: member_stride %zu is below the %zu points of the network", call, *member_stride, P);
    size_t bytes = 0;
    if (!dense_span(P, c->members, *member_stride, &bytes)) return fail(FLUID_E_INVALID, "%s: member_stride %zu is too large", call, *member_stride);
    return check_device_span(c, call, "record_dev", record_dev, bytes);
}

// Where the h_k[p] of a Gram call come from: a field (or FLUID_FIELD_OF_POINT) sampled now, or -- `record` non-null, `field`
// is then not looked at -- the floats of a record.  One body per direct / recorded pair takes it.
struct GramSource {
    int field = 0;
    const void* record = nullptr;
    size_t stride = 0;
    explicit GramSource(int f) : field(f) {}
    GramSource(const void* r, size_t s) : record(r), stride(s) {}
};

// check_observe for either source; a record's stride comes back resolved
static int check_gram_source(const fluid_ctx* c, const char* call, GramSource* src)
{
    if (!src->record) return check_observe(c, call, src->field);
    TRY(refuse_slabs(c, call));
    if (c->observe.points == 0) return fail(FLUID_E_INVALID, "%s: no observation network is set (fluid_set_observation_points)", call);
    return check_record(c, call, src->record, &src->stride);
}

// What an observing launch reads: one field and its 1 / scale, or -- FLUID_FIELD_OF_POINT -- the table the points' field ids
// index.  As pack_range sees a field: the lazy state settled, a scale kept and divided back in the kernel.  The table is
// built after EVERY field of the network is settled, because settling one field may hand another one's buffer on.
// A record is read as it lies: no field is settled or looked at.
struct ObservedFrom {
    const void* x = nullptr;
    float inv = 1.0f;
    fluid::FieldSources table = {};
    bool typed = false;
    fluid::RecordedValues record = {};
    const fluid::FieldSources* sources() const { return typed ? &table : nullptr; }
    const fluid::RecordedValues* recorded() const { return record.h ? &record : nullptr; }
};

static int settle_for_observing(fluid_ctx* c, const GramSource& src, ObservedFrom* from)
{
    auto inv_of = [&](int f) { return c->st != fluid::STORAGE_F32 ? 1.0f / c->field[f].fscale : 1.0f; };
    const int field = src.field;
    if (src.record) {
        from->record = {static_cast<const float*>(src.record), src.stride};
        return FLUID_OK;
    }
    if (field != FLUID_FIELD_OF_POINT) {
        from->inv = inv_of(field);
        TRY(materialize(c, field, /*keep_scale=*/from->inv != 1.0f));
        from->x = c->ptr(field);
        return FLUID_OK;
    }
    from->typed = true;
    for (int f = 0; f < FLUID_NFIELDS; ++f)
        if (c->observe.mask >> f & 1u) {
            from->table.of[f].inv = inv_of(f);
            TRY(materialize(c, f, /*keep_scale=*/from->table.of[f].inv != 1.0f));
        }
    for (int f = 0; f < FLUID_NFIELDS; ++f)
        if (c->observe.mask >> f & 1u) from->table.of[f].base = reinterpret_cast<unsigned long long>(c->ptr(f));
    return FLUID_OK;
}

int fluid_observe_members(fluid_ctx* c, int field, void* out_dev, size_t member_stride)
{
    if (!out_dev) return fail(FLUID_E_INVALID, "fluid_observe_members: null device pointer `out_dev`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_observe_members: null context");
    TRY(check_observe(c, "fluid_observe_members", field));
    const size_t P = (size_t)c->observe.points;
    if (member_stride == 0) member_stride = P;
    if (member_stride < P) return fail(FLUID_E_INVALID, "fluid_observe_members: member_stride %zu is below the %zu points of the network", member_stride, P);
    size_t bytes = 0;
    if (!dense_span(P, c->members, member_stride, &bytes)) return fail(FLUID_E_INVALID, "fluid_observe_members: member_stride %zu is too large", member_stride);
    TRY(check_device_span(c, "fluid_observe_members", "out_dev", out_dev, bytes));
    ObservedFrom from;
    TRY(settle_for_observing(c, GramSource(field), &from));
    fluid::launch_observe_members(c->stream, c->st, from.x, c->pitch, c->mb(), from.inv, from.sources(), 0, observation_points(c), 0, (int)P,
                                  static_cast<float*>(out_dev), member_stride);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

// fluid_observe_members_range behind its checks, and every observation of fluid_run_window: the launch of
// fluid_observe_members with p0, np and the output pointer advanced by `first`.  An empty range launches and settles nothing.
static int observe_range(fluid_ctx* c, int field, int first, int count, void* record_dev, size_t member_stride)
{
    if (count == 0) return FLUID_OK;
    ObservedFrom from;
    TRY(settle_for_observing(c, GramSource(field), &from));
    fluid::launch_observe_members(c->stream, c->st, from.x, c->pitch, c->mb(), from.inv, from.sources(), 0, observation_points(c), first, count,
                                  static_cast<float*>(record_dev) + first, member_stride);
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

int fluid_observe_members_range(fluid_ctx* c, int field, int first, int count, void* record_dev, size_t member_stride)
{
    const char* call = "fluid_observe_members_range";
    if (!record_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `record_dev`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(check_observe(c, call, field));
    const int P = c->observe.points;
    if (first < 0 || first > P || count < 0 || count > P - first)
        return fail(FLUID_E_INVALID, "%s: first = %d, count = %d: the points [%d, %lld) do not lie inside the [0, %d) of the network", call, first,
                    count, first, (long long)first + (long long)count, P);
    TRY(check_record(c, call, record_dev, &member_stride));
    return observe_range(c, field, first, count, record_dev, member_stride);
}

// Through the staging buffer of fluid_download_members, whatever its size: as many whole members per group as fit in it,
// or -- a network larger than the buffer -- one member at a time in pieces of points.  Groups in stream order, one wait.
int fluid_observe_members_host(fluid_ctx* c, int field, float* host)
{
    if (!host) return fail(FLUID_E_INVALID, "fluid_observe_members_host: null host pointer `host`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_observe_members_host: null context");
    TRY(check_observe(c, "fluid_observe_members_host", field));
    TRY(ensure_stage(c, "fluid_observe_members_host"));
    ObservedFrom from;
    TRY(settle_for_observing(c, GramSource(field), &from));
    const size_t P = (size_t)c->observe.points, room = (size_t)c->stage.members * member_cells(c);
    const int group = (int)std::max<size_t>(1, std::min<size_t>((size_t)c->members, room / P));
    const size_t piece = std::min(P, room);
    const fluid::ObservationPoints pts = observation_points(c);
    for (int first = 0; first < c->members; first += group) {
        const int count = std::min(group, c->members - first);
        // one field: the group's first member by its address; the points' own fields: by its index, applied to every field's base
        const char* x = from.typed ? nullptr : static_cast<const char*>(from.x) + (size_t)first * c->field_bytes;
        for (size_t p0 = 0; p0 < P; p0 += piece) {                       // (one piece unless the network outgrows the buffer: count is 1 then)
            const size_t np = std::min(piece, P - p0);
            fluid::launch_observe_members(c->stream, c->st, x, c->pitch, {count, c->field_floats}, from.inv, from.sources(), first, pts, (int)p0,
                                          (int)np, c->stage.dev(), np);
            HIP_TRY(hipGetLastError());
            if (np == P)
                HIP_TRY(hipMemcpyAsync(host + (size_t)first * P, c->stage.dev(), (size_t)count * P * sizeof(float), hipMemcpyDeviceToHost, c->stream));
            else
                HIP_TRY(hipMemcpyAsync(host + (size_t)first * P + p0, c->stage.dev(), np * sizeof(float), hipMemcpyDeviceToHost, c->stream));
        }
    }
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FLUID_OK;
}

// ---- screening observations: the gate of the Gram and analysis calls (include/fluid_amd.h "screening observations") -------
// With a resident threshold above 0 a call that has `obs` screens the h it is about to use: one launch behind the uploads
// and the settling, in front of the Gram launch, no wait.  It leaves the flags in Observation::flags and 1 / sigma -- +0 at
// the rejected points, the caller's float or 1 elsewhere -- in Observation::sigma(), which the Gram launch then reads
// whether the caller gave an inv_sigma or not.  gate_reserve: with the call's other buffers, before anything is enqueued.
static bool gated(const fluid_ctx* c, const float* obs) { return c->observe.qc > 0.0f && obs; }

static int gate_reserve(fluid_ctx* c, const char* call, const float* obs)
{
    if (!gated(c, obs)) return FLUID_OK;
    return reserve(c, c->observe.flags, (size_t)c->observe.points, true, call, "screening flags");
}

// *sigma: the device buffer the Gram launch reads, null for none -- as the call had it without the gate
static int gate_launch(fluid_ctx* c, const ObservedFrom& from, const float* obs, const float* inv_sigma, const float** sigma)
{
    Observation& o = c->observe;
    *sigma = inv_sigma ? o.sigma() : nullptr;
    if (!gated(c, obs)) return FLUID_OK;
    fluid::ScreenOutputs out;
    out.sigma = o.sigma();
    out.flag = o.flags.d<unsigned char>();
    fluid::launch_observation_screen(c->stream, c->st, from.x, c->pitch, c->mb(), from.inv, from.sources(), observation_points(c), o.obs(), *sigma,
                                     o.qc, out, from.recorded());
    HIP_TRY(hipGetLastError());
    o.qc_checked = true;
    *sigma = o.sigma();
    return FLUID_OK;
}

// fluid_observation_gram / fluid_observation_gram_recorded: one body, under the caller's name
static int observation_gram_body(fluid_ctx* c, const char* call, GramSource src, int centre, const float* obs, const float* inv_sigma,
                                 double* gram, double* rhs, double* dd)
{
    if (!gram) return fail(FLUID_E_INVALID, "%s: null array `gram`", call);
    if (!obs && (rhs || dd)) return fail(FLUID_E_INVALID, "%s: `%s` is given but `obs` is null", call, rhs ? "rhs" : "dd");
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (!src.record && src.field != FLUID_FIELD_OF_POINT && !c->valid_field(src.field))
        return fail(FLUID_E_INVALID, "%s: bad field id %d", call, src.field);
    if (c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: this context has %d members, above FLUID_TRANSFORM_MAX_MEMBERS = %d", call, c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    TRY(check_gram_source(c, call, &src));
    Observation& o = c->observe;
    const size_t P = (size_t)o.points;
    if (inv_sigma)
        for (size_t p = 0; p < P; ++p)
            if (!std::isfinite(inv_sigma[p])) return fail(FLUID_E_INVALID, "%s: inv_sigma[%zu] (point %zu) is not finite", call, p, p);
    const int M = c->members, mp = fluid::gram_padded(M);
    const size_t entries = fluid::observation_gram_entries(M) * sizeof(double);
    // partials for the blocks of this network (a larger network later: they grow), the folded result and its twin
    TRY(reserve(c, o.partials, entries * (size_t)fluid::observation_gram_blocks(o.points, M), false, call, "partial results"));
    TRY(reserve(c, o.result, entries, true, call, "the result"));
    TRY(gate_reserve(c, call, obs));
    if (obs) HIP_TRY(hipMemcpyAsync(o.obs(), obs, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (inv_sigma) HIP_TRY(hipMemcpyAsync(o.sigma(), inv_sigma, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    ObservedFrom from;
    TRY(settle_for_observing(c, src, &from));
    const float* sigma = nullptr;
    TRY(gate_launch(c, from, obs, inv_sigma, &sigma));
    fluid::launch_observation_gram(c->stream, c->st, from.x, c->pitch, c->mb(), from.inv, from.sources(), observation_points(c), centre != 0,
                                   obs ? o.obs() : nullptr, sigma, o.partials.d<double>(), o.result.d<double>(), from.recorded());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(o.result.host, o.result.dev, entries, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    const double* host = o.result.h<double>();
    for (int k = 0; k < M; ++k)                    // the upper triangle was computed; the lower one is its mirror
        for (int m = k; m < M; ++m) gram[(size_t)k * M + m] = gram[(size_t)m * M + k] = host[(size_t)k * mp + m];
    if (rhs)
        for (int k = 0; k < M; ++k) rhs[k] = host[(size_t)mp * mp + k];
    if (dd) *dd = host[(size_t)mp * mp + mp];
    return FLUID_OK;
}

int fluid_observation_gram(fluid_ctx* c, int field, int centre, const float* obs, const float* inv_sigma, double* gram, double* rhs, double* dd)
{
    return observation_gram_body(c, "fluid_observation_gram", GramSource(field), centre, obs, inv_sigma, gram, rhs, dd);
}

int fluid_observation_gram_recorded(fluid_ctx* c, const void* record_dev, size_t member_stride, int centre, const float* obs,
                                    const float* inv_sigma, double* gram, double* rhs, double* dd)
{
    const char* call = "fluid_observation_gram_recorded";
    if (!record_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `record_dev`", call);
    return observation_gram_body(c, call, {record_dev, member_stride}, centre, obs, inv_sigma, gram, rhs, dd);
}

// ---- screening observations: fluid_observation_departures, the resident gate and its result --------------------------------
static int check_threshold(const char* call, float threshold)
{
    if (!std::isfinite(threshold) || threshold < 0.0f)
        return fail(FLUID_E_INVALID, "%s: threshold = %g is not finite or is negative", call, (double)threshold);
    return FLUID_OK;
}

// fluid_observation_departures / fluid_observation_departures_recorded: one body, under the caller's name.  The launch of
// the gate with every output asked for; the results come back through Observation::screen in one copy.
static int departures_body(fluid_ctx* c, const char* call, GramSource src, const float* obs, const float* inv_sigma, float threshold, float* mean,
                           float* spread, float* departure, unsigned char* rank, unsigned char* flag, double* sums)
{
    if (!obs && (departure || rank || flag || sums))
        return fail(FLUID_E_INVALID, "%s: `%s` is given but `obs` is null", call, departure ? "departure" : rank ? "rank" : flag ? "flag" : "sums");
    TRY(check_threshold(call, threshold));
    if (!obs && threshold != 0.0f) return fail(FLUID_E_INVALID, "%s: threshold = %g needs `obs`, which is null", call, (double)threshold);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (!src.record && src.field != FLUID_FIELD_OF_POINT && !c->valid_field(src.field))
        return fail(FLUID_E_INVALID, "%s: bad field id %d", call, src.field);
    TRY(refuse_slabs(c, call));                                          // (a slab context has one member: say what it is first)
    if (c->members < 2 || c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: this context has %d members, outside [2, FLUID_TRANSFORM_MAX_MEMBERS = %d]", call, c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    TRY(check_gram_source(c, call, &src));
    Observation& o = c->observe;
    const size_t P = (size_t)o.points;
    if (inv_sigma)
        for (size_t p = 0; p < P; ++p)
            if (!std::isfinite(inv_sigma[p])) return fail(FLUID_E_INVALID, "%s: inv_sigma[%zu] (point %zu) is not finite", call, p, p);
    constexpr size_t kSums = 32;                                         // three doubles, the floats behind them 16-byte aligned
    const size_t bytes = kSums + P * (3 * sizeof(float) + 2);
    TRY(reserve(c, o.screen, bytes, true, call, "the results"));
    if (sums) TRY(reserve(c, o.chunk_sums, fluid::observation_screen_chunks(o.points) * 3 * sizeof(double), false, call, "partial sums"));
    if (obs) HIP_TRY(hipMemcpyAsync(o.obs(), obs, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (inv_sigma) HIP_TRY(hipMemcpyAsync(o.sigma(), inv_sigma, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    ObservedFrom from;
    TRY(settle_for_observing(c, src, &from));
    fluid::ScreenOutputs out;
    out.mean = o.screen.d<float>(kSums);
    out.spread = out.mean + P;
    if (obs) {
        out.departure = out.spread + P;
        out.rank = o.screen.d<unsigned char>(kSums + P * 3 * sizeof(float));
        out.flag = out.rank + P;
    }
    if (sums) {
        out.chunk_sums = o.chunk_sums.d<double>();
        out.sums = o.screen.d<double>();
    }
    fluid::launch_observation_screen(c->stream, c->st, from.x, c->pitch, c->mb(), from.inv, from.sources(), observation_points(c),
                                     obs ? o.obs() : nullptr, inv_sigma ? o.sigma() : nullptr, threshold, out, from.recorded());
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(o.screen.host, o.screen.dev, bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->etkf.in_flight = false;
    const float* hf = o.screen.h<float>(kSums);
    const unsigned char* hb = o.screen.h<unsigned char>(kSums + P * 3 * sizeof(float));
    if (mean) std::memcpy(mean, hf, P * sizeof(float));
    if (spread) std::memcpy(spread, hf + P, P * sizeof(float));
    if (departure) std::memcpy(departure, hf + 2 * P, P * sizeof(float));
    if (rank) std::memcpy(rank, hb, P);
    if (flag) std::memcpy(flag, hb + P, P);
    if (sums) std::memcpy(sums, o.screen.host, 3 * sizeof(double));
    return FLUID_OK;
}

int fluid_observation_departures(fluid_ctx* c, int field, const float* obs, const float* inv_sigma, float threshold, float* mean, float* spread,
                                 float* departure, unsigned char* rank, unsigned char* flag, double* sums)
{
    return departures_body(c, "fluid_observation_departures", GramSource(field), obs, inv_sigma, threshold, mean, spread, departure, rank, flag, sums);
}

int fluid_observation_departures_recorded(fluid_ctx* c, const void* record_dev, size_t member_stride, const float* obs, const float* inv_sigma,
                                          float threshold, float* mean, float* spread, float* departure, unsigned char* rank,
                                          unsigned char* flag, double* sums)
{
    const char* call = "fluid_observation_departures_recorded";
    if (!record_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `record_dev`", call);
    return departures_body(c, call, {record_dev, member_stride}, obs, inv_sigma, threshold, mean, spread, departure, rank, flag, sums);
}

int fluid_set_observation_qc(fluid_ctx* c, float threshold)
{
    const char* call = "fluid_set_observation_qc";
    TRY(check_threshold(call, threshold));
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(refuse_slabs(c, call));
    if (c->members < 2) return fail(FLUID_E_INVALID, "%s: this context has %d members, below 2", call, c->members);
    c->observe.qc = threshold;
    return FLUID_OK;
}

int fluid_observation_qc(fluid_ctx* c, float* threshold)
{
    if (!threshold) return fail(FLUID_E_INVALID, "fluid_observation_qc: null pointer `threshold`");
    if (!c) return fail(FLUID_E_INVALID, "fluid_observation_qc: null context");
    *threshold = c->observe.qc;
    return FLUID_OK;
}

int fluid_observation_qc_result(fluid_ctx* c, unsigned char* flags, int* checked, int* rejected)
{
    const char* call = "fluid_observation_qc_result";
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    Observation& o = c->observe;
    if (!o.qc_checked) return fail(FLUID_E_INVALID, "%s: no gated call has run on this network (fluid_set_observation_qc)", call);
    const size_t P = (size_t)o.points;
    HIP_TRY(hipMemcpyAsync(o.flags.host, o.flags.dev, P, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->etkf.in_flight = false;
    const unsigned char* h = o.flags.h<unsigned char>();
    int n = 0;
    for (size_t p = 0; p < P; ++p) n += h[p] != 0;
    if (flags) std::memcpy(flags, h, P);
    if (checked) *checked = (int)P;
    if (rejected) *rejected = n;
    return FLUID_OK;
}

// ---- lattice observations: fluid_observation_gram_lattice ------------------------------------------------------------------
// (include/fluid_amd.h "lattice observations".)  Which points a node sees is found here, on the host, from the copy of the
// network's positions fluid_set_observation_points keeps: per point only the nodes whose row and column lie within 2c of it
// (from the lattice geometry, one node of margin on each side) are tried, and the weight is the taper kernel's own function.
// `fn(node, point, w)` is called for every pair with w != 0, points in increasing order.
extern "C++" {
template <typename F>
static void lattice_pairs(const fluid_ctx* c, int nodes_row, int nodes_col, int row0, int col0, int step, float hw, F fn)
{
    const double reach = 2.0 * (double)hw, hwd = (double)hw, s = (double)step;
    const size_t P = (size_t)c->observe.points;
    auto range = [&](double x, int origin, int count, int* lo, int* hi) {    // nodes origin + i * step with |x - node| <= reach, and one more
        const double a = std::floor((x - reach - (double)origin) / s) - 1.0, b = std::ceil((x + reach - (double)origin) / s) + 1.0;
        *lo = a <= 0.0 ? 0 : a >= (double)count ? count : (int)a;
        *hi = b < 0.0 ? -1 : b >= (double)(count - 1) ? count - 1 : (int)b;
    };
    for (size_t p = 0; p < P; ++p) {
        const double col = (double)c->lgram.coords[2 * p], row = (double)c->lgram.coords[2 * p + 1];
        int a_lo, a_hi, b_lo, b_hi;
        range(row, row0, nodes_row, &a_lo, &a_hi);
        range(col, col0, nodes_col, &b_lo, &b_hi);
        for (int a = a_lo; a <= a_hi; ++a) {
            const double dy = row - (double)((long long)row0 + (long long)a * step);
            for (int b = b_lo; b <= b_hi; ++b) {
                const double dx = col - (double)((long long)col0 + (long long)b * step);
                const float w = (float)fluid::taper_value(fluid::taper_radius(dx, dy, hwd));
                if (w != 0.0f) fn(a * nodes_col + b, (int)p, w);
            }
        }
    }
}
}  // extern "C++"

// What fluid_observation_gram_lattice and fluid_analyse_lattice share, under the caller's name: the refusals beyond the
// call's own pointers, the point lists (built, cached and uploaded here and nowhere else), and the two launches that leave
// every node's result in LatticeGram::out.  Nothing is waited for, except where the lists an analysis in flight may still
// read are about to be rewritten, or a buffer grows (reserve).
static int enqueue_lattice_gram(fluid_ctx* c, const char* call, GramSource src, int centre, const float* obs, const float* inv_sigma,
                                int nodes_row, int nodes_col, int row0, int col0, int step, float hw)
{
    TRY(check_gram_source(c, call, &src));
    if (c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: this context has %d members, above FLUID_TRANSFORM_MAX_MEMBERS = %d", call, c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    if (nodes_row < 1) return fail(FLUID_E_INVALID, "%s: nodes_row = %d is below 1", call, nodes_row);
    if (nodes_col < 1) return fail(FLUID_E_INVALID, "%s: nodes_col = %d is below 1", call, nodes_col);
    if ((long long)nodes_row * (long long)nodes_col > FLUID_LATTICE_MAX_NODES)
        return fail(FLUID_E_INVALID, "%s: %d x %d = %lld nodes, above FLUID_LATTICE_MAX_NODES = %d", call, nodes_row, nodes_col,
                    (long long)nodes_row * (long long)nodes_col, FLUID_LATTICE_MAX_NODES);
    if (step < 8 || step % 8 != 0) return fail(FLUID_E_INVALID, "%s: step = %d is not a positive multiple of 8", call, step);
    if (!std::isfinite(hw) || !(hw > 0.0f)) return fail(FLUID_E_INVALID, "%s: c = %g is not finite or not above 0", call, (double)hw);
    Observation& o = c->observe;
    LatticeGram& g = c->lgram;
    const size_t P = (size_t)o.points, B = (size_t)nodes_row * (size_t)nodes_col;
    if (inv_sigma)
        for (size_t p = 0; p < P; ++p)
            if (!std::isfinite(inv_sigma[p])) return fail(FLUID_E_INVALID, "%s: inv_sigma[%zu] (point %zu) is not finite", call, p, p);

    // the lists of the call before serve when the network, the lattice and c are the same
    const bool cached = g.valid && g.nodes_row == nodes_row && g.nodes_col == nodes_col && g.row0 == row0 && g.col0 == col0 &&
                        g.step == step && g.c == hw;
    std::vector<int> start;                                              // start[node + 1]: the entries of the nodes up to and with `node`
    long long pairs = g.pairs;
    if (!cached && c->etkf.in_flight) {                                  // an analysis may still read the lists about to be replaced
        HIP_TRY(hipStreamSynchronize(c->stream));
        c->etkf.in_flight = false;
    }
    if (!cached) {
        start.assign(B + 1, 0);
        pairs = 0;
        lattice_pairs(c, nodes_row, nodes_col, row0, col0, step, hw, [&](int node, int, float) {
            ++start[(size_t)node + 1];
            ++pairs;
        });
        if (pairs > (long long)FLUID_LATTICE_GRAM_MAX_ENTRIES)
            return fail(FLUID_E_INVALID, "%s: the nodes see %lld (point, node) pairs, above FLUID_LATTICE_GRAM_MAX_ENTRIES = %d", call, pairs,
                        FLUID_LATTICE_GRAM_MAX_ENTRIES);
        for (size_t b = 0; b < B; ++b) start[b + 1] += start[b];
    }
    const int M = c->members, mp = fluid::gram_padded(M);
    const size_t E = fluid::observation_gram_entries(M), start_bytes = ((B + 1) * sizeof(int) + 7) & ~(size_t)7;
    const size_t list_bytes = start_bytes + (size_t)pairs * sizeof(int2);
    bool grew = false;
    TRY(reserve(c, g.lists, list_bytes, true, call, "point lists", &grew));
    if (grew) g.valid = false;                                           // (not cached, then) the old lists went with the old buffer
    TRY(reserve(c, g.operands, P * (size_t)(mp + 2) * sizeof(double), false, call, "point operands"));
    TRY(reserve(c, g.out, B * E * sizeof(double), true, call, "node results"));
    TRY(gate_reserve(c, call, obs));
    int* h_start = g.lists.h<int>();
    int2* h_entry = g.lists.h<int2>(start_bytes);
    if (!cached) {
        g.valid = false;
        std::vector<int> at(start.begin(), start.end() - 1);             // where the next entry of a node goes
        bool inside = true;
        lattice_pairs(c, nodes_row, nodes_col, row0, col0, step, hw, [&](int node, int p, float w) {
            const int slot = at[(size_t)node]++;
            if (slot >= start[(size_t)node + 1] || p < 0 || (size_t)p >= P) { inside = false; return; }
            unsigned bits;
            std::memcpy(&bits, &w, sizeof bits);
            h_entry[slot] = make_int2(p, (int)bits);
        });
        for (size_t b = 0; b < B; ++b) inside = inside && at[b] == start[b + 1];
        if (!inside) return fail(FLUID_E_INVALID, "%s: the point lists do not match their count (internal error)", call);
        std::memcpy(h_start, start.data(), (B + 1) * sizeof(int));
        HIP_TRY(hipMemcpyAsync(g.lists.dev, g.lists.host, list_bytes, hipMemcpyHostToDevice, c->stream));
        g.nodes_row = nodes_row; g.nodes_col = nodes_col; g.row0 = row0; g.col0 = col0; g.step = step; g.c = hw;
        g.pairs = pairs;
        g.valid = true;
    }
    if (obs) HIP_TRY(hipMemcpyAsync(o.obs(), obs, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    if (inv_sigma) HIP_TRY(hipMemcpyAsync(o.sigma(), inv_sigma, P * sizeof(float), hipMemcpyHostToDevice, c->stream));
    ObservedFrom from;
    TRY(settle_for_observing(c, src, &from));
    const float* sigma = nullptr;
    TRY(gate_launch(c, from, obs, inv_sigma, &sigma));
    const fluid::LatticeLists lists = {g.lists.d<int>(), g.lists.d<int2>(start_bytes), (int)B};
    fluid::launch_observation_gram_lattice(c->stream, c->st, from.x, c->pitch, c->mb(), from.inv, from.sources(), observation_points(c), centre != 0,
                                           obs ? o.obs() : nullptr, sigma, g.operands.d<double>(), lists, g.out.d<double>(), from.recorded());
    HIP_TRY(hipGetLastError());
    return FLUID_OK;
}

// fluid_observation_gram_lattice / fluid_observation_gram_lattice_recorded: one body, under the caller's name
static int lattice_gram_body(fluid_ctx* c, const char* call, const GramSource& src, int centre, const float* obs, const float* inv_sigma,
                             int nodes_row, int nodes_col, int row0, int col0, int step, float hw, double* gram, double* rhs, double* dd,
                             int* counts)
{
    if (!gram) return fail(FLUID_E_INVALID, "%s: null array `gram`", call);
    if (!obs && (rhs || dd)) return fail(FLUID_E_INVALID, "%s: `%s` is given but `obs` is null", call, rhs ? "rhs" : "dd");
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(enqueue_lattice_gram(c, call, src, centre, obs, inv_sigma, nodes_row, nodes_col, row0, col0, step, hw));
    LatticeGram& g = c->lgram;
    const size_t B = (size_t)nodes_row * (size_t)nodes_col;
    const int M = c->members, mp = fluid::gram_padded(M);
    const size_t E = fluid::observation_gram_entries(M);
    const int* h_start = g.lists.h<int>();
    HIP_TRY(hipMemcpyAsync(g.out.host, g.out.dev, B * E * sizeof(double), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->etkf.in_flight = false;
    for (size_t b = 0; b < B; ++b) {
        const int count = h_start[b + 1] - h_start[b];
        const double* r = g.out.h<double>() + b * E;
        double* gm = gram + b * (size_t)M * M;
        if (counts) counts[b] = count;
        for (int k = 0; k < M; ++k)                // k <= m was computed (an empty node: nothing was); the rest is its mirror
            for (int m = k; m < M; ++m) gm[(size_t)k * M + m] = gm[(size_t)m * M + k] = count ? r[(size_t)k * mp + m] : 0.0;
        if (rhs)
            for (int k = 0; k < M; ++k) rhs[b * M + k] = count ? r[(size_t)mp * mp + k] : 0.0;
        if (dd) dd[b] = count ? r[(size_t)mp * mp + mp] : 0.0;
    }
    return FLUID_OK;
}

int fluid_observation_gram_lattice(fluid_ctx* c, int field, int centre, const float* obs, const float* inv_sigma, int nodes_row, int nodes_col,
                                   int row0, int col0, int step, float hw, double* gram, double* rhs, double* dd, int* counts)
{
    return lattice_gram_body(c, "fluid_observation_gram_lattice", GramSource(field), centre, obs, inv_sigma, nodes_row, nodes_col, row0, col0, step, hw,
                             gram, rhs, dd, counts);
}

int fluid_observation_gram_lattice_recorded(fluid_ctx* c, const void* record_dev, size_t member_stride, int centre, const float* obs,
                                            const float* inv_sigma, int nodes_row, int nodes_col, int row0, int col0, int step, float hw,
                                            double* gram, double* rhs, double* dd, int* counts)
{
    const char* call = "fluid_observation_gram_lattice_recorded";
    if (!record_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `record_dev`", call);
    return lattice_gram_body(c, call, {record_dev, member_stride}, centre, obs, inv_sigma, nodes_row, nodes_col, row0, col0, step, hw, gram, rhs,
                             dd, counts);
}

// ---- one-call analysis: fluid_etkf_increments, fluid_analyse_lattice, fluid_analyse_lattice_status -------------------------
// (include/fluid_amd.h "one-call analysis".)  One kernel solves every node (fluid_kernels.hip: k_etkf_solve); the host
// route feeds it from and to host arrays through the buffers of EtkfBuffers and waits, the fused route points it at the
// results fluid_observation_gram_lattice's launches leave on the device and at the node tables the lattice launch reads,
// and waits for nothing.
static int check_etkf(const fluid_ctx* c, const char* call, float rho)
{
    static_assert(FLUID_ETKF_MAX_SWEEPS == fluid::kEtkfMaxSweeps, "the header's cap is the kernel's");
    TRY(refuse_slabs(c, call));                                          // (a slab context has one member: say what it is first)
    if (c->members < 2) return fail(FLUID_E_INVALID, "%s: this context has %d members, below 2", call, c->members);
    if (c->members > FLUID_TRANSFORM_MAX_MEMBERS)
        return fail(FLUID_E_INVALID, "%s: this context has %d members, above FLUID_TRANSFORM_MAX_MEMBERS = %d", call, c->members,
                    FLUID_TRANSFORM_MAX_MEMBERS);
    if (!std::isfinite(rho) || !(rho > 0.0f)) return fail(FLUID_E_INVALID, "%s: rho = %g is not finite or not above 0", call, (double)rho);
    return FLUID_OK;
}

int fluid_etkf_increments(fluid_ctx* c, int nodes, const double* gram, const double* rhs, const int* counts, float rho, float* increments,
                          int* status)
{
    const char* call = "fluid_etkf_increments";
    if (!gram) return fail(FLUID_E_INVALID, "%s: null array `gram`", call);
    if (!rhs) return fail(FLUID_E_INVALID, "%s: null array `rhs`", call);
    if (!increments) return fail(FLUID_E_INVALID, "%s: null array `increments`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    if (nodes < 1 || nodes > FLUID_LATTICE_MAX_NODES)
        return fail(FLUID_E_INVALID, "%s: nodes = %d outside [1, FLUID_LATTICE_MAX_NODES = %d]", call, nodes, FLUID_LATTICE_MAX_NODES);
    TRY(check_etkf(c, call, rho));
    const int M = c->members;
    const size_t B = (size_t)nodes, MM = (size_t)M * M;
    for (size_t b = 0; b < B; ++b) {
        if (counts && counts[b] == 0) continue;                          // an empty node is not read
        for (int k = 0; k < M; ++k) {
            for (int m = k; m < M; ++m)
                if (!std::isfinite(gram[b * MM + (size_t)k * M + m]))
                    return fail(FLUID_E_INVALID, "%s: gram of node %zu, k = %d, m = %d is not finite", call, b, k, m);
            if (!std::isfinite(rhs[b * M + k])) return fail(FLUID_E_INVALID, "%s: rhs of node %zu, k = %d is not finite", call, b, k);
        }
    }
    EtkfBuffers& e = c->etkf;
    const size_t gram_bytes = B * MM * sizeof(double), rhs_bytes = B * M * sizeof(double), word_bytes = B * sizeof(int);
    const size_t inc_bytes = B * MM * sizeof(float);
    TRY(reserve(c, e.in, gram_bytes + rhs_bytes + word_bytes, true, call, "operands"));
    TRY(reserve(c, e.out, inc_bytes + word_bytes, true, call, "results"));
    std::memcpy(e.in.host, gram, gram_bytes);
    std::memcpy(e.in.host + gram_bytes, rhs, rhs_bytes);
    if (counts) std::memcpy(e.in.host + gram_bytes + rhs_bytes, counts, word_bytes);
    HIP_TRY(hipMemcpyAsync(e.in.dev, e.in.host, gram_bytes + rhs_bytes + (counts ? word_bytes : 0), hipMemcpyHostToDevice, c->stream));
    fluid::EtkfOperands in;
    in.gram = e.in.d<double>();
    in.gram_node = MM;
    in.gram_row = (size_t)M;
    in.rhs = e.in.d<double>(gram_bytes);
    in.rhs_node = (size_t)M;
    in.counts = counts ? e.in.d<int>(gram_bytes + rhs_bytes) : nullptr;
    fluid::EtkfResults out;
    out.increments = e.out.d<float>();
    out.status = e.out.d<int>(inc_bytes);
    fluid::launch_etkf_solve(c->stream, M, (double)(M - 1) / (double)rho, in, out, nodes);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(e.out.host, e.out.dev, inc_bytes + word_bytes, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    e.in_flight = false;
    std::memcpy(increments, e.out.host, inc_bytes);
    if (status) std::memcpy(status, e.out.host + inc_bytes, word_bytes);
    return FLUID_OK;
}

// fluid_analyse_lattice / fluid_analyse_lattice_recorded: one body, under the caller's name
static int analyse_lattice_body(fluid_ctx* c, const char* call, const GramSource& src, const float* obs, const float* inv_sigma, int nodes_row,
                                int nodes_col, int row0, int col0, int step, float hw, float rho, const int* fields, int nfields)
{
    if (!obs) return fail(FLUID_E_INVALID, "%s: null array `obs`", call);
    if (!fields) return fail(FLUID_E_INVALID, "%s: null array `fields`", call);
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    TRY(check_transform(c, call, fields, nfields));
    TRY(check_etkf(c, call, rho));
    // the status words: one int per node of the largest lattice, and their twin
    TRY(reserve(c, c->etkf.status, (size_t)FLUID_LATTICE_MAX_NODES * sizeof(int), true, call, "status words"));
    // the two Gram launches: every node's C, rhs and dd in LatticeGram::out, its point count in the start offsets of the lists
    TRY(enqueue_lattice_gram(c, call, src, /*centre=*/1, obs, inv_sigma, nodes_row, nodes_col, row0, col0, step, hw));
    const int M = c->members, MP = fluid::transform_padded(M), mp = fluid::gram_padded(M), nodes = nodes_row * nodes_col;
    const size_t E = fluid::observation_gram_entries(M);
    const size_t table_bytes = (size_t)nodes * M * MP * sizeof(double), bits_bytes = (size_t)nodes * M * sizeof(unsigned long long);
    TRY(ensure_lattice(c, call, table_bytes + bits_bytes + (size_t)nodes * sizeof(unsigned long long)));
    LatticeNodeTables& t = c->lattice;          // written on the device, in stream order: the pinned twin and its event stay out of it
    LatticeGram& g = c->lgram;
    fluid::EtkfOperands in;
    in.gram = g.out.d<double>();
    in.gram_node = E;
    in.gram_row = (size_t)mp;
    in.rhs = g.out.d<double>() + (size_t)mp * mp;
    in.rhs_node = E;
    in.counts = g.lists.d<int>();
    in.starts = true;
    fluid::EtkfResults out;
    out.table = t.tables.d<double>();
    out.bits = t.tables.d<unsigned long long>(table_bytes);
    out.cols = out.bits + (size_t)nodes * M;
    out.status = c->etkf.status.d<int>();
    fluid::launch_etkf_solve(c->stream, M, (double)(M - 1) / (double)rho, in, out, nodes);
    HIP_TRY(hipGetLastError());
    c->etkf.analysed = nodes;
    c->etkf.in_flight = true;
    fluid::LatticeTables dev;
    dev.table = out.table;
    dev.bits = out.bits;
    dev.cols = out.cols;
    const fluid::Lattice lat = {nodes_row, nodes_col, row0, col0, step};
    for (int k = 0; k < nfields; ++k) {
        const int f = fields[k];
        const float scale = c->st != fluid::STORAGE_F32 ? c->field[f].fscale : 1.0f;           // as pack_range sees the field
        TRY(materialize(c, f, /*keep_scale=*/scale != 1.0f));
        // the general path: whether every increment is non-zero is not known here, and the bits do not depend on it
        fluid::launch_transform_members_lattice(c->stream, c->st, c->ptr(f), c->pitch, c->n, c->mb(), 1.0f / scale, scale, dev, /*dense=*/false, lat);
        HIP_TRY(hipGetLastError());
        wrote(c, f, kEverywhere);                                    // nothing owed ...
        c->field[f].fscale = scale;                                  // ... and the scale it had: the launch stored at it
    }
    return FLUID_OK;
}

int fluid_analyse_lattice(fluid_ctx* c, int field, const float* obs, const float* inv_sigma, int nodes_row, int nodes_col, int row0, int col0,
                          int step, float hw, float rho, const int* fields, int nfields)
{
    return analyse_lattice_body(c, "fluid_analyse_lattice", GramSource(field), obs, inv_sigma, nodes_row, nodes_col, row0, col0, step, hw, rho, fields,
                                nfields);
}

int fluid_analyse_lattice_recorded(fluid_ctx* c, const void* record_dev, size_t member_stride, const float* obs, const float* inv_sigma,
                                   int nodes_row, int nodes_col, int row0, int col0, int step, float hw, float rho, const int* fields,
                                   int nfields)
{
    const char* call = "fluid_analyse_lattice_recorded";
    if (!record_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `record_dev`", call);
    return analyse_lattice_body(c, call, {record_dev, member_stride}, obs, inv_sigma, nodes_row, nodes_col, row0, col0, step, hw, rho, fields,
                                nfields);
}

int fluid_analyse_lattice_status(fluid_ctx* c, int* solved, int* empty, int* failed)
{
    const char* call = "fluid_analyse_lattice_status";
    if (!c) return fail(FLUID_E_INVALID, "%s: null context", call);
    EtkfBuffers& e = c->etkf;
    if (e.analysed == 0) return fail(FLUID_E_INVALID, "%s: no fluid_analyse_lattice has run in this context", call);
    HIP_TRY(hipMemcpyAsync(e.status.host, e.status.dev, (size_t)e.analysed * sizeof(int), hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    e.in_flight = false;
    const int* status = e.status.h<int>();
    int n[3] = {0, 0, 0};
    for (int b = 0; b < e.analysed; ++b) n[status[b] == 0 ? 0 : status[b] == 1 ? 1 : 2] += 1;
    if (solved) *solved = n[0];
    if (empty) *empty = n[1];
    if (failed) *failed = n[2];
    return FLUID_OK;
}

// fluid_run / fluid_run_members: one body (see "calls whose physical parameters are one value for everybody or one per
// member").  Defined as the loop of existing calls it replaces: per step the three source blocks unpacked and a step that
// consumes them, or fluid_step's rule; after every `every`-th step each listed field packed into its snapshot slot.
// factor 0: the dense snapshots of fluid_run / fluid_run_members; a coarse factor: every snapshot pack is the block-averaged one
// and `snapshots` / `capacity` count coarse floats (the sources stay full resolution).
// A window (fluid_run_window; null for every other run): the slots in the order they are observed -- by step, slots of one
// step in slot order -- and where the next one is.  Before the first step and behind every step's snapshot packs run_body
// observes the slots due, each one a fluid_observe_members_range.
struct WindowSchedule {
    const fluid_obs_window* w = nullptr;
    size_t stride = 0;                    // w->member_stride, resolved
    std::vector<int> order;
    size_t next = 0;
};

static int observe_due(fluid_ctx* c, WindowSchedule* ws, int steps_done)
{
    const fluid_obs_window* w = ws->w;
    for (; ws->next < ws->order.size() && w->slot_step[ws->order[ws->next]] == steps_done; ++ws->next) {
        const int s = ws->order[ws->next], first = w->slot_first[s];
        TRY(observe_range(c, w->field, first, w->slot_first[s + 1] - first, w->record_dev, ws->stride));
    }
    return FLUID_OK;
}

// what fluid_run_window refuses of its window, and the schedule
static int check_window(const fluid_ctx* c, const char* call, const fluid_run_plan* p, const fluid_obs_window* w, WindowSchedule* ws)
{
    TRY(check_observe(c, call, w->field));
    const int P = c->observe.points;
    if (p->nsteps < 0) return fail(FLUID_E_INVALID, "%s: nsteps < 0", call);
    for (int s = 0; s < w->nslots; ++s) {
        const int lo = w->slot_first[s], hi = w->slot_first[s + 1];
        if (lo < 0 || lo > hi || hi > P)
            return fail(FLUID_E_INVALID, "%s: slot %d holds points [%d, %d): the slots' points must not decrease and lie inside [0, %d points]",
                        call, s, lo, hi, P);
        if (w->slot_step[s] < 0 || w->slot_step[s] > p->nsteps)
            return fail(FLUID_E_INVALID, "%s: slot %d is observed after %d steps, outside [0, nsteps = %d]", call, s, w->slot_step[s], p->nsteps);
    }
    ws->w = w;
    ws->stride = w->member_stride;
    TRY(check_record(c, call, w->record_dev, &ws->stride));
    ws->order.resize((size_t)w->nslots);
    for (int s = 0; s < w->nslots; ++s) ws->order[(size_t)s] = s;
    std::stable_sort(ws->order.begin(), ws->order.end(), [w](int a, int b) { return w->slot_step[a] < w->slot_step[b]; });
    return FLUID_OK;
}

static int run_body(fluid_ctx* c, const char* call, const MemberVal& dt, const MemberVal& diff, const MemberVal& visc, const fluid_run_plan* p,
                    int factor, int* snapshots_written, WindowSchedule* window = nullptr)
{
    TRY(refuse_slabs(c, call));
    if (factor) TRY(check_factor(call, c->n, factor));
    if (p->iters < 0 || (p->iters & 1)) return fail(FLUID_E_INVALID, "%s: sweep count must be even and >= 0 (got %d)", call, p->iters);
    if (p->nsteps < 0) return fail(FLUID_E_INVALID, "%s: nsteps < 0", call);
    if (p->every < 0) return fail(FLUID_E_INVALID, "%s: every < 0", call);
    const size_t cells = member_cells(c), block = (size_t)c->members * cells;
    const size_t snap_cells = member_cells(c, factor), snap_block = (size_t)c->members * snap_cells;
    const int snapshots = p->every ? p->nsteps / p->every : 0;
    if (p->every > 0) {
        if (p->nfields < 1 || p->nfields > FLUID_NFIELDS) return fail(FLUID_E_INVALID, "%s: nfields %d outside [1, %d]", call, p->nfields, FLUID_NFIELDS);
        if (!p->fields) return fail(FLUID_E_INVALID, "%s: null `fields`", call);
        if (!p->snapshots) return fail(FLUID_E_INVALID, "%s: null device pointer `snapshots`", call);
        for (int k = 0; k < p->nfields; ++k)
            if (!c->valid_field(p->fields[k])) return fail(FLUID_E_INVALID, "%s: bad field id %d", call, p->fields[k]);
        const size_t need = (size_t)snapshots * (size_t)p->nfields * snap_block;
        if (p->capacity < need)
            return fail(FLUID_E_INVALID, "%s: capacity %zu floats is below the %zu of %d snapshots x %d fields x %d members", call, p->capacity, need,
                        snapshots, p->nfields, c->members);
        TRY(check_device_span(c, call, "snapshots", p->snapshots, need * sizeof(float)));
    }
    if (p->sources) TRY(check_device_span(c, call, "sources", p->sources, 3 * block * sizeof(float)));
    const float* src = static_cast<const float*>(p->sources);
    float* snap = static_cast<float*>(p->snapshots);
    if (window) TRY(observe_due(c, window, 0));
    for (int z = 0; z < p->nsteps; ++z) {
        if (src) {
            for (int k = 0; k < 3; ++k) TRY(unpack_range(c, FLUID_U_PREV + k, 0, c->members, src + (size_t)k * block, cells));
        } else if (!(p->use_sources && z == 0)) {
            TRY(zero_sources(c));
        }
        TRY(full_step(c, dt, diff, visc, p->iters));
        if (p->every && (z + 1) % p->every == 0)
            for (int k = 0; k < p->nfields; ++k) {
                TRY(pack_range(c, p->fields[k], 0, c->members, snap, snap_cells, factor));
                snap += snap_block;
            }
        if (window) TRY(observe_due(c, window, z + 1));
    }
    HIP_TRY(hipGetLastError());
    if (snapshots_written) *snapshots_written = snapshots;
    return FLUID_OK;
}

int fluid_run(fluid_ctx* c, float dt, float diff, float visc, const fluid_run_plan* plan, int* snapshots_written)
{
    if (!plan) return fail(FLUID_E_INVALID, "fluid_run: null plan");
    if (!c) return fail(FLUID_E_INVALID, "fluid_run: null context");
    return run_body(c, "fluid_run", dt, diff, visc, plan, 0, snapshots_written);
}

int fluid_run_coarse(fluid_ctx* c, float dt, float diff, float visc, const fluid_run_plan* plan, int factor, int* snapshots_written)
{
    TRY(refuse_factor_zero("fluid_run_coarse", factor));
    if (!plan) return fail(FLUID_E_INVALID, "fluid_run_coarse: null plan");
    if (!c) return fail(FLUID_E_INVALID, "fluid_run_coarse: null context");
    return run_body(c, "fluid_run_coarse", dt, diff, visc, plan, factor, snapshots_written);
}

// fluid_run_members (factor 0) / fluid_run_members_coarse
// ... / fluid_run_window (either factor; `window` non-null)
static int run_members_body(fluid_ctx* c, const char* call, const float* dt, const float* diff, const float* visc, const fluid_run_plan* plan,
                            int factor, int* snapshots_written, const fluid_obs_window* window = nullptr)
{
    if (!plan) return fail(FLUID_E_INVALID, "%s: null plan", call);
    TRY(check_member_args(c, call, {{"dt", dt}, {"diff", diff}, {"visc", visc}}));
    WindowSchedule schedule, *ws = window ? &schedule : nullptr;
    if (window) TRY(check_window(c, call, plan, window, ws));
    if (c->members == 1) return run_body(c, call, dt[0], diff[0], visc[0], plan, factor, snapshots_written, ws);
    if (factor) TRY(check_factor(call, c->n, factor));      // before ensure_consts: a refusal changes nothing
    TRY(ensure_consts(c));
    return run_body(c, call, {dt, c->members}, {diff, c->members}, {visc, c->members}, plan, factor, snapshots_written, ws);
}

int fluid_run_members(fluid_ctx* c, const float* dt, const float* diff, const float* visc, const fluid_run_plan* plan, int* snapshots_written)
{
    return run_members_body(c, "fluid_run_members", dt, diff, visc, plan, 0, snapshots_written);
}

int fluid_run_members_coarse(fluid_ctx* c, const float* dt, const float* diff, const float* visc, const fluid_run_plan* plan, int factor,
                             int* snapshots_written)
{
    TRY(refuse_factor_zero("fluid_run_members_coarse", factor));
    return run_members_body(c, "fluid_run_members_coarse", dt, diff, visc, plan, factor, snapshots_written);
}

// fluid_run_window (include/fluid_amd.h "asynchronous observations"): the members' run of either kind with a window
int fluid_run_window(fluid_ctx* c, const float* dt, const float* diff, const float* visc, const fluid_run_plan* plan, int factor,
                     const fluid_obs_window* window, int* snapshots_written)
{
    const char* call = "fluid_run_window";
    if (!window) return fail(FLUID_E_INVALID, "%s: null window", call);
    if (!window->record_dev) return fail(FLUID_E_INVALID, "%s: null device pointer `record_dev`", call);
    if (window->nslots < 0 || window->nslots > FLUID_WINDOW_MAX_SLOTS)
        return fail(FLUID_E_INVALID, "%s: nslots = %d outside [0, FLUID_WINDOW_MAX_SLOTS = %d]", call, window->nslots, FLUID_WINDOW_MAX_SLOTS);
    if (window->nslots > 0 && !window->slot_first) return fail(FLUID_E_INVALID, "%s: null array `slot_first`", call);
    if (window->nslots > 0 && !window->slot_step) return fail(FLUID_E_INVALID, "%s: null array `slot_step`", call);
    return run_members_body(c, call, dt, diff, visc, plan, factor, snapshots_written, window);
}

// ---- timing -------------------------------------------------------------------
int fluid_timing_enable(fluid_ctx* c, int on)
{
    TRY(check_ctx(c));
    TRY(timing_collect(c));
    c->timing = on != 0;
    return FLUID_OK;
}

int fluid_timing_read(fluid_ctx* c, fluid_timing* out, int reset)
{
    TRY(check_ctx(c));
    if (!out) return fail(FLUID_E_INVALID, "null pointer");
    TRY(timing_collect(c));
    out->jacobi_ms = c->cat_ms[FLUID_TIME_DIFFUSION];
    out->sweeps = c->sweeps;
    out->jacobi_launches = c->launches;
    out->jacobi_field_launches = c->field_launches;
    out->pressure_ms = c->pressure_ms;
    out->pressure_sweeps = c->pressure_sweeps;
    out->solves = c->cat_calls[FLUID_TIME_DIFFUSION];
    for (int k = 0; k < FLUID_TIMING_CATEGORIES; ++k) {
        out->category_ms[k] = c->cat_ms[k];
        out->category_calls[k] = c->cat_calls[k];
    }
    if (reset) {
        for (int k = 0; k < FLUID_TIMING_CATEGORIES; ++k) {
            c->cat_ms[k] = 0.0;
            c->cat_calls[k] = 0;
        }
        c->sweeps = 0;
        c->launches = c->field_launches = 0;
        c->pressure_ms = 0.0;
        c->pressure_sweeps = 0;
    }
    return FLUID_OK;
}

// Opt-in, NOT the reference's behaviour (it always runs a fixed count,
// FluidSequential.c:91): Jacobi in blocks of `check_every` sweeps until the
// max-norm residual drops to `tol` or `max_iters` is reached.
int fluid_op_diffuse_tol(fluid_ctx* c, int b, int x, int x0, float alpha, float beta, float tol, int max_iters,
                         int check_every, int* iters_done, float* residual)
{
    TRY(check_ctx(c));
    // (a residual-terminated solve would make every member's sweep count depend on the others)
    TRY(fluid_detail::refuse_ensemble(c, "fluid_op_diffuse_tol"));
    TRY(check_fields(c, {x, x0}));
    TRY(check_b(b));
    if (check_every < 2 || (check_every & 1) || max_iters < 0 || !(tol >= 0.f))
        return fail(FLUID_E_INVALID, "diffuse_tol: check_every must be even and >= 2, max_iters >= 0, tol >= 0");
    int done = 0;
    float res = 0.f;
    TRY(fluid_residual(c, x, x0, alpha, beta, &res));
    while (res > tol && done < max_iters) {
        const int blk = std::min(check_every, (max_iters - done) & ~1);
        if (blk <= 0) break;
        TRY(op_diffuse(c, b, x, x0, {alpha, beta}, blk));
        done += blk;
        TRY(fluid_residual(c, x, x0, alpha, beta, &res));
    }
    if (iters_done) *iters_done = done;
    if (residual) *residual = res;
    return FLUID_OK;
}

// ---- the reference's loop body on host arrays -----------------------------------
// The host arrays are ordinary pageable memory (the reference malloc()s them, FluidSequential.c:277-282) and travel
// at PCIe speed as they are: measured 8.7 ms per step() at 4096^2 against 7.1 ms for the same 384 MiB through pinned
// buffers plus 1.6 ms of compute (tools/step_timing.py).  All copies of a call are enqueued on the context's stream
// and waited for once.
int fluid_release_cached(void)
{
    fluid_ctx* c = g_cached;
    g_cached = nullptr;
    return fluid_destroy(c);
}

static int cached_ctx(int N, fluid_ctx** out)
{
    if (g_cached && g_cached->n != N) TRY(fluid_release_cached());
    if (!g_cached) TRY(fluid_create(N, &g_cached));
    *out = g_cached;
    return FLUID_OK;
}

int step_src(int N, float dt, float diff, float visc, int iters, float* u, float* v, float* dens, float* u_prev,
             float* v_prev, float* dens_prev)
{
    if (!u || !v || !dens || !u_prev || !v_prev || !dens_prev) return fail(FLUID_E_INVALID, "step_src: null field");
    TRY(check_iters(iters));
    fluid_ctx* c;
    TRY(cached_ctx(N, &c));
    float* host[6] = {u, v, dens, u_prev, v_prev, dens_prev};
    for (int k = 0; k < 6; ++k) TRY(copy_rows(c, k, nullptr, host[k], 0, c->w, true, false));
    TRY(fluid_step(c, dt, diff, visc, iters, 1, 1));
    for (int k = 0; k < 6; ++k) TRY(copy_rows(c, k, host[k], nullptr, 0, c->w, false, false));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FLUID_OK;
}

int step(int N, float dt, float diff, float visc, float* u, float* v, float* dens)
{
    if (!u || !v || !dens) return fail(FLUID_E_INVALID, "step: null field");
    fluid_ctx* c;
    TRY(cached_ctx(N, &c));
    float* host[3] = {u, v, dens};
    for (int k = 0; k < 3; ++k) TRY(copy_rows(c, k, nullptr, host[k], 0, c->w, true, false));
    TRY(fluid_step(c, dt, diff, visc, 40, 1, 0));   // 40 sweeps: FluidSequential.c:91
    for (int k = 0; k < 3; ++k) TRY(copy_rows(c, k, host[k], nullptr, 0, c->w, false, false));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return FLUID_OK;
}

}  // extern "C"

namespace {
CachedCtx::~CachedCtx()
{
    fluid_ctx* mine = c;
    c = nullptr;
    if (mine) (void)fluid_destroy(mine);
}
}  // namespace
