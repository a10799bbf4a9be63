// fluid_ctx.h -- the context behind include/fluid_amd.h's opaque fluid_ctx, shared by the orchestrator
// (fluid_solver.hip) and the native RCCL exchange (fluid_exchange_rccl.hip).  Private to csrc/.
#pragma once
#include <hip/hip_runtime.h>

#include <string>
#include <utility>
#include <vector>

#include "../../include/fluid_amd.h"
#include "fluid_kernels.h"

namespace fluid_detail {
int fail(int code, const char* fmt, ...);      // records the calling thread's error string, returns `code`
int materialize_zero(fluid_ctx* c, int f);      // a field zero by definition gets its zeros in memory (fluid_solver.hip)
int refuse_ensemble(const fluid_ctx* c, const char* what);   // FLUID_E_INVALID on a context of more than one member
struct RcclExchange;                            // fluid_exchange_rccl.hip
void rccl_release(RcclExchange* x);
}  // namespace fluid_detail

#define HIP_TRY(expr)                                                                                      \
    do {                                                                                                   \
        hipError_t e_ = (expr);                                                                            \
        if (e_ != hipSuccess)                                                                              \
            return fluid_detail::fail(e_ == hipErrorOutOfMemory ? FLUID_E_NOMEM : FLUID_E_HIP, "%s: %s",   \
                                      #expr, hipGetErrorString(e_));                                       \
    } while (0)

#define TRY(expr)                        \
    do {                                 \
        int rc_ = (expr);                \
        if (rc_ != FLUID_OK) return rc_; \
    } while (0)

// A physical parameter of a call, or a value a field's record keeps from one: the same float for every member of the
// context, or one float per member (the fluid_*_members calls; exactly `members` of them, copied from the caller's array).
// at(0) is member 0's value either way -- what a launch passes by value beside a per-member table -- and that is arranged
// by the constructors here and nowhere else.
class MemberVal {
    float s_;
    std::vector<float> v_;      // empty: s_ holds for everybody
    explicit MemberVal(std::vector<float>&& v) : s_(v[0]), v_(std::move(v)) {}

public:
    MemberVal(float v = 0.0f) : s_(v) {}
    MemberVal(const float* per_member, int members) : s_(per_member[0]), v_(per_member, per_member + members) {}
    bool uniform() const { return v_.empty(); }
    float at(int m) const { return v_.empty() ? s_ : v_[(size_t)m]; }
    const std::vector<float>& values() const { return v_; }      // one per member; empty when uniform
    // floats compared by value (NaN differs from itself), and a uniform value differs from a per-member one
    bool operator==(const MemberVal& o) const { return s_ == o.s_ && v_ == o.v_; }
    // f(this member's value, b's) for every member: uniform if both are
    template <class F>
    MemberVal map(const MemberVal& b, F f) const
    {
        if (uniform() && b.uniform()) return MemberVal(f(s_, b.s_));
        std::vector<float> r(uniform() ? b.v_.size() : v_.size());
        for (size_t m = 0; m < r.size(); ++m) r[m] = f(at((int)m), b.at((int)m));
        return MemberVal(std::move(r));
    }
    template <class F>
    MemberVal map(F f) const { return map(MemberVal(), [&](float x, float) { return f(x); }); }
};

// What one field's buffer holds beyond its memory (fluid_solver.hip: "row-slab bookkeeping", "fields that are zero by
// definition").  Two fields trade buffers by trading the whole record; only wrote() and mark_zero() reset one.
// An ensemble keeps ONE record per field id too: every member goes through the same calls, so what is owed or known of a
// field is the same for all of them -- only the two amounts owed (pend_inc, src_dt) may be one per member, after a
// fluid_*_members call -- and `ptr` is member 0's copy (member m: m * field_floats elements behind it).
struct FieldState {
    void* ptr = nullptr;
    int reach = 0;            // rows past each inner slab edge that hold their owner's values (see "row-slab bookkeeping")
    bool zero = false;        // all +0 by definition; the memory is NOT (yet) zeroed
    bool pend = false;        // owes itself `+ pend_inc` in every cell (deferred add_source of a zero source)
    MemberVal pend_inc;
    // add_source of a real source, deferred into the next diffusion's first launch (fluid_solver.hip: op_add_source)
    int src_of = 0;           // 0: nothing owed; else 1 + the id of the source field s: owes itself + src_dt * s
    MemberVal src_dt;
    // fp16 storage: a projection's pressure is of the order h * |velocity| -- 1e-5 at 16384^2, fp16 subnormals -- so in a
    // step the divergence and the pressure are kept multiplied by a power of two (fluid_solver.hip: project): fscale (1:
    // plain values), undone exactly when the field is downloaded and by a pass over it for any reader that does not know
    float fscale = 1.0f;
};

// What the ensemble calls need beyond the fields is library-owned and outside the arena, and every piece of it is one of
// these: `bytes` of device memory and, where a call asked for one, a pinned host twin of the same size.  ONE function
// allocates and grows them (fluid_solver.hip: reserve), at the first call that needs the room: enough room is left
// alone; otherwise the new pair is allocated first, the context's stream is waited for -- launches enqueued so far may
// still read the old pair -- and only then the old pair is freed.  A grown buffer does not keep its contents.  A failure
// (FLUID_E_NOMEM for an allocation the device or the host refuses) frees what the call had allocated and leaves the
// buffer, and so the context, as it was.  An owner of several buffers reserves them one by one, so a call that failed
// part-way is completed by the next.  The destructor frees both: it runs when fluid_destroy, after its waits, deletes the
// context.
struct Scratch {
    char *dev = nullptr, *host = nullptr;
    size_t bytes = 0;                     // the room of each
    Scratch() = default;
    Scratch(const Scratch&) = delete;
    Scratch& operator=(const Scratch&) = delete;
    ~Scratch() { release(); }
    void release()
    {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        dev = host = nullptr;
        bytes = 0;
    }
    template <class T> T* d(size_t byte_offset = 0) const { return reinterpret_cast<T*>(dev + byte_offset); }
    template <class T> T* h(size_t byte_offset = 0) const { return reinterpret_cast<T*>(host + byte_offset); }
};

// Per-member constants (the fluid_*_members calls) reach the kernels through tables in device memory: a ring with a
// pinned twin.  A table is copied host twin -> device on the context's stream, so it is in place before the launches that
// read it and is not overwritten before the launches queued ahead of the next copy have run; the host twin's bytes are
// reused only after the event behind their copy has completed.  A table whose bytes equal one still in the ring is not
// copied again (fluid_solver.hip: member_consts): a stepping loop with the same arrays every call uploads nothing and
// waits for nothing.
struct ConstRing {
    Scratch ring;
    size_t head = 0;
    struct Blob { size_t off, len; unsigned long long hash; hipEvent_t copied; };
    std::vector<Blob> live;                 // tables in the ring, oldest first
    std::vector<hipEvent_t> free_events;
};

// What the ensemble diagnostics (fluid_*_members maxima, fluid_member_moments, fluid_ensemble_stats, fluid_member_gram) need
// beyond the fields.  The twin of `moments` also takes the members' result words on their way to the host.
struct EnsembleReduce {
    Scratch max;                          // [members] result words (k_residual / k_absmax2 with a result stride of 1)
    Scratch moments;                      // [members] double2 {sum, sum of squares}, and its twin
    Scratch partials;                     // [members][moment_blocks()] per-block double2 pairs
    Scratch mean, var;                    // the two statistics fields, field_floats floats each: zeroed once, so the pads stay zero
    bool have_stats = false;              // a fluid_ensemble_stats has filled them
    // fluid_member_gram, MP = gram_padded(members):
    Scratch gram_partials;                // [gram_blocks()] per-block MP x MP double matrices
    Scratch gram;                         // the folded MP x MP matrix, and its twin
};

// Verifying ensembles (fluid_verify_members): the per-block partial sums and rank counts of the scoring launch, folded by the
// launch behind it.  One buffer, reused field after field and call after call in stream order; sized by the call's box
// (fluid_verify.h: verify_partial_bytes), so a larger box grows it.
struct EnsembleVerify {
    Scratch partials;
};

// The bulk host copies (fluid_download_members / fluid_upload_members) go through a dense float staging buffer on the
// device.  It holds `members` whole members; a call moves its members group by group in stream order.
struct MemberStage {
    Scratch buf;
    int members = 0;
    float* dev() const { return buf.d<float>(); }
};

// The weight tables of fluid_transform_members / fluid_select_members: kSlots slots of one padded table each, with a twin.
// A call fills the next host slot and copies it to its device slot on the context's stream: the copy runs behind every
// launch enqueued so far, so the device bytes need no wait, and the host bytes are reused only after the event behind
// their own copy -- kSlots calls ago -- has completed.  (The ConstRing is sized for the per-member records: 64 KiB at
// small M, where one 64-member table is 32.5 KiB.)
struct TransformTables {
    static constexpr int kSlots = 8;
    Scratch tables;
    int next = 0;
    hipEvent_t copied[kSlots] = {};
    bool in_use[kSlots] = {};
};

// The node tables of fluid_transform_members_lattice: ONE buffer with a twin.  Per call: [nodes][M][MP] doubles, then
// [nodes][M] words of non-zero bits, then [nodes] words of their OR.  The copy runs on the context's stream behind the
// launches of the call before, so the device bytes need no wait; the host bytes are refilled only after the event behind
// their last copy has completed.  (fluid_analyse_lattice writes the device tables itself and leaves twin and event alone.)
struct LatticeNodeTables {
    Scratch tables;
    hipEvent_t copied = nullptr;
    bool in_use = false;                  // `copied` has been recorded since the tables last grew
};

// Observing ensembles (fluid_set_observation_points, fluid_observe_members, fluid_observation_gram): the network and the
// scratch of its Gram call.  The network is ONE allocation of 32 bytes per point, replaced as a whole by the call that sets
// it and freed in fluid_destroy: four floats of weights, the 64-bit tap offset, and one float each for the observed values
// and 1 / sigma a Gram call copies in.  A TYPED network (fluid_set_observation_network with per-point fields) has one more
// byte per point behind them, 33 in all: the id of the field the point observes, the index into the launch's
// fluid::FieldSources.  `fields` is its host copy, `mask` the fields some point observes; an untyped network has neither.
struct Observation {
    char* table = nullptr;                // [points] float4 weights | [points] tap offsets | [points] obs | [points] 1 / sigma | typed: [points] field ids
    int points = 0;
    bool typed = false;
    unsigned mask = 0;                    // bit f: some point observes field f (0: untyped)
    std::vector<unsigned char> fields;    // [points], typed only
    const unsigned char* field_of_point() const { return typed ? reinterpret_cast<const unsigned char*>(table + (size_t)points * 32) : nullptr; }
    Scratch partials;                     // [observation_gram_blocks()] per-block results of the network in place, or of a larger one before it
    Scratch result;                       // the folded result, fluid::observation_gram_entries doubles, and its twin
    const float* weight() const { return reinterpret_cast<const float*>(table); }
    const unsigned long long* tap() const { return reinterpret_cast<const unsigned long long*>(table + (size_t)points * 16); }
    float* obs() const { return reinterpret_cast<float*>(table + (size_t)points * 24); }
    float* sigma() const { return reinterpret_cast<float*>(table + (size_t)points * 28); }
    // Screening observations (fluid_set_observation_qc, fluid_observation_departures).  The gate: `qc` > 0 makes the six Gram
    // and analysis calls screen their points first; the launch writes sigma() and `flags`, one byte per point and its twin,
    // which fluid_observation_qc_result copies back.  `qc` outlives the network, `qc_checked` does not.
    float qc = 0.0f;                      // the resident threshold, 0: off
    bool qc_checked = false;              // a gated call has filled `flags` for the network in place
    Scratch flags;
    // fluid_observation_departures: ONE buffer with a twin, copied back whole -- three sums (32 bytes), then [points] floats
    // of mean, spread and departure, then [points] bytes of rank and flag; and the sums' per-chunk partials, three doubles each
    Scratch screen, chunk_sums;
};

// Lattice observations (fluid_observation_gram_lattice): the point lists of the nodes, the operands of every point and the
// results of every node.  `coords` is the host copy of the network's positions (fluid_set_observation_points keeps it: col,
// row per point) the lists are built from.  The lists are ONE buffer with a twin: [nodes + 1] ints, the start of every
// node's entries, then the entries, {point index, the bits of the float weight}, a node's in increasing point index.  They
// are kept: `valid` says that they are the lists of the network in place and of the lattice arguments and c below, and
// then a call builds and uploads nothing.
struct LatticeGram {
    std::vector<float> coords;            // [points] {col, row}
    Scratch lists;
    Scratch operands;                     // [points][MP + 2] doubles: a_k (padding members 0), then d, then 0
    Scratch out;                          // [nodes] partial-shaped results (fluid::observation_gram_entries doubles) and their twin
    bool valid = false;
    int nodes_row = 0, nodes_col = 0, row0 = 0, col0 = 0, step = 0;
    float c = 0.0f;
    long long pairs = 0;                  // entries of the lists
};

// The ETKF solve (fluid_etkf_increments, fluid_analyse_lattice).  The host route's operands ([nodes] M x M doubles, [nodes]
// M doubles, [nodes] ints) and results ([nodes] M x M floats, [nodes] ints) each are ONE buffer with a twin; every call of
// that route ends in a wait.  The fused route's status words, one per node, have a fixed size: FLUID_LATTICE_MAX_NODES
// ints and their twin.  `in_flight`: an analysis has been enqueued and nothing has waited for the stream since -- its
// launches may still read the point lists and their twin.
struct EtkfBuffers {
    Scratch in, out, status;
    int analysed = 0;                     // nodes of the last fluid_analyse_lattice, 0 before the first
    bool in_flight = false;
};

struct fluid_ctx {
    int n = 0, w = 0, pitch = 0;
    size_t field_floats = 0;
    int members = 1;                      // simulations in this context (fluid_create_ensemble): all of the same n, storage and
                                          // knobs, all going through every call together; the arena is laid out [field][member]
    char* arena = nullptr;
    bool own_arena = false;
    int st = fluid::STORAGE_F32;          // field storage type
    size_t esz = 4;                       // bytes per stored element
    hipStream_t stream = nullptr;
    bool own_stream = false;
    hipStream_t stream2 = nullptr;        // slabs: the density diffusion runs beside the velocity path (full_step)
    hipEvent_t ev_fork = nullptr, ev_join = nullptr;
    bool slab_overlap = true;
    // slabs: every exchange is enqueued on a stream of its own (one stream per communicator: the ranks issue their
    // collectives in one order), ordered against the compute stream(s) by events.  An exchange issued `async` is not waited
    // for at once: the first launch of the solve it feeds runs its interior strips -- rows that depend on this slab's own rows
    // only -- while the halo rows travel, and its edge strips behind the exchange's event (fluid_solver.hip: call_exchange,
    // launch_fused).  FLUID_PARAM_XCHG_OVERLAP.
    hipStream_t xstream = nullptr;
    hipEvent_t ev_xbegin = nullptr, ev_xdone = nullptr;
    bool xchg_overlap = true;
    unsigned xowed = 0;                    // compute streams that owe a wait on ev_xdone: bit 0 main, bit 1 stream2 (xchg_join)
    long long split_launches = 0;          // first launches that ran as interior + edge strips around an exchange
    bool early_advect = true;                      // FLUID_PARAM_EARLY_ADVECT
    float vmax_prev[2] = {-1.0f, -1.0f};           // the last global bounds of the velocity / density advection (-1: none yet)
    FieldState field[FLUID_NFIELDS];
    size_t field_bytes = 0;
    unsigned int* d_scalar = nullptr;     // device word for the reductions
    float* d_partials = nullptr;          // slabs: per-block maxima of the gradient subtraction (launch_subtract_gradient)
    ConstRing consts;                     // tables of per-member constants (fluid_*_members)
    EnsembleReduce red;                   // results and scratch of the ensemble diagnostics
    EnsembleVerify verify;                // per-block partials of fluid_verify_members
    MemberStage stage;                    // device staging of the bulk host copies
    TransformTables xform;                // weight tables of fluid_transform_members / fluid_select_members
    LatticeNodeTables lattice;            // node tables of fluid_transform_members_lattice
    Observation observe;                  // the observation network and the scratch of fluid_observation_gram
    LatticeGram lgram;                    // point lists, operands and results of fluid_observation_gram_lattice
    EtkfBuffers etkf;                     // operands, results and status words of the ETKF solve
    unsigned int* tiles = nullptr;        // 3 x members x tile_rows x tile_pitch words: |x0| minima per tile for division mode 3
    unsigned int* h_scalar = nullptr;     // pinned host mirror
    hipEvent_t scalar_ready = nullptr;    // recorded behind the scalar's device-to-host copy
    int variant = fluid::JACOBI_TB;
    int tb_max_t = 16, tb_rows = 0, num_cu = 256;   // temporal blocking: sweeps/launch cap, rows/strip (0 = auto)
    long long tb_min_cells = 0;                    // smaller slabs use single-sweep launches (never faster since the 2-column lanes)
    long long tb_t16_min_cells = -1;               // >= 0: 16-sweep launches on every slab of at least this many cells (tests, tuning);
                                                   // -1: the measured rule of pick_sweeps()
    bool fuse_divergence = true;                   // a projection's divergence is computed inside its solve's first launch
    bool tb_fill = true;                           // FLUID_PARAM_TB_FILL: the fused kernel skips the fill evaluations nothing reads
    bool autotune = true;                          // strip heights of the fused kernel measured at run time (fluid_solver.hip: RbTuner)
    struct Trial { unsigned long long key; int cand; hipEvent_t a, b; };
    std::vector<Trial> trials;                     // launches being timed for the tuner
    std::vector<hipEvent_t> free_events;
    bool defer_zero_source = true;                 // see settle()
    bool in_halo_exchange = false;
    int tb_nv = 2;                                 // columns per lane of the fused kernel (2: 4 waves/SIMD; 4: 2 waves/SIMD)
    int tb_edge_pct = 40;                          // strip height of the two edge windows, % of the others'
    int fast_div = 2;                              // FLUID_PARAM_TB_FAST_DIVISION: 0 always divide; 2 (default) division modes 5 / 4;
                                                   // 3 modes 2 / 4 (round 2's default); 1 also the two-term mode 3 where |x0|
                                                   // allows it.  Every (mode, beta) is proven on the device first
    // slab decomposition
    int rank = 0, nranks = 1, own0 = 1, own1 = 1, min_slab = 0, halo = 1;
    bool fuse_add_source = true;              // FLUID_PARAM_FUSE_ADD_SOURCE
    float pscale = 1.0f;                      // fp16 storage: the factor of a projection's scaled fields (FieldState::fscale)
    fluid_exchange_fn xchg = nullptr;
    void* xchg_user = nullptr;
    fluid_detail::RcclExchange* rccl = nullptr;   // the library's own exchange, when attached (fluid_exchange_rccl_attach)
    // timing
    bool timing = false;
    struct Ev { hipEvent_t a, b; int cat; bool pressure; };
    std::vector<Ev> ev_pool;
    size_t ev_used = 0;
    double cat_ms[FLUID_TIMING_CATEGORIES] = {};
    long long cat_calls[FLUID_TIMING_CATEGORIES] = {};
    long long sweeps = 0, pending_sweeps = 0, launches = 0, field_launches = 0;
    double pressure_ms = 0.0;                      // the part of cat_ms[DIFFUSION] spent in pressure solves (project())
    long long pressure_sweeps = 0, pending_pressure_sweeps = 0;
    bool in_pressure_solve = false;

    bool valid_field(int id) const { return id >= 0 && id < FLUID_NFIELDS; }
    void* ptr(int id) const { return field[id].ptr; }
    fluid::Members mb() const { return {members, field_floats}; }      // what every launch_* takes
    size_t all_bytes() const { return field_bytes * (size_t)members; }   // one field in all its members (contiguous)
    void* row(int id, int r) const { return static_cast<char*>(ptr(id)) + (size_t)r * pitch * esz; }
    int lo_all() const { return own0 - (rank == 0 ? 1 : 0); }          // owned rows incl. ghost row
    int hi_all() const { return own1 + (rank == nranks - 1 ? 1 : 0); }
};

