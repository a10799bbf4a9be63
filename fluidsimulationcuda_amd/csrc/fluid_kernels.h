// fluid_kernels.h -- launch interface of the gfx950 kernels (fluid_kernels.hip).
#pragma once
#include <hip/hip_runtime.h>

namespace fluid {

// column c of a device row lives at element index c + XOFF (column 1 => a 256-B (fp32) / 128-B (fp16) line start)
constexpr int XOFF = 63;

enum JacobiVariant { JACOBI_STREAM = 0, JACOBI_LDS = 1, JACOBI_NAIVE = 2, JACOBI_TB = 3, JACOBI_VARIANTS = 4 };

// field storage: fp32 (the reference's type; bit parity) or fp16 (fp32 arithmetic, rounded on store)
enum Storage { STORAGE_F32 = 0, STORAGE_F16 = 1 };
typedef _Float16 half_t;
inline size_t storage_bytes(int st) { return st == STORAGE_F16 ? 2 : 4; }

// pitch (elements) for interior size n: room for XOFF, ceil(n/4) 4-vectors and the
// right ghost, rounded to a multiple of 64 elements.
inline int pitch_for(int n) { return ((XOFF + 1 + 4 * ((n + 3) / 4) + 1) + 63) / 64 * 64; }

// An ensemble: `count` members of every field, member m lying m * `stride` elements behind member 0 (fluid_ctx: fields are laid
// out [field][member]).  Every launch below takes one and does to each member what it does to a single field: the member
// index rides in the grid -- blockIdx.z of the kernels whose y is a row, blockIdx.y of the one-dimensional ones, blockIdx.z /
// (solves per launch) of the fused Jacobi kernel -- so the number of launches does not depend on it.  {1, 0}: one simulation.
struct Members {
    int count = 1;
    size_t stride = 0;
};

// Per-member constants of one solve of a fused launch (the fluid_*_members calls): what TbBatch carries once per solve, here
// once per (solve, member) in a table in device memory, record [solve * members + member].  Each wave reads its record in
// the kernel's prologue with wave-uniform loads; the host writes the table (a copy), nothing on the device does.
struct TbMemberK {
    double yd;
    float alpha, beta, hi, lo;   // as TbBatch's
    float x0_inc, div_scale;     // div_scale: the source-adding launch's dt (other forms: the launch's own value)
    unsigned tile_thr, pad;
};

// up to three independent solves of the same shape, blockIdx.z % count of the fused Jacobi kernel (blockIdx.z / count: the
// ensemble member, whose fields lie member * mstride elements behind the addresses given here)
struct TbBatch {
    const void* x[3];
    const void* x0[3];
    void* out[3];
    float alpha[3], beta[3];     // beta: divisor; its exact reciprocal in division mode 4; RN32(1/beta) in mode 5
    double yd[3];                // RN64(1/beta) for division mode 2 (and the fall-backs of modes 3 and 5)
    float hi[3], lo[3];          // division mode 3: hi = RD32(1/beta), lo = RN32(1/beta - hi); mode 5: beta * 2^24, -(RN32(1/beta) * 2^-24)
    const unsigned* tiles[3];    // division mode 3: |x0| minima per tile (k_tile_min_abs), tile_pitch words per tile row
    unsigned tile_thr[3];        //   ... and the bit pattern of beta * 2^-72 they must reach
    int tile_pitch;
    void* div[3];                // divergence-sourced launch (TB_DIVSRC): x / x0 hold u / v, the divergence is
    float div_scale;             //   written here; div_scale = -0.5f * h.  Source-adding launch (TB_ADDSRC): x is the source
                                 //   field s, x0 + div_scale * s (div_scale = dt) is the right-hand side and is written here
    int b[3];
    int x_zero[3];               // first guess known to be all +0: never read
    float x0_inc[3];             // added to every x0 value as it is loaded (-0.0f: nothing pending)
    int count;
    int members;                 // ensemble members per solve (>= 1): gridDim.z = count * members
    size_t mstride;              // elements between two members of a field
    size_t tile_mstride;         // words between two members' tile minima (division mode 3)
    const TbMemberK* mk;         // nullptr: alpha .. x0_inc, tile_thr and div_scale above hold for every member; else this table does
};

void launch_set_bnd(hipStream_t s, int st, void* f, int pitch, int n, int b, Members mb = {});
void launch_add_source(hipStream_t s, int st, void* x, const void* src, int pitch, int row_lo, int row_hi, float dt, Members mb = {},
                       const float* mdt = nullptr);
// mdt / mab / mdt0 (here and below): nullptr, or a device array with one value per member that replaces the scalar argument
// (dt or the increment; float2 {alpha, beta}; dt0) -- read once per wave, indexed by the member's grid coordinate
void launch_jacobi(hipStream_t s, int st, int variant, const void* x, const void* x0, void* out, int pitch, int n,
                   int row_lo, int row_hi, float alpha, float beta, int b, Members mb = {}, const float2* mab = nullptr);
// Shapes of the fused Jacobi kernel (k_jacobi_tb): sweeps T, division mode, columns per lane, and the form -- plain, the
// first launch of a pressure solve that forms the divergence as its right-hand side (DIVSRC), or the first launch of a
// diffusion that adds a deferred source to it (ADDSRC).  This table is the set of kernels built per storage type and the
// set launch_jacobi_tb accepts; 4-column lanes stop at 8 sweeps (more would need > 256 registers).
enum TbForm { TB_PLAIN = 0, TB_DIVSRC = 1, TB_ADDSRC = 2 };
struct TbShape { int T, divmode, nv, form; };
inline constexpr TbShape kTbShapes[] = {
    {2, 0, 2, TB_PLAIN},   {2, 2, 2, TB_PLAIN},   {2, 3, 2, TB_PLAIN},   {2, 4, 2, TB_PLAIN},   {2, 5, 2, TB_PLAIN},
    {2, 0, 4, TB_PLAIN},   {2, 2, 4, TB_PLAIN},   {2, 3, 4, TB_PLAIN},   {2, 4, 4, TB_PLAIN},   {2, 5, 4, TB_PLAIN},
    {4, 0, 2, TB_PLAIN},   {4, 2, 2, TB_PLAIN},   {4, 3, 2, TB_PLAIN},   {4, 4, 2, TB_PLAIN},   {4, 5, 2, TB_PLAIN},
    {4, 0, 4, TB_PLAIN},   {4, 2, 4, TB_PLAIN},   {4, 3, 4, TB_PLAIN},   {4, 4, 4, TB_PLAIN},   {4, 5, 4, TB_PLAIN},
    {8, 0, 2, TB_PLAIN},   {8, 2, 2, TB_PLAIN},   {8, 3, 2, TB_PLAIN},   {8, 4, 2, TB_PLAIN},   {8, 5, 2, TB_PLAIN},
    {8, 0, 4, TB_PLAIN},   {8, 2, 4, TB_PLAIN},   {8, 3, 4, TB_PLAIN},   {8, 4, 4, TB_PLAIN},   {8, 5, 4, TB_PLAIN},
    {12, 0, 2, TB_PLAIN},  {12, 2, 2, TB_PLAIN},  {12, 3, 2, TB_PLAIN},  {12, 4, 2, TB_PLAIN},  {12, 5, 2, TB_PLAIN},
    {16, 0, 2, TB_PLAIN},  {16, 2, 2, TB_PLAIN},  {16, 3, 2, TB_PLAIN},  {16, 4, 2, TB_PLAIN},  {16, 5, 2, TB_PLAIN},
    {8, 4, 2, TB_DIVSRC},  {12, 4, 2, TB_DIVSRC}, {16, 4, 2, TB_DIVSRC}, {8, 0, 2, TB_ADDSRC},  {8, 2, 2, TB_ADDSRC},  {8, 5, 2, TB_ADDSRC},
    {12, 0, 2, TB_ADDSRC}, {12, 2, 2, TB_ADDSRC}, {12, 5, 2, TB_ADDSRC}, {16, 0, 2, TB_ADDSRC}, {16, 2, 2, TB_ADDSRC}, {16, 5, 2, TB_ADDSRC},
};
constexpr int kTbShapeCount = sizeof(kTbShapes) / sizeof(kTbShapes[0]);
// index of a shape in kTbShapes, -1 if it does not exist; a negative T or divmode matches any
constexpr int jacobi_tb_index(int T, int divmode, int nv, int form)
{
    for (int i = 0; i < kTbShapeCount; ++i) {
        const TbShape& s = kTbShapes[i];
        if ((T < 0 || s.T == T) && (divmode < 0 || s.divmode == divmode) && s.nv == nv && s.form == form) return i;
    }
    return -1;
}
constexpr bool jacobi_tb_exists(int T, int divmode, int nv, int form) { return jacobi_tb_index(T, divmode, nv, form) >= 0; }
constexpr bool tb_shapes_unique(int i = 0)
{
    return i == kTbShapeCount || (jacobi_tb_index(kTbShapes[i].T, kTbShapes[i].divmode, kTbShapes[i].nv, kTbShapes[i].form) == i && tb_shapes_unique(i + 1));
}
static_assert(kTbShapeCount == 52 && tb_shapes_unique(), "52 distinct shapes: adding or removing one is a change of this table");
// sweeps per launch the fused kernel is built for, deepest first (FLUID_PARAM_TB_MAX_SWEEPS takes one of them)
inline constexpr int kTbDepths[] = {16, 12, 8, 4, 2};
constexpr bool is_tb_depth(int T) { for (int d : kTbDepths) if (d == T) return true; return false; }
// false (nothing launched): the shape is not in kTbShapes
bool launch_jacobi_tb(hipStream_t s, int st, int T, int divmode, int nv, int form, const TbBatch& batch, int pitch, int n, int row_lo,
                      int row_hi, int rb, int rb_edge, int hole_lo = 0, int hole_hi = 0, bool fill = true);
// tiles of kTileRows x kTileCols interior cells, tile (r, c) = rows 1 + r*kTileRows.., columns 1 + c*kTileCols..
constexpr int kTileRows = 32, kTileCols = 64;
inline int tile_rows(int n) { return (n + kTileRows - 1) / kTileRows; }
inline int tile_pitch(int n) { return (n + kTileCols - 1) / kTileCols; }
// blockIdx.z = solve + count * member: a member's minima lie member * tile_mstride words behind tiles[solve]
struct TileBatch {
    const void* field[3];
    unsigned* tiles[3];
    int count;
    size_t mstride, tile_mstride;
};
void launch_tile_min_abs(hipStream_t s, int st, const TileBatch& tb, int count, int pitch, int n, int row_lo, int row_hi, int tile_pitch,
                         Members mb = {}, size_t tile_mstride = 0);
void launch_validate_div(hipStream_t s, int divmode, float beta, float kbeta, double yd, float hi, float lo, unsigned long long* bad);
void launch_advect(hipStream_t s, int st, void* d, const void* d0, const void* u, const void* v, int pitch, int n,
                   int row_lo, int row_hi, float dt0, int b, Members mb = {}, const float* mdt0 = nullptr);
void launch_advect2(hipStream_t s, int st, void* da, const void* d0a, int ba, void* db, const void* d0b, int bb, const void* u,
                    const void* v, int pitch, int n, int row_lo, int row_hi, float dt0, Members mb = {}, const float* mdt0 = nullptr);
// pscale: power of two the divergence is stored multiplied by (1: plain)
void launch_divergence(hipStream_t s, int st, const void* u, const void* v, void* p, void* div, int pitch, int n,
                       int row_lo, int row_hi, float h, int write_p, float pscale = 1.0f, Members mb = {});
void launch_scale(hipStream_t s, int st, void* x, int pitch, int row_lo, int row_hi, float factor, Members mb = {});
// max_out != nullptr: also leaves max(|u|, |v|) of the stored interior values in *max_out (the bit pattern of a
// non-negative float; what launch_absmax2 would produce for the same rows), via `partials` (kMaxPartials floats of scratch);
// that form serves row slabs, which are never ensembles: one member only
constexpr int kMaxPartials = 8192;
void launch_subtract_gradient(hipStream_t s, int st, void* u, void* v, const void* p, int pitch, int n, int row_lo,
                              int row_hi, float h, float* partials = nullptr, unsigned int* max_out = nullptr, float pinv = 1.0f,
                              Members mb = {});
void launch_gradient_advect(hipStream_t s, int st, void* u, void* v, const void* p, void* d, const void* d0, int pitch, int n,
                            int row_lo, int row_hi, float h, float dt0, int b, float pinv = 1.0f, Members mb = {},
                            const float* mdt0 = nullptr);
// absmax2, residual: every block ends in an atomicMax on its member's result word, result[member * rstride] -- rstride 0:
// the maximum over all members in the one word; 1: one word per member.  The caller zeroes the word(s) first.
void launch_absmax2(hipStream_t s, int st, const void* u, const void* v, int pitch, int n, int row_lo, int row_hi,
                    unsigned int* result, Members mb = {}, int rstride = 0);
void launch_residual(hipStream_t s, int st, const void* x, const void* x0, int pitch, int n, int row_lo, int row_hi,
                     float alpha, float beta, unsigned int* result, Members mb = {}, int rstride = 0, const float2* mab = nullptr);
// Per member, the sum of x and of x * x over the interior cells, in double: out[member] = {sum, sum of squares}.  Two
// launches whatever the member count: moment_blocks(n, members) blocks per member each leave their pair in `partials`
// (members * moment_blocks(n, members) pairs of scratch), a second kernel adds each member's in a fixed order.
constexpr int kMomentBlocks = 4096;      // blocks of the whole launch: a few rounds of 256 CUs x 8 resident blocks
int moment_blocks(int n, int members);
void launch_member_moments(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, double2* partials, double2* out);
// Per cell over the members (every row and column, ghosts included): mean and population variance as float fields in
// the layout of a field; their pad columns are not written.  One launch; the members are walked inside the kernel.
void launch_ensemble_stats(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float* mean, float* var);
// Relaxation to prior spread (include/fluid_amd.h "relaxation to prior spread"), mb.count >= 2, any count.  `out`, `prior`: a
// dense (n + 2)^2 float array, row-major with the ghost ring, aligned to 4 bytes.  `inv`, `scale`: as for
// launch_transform_members_local.  spread: out = (float)sqrt(q / (mb.count - 1)), q the second chain of launch_ensemble_stats
// over widen(x) * inv.  relax: every cell with q != 0 and f = 1 + alpha * (prior - sa) / sa != 1 becomes narrow((float)(mean_d +
// f * d_m)) times scale in every member, in place; the other cells keep their bits.  One launch each; pads are not touched.
void launch_member_spread(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, float* out);
void launch_relax_spread(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, float scale, const float* prior,
                         float alpha);
// All mb.count members of a field (x: the first of them) <-> a dense float array, member m of it m * dstride floats behind
// `dense`, each the (n + 2)^2 row-major array with its ghost ring.  One launch each; pad columns are not touched.
// pack: dense = widen(x) * inv (fp16 storage; fp32 copies the words); unpack: x = narrow(dense), to nearest even.
void launch_pack_members(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, float* dense, size_t dstride);
void launch_unpack_members(hipStream_t s, int st, void* x, int pitch, int n, Members mb, const float* dense, size_t dstride);
// The block-averaged pack: every factor x factor block of a member's (n + 2)^2 array as one float (the order of the sum:
// include/fluid_amd.h "coarse snapshots"), member m of the result m * cstride floats behind `coarse`, ((n + 2) / factor)^2
// floats each.  factor: 2, 4 .. 64, a divisor of n + 2.  One launch, one read of the field.
void launch_pack_members_coarse(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, int factor, float* coarse,
                                size_t cstride);
// Recombining the members of a field in place (include/fluid_amd.h "recombining ensembles"): new member m of every cell =
// the sum over the old members k, in member order, of widen(x_k) * inv * table[k * MP + m] in double, rounded once to float
// and narrowed.  mb.count in [1, kTransformMaxMembers]; MP = transform_padded(mb.count); `table`: device memory, [mb.count][MP]
// doubles, padding columns 0.  dense: no weight of the mb.count x mb.count matrix is zero and `bits` is not read; otherwise
// bit m of bits[k] (device memory) says that table[k * MP + m] takes part -- a zero weight of either sign does not -- and
// bit m of `empty` that column m has no term and is stored as +0.  One launch; pad columns are not touched.
constexpr int kTransformMaxMembers = 64;
inline int transform_padded(int members)
{
    int mp = 1;
    while (mp < members) mp <<= 1;
    return mp;
}
void launch_transform_members(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, const double* table,
                              const unsigned long long* bits, unsigned long long empty, bool dense);
// The Gram matrix of the members of a field over the interior cells (include/fluid_amd.h "ensemble diagnostics",
// fluid_member_gram): out[k * MP + m], k <= m < mb.count, MP = gram_padded(mb.count) = the sum of a_k * a_m in double, a_k =
// widen(x_k) * inv, less the per-cell mean over the members with `centre`; entries below the diagonal are not written.
// mb.count in [1, kTransformMaxMembers].  Two launches whatever the member count: gram_blocks(n, members) blocks each leave
// their MP x MP matrix in `partials` (gram_blocks * MP * MP doubles of scratch), a second kernel adds them in a fixed order.
inline int gram_padded(int members) { return members > 8 ? transform_padded(members) : 8; }
int gram_blocks(int n, int members);
void launch_member_gram(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, bool centre, double* partials,
                        double* out);

// Observing ensembles (include/fluid_amd.h "observing ensembles").  The network is a table in device memory, one record per
// point: `tap`, the element offset of x[i0][j0] within a member (i0 * pitch + XOFF + j0), and four floats of `weight`
// (16-byte aligned), {s0, s1, t0, t1} of the header's definition -- computed on the host, where the points are validated.
// A TYPED network (include/fluid_amd.h "typed networks") has one more byte per point: `field`, the id of the field the point
// observes, null for an untyped one.
struct ObservationPoints {
    const unsigned long long* tap = nullptr;
    const float* weight = nullptr;
    int count = 0;
    const unsigned char* field = nullptr;
};
// What the points of a typed network read, per field id: `base`, the address of member 0 of the field, and `inv`, its own
// 1 / scale (as for the pack).  Built by the host per launch, after every field is settled; passed to the kernel by value
// and copied into LDS at block start, where a lane looks its point's entry up once per chunk of points.  Entries of fields
// no point observes are never read.
constexpr int kObservedFields = 12;
struct FieldSource {                      // (no initialisers: it lives in LDS)
    unsigned long long base;
    float inv, unused;                    // (16 bytes: one LDS read per lookup)
};
struct FieldSources {
    FieldSource of[kObservedFields];
};
// The two Gram launches take a third source, `recorded` non-null (include/fluid_amd.h "asynchronous observations"): h_k[p] =
// h[k * stride + p], floats an earlier launch on the stream left; st, x, inv, typed and the taps of `pts` are then not read
// (pts.count still is).  One instantiation serves every storage type.
struct RecordedValues {
    const float* h = nullptr;
    size_t stride = 0;
};
// The three observing launches below take (`x`, `inv`) -- every point observes that field -- or, `typed` non-null, the table
// pts.field indexes (`x` and `inv` are then not read).  These are different kernels: the one-field instantiations have no
// per-point lookup.
// out[m * ostride + p - first_point] = the observation of member m (m < mb.count) at point p, first_point <= p < first_point +
// npoints: one launch whatever the counts, the member in the grid.  `inv`: as for the pack.  Typed: member m is member
// first_member + m of every field of the table (one field: the caller offsets `x`).
void launch_observe_members(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed, int first_member,
                            const ObservationPoints& pts, int first_point, int npoints, float* out, size_t ostride);
// fluid_observation_gram: out[observation_gram_entries(mb.count)] = the padded MP x MP matrix as launch_member_gram leaves it
// (MP = gram_padded(mb.count), entries below the diagonal not written), then rhs[MP], then dd -- the last two only with `obs`.
// `obs`, `sigma`: pts.count floats of device memory each, or null (no innovation; 1 / sigma = 1).  mb.count in [1,
// kTransformMaxMembers].  Two launches: observation_gram_blocks(points, members) blocks each leave one partial of
// observation_gram_entries doubles in `partials`, a second kernel adds them in a fixed order.
inline size_t observation_gram_entries(int members)
{
    const size_t mp = (size_t)gram_padded(members);
    return mp * mp + mp + 1;
}
int observation_gram_blocks(int points, int members);
void launch_observation_gram(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed,
                             const ObservationPoints& pts, bool centre, const float* obs, const float* sigma, double* partials, double* out,
                             const RecordedValues* recorded = nullptr);

// Screening observations (include/fluid_amd.h "screening observations"): per point of the network the ensemble mean and
// spread of h, the departure of `obs` from the mean, its rank among the members and the decision of the background check
// at `threshold` (0: nothing is rejected), rules 2 - 5 of the header.  `obs`, `sigma`: as for launch_observation_gram; `obs`
// null leaves only mean and spread defined.  Every pointer of ScreenOutputs is device memory and may be null: pts.count
// entries each; `sigma`, the 1 / sigma the Gram launches behind this one read -- +0 at a rejected point, the input's float
// (1 for a null input) elsewhere; it may be the input buffer; `sums`, three doubles over the points not rejected (count, sum
// of d * d, sum of var / sigma^2) through `chunk_sums`, three doubles per chunk of 64 points, in a fixed order.  mb.count in
// [2, kTransformMaxMembers].  One launch, and a second small one for `sums`.
struct ScreenOutputs {
    float* sigma = nullptr;
    float *mean = nullptr, *spread = nullptr, *departure = nullptr;
    unsigned char *rank = nullptr, *flag = nullptr;
    double *chunk_sums = nullptr, *sums = nullptr;
};
inline size_t observation_screen_chunks(int points) { return ((size_t)points + 63) / 64; }
void launch_observation_screen(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed,
                               const ObservationPoints& pts, const float* obs, const float* sigma, float threshold, const ScreenOutputs& out,
                               const RecordedValues* recorded = nullptr);

// Localised updates (include/fluid_amd.h "localised updates").
// The box of a launch, half-open, in cells of the (n + 2)^2 array: rows [row_lo, row_hi), columns [col_lo, col_hi).
struct CellBox {
    int row_lo, row_hi, col_lo, col_hi;
    bool empty() const { return row_lo >= row_hi || col_lo >= col_hi; }
};
// The tapered increment in place: per cell of `box` with taper g != 0 and per member m with bit m of `used` set, x_m =
// narrow((float)(widen(x_m) + g * s_m)), s_m the member-order sum of launch_transform_members over `table` (the increments)
// -- product and sum rounded one after the other, in double.  `inv`, `scale`: 1 / FieldState::fscale and fscale of an fp16
// field held scaled (powers of two; both 1 otherwise): values are read as widen(x) * inv, narrow(y) is stored times scale.
// `table`, `bits`, `dense`: as for launch_transform_members; `taper`: (n + 2)^2 floats of device memory, row-major, or null
// for g = 1.  One launch, its grid the box; cells outside it are neither read nor written.  The box is not empty.
void launch_transform_members_local(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, float scale,
                                    const double* table, const unsigned long long* bits, unsigned long long used, bool dense,
                                    const float* taper, CellBox box);
// Lattice updates (include/fluid_amd.h "lattice updates").  The node tables in device memory: `table`, per node the
// [mb.count][MP] doubles of launch_transform_members (the node's increments, padding columns 0), nodes in row-major order;
// `bits`, per node and old member the word of non-zero columns; `cols`, per node the OR of its words: the columns with a term.
struct LatticeTables {
    const double* table = nullptr;
    const unsigned long long* bits = nullptr;
    const unsigned long long* cols = nullptr;
};
// node (a, b) on cell row row0 + a * step, column col0 + b * step
struct Lattice {
    int nodes_row, nodes_col, row0, col0, step;
};
// Every cell of the (n + 2)^2 array, per member m with a term in a corner node of weight phi != 0: x_m = narrow((float)
// (widen(x_m) + s)), s the sum over those corners, in row-major node order, of phi * (the node's member-order sum of
// launch_transform_members) -- each product and sum rounded on its own, in double; the header has the rules.  `inv`,
// `scale`: as for launch_transform_members_local.  dense: no increment of any node is zero.  One launch.
void launch_transform_members_lattice(hipStream_t s, int st, void* x, int pitch, int n, Members mb, float inv, float scale,
                                      const LatticeTables& t, bool dense, const Lattice& lat);
// The Gaspari-Cohn taper of half-width c about (col, row), one definition for the kernel and for the host's bounding box:
// taper_radius is r at a cell dx columns and dy rows from the centre, taper_value the piecewise polynomial in Horner form,
// clamped to [0, 1]; every operation rounds once (no contraction), in double.
__host__ __device__ inline double taper_radius(double dx, double dy, double c)
{
#pragma clang fp contract(off)
    const double xx = dx * dx, yy = dy * dy;
    return sqrt(xx + yy) / c;
}
__host__ __device__ inline double taper_value(double r)
{
#pragma clang fp contract(off)
    if (!(r < 2.0)) return 0.0;
    double g;
    if (r <= 1.0) {
        g = -0.25 * r + 0.5;
        g = g * r + 0.625;
        g = g * r - 5.0 / 3.0;
        g = g * r;
        g = g * r + 1.0;
    } else {
        g = (1.0 / 12.0) * r - 0.5;
        g = g * r + 0.625;
        g = g * r + 5.0 / 3.0;
        g = g * r - 5.0;
        g = g * r + 4.0;
        g = g - (2.0 / 3.0) / r;
    }
    return g < 0.0 ? 0.0 : g > 1.0 ? 1.0 : g;
}
// out[i * (n + 2) + j] = (float)taper_value(taper_radius(j - col, i - row, c)) for every cell of the (n + 2)^2 array: one launch
void launch_taper_gaspari_cohn(hipStream_t s, float* out, int n, float col, float row, float c);

// Lattice observations (include/fluid_amd.h "lattice observations").  The point lists of the nodes in device memory, built
// and bounds-checked on the host: start[node] .. start[node + 1] index node's entries in `entry`, each {point index < pts.count,
// the bits of the float weight w = (float)taper_value(..) != 0}, a node's in increasing point index.
struct LatticeLists {
    const int* start = nullptr;           // [nodes + 1]
    const int2* entry = nullptr;
    int nodes = 0;
};
// fluid_observation_gram_lattice: out[node * observation_gram_entries(mb.count) + ..] = the node's matrix, rhs and dd in the
// layout launch_observation_gram leaves one result in, the sums of (w * a_k) * a_m, (w * a_k) * d, (w * d) * d over the
// node's entries; a node without entries is not written.  Within a diagonal tile the entries with k > m are not the
// header's (the weight rides on the row operand): the caller mirrors k <= m.  `operands`: pts.count * (gram_padded(mb.count)
// + 2) doubles of scratch.  Two launches whatever the counts: every point is observed once, then one block per node.
void launch_observation_gram_lattice(hipStream_t s, int st, const void* x, int pitch, Members mb, float inv, const FieldSources* typed,
                                     const ObservationPoints& pts, bool centre, const float* obs, const float* sigma, double* operands, const LatticeLists& lists,
                                     double* out, const RecordedValues* recorded = nullptr);

}  // namespace fluid
