// Verifying ensembles (include/fluid_amd.h "verifying ensembles"): what fluid_solver.hip needs of fluid_verify.hip.
#pragma once
#include "fluid_kernels.h"

namespace fluid {

// The score row of the header: kVerifySums leading entries (count, then the four sums), then one bin per rank 0 .. 64.
constexpr int kVerifySums = 5, kVerifyBins = kTransformMaxMembers + 1, kVerifyRow = kVerifySums + kVerifyBins;
// Blocks of the scoring launch: one lane per cell of the box, 256 lanes per block, at most kVerifyBlocks blocks -- two
// rounds of 256 CUs x 4 resident blocks at the 64-member kernel's registers -- whose lanes then stride over the cells.  A
// function of the box alone: it fixes the order of every sum.  0 for an empty box.
constexpr int kVerifyBlocks = 2048;
inline int verify_blocks(CellBox box)
{
    if (box.empty()) return 0;
    const size_t cells = (size_t)(box.row_hi - box.row_lo) * (size_t)(box.col_hi - box.col_lo);
    const size_t blocks = (cells + 255) / 256;
    return (int)(blocks < (size_t)kVerifyBlocks ? blocks : (size_t)kVerifyBlocks);
}
// Scratch of one call, reused field after field in stream order: per block four doubles, laid out [sum][block], then one
// word per bin, [bin][block].
inline size_t verify_partial_bytes(int blocks) { return (size_t)blocks * (4 * sizeof(double) + kVerifyBins * sizeof(unsigned)); }

// One field, all mb.count members (2 .. kTransformMaxMembers), every cell of `box`: rules 1 - 6 of the header.  `truth`, `crps_map`
// (may be null): dense (n + 2)^2 float arrays, row-major with the ghost ring, aligned to 4 bytes; `row`: kVerifyRow doubles,
// aligned to 8 bytes; `partials`: verify_partial_bytes(verify_blocks(box)) bytes of scratch.  `inv`: as for the pack.  Two
// launches -- the scoring kernel, then the fold -- or, for an empty box, the fold alone.  Pad columns are not read.
void launch_verify_members(hipStream_t s, int st, const void* x, int pitch, int n, Members mb, float inv, const float* truth, CellBox box,
                           bool fair, float* crps_map, void* partials, double* row);

}  // namespace fluid
