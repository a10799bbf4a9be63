// The ETKF solve of the one-call analysis (include/fluid_amd.h "one-call analysis"): what fluid_solver.hip needs of
// fluid_etkf.hip.
#pragma once
#include "fluid_kernels.h"

namespace fluid {

// The ETKF solve of every node (include/fluid_amd.h "one-call analysis").  Operands in device memory: node b's matrix at
// gram + b * gram_node, entry [k][m] at k * gram_row + m, only k <= m read; its right-hand side at rhs + b * rhs_node.
// `counts`: null (every node is solved), one count per node, or -- `starts` -- the [nodes + 1] start offsets of
// LatticeLists, whose differences are the counts; a node whose count is 0 is neither read nor solved.
struct EtkfOperands {
    const double* gram = nullptr;
    size_t gram_node = 0, gram_row = 0;
    const double* rhs = nullptr;
    size_t rhs_node = 0;
    const int* counts = nullptr;
    bool starts = false;
};
// Where a node's result goes: `increments` ([node][k][m] floats; fluid_etkf_increments) or, `increments` null, the tables
// of LatticeTables written in place as fluid_transform_members_lattice's host loop writes them (transform_padded(M) doubles
// per row, padding columns 0, the non-zero word per row, their OR per node); `status`, one int per node, may be null.
struct EtkfResults {
    float* increments = nullptr;
    double* table = nullptr;
    unsigned long long* bits = nullptr;
    unsigned long long* cols = nullptr;
    int* status = nullptr;
};
// the cap on the Jacobi sweeps of one node: include/fluid_amd.h, FLUID_ETKF_MAX_SWEEPS
constexpr int kEtkfMaxSweeps = 28;
// members in [2, kTransformMaxMembers]; shift = (double)(members - 1) / (double)rho, what the diagonal gets.  One launch
// whatever the node count: one block per node, the matrix and its eigenvectors in LDS.
void launch_etkf_solve(hipStream_t s, int members, double shift, const EtkfOperands& in, const EtkfResults& out, int nodes);

}  // namespace fluid
