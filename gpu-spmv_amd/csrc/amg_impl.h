// amg_impl.h — the hierarchy behind spmv/amg.h, shared by amg_host.cpp (setup, update), amg.hip (the V-cycle) and
// cg.hip (cg_solve_amg).  Internal: not installed under include/.
#ifndef SPMV_AMD_AMG_IMPL_H
#define SPMV_AMD_AMG_IMPL_H

#include "spmv/amg.h"

#include <hip/hip_runtime.h>

#include <vector>

namespace spmv {

constexpr int kAmgDenseRows = 1024;      // largest coarsest level that is inverted

struct AMGLevel {
    CSRMatrix view{};             // this level's matrix: device arrays only, owns nothing
    CSRMatrix* A = nullptr;       // levels > 0: the owner of view's arrays (spgemm_csr's output)
    // below the coarsest level
    CSRMatrix* P = nullptr;       // n_l x n_{l+1}, one unit entry per row; its column array is the aggregate map
    CSRMatrix* PT = nullptr;      // its transpose: the member list of each aggregate, rows ascending
    CSRMatrix* AP = nullptr;      // A_l P_l, kept for amg_update's refill
    int num_aggregates = 0;
    int lanes = 1;                // pick_lanes_per_row of the mean row length
    float* d_wd = nullptr;        // [n] omega / d_i
    float* d_work = nullptr;      // level 0: xa, xb; below: f, sol, xa, xb (n floats each)
    std::vector<int> row_ptrs, cols;   // host copy of the structure (diagonals, the dense coarse matrix)
};

struct AMGHierarchy {
    AMGConfig config;
    int num_rows = 0;
    int nnz = 0;
    std::vector<AMGLevel> levels;
    int coarse_solver = 0;
    float* d_cinv = nullptr;      // coarse_solver 0: [n_c * n_c] row-major
};

namespace detail {

// The V-cycle's launches on `s`, none synchronises.  d_done (may be null) points at a device int: every kernel returns
// at once when it is not 0 (the `done` of a solver's state).  forced_lanes: 0, or the lane count every level takes.
hipError_t amg_vcycle(const AMGHierarchy& H, const float* d_r, float* d_z, const int* d_done, int forced_lanes,
                      hipStream_t s);
// SPMV_DEBUG's amg_lanes=N when it is 1, 2, 4, ... 64, else 0
int amg_forced_lanes();

} // namespace detail
} // namespace spmv

#endif
