// amg_impl.h — the hierarchy behind spmv/amg.h, shared by amg_host.cpp (setup, update), amg_setup.hip (the device-side
// setup), amg_mis2_host.cpp (the MIS-2 aggregation's definition), amg.hip (the V-cycle) and cg.hip (cg_solve_amg).
// Internal: not installed under include/.
#ifndef SPMV_AMD_AMG_IMPL_H
#define SPMV_AMD_AMG_IMPL_H

#include "spmv/amg.h"

#include <hip/hip_runtime.h>

#include <cmath>
#include <vector>

#if defined(__HIPCC__)
#define SPMV_AMG_HD __host__ __device__ __forceinline__
#else
#define SPMV_AMG_HD inline
#endif

namespace spmv {

constexpr int kAmgDenseRows = 1024;      // largest coarsest level that is inverted

struct AMGLevel {
    CSRMatrix view{};             // this level's matrix: device arrays only, owns nothing
    CSRMatrix* A = nullptr;       // levels > 0: the owner of view's arrays (spgemm_csr's output)
    // below the coarsest level
    CSRMatrix* P = nullptr;       // n_l x n_{l+1}, one unit entry per row; its column array is the aggregate map
    CSRMatrix* PT = nullptr;      // its transpose: the member list of each aggregate, rows ascending
    CSRMatrix* AP = nullptr;      // A_l P_l, kept for amg_update's refill
    // a smoothed hierarchy only (amg_setup_smoothed): P above is the smoothed prolongator, PT its transpose with values
    CSRMatrix* T = nullptr;       // the tentative prolongator (what P is on a plain hierarchy): its columns are the map
    CSRMatrix* AT = nullptr;      // A_l T_l, kept for the refill
    float* d_s = nullptr;         // [n] s_i = float(-double(omega_p) / double(d_i)), then [nnz(AT)] S = diag(s) AT
    float* d_res = nullptr;       // [n] the residual the weighted restriction reads
    int p_lanes = 1, pt_lanes = 1;     // pick_lanes_per_row of P's and of PT's mean row length
    int num_aggregates = 0;
    int lanes = 1;                // pick_lanes_per_row of the mean row length
    float* d_wd = nullptr;        // [n] omega / d_i
    float* d_work = nullptr;      // level 0: xa, xb; below: f, sol, xa, xb (n floats each)
    std::vector<int> row_ptrs, cols;   // host copy of the structure (diagonals, the dense coarse matrix); a
                                       // device-built hierarchy holds it for the coarsest level only
    int rounds = 0;               // amg_setup_device: rounds the root selection of this level took
};

struct AMGHierarchy {
    AMGConfig config;
    int num_rows = 0;
    int nnz = 0;
    std::vector<AMGLevel> levels;
    int coarse_solver = 0;
    float* d_cinv = nullptr;      // coarse_solver 0: [n_c * n_c] row-major
    bool device_built = false;    // amg_setup_device made it: amg_update keeps the levels off the host
    bool smoothed = false;        // amg_setup_smoothed / amg_setup_smoothed_device made it
    AMGSmoothing smoothing;
};

namespace detail {

// ---- host pieces both setups and the two aggregations' definitions share ----
inline bool amg_structure_ok(int n, long long nnz, const int* rp, const int* ci) {
    if (rp[0] != 0 || rp[n] != nnz) return false;
    for (int i = 0; i < n; ++i) {
        if (rp[i + 1] < rp[i] || rp[i + 1] > nnz) return false;
    }
    for (long long p = 0; p < nnz; ++p) {
        if (ci[p] < 0 || ci[p] >= n) return false;
    }
    return true;
}

// fp32 sum of the stored (i,i) entries in storage order; found[i] = 0 where the row stores none
inline void amg_diagonal(int n, const int* rp, const int* ci, const float* va, std::vector<float>* d,
                         std::vector<char>* found) {
    d->assign(static_cast<size_t>(n), 0.0f);
    if (found) found->assign(static_cast<size_t>(n), 0);
    for (int i = 0; i < n; ++i) {
        float sum = 0.0f;
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            if (ci[p] == i) {
                sum = sum + va[p];
                if (found) (*found)[i] = 1;
            }
        }
        (*d)[i] = sum;
    }
}

// amg.h's strength test on one stored entry (i,j) of value v
SPMV_AMG_HD bool amg_strong(int i, int j, float v, double theta2, float di, float dj) {
    if (j == i || v == 0.0f) return false;
    return static_cast<double>(v) * static_cast<double>(v) >=
           theta2 * __builtin_fabs(static_cast<double>(di) * static_cast<double>(dj));
}

// amg_host.cpp, for amg_setup_device / amg_update on its hierarchies (amg_setup.hip):
bool amg_config_ok(const AMGConfig& cfg);                       // the ranges of amg.h
int amg_level_workspace(AMGHierarchy& H, AMGResult& res, int l);          // lanes and d_work of level l
// the coarsest level downloaded when it is inverted, its solver, the complexities; the error code left in res
int amg_finish(AMGHierarchy& H, AMGResult& res, hipStream_t s);
// amg_setup.hip: amg_update on a hierarchy amg_setup_device built (the argument checks have passed)
AMGResult amg_update_device(AMGHierarchy* H, const CSRMatrix* A);
bool amg_smoothing_ok(const AMGSmoothing& sm);                  // the ranges of amg.h
// amg_setup.hip: the smoothed-aggregation step of level l, for both builders.  lv.T holds the tentative prolongator on
// the device, lv.P / PT / AP / AT and level l + 1's A exist (empty at setup, filled by it for a refill), d_diag is the
// level's diagonal on the device (n floats, checked).  In this order: AT = A_l T, s, S = diag(s) AT, P = T + S,
// PT = P^T, AP = A_l P, A_{l+1} = PT AP.  refill: the values alone through the *_numeric forms, except PT, which is
// transposed again (csr_transpose_gpu has no values-only form: PT's arrays are released and allocated anew).
// Returns 0 or the SpMVError code of the call that failed.
int amg_smooth_coarsen(AMGHierarchy& H, int l, const float* d_diag, bool refill, hipStream_t s);

// The V-cycle's launches on `s`, none synchronises.  d_done (may be null) points at a device int: every kernel returns
// at once when it is not 0 (the `done` of a solver's state).  forced_lanes: 0, or the lane count every level takes.
hipError_t amg_vcycle(const AMGHierarchy& H, const float* d_r, float* d_z, const int* d_done, int forced_lanes,
                      hipStream_t s);
// SPMV_DEBUG's amg_lanes=N when it is 1, 2, 4, ... 64, else 0
int amg_forced_lanes();

} // namespace detail
} // namespace spmv

#endif
