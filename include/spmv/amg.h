// spmv/amg.h — plain (unsmoothed) aggregation algebraic multigrid for a symmetric positive definite CSR matrix: a
// hierarchy built once per matrix (amg_setup), refilled when only the values change (amg_update), and one symmetric
// V-cycle on the device per application (amg_apply).  cg_solve_amg (spmv/cg.h) uses it as the preconditioner of the
// device-resident CG loop.  Kernels in gpu-spmv_amd/csrc/amg.hip, setup in amg_host.cpp, DESIGN.md §4.16.
//
// Hierarchy.  Level 0 is A.  Below the coarsest level, level l has an aggregate map agg_l (row i of level l belongs
// to aggregate agg_l[i]); P_l is the n_l x n_{l+1} matrix with the single entry P_l[i, agg_l[i]] = 1, and
//     A_{l+1} = P_l^T (A_l P_l)
// is formed on the device by csr_transpose_gpu and two spgemm_csr calls, so every level matrix is bit for bit
// spgemm_cpu_csr(P^T, spgemm_cpu_csr(A_l, P_l)) (spmv/spgemm.h): columns ascending, cancelled entries kept.  The
// restriction is kept as the member list of each aggregate (the structure of P_l^T, rows ascending); it has no values.
//
// Diagonal.  d_i of a level is the fp32 sum of the row's stored (i,i) entries in storage order (the rule of cg_solve).
// Strength.  A stored entry (i,j), j != i, of value v != 0 is strong when, in fp64,
//     double(v) * double(v) >= (double(theta) * double(theta)) * |double(d_i) * double(d_j)|.
// Aggregation (amg_aggregate_cpu_csr is its definition; it runs on the host on a copy of the level, as the level
// schedule of sptrsv_csr does).  Three passes over the rows in ascending order:
//   1. a row that is unaggregated and whose strong neighbours are all unaggregated opens an aggregate of itself and
//      those neighbours (a row without strong neighbours becomes a singleton);
//   2. a row still unaggregated that has a strong neighbour aggregated by pass 1 joins that neighbour's aggregate
//      (membership as of the end of pass 1; the entry with the largest |v| wins, the first in storage order on a tie);
//   3. every remaining row opens an aggregate of itself and its still unaggregated strong neighbours.
// Aggregates are numbered in order of creation.
// Stopping.  Level l is the coarsest when n_l <= coarse_rows, or l + 1 == max_levels, or aggregation left the size
// unchanged (n_{l+1} == n_l: nothing is strong any more).
// Coarsest level.  With n <= 1024 the host factors the level by Cholesky in fp64, inverts it, symmetrises the inverse
// and stores it as a dense fp32 array on the device (coarse_solver 0); the solve is z_i = sum_j Cinv[i,j] f_j with
// the exact fp32 x fp32 products accumulated in fp64 (64 lanes per row, lane t takes j = t, t + 64, ...; the lanes
// are folded by a fixed butterfly) and rounded once.  A larger coarsest level (coarse_solver 1) takes coarse_sweeps
// damped Jacobi sweeps from zero with the smoother's kernels.
//
// V-cycle (amg_apply), per level l below the coarsest with right-hand side f (f = r on level 0),
// wd_i = float(double(omega) / double(d_i)):
//   1. x_i = wd_i * f_i                                      the first pre-sweep from a zero guess
//   2. x'_i = fmaf(wd_i, f_i - (A x)_i, x_i)                 each further pre-sweep (ping-pong buffers)
//   3. f_{l+1}[a] = sum over the members i of a, ascending, of (f_i - (A x)_i), added in fp32 starting from +0
//   4. e = the cycle on level l + 1
//   5. x_i = x_i + e[agg_i]
//   6. post_sweeps sweeps as in 2.
// (A x)_i is the vector-CSR row sum of the library: the row's entries spread over a group of 1 .. 64 lanes, four per
// lane and step, each lane an fmaf chain, the lanes folded by a fixed butterfly.  The lane count of a level is
// pick_lanes_per_row of its mean row length; at a fixed lane count two applications give the same bits.  No float
// atomics, no workgroup waits for another.
#ifndef SPMV_AMG_H
#define SPMV_AMG_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct AMGConfig {
    int   max_levels;     // >= 1
    int   coarse_rows;    // stop coarsening at a level with <= this many rows; 1 .. 1024
    float strength;       // theta >= 0
    int   pre_sweeps;     // >= 1
    int   post_sweeps;    // >= 0 (pre == post makes the cycle symmetric: required by cg_solve_amg)
    float jacobi_weight;  // omega in (0, 2)
    int   coarse_sweeps;  // >= 1: only used when the coarsest level is too large for the dense solve
    AMGConfig() : max_levels(10), coarse_rows(64), strength(0.08f), pre_sweeps(1), post_sweeps(1),
                  jacobi_weight(2.0f / 3.0f), coarse_sweeps(4) {}
};

// Caller-given aggregates: host arrays, map[l][i] = aggregate of row i of level l, for l = 0 .. levels - 1.
struct AMGAggregates {
    int levels;
    const int* const* map;
};

struct AMGResult {
    int    error_code;           // SpMVError as int
    int    levels;
    int    coarse_solver;        // 0 dense inverse, 1 Jacobi sweeps
    int    bad_row;              // the row a diagonal or pivot check failed at, or -1
    int    bad_level;            // its level, or -1
    double grid_complexity;      // sum of n_l / n_0
    double operator_complexity;  // sum of nnz_l / nnz_0
    float  setup_ms;             // host wall time of the call
    AMGResult() : error_code(0), levels(0), coarse_solver(0), bad_row(-1), bad_level(-1), grid_complexity(0.0),
                  operator_complexity(0.0), setup_ms(0.0f) {}
};

// Opaque; owns all its device memory, the V-cycle's workspace included: ONE HIERARCHY SERVES ONE STREAM AT A TIME
// (two concurrent amg_apply / cg_solve_amg calls on one hierarchy would share its level vectors).  Level 0 is a view
// over A's own device arrays, which must stay alive and unchanged while the hierarchy is used.
struct AMGHierarchy;

// Builds the hierarchy of the square device-resident matrix A (csr_to_gpu / csr_wrap_device).  A's rows may be
// unsorted and may repeat a column.  config == nullptr: AMGConfig().  With aggregates != nullptr the maps are taken as
// given: level l + 1 has max(map[l]) + 1 rows, and the only stopping rule left is the level count (at most
// min(aggregates->levels, max_levels - 1) maps are used).  Runs on the library stream (spmv_set_stream) and returns
// after completion.
// Checks, in this order, before any device work; on every failure *out is null and nothing stays allocated:
//   null out / A -> INVALID_ARGUMENT; num_rows != num_cols or num_rows < 1 -> INVALID_DIMENSION; missing device arrays
//   -> INVALID_FORMAT; a config field outside the range above -> INVALID_ARGUMENT; aggregates with levels < 0, a null
//   map, an entry outside [0, n_l), or an aggregate without members (a number below the maximum that no row carries)
//   -> INVALID_ARGUMENT.
// Then, on the downloaded arrays: row pointers that do not start at 0, decrease or do not end at nnz, or a column
// outside [0, n) -> INVALID_FORMAT; a diagonal of any level that is missing, not > 0 or not finite -> INVALID_ARGUMENT
// with bad_level / bad_row; a Cholesky pivot of the coarsest level that is not > 0 -> INVALID_ARGUMENT with bad_level
// / bad_row; allocation failure -> CUDA_MALLOC; the codes of csr_transpose_gpu / spgemm_csr pass through.
AMGResult amg_setup(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config = nullptr,
                    const AMGAggregates* aggregates = nullptr);

// New values in the same pattern: keeps the aggregates, refills every level with spgemm_csr_numeric, recomputes the
// diagonals and the coarse inverse; allocates nothing setup had allocated.  A may be another handle (level 0 becomes a
// view over ITS arrays).  Checks, before anything changes: null H / A -> INVALID_ARGUMENT; dimensions or nnz other
// than at setup -> INVALID_DIMENSION; missing device arrays -> INVALID_FORMAT.  After those the hierarchy is being
// rewritten: a pattern that differs surfaces as spgemm_csr_numeric's INVALID_FORMAT (or the structure check's), a bad
// diagonal or pivot as in amg_setup, and the hierarchy then holds unspecified values until an amg_update succeeds.
AMGResult amg_update(AMGHierarchy* H, const CSRMatrix* A);
void      amg_destroy(AMGHierarchy* H);            // null is fine
int       amg_num_levels(const AMGHierarchy* H);   // 0 for null

// Level `level` as a non-owning device view (as csr_wrap_device gives: host pointers null, nothing owned); level 0's
// view is over A's own arrays.  *d_aggregate: the level's map on the device (n_l ints), null on the coarsest level;
// *num_aggregates: n_{l+1}, 0 on the coarsest level.  view / d_aggregate / num_aggregates may each be null.
// null H -> INVALID_ARGUMENT; level outside [0, levels) -> INVALID_DIMENSION.
int       amg_level(const AMGHierarchy* H, int level, CSRMatrix* view, const int** d_aggregate, int* num_aggregates);

// z = one V-cycle on r from a zero guess (n_0 floats each, device).  Runs on the library stream and returns after
// completion.  null H / d_r / d_z, or overlapping d_r and d_z -> INVALID_ARGUMENT, before any device work.
int       amg_apply(const AMGHierarchy* H, const float* d_r, float* d_z);

// The aggregation of one level on HOST arrays: aggregate[num_rows], *num_aggregates.  Checks, in this order: null
// argument -> INVALID_ARGUMENT; not square -> INVALID_DIMENSION; missing host arrays, malformed row pointers or a
// column out of range -> INVALID_FORMAT; strength < 0 or NaN -> INVALID_ARGUMENT.  Nothing is written on failure.
// Diagonals are taken as they come (a missing one counts as 0).
int       amg_aggregate_cpu_csr(const CSRMatrix* A_host, float strength, int* aggregate, int* num_aggregates);

} // namespace spmv

#endif
