// spmv/amg.h — plain (unsmoothed) aggregation algebraic multigrid for a symmetric positive definite CSR matrix: a
// hierarchy built once per matrix (amg_setup), refilled when only the values change (amg_update), and one symmetric
// V-cycle on the device per application (amg_apply).  cg_solve_amg (spmv/cg.h) uses it as the preconditioner of the
// device-resident CG loop.  Kernels in gpu-spmv_amd/csrc/amg.hip, setup in amg_host.cpp, DESIGN.md §4.16.  The
// smoothed-aggregation variant (amg_setup_smoothed, at the end of this header) builds on everything below.
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

// ---- The device-side setup: MIS-2 aggregation (kernels in gpu-spmv_amd/csrc/amg_setup.hip) --------
// The three passes above depend on visiting the rows in ascending order, so amg_setup runs them on the host.
// amg_setup_device builds the same kind of hierarchy without the host: every level's diagonal, aggregation and P are
// made on the device, and only the coarsest level is downloaded (for the Cholesky).  Its aggregation is another rule,
// parallel but with a sequential definition (amg_aggregate_mis2_cpu_csr), as csr_color has in csr_color_cpu:
//   Neighbourhoods.  N(i) = the columns of the strong entries of row i (diagonal and strength as above);
//     N2(i) = (N(i) u the union of N(u) over u in N(i)) \ {i}.  Both are read from A's ROWS only (a pull): on an
//     unsymmetric strong graph u in N2(v) does not imply v in N2(u).
//   Priority.  That of i is the pair (fmix32(i ^ seed), i), larger first: csr_color's (spmv/reorder.h).
//   Roots.  The vertices are visited in descending priority; v is a ROOT iff no u in N2(v) of higher priority is a
//     ROOT (the lexicographically first distance-2 independent set).  A row without strong neighbours is a root.
//   Numbers.  The roots are numbered by ascending row index; root r's aggregate carries r's number.
//   Phase 1.  A non-root with a root in N(i) joins the aggregate of the first such root in storage order (on a
//     symmetric strong graph there is exactly one).
//   Phase 2.  A vertex still free joins the aggregate of the column of the strong entry with the largest |v| among
//     the columns that are roots or phase-1 members (membership as of the end of phase 1), the first in storage
//     order on a tie.
//   Free.  A vertex still free after phase 2 (possible only on an unsymmetric strong graph) gets -1 from the two
//     single-level functions; amg_setup_device returns INVALID_ARGUMENT with bad_level / bad_row = the first such row.
//   Synchronous round count.  The count of a loop in which every vertex reads the others' states as they stood at
//     the start of the round: an undecided v becomes OUT if a higher-priority vertex of N2(v) is a ROOT, else ROOT if
//     every higher-priority vertex of N2(v) is OUT, else it waits; rounds are counted while a vertex is undecided.
//     The device updates the states in place, sees at least what this loop sees, and never takes more rounds.
//
// The definition on HOST arrays: aggregate[num_rows] (-1 = free), *num_aggregates = the number of roots, *rounds (may
// be null) = the synchronous round count.  Checks as amg_aggregate_cpu_csr, in the same order; nothing is written on
// failure.
int       amg_aggregate_mis2_cpu_csr(const CSRMatrix* A_host, float strength, unsigned seed, int* aggregate,
                                     int* num_aggregates, int* rounds);

// The same ints on DEVICE arrays, on every run, stream and lane count: d_aggregate holds num_rows ints on the device;
// *rounds (may be null) = the rounds the root selection took, <= the synchronous count.  Runs on the library stream
// and returns after completion.  Checks, in this order: null A / d_aggregate / num_aggregates -> INVALID_ARGUMENT; not
// square -> INVALID_DIMENSION; num_rows < 0, nnz < 0 or missing device arrays -> INVALID_FORMAT; strength < 0 or NaN
// -> INVALID_ARGUMENT; then, on the device and before anything is written, the structure (csr_transpose_gpu's rule)
// -> INVALID_FORMAT.  SPMV_DEBUG's mis_lanes=N (1, 2, 4, ... 64) forces the lanes that share a row.
int       amg_aggregate_mis2_gpu(const CSRMatrix* A_dev, float strength, unsigned seed, int* d_aggregate,
                                 int* num_aggregates, int* rounds);

// amg_setup without the host: the argument checks (those before the aggregates'), stopping rules, coarsest-level
// solver, workspace and complexities of amg_setup; the aggregation is the MIS-2 rule with `seed`.  Every level is bit
// for bit what amg_setup gives when handed, as caller-given aggregates, the maps amg_aggregate_mis2_cpu_csr produces
// level by level.  The hierarchy is an ordinary one: amg_apply, amg_level, cg_solve_amg and amg_destroy work on it
// unchanged, and amg_update recomputes its diagonals on the device and downloads the coarsest level only.
// After the checks: a malformed structure -> INVALID_FORMAT; a bad diagonal (the smallest such row) or pivot ->
// INVALID_ARGUMENT with bad_level / bad_row; a vertex left free -> INVALID_ARGUMENT with bad_level / bad_row.
AMGResult amg_setup_device(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config = nullptr,
                           unsigned seed = 0);

// The rounds the root selection of level `level` took; 0 for the coarsest level, a hierarchy amg_setup built, a null
// H or a level outside the hierarchy.
int       amg_setup_rounds(const AMGHierarchy* H, int level);

// ---- Smoothed aggregation (setup step in amg_setup.hip, kernels in amg.hip) ------------------------
// One damped-Jacobi step applied to the tentative prolongator.  Per level l below the coarsest, with A_l, its diagonal
// d (the rule above) and the aggregate map:
//     T   = the tentative prolongator (the P of the plain hierarchy)
//     AT  = spgemm(A_l, T)
//     s_i = float(-double(omega_p) / double(d_i))
//     S   = csr_scale(AT, rows = s)
//     P   = csr_add(1, T, 1, S)        AT's pattern (row i of AT always stores column agg_i: it holds a_ii and spgemm
//                                      keeps cancelled entries): fl(1 + fl(s_i at)) at column agg_i, fl(s_i at) elsewhere
//     PT  = csr_transpose(P)           csr_transpose_gpu's stable order
//     AP  = spgemm(A_l, P),   A_{l+1} = spgemm(PT, AP)
// so every level matrix and every P is bit for bit the same chain through spgemm_cpu_csr, csr_scale_cpu and
// csr_add_cpu; amg_prolongator_cpu_csr is that chain for one level's P.
// Strength.  theta_0 = config.strength, theta_{l+1} = fl32(theta_l * strength_decay): the smoothed coarse operators
// are denser and their entries relatively smaller, so a fixed theta stalls the coarsening (Vanek's rule halves it).
// Each theta_l goes to the level's aggregation; it is not used with caller-given maps.
// V-cycle on a smoothed level: the pre-sweeps as above; r_i = f_i - (A x)_i, stored; f_{l+1}[a] = (PT r)_a; the cycle
// on level l + 1; x_i = x_i + (P e)_i; the post-sweeps.  Every (M v)_i is the vector-CSR row sum described above; P
// and PT take their own lane counts from their own mean row lengths (SPMV_DEBUG's amg_lanes=N forces all of them).
// pre + 2 + 1 + post launches per level.  The residual is stored because rows of PT overlap: recomputing it per
// aggregate would cost nnz(P) / n passes over A_l, scattering it would need float atomics.
struct AMGSmoothing {            // 8 bytes
    float prolongator_weight;    // omega_p in (0, 2)
    float strength_decay;        // in (0, 1]
    AMGSmoothing() : prolongator_weight(2.0f / 3.0f), strength_decay(0.5f) {}
};

// amg_setup with smoothed prolongators.  Checks, stopping rules, coarsest-level solver, complexities and workspace are
// amg_setup's (every level below the coarsest holds one more n-vector, the residual); smoothing == nullptr:
// AMGSmoothing(); a weight outside (0, 2), a decay outside (0, 1] or a NaN -> INVALID_ARGUMENT, checked after the
// config and before the aggregates.  The hierarchy is used like any other: amg_apply, cg_solve_amg, amg_level,
// amg_update (which leaves every level and every P bit for bit what a fresh setup on the new values gives; it
// transposes P again, so PT's arrays are released and allocated anew) and amg_destroy.
AMGResult amg_setup_smoothed(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config = nullptr,
                             const AMGSmoothing* smoothing = nullptr, const AMGAggregates* aggregates = nullptr);
// amg_setup_device with smoothed prolongators: the MIS-2 aggregation with `seed` and theta_l per level.
AMGResult amg_setup_smoothed_device(AMGHierarchy** out, const CSRMatrix* A, const AMGConfig* config = nullptr,
                                    const AMGSmoothing* smoothing = nullptr, unsigned seed = 0);
int       amg_is_smoothed(const AMGHierarchy* H);                       // 0 for null

// P and P^T of level `level` as non-owning device views (either may be null).  On a plain hierarchy they are the unit
// P and its transpose.  null H -> INVALID_ARGUMENT; level outside [0, levels - 1) -> INVALID_DIMENSION.  A view of PT
// is stale after amg_update on a smoothed hierarchy.
int       amg_level_transfer(const AMGHierarchy* H, int level, CSRMatrix* P_view, CSRMatrix* PT_view);

// The host definition of one level's smoothed P from HOST arrays: aggregate[num_rows] with values in
// [0, num_aggregates).  Checks, in this order, P untouched by every failure: null P / A_host / aggregate ->
// INVALID_ARGUMENT; not square -> INVALID_DIMENSION; missing host arrays, malformed row pointers or a column out of
// range -> INVALID_FORMAT; weight outside (0, 2) or NaN, num_aggregates < 1, a map entry outside [0, num_aggregates),
// a diagonal that is missing, not > 0 or not finite -> INVALID_ARGUMENT.  On success P owns new host arrays.
int       amg_prolongator_cpu_csr(CSRMatrix* P, const CSRMatrix* A_host, const int* aggregate, int num_aggregates,
                                  float weight);

// The two transfers of level `level` on their own (device vectors), for cycles other than the V-cycle:
//   amg_restrict   d_f_coarse[a] = (PT (f - A_l x))_a     n_l, n_l and n_{l+1} floats
//   amg_prolong    d_x_i = d_x_i + (P e)_i, in place       n_{l+1} and n_l floats
// On a plain hierarchy they run the member-list restriction and the gather of the plain cycle.  They use the
// hierarchy's residual vector: one stream at a time, as amg_apply.  Run on the library stream, return after
// completion.  Null pointers, d_f_coarse overlapping d_f or d_x, d_e overlapping d_x -> INVALID_ARGUMENT; level
// outside [0, levels - 1) -> INVALID_DIMENSION.
int       amg_restrict(const AMGHierarchy* H, int level, const float* d_f, const float* d_x, float* d_f_coarse);
int       amg_prolong(const AMGHierarchy* H, int level, const float* d_e, float* d_x);

} // namespace spmv

#endif
