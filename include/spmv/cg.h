// spmv/cg.h — device-resident preconditioned conjugate gradient solver for A x = b (A symmetric positive definite).
//
// The whole iteration runs on the device (gpu-spmv_amd/csrc/cg.hip): no host round-trip for alpha or beta, no
// device-to-host vector copies inside the loop.  Built on the same pattern as pagerank(): the scalars live in a
// device state, every kernel of a step returns at once when the state says `done`, and the host enqueues step k+1
// before it reads the outcome of step k.  See DESIGN.md §4.9.
#ifndef SPMV_CG_H
#define SPMV_CG_H

#include "bsr_matrix.h"
#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct CGConfig {
    enum Preconditioner { NONE = 0, JACOBI = 1, BLOCK_JACOBI = 2 };   // BLOCK_JACOBI: cg_solve_bsr only
    float tolerance;       // stop when ||r_k||_2 <= tolerance * ||b||_2 (recurrence residual)
    int   max_iterations;
    int   preconditioner;  // Preconditioner
    int   engine;          // -1 auto, 0 direct kernels only, 1 tiled plan from the start where tiled_eligible(A)
    CGConfig() : tolerance(1e-6f), max_iterations(1000), preconditioner(JACOBI), engine(-1) {}
};

struct CGResult {
    int   error_code;         // SpMVError as int
    int   iterations;         // committed iterations
    float relative_residual;  // ||r||/||b|| (recurrence) at exit
    int   converged;
    int   breakdown;          // p.Ap <= 0 or r.z <= 0 was met: A (or M) is not SPD; x holds the last good iterate
    float elapsed_ms;         // device-event time of the iteration loop (setup excluded)
    CGResult() : error_code(0), iterations(0), relative_residual(0.0f), converged(0), breakdown(0),
                 elapsed_ms(0.0f) {}
};

// Solves A x = b by preconditioned CG (M = diag(A) with JACOBI, M = I with NONE):
//     r0 = b - A x0;  z0 = M^-1 r0;  p0 = z0
//     repeat: q = A p;  alpha = (r.z) / (p.q);  x += alpha p;  r -= alpha q;  z = M^-1 r;
//             beta = (r.z)_new / (r.z)_old;  p = z + beta p
// d_b: num_rows floats (device).  d_x: num_rows floats (device): the initial guess on entry, the solution on exit.
// A must be square and resident on the device (csr_to_gpu / csr_wrap_device).  config == nullptr: CGConfig().
//
// Numerics: vectors are fp32.  Every dot product accumulates the per-element products in fp64 into per-workgroup
// partials that are folded in a fixed order; nothing uses float atomics, so a solve is bitwise reproducible from
// run to run on each engine.  alpha and beta are computed in fp64 on the device and applied to the vectors rounded
// to fp32, with fmaf (x = fmaf(alpha, p, x), r = fmaf(-alpha, q, r), p = fmaf(beta, p, z)).  z is never stored: it
// is recomputed as r * dinv, dinv = 1 / diag(A) in fp32 (1 with NONE).  After every iteration the device tests
// sqrt(r.r) <= tolerance * ||b|| (r the recurrence residual); that iteration is the last one.  The diagonal of row i
// is the fp32 sum of its stored (i,i) entries in storage order.
//
// Checks, in this order, before any device work; nothing is written to d_x when one fails:
//   null A / d_b / d_x -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS,
//   converged, 0 iterations; missing device arrays -> INVALID_FORMAT; tolerance < 0 or NaN, max_iterations < 0, an
//   unknown preconditioner or engine -> INVALID_ARGUMENT; overlapping d_b and d_x ranges -> INVALID_ARGUMENT; with
//   JACOBI, a row whose diagonal is missing or not > 0 -> INVALID_ARGUMENT (checked on the device, read back once
//   during setup).
// ||b|| == 0 writes zeros to x and returns converged after 0 iterations.  An initial guess with
// ||r0|| <= tolerance * ||b|| returns converged after 0 iterations and leaves x unchanged.  A breakdown (p.q <= 0,
// or r.z <= 0 for a residual above the tolerance) ends the solve with breakdown = 1 and x at the last good iterate.
//
// Engines: 0 runs a fused vector-CSR SpMV + dot kernel per iteration; 1 runs the LDS-tiled engine (tiled_spmv)
// from the first iteration when the matrix is eligible (> 32768 columns, >= 1 M entries; else as 0), falling back to
// the direct kernel when the tiled engine has no scratch for this stream.  -1 (auto) follows pagerank()'s rule: a
// plan A already holds is used from the start; otherwise an eligible matrix gets its plan after 4 direct iterations,
// if the loop has not converged by then.  A plan cg_solve builds is cached on A, exactly as pagerank() caches its
// plan (the plan build counts inside elapsed_ms).  cg_solve never touches A's promotion count or its merge-path
// state.  It runs on spmv_get_stream() and returns after the solve completed; its setup (workspace, diagonal,
// plan for engine 1) and its one setup read-back synchronise that stream — make the call outside a graph capture.
CGResult cg_solve(const CSRMatrix* A, const float* d_b, float* d_x, const CGConfig* config = nullptr);

// cg_solve for k right-hand sides on one matrix, the matrix read once per step for all of them.
// d_B and d_X are num_rows x k, row-major, on the device, with leading dimensions ldb, ldx >= k (spmv_csr_multi's
// layout); d_X holds the k initial guesses on entry and the k solutions on exit.  results: k CGResult on the host,
// one per column.  Returns a SpMVError as int.  1 <= k <= 32.
//
// Column j runs exactly cg_solve's iteration and numerics above (NONE or JACOBI; dinv is computed once and shared),
// and the contract is bitwise: X[:, j] and results[j].iterations / converged / breakdown / relative_residual /
// error_code equal what cg_solve(A, B[:, j], X0[:, j], config) with engine = 0 gives, whatever the other columns do
// (the row sums, the per-workgroup fp64 partials and their fold depend on the thread-to-row mapping and the grids
// alone, and the k-wide kernels keep both).  max_iterations applies per column.  elapsed_ms is the time of the
// batched loop, the same in every result.
//
// Columns finish independently: one that has converged, broken down or started converged is frozen (its x is not
// written again, its result stands) while the others go on; a column with ||b_j|| == 0 gets x_j = 0, converged, 0
// iterations.  The loop ends when every column is done or max_iterations steps are enqueued.  Columns k..ldx-1 of
// d_X are never written and d_B is never written.
//
// Checks, in this order, before any device work; when one fails nothing is written to d_X, and of `results` only
// error_code (of all k entries; of none when k itself is out of range: the return value carries the code):
//   null A / d_B / d_X / results -> INVALID_ARGUMENT; k < 1 or k > 32 -> INVALID_ARGUMENT; ldb < k or ldx < k ->
//   INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS, every column converged
//   after 0 iterations; missing device arrays -> INVALID_FORMAT; cg_solve's config checks, with engine -1 or 0 only
//   (both run the direct kernels; engine = 1 -> INVALID_ARGUMENT: the LDS-tiled engine has no k-wide form); the
//   ranges d_B[0, (num_rows - 1) * ldb + k) and d_X[0, (num_rows - 1) * ldx + k) overlap -> INVALID_ARGUMENT; with
//   JACOBI, a bad diagonal -> INVALID_ARGUMENT (on the device, in the one setup read-back, d_X untouched).
// Runs on spmv_get_stream() and returns after the solve; call it outside a graph capture.  It never touches A's
// promotion count, merge-path state or tiled plan.  The workspace is three arrays of num_rows x k floats, k rounded up
// to 4 (k <= 4) or to a multiple of 8.
int cg_solve_multi(const CSRMatrix* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                   const CGConfig* config, CGResult* results);

// cg_solve preconditioned by M = L L^T: L is the lower triangle of the square device matrix F with its stored
// diagonal, L^T is F's upper triangle with its stored diagonal (entries are taken as stored: nothing tests that the
// two triangles are each other's transpose).  F has num_rows == A->num_rows; the usual one wraps the output of
// ic0_csr (spmv/ic0.h) over A's own structure arrays.
//     r0 = b - A x0;  z0 = L^-T (L^-1 r0);  p0 = z0
//     repeat: q = A p;  alpha = (r.z) / (p.q);  x += alpha p;  r -= alpha q;  stop test on ||r||;
//             z = L^-T (L^-1 r);  beta = (r.z)_new / (r.z)_old;  p = z + beta p
// Numerics as above, except that z is a stored vector: per step two sptrsv_csr launch sequences with ordered = 0
// (LOWER NON_UNIT from r into z, then UPPER NON_UNIT in place) fill it, r.z is a dot product of its own, and
// p = fmaf(beta, p, z) reads it.  The SpMV half of a step, the engines, the plan caching and the stop rules are
// cg_solve's; a solve is bitwise reproducible from run to run on each engine.
//
// Checks, before any write to d_x: cg_solve's, in their order (config->preconditioner is not read), then: null F ->
// INVALID_ARGUMENT; F not square or of another size than A -> INVALID_DIMENSION; F's device arrays missing ->
// INVALID_FORMAT; setup builds (or finds) both of F's sptrsv_csr schedules: malformed structure -> INVALID_FORMAT; a
// row of F whose diagonal is missing, not > 0 or not finite -> INVALID_ARGUMENT (checked on the device, read back
// once during setup).  cg_solve itself keeps rejecting preconditioner values other than NONE and JACOBI.
// The first call with a factor builds its schedules and synchronises the stream for them; the workspace is four
// vectors (r, p, q, z).
CGResult cg_solve_ic(const CSRMatrix* A, const CSRMatrix* F, const float* d_b, float* d_x,
                     const CGConfig* config = nullptr);

// cg_solve_ic for k right-hand sides: cg_solve_multi's layout (d_B, d_X num_rows x k row-major, ldb, ldx >= k,
// 1 <= k <= 32, results: k CGResult) with cg_solve_ic's preconditioner M = L L^T from the factor matrix F (DESIGN.md
// §4.19).  The contract is bitwise: X[:, j] and results[j].iterations / converged / breakdown / relative_residual /
// error_code equal what cg_solve_ic(A, F, B[:, j], X0[:, j], config) with engine = 0 gives, whatever the other
// columns do.  Per step the matrix is read once (cg_solve_multi's SpMV half) and the two triangular solves are ONE
// k-wide launch sequence each (sptrsv_csr_multi's kernel on the solver's windowed workspace): the launches of a step
// are cg_solve_ic's, whatever k.  Columns freeze as in cg_solve_multi; the triangular solves do not read `done` and
// recompute z for every column, a frozen column's z is never read.
//
// Checks: cg_solve_multi's, in their order (config->preconditioner is not read; engine = 1 -> INVALID_ARGUMENT), then
// cg_solve_ic's for F: null F -> INVALID_ARGUMENT; F not square or of another size than A -> INVALID_DIMENSION; F's
// device arrays missing -> INVALID_FORMAT; malformed structure -> INVALID_FORMAT; a row of F whose diagonal is
// missing, not > 0 or not finite -> INVALID_ARGUMENT (on the device, in the one setup read-back, d_X untouched).  On
// failure, of `results` only error_code is written.  The workspace is four windowed arrays (r, p, q, z).
int cg_solve_multi_ic(const CSRMatrix* A, const CSRMatrix* F, const float* d_B, int ldb, float* d_X, int ldx, int k,
                      const CGConfig* config, CGResult* results);

// cg_solve preconditioned by one V-cycle of the aggregation AMG hierarchy H (spmv/amg.h: amg_setup on A):
// cg_solve_ic's iteration with z = amg_apply(r) in place of the two triangular solves.  z is a stored vector; the
// stored-z step kernels, the SpMV half of a step, the engines, the plan caching, the stop rules and the breakdown rule
// are cg_solve_ic's, and the V-cycle's kernels return at once when the state says `done`, like every loop kernel.  A
// solve is bitwise reproducible from run to run on each engine.  The hierarchy's workspace is used: one solve per
// hierarchy at a time.
//
// Checks, before any write to d_x: cg_solve's, in their order (config->preconditioner is not read), then: null H ->
// INVALID_ARGUMENT; H built for another number of rows than A's -> INVALID_DIMENSION; H->config.pre_sweeps !=
// post_sweeps (the cycle is not symmetric, so M is not) -> INVALID_ARGUMENT.  A cycle that is not positive definite
// (jacobi_weight too large for the matrix) surfaces as a breakdown, x at the last good iterate.
struct AMGHierarchy;
CGResult cg_solve_amg(const CSRMatrix* A, const AMGHierarchy* H, const float* d_b, float* d_x,
                      const CGConfig* config = nullptr);

// cg_solve preconditioned by a factorised sparse approximate inverse M^-1 = GT G (spmv/fsai.h): cg_solve_ic's
// iteration with z = GT (G r), two SpMVs, in place of the two triangular solves.  The preconditioner comes in as
// matrices: G is usually fsai_csr's output and GT csr_transpose_gpu(GT, G); entries are taken as stored, nothing tests
// that GT is G's transpose.  config->preconditioner is not read.  z is a stored vector and t = G r a fifth workspace
// vector; the stored-z step kernels, the SpMV half of a step, the engines for A, the plan caching, the stop rules and
// the breakdown rule are cg_solve_ic's.  The two SpMVs are direct vector-CSR launches with the lanes per row of each
// matrix's own mean row length: they never go through the dispatcher, so no promotion count, merge-path state or tiled
// plan of G or GT is touched.  Per step on the direct engine six launches (SpMV + dot, update, G, GT, r.z, direction),
// whatever the matrix.  A solve is bitwise reproducible from run to run on each engine.
//
// Checks, before any write to d_x: cg_solve's, in their order, then: null G or GT -> INVALID_ARGUMENT; either not
// square or of another size than A -> INVALID_DIMENSION; device arrays of either missing -> INVALID_FORMAT.  An M that
// is not positive definite surfaces as a breakdown, x at the last good iterate, as with cg_solve_amg.
CGResult cg_solve_fsai(const CSRMatrix* A, const CSRMatrix* G, const CSRMatrix* GT, const float* d_b, float* d_x,
                       const CGConfig* config = nullptr);

// cg_solve on a block CSR matrix (spmv/bsr.h): the same iteration, numerics, stop rules, breakdown
// rule, ||b|| == 0 rule and checks, in cg_solve's order, with "nothing written to d_x when one fails".  The
// preconditioner is NONE, JACOBI or BLOCK_JACOBI:
//   JACOBI        dinv = 1 / the (k,k) entry of the stored diagonal block of row I*b + k; a missing diagonal block or an
//                 entry that is not > 0 -> INVALID_ARGUMENT (on the device, in the one setup read-back)
//   BLOCK_JACOBI  M = the block diagonal of A: z = D^-1 r by bsr_diag_apply's ordered sum with the inverses of
//                 bsr_diag_inverse_gpu (spmv/bsr.h), built in one setup launch; a missing diagonal block or a pivot that
//                 is not > 0 or not finite -> INVALID_ARGUMENT, in the same read-back
// engine must be -1 or 0: there is no tiled BSR engine, engine = 1 -> INVALID_ARGUMENT (cg_solve_multi's rule).
// cg_solve, cg_solve_multi and every other entry point keep rejecting BLOCK_JACOBI.
//
// q = A p is the lane-group product of spmv_bsr (VECTOR_CSR), its lane count (SPMV_DEBUG=bsr_lanes=N forces one) and
// its bits, fused with the partials of p.q.  z is a stored vector; per step THREE launches whatever b and whatever the
// preconditioner: product + p.q; the update of x and r with z = M^-1 r and the partials of r.z and r.r in one kernel
// (one thread per scalar row, the block's new r exchanged through LDS); the direction step.  Setup takes up to seven:
// the inverses or the diagonal, r0 with r.r and b.b, z0, r.z, the copy p0 = z0, the state.  A solve is bitwise
// reproducible from run to run at a fixed lane count.  The workspace is r, p, q, z and n floats (JACOBI) or
// num_block_rows * b * b floats (BLOCK_JACOBI).  A is only read: no cache on it is built, used or dropped.  Runs on
// spmv_get_stream() and returns after the solve; call it outside a graph capture.
CGResult cg_solve_bsr(const BSRMatrix* A, const float* d_b, float* d_x, const CGConfig* config = nullptr);

// cg_solve_ic's iteration on cg_solve_bsr's kernels: M = L L^T given as the block factor matrix F of
// spmv/bsr_factor.h, usually bsr_ic0's output wrapped over A's structure arrays:
//     bsr_wrap_device(n, n, b, num_blocks, A->d_block_row_ptrs, A->d_block_cols, d_f_values).
// One step: the product fused with p.q (cg_solve_bsr's, so q has spmv_bsr's bits); the update of x and r with the r.r
// partials; z = L^-T (L^-1 r) by a LOWER solve from r into z and an UPPER solve in place (sptrsv_bsr, ordered = 0); r.z;
// the direction step: 4 + launches(LOWER) + launches(UPPER) launches.  Numerics, stop rules, breakdown rule, the
// ||b|| == 0 rule and the engine rule are cg_solve_bsr's.
// Checks, in this order, nothing written to d_x when one fails: cg_solve_bsr's (config->preconditioner is not read);
// null F -> INVALID_ARGUMENT; F not square, or of another size or block_dim than A -> INVALID_DIMENSION; missing device
// arrays of F -> INVALID_FORMAT; a malformed block pattern of F -> INVALID_FORMAT; a block row of F whose block columns
// are not strictly ascending -> INVALID_ARGUMENT; a diagonal block of F missing, or with a diagonal entry that is not
// > 0 or not finite -> INVALID_ARGUMENT (on the device, in the one setup read-back).
// The schedules of F's block pattern are the cached ones of sptrsv_bsr (built, and the stream synchronised, by the
// first use per pattern and triangle).
CGResult cg_solve_bsr_ic(const BSRMatrix* A, const BSRMatrix* F, const float* d_b, float* d_x,
                         const CGConfig* config = nullptr);

} // namespace spmv

#endif
