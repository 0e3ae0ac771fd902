// spmv/gmres.h — device-resident restarted GMRES(m) for A x = b (A square, non-singular, not necessarily symmetric),
// right-preconditioned by nothing, by diag(A) or by a given factorisation L U.
//
// The whole iteration runs on the device (gpu-spmv_amd/csrc/gmres.hip) the way bicgstab_solve does
// (spmv/bicgstab.h): the Hessenberg column, the Givens rotations and the stop tests live in device memory, every
// kernel of a step returns at once when the state says the cycle is closed or the solve is done, and the host
// enqueues step k+1 before it reads the outcome of step k.  See DESIGN.md §4.14.
#ifndef SPMV_GMRES_H
#define SPMV_GMRES_H

#include "cg.h"
#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct GMRESConfig {
    float tolerance;       // converged when ||b - A x||_2 <= tolerance * ||b||_2, on the recomputed residual
    int   max_iterations;  // cap on the Arnoldi steps of all cycles together
    int   restart;         // m: Arnoldi steps per cycle, 1..64
    int   preconditioner;  // CGConfig::Preconditioner (gmres_solve only)
    int   engine;          // -1 auto, 0 direct kernels only, 1 tiled plan from the start where tiled_eligible(A)
    GMRESConfig() : tolerance(1e-6f), max_iterations(1000), restart(30), preconditioner(CGConfig::JACOBI),
                    engine(-1) {}
};

struct GMRESResult {
    enum Breakdown { NONE = 0, SINGULAR = 1, NOT_FINITE = 2 };
    int   error_code;         // SpMVError as int
    int   iterations;         // Arnoldi steps (Hessenberg columns committed to x) over all cycles
    int   restarts;           // cycles begun after the first
    float relative_residual;  // ||b - A x|| / ||b|| of the returned x, recomputed (never the Arnoldi estimate)
    int   converged;
    int   breakdown;          // Breakdown
    float elapsed_ms;         // device-event time of the iteration loop (setup excluded, a plan build included)
    GMRESResult() : error_code(0), iterations(0), restarts(0), relative_residual(0.0f), converged(0),
                    breakdown(NONE), elapsed_ms(0.0f) {}
};

// Solves A x = b by GMRES(m), m = config->restart, with right preconditioning (M = diag(A) with JACOBI, M = I with
// NONE).  d_b: num_rows floats (device).  d_x: num_rows floats (device): the initial guess on entry, the solution on
// exit.  A must be square and resident on the device (csr_to_gpu / csr_wrap_device).  config == nullptr:
// GMRESConfig().
//
// Numerics.  Vectors are fp32.  Every dot product accumulates the exact fp64 products of the fp32 entries into
// per-workgroup partials that are folded in a fixed order; nothing uses float atomics, so a solve is bitwise
// reproducible from run to run on each engine.  The Hessenberg matrix, the rotations, g and y are fp64, with every
// product and sum rounded separately (no fused multiply-adds).
//
// Setup and every restart are the same code:
//     r = fp32(b - A x) (the engine's SpMV, one subtraction);  beta = sqrt(r.r);  threshold = fp64(tolerance) ||b||
//     beta <= threshold: the solve ends converged;  else v_0 = r * fp32(1 / beta) and g_0 = beta.
// A restart is therefore bit for bit a new solve from the current x.
//
// Step j (0 <= j < m), classical Gram-Schmidt applied twice:
//     z = M^-1 v_j (stored only when M != I; with JACOBI z = v_j * dinv);  w = A z
//     h1_i = v_i.w for all i <= j in one pass;  w <- fmaf(-fp32(h1_i), v_i, w) for i ascending
//     h2_i = v_i.w on the updated w;            w <- fmaf(-fp32(h2_i), v_i, w) for i ascending
//     the column records what was applied: h_i = double(fp32(h1_i)) + double(fp32(h2_i)),  h_j+1 = sqrt(w.w)
//     the earlier rotations (c_i, s_i), i < j, are applied to the column: (h_i, h_i+1) <- (c_i h_i + s_i h_i+1,
//     -s_i h_i + c_i h_i+1);  d = sqrt(h_j^2 + h_j+1^2);  c_j = h_j / d, s_j = h_j+1 / d, h_j <- d
//     g_j+1 = -s_j g_j;  g_j = c_j g_j;  the estimate of the residual norm is |g_j+1|.
// If any of h_0..h_j+1 or d is not finite the breakdown is NOT_FINITE; else if d is 0 it is SINGULAR.
//
// The cycle closes after step j when the estimate <= threshold, or j + 1 = m, or the total number of steps reaches
// max_iterations, or h_j+1 = 0 (the lucky breakdown: there is no next vector, and it is not an error).  Otherwise
// v_j+1 = w * fp32(1 / h_j+1).
//
// Closing a cycle of k columns: R y = g by back-substitution in fp64 (R the rotated columns);
// u = sum over i ascending of fmaf(fp32(y_i), v_i, u) from u = 0;  x <- x + fp32(M^-1 u), one rounded addition (with
// JACOBI M^-1 u = u * dinv, one rounded product).  Then r = b - A x and its norm are recomputed as at setup.
// `converged` and `relative_residual` ALWAYS come from that recomputed residual, never from the estimate: if the
// estimate was optimistic, the next cycle simply begins (unless max_iterations is reached).  This is the property
// cg_solve and bicgstab_solve do not have: their flags rest on a recurrence residual.
//
// A breakdown in column j ends the solve: columns 0..j-1 of the cycle are committed to x as above (x is unchanged
// if j = 0), the residual is recomputed, `iterations` counts committed columns only, and `converged` is 0 unless the
// recomputed residual passes.  A b or an A x0 that is not finite is NOT_FINITE at setup: x is left at the guess.
//
// dinv = 1 / diag(A) in fp32 (correctly rounded), the diagonal of row i being the fp32 sum of its stored (i,i)
// entries in storage order, as in bicgstab_solve; a negative diagonal is accepted.
//
// Checks, in this order, before any device work; nothing is written to d_x when one fails:
//   null A / d_b / d_x -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS,
//   converged, 0 iterations; missing device arrays -> INVALID_FORMAT; tolerance < 0 or NaN, max_iterations < 0,
//   restart outside [1, 64], an unknown preconditioner or engine -> INVALID_ARGUMENT; overlapping d_b and d_x
//   ranges -> INVALID_ARGUMENT; with JACOBI, a row whose diagonal is missing, zero or not finite -> INVALID_ARGUMENT
//   (checked on the device, read back once during setup).  A failed allocation of the basis ((restart + 1) vectors
//   with a leading dimension rounded up to 256 bytes) or of the work vectors -> CUDA_MALLOC, x untouched.
// ||b|| == 0 writes zeros to x and returns converged after 0 iterations.  An initial guess with
// ||b - A x0|| <= tolerance * ||b|| returns converged after 0 iterations and leaves x unchanged.  max_iterations == 0
// returns the guess with its residual.
//
// Engines, as bicgstab_solve: 0 runs a vector-CSR SpMV kernel per step; 1 runs the LDS-tiled engine (tiled_spmv)
// from the first step when the matrix is eligible (else as 0), falling back to the direct kernels when the tiled
// engine has no scratch for this stream; -1 (auto) uses a plan A already holds from the start, else builds one after
// 4 direct steps for an eligible matrix if the loop has not ended by then.  A plan gmres_solve builds is cached on
// A.  gmres_solve never touches A's promotion count or its merge-path state.  It runs on spmv_get_stream() and
// returns after the solve completed; its setup synchronises that stream — make the call outside a graph capture.
GMRESResult gmres_solve(const CSRMatrix* A, const float* d_b, float* d_x, const GMRESConfig* config = nullptr);

// The same iteration right-preconditioned by a given factorisation M = L U: L the unit lower triangle of LU, U the
// upper triangle of LU with the stored diagonal, as in bicgstab_solve_lu (usually ilu0_csr's output wrapped over A's
// structure arrays).  z = U^-1 (L^-1 v_j) and M^-1 u = U^-1 (L^-1 u) are two sparse triangular solves of sptrsv_csr's
// kind each (LOWER UNIT, then UPPER NON_UNIT in place, ordered = 0 with the schedule's lane count).  Both level
// schedules of LU are built (and cached with LU) during setup, before the timed loop.
//
// config->preconditioner is not read.  Checks, in gmres_solve's order with bicgstab_solve_lu's additions; nothing is
// written to d_x when one fails:
//   null LU -> INVALID_ARGUMENT (with the other nulls); LU not square or num_rows != A->num_rows -> INVALID_DIMENSION
//   (after A's own); LU without device arrays -> INVALID_FORMAT (with A's); malformed row_ptrs / col_indices of LU ->
//   INVALID_FORMAT (from the analysis); a row of LU whose diagonal is missing, zero or not finite -> INVALID_ARGUMENT
//   (checked on the device, read back once with the setup state).
GMRESResult gmres_solve_lu(const CSRMatrix* A, const CSRMatrix* LU, const float* d_b, float* d_x,
                           const GMRESConfig* config = nullptr);

} // namespace spmv

#endif
