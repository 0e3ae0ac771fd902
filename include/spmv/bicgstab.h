// spmv/bicgstab.h — device-resident Jacobi-preconditioned BiCGSTAB solver for A x = b (A square, non-singular,
// not necessarily symmetric).
//
// The whole iteration runs on the device (gpu-spmv_amd/csrc/bicgstab.hip) the way cg_solve does (spmv/cg.h): the
// scalars alpha, omega and rho live in a device state, every kernel of a step returns at once when the state says
// `done`, and the host enqueues step k+1 before it reads the outcome of step k.  See DESIGN.md §4.10.
#ifndef SPMV_BICGSTAB_H
#define SPMV_BICGSTAB_H

#include "cg.h"
#include "common.h"
#include "csr_matrix.h"

namespace spmv {

// Same fields, defaults and meanings as CGConfig; preconditioner takes CGConfig::NONE or CGConfig::JACOBI.
struct BiCGStabConfig {
    float tolerance;       // stop when ||r||_2 (or ||s||_2 at the half step) <= tolerance * ||b||_2 (recurrences)
    int   max_iterations;
    int   preconditioner;  // CGConfig::Preconditioner
    int   engine;          // -1 auto, 0 direct kernels only, 1 tiled plan from the start where tiled_eligible(A)
    BiCGStabConfig() : tolerance(1e-6f), max_iterations(1000), preconditioner(CGConfig::JACOBI), engine(-1) {}
};

struct BiCGStabResult {
    enum Breakdown { NONE = 0, RHO = 1, ALPHA = 2, OMEGA = 3 };
    int   error_code;         // SpMVError as int
    int   iterations;         // committed iterations (a half step that ends the solve counts as one)
    float relative_residual;  // ||r||/||b|| (recurrence; ||s||/||b|| after a half step) at exit
    int   converged;
    int   breakdown;          // Breakdown
    float elapsed_ms;         // device-event time of the iteration loop (setup excluded, a plan build included)
    BiCGStabResult() : error_code(0), iterations(0), relative_residual(0.0f), converged(0), breakdown(NONE),
                       elapsed_ms(0.0f) {}
};

// Solves A x = b by BiCGSTAB with right preconditioning (M = diag(A) with JACOBI, M = I with NONE):
//     r0 = b - A x0;  r^ = r0 (a stored copy);  p0 = r0;  rho0 = r^.r0
//     step k: p^ = M^-1 p;  v = A p^;  alpha = rho_k / (r^.v);  s = r - alpha v
//             if ||s|| <= tolerance * ||b||: x += alpha p^ and stop (the half step)
//             s^ = M^-1 s;  t = A s^;  omega = (t.s) / (t.t);  x += alpha p^ + omega s^;  r = s - omega t
//             rho_k+1 = r^.r;  stop if ||r|| <= tolerance * ||b||
//             beta = (rho_k+1 / rho_k) (alpha / omega);  p = r + beta (p - omega v)
// d_b: num_rows floats (device).  d_x: num_rows floats (device): the initial guess on entry, the solution on exit.
// A must be square and resident on the device (csr_to_gpu / csr_wrap_device).  config == nullptr: BiCGStabConfig().
//
// Numerics: vectors are fp32.  Every dot product accumulates the exact fp64 products of the fp32 entries into
// per-workgroup partials that are folded in a fixed order; nothing uses float atomics, so a solve is bitwise
// reproducible from run to run on each engine.  alpha = fp32(rho_k / r^.v) and omega = fp32(t.s / t.t) are divided
// in fp64; beta = fp32((rho_k+1 / rho_k) * (alpha / omega)) in fp64 from the fp32 alpha and omega.  They are applied
// with fmaf: s = fmaf(-alpha, v, r) (s overwrites r), x = fmaf(omega, s^, fmaf(alpha, p^, x)),
// r = fmaf(-omega, t, s), p = fmaf(beta, fmaf(-omega, v, p), r).  dinv = 1 / diag(A) in fp32 (__fdiv_rn), where the
// diagonal of row i is the fp32 sum of its stored (i,i) entries in storage order; p^ = p * dinv and s^ = s * dinv
// are stored.  With NONE there is no dinv: p^ is p and s^ is s, and neither copy is stored or read.
//
// Breakdowns end the solve with converged = 0 and a code:
//   ALPHA  r^.v is 0 or not finite (step k): x = x_k unchanged, iterations k, the residual of r_k;
//   OMEGA  omega is 0 or not finite, which includes t.t = 0: x = x_k + alpha p^ (the half step whose residual is s),
//          iterations k + 1, relative residual ||s|| / ||b||; if ||s|| is not finite, x = x_k and iterations k;
//   RHO    rho_k+1 = r^.r is 0 or not finite while ||r|| is above the tolerance: x = x_k+1, iterations k + 1, the
//          residual of r_k+1 (rho_0 is tested the same way at setup, with 0 iterations).
//
// Checks, in this order, before any device work; nothing is written to d_x when one fails:
//   null A / d_b / d_x -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS,
//   converged, 0 iterations; missing device arrays -> INVALID_FORMAT; tolerance < 0 or NaN, max_iterations < 0, an
//   unknown preconditioner or engine -> INVALID_ARGUMENT; overlapping d_b and d_x ranges -> INVALID_ARGUMENT; with
//   JACOBI, a row whose diagonal is missing, zero or not finite -> INVALID_ARGUMENT (checked on the device, read
//   back once during setup).  Unlike cg_solve, a negative diagonal is accepted: BiCGSTAB needs no SPD M.
// ||b|| == 0 writes zeros to x and returns converged after 0 iterations.  An initial guess with
// ||r0|| <= tolerance * ||b|| returns converged after 0 iterations and leaves x unchanged.  max_iterations steps at
// most are run.
//
// Engines, exactly as cg_solve: 0 runs two fused vector-CSR SpMV + dot kernels per iteration; 1 runs the LDS-tiled
// engine (tiled_spmv plus a dot kernel, twice) from the first iteration when the matrix is eligible (else as 0),
// falling back to the direct kernels when the tiled engine has no scratch for this stream; -1 (auto) uses a plan A
// already holds from the start, else builds one after 4 direct iterations for an eligible matrix if the loop has not
// ended by then.  A plan bicgstab_solve builds is cached on A.  bicgstab_solve never touches A's promotion count or
// its merge-path state.  It runs on spmv_get_stream() and returns after the solve completed; its setup synchronises
// that stream — make the call outside a graph capture.
BiCGStabResult bicgstab_solve(const CSRMatrix* A, const float* d_b, float* d_x,
                              const BiCGStabConfig* config = nullptr);

// The same iteration right-preconditioned by a given factorisation M = L U: L the unit lower triangle of LU (its
// stored diagonal is U's), U the upper triangle of LU with the stored diagonal.  LU is any square device CSR matrix
// with num_rows == A->num_rows; the usual one wraps the output of ilu0_csr (spmv/ilu0.h) over A's own structure
// arrays, but its pattern need not be A's.  p^ = U^-1 (L^-1 p) and s^ = U^-1 (L^-1 s) are stored; each is two sparse
// triangular solves of sptrsv_csr's kind (spmv/sptrsv.h: LOWER UNIT, then UPPER NON_UNIT in place, ordered = 0 with
// the schedule's lane count), so a step costs four solves on top of bicgstab_solve's kernels with NONE.  Both level
// schedules of LU are built (and cached with LU) during setup, before the timed loop.
//
// config->preconditioner is not read; tolerance, max_iterations and engine mean what they mean above, and the engine
// choice applies to A only.  Breakdown codes, the half step, ||b|| == 0 and the good-initial-guess return are
// bicgstab_solve's.  Checks, in bicgstab_solve's order with these additions; nothing is written to d_x when one fails:
//   null LU -> INVALID_ARGUMENT (with the other nulls); LU not square or num_rows != A->num_rows -> INVALID_DIMENSION
//   (after A's own); LU without device arrays -> INVALID_FORMAT (with A's); malformed row_ptrs / col_indices of LU ->
//   INVALID_FORMAT (from the analysis); a row of LU whose diagonal is missing, zero or not finite -> INVALID_ARGUMENT
//   (checked on the device, read back once with the setup state; the diagonal of a row is the fp32 sum of its stored
//   (i,i) entries, the rule of sptrsv_csr).
BiCGStabResult bicgstab_solve_lu(const CSRMatrix* A, const CSRMatrix* LU, const float* d_b, float* d_x,
                                 const BiCGStabConfig* config = nullptr);

} // namespace spmv

#endif
