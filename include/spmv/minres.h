// spmv/minres.h — device-resident preconditioned MINRES for (A - shift I) x = b, A symmetric, definite or not.
//
// The short-recurrence, residual-minimising Krylov method for a symmetric matrix (Paige and Saunders 1975): what
// cg_solve is for an SPD matrix and gmres_solve for a non-symmetric one.  The whole iteration runs on the device
// (gpu-spmv_amd/csrc/minres.hip) the way cg_solve does (spmv/cg.h): the scalars of the Lanczos and rotation
// recurrences live in a device state, every kernel of a step returns at once when the state says `done`, and the host
// enqueues step k+1 before it reads the outcome of step k.  See DESIGN.md §4.33.
#ifndef SPMV_MINRES_H
#define SPMV_MINRES_H

#include "cg.h"
#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct MinresConfig {
    float tolerance;       // stop when phibar_k <= tolerance * sqrt(b.M^-1 b) (the recurrence, in the M^-1-norm)
    int   max_iterations;
    int   preconditioner;  // CGConfig::NONE or CGConfig::JACOBI
    int   engine;          // -1 auto, 0 direct kernels only, 1 tiled plan from the start where tiled_eligible(A)
    float shift;           // solves (A - shift I) x = b; the shifted matrix is never formed
    MinresConfig() : tolerance(1e-6f), max_iterations(1000), preconditioner(CGConfig::JACOBI), engine(-1),
                     shift(0.0f) {}
};

struct MinresResult {
    enum Breakdown { NONE = 0, PRECONDITIONER = 1, NOT_FINITE = 2, SINGULAR = 3 };
    int   error_code;              // SpMVError as int
    int   iterations;              // committed steps
    float relative_residual;       // the recurrence: phibar_k / sqrt(b.M^-1 b) at exit (the M^-1-norm; 2-norm with NONE)
    float true_relative_residual;  // ||b - (A - shift I) x||_2 / ||b||_2, recomputed once after the loop from the returned x
    int   converged;
    int   breakdown;               // Breakdown
    float elapsed_ms;              // device-event time of the loop and the recomputed residual (setup excluded, a plan build included)
    MinresResult() : error_code(0), iterations(0), relative_residual(0.0f), true_relative_residual(0.0f),
                     converged(0), breakdown(NONE), elapsed_ms(0.0f) {}
};

// Solves (A - sigma I) x = b, sigma = config->shift, by Paige-Saunders MINRES preconditioned with an SPD M (M = I with
// NONE, M = |diag(A - sigma I)| with JACOBI):
//     r1 = b - (A - sigma I) x0;  y = M^-1 r1;  beta_1 = sqrt(r1.y);  r2 = r1
//     oldb = 0;  dbar = 0;  epsln = 0;  phibar = beta_1;  cs = -1;  sn = 0;  w_0 = w_-1 = 0
//     step k = 1, 2, ...:
//        v = y / beta
//        y = A v - sigma v;  if k >= 2: y -= (beta / oldb) r1
//        alpha = v.y
//        y -= (alpha / beta) r2
//        r1 <- r2 <- y;  y = M^-1 r2
//        oldb = beta;  beta = sqrt(r2.y)
//        oldeps = epsln;  delta = cs dbar + sn alpha;  gbar = sn dbar - cs alpha;  epsln = sn beta;  dbar = -cs beta
//        gamma = sqrt(gbar^2 + beta^2);  cs = gbar / gamma;  sn = beta / gamma;  phi = cs phibar;  phibar = sn phibar
//        w_k = (v - oldeps w_k-2 - delta w_k-1) / gamma
//        x += phi w_k
//        stop if phibar <= tolerance * sqrt(b.M^-1 b)
// d_b: num_rows floats (device).  d_x: num_rows floats (device): the initial guess on entry, the solution on exit.
// A must be square, symmetric (nothing tests that) and resident on the device (csr_to_gpu / csr_wrap_device).
// config == nullptr: MinresConfig().
//
// The stop rule and relative_residual are the recurrence's: phibar_k is ||b - (A - sigma I) x_k|| in the norm of
// M^-1, sqrt(r.M^-1 r), and it is compared with sqrt(b.M^-1 b).  With NONE this is the 2-norm; with JACOBI or a factor
// matrix it is NOT, so the solver always recomputes true_relative_residual, the 2-norm figure, from the x it returns:
// one more fused SpMV-and-dot launch after the loop, inside elapsed_ms, never used for the stop decision and never
// changing `converged`.  The recurrence residual never increases from one step to the next.
//
// Numerics: vectors are fp32.  Every dot product accumulates the exact fp64 products of the fp32 entries into
// per-workgroup partials that are folded in a fixed order; nothing uses float atomics, so a solve is bitwise
// reproducible from run to run on each engine.  alpha, beta, oldb, dbar, epsln, phibar, cs, sn, delta, gbar, gamma and
// phi are fp64 in the device state and never rounded there.  Six coefficients are rounded to fp32 where they meet a
// vector, each computed in fp64 first:
//     c1 = fp32(beta / oldb)    y  = fmaf(-c1, r1, fmaf(-sigma, v, A v))    (k = 1: y = fmaf(-sigma, v, A v))
//     c2 = fp32(alpha / beta)   y  = fmaf(-c2, r2, y)
//     oe = fp32(oldeps), de = fp32(delta), g = fp32(gamma)
//                               w_k = fmaf(-de, w_k-1, fmaf(-oe, w_k-2, v)) / g      (an fp32 division, rounded once)
//     ph = fp32(phi)            x  = fmaf(ph, w_k, x)
//     bt = fp32(beta)           v  = (M^-1 r2) / bt                                   (an fp32 division, rounded once)
// A v is the vector-CSR row sum of the engine in use, sigma the fp32 shift.  With JACOBI, M^-1 r2 = r2 * dinv is never
// stored: dinv = 1 / |d| in fp32 (__fdiv_rn), d = fp32(the fp32 sum of the row's stored (i,i) entries in storage order
// - sigma).  With NONE there is no dinv.  r1, r2 and y share two buffers: y is written over r1, entry by entry, by the
// kernel that reads r1 for the last time, and the two swap roles from step to step.
//
// Ends.  beta == 0 or phibar == 0 is convergence (the Krylov space is exhausted: x is exact in it), not a breakdown.
// Breakdowns end the solve with converged = 0, a code, and x at the last committed iterate:
//   PRECONDITIONER  r.M^-1 r < 0 (at setup, or for the new r2 of a step): M is not positive definite;
//   NOT_FINITE      alpha, beta or gamma is not finite (at setup: r1.y, b.b or b.M^-1 b);
//   SINGULAR        gamma == 0: the Lanczos matrix is singular at this step and the residual cannot be reduced.
// `iterations` counts the committed steps; a step that breaks down is not committed.
//
// Checks, in this order, before any device work; nothing is written to d_x when one fails:
//   null A / d_b / d_x -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS,
//   converged, 0 iterations; missing device arrays -> INVALID_FORMAT; tolerance < 0 or NaN, max_iterations < 0, an
//   unknown preconditioner or engine, a shift that is not finite -> INVALID_ARGUMENT; overlapping d_b and d_x ranges ->
//   INVALID_ARGUMENT; with JACOBI, a row whose diagonal is missing, equal to the shift or not finite ->
//   INVALID_ARGUMENT (checked on the device, read back once during setup).  A negative diagonal is accepted: M takes
//   its absolute value.
// ||b|| == 0 writes zeros to x and returns converged after 0 iterations.  An initial guess with
// beta_1 <= tolerance * sqrt(b.M^-1 b) returns converged after 0 iterations and leaves x unchanged.  max_iterations
// steps at most are run; max_iterations == 0 returns the guess with both of its residuals.
//
// Engines, exactly as cg_solve: 0 runs three launches per step whatever the matrix (the fused vector-CSR SpMV with
// the three-term subtraction and v.y; the alpha subtraction with r2.M^-1 r2; the rotation with w, x and the next v);
// 1 runs the LDS-tiled engine (tiled_spmv into a scratch vector plus an element-wise kernel in place of the first
// launch) from the first step when the matrix is eligible (else as 0), falling back to the direct kernel when the
// tiled engine has no scratch for this stream; -1 (auto) uses a plan A already holds from the start, else builds one
// after 4 direct steps for an eligible matrix if the loop has not ended by then.  A plan minres_solve builds is cached
// on A.  minres_solve never touches A's promotion count or its merge-path state.  It runs on spmv_get_stream() and
// returns after the solve completed; its setup synchronises that stream — make the call outside a graph capture.  The
// workspace is six vectors (two for r1 / r2 / y, v, w_k-1, w_k-2, the tiled engine's A v) and dinv with JACOBI.
MinresResult minres_solve(const CSRMatrix* A, const float* d_b, float* d_x, const MinresConfig* config = nullptr);

// The same iteration preconditioned by M = L L^T: L is the lower triangle of the square device matrix F with its
// stored diagonal, L^T is F's upper triangle with its stored diagonal (cg_solve_ic's contract: entries are taken as
// stored, nothing tests that the two triangles are each other's transpose).  The usual F is ic0_csr of an SPD matrix,
// used for its shifted, indefinite sibling.  z = M^-1 r2 is a stored vector: per step two sptrsv_csr launch sequences
// with ordered = 0 (LOWER NON_UNIT from r2 into z, then UPPER NON_UNIT in place) and one kernel for the partials of
// r2.z come between the second and the third launch, so a step costs 4 + launches(LOWER) + launches(UPPER).  Setup
// applies M^-1 to b once as well, for sqrt(b.M^-1 b).  Everything else — the numerics, the norm of the stop rule, the
// ends, the engines for A — is minres_solve's.  config->preconditioner is not read.
//
// Checks, before any write to d_x: minres_solve's, in their order, then cg_solve_ic's for F: null F ->
// INVALID_ARGUMENT; F not square or of another size than A -> INVALID_DIMENSION; F's device arrays missing ->
// INVALID_FORMAT; malformed structure of F -> INVALID_FORMAT (from the schedule analysis); a row of F whose diagonal is
// missing, not > 0 or not finite -> INVALID_ARGUMENT (checked on the device, read back once during setup).  An F with
// positive diagonal whose L L^T is still not positive definite surfaces as PRECONDITIONER.
MinresResult minres_solve_ic(const CSRMatrix* A, const CSRMatrix* F, const float* d_b, float* d_x,
                             const MinresConfig* config = nullptr);

} // namespace spmv

#endif
