// spmv/eigs.h — device-resident thick-restart Lanczos for a few extreme eigenpairs of a symmetric matrix, and the
// small dense symmetric eigen-solve it is built on.
//
// The whole iteration runs on the device (gpu-spmv_amd/csrc/eigs.hip) the way gmres_solve does (spmv/gmres.h): the
// projected matrix T, the Ritz decomposition and the stop tests live in device memory, every kernel of a step returns
// at once when the state says the cycle is closed or the call is done, and the host enqueues step j+1 before it reads
// the outcome of step j.  See DESIGN.md §4.20.
#ifndef SPMV_EIGS_H
#define SPMV_EIGS_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct EigsConfig {
    enum Which { LARGEST = 0, SMALLEST = 1 };   // algebraic: the most positive / the most negative end
    int   num_values;      // k, 1..32 and <= num_rows
    int   which;           // Which
    int   basis;           // m: Lanczos vectors per cycle, k < m <= 64; 0 = min(max(2k, 20), 64)
    float tolerance;       // pair i passes when ||A y_i - theta_i y_i||_2 <= tolerance * max_l |theta_l|
    int   max_iterations;  // cap on the Lanczos steps (= SpMVs of the iteration) of all cycles together
    int   engine;          // -1 auto, 0 direct kernels only, 1 tiled plan from the start where tiled_eligible(A)
    EigsConfig() : num_values(1), which(LARGEST), basis(0), tolerance(1e-5f), max_iterations(1000), engine(-1) {}
};

struct EigsResult {
    enum Breakdown { NONE = 0, INVARIANT_SUBSPACE = 1, NOT_FINITE = 2 };
    int   error_code;     // SpMVError as int
    int   iterations;     // Lanczos steps (columns of T committed) over all cycles
    int   restarts;       // thick restarts
    int   converged;      // number of returned pairs whose RECOMPUTED residual passes
    int   breakdown;      // Breakdown
    float max_residual;   // the largest recomputed residual norm of the returned pairs (0 when none is returned)
    float elapsed_ms;     // device-event time of the iteration loop and the finish (setup excluded, a plan build included)
    EigsResult() : error_code(0), iterations(0), restarts(0), converged(0), breakdown(NONE), max_residual(0.0f),
                   elapsed_ms(0.0f) {}
};

// Computes k = config->num_values eigenpairs (theta_i, y_i) at one end of the spectrum of the symmetric matrix A.
// A: square, resident on the device (csr_to_gpu / csr_wrap_device).  A is symmetric BY THE CALLER'S CONTRACT: it is
// not checked (as cg_solve does not check it); for a non-symmetric A the results are meaningless but defined.
// d_values: k floats (device), in the order asked for: descending for LARGEST, ascending for SMALLEST.
// d_vectors: vector i is num_rows floats at d_vectors + i * ldv, ldv >= num_rows; elements [num_rows, ldv) of each
// vector are never written.  d_residuals: k floats (device) or null.  d_v0: the start vector, num_rows floats
// (device), or null.  No alignment beyond that of a float is demanded of any pointer.  config == nullptr:
// EigsConfig().
//
// A limit of every single-vector Krylov method: it returns ONE copy of a multiple eigenvalue.  "The k extreme
// eigenvalues" therefore holds for spectra whose extreme eigenvalues are simple; otherwise every returned pair is a
// true eigenpair to the stated residual, and the values are the extreme ones of the Krylov space of the start vector.
//
// The start vector.  d_v0 == nullptr: start_e = to_unit(draw(kEigsStartSeed, stream 3, kEigsStartTag, e)), the
// floats of gen_vector(seed = 0x45494753, tag = 0) and of synth.vector(0x45494753, 0, n): uniform in [-1, 1), never
// the zero vector and never the all-ones vector (an eigenvector of every graph Laplacian).  beta_0 = sqrt(start.start);
// v_0 = start * fp32(1 / beta_0).  A caller's start vector with beta_0 == 0 -> INVALID_ARGUMENT, with a beta_0 that is
// not finite -> breakdown NOT_FINITE (both found on the device, read back once during setup).
//
// Numerics.  Vectors are fp32.  Every dot product accumulates the exact fp64 products of the fp32 entries into
// per-workgroup partials that are folded in a fixed order; nothing uses float atomics, so a call is bitwise
// reproducible from run to run on each engine.  T, the Ritz decomposition and the tests are fp64.
//
// Step j (the basis v_0..v_j is ready), classical Gram-Schmidt applied twice against ALL of v_0..v_j, exactly
// gmres_solve's rule:
//     w = A v_j (the engine's SpMV)
//     h1_i = v_i.w for all i <= j in one pass;  w <- fmaf(-fp32(h1_i), v_i, w) for i ascending
//     h2_i = v_i.w on the updated w;            w <- fmaf(-fp32(h2_i), v_i, w) for i ascending
//     h_i = double(fp32(h1_i)) + double(fp32(h2_i));   beta = sqrt(w.w)
//     T is a dense symmetric m x m matrix: T[i][j] = T[j][i] = h_i for i <= j.  It is NOT stored as a tridiagonal:
//     after a thick restart the "arrowhead" entries come out of the same orthogonalisation with no special case.
// If any h_i or beta is not finite the breakdown is NOT_FINITE: the call ends, see "Outputs" below.  The space is
// INVARIANT when beta <= 2^-20 * max_i |h_i| (beta == 0, the lucky breakdown, or a w that is nothing but the rounding
// of the orthogonalisation: at fp32 such a w has no direction left), or when j + 1 == num_rows (the space is the
// whole one).  Otherwise v_j+1 = w * fp32(1 / beta).  `iterations` counts the committed columns.
//
// A cycle closes after step j when j + 1 == m, or `iterations` reaches max_iterations, or the space is invariant.
// Closing a cycle with c columns:
//     (theta, S) = sym_eig_small of T[0:c, 0:c] (below); the Ritz values are sorted by `which` (descending for
//     LARGEST, ascending for SMALLEST), equal values by ascending index in sym_eig_small's output.
//     The residual estimate of pair i is |beta * S[c-1, i]|; it passes when <= fp64(tolerance) * max_l |theta_l| over
//     all c Ritz values.
//     If the first k estimates pass (c >= k), or the cap is reached, or the space is invariant: finish.
//     Otherwise thick-restart: p = min(k + (m - k) / 2, c - 1);
//         v_i <- fp32(sum over l < c ascending of double(fp32(S[l,i])) * double(v_l)) for i < p, each sum in fp64
//         and rounded once;  v_p <- v_c;  T <- diag(theta_0..theta_p-1);  the next step is column p.
// Finish.  The f = min(k, c) wanted Ritz vectors are rotated out the same way into d_vectors.  Then, on the device,
// for every returned pair: t = A y_i (a vector-CSR SpMV on every engine: the caller's pitch need not suit the tiled
// engine), d_e = fmaf(-fp32(theta_i), y_e, t_e), r_i = sqrt(d.d) in fp64.  Pair i passes when
// r_i <= fp64(tolerance) * max_l |theta_l|.  `converged`, `max_residual` and d_residuals ALWAYS come from these
// recomputed figures, never from the estimate.  If a pair fails although its estimate passed, and neither the cap nor
// an invariant space ends the call, the thick restart is taken after all and the iteration goes on; the outputs are
// rewritten by the next finish.
//
// The floor of an fp32 basis.  The recomputed residual cannot fall below the rounding of the fp32 basis, the
// rotation and one SpMV.  Measured with the numpy restatement on the matrices and (k, m) pairs of tests/eigs_cases.py
// (relative to max |theta|): at the default 1e-5 every case converges; at 1e-6 every case with
// m >= 2k does, and a basis of m = k + 2 no longer does on two of the matrices (2 and 4 of 7 pairs after 6000 steps);
// at 3e-7 the cases with m >= 2k still converge and seven with m = k + 2 do not.  A smaller tolerance is accepted,
// but the call may then run to max_iterations and return converged < k.
//
// Outputs.  d_values[i] = fp32(theta_i), d_residuals[i] = fp32(r_i) for i < f.  When fewer than k pairs are returned
// (f < k: max_iterations reached before k columns, or an invariant space of fewer than k dimensions, breakdown
// INVARIANT_SUBSPACE then) and for every i when the breakdown is NOT_FINITE (f = 0), d_values[i] and d_residuals[i]
// are NaN and vector i is zero.  `converged` counts the returned pairs that pass.
//
// Checks, in this order, before any device work; nothing is written when one fails:
//   null A / d_values / d_vectors -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 ->
//   SUCCESS, nothing written; missing device arrays -> INVALID_FORMAT; num_values outside [1, 32] or > num_rows ->
//   INVALID_ARGUMENT; basis not 0 and outside (num_values, 64] -> INVALID_ARGUMENT; tolerance < 0 or NaN ->
//   INVALID_ARGUMENT; max_iterations < 0 -> INVALID_ARGUMENT; an unknown which or engine -> INVALID_ARGUMENT;
//   ldv < num_rows -> INVALID_ARGUMENT; any two of the ranges d_values[0, k), d_residuals[0, k), d_v0[0, n) and
//   d_vectors[0, (k - 1) ldv + n) overlapping -> INVALID_ARGUMENT.  Then a failed allocation -> CUDA_MALLOC.
// The basis is validated against k alone; the m that is used is min(basis or its default, num_rows).  For
// num_rows <= k that m equals num_rows, no thick restart can happen (a cycle that reaches m == num_rows columns spans
// the whole space and finishes), and at num_rows == 1 the call is one step: theta_0 = A[0][0], y_0 = +-1.
//
// Engines, as gmres_solve.  It runs on spmv_get_stream() and returns after the call completed; it synchronises that
// stream at setup and at every cycle close — make the call outside a graph capture.
EigsResult eigs_sym(const CSRMatrix* A, float* d_values, float* d_vectors, long long ldv, float* d_residuals,
                    const float* d_v0, const EigsConfig* config = nullptr);

constexpr unsigned long long kEigsStartSeed = 0x45494753ull;
constexpr unsigned long long kEigsStartTag = 0ull;

// The eigen-decomposition of the dense symmetric fp64 matrix T of order n <= 64 (T[i * ld + j], ld >= n; only what
// lies inside [0, n) x [0, n) is read; both triangles are read and should agree): values[i] ascending (equal values
// in the order of their diagonal position), eigenvector i as n doubles at vectors + i * ld.  HOST pointers; with
// on_device != 0 the matrix is copied to the device, decomposed there by the one-workgroup kernel eigs_sym uses, and
// copied back.  Both forms give the same bits.  Returns an SpMVError code: INVALID_ARGUMENT for a null pointer, n < 0,
// n > 64 or ld < n; n == 0 writes nothing.
//
// The rule: cyclic Jacobi with a fixed round-robin pairing.  Every fp64 product, sum, quotient and root below is
// rounded separately (no contraction into fused multiply-adds).
//     W = T, S = I, N = n rounded up to even, scale = max |T[i][j]|, thr = scale * 2^-53.
//     A sweep is N - 1 rounds.  Round r pairs position 0: (r, N - 1) and position i = 1..N/2 - 1:
//     ((r + i) mod (N - 1), (r - i + N - 1) mod (N - 1)); each pair is ordered p < q; a pair with q >= n (the bye of
//     an odd order) does nothing.
//     A pair rotates when |W[p][q]| > thr.  Then tau = (W[q][q] - W[p][p]) / (2 W[p][q]),
//     t = sign(tau) / (|tau| + sqrt(1 + tau tau)) (sign(0) = +1), c = 1 / sqrt(1 + t t), s = t c.
//     All parameters of a round come from W as the round finds it.  Then for every rotating pair
//         columns: (W[i][p], W[i][q]) <- (c W[i][p] - s W[i][q],  s W[i][p] + c W[i][q]) for all i, and the same for S;
//         rows, after the columns of ALL pairs: (W[p][j], W[q][j]) <- (c W[p][j] - s W[q][j],  s W[p][j] + c W[q][j]);
//         W[p][q] = W[q][p] = 0.
//     The pairs of a round touch disjoint rows and columns, so the order among them does not matter.
//     Stop after the first sweep in which no pair rotated, or after 30 sweeps.
//     values = diag(W) sorted ascending, ties by position; vectors = the columns of S in that order.
int sym_eig_small(int n, const double* T, int ld, double* values, double* vectors, int on_device);

} // namespace spmv

#endif
