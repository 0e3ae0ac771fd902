// spmv/ic0.h — incomplete Cholesky factorisation without fill, IC(0), of a square CSR matrix on the device.
//
// A ~ L L^T on the pattern of A's lower triangle: L lower triangular with its diagonal stored.  The rows depend on
// each other exactly as the rows of a LOWER triangular solve do, so the factorisation runs over the level schedule
// sptrsv_csr keeps with the matrix (spmv/sptrsv.h; kernels in gpu-spmv_amd/csrc/factor0.hip).  The
// factor feeds sptrsv_csr (LOWER NON_UNIT, then UPPER NON_UNIT) and cg_solve_ic (spmv/cg.h).
#ifndef SPMV_IC0_H
#define SPMV_IC0_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct IC0Result {
    int   error_code;     // SpMVError as int
    int   num_levels;     // dependency levels of A's lower triangle
    int   launches;       // kernel launches of the factorisation (groups of levels)
    int   lanes_per_row;  // lanes that shared a row
    int   bad_pivot;      // lowest row whose finished l_ii is not > 0 or not finite; -1 when there is none
    float analysis_ms;    // host time of the analysis this call ran; 0 when the cached schedule was used
    float elapsed_ms;     // device-event time of the factorisation launches (the pivot scan included)
    IC0Result() : error_code(0), num_levels(0), launches(0), lanes_per_row(0), bad_pivot(-1), analysis_ms(0.0f),
                  elapsed_ms(0.0f) {}
};

// Factors the square matrix A (resident on the device: csr_to_gpu / csr_wrap_device) into d_l_values.  Only the
// values of A's lower triangle and diagonal are read (A is taken to be symmetric).
//
// Storage: d_l_values holds A->nnz floats (device) in A's own pattern: the positions on and left of the diagonal hold
// L, and position (i,j) with j > i holds l_ji, that is L^T.  A header over A's structure arrays and d_l_values that
// owns nothing (C ABI and Python:
//     csr_wrap_device(n, n, nnz, A->d_row_ptrs, A->d_col_indices, d_l_values);
// from C++, a CSRMatrix{} with those six fields filled in) therefore serves both sptrsv_csr LOWER NON_UNIT and UPPER
// NON_UNIT: no transpose and no second array.  d_l_values == A->d_values factors in place (A's upper values are then
// replaced by L^T); any other overlap of the two ranges is INVALID_ARGUMENT.
//
// Arithmetic (ic0_cpu_csr below is its definition): rows in ascending order; row i starts from A's lower and diagonal
// values w; for each stored k < i in ascending column order, l_ik = w_ik / l_kk (one rounding), then for every stored
// j of row i with k < j < i for which (k,j) is stored, w_ij = fmaf(-l_ik, l_jk, w_ij), and w_ii = fmaf(-l_ik, l_ik,
// w_ii); at the end l_ii = sqrt(w_ii), correctly rounded.  Every entry takes one operation per k, in ascending k, so
// the result does not depend on how many lanes share a row: the device factor is bit-identical to ic0_cpu_csr at
// every lane count.  There is no tolerance and no ordered / unordered switch.
//
// Requirements on A, checked in this order before any device work; d_l_values is untouched when one fails:
//   null A / d_l_values -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS;
//   missing device arrays -> INVALID_FORMAT; d_l_values overlapping A->d_values without being equal ->
//   INVALID_ARGUMENT; then from the analysis: row_ptrs not monotone (or outside [0, nnz]) or a column index outside
//   [0, num_rows) -> INVALID_FORMAT; a row whose columns are not strictly ascending -> INVALID_ARGUMENT; a row without
//   a stored diagonal -> INVALID_ARGUMENT; a pattern that is not structurally symmetric (a stored (i,k) without a
//   stored (k,i)) -> INVALID_ARGUMENT.
//
// Pivots: a non-positive or non-finite w_ii is not an error; the square root and the divisions give their IEEE
// results and error_code stays SUCCESS.  bad_pivot reports the lowest row whose finished l_ii is not > 0 or not finite
// (an integer minimum over a scan of the diagonal: deterministic).
//
// Schedule: A's cached LOWER schedule of sptrsv_csr, built (and the stream synchronised) by the first call on the
// matrix, found again by later calls (analysis_ms == 0) and by LOWER solves with the factor matrix, which shares A's
// structure arrays.  The symmetry of the pattern is tested by that analysis and kept with the schedule.  Launches as
// ilu0_csr's.  1, 2, 4, ... or 64 lanes share a row, from the mean number of stored entries per row.  Runs on
// spmv_get_stream() and returns after the factorisation completed.
IC0Result ic0_csr(const CSRMatrix* A, float* d_l_values);

// The same factorisation enqueued on `stream` without timing, the pivot scan or a final synchronisation; returns the
// error code.  A first call per matrix still runs the analysis and synchronises `stream` for it: call
// sptrsv_analyze(A, LOWER) (or ic0_csr) first.
int ic0_csr_async(const CSRMatrix* A, float* d_l_values, hipStream_t stream);

// The factorisation on A's HOST arrays, the definition of the arithmetic above.  l_values: A->nnz floats, may be
// A->values (in place).  *bad_pivot (may be null) as IC0Result::bad_pivot.  Returns the error code: null arguments or
// missing host arrays -> INVALID_ARGUMENT, not square -> INVALID_DIMENSION, malformed arrays -> INVALID_FORMAT, a row
// not strictly ascending or without a stored diagonal, or a one-sided entry -> INVALID_ARGUMENT; l_values is untouched
// on any error.
int ic0_cpu_csr(const CSRMatrix* A, float* l_values, int* bad_pivot);

} // namespace spmv

#endif
