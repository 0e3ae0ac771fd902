// spmv/ilu0.h — incomplete LU factorisation without fill, ILU(0), of a square CSR matrix on the device.
//
// A ~ L U on A's own sparsity pattern: L unit lower triangular, U upper triangular, both kept in one value array laid
// out like A's.  The rows depend on each other exactly as the rows of a LOWER triangular solve do, so the
// factorisation runs over the level schedule sptrsv_csr keeps with the matrix (spmv/sptrsv.h; kernels in
// gpu-spmv_amd/csrc/factor0.hip).  The factor feeds sptrsv_csr (LOWER UNIT, then UPPER NON_UNIT) and
// bicgstab_solve_lu (spmv/bicgstab.h).
#ifndef SPMV_ILU0_H
#define SPMV_ILU0_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct ILU0Result {
    int   error_code;     // SpMVError as int
    int   num_levels;     // dependency levels of A's lower triangle
    int   launches;       // kernel launches of the factorisation (groups of levels)
    int   lanes_per_row;  // lanes that shared a row
    int   zero_pivot;     // lowest row whose u_ii is zero or not finite in the finished factor; -1 when there is none
    float analysis_ms;    // host time of the analysis this call ran; 0 when the cached schedule was used
    float elapsed_ms;     // device-event time of the factorisation launches (the pivot scan included)
    ILU0Result() : error_code(0), num_levels(0), launches(0), lanes_per_row(0), zero_pivot(-1), analysis_ms(0.0f),
                   elapsed_ms(0.0f) {}
};

// Factors the square matrix A (resident on the device: csr_to_gpu / csr_wrap_device) into d_lu_values.
//
// Storage: d_lu_values holds A->nnz floats (device) in A's own pattern: the positions left of the diagonal hold L
// (its unit diagonal is not stored), the diagonal and the positions right of it hold U.  d_lu_values == A->d_values
// factors in place; any other overlap of the two ranges is INVALID_ARGUMENT.  The factor matrix is a header over
// A's structure arrays and d_lu_values that owns nothing (C ABI and Python:
//     csr_wrap_device(n, n, nnz, A->d_row_ptrs, A->d_col_indices, d_lu_values);
// from C++, a CSRMatrix{} with those six fields filled in); nothing else is allocated for it.
//
// Arithmetic (ilu0_cpu_csr below is its definition): rows in ascending order; row i starts from A's values; for each
// stored k < i in ascending column order, l_ik = a_ik / u_kk (one rounding, __fdiv_rn), and for every stored j > k of
// row i that row k also stores, a_ij = fmaf(-l_ik, u_kj, a_ij).  Every entry is updated by one operation per k, in
// ascending k, so the result does not depend on how many lanes share a row: the device factor is bit-identical to
// ilu0_cpu_csr at every lane count.  There is no tolerance and no ordered / unordered switch.
//
// Requirements on A, checked in this order before any device work; d_lu_values is untouched when one fails:
//   null A / d_lu_values -> INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS;
//   missing device arrays -> INVALID_FORMAT; d_lu_values overlapping A->d_values without being equal ->
//   INVALID_ARGUMENT; then from the analysis: row_ptrs not monotone (or outside [0, nnz]) or a column index outside
//   [0, num_rows) -> INVALID_FORMAT; a row whose columns are not strictly ascending (unsorted or repeated columns,
//   legal elsewhere in the library) -> INVALID_ARGUMENT; a row without a stored diagonal -> INVALID_ARGUMENT.
//
// Pivots: a zero or non-finite pivot is not an error; the divisions give the IEEE quotient, as in sptrsv_csr, and
// error_code stays SUCCESS.  zero_pivot reports the lowest such row of the finished factor (an integer minimum over a
// scan of the diagonal: deterministic).
//
// Schedule: A's cached LOWER schedule of sptrsv_csr, built (and the stream synchronised) by the first call on the
// matrix, found again by later calls (analysis_ms == 0) and by LOWER solves with the factor matrix, which shares A's
// structure arrays.  Launches as sptrsv_csr's: a level of more than 256 rows is a launch of its own, consecutive
// narrower levels are one launch of one workgroup with a barrier in between (at most 8192 levels per launch); no
// workgroup waits for another one.  1, 2, 4, ... or 64 lanes share a row, from the mean number of stored entries per
// row.  Runs on spmv_get_stream() and returns after the factorisation completed.
ILU0Result ilu0_csr(const CSRMatrix* A, float* d_lu_values);

// The same factorisation enqueued on `stream` without timing, the pivot scan or a final synchronisation; returns the
// error code.  A first call per matrix still runs the analysis and synchronises `stream` for it: call
// sptrsv_analyze(A, LOWER) (or ilu0_csr) first.
int ilu0_csr_async(const CSRMatrix* A, float* d_lu_values, hipStream_t stream);

// The factorisation on A's HOST arrays, the definition of the arithmetic above.  lu_values: A->nnz floats, may be
// A->values (in place).  *zero_pivot (may be null) as ILU0Result::zero_pivot.  Returns the error code: null arguments
// or missing host arrays -> INVALID_ARGUMENT, not square -> INVALID_DIMENSION, malformed arrays -> INVALID_FORMAT, a
// row not strictly ascending or without a stored diagonal -> INVALID_ARGUMENT; lu_values is untouched on any error.
int ilu0_cpu_csr(const CSRMatrix* A, float* lu_values, int* zero_pivot);

} // namespace spmv

#endif
