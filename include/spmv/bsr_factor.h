// spmv/bsr_factor.h — block IC(0) of a square BSR matrix and the block triangular solves with its factor (kernels in
// gpu-spmv_amd/csrc/bsr_tri.hip, host twins, checks and drivers in bsr_tri_host.cpp, the arithmetic both sides share in
// bsr_tri_impl.h).  The solver that uses them is cg_solve_bsr_ic in spmv/cg.h.
//
// THE FACTOR FORMAT.  d_f_values holds num_blocks * b * b floats in A's own block pattern, so
//     bsr_wrap_device(n, n, b, num_blocks, A->d_block_row_ptrs, A->d_block_cols, d_f_values)
// is the factor matrix F and serves both solves.  With size_I = min(b, n - I*b):
//   position (I,K), K < I   L_IK, row-major
//   position (I,I)          V_I = fl32(L_II^-1), STORED SYMMETRICALLY: element (r,c) with r >= c holds V_rc and element
//                           (c,r) holds the same number.  The forward solve reads the lower triangle of the block row by
//                           row, the backward solve reads the upper triangle row by row and so gets L_II^-T; neither
//                           transposes.  Rows and columns >= size_I are +0.0f.
//   position (K,I), K < I   L_IK^T: element (m,r) = (L_IK)_rm
// THE INVERSE OF THE DIAGONAL BLOCK IS STORED, NOT L_II ITSELF: the solves then end every block row in a b x b multiply
// instead of a dependent substitution.  (A caller that wants L_II inverts the lower triangle of V_I.)
#ifndef SPMV_BSR_FACTOR_H
#define SPMV_BSR_FACTOR_H

#include "bsr_matrix.h"
#include "common.h"
#include "sptrsv.h"

namespace spmv {

struct BsrIC0Result {
    int   error_code;     // SpMVError as int
    int   num_levels;     // dependency levels of the block pattern's lower triangle
    int   launches;       // kernel launches of the factorisation (groups of levels)
    int   lanes_per_row;  // lanes that shared a BLOCK row
    int   bad_pivot;      // lowest block row whose diagonal stage met a pivot that is not > 0 or not finite; -1: none
    float analysis_ms;    // host time of the analysis this call ran; 0 when the cached schedule was used
    float elapsed_ms;     // device-event time of the factorisation launches
    BsrIC0Result() : error_code(0), num_levels(0), launches(0), lanes_per_row(0), bad_pivot(-1), analysis_ms(0.0f),
                     elapsed_ms(0.0f) {}
};

// ---- block IC(0) ----
// bsr_ic0_cpu (host arrays; f_values may be A->values) is the definition.  Block rows in ascending order.  Block row I
// starts from W = A's blocks (I,J), J <= I; of the diagonal block only r >= c is read, A is taken as symmetric.  For
// every stored K < I, in ascending block column:
//   1. L_IK = W_IK L_KK^-T in fp32: (L_IK)_rc = s after s = +0.0f; s = fmaf(w_rm, V_K[c][m], s) for m = 0 .. c
//   2. for every stored J of block row I with K < J < I for which (K,J) is stored, at position q (F_q holds L_JK^T):
//      w^IJ_rc = fmaf(-l_rm, F_q[m][c], w^IJ_rc) for m = 0 .. b-1
//   3. on the diagonal block, for r >= c: w_rc = fmaf(-l_rm, l_cm, w_rc), m = 0 .. b-1
//   and L_IK is mirrored to (K,I).
// At the end the leading size_I part of W_II's lower triangle goes to fp64: Cholesky, then the inverse of the factor,
// every product, sum, division and root rounded on its own (the first two stages of bsr_diag_inverse_cpu, spmv/bsr.h),
// and every entry of V is rounded once to fp32.  Rows >= size_I of the last block row's blocks, and the matching
// columns of its mirrors, are written +0.0f and not computed.
// Every element takes a fixed sequence of operations, so the device factor is bit for bit bsr_ic0_cpu at every lane
// count: no tolerance, no ordered switch.
//
// Pivots: a pivot that is not > 0 or not finite is not an error; the IEEE results flow on and error_code stays
// SUCCESS.  bad_pivot is the lowest block row that met one (an integer minimum: deterministic).
//
// Checks, in this order; the output is untouched when one fails: null A / output -> INVALID_ARGUMENT; not square ->
// INVALID_DIMENSION; no rows -> SUCCESS; a bad shape or missing arrays -> INVALID_FORMAT; an output that overlaps A's
// values without being equal -> INVALID_ARGUMENT; a malformed block pattern -> INVALID_FORMAT; a block row whose block
// columns are not strictly ascending, a block row without a diagonal block, or a block pattern that is not structurally
// symmetric -> INVALID_ARGUMENT.
int bsr_ic0_cpu(const BSRMatrix* A, float* f_values, int* bad_pivot);

// The device factorisation: walks the LOWER level schedule of the block pattern (the schedule of sptrsv_bsr below, kept
// with the matrix) with the two launch shapes of sptrsv_csr: a grid over a wide level, one workgroup over a run of
// narrow levels with a barrier in between.  No workgroup waits for another.  A group of 1 .. 64 lanes owns a block row
// (spmv_bsr's rule on the lower triangle; SPMV_DEBUG=bsr_tri_lanes=N forces a count).  d_f_values == A->d_values factors
// in place.  Runs on spmv_get_stream() and returns after the factorisation completed.
BsrIC0Result bsr_ic0(const BSRMatrix* A, float* d_f_values);
// The launches alone on `stream`: no timing, no bad_pivot, no final synchronisation.  A first call per matrix still
// analyses and synchronises `stream`: call sptrsv_analyze_bsr(A, LOWER) first.
int bsr_ic0_async(const BSRMatrix* A, float* d_f_values, hipStream_t stream);

// ---- block triangular solve ----
// T x = b, T the config->uplo block triangle of a square BSRMatrix F in the factor format above.  sptrsv_cpu_bsr (host
// arrays) is the definition.  Block rows ascending for LOWER, descending for UPPER.  For r < size_I:
//   s_r = +0.0f; over the stored blocks J on the triangle's side of I in stored order, c = 0 .. b-1 with J*b + c < n:
//       s_r = fl(s_r + fl(F_IJ[r][c] * x[J*b + c]))                       (spmv_cpu_bsr's sum)
//   t_r = fl(b[I*b + r] - s_r)
//   NON_UNIT: x[I*b + r] = u after u = +0.0f; u = fl(u + fl(F_II[r][c] * t_c)), c = 0 .. r (LOWER), c = r .. size_I - 1
//             (UPPER);   UNIT: x = t, the diagonal block is not read
// Blocks on the other side of the diagonal are skipped, not an error.  d_b == d_x solves in place; any other overlap is
// INVALID_ARGUMENT.  Block columns are strictly ascending inside a block row (the container's rule).
// ordered = 1: one lane per block row, bit for bit sptrsv_cpu_bsr.  ordered = 0 (default): a group of 1 .. 64 lanes owns a
// block row, lane l takes the triangle's blocks l, l + LANES, ... with b fmaf accumulators, the sums fold in a fixed
// butterfly and one lane applies the diagonal step by the ordered rule: the same bits on every run and stream at a
// fixed lane count.
// Checks as sptrsv_csr's, on the block pattern: null -> INVALID_ARGUMENT; not square -> INVALID_DIMENSION; no rows ->
// SUCCESS; a bad shape or missing arrays -> INVALID_FORMAT; a bad config or a partial overlap -> INVALID_ARGUMENT;
// malformed pattern -> INVALID_FORMAT; NON_UNIT and a block row without a diagonal block, or whose block columns are
// not strictly ascending (the diagonal block is found by a binary search) -> INVALID_ARGUMENT.  UNIT solves take
// block rows in any order of columns: the triangle's blocks are picked by their block column.
// The schedule lives in the side table under the block row-pointer array: F shares it with A (analysis_ms == 0 on a
// second call and on F after A); bsr_free_gpu, a rebuild and bsr_invalidate_gpu_cache drop it.
int          sptrsv_cpu_bsr(const BSRMatrix* F, const float* b, float* x, const SpTRSVConfig* config = nullptr);
SpTRSVResult sptrsv_bsr(const BSRMatrix* F, const float* d_b, float* d_x, const SpTRSVConfig* config = nullptr);
int          sptrsv_bsr_async(const BSRMatrix* F, const float* d_b, float* d_x, const SpTRSVConfig* config,
                              hipStream_t stream);
// builds (or finds) the schedule of one triangle ahead of a timed call
SpTRSVResult sptrsv_analyze_bsr(const BSRMatrix* A, int uplo);

} // namespace spmv

#endif // SPMV_BSR_FACTOR_H
