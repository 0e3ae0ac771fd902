// spmv/fsai.h — factorised sparse approximate inverse (FSAI, Kolotilina-Yeremin) of a square SPD CSR matrix on the
// device.
//
// G is sparse and lower triangular with G ~ L^-1 for A = L L^T, so M^-1 = G^T G and the preconditioner is APPLIED by
// two SpMVs: z = G^T (G r) (cg_solve_fsai, spmv/cg.h).  Every row of G comes from one small dense SPD system and is
// independent of every other row: no level schedule, no waiting between workgroups (kernels in
// gpu-spmv_amd/csrc/fsai.hip).
#ifndef SPMV_FSAI_H
#define SPMV_FSAI_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

constexpr int kFsaiMaxRow = 64;       // the longest pattern row fsai_csr takes

struct FSAIResult {
    int   error_code;      // SpMVError as int
    int   nnz;             // stored entries of G
    int   max_row;         // longest pattern row (entries on or left of the diagonal)
    int   row_class;       // capacity class the kernel ran at: 4, 8, 16, 32 or 64 (>= max_row)
    int   lanes_per_row;   // lanes that shared a row
    int   bad_row;         // lowest row whose finished g_ii is not > 0 or not finite; -1 when none
    int   long_row;        // lowest row with more than 64 pattern entries; -1 when none
    float elapsed_ms;      // device-event time of structure build + numeric kernel
    FSAIResult() : error_code(0), nnz(0), max_row(0), row_class(0), lanes_per_row(0), bad_row(-1), long_row(-1),
                   elapsed_ms(0.0f) {}
};

// G = FSAI of the square matrix A (resident on the device, rows strictly ascending) on the pattern of S (nullptr: A).
// Only the values on and left of A's diagonal are read (A is taken to be symmetric, as in ic0_csr); A need not be
// structurally symmetric.  Only S's structure arrays are read, a stored zero counts: row i of G has exactly the columns
// j <= i stored in row i of S.  S = spgemm_csr(A, A) is the documented way to a stronger G.
//
// G comes back as csr_transpose_gpu and spgemm_csr leave their outputs: it owns new device arrays, its host arrays are
// allocated at the new size and hold no data until csr_from_gpu(G).  It is n x n, lower triangular, rows sorted, the
// diagonal stored last in each row.
//
// Arithmetic (fsai_cpu_csr below is its definition; every fp64 operation is rounded separately).  For row i let
// P = (j_1 < ... < j_m = i) be its pattern and M = A[P,P] in fp64: M_pq for q <= p is the stored (j_p, j_q) of A,
// +0.0 where it is not stored.
//   1. Cholesky C C^T = M: for q = 1..m and p = q..m: w = M_pq; for k = 1..q-1 ascending w = fma(-c_pk, c_qk, w);
//      c_qq = sqrt(w); c_pq = w / c_qq for p > q.
//   2. u = C^-T e_m: u_m = 1 / c_mm; for p = m-1 down to 1: t = +0.0; for q = m down to p+1 t = fma(c_qp, u_q, t);
//      u_p = (-t) / c_pp.
//   3. g_{i,j_p} = (float) u_p, one rounding to nearest.
// G A G^T then has a unit diagonal.  Every entry has a fixed operation sequence, so the result does not depend on how
// many lanes share a row or on the capacity class: the device G equals fsai_cpu_csr's G bit for bit at every lane count
// and every row class.
//
// A non-positive or non-finite pivot is not an error: the IEEE results propagate, error_code stays SUCCESS and bad_row
// reports the lowest affected row (an integer minimum over a scan of G's diagonal: deterministic).
//
// Checks, in this order; G is untouched when one fails:
//   null G or A -> INVALID_ARGUMENT; G == A or G == S -> INVALID_ARGUMENT; A not square -> INVALID_DIMENSION; S not
//   square or of another size than A -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS with an empty G; missing device
//   arrays of A or S -> INVALID_FORMAT; then the device validation, read back once together with G's entry count:
//   row_ptrs not monotone or outside [0, nnz], or a column outside [0, n), in A or S -> INVALID_FORMAT; a row of A or S
//   not strictly ascending -> INVALID_ARGUMENT; a row of S without a stored diagonal -> INVALID_ARGUMENT; a pattern row
//   longer than 64 -> INVALID_ARGUMENT with long_row set.
//
// The kernel: one group of 1, 2, ... or 64 lanes per row, M and C packed lower triangular in LDS.  row_class (4, 8, 16,
// 32 or 64) sizes the LDS slab; it is chosen once per call from max_row.  SPMV_DEBUG=fsai_lanes=N,fsai_class=C forces
// either; a forced class below max_row is INVALID_ARGUMENT.  Runs on spmv_get_stream() and returns after G is complete.
FSAIResult fsai_csr(CSRMatrix* G, const CSRMatrix* A, const CSRMatrix* S = nullptr);

// G's values again from a new A on G's existing pattern (G as fsai_csr left it): the refill step of a time-stepping
// loop, next to csr_coo_refill and amg_update.  Allocates nothing and reads nothing back except the bad_row scan; the
// bits equal those of a fresh fsai_csr on the same pattern.  Checks: null G or A, G == A -> INVALID_ARGUMENT; A or G
// not square, or G of another size than A -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS; missing device arrays ->
// INVALID_FORMAT.  The structure of A and G is not validated again: arrays rewritten since fsai_csr give wrong numbers,
// never an access outside them.
FSAIResult fsai_csr_numeric(CSRMatrix* G, const CSRMatrix* A);

// The same operation on HOST arrays, the definition of the arithmetic above.  G gets new host arrays (its device arrays,
// if any, are freed).  *bad_row (may be null) as FSAIResult::bad_row.  Returns the error code of the checks above, with
// "host arrays" for "device arrays"; G is untouched on any error.
int fsai_cpu_csr(CSRMatrix* G, const CSRMatrix* A, const CSRMatrix* S, int* bad_row);

} // namespace spmv

#endif
