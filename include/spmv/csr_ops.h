// spmv/csr_ops.h — CSR algebra on the device and on the host, bit for bit the same: the weighted sum of two matrices
// C = alpha*A + beta*B with a values-only refill, row / column scaling, and the diagonal in and out (kernels in
// gpu-spmv_amd/csrc/csr_ops.hip, host twins and argument checks in csr_ops_host.cpp; the recipes —
// M + dt*K, A - sigma*I, L = D - A, (A + A^T)/2, D^-1/2 A D^-1/2 — are in INTEGRATION.md).
//
// Everything is fp32 values and int32 indices.
//
// The sum (csr_add_cpu is its definition): A and B are m×n with columns STRICTLY ASCENDING inside every row of both.
// Row i of C is the two-pointer merge of the two rows: columns ascending, one entry per column of the union, with
//     column in A only      fl(alpha * a)
//     column in B only      fl(beta * b)
//     column in both        fl(fl(alpha * a) + fl(beta * b))
// every product and the sum rounded to fp32 on its own (no FMA).  The pattern is ALWAYS the union: an entry that
// cancels to 0.0f is kept, so are explicit zeros, and alpha = 0 or beta = 0 removes nothing (0 * Inf gives the NaN the
// rule says).  NaN, ±Inf, -0.0f and denormals follow IEEE and are not flushed.  A and B may be the same matrix; C may
// be neither.
// Rows that are unsorted or repeat a column (files loaded by the reference's containers may hold such rows) are
// INVALID_FORMAT here: csr_row_indices_gpu + csr_from_coo_gpu (spmv/assemble.h) normalise a matrix first.
#ifndef SPMV_CSR_OPS_H
#define SPMV_CSR_OPS_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct CsrAddResult {
    int   error_code;     // SpMVError as int
    int   nnz;            // entries of C
    int   common;         // columns found in both matrices, summed over the rows
    int   max_row_nnz;    // longest row of C
    int   lanes;          // lanes that share one row
    int   launches;       // kernel launches of the call
    float symbolic_ms;    // device-event time of the counting pass and the scan (0 for csr_add_numeric)
    float numeric_ms;     // device-event time of the numeric pass
    CsrAddResult() : error_code(0), nnz(0), common(0), max_row_nnz(0), lanes(0), launches(0), symbolic_ms(0.0f),
                     numeric_ms(0.0f) {}
};

// The sum on HOST arrays, by the rule above.
// Checks, in this order, C untouched when one fails: null C / A / B -> INVALID_ARGUMENT; C is A or B ->
// INVALID_ARGUMENT; rows or columns of A and B differ -> INVALID_DIMENSION; missing host arrays, row pointers that do
// not start at 0, decrease or do not end at nnz, a column outside [0, n) or not strictly above its left neighbour ->
// INVALID_FORMAT; more than INT_MAX entries in C -> INVALID_DIMENSION.  On SUCCESS C gets new host arrays
// (owns_host_memory); its device arrays, which would be stale, are freed.
int csr_add_cpu(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B);

// The sum of two device-resident matrices (csr_to_gpu / csr_wrap_device; the arrays may be views at any 4-byte
// offset).  C is left exactly as csr_transpose_gpu and spgemm_csr leave theirs: it owns new device arrays, its host
// arrays are allocated at the new size and hold no data until csr_from_gpu(C); what C owned before is released.  Runs
// on the library stream (spmv_set_stream) and returns after completion, all scratch freed.
//
// Two passes, no sort, no hash table, no atomics, no workgroup waits for another: a group of `lanes` lanes owns a row.
// The counting pass strides over both rows, checks them, looks every entry of A up in B's row and counts
// len(A) + len(B) - matches; an exclusive scan turns the counts into row pointers.  The numeric pass is a merge by
// rank: entry i_a of A with column c goes to slot i_a + lower_bound_B(c) - (matched entries of A before i_a), an
// unmatched entry j_b of B to j_b + lower_bound_A(c) - (matched entries of B before j_b).  Every slot has one writer
// and its value does not depend on the lane count, so the bits are csr_add_cpu's at every lane count.  A row of any
// length is handled by the same loop; a row much longer than the mean is walked by a whole wavefront instead of its
// group, in the same launch.
//
// Checks, in this order, C untouched by every failure:
//   1. null C / A / B -> INVALID_ARGUMENT
//   2. C is A or B -> INVALID_ARGUMENT
//   3. rows or columns of A and B differ -> INVALID_DIMENSION
//   4. missing device arrays (the rule of csr_transpose_gpu) -> INVALID_FORMAT
//   5. on the device, by the counting pass, read back before C is allocated: row pointers of both start at 0, do not
//      decrease and end at nnz; every column in [0, n) and strictly above its left neighbour -> INVALID_FORMAT
//   6. nnz(C) > INT_MAX (row counts are summed in 64 bits) -> INVALID_DIMENSION
//   7. allocation failure -> CUDA_MALLOC, nothing leaked
// m == 0, n == 0 or two empty matrices give a valid C with nnz = 0.
// result (may be null) receives the statistics; the return value equals result->error_code.
int csr_add(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B,
            CsrAddResult* result = nullptr);

// Recomputes only C->d_values into the pattern an earlier csr_add made from matrices of the same structure: a new dt
// or sigma, or new values after csr_coo_refill.  One kernel and no allocation beyond a flag word: the numeric pass
// with every slot compared with C's column instead of written.  Checks 1 - 4 as above, then C must be m×n
// (INVALID_DIMENSION) and have device arrays (INVALID_FORMAT); the kernel validates A and B as check 5 does and
// requires every row of C to be exactly the union of the two rows, the same count and the same columns:
// INVALID_FORMAT otherwise, with C's values unspecified.  C's structure arrays are never written.  On success
// csr_invalidate_gpu_cache(C) is called, as csr_coo_refill does: a tiled plan, a transpose or a level schedule that
// holds the old values never serves another call.  result receives nnz (C's), lanes, launches (1) and numeric_ms;
// common, max_row_nnz and symbolic_ms stay 0.
int csr_add_numeric(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B,
                    CsrAddResult* result = nullptr);

// Scaling: out[p] = fl(a[p] * fl(r[i] * c[col[p]])) for entry p of row i; with one scale null fl(a * r[i]) or
// fl(a * c[j]); with both null a copy.  The two scales are folded FIRST on purpose: with r == c and a symmetric A the
// result is symmetric bit for bit (fl(r_i * r_j) commutes), so D^-1/2 A D^-1/2 stays a matrix cg_solve and ic0_csr
// may take.  Note that r_i * c_j may overflow or underflow on its own where a * r_i * c_j would not.
// d_row_scale: num_rows floats, d_col_scale: num_cols floats, d_values_out: nnz floats (for instance the value array
// of another header over the same structure).  d_values_out null or equal to A->d_values is the in-place case, which
// ends with csr_invalidate_gpu_cache(A).
// Checks, in this order: null A -> INVALID_ARGUMENT; missing device arrays -> INVALID_FORMAT; the output overlaps the
// values without being the values, or overlaps either scale vector -> INVALID_ARGUMENT; then A's structure on the
// device by csr_transpose_gpu's rule -> INVALID_FORMAT, before anything is written.  One launch on the library stream,
// waited for.
int csr_scale_gpu(CSRMatrix* A, const float* d_row_scale, const float* d_col_scale, float* d_values_out);
// The same on host arrays; values_out (nnz floats, may be A->values) must not be null when A has entries.
// Checks: null A, or null values_out with nnz > 0 -> INVALID_ARGUMENT; missing host arrays or a malformed structure
// (csr_transpose_gpu's rule: sorted rows are not required) -> INVALID_FORMAT.
int csr_scale_cpu(const CSRMatrix* A, const float* row_scale, const float* col_scale, float* values_out);

// d_diag[i] = the fp32 sum, from +0.0f and in storage order, of row i's stored (i, i) entries: what the solvers'
// Jacobi set-up computes, without an acceptance rule.  0.0f where the row stores none; A need not be square (rows
// past num_cols get 0).  d_diag: num_rows floats.
// Checks, in this order: null A, or null d_diag with num_rows > 0 -> INVALID_ARGUMENT; missing device arrays ->
// INVALID_FORMAT; A's structure on the device (csr_transpose_gpu's rule) -> INVALID_FORMAT, before d_diag is written.
int csr_diagonal_gpu(const CSRMatrix* A, float* d_diag);
int csr_diagonal_cpu(const CSRMatrix* A, float* diag);

// D = the n×n diagonal matrix of d_diag (n floats): row_ptrs 0 .. n, column i in row i, value d_diag[i], or 1.0f when
// d_diag is null (the identity).  Zeros are kept.  D is left as csr_add leaves C.
// Checks, in this order: null D -> INVALID_ARGUMENT; negative n -> INVALID_DIMENSION; allocation failure ->
// CUDA_MALLOC.
int csr_diag_matrix_gpu(CSRMatrix* D, int n, const float* d_diag);
// The same on the host: D gets new host arrays, its device arrays (stale) are freed.
int csr_diag_matrix_cpu(CSRMatrix* D, int n, const float* diag);

} // namespace spmv

#endif
