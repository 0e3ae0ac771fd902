// spmv/spgemm.h — sparse matrix-matrix product C = A·B of two CSR matrices, on the device and on the host, bit for bit
// the same (kernels in gpu-spmv_amd/csrc/spgemm.hip, the host routine in spgemm_host.cpp).
//
// Arithmetic (spgemm_cpu_csr is its definition): fp32 values, int32 indices, A m×k, B k×n, C m×n.  For row i the
// accumulators start at +0.0f; A's entries p = row_ptrs[i] .. row_ptrs[i+1]-1 are walked in storage order, and for
// each p B's row col_A[p] is walked in storage order with
//     acc[col_B[q]] = acc[col_B[q]] + (val_A[p] * val_B[q])
// the product and the sum each rounded to fp32 (no FMA), the rule of spmv_cpu_csr.  Row i of C holds every column
// that was touched at least once, in ascending order: an entry that cancels to 0.0f, or whose factors are explicit
// zeros, is kept (the pattern is the symbolic product).  A may have unsorted rows and duplicate entries, which are
// just further steps of the walk; B's columns must be strictly ascending inside each row (INVALID_FORMAT otherwise):
// the lanes that share a row of C then never meet in one accumulator within a step, and the device order is the host
// order without any ordering machinery.
#ifndef SPMV_SPGEMM_H
#define SPMV_SPGEMM_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct SpGEMMResult {
    int       error_code;        // SpMVError as int
    int       nnz;               // entries of C
    long long products;          // sum over A's entries of the length of the B row they point at
    int       max_row_products;  // clamped to INT_MAX
    int       max_row_nnz;
    int       symbolic_rows[8];  // rows per accumulator class in the symbolic pass ([0] = rows without products)
    int       numeric_rows[8];   // the same for the numeric pass
    int       lanes;             // lanes that share one row of C (classes of many tables per workgroup)
    float     symbolic_ms;       // device-event times; validation and allocation are outside both
    float     numeric_ms;
    SpGEMMResult() : error_code(0), nnz(0), products(0), max_row_products(0), max_row_nnz(0), symbolic_rows{},
                     numeric_rows{}, lanes(0), symbolic_ms(0.0f), numeric_ms(0.0f) {}
};

// The product on HOST arrays, in the order above (Gustavson's algorithm, a dense accumulator and a touched list).
// Checks, in this order: null C / A / B -> INVALID_ARGUMENT; C is A or B -> INVALID_ARGUMENT; A.num_cols !=
// B.num_rows -> INVALID_DIMENSION; missing host arrays, row pointers that do not start at 0, decrease or do not end
// at nnz, a column of A outside [0, B.num_rows), a column of B outside [0, B.num_cols) or not strictly above its left
// neighbour -> INVALID_FORMAT; more than INT_MAX entries in C -> INVALID_DIMENSION.  C is untouched on any error.  On
// SUCCESS C gets new host arrays (owns_host_memory); its device arrays, which would be stale, are freed.
int spgemm_cpu_csr(CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B);

// The product of two device-resident matrices (csr_to_gpu / csr_wrap_device).  C is left exactly as
// csr_transpose_gpu leaves AT: it owns new device arrays, its host arrays are allocated at the new size and hold no
// data until csr_from_gpu(C); what C owned before is released.  Runs on the library stream (spmv_set_stream) and
// returns after completion, all scratch freed.
// Checks, in this order: null C / A / B -> INVALID_ARGUMENT; C is A or B -> INVALID_ARGUMENT; A.num_cols !=
// B.num_rows -> INVALID_DIMENSION; missing device arrays (the rule of csr_transpose_gpu) -> INVALID_FORMAT; then ONE
// device pass over both matrices (row pointers start at 0, do not decrease and end at nnz; A's columns in
// [0, B.num_rows); B's columns in [0, B.num_cols) and strictly ascending in each row) -> INVALID_FORMAT, read before
// anything is allocated; after the symbolic pass nnz(C) > INT_MAX -> INVALID_DIMENSION (row counts are summed in 64
// bits); allocation failure -> CUDA_MALLOC, nothing leaked.  C is untouched by every failure.
// m == 0, n == 0 or no products at all give a valid C with nnz = 0 and all row pointers zero.
// result (may be null) receives the statistics; the return value equals result->error_code.
int spgemm_csr(CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, SpGEMMResult* result = nullptr);

// Recomputes only C->d_values into the pattern an earlier spgemm_csr produced from matrices of the same structure
// (a Galerkin product or A^T A whose values changed).  Validates A and B as above, and C's structure arrays the same
// way; then every row of C must have exactly the row's distinct-column count and each of its columns must have been
// produced: INVALID_FORMAT otherwise, with C's values unspecified.  C's dimensions must be A.num_rows x B.num_cols
// (INVALID_DIMENSION).  C's structure arrays are never written.
int spgemm_csr_numeric(CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, SpGEMMResult* result = nullptr);

// Most distinct columns a row may have in accumulator class cls (1-based): the LDS hash tables in growing size, then
// INT_MAX for the dense class, -1 past it (and for cls < 1).  Tests derive their shapes from it.
int spgemm_class_capacity(int cls);

} // namespace spmv

#endif
