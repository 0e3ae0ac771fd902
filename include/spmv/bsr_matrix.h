// spmv/bsr_matrix.h — block CSR (BSR) container: square b×b blocks, host arrays + device mirrors in HBM (extension;
// conversions and SpMV in spmv/bsr.h).
//
// Layout (the array triple rocSPARSE's bsrmv takes, row-major blocks):
//   * blocks are stored by block row; inside a block row the block columns are STRICTLY ASCENDING;
//   * block p holds b*b floats, row-major: position (r, c) of block p is values[(p*b + r)*b + c];
//   * offsets into values are 64-bit everywhere (num_blocks * b * b may pass 2^31);
//   * when num_rows or num_cols is not a multiple of b, the positions of the last block row / block column that
//     fall outside the matrix always hold +0.0f and are never used (not multiplied, not converted back).
// block_dim is 2, 3, 4 or 8.  sizeof(BSRMatrix) == 80.
#ifndef SPMV_BSR_MATRIX_H
#define SPMV_BSR_MATRIX_H

#include "common.h"

namespace spmv {

struct BSRMatrix {
    int num_rows;          // of the scalar matrix
    int num_cols;
    int block_dim;         // b
    int num_block_rows;    // ceil(num_rows / b)
    int num_block_cols;    // ceil(num_cols / b)
    int num_blocks;

    // host arrays (new[]-owned when owns_host_memory)
    float* values;           // [num_blocks * b * b]
    int*   block_cols;       // [num_blocks], ascending inside a block row
    int*   block_row_ptrs;   // [num_block_rows + 1]

    // device arrays (hipMalloc-owned when owns_device_memory)
    float* d_values;
    int*   d_block_cols;
    int*   d_block_row_ptrs;

    bool owns_host_memory;
    bool owns_device_memory;
};

inline bool bsr_block_dim_supported(int block_dim) {
    return block_dim == 2 || block_dim == 3 || block_dim == 4 || block_dim == 8;
}

// Zero-filled host arrays, no device arrays.  nullptr on a negative size or an unsupported block_dim.
BSRMatrix* bsr_create(int rows, int cols, int block_dim, int num_blocks);
void bsr_destroy(BSRMatrix* mat);

int bsr_to_gpu(BSRMatrix* mat);     // (re)uploads the host arrays to HBM; the matrix owns the device arrays
int bsr_from_gpu(BSRMatrix* mat);   // downloads the device arrays into the host arrays
void bsr_free_gpu(BSRMatrix* mat);
// A header over device arrays the caller owns (no host arrays, nothing owned), like the C ABI's csr_wrap_device; the
// arrays may be views at any 4-byte offset.  nullptr on a negative size or an unsupported block_dim.  bsr_destroy
// frees the header only.
BSRMatrix* bsr_wrap_device(int rows, int cols, int block_dim, int num_blocks, const int* d_block_row_ptrs,
                           const int* d_block_cols, const float* d_values);
// After writing into the device arrays in place (bsr_from_csr_numeric calls it): drops what the library keeps per BSR
// matrix in its side table under d_block_row_ptrs, the level schedules of the block pattern (sptrsv_bsr, bsr_ic0,
// cg_solve_bsr_ic; spmv/bsr_factor.h), which every matrix over the same structure arrays shares.  bsr_free_gpu and every
// rebuild into an existing matrix drop them too: the CSR rules.
void bsr_invalidate_gpu_cache(const BSRMatrix* mat);

} // namespace spmv

#endif // SPMV_BSR_MATRIX_H
