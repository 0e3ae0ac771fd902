// bsr_impl.h — what bsr.hip, bsr_host.cpp and bsr_matrix.cpp share (include/spmv/bsr.h): the
// hand-over of a built BSR matrix and the argument checks of the device entry points, which need no device and live
// in the host file.
#ifndef SPMV_AMD_BSR_IMPL_H
#define SPMV_AMD_BSR_IMPL_H

#include "spmv/bsr.h"

#include <vector>

namespace spmv {
namespace detail {
namespace bsr {

inline int blocks_along(int n, int block_dim) {
    return static_cast<int>((static_cast<long long>(n) + block_dim - 1) / block_dim);
}

// How a device builder hands B over (csr_adopt_device's rule): B's old device arrays are released, it owns the three
// hipMalloc'ed arrays from now on (d_block_cols and d_values may be null without blocks), and its host arrays are
// allocated at the new size without data.
void adopt_device(BSRMatrix* B, int rows, int cols, int block_dim, int num_blocks, int* d_block_row_ptrs,
                  int* d_block_cols, float* d_values);
// How the host twin hands B over (csr_adopt_host's rule): copied first, so a failed allocation leaves B untouched; a
// device copy, which would be stale, is freed.
void adopt_host(BSRMatrix* B, int rows, int cols, int block_dim, const std::vector<int>& block_row_ptrs,
                const std::vector<int>& block_cols, const std::vector<float>& values);

// checks 1 - 3 of bsr_from_csr_gpu (B may be null for csr_block_count_gpu, which passes a dummy)
int from_csr_check(const BSRMatrix* B, const CSRMatrix* A, int block_dim);
// the checks of bsr_from_csr_numeric before the device
int numeric_check(const BSRMatrix* B, const CSRMatrix* A);
// B's shape is one a BSR matrix can have: supported block_dim, no negative size, block counts that match
bool shape_ok(const BSRMatrix* B);
// shape_ok and the device arrays: the block row pointers always, the other two where there are blocks
bool device_arrays_ok(const BSRMatrix* B);
// the checks of bsr_to_csr_gpu before the device
int to_csr_check(const CSRMatrix* A, const BSRMatrix* B);
// front half of spmv_bsr / spmv_bsr_async (spmv_csr's order); SUCCESS when a launch should follow
int spmv_check(const BSRMatrix* A, const float* d_x, const float* d_y, int vec_size, bool* nothing_to_do);

} // namespace bsr
} // namespace detail
} // namespace spmv

#endif
