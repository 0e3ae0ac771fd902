// csr_ops_impl.h — what csr_ops.hip and csr_ops_host.cpp share (include/spmv/csr_ops.h): the
// argument checks of the device entry points, which need no device and live in the host file.
#ifndef SPMV_AMD_CSR_OPS_IMPL_H
#define SPMV_AMD_CSR_OPS_IMPL_H

#include "spmv/csr_ops.h"

namespace spmv {
namespace detail {
namespace csr_ops {

// checks 1 - 4 of csr_add; with `refill` also C's shape (INVALID_DIMENSION) and device arrays (INVALID_FORMAT)
int add_check(const CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, bool refill);
// the checks of csr_scale_gpu before the device; *out = the array the call writes, *in_place = that is A->d_values
int scale_check(const CSRMatrix* A, const float* d_row_scale, const float* d_col_scale, float* d_values_out,
                float** out, bool* in_place);
int diagonal_check(const CSRMatrix* A, const float* d_diag);
int diag_matrix_check(const CSRMatrix* D, int n);

} // namespace csr_ops
} // namespace detail
} // namespace spmv

#endif
