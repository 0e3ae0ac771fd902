// bsr_diag_host.cpp — the host side of the block-Jacobi part of include/spmv/bsr.h:
// bsr_diag_inverse_cpu and bsr_diag_apply_cpu, which define what the device routines in cg_bsr.hip compute, and the
// argument checks of those device entry points and of cg_solve_bsr, which need no device.
// Compiled with -ffp-contract=off: every product and every sum of bsr_diag_impl.h is a rounding of its own.
#include "bsr_diag_impl.h"
#include "bsr_impl.h"
#include "internal.h"

#include <cstdint>

namespace spmv {

namespace detail {
namespace bsr {

int diag_check(const BSRMatrix* A, const void* out, bool device) {
    if (!A || !out) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (device) return device_arrays_ok(A) ? 0 : code(SpMVError::INVALID_FORMAT);
    if (!shape_ok(A) || !A->block_row_ptrs) return code(SpMVError::INVALID_FORMAT);
    if (A->num_blocks > 0 && (!A->block_cols || !A->values)) return code(SpMVError::INVALID_FORMAT);
    return 0;
}

int cg_check(const BSRMatrix* A, const float* d_b, const float* d_x, const CGConfig& cfg, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_b || !d_x) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return 0;
    }
    if (!device_arrays_ok(A)) return code(SpMVError::INVALID_FORMAT);
    if (!(cfg.tolerance >= 0.0f) || cfg.max_iterations < 0 ||
        (cfg.preconditioner != CGConfig::NONE && cfg.preconditioner != CGConfig::JACOBI &&
         cfg.preconditioner != CGConfig::BLOCK_JACOBI) ||
        cfg.engine < -1 || cfg.engine > 0) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const uintptr_t b0 = reinterpret_cast<uintptr_t>(d_b), x0 = reinterpret_cast<uintptr_t>(d_x);
    const uintptr_t bytes = static_cast<uintptr_t>(A->num_rows) * sizeof(float);
    if (b0 < x0 + bytes && x0 < b0 + bytes) return code(SpMVError::INVALID_ARGUMENT);
    return 0;
}

} // namespace bsr
} // namespace detail

namespace {

template <int B>
int inverse_cpu(const BSRMatrix* A, float* inv) {
    const int n = A->num_rows;
    for (int I = 0; I < A->num_block_rows; ++I) {
        const int at = detail::bsr::find_block(A->block_cols, A->block_row_ptrs[I], A->block_row_ptrs[I + 1], I);
        if (at < 0) return detail::code(SpMVError::INVALID_ARGUMENT);
        const int size = n - I * B < B ? n - I * B : B;
        if (!detail::bsr::diag_block_inverse<B>(A->values + static_cast<size_t>(at) * B * B, size,
                                                inv + static_cast<size_t>(I) * B * B)) {
            return detail::code(SpMVError::INVALID_ARGUMENT);
        }
    }
    return 0;
}

template <int B>
void apply_cpu(int n, const float* inv, const float* r, float* z) {
    for (int i = 0; i < n; ++i) {
        const long long first = static_cast<long long>(i / B) * B;
        z[i] = detail::bsr::diag_apply_row<B>(inv + static_cast<size_t>(i) * B, r + first, first, n);
    }
}

} // namespace

int bsr_diag_inverse_cpu(const BSRMatrix* A, float* inv) {
    const int status = detail::bsr::diag_check(A, inv, false);
    if (status != 0) return status;
    switch (A->block_dim) {
        case 2:  return inverse_cpu<2>(A, inv);
        case 3:  return inverse_cpu<3>(A, inv);
        case 4:  return inverse_cpu<4>(A, inv);
        default: return inverse_cpu<8>(A, inv);
    }
}

void bsr_diag_apply_cpu(const BSRMatrix* A, const float* inv, const float* r, float* z) {
    switch (A->block_dim) {
        case 2:  return apply_cpu<2>(A->num_rows, inv, r, z);
        case 3:  return apply_cpu<3>(A->num_rows, inv, r, z);
        case 4:  return apply_cpu<4>(A->num_rows, inv, r, z);
        default: return apply_cpu<8>(A->num_rows, inv, r, z);
    }
}

} // namespace spmv
