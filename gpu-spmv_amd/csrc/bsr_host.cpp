// bsr_host.cpp — the host side of include/spmv/bsr.h: bsr_from_csr_cpu, bsr_to_csr_cpu and
// spmv_cpu_bsr, which define what the device routines in bsr.hip compute, and the argument checks of those device
// entry points, which need no device.
// Compiled with -ffp-contract=off: every product and every sum of spmv_cpu_bsr is a rounding of its own.
#include "bsr_impl.h"
#include "internal.h"

#include <climits>
#include <cstdint>
#include <cstring>
#include <vector>

namespace spmv {

namespace {

using detail::code;

// host arrays present, row pointers well formed, every column in [0, num_cols) and strictly ascending
bool host_csr_ok(const CSRMatrix* M) {
    if (M->num_rows < 0 || M->num_cols < 0 || M->nnz < 0 || !M->row_ptrs) return false;
    if (M->nnz > 0 && (!M->col_indices || !M->values)) return false;
    if (M->row_ptrs[0] != 0 || M->row_ptrs[M->num_rows] != M->nnz) return false;
    for (int i = 0; i < M->num_rows; ++i) {
        if (M->row_ptrs[i] > M->row_ptrs[i + 1]) return false;
    }
    for (int i = 0; i < M->num_rows; ++i) {
        for (int p = M->row_ptrs[i]; p < M->row_ptrs[i + 1]; ++p) {
            const int c = M->col_indices[p];
            if (c < 0 || c >= M->num_cols) return false;
            if (p > M->row_ptrs[i] && c <= M->col_indices[p - 1]) return false;
        }
    }
    return true;
}

bool host_bsr_ok(const BSRMatrix* B) {
    if (!detail::bsr::shape_ok(B) || !B->block_row_ptrs) return false;
    if (B->num_blocks > 0 && (!B->block_cols || !B->values)) return false;
    const int* rp = B->block_row_ptrs;
    if (rp[0] != 0 || rp[B->num_block_rows] != B->num_blocks) return false;
    for (int i = 0; i < B->num_block_rows; ++i) {
        if (rp[i] > rp[i + 1]) return false;
    }
    for (int i = 0; i < B->num_block_rows; ++i) {
        for (int p = rp[i]; p < rp[i + 1]; ++p) {
            const int c = B->block_cols[p];
            if (c < 0 || c >= B->num_block_cols) return false;
            if (p > rp[i] && c <= B->block_cols[p - 1]) return false;
        }
    }
    return true;
}

bool is_zero(float v) {
    uint32_t bits;
    std::memcpy(&bits, &v, sizeof(bits));
    return (bits & 0x7FFFFFFFu) == 0;
}

} // namespace

namespace detail {
namespace bsr {

bool shape_ok(const BSRMatrix* B) {
    if (!bsr_block_dim_supported(B->block_dim) || B->num_rows < 0 || B->num_cols < 0 || B->num_blocks < 0) return false;
    return B->num_block_rows == blocks_along(B->num_rows, B->block_dim) &&
           B->num_block_cols == blocks_along(B->num_cols, B->block_dim);
}

bool device_arrays_ok(const BSRMatrix* B) {
    if (!shape_ok(B) || !B->d_block_row_ptrs) return false;
    return B->num_blocks == 0 || (B->d_block_cols && B->d_values);
}

int from_csr_check(const BSRMatrix* B, const CSRMatrix* A, int block_dim) {
    if (!B || !A) return code(SpMVError::INVALID_ARGUMENT);
    if (!bsr_block_dim_supported(block_dim)) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    return 0;
}

int numeric_check(const BSRMatrix* B, const CSRMatrix* A) {
    if (!B || !A) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    if (B->num_rows != A->num_rows || B->num_cols != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (!device_arrays_ok(B)) return code(SpMVError::INVALID_FORMAT);
    return 0;
}

int to_csr_check(const CSRMatrix* A, const BSRMatrix* B) {
    if (!A || !B) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_ok(B)) return code(SpMVError::INVALID_FORMAT);
    return 0;
}

int spmv_check(const BSRMatrix* A, const float* d_x, const float* d_y, int vec_size, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_x || !d_y) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return code(SpMVError::SUCCESS);
    }
    if (vec_size >= 0 && !spmv_validate_dimensions(A->num_cols, vec_size)) return code(SpMVError::INVALID_DIMENSION);
    if (!device_arrays_ok(A)) return code(SpMVError::INVALID_FORMAT);
    return code(SpMVError::SUCCESS);
}

} // namespace bsr
} // namespace detail

int bsr_from_csr_cpu(BSRMatrix* B, const CSRMatrix* A, int block_dim) {
    if (!B || !A) return code(SpMVError::INVALID_ARGUMENT);
    if (!bsr_block_dim_supported(block_dim)) return code(SpMVError::INVALID_ARGUMENT);
    if (!host_csr_ok(A)) return code(SpMVError::INVALID_FORMAT);
    const int m = A->num_rows, b = block_dim;
    const int block_rows = detail::bsr::blocks_along(m, b);

    std::vector<int> block_row_ptrs(static_cast<size_t>(block_rows) + 1, 0);
    std::vector<int> block_cols;
    std::vector<float> values;
    for (int I = 0; I < block_rows; ++I) {
        const int r0 = I * b, rows_here = std::min(b, m - r0);
        int cursor[8], end[8];
        for (int k = 0; k < rows_here; ++k) {
            cursor[k] = A->row_ptrs[r0 + k];
            end[k] = A->row_ptrs[r0 + k + 1];
        }
        for (;;) {                                   // a b-way merge of the rows by block column
            int J = INT_MAX;
            for (int k = 0; k < rows_here; ++k) {
                if (cursor[k] < end[k]) J = std::min(J, A->col_indices[cursor[k]] / b);
            }
            if (J == INT_MAX) break;
            if (block_cols.size() == static_cast<size_t>(INT_MAX)) return code(SpMVError::INVALID_DIMENSION);
            const size_t base = values.size();
            block_cols.push_back(J);
            values.resize(base + static_cast<size_t>(b) * b, 0.0f);
            for (int k = 0; k < rows_here; ++k) {
                while (cursor[k] < end[k] && A->col_indices[cursor[k]] / b == J) {
                    values[base + static_cast<size_t>(k) * b + (A->col_indices[cursor[k]] - J * b)] = A->values[cursor[k]];
                    ++cursor[k];
                }
            }
        }
        block_row_ptrs[I + 1] = static_cast<int>(block_cols.size());
    }
    detail::bsr::adopt_host(B, m, A->num_cols, b, block_row_ptrs, block_cols, values);
    return code(SpMVError::SUCCESS);
}

int bsr_to_csr_cpu(CSRMatrix* A, const BSRMatrix* B, int keep_zeros) {
    if (!A || !B) return code(SpMVError::INVALID_ARGUMENT);
    if (!host_bsr_ok(B)) return code(SpMVError::INVALID_FORMAT);
    const int m = B->num_rows, n = B->num_cols, b = B->block_dim;

    std::vector<int> row_ptrs(static_cast<size_t>(m) + 1, 0);
    std::vector<int> cols;
    std::vector<float> vals;
    for (int i = 0; i < m; ++i) {
        const int I = i / b, r = i % b;
        for (int p = B->block_row_ptrs[I]; p < B->block_row_ptrs[I + 1]; ++p) {
            const int first = B->block_cols[p] * b;
            const float* line = B->values + (static_cast<size_t>(p) * b + r) * b;
            for (int c = 0; c < b && first + c < n; ++c) {
                if (!keep_zeros && is_zero(line[c])) continue;
                if (cols.size() == static_cast<size_t>(INT_MAX)) return code(SpMVError::INVALID_DIMENSION);
                cols.push_back(first + c);
                vals.push_back(line[c]);
            }
        }
        row_ptrs[i + 1] = static_cast<int>(cols.size());
    }
    detail::csr_adopt_host(A, m, n, row_ptrs, cols, vals);
    return code(SpMVError::SUCCESS);
}

void spmv_cpu_bsr(const BSRMatrix* A, const float* x, float* y) {
    const int b = A->block_dim, n = A->num_cols;
    for (int i = 0; i < A->num_rows; ++i) {
        const int I = i / b, r = i % b;
        float s = 0.0f;
        for (int p = A->block_row_ptrs[I]; p < A->block_row_ptrs[I + 1]; ++p) {
            const int first = A->block_cols[p] * b;
            const float* line = A->values + (static_cast<size_t>(p) * b + r) * b;
            for (int c = 0; c < b && first + c < n; ++c) {
                const float product = line[c] * x[first + c];
                s = s + product;
            }
        }
        y[i] = s;
    }
}

} // namespace spmv
