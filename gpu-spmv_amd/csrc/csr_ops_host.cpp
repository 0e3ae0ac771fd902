// csr_ops_host.cpp — the host side of include/spmv/csr_ops.h: csr_add_cpu, which defines the sum;
// the host twins of the scaling and of the diagonal in and out; and the argument checks of the device entry points in
// csr_ops.hip, which need no device.
// Compiled with -ffp-contract=off: every product and every sum is a rounding of its own.
#include "csr_ops_impl.h"
#include "internal.h"

#include <climits>
#include <cstdint>
#include <vector>

namespace spmv {

namespace {

using detail::code;

// host arrays present and row pointers well formed; every column in [0, num_cols), strictly ascending when asked
bool host_matrix_ok(const CSRMatrix* M, bool ascending) {
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
            if (ascending && p > M->row_ptrs[i] && c <= M->col_indices[p - 1]) return false;
        }
    }
    return true;
}

bool ranges_overlap(const float* a, long long na, const float* b, long long nb) {
    if (!a || !b || na <= 0 || nb <= 0) return false;
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) * sizeof(float) && b0 < a0 + static_cast<uintptr_t>(na) * sizeof(float);
}

} // namespace

namespace detail {
namespace csr_ops {

int add_check(const CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B, bool refill) {
    if (!C || !A || !B) return code(SpMVError::INVALID_ARGUMENT);
    if (C == A || C == B) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != B->num_rows || A->num_cols != B->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (!device_arrays_lenient(A) || !device_arrays_lenient(B)) return code(SpMVError::INVALID_FORMAT);
    if (refill) {
        if (C->num_rows != A->num_rows || C->num_cols != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
        if (!device_arrays_lenient(C)) return code(SpMVError::INVALID_FORMAT);
    }
    return 0;
}

int scale_check(const CSRMatrix* A, const float* d_row_scale, const float* d_col_scale, float* d_values_out,
                float** out, bool* in_place) {
    if (!A) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    *out = d_values_out ? d_values_out : A->d_values;
    *in_place = *out == A->d_values;
    if (!*in_place && ranges_overlap(*out, A->nnz, A->d_values, A->nnz)) return code(SpMVError::INVALID_ARGUMENT);
    if (ranges_overlap(*out, A->nnz, d_row_scale, A->num_rows) || ranges_overlap(*out, A->nnz, d_col_scale, A->num_cols)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    return 0;
}

int diagonal_check(const CSRMatrix* A, const float* d_diag) {
    if (!A || (!d_diag && A->num_rows > 0)) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    return 0;
}

int diag_matrix_check(const CSRMatrix* D, int n) {
    if (!D) return code(SpMVError::INVALID_ARGUMENT);
    if (n < 0) return code(SpMVError::INVALID_DIMENSION);
    return 0;
}

} // namespace csr_ops
} // namespace detail

int csr_add_cpu(CSRMatrix* C, float alpha, const CSRMatrix* A, float beta, const CSRMatrix* B) {
    if (!C || !A || !B) return code(SpMVError::INVALID_ARGUMENT);
    if (C == A || C == B) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != B->num_rows || A->num_cols != B->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (!host_matrix_ok(A, true) || !host_matrix_ok(B, true)) return code(SpMVError::INVALID_FORMAT);
    const int m = A->num_rows, n = A->num_cols;

    std::vector<int> row_ptrs(static_cast<size_t>(m) + 1, 0);
    std::vector<int> cols;
    std::vector<float> vals;
    for (int i = 0; i < m; ++i) {
        int p = A->row_ptrs[i], q = B->row_ptrs[i];
        const int p_end = A->row_ptrs[i + 1], q_end = B->row_ptrs[i + 1];
        while (p < p_end || q < q_end) {
            if (cols.size() == static_cast<size_t>(INT_MAX)) return code(SpMVError::INVALID_DIMENSION);
            const bool take_a = p < p_end && (q == q_end || A->col_indices[p] <= B->col_indices[q]);
            const bool take_b = q < q_end && (p == p_end || B->col_indices[q] <= A->col_indices[p]);
            float v;
            if (take_a && take_b) {
                const float left = alpha * A->values[p];
                const float right = beta * B->values[q];
                v = left + right;
            } else if (take_a) {
                v = alpha * A->values[p];
            } else {
                v = beta * B->values[q];
            }
            cols.push_back(take_a ? A->col_indices[p] : B->col_indices[q]);
            vals.push_back(v);
            p += take_a;
            q += take_b;
        }
        row_ptrs[i + 1] = static_cast<int>(cols.size());
    }
    detail::csr_adopt_host(C, m, n, row_ptrs, cols, vals);
    return code(SpMVError::SUCCESS);
}

int csr_scale_cpu(const CSRMatrix* A, const float* row_scale, const float* col_scale, float* values_out) {
    if (!A || (!values_out && A->nnz > 0)) return code(SpMVError::INVALID_ARGUMENT);
    if (!host_matrix_ok(A, false)) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < A->num_rows; ++i) {
        for (int p = A->row_ptrs[i]; p < A->row_ptrs[i + 1]; ++p) {
            const float a = A->values[p];
            float v = a;
            if (row_scale && col_scale) {
                const float both = row_scale[i] * col_scale[A->col_indices[p]];
                v = a * both;
            } else if (row_scale) {
                v = a * row_scale[i];
            } else if (col_scale) {
                v = a * col_scale[A->col_indices[p]];
            }
            values_out[p] = v;
        }
    }
    return code(SpMVError::SUCCESS);
}

int csr_diagonal_cpu(const CSRMatrix* A, float* diag) {
    if (!A || (!diag && A->num_rows > 0)) return code(SpMVError::INVALID_ARGUMENT);
    if (!host_matrix_ok(A, false)) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < A->num_rows; ++i) {
        float d = 0.0f;
        for (int p = A->row_ptrs[i]; p < A->row_ptrs[i + 1]; ++p) {
            if (A->col_indices[p] == i) d = d + A->values[p];
        }
        diag[i] = d;
    }
    return code(SpMVError::SUCCESS);
}

int csr_diag_matrix_cpu(CSRMatrix* D, int n, const float* diag) {
    const int status = detail::csr_ops::diag_matrix_check(D, n);
    if (status != 0) return status;
    std::vector<int> row_ptrs(static_cast<size_t>(n) + 1), cols(static_cast<size_t>(n));
    std::vector<float> vals(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        row_ptrs[i] = i;
        cols[i] = i;
        vals[i] = diag ? diag[i] : 1.0f;
    }
    row_ptrs[n] = n;
    detail::csr_adopt_host(D, n, n, row_ptrs, cols, vals);
    return code(SpMVError::SUCCESS);
}

} // namespace spmv
