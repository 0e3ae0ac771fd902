// spgemm_host.cpp — the host side of C = A·B (include/spmv/spgemm.h): spgemm_cpu_csr, which defines
// the arithmetic and the pattern, and the table of accumulator classes the device passes and the tests share.
// Compiled with -ffp-contract=off: the product and the sum are two roundings, as in spmv_cpu_csr.
#include "internal.h"
#include "spmv/spgemm.h"

#include <algorithm>
#include <climits>
#include <vector>

namespace spmv {

int spgemm_class_capacity(int cls) {
    if (cls < 1 || cls > detail::kSpgemmClasses) return -1;
    if (cls == detail::kSpgemmClasses) return INT_MAX;
    return detail::kSpgemmSlots[cls - 1] / 2;         // load factor 1/2
}

namespace {

// host arrays present and row pointers well formed; every column in [0, limit), strictly ascending when asked
bool host_matrix_ok(const CSRMatrix* M, int limit, bool ascending) {
    if (M->num_rows < 0 || M->num_cols < 0 || M->nnz < 0 || !M->row_ptrs) return false;
    if (M->nnz > 0 && (!M->col_indices || !M->values)) return false;
    if (M->row_ptrs[0] != 0 || M->row_ptrs[M->num_rows] != M->nnz) return false;
    for (int i = 0; i < M->num_rows; ++i) {
        if (M->row_ptrs[i] > M->row_ptrs[i + 1]) return false;
    }
    for (int i = 0; i < M->num_rows; ++i) {
        for (int p = M->row_ptrs[i]; p < M->row_ptrs[i + 1]; ++p) {
            const int c = M->col_indices[p];
            if (c < 0 || c >= limit) return false;
            if (ascending && p > M->row_ptrs[i] && c <= M->col_indices[p - 1]) return false;
        }
    }
    return true;
}

} // namespace

int spgemm_cpu_csr(CSRMatrix* C, const CSRMatrix* A, const CSRMatrix* B) {
    using detail::code;
    if (!C || !A || !B) return code(SpMVError::INVALID_ARGUMENT);
    if (C == A || C == B) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_cols != B->num_rows) return code(SpMVError::INVALID_DIMENSION);
    if (!host_matrix_ok(A, B->num_rows, false) || !host_matrix_ok(B, B->num_cols, true)) {
        return code(SpMVError::INVALID_FORMAT);
    }
    const int m = A->num_rows, n = B->num_cols;

    // Gustavson: a dense accumulator, a mark per column and the list of the columns the row touched
    std::vector<float> acc(static_cast<size_t>(n), 0.0f);
    std::vector<unsigned char> seen(static_cast<size_t>(n), 0);
    std::vector<int> touched;
    std::vector<int> row_ptrs(static_cast<size_t>(m) + 1, 0);
    std::vector<int> cols;
    std::vector<float> vals;
    for (int i = 0; i < m; ++i) {
        touched.clear();
        for (int p = A->row_ptrs[i]; p < A->row_ptrs[i + 1]; ++p) {
            const int k = A->col_indices[p];
            const float a = A->values[p];
            for (int q = B->row_ptrs[k]; q < B->row_ptrs[k + 1]; ++q) {
                const int c = B->col_indices[q];
                if (!seen[c]) {
                    seen[c] = 1;
                    touched.push_back(c);
                }
                const float product = a * B->values[q];
                acc[c] = acc[c] + product;
            }
        }
        std::sort(touched.begin(), touched.end());
        if (cols.size() + touched.size() > static_cast<size_t>(INT_MAX)) return code(SpMVError::INVALID_DIMENSION);
        for (int c : touched) {
            cols.push_back(c);
            vals.push_back(acc[c]);
            acc[c] = 0.0f;
            seen[c] = 0;
        }
        row_ptrs[i + 1] = static_cast<int>(cols.size());
    }

    detail::csr_adopt_host(C, m, n, row_ptrs, cols, vals);
    return code(SpMVError::SUCCESS);
}

} // namespace spmv
