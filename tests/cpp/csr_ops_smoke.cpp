// csr_ops_smoke.cpp — a C++ caller of include/spmv/csr_ops.h written against the public headers and CudaBuffer only:
// the implicit time-stepping matrix M + dt K through csr_add, a new dt through csr_add_numeric, the shift A - sigma I
// through csr_diag_matrix_gpu, the symmetric scaling D^-1/2 A D^-1/2 through csr_diagonal_gpu and csr_scale_gpu, and the
// result fed to spmv_csr.  Compiled and run by tests/test_gpu_csr_ops.py.
#include "spmv/csr_matrix.h"
#include "spmv/csr_ops.h"
#include "spmv/cuda_buffer.h"
#include "spmv/spmv.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

static bool same_matrix(const CSRMatrix* x, const CSRMatrix* y) {
    return x->num_rows == y->num_rows && x->num_cols == y->num_cols && x->nnz == y->nnz &&
           std::memcmp(x->row_ptrs, y->row_ptrs, sizeof(int) * (x->num_rows + 1)) == 0 &&
           std::memcmp(x->col_indices, y->col_indices, sizeof(int) * x->nnz) == 0 &&
           std::memcmp(x->values, y->values, sizeof(float) * x->nnz) == 0;
}

int main() {
    // M: tridiagonal mass matrix; K: a five-wide stiffness band, so the two patterns differ
    const int n = 500;
    std::vector<float> dm(static_cast<size_t>(n) * n, 0.0f), dk(static_cast<size_t>(n) * n, 0.0f);
    for (int i = 0; i < n; ++i) {
        for (int j = i - 2; j <= i + 2; ++j) {
            if (j < 0 || j >= n) continue;
            const int d = j > i ? j - i : i - j;
            if (d <= 1) dm[static_cast<size_t>(i) * n + j] = d == 0 ? 4.0f / 6.0f : 1.0f / 6.0f;
            dk[static_cast<size_t>(i) * n + j] = d == 0 ? 6.0f : (d == 1 ? -2.5f : -0.5f);
        }
    }
    CSRMatrix* M = csr_create(0, 0, 0);
    CSRMatrix* K = csr_create(0, 0, 0);
    CHECK(csr_from_dense(M, dm.data(), n, n) == 0 && csr_to_gpu(M) == 0);
    CHECK(csr_from_dense(K, dk.data(), n, n) == 0 && csr_to_gpu(K) == 0);

    CSRMatrix* C = csr_create(0, 0, 0);
    CSRMatrix* H = csr_create(0, 0, 0);
    CsrAddResult res;
    CHECK(csr_add(C, 1.0f, M, 0.01f, K, &res) == 0 && res.error_code == 0 && res.nnz == K->nnz && res.common == M->nnz);
    CHECK(res.max_row_nnz == 5 && res.lanes >= 1 && res.launches >= 3);
    CHECK(C->num_rows == n && C->num_cols == n && C->owns_device_memory && csr_from_gpu(C) == 0);
    CHECK(csr_add_cpu(H, 1.0f, M, 0.01f, K) == 0 && same_matrix(C, H));

    // another time step: only the values
    const int* structure = C->d_col_indices;
    CHECK(csr_add_numeric(C, 1.0f, M, 0.25f, K, &res) == 0 && res.launches == 1 && C->d_col_indices == structure);
    CHECK(csr_from_gpu(C) == 0 && csr_add_cpu(H, 1.0f, M, 0.25f, K) == 0 && same_matrix(C, H));
    CHECK(csr_add_numeric(M, 1.0f, M, 0.25f, K) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CSRMatrix* wrong = csr_create(0, 0, 0);
    CHECK(csr_add(wrong, 1.0f, M, 1.0f, M) == 0);                              // M's pattern is not the union's
    CHECK(csr_add_numeric(wrong, 1.0f, M, 0.25f, K) == static_cast<int>(SpMVError::INVALID_FORMAT));

    // the shift: S = C - sigma I
    CSRMatrix* I = csr_create(0, 0, 0);
    CSRMatrix* S = csr_create(0, 0, 0);
    CHECK(csr_diag_matrix_gpu(I, n, nullptr) == 0 && I->nnz == n);
    CHECK(csr_add(S, 1.0f, C, -0.125f, I) == 0 && S->nnz == C->nnz && csr_from_gpu(S) == 0);
    for (int i = 0; i < n; ++i) {
        const float shifted = csr_get_element(C, i, i) + (-0.125f * 1.0f);
        CHECK(csr_get_element(S, i, i) == shifted);
    }

    // the symmetric scaling D^-1/2 S D^-1/2: symmetric entry for entry, with a unit diagonal up to rounding
    CudaBuffer<float> d_diag(n);
    std::vector<float> diag(n), scale(n);
    CHECK(csr_diagonal_gpu(S, d_diag.get()) == 0);
    d_diag.copyToHost(diag.data(), n);
    for (int i = 0; i < n; ++i) {
        CHECK(diag[i] == csr_get_element(S, i, i));
        scale[i] = 1.0f / std::sqrt(diag[i]);
    }
    CHECK(csr_diagonal_cpu(S, scale.data()) == 0 && std::memcmp(scale.data(), diag.data(), sizeof(float) * n) == 0);
    for (int i = 0; i < n; ++i) scale[i] = 1.0f / std::sqrt(diag[i]);
    CudaBuffer<float> d_scale(n);
    d_scale.copyFromHost(scale.data(), n);
    std::vector<float> want(S->nnz);
    CHECK(csr_scale_cpu(S, scale.data(), scale.data(), want.data()) == 0);
    CHECK(csr_scale_gpu(S, d_scale.get(), d_scale.get(), nullptr) == 0 && csr_from_gpu(S) == 0);
    CHECK(std::memcmp(S->values, want.data(), sizeof(float) * S->nnz) == 0);
    for (int i = 0; i < n; ++i) {
        CHECK(std::fabs(csr_get_element(S, i, i) - 1.0f) < 1e-6f);
        for (int p = S->row_ptrs[i]; p < S->row_ptrs[i + 1]; ++p) {
            CHECK(csr_get_element(S, S->col_indices[p], i) == S->values[p]);
        }
    }

    // the sum is a matrix like any other: y = S x against the host
    std::vector<float> x(n), y(n), ref(n);
    for (int j = 0; j < n; ++j) x[j] = float(j % 7) - 3.0f;
    CudaBuffer<float> d_x(n), d_y(n);
    d_x.copyFromHost(x.data(), n);
    const SpMVResult r = spmv_csr(S, d_x.get(), d_y.get(), nullptr);
    CHECK(r.error_code == 0);
    d_y.copyToHost(y.data(), n);
    spmv_cpu_csr(S, x.data(), ref.data());
    CHECK(std::memcmp(y.data(), ref.data(), sizeof(float) * n) == 0);          // the default kernel keeps the host's order

    // the checks a caller meets first
    CHECK(csr_add(nullptr, 1.0f, M, 1.0f, K) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(csr_add(M, 1.0f, M, 1.0f, K) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CSRMatrix* R = csr_create(0, 0, 0);
    CHECK(csr_diag_matrix_gpu(R, n + 1, nullptr) == 0);
    CHECK(csr_add(C, 1.0f, M, 1.0f, R) == static_cast<int>(SpMVError::INVALID_DIMENSION));
    CHECK(csr_scale_gpu(S, d_scale.get(), d_scale.get(), d_scale.get()) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    for (CSRMatrix* m : {M, K, C, H, wrong, I, S, R}) csr_destroy(m);
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
