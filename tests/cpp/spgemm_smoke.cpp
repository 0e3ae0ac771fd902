// spgemm_smoke.cpp — a C++ caller of spgemm_csr / spgemm_csr_numeric written against spmv/spgemm.h, csr_matrix.h and
// CudaBuffer only: the normal equations A^T A through csr_transpose_gpu and spgemm_csr, the values again through
// spgemm_csr_numeric after A was rescaled, and the product fed to spmv_csr.  Compiled and run by
// tests/test_gpu_spgemm.py.
#include "spmv/csr_matrix.h"
#include "spmv/cuda_buffer.h"
#include "spmv/spgemm.h"
#include "spmv/spmv.h"

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
    // A: 300 x 40, three to five small-integer entries per row, columns ascending
    const int rows = 300, cols = 40;
    std::vector<float> dense(static_cast<size_t>(rows) * cols, 0.0f);
    for (int i = 0; i < rows; ++i) {
        for (int j = 0; j < 3 + i % 3; ++j) dense[static_cast<size_t>(i) * cols + (i * 7 + j * 11) % cols] = float(1 + (i + j) % 5);
    }
    CSRMatrix* A = csr_create(0, 0, 0);
    CHECK(csr_from_dense(A, dense.data(), rows, cols) == 0 && csr_to_gpu(A) == 0);

    CSRMatrix* AT = csr_create(0, 0, 0);
    CHECK(csr_transpose_gpu(AT, A) == 0 && csr_from_gpu(AT) == 0);
    CSRMatrix* C = csr_create(0, 0, 0);
    SpGEMMResult res;
    CHECK(spgemm_csr(C, AT, A, &res) == 0 && res.error_code == 0 && res.nnz == C->nnz && res.products > res.nnz);
    CHECK(C->num_rows == cols && C->num_cols == cols && C->owns_device_memory && csr_from_gpu(C) == 0);
    CSRMatrix* H = csr_create(0, 0, 0);
    CHECK(spgemm_cpu_csr(H, AT, A) == 0 && same_matrix(C, H));
    for (int i = 0; i < cols; ++i) {                     // A^T A is symmetric, entry for entry
        for (int p = C->row_ptrs[i]; p < C->row_ptrs[i + 1]; ++p) {
            CHECK(csr_get_element(C, C->col_indices[p], i) == C->values[p]);
        }
    }

    // rescale A (host and device), transpose again, and refill C's values only
    for (int p = 0; p < A->nnz; ++p) A->values[p] *= 0.5f;
    CHECK(hipMemcpy(A->d_values, A->values, sizeof(float) * A->nnz, hipMemcpyHostToDevice) == hipSuccess);
    csr_invalidate_gpu_cache(A);
    CHECK(csr_transpose_gpu(AT, A) == 0 && csr_from_gpu(AT) == 0);
    const int* structure = C->d_col_indices;
    CHECK(spgemm_csr_numeric(C, AT, A, &res) == 0 && C->d_col_indices == structure && csr_from_gpu(C) == 0);
    CHECK(spgemm_cpu_csr(H, AT, A) == 0 && same_matrix(C, H));

    // the product is a matrix like any other: y = (A^T A) x against the host
    std::vector<float> x(cols), y(cols), want(cols);
    for (int j = 0; j < cols; ++j) x[j] = float(j % 7) - 3.0f;
    CudaBuffer<float> d_x(cols), d_y(cols);
    d_x.copyFromHost(x.data(), cols);
    const SpMVResult r = spmv_csr(C, d_x.get(), d_y.get(), nullptr);
    CHECK(r.error_code == 0);
    d_y.copyToHost(y.data(), cols);
    spmv_cpu_csr(H, x.data(), want.data());
    CHECK(std::memcmp(y.data(), want.data(), sizeof(float) * cols) == 0);      // quarter-integers: exact in any order

    // the checks a caller meets first
    CHECK(spgemm_csr(nullptr, AT, A) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(spgemm_csr(AT, AT, A) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(spgemm_csr(C, A, A) == static_cast<int>(SpMVError::INVALID_DIMENSION));
    for (CSRMatrix* m : {A, AT, C, H}) csr_destroy(m);
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
