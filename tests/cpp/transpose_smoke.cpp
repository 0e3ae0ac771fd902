// transpose_smoke.cpp — a C++ caller of csr_transpose_gpu and spmv_csr_transpose written the way the reference's
// tests are: `#include "spmv/*.h"`, namespace spmv, CudaBuffer.  The device transpose is checked entry for entry
// against a host transpose, and y = A^T x against spmv_cpu_csr on that host transpose: bit for bit for SCALAR_CSR,
// within the reordered-sum bound for VECTOR_CSR / MERGE_PATH.  Built with plain g++ against include/ and
// libspmv_amd.so by tests/test_gpu_transpose.py.  Needs a GPU.
#include "spmv/spmv.h"
#include "spmv/cuda_buffer.h"
#include "spmv/test_utils.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;
using namespace spmv::test;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

// stable counting-sort transpose on the host: row c holds column c's entries in source order
static CSRMatrix* host_transpose(const CSRMatrix* A) {
    CSRMatrix* T = csr_create(A->num_cols, A->num_rows, A->nnz);
    for (int p = 0; p < A->nnz; ++p) ++T->row_ptrs[A->col_indices[p] + 1];
    for (int c = 0; c < A->num_cols; ++c) T->row_ptrs[c + 1] += T->row_ptrs[c];
    std::vector<int> next(T->row_ptrs, T->row_ptrs + A->num_cols);
    for (int r = 0; r < A->num_rows; ++r) {
        for (int p = A->row_ptrs[r]; p < A->row_ptrs[r + 1]; ++p) {
            const int slot = next[A->col_indices[p]]++;
            T->col_indices[slot] = r;
            T->values[slot] = A->values[p];
        }
    }
    return T;
}

// |got - want| <= 1e-5 * max(|want|, sum_j |a_ij x_j|)
static bool reordered_ok(const CSRMatrix* A, const float* x, const float* want, const float* got) {
    for (int i = 0; i < A->num_rows; ++i) {
        double abs_sum = 0.0;
        for (int j = A->row_ptrs[i]; j < A->row_ptrs[i + 1]; ++j) {
            abs_sum += std::fabs(static_cast<double>(A->values[j]) * x[A->col_indices[j]]);
        }
        const double scale = std::fmax(std::fabs(want[i]), abs_sum);
        if (std::fabs(static_cast<double>(want[i]) - got[i]) > 1e-5 * std::fmax(scale, 1e-30)) return false;
    }
    return true;
}

int main() {
    RandomGenerator rng(11);
    for (int iter = 0; iter < 12; ++iter) {
        const int rows = rng.randInt(1, 400), cols = rng.randInt(1, 400);
        auto dense = generateRandomDenseMatrix(rows, cols, rng.randFloat(0.01f, 0.3f), rng);
        CSRMatrix* A = csr_create(0, 0, 0);
        csr_from_dense(A, dense.data(), rows, cols);
        CHECK(csr_to_gpu(A) == 0);
        CSRMatrix* want = host_transpose(A);

        CSRMatrix* AT = csr_create(0, 0, 0);
        CHECK(csr_transpose_gpu(AT, A) == 0);
        CHECK(AT->num_rows == cols && AT->num_cols == rows && AT->nnz == A->nnz && AT->owns_device_memory);
        CHECK(csr_from_gpu(AT) == 0);
        CHECK(std::memcmp(AT->row_ptrs, want->row_ptrs, sizeof(int) * (cols + 1)) == 0);
        if (A->nnz > 0) {
            CHECK(std::memcmp(AT->col_indices, want->col_indices, sizeof(int) * A->nnz) == 0);
            CHECK(std::memcmp(AT->values, want->values, sizeof(float) * A->nnz) == 0);
        }

        std::vector<float> x(rows), y_cpu(cols), y(cols);
        for (float& v : x) v = rng.randFloat(-1.0f, 1.0f);
        spmv_cpu_csr(want, x.data(), y_cpu.data());
        CudaBuffer<float> d_x(rows), d_y(cols);
        d_x.copyFromHost(x.data(), rows);
        for (auto kt : {SpMVConfig::SCALAR_CSR, SpMVConfig::VECTOR_CSR, SpMVConfig::MERGE_PATH}) {
            SpMVConfig cfg;
            cfg.kernel_type = kt;
            const SpMVResult r = spmv_csr_transpose(A, d_x.get(), d_y.get(), &cfg, rows);
            CHECK(r.error_code == 0 && r.y == d_y.get());
            d_y.copyToHost(y.data(), cols);
            if (kt == SpMVConfig::SCALAR_CSR) {
                CHECK(std::memcmp(y.data(), y_cpu.data(), sizeof(float) * cols) == 0);
            } else {
                CHECK(reordered_ok(want, x.data(), y_cpu.data(), y.data()));
            }
        }
        CHECK(spmv_csr_transpose(A, d_x.get(), d_y.get(), nullptr, rows + 1).error_code ==
              static_cast<int>(SpMVError::INVALID_DIMENSION));
        csr_destroy(AT);
        csr_destroy(want);
        csr_destroy(A);
    }
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
