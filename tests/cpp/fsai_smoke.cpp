// fsai_smoke.cpp — a C++ caller of the factorised sparse approximate inverse and the FSAI-preconditioned CG, written
// against the installed headers only (`#include "spmv/fsai.h"`, namespace spmv, CudaBuffer, direct struct-field access)
// and built with plain g++ against include/ and libspmv_amd.so: build G on the host and on the device, transpose,
// refill, solve, check the residual.  Needs a GPU to run.
#include "spmv/cg.h"
#include "spmv/cuda_buffer.h"
#include "spmv/fsai.h"
#include "spmv/spgemm.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

// 5-point Laplacian on an m x m grid: symmetric positive definite, columns ascending
static CSRMatrix* laplacian(int m) {
    const int n = m * m;
    std::vector<int> ptr(1, 0), col;
    std::vector<float> val;
    for (int i = 0; i < n; ++i) {
        const int gx = i % m, gy = i / m;
        if (gy > 0) { col.push_back(i - m); val.push_back(-1.0f); }
        if (gx > 0) { col.push_back(i - 1); val.push_back(-1.0f); }
        col.push_back(i); val.push_back(4.0f);
        if (gx + 1 < m) { col.push_back(i + 1); val.push_back(-1.0f); }
        if (gy + 1 < m) { col.push_back(i + m); val.push_back(-1.0f); }
        ptr.push_back(static_cast<int>(col.size()));
    }
    CSRMatrix* A = csr_create(n, n, static_cast<int>(col.size()));
    std::memcpy(A->row_ptrs, ptr.data(), ptr.size() * sizeof(int));
    std::memcpy(A->col_indices, col.data(), col.size() * sizeof(int));
    std::memcpy(A->values, val.data(), val.size() * sizeof(float));
    return A;
}

static double residual(const CSRMatrix* A, const std::vector<float>& b, const std::vector<float>& x) {
    double rr = 0.0, bb = 0.0;
    for (int i = 0; i < A->num_rows; ++i) {
        double s = b[i];
        for (int j = A->row_ptrs[i]; j < A->row_ptrs[i + 1]; ++j) s -= static_cast<double>(A->values[j]) * x[A->col_indices[j]];
        rr += s * s;
        bb += static_cast<double>(b[i]) * b[i];
    }
    return std::sqrt(rr / bb);
}

static bool same(const CSRMatrix* X, const CSRMatrix* Y) {
    return X->num_rows == Y->num_rows && X->nnz == Y->nnz &&
           std::memcmp(X->row_ptrs, Y->row_ptrs, (X->num_rows + 1) * sizeof(int)) == 0 &&
           std::memcmp(X->col_indices, Y->col_indices, X->nnz * sizeof(int)) == 0 &&
           std::memcmp(X->values, Y->values, X->nnz * sizeof(float)) == 0;
}

int main() {
    const int m = 32, n = m * m;
    CSRMatrix* A = laplacian(m);
    CHECK(csr_to_gpu(A) == 0);

    // G on the host and on the device: the same bits
    CSRMatrix* want = csr_create(0, 0, 0);
    CSRMatrix* G = csr_create(0, 0, 0);
    CSRMatrix* GT = csr_create(0, 0, 0);
    int cpu_bad = 7;
    CHECK(fsai_cpu_csr(want, A, nullptr, &cpu_bad) == 0 && cpu_bad == -1);
    FSAIResult f = fsai_csr(G, A);
    CHECK(f.error_code == 0 && f.bad_row == -1 && f.long_row == -1 && f.max_row == 3 && f.row_class == 4);
    CHECK(f.nnz == want->nnz && f.lanes_per_row == 4 && f.elapsed_ms > 0.0f);
    CHECK(csr_from_gpu(G) == 0 && same(G, want));
    CHECK(csr_transpose_gpu(GT, G) == 0 && GT->nnz == G->nnz);
    // the refill writes the same bits again
    f = fsai_csr_numeric(G, A);
    CHECK(f.error_code == 0 && f.bad_row == -1 && f.row_class == 4 && csr_from_gpu(G) == 0 && same(G, want));

    std::vector<float> b(n), x(n, 0.0f), zero(n, 0.0f);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * static_cast<float>(i)) + 0.1f;
    CudaBuffer<float> d_b(n), d_x(n);
    d_b.copyFromHost(b.data(), n);
    d_x.copyFromHost(x.data(), n);
    CGConfig cfg;
    cfg.tolerance = 1e-6f;
    cfg.engine = 0;
    cfg.preconditioner = 99;                                    // not read by cg_solve_fsai
    const CGResult own = cg_solve_fsai(A, G, GT, d_b.get(), d_x.get(), &cfg);
    CHECK(own.error_code == 0 && own.converged == 1 && own.breakdown == 0 && own.iterations >= 1);
    CHECK(own.relative_residual <= 1e-6f);
    d_x.copyToHost(x.data(), n);
    CHECK(residual(A, b, x) <= 1e-5);

    // the stronger G on the pattern of A*A
    CSRMatrix* S = csr_create(0, 0, 0);
    CSRMatrix* G2 = csr_create(0, 0, 0);
    CSRMatrix* GT2 = csr_create(0, 0, 0);
    CHECK(spgemm_csr(S, A, A) == 0);
    f = fsai_csr(G2, A, S);
    CHECK(f.error_code == 0 && f.bad_row == -1 && f.max_row == 7 && f.row_class == 8 && f.nnz > G->nnz);
    CHECK(csr_transpose_gpu(GT2, G2) == 0);
    d_x.copyFromHost(zero.data(), n);
    const CGResult rich = cg_solve_fsai(A, G2, GT2, d_b.get(), d_x.get(), &cfg);
    CHECK(rich.error_code == 0 && rich.converged == 1);
    d_x.copyToHost(x.data(), n);
    CHECK(residual(A, b, x) <= 1e-5);

    d_x.copyFromHost(zero.data(), n);
    cfg.preconditioner = CGConfig::JACOBI;
    const CGResult jacobi = cg_solve(A, d_b.get(), d_x.get(), &cfg);
    CHECK(jacobi.error_code == 0 && jacobi.converged == 1);
    CHECK(rich.iterations < own.iterations && own.iterations < jacobi.iterations);
    std::printf("iterations: FSAI on A*A %d, FSAI %d, Jacobi %d\n", rich.iterations, own.iterations, jacobi.iterations);

    // argument checks through the C++ entry points
    CHECK(fsai_csr(nullptr, A).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(fsai_csr(A, A).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(fsai_csr_numeric(G, nullptr).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(cg_solve_fsai(A, nullptr, GT, d_b.get(), d_x.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(cg_solve_fsai(A, G, nullptr, d_b.get(), d_x.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));

    for (CSRMatrix* M : {A, want, G, GT, S, G2, GT2}) csr_destroy(M);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
