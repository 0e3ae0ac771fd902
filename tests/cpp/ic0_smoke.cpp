// ic0_smoke.cpp — a C++ caller of the IC(0) factorisation and the IC-preconditioned CG, written against the installed
// headers only (`#include "spmv/ic0.h"`, namespace spmv, CudaBuffer, direct struct-field access) and built with plain
// g++ against include/ and libspmv_amd.so: factor, wrap, two triangular solves, solve, check the residual.  Needs a
// GPU to run.
#include "spmv/cg.h"
#include "spmv/cuda_buffer.h"
#include "spmv/ic0.h"
#include "spmv/sptrsv.h"

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

int main() {
    const int m = 32, n = m * m;
    CSRMatrix* A = laplacian(m);
    const int nnz = A->nnz;
    CHECK(csr_to_gpu(A) == 0);

    // factor on the host and on the device: the same bits
    std::vector<float> want(nnz), got(nnz);
    int cpu_pivot = 7;
    CHECK(ic0_cpu_csr(A, want.data(), &cpu_pivot) == 0 && cpu_pivot == -1);
    CudaBuffer<float> d_l(nnz);
    IC0Result f = ic0_csr(A, d_l.get());
    CHECK(f.error_code == 0 && f.bad_pivot == -1 && f.analysis_ms > 0.0f && f.num_levels == 2 * m - 1);
    CHECK(f.launches >= 1 && f.lanes_per_row >= 1 && f.lanes_per_row <= 64);
    d_l.copyToHost(got.data(), nnz);
    CHECK(std::memcmp(got.data(), want.data(), nnz * sizeof(float)) == 0);
    f = ic0_csr(A, d_l.get());
    CHECK(f.error_code == 0 && f.analysis_ms == 0.0f);
    CHECK(ic0_csr_async(A, d_l.get(), nullptr) == 0 && hipDeviceSynchronize() == hipSuccess);
    d_l.copyToHost(got.data(), nnz);
    CHECK(std::memcmp(got.data(), want.data(), nnz * sizeof(float)) == 0);

    // wrap the factor over A's structure arrays (a header that owns nothing): one matrix for both triangles
    CSRMatrix wrap{};
    wrap.num_rows = wrap.num_cols = n;
    wrap.nnz = nnz;
    wrap.d_row_ptrs = A->d_row_ptrs;
    wrap.d_col_indices = A->d_col_indices;
    wrap.d_values = d_l.get();
    wrap.row_ptrs = A->row_ptrs;                                // host side for sptrsv_cpu_csr below
    wrap.col_indices = A->col_indices;
    wrap.values = want.data();
    const CSRMatrix* F = &wrap;
    std::vector<float> b(n), x(n, 0.0f), y(n), y_ref(n);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * static_cast<float>(i)) + 0.1f;
    CudaBuffer<float> d_b(n), d_x(n), d_y(n);
    d_b.copyFromHost(b.data(), n);
    d_x.copyFromHost(x.data(), n);
    SpTRSVConfig lower, upper;
    lower.uplo = SpTRSVConfig::LOWER;
    upper.uplo = SpTRSVConfig::UPPER;
    lower.diag = upper.diag = SpTRSVConfig::NON_UNIT;
    lower.ordered = upper.ordered = 1;
    const SpTRSVResult t = sptrsv_csr(F, d_b.get(), d_y.get(), &lower);
    CHECK(t.error_code == 0 && t.analysis_ms == 0.0f);          // the schedule the factorisation used
    CHECK(sptrsv_csr(F, d_y.get(), d_y.get(), &upper).error_code == 0);
    d_y.copyToHost(y.data(), n);
    CHECK(sptrsv_cpu_csr(F, b.data(), y_ref.data(), &lower) == 0 && sptrsv_cpu_csr(F, y_ref.data(), y_ref.data(), &upper) == 0);
    CHECK(std::memcmp(y.data(), y_ref.data(), n * sizeof(float)) == 0);

    CGConfig cfg;
    cfg.tolerance = 1e-6f;
    cfg.engine = 0;
    cfg.preconditioner = 99;                                    // not read by cg_solve_ic
    const CGResult ic = cg_solve_ic(A, F, d_b.get(), d_x.get(), &cfg);
    CHECK(ic.error_code == 0 && ic.converged == 1 && ic.breakdown == 0 && ic.iterations >= 1);
    CHECK(ic.relative_residual <= 1e-6f);
    d_x.copyToHost(x.data(), n);
    CHECK(residual(A, b, x) <= 4e-6);

    std::vector<float> zero(n, 0.0f);
    d_x.copyFromHost(zero.data(), n);
    cfg.preconditioner = CGConfig::JACOBI;
    const CGResult jacobi = cg_solve(A, d_b.get(), d_x.get(), &cfg);
    CHECK(jacobi.error_code == 0 && jacobi.converged == 1);
    CHECK(ic.iterations < jacobi.iterations);
    std::printf("iterations: IC(0) %d, Jacobi %d\n", ic.iterations, jacobi.iterations);

    // argument checks through the C++ entry points
    CHECK(ic0_csr(nullptr, d_l.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(ic0_csr(A, static_cast<float*>(A->d_values) + 1).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(cg_solve_ic(A, nullptr, d_b.get(), d_x.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    cfg.preconditioner = 2;
    CHECK(cg_solve(A, d_b.get(), d_x.get(), &cfg).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));

    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
