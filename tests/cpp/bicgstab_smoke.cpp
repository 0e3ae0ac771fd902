// bicgstab_smoke.cpp — a C++ caller of bicgstab_solve written the way the reference's tests are: `#include
// "spmv/*.h"`, namespace spmv, CudaBuffer.  Solves a 2-D convection-diffusion system (5-point Laplacian plus
// first-order upwind convection, 48 x 48, wind 2 on both axes: non-symmetric) with both preconditioners and checks
// the true residual ||b - A x|| / ||b|| in fp64 on the host (to 1e-3: fp32 vectors), then a breakdown and the
// argument checks.  Built with plain g++ against include/ and libspmv_amd.so by tests/test_gpu_bicgstab.py.
// Needs a GPU.
#include "spmv/bicgstab.h"
#include "spmv/cuda_buffer.h"
#include "spmv/spmv.h"

#include <cmath>
#include <cstdio>
#include <vector>

using namespace spmv;

static int g_failures = 0;
#define CHECK(cond) \
    do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static CSRMatrix* from_entries(int n, const std::vector<int>& rp, const std::vector<int>& ci,
                               const std::vector<float>& va) {
    CSRMatrix* A = csr_create(n, n, static_cast<int>(ci.size()));
    for (int i = 0; i <= n; ++i) A->row_ptrs[i] = rp[i];
    for (size_t k = 0; k < ci.size(); ++k) {
        A->col_indices[k] = ci[k];
        A->values[k] = va[k];
    }
    return A;
}

static CSRMatrix* convdiff2d(int m, float wind) {
    const int n = m * m;
    std::vector<int> rp(1, 0), ci;
    std::vector<float> va;
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) {
            const int row = i * m + j;
            if (i > 0) { ci.push_back(row - m); va.push_back(-1.0f - wind); }     // upstream on both axes
            if (j > 0) { ci.push_back(row - 1); va.push_back(-1.0f - wind); }
            ci.push_back(row); va.push_back(4.0f + 2.0f * wind);
            if (j + 1 < m) { ci.push_back(row + 1); va.push_back(-1.0f); }
            if (i + 1 < m) { ci.push_back(row + m); va.push_back(-1.0f); }
            rp.push_back(static_cast<int>(ci.size()));
        }
    }
    return from_entries(n, rp, ci, va);
}

static double true_residual(const CSRMatrix* A, const std::vector<float>& b, const std::vector<float>& x) {
    double num = 0.0, den = 0.0;
    for (int i = 0; i < A->num_rows; ++i) {
        double ax = 0.0;
        for (int k = A->row_ptrs[i]; k < A->row_ptrs[i + 1]; ++k) {
            ax += static_cast<double>(A->values[k]) * x[A->col_indices[k]];
        }
        num += (b[i] - ax) * (b[i] - ax);
        den += static_cast<double>(b[i]) * b[i];
    }
    return std::sqrt(num / den);
}

int main() {
    CSRMatrix* A = convdiff2d(48, 2.0f);
    const int n = A->num_rows;
    CHECK(csr_to_gpu(A) == 0);
    std::vector<float> b(n), x(n);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * i);     // zero-mean: see the residual check below
    CudaBuffer<float> d_b(n), d_x(n);
    d_b.copyFromHost(b.data(), n);

    for (int pre : {CGConfig::NONE, CGConfig::JACOBI}) {
        BiCGStabConfig cfg;
        cfg.tolerance = 1e-5f;
        cfg.preconditioner = pre;
        std::vector<float> zero(n, 0.0f);
        d_x.copyFromHost(zero.data(), n);
        const BiCGStabResult r = bicgstab_solve(A, d_b.get(), d_x.get(), &cfg);
        CHECK(r.error_code == 0 && r.converged == 1 && r.breakdown == BiCGStabResult::NONE);
        CHECK(r.iterations > 0 && r.iterations < 1000 && r.relative_residual <= 1e-5f && r.elapsed_ms > 0.0f);
        d_x.copyToHost(x.data(), n);
        const double res = true_residual(A, b, x);
        // fp32 vectors: the true residual drifts from the recurrence one (to ~1e-3 here with b = sin + 0.5, in the
        // numpy restatement as on the device; ~1e-5 with this b)
        CHECK(res <= 1e-3);
        std::printf("preconditioner %d: %d iterations, relative residual %.3g (true %.3g), %.3f ms\n", pre,
                    r.iterations, r.relative_residual, res, r.elapsed_ms);
    }
    // defaults (JACOBI, 1e-6) through a null config
    CHECK(bicgstab_solve(A, d_b.get(), d_x.get()).converged == 1);

    // [[0, 1], [-1, 0]] x = (1, 0): r^.v = 0 at the first step, x stays 0
    {
        CSRMatrix* R = from_entries(2, {0, 1, 2}, {1, 0}, {1.0f, -1.0f});
        CHECK(csr_to_gpu(R) == 0);
        CudaBuffer<float> rb(2), rx(2);
        const float one_zero[2] = {1.0f, 0.0f};
        const float zeros[2] = {0.0f, 0.0f};
        rb.copyFromHost(one_zero, 2);
        rx.copyFromHost(zeros, 2);
        BiCGStabConfig cfg;
        cfg.preconditioner = CGConfig::NONE;
        const BiCGStabResult r = bicgstab_solve(R, rb.get(), rx.get(), &cfg);
        float got[2] = {1.0f, 1.0f};
        rx.copyToHost(got, 2);
        CHECK(r.error_code == 0 && r.breakdown == BiCGStabResult::ALPHA && r.iterations == 0 && r.converged == 0);
        CHECK(got[0] == 0.0f && got[1] == 0.0f);
        csr_destroy(R);
    }

    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CHECK(bicgstab_solve(nullptr, d_b.get(), d_x.get()).error_code == invalid_argument);
    CHECK(bicgstab_solve(A, d_b.get(), d_b.get()).error_code == invalid_argument);
    BiCGStabConfig bad;
    bad.engine = 7;
    CHECK(bicgstab_solve(A, d_b.get(), d_x.get(), &bad).error_code == invalid_argument);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
