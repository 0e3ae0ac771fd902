// minres_smoke.cpp — a C++ caller of minres_solve written the way the reference's tests are: `#include "spmv/*.h"`,
// namespace spmv, CudaBuffer.  Solves a shifted 2-D Poisson system (5-point Laplacian, 32 x 32, shift 0.081: four
// negative eigenvalues) with both preconditioners and with diag(2) as the factor of minres_solve_ic (M = 4 I), checks the
// recomputed residual against ||b - (A - shift I) x|| / ||b|| in fp64 on the host, then a breakdown and the argument
// checks.  Built with plain g++ against include/ and libspmv_amd.so by tests/test_gpu_minres.py.  Needs a GPU.
#include "spmv/cuda_buffer.h"
#include "spmv/minres.h"
#include "spmv/spmv.h"

#include <cmath>
#include <cstdio>
#include <limits>
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

static CSRMatrix* poisson2d(int m) {
    const int n = m * m;
    std::vector<int> rp(1, 0), ci;
    std::vector<float> va;
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) {
            const int row = i * m + j;
            if (i > 0) { ci.push_back(row - m); va.push_back(-1.0f); }
            if (j > 0) { ci.push_back(row - 1); va.push_back(-1.0f); }
            ci.push_back(row); va.push_back(4.0f);
            if (j + 1 < m) { ci.push_back(row + 1); va.push_back(-1.0f); }
            if (i + 1 < m) { ci.push_back(row + m); va.push_back(-1.0f); }
            rp.push_back(static_cast<int>(ci.size()));
        }
    }
    return from_entries(n, rp, ci, va);
}

static double true_residual(const CSRMatrix* A, float shift, const std::vector<float>& b,
                            const std::vector<float>& x) {
    double num = 0.0, den = 0.0;
    for (int i = 0; i < A->num_rows; ++i) {
        double ax = -static_cast<double>(shift) * x[i];
        for (int k = A->row_ptrs[i]; k < A->row_ptrs[i + 1]; ++k) {
            ax += static_cast<double>(A->values[k]) * x[A->col_indices[k]];
        }
        num += (b[i] - ax) * (b[i] - ax);
        den += static_cast<double>(b[i]) * b[i];
    }
    return std::sqrt(num / den);
}

int main() {
    CSRMatrix* A = poisson2d(32);
    const int n = A->num_rows;
    const float shift = 0.081f;
    CHECK(csr_to_gpu(A) == 0);
    std::vector<float> b(n), x(n), zero(n, 0.0f);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * i);
    CudaBuffer<float> d_b(n), d_x(n);
    d_b.copyFromHost(b.data(), n);

    // diag(2) as a factor: M = L L^T = 4 I
    std::vector<int> drp(n + 1), dci(n);
    for (int i = 0; i <= n; ++i) drp[i] = i;
    for (int i = 0; i < n; ++i) dci[i] = i;
    CSRMatrix* D = from_entries(n, drp, dci, std::vector<float>(n, 2.0f));
    CHECK(csr_to_gpu(D) == 0);

    int steps[3] = {0, 0, 0};
    for (int mode = 0; mode < 3; ++mode) {          // NONE, JACOBI, M = L L^T with L = diag(2)
        MinresConfig cfg;
        cfg.tolerance = 1e-5f;
        cfg.max_iterations = 2000;
        cfg.shift = shift;
        cfg.preconditioner = mode == 1 ? CGConfig::JACOBI : CGConfig::NONE;
        d_x.copyFromHost(zero.data(), n);
        const MinresResult r = mode == 2 ? minres_solve_ic(A, D, d_b.get(), d_x.get(), &cfg)
                                         : minres_solve(A, d_b.get(), d_x.get(), &cfg);
        CHECK(r.error_code == 0 && r.converged == 1 && r.breakdown == MinresResult::NONE);
        CHECK(r.iterations > 0 && r.iterations < 2000 && r.relative_residual <= 1e-5f && r.elapsed_ms > 0.0f);
        d_x.copyToHost(x.data(), n);
        const double res = true_residual(A, shift, b, x);
        // the recomputed residual: fp32 against fp64, a few units of fp32 rounding of the row sums
        CHECK(std::fabs(res - r.true_relative_residual) <= 2e-6 && res <= 1e-3);
        steps[mode] = r.iterations;
        std::printf("mode %d: %d steps, recurrence %.3g, recomputed %.3g (fp64 %.3g), %.3f ms\n", mode, r.iterations,
                    r.relative_residual, r.true_relative_residual, res, r.elapsed_ms);
    }
    // M = 4 I scales every vector by a power of two: the IC form walks NONE's path step for step
    CHECK(steps[0] == steps[2]);
    // defaults (JACOBI, 1e-6, no shift: the SPD matrix) through a null config
    d_x.copyFromHost(zero.data(), n);
    CHECK(minres_solve(A, d_b.get(), d_x.get()).converged == 1);

    // [[0, 0], [0, 1]] x = (1, 0): A v = 0, gamma = 0, SINGULAR at the first step, x stays at the guess
    {
        CSRMatrix* S = from_entries(2, {0, 1, 2}, {0, 1}, {0.0f, 1.0f});
        CHECK(csr_to_gpu(S) == 0);
        CudaBuffer<float> sb(2), sx(2);
        const float one_zero[2] = {1.0f, 0.0f};
        const float guess[2] = {0.0f, 0.0f};
        sb.copyFromHost(one_zero, 2);
        sx.copyFromHost(guess, 2);
        MinresConfig cfg;
        cfg.preconditioner = CGConfig::NONE;
        const MinresResult r = minres_solve(S, sb.get(), sx.get(), &cfg);
        float got[2] = {1.0f, 1.0f};
        sx.copyToHost(got, 2);
        CHECK(r.error_code == 0 && r.breakdown == MinresResult::SINGULAR && r.iterations == 0 && r.converged == 0);
        CHECK(got[0] == 0.0f && got[1] == 0.0f && r.true_relative_residual == 1.0f);
        csr_destroy(S);
    }

    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CHECK(minres_solve(nullptr, d_b.get(), d_x.get()).error_code == invalid_argument);
    CHECK(minres_solve(A, d_b.get(), d_b.get()).error_code == invalid_argument);
    MinresConfig bad;
    bad.shift = std::numeric_limits<float>::infinity();
    CHECK(minres_solve(A, d_b.get(), d_x.get(), &bad).error_code == invalid_argument);
    CHECK(minres_solve_ic(A, nullptr, d_b.get(), d_x.get()).error_code == invalid_argument);
    csr_destroy(D);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
