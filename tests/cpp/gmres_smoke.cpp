// gmres_smoke.cpp — a C++ caller of gmres_solve written the way the reference's tests are: `#include "spmv/*.h"`,
// namespace spmv, CudaBuffer.  Solves a 2-D convection-diffusion system (5-point Laplacian plus first-order upwind
// convection, 48 x 48, wind 2 on both axes: non-symmetric) with both preconditioners and with diag(A) as the factor
// of gmres_solve_lu, checks the reported residual against ||b - A x|| / ||b|| in fp64 on the host, then a
// breakdown and the argument checks.  Built with plain g++ against include/ and libspmv_amd.so by
// tests/test_gpu_gmres.py.  Needs a GPU.
#include "spmv/cuda_buffer.h"
#include "spmv/gmres.h"
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
    std::vector<float> b(n), x(n), zero(n, 0.0f);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * i);
    CudaBuffer<float> d_b(n), d_x(n);
    d_b.copyFromHost(b.data(), n);

    // diag(A) as a factor: L = I, U = diag(A)
    std::vector<int> drp(n + 1), dci(n);
    for (int i = 0; i <= n; ++i) drp[i] = i;
    for (int i = 0; i < n; ++i) dci[i] = i;
    CSRMatrix* D = from_entries(n, drp, dci, std::vector<float>(n, 8.0f));
    CHECK(csr_to_gpu(D) == 0);

    for (int mode = 0; mode < 3; ++mode) {          // NONE, JACOBI, M = L U with L = I and U = diag(A)
        GMRESConfig cfg;
        cfg.tolerance = 1e-5f;
        cfg.restart = 20;
        cfg.preconditioner = mode == 1 ? CGConfig::JACOBI : CGConfig::NONE;
        d_x.copyFromHost(zero.data(), n);
        const GMRESResult r = mode == 2 ? gmres_solve_lu(A, D, d_b.get(), d_x.get(), &cfg)
                                        : gmres_solve(A, d_b.get(), d_x.get(), &cfg);
        CHECK(r.error_code == 0 && r.converged == 1 && r.breakdown == GMRESResult::NONE);
        CHECK(r.iterations > 0 && r.iterations < 1000 && r.relative_residual <= 1e-5f && r.elapsed_ms > 0.0f);
        CHECK(r.restarts >= (r.iterations - 1) / 20);          // more only after an optimistic estimate
        d_x.copyToHost(x.data(), n);
        const double res = true_residual(A, b, x);
        // the reported residual is the recomputed one: fp32 against fp64, a few units of fp32 rounding of the row sums
        CHECK(std::fabs(res - r.relative_residual) <= 2e-6 && res <= 1.2e-5);
        std::printf("mode %d: %d steps, %d restarts, relative residual %.3g (true %.3g), %.3f ms\n", mode,
                    r.iterations, r.restarts, r.relative_residual, res, r.elapsed_ms);
    }
    // defaults (JACOBI, 1e-6, restart 30) through a null config
    CHECK(gmres_solve(A, d_b.get(), d_x.get()).converged == 1);

    // [[2, 0], [0, 0]] x = (0, 1): A v_0 = 0, SINGULAR in the first column, x stays at the guess
    {
        CSRMatrix* S = from_entries(2, {0, 1, 1}, {0}, {2.0f});
        CHECK(csr_to_gpu(S) == 0);
        CudaBuffer<float> sb(2), sx(2);
        const float zero_one[2] = {0.0f, 1.0f};
        const float guess[2] = {0.0f, 5.0f};
        sb.copyFromHost(zero_one, 2);
        sx.copyFromHost(guess, 2);
        GMRESConfig cfg;
        cfg.preconditioner = CGConfig::NONE;
        const GMRESResult r = gmres_solve(S, sb.get(), sx.get(), &cfg);
        float got[2] = {1.0f, 1.0f};
        sx.copyToHost(got, 2);
        CHECK(r.error_code == 0 && r.breakdown == GMRESResult::SINGULAR && r.iterations == 0 && r.converged == 0);
        CHECK(got[0] == 0.0f && got[1] == 5.0f);
        csr_destroy(S);
    }

    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CHECK(gmres_solve(nullptr, d_b.get(), d_x.get()).error_code == invalid_argument);
    CHECK(gmres_solve(A, d_b.get(), d_b.get()).error_code == invalid_argument);
    GMRESConfig bad;
    bad.restart = 65;
    CHECK(gmres_solve(A, d_b.get(), d_x.get(), &bad).error_code == invalid_argument);
    CHECK(gmres_solve_lu(A, nullptr, d_b.get(), d_x.get()).error_code == invalid_argument);
    csr_destroy(D);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
