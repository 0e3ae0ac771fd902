// cg_multi_smoke.cpp — a C++ caller of cg_solve_multi written the way the reference's tests are: `#include
// "spmv/*.h"`, namespace spmv, CudaBuffer.  Solves a 2-D Poisson system (5-point, 32 x 32) for k = 4 right-hand sides
// in one call, in a layout with padding (ldb = 4, ldx = 6), and checks every column against cg_solve(engine = 0) on
// that column alone: x bit for bit, the counters and flags, and the bits of relative_residual.  Then argument checks.
// Built with plain g++ against include/ and libspmv_amd.so by tests/test_gpu_cg_multi.py.  Needs a GPU.
#include "spmv/cg.h"
#include "spmv/cuda_buffer.h"
#include "spmv/spmv.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

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
    CSRMatrix* A = csr_create(n, n, static_cast<int>(ci.size()));
    for (int i = 0; i <= n; ++i) A->row_ptrs[i] = rp[i];
    for (size_t k = 0; k < ci.size(); ++k) {
        A->col_indices[k] = ci[k];
        A->values[k] = va[k];
    }
    return A;
}

int main() {
    CSRMatrix* A = poisson2d(32);
    const int n = A->num_rows, k = 4, ldb = 4, ldx = 6;
    CHECK(csr_to_gpu(A) == 0);
    const float pad = -123.5f;
    std::vector<float> B(static_cast<size_t>(n) * ldb), X0(static_cast<size_t>(n) * ldx, pad), X(X0.size());
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < k; ++j) {
            B[i * ldb + j] = j == 2 ? 0.0f : std::sin(0.37f * i + j) + 0.25f * j;      // column 2: b = 0
            X0[i * ldx + j] = j == 1 ? 0.125f : 0.0f;
        }
    }
    CudaBuffer<float> d_B(B.size()), d_X(X.size()), d_b(n), d_x(n);
    d_B.copyFromHost(B.data(), B.size());

    for (int pre : {CGConfig::NONE, CGConfig::JACOBI}) {
        CGConfig cfg;
        cfg.tolerance = 1e-5f;
        cfg.preconditioner = pre;
        cfg.engine = 0;
        d_X.copyFromHost(X0.data(), X0.size());
        CGResult results[4];
        CHECK(cg_solve_multi(A, d_B.get(), ldb, d_X.get(), ldx, k, &cfg, results) == 0);
        d_X.copyToHost(X.data(), X.size());
        for (int j = 0; j < k; ++j) {
            std::vector<float> b(n), x(n);
            for (int i = 0; i < n; ++i) {
                b[i] = B[i * ldb + j];
                x[i] = X0[i * ldx + j];
            }
            d_b.copyFromHost(b.data(), n);
            d_x.copyFromHost(x.data(), n);
            const CGResult ref = cg_solve(A, d_b.get(), d_x.get(), &cfg);
            d_x.copyToHost(x.data(), n);
            const CGResult& r = results[j];
            CHECK(r.error_code == 0 && ref.error_code == 0 && r.converged == 1);
            CHECK(r.iterations == ref.iterations && r.converged == ref.converged && r.breakdown == ref.breakdown);
            CHECK(std::memcmp(&r.relative_residual, &ref.relative_residual, sizeof(float)) == 0);
            CHECK(r.elapsed_ms == results[0].elapsed_ms);
            int differ = 0;
            for (int i = 0; i < n; ++i) differ += std::memcmp(&X[i * ldx + j], &x[i], sizeof(float)) != 0;
            CHECK(differ == 0);
            std::printf("preconditioner %d column %d: %d iterations, relative residual %.3g, %d rows differ\n", pre, j,
                        r.iterations, r.relative_residual, differ);
        }
        CHECK(results[2].iterations == 0 && results[0].iterations > 0);
        int pad_written = 0;
        for (int i = 0; i < n; ++i) {
            for (int j = k; j < ldx; ++j) pad_written += X[i * ldx + j] != pad;
        }
        CHECK(pad_written == 0);
    }

    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CGResult results[4];
    CHECK(cg_solve_multi(nullptr, d_B.get(), ldb, d_X.get(), ldx, k, nullptr, results) == invalid_argument);
    results[0].error_code = 77;
    CHECK(cg_solve_multi(A, d_B.get(), ldb, d_X.get(), ldx, 33, nullptr, results) == invalid_argument);
    CHECK(results[0].error_code == 77);      // k out of range: `results` is not touched
    CHECK(cg_solve_multi(A, d_B.get(), 3, d_X.get(), ldx, k, nullptr, results) == invalid_argument);
    CHECK(cg_solve_multi(A, d_B.get(), ldb, d_B.get(), ldb, k, nullptr, results) == invalid_argument);
    CGConfig tiled;
    tiled.engine = 1;
    CHECK(cg_solve_multi(A, d_B.get(), ldb, d_X.get(), ldx, k, &tiled, results) == invalid_argument);
    CHECK(results[3].error_code == invalid_argument);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
