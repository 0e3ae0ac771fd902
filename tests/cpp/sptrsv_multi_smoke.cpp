// sptrsv_multi_smoke.cpp — a C++ caller of sptrsv_csr_multi and cg_solve_multi_ic written the way the reference's
// tests are: `#include "spmv/*.h"`, namespace spmv, CudaBuffer.  On a 2-D Poisson matrix (5-point, 40 x 40, with a weak
// non-symmetric coupling for the triangular solves) it solves k = 5 right-hand sides in one launch sequence, in a layout
// with padding (ldb = 5, ldx = 7) and in place, and checks every column against sptrsv_csr on that column bit for bit and
// the ordered solve against sptrsv_cpu_csr_multi; then IC-preconditioned CG for the five columns against cg_solve_ic
// column by column.  Built with plain g++ against include/ and libspmv_amd.so by tests/test_gpu_sptrsv_multi.py.  Needs
// a GPU.
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

// 5-point Laplacian on an m x m grid, columns ascending; with `skew`, a weak coupling (i, i + 7) on top
static CSRMatrix* grid_matrix(int m, bool skew) {
    const int n = m * m;
    std::vector<int> ptr(1, 0), col;
    std::vector<float> val;
    for (int i = 0; i < n; ++i) {
        const int gx = i % m, gy = i / m;
        if (gy > 0) { col.push_back(i - m); val.push_back(-1.0f); }
        if (gx > 0) { col.push_back(i - 1); val.push_back(-1.0f); }
        col.push_back(i); val.push_back(4.0f + (skew ? 0.001f * static_cast<float>(i % 13) : 0.0f));
        if (gx + 1 < m) { col.push_back(i + 1); val.push_back(-1.0f); }
        if (skew && i % 3 == 0 && i + 7 < n) { col.push_back(i + 7); val.push_back(0.25f); }
        if (gy + 1 < m) { col.push_back(i + m); val.push_back(-1.0f); }
        ptr.push_back(static_cast<int>(col.size()));
    }
    CSRMatrix* A = csr_create(n, n, static_cast<int>(col.size()));
    std::memcpy(A->row_ptrs, ptr.data(), ptr.size() * sizeof(int));
    std::memcpy(A->col_indices, col.data(), col.size() * sizeof(int));
    std::memcpy(A->values, val.data(), val.size() * sizeof(float));
    return A;
}

static int rows_that_differ(const std::vector<float>& X, int ld, int j, const std::vector<float>& x) {
    int differ = 0;
    for (size_t i = 0; i < x.size(); ++i) differ += std::memcmp(&X[i * ld + j], &x[i], sizeof(float)) != 0;
    return differ;
}

int main() {
    const int m = 40, n = m * m, k = 5, ldb = 5, ldx = 7;
    const float pad = -123.5f;
    std::vector<float> B(static_cast<size_t>(n) * ldb), X0(static_cast<size_t>(n) * ldx, pad), X(X0.size());
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j < k; ++j) B[i * ldb + j] = std::sin(0.37f * i + j) + 0.25f * j;
    }
    CudaBuffer<float> d_B(B.size()), d_X(X.size()), d_b(n), d_x(n);
    d_B.copyFromHost(B.data(), B.size());
    std::vector<float> b(n), x(n);

    // ---- the triangular solve
    CSRMatrix* T = grid_matrix(m, true);
    CHECK(csr_to_gpu(T) == 0);
    for (int uplo = 0; uplo < 2; ++uplo) {
        for (int ordered = 0; ordered < 2; ++ordered) {
            SpTRSVConfig cfg;
            cfg.uplo = uplo;
            cfg.ordered = ordered;
            d_X.copyFromHost(X0.data(), X0.size());
            const SpTRSVResult multi = sptrsv_csr_multi(T, d_B.get(), ldb, d_X.get(), ldx, k, &cfg);
            CHECK(multi.error_code == 0 && multi.launches >= 1);
            d_X.copyToHost(X.data(), X.size());
            for (int j = 0; j < k; ++j) {
                for (int i = 0; i < n; ++i) b[i] = B[i * ldb + j];
                d_b.copyFromHost(b.data(), n);
                const SpTRSVResult single = sptrsv_csr(T, d_b.get(), d_x.get(), &cfg);
                d_x.copyToHost(x.data(), n);
                CHECK(single.error_code == 0 && single.analysis_ms == 0.0f);         // the multi call's schedule
                CHECK(single.launches == multi.launches && single.num_levels == multi.num_levels &&
                      single.lanes_per_row == multi.lanes_per_row);
                CHECK(rows_that_differ(X, ldx, j, x) == 0);
            }
            int pad_written = 0;
            for (int i = 0; i < n; ++i) {
                for (int j = k; j < ldx; ++j) pad_written += X[i * ldx + j] != pad;
            }
            CHECK(pad_written == 0);
            if (ordered) {
                std::vector<float> want(B.size());
                CHECK(sptrsv_cpu_csr_multi(T, B.data(), ldb, want.data(), ldb, k, &cfg) == 0);
                int differ = 0;
                for (int i = 0; i < n; ++i) {
                    differ += std::memcmp(&want[i * ldb], &X[i * ldx], k * sizeof(float)) != 0;
                }
                CHECK(differ == 0);
            }
            // in place, through the async entry point
            CudaBuffer<float> d_Y(B.size());
            std::vector<float> Y(B.size());
            d_Y.copyFromHost(B.data(), B.size());
            CHECK(sptrsv_csr_multi_async(T, d_Y.get(), ldb, d_Y.get(), ldb, k, &cfg, nullptr) == 0);
            CHECK(hipDeviceSynchronize() == hipSuccess);
            d_Y.copyToHost(Y.data(), Y.size());
            int differ = 0;
            for (int i = 0; i < n; ++i) differ += std::memcmp(&Y[i * ldb], &X[i * ldx], k * sizeof(float)) != 0;
            CHECK(differ == 0);
            std::printf("uplo %d ordered %d: %d levels, %d launches, %d lanes, %.3f ms\n", uplo, ordered,
                        multi.num_levels, multi.launches, multi.lanes_per_row, multi.elapsed_ms);
        }
    }
    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CHECK(sptrsv_csr_multi(nullptr, d_B.get(), ldb, d_X.get(), ldx, k).error_code == invalid_argument);
    CHECK(sptrsv_csr_multi(T, d_B.get(), ldb, d_X.get(), ldx, 33).error_code == invalid_argument);
    CHECK(sptrsv_csr_multi(T, d_B.get(), 4, d_X.get(), ldx, k).error_code == invalid_argument);
    CHECK(sptrsv_csr_multi(T, d_B.get(), ldb, d_B.get(), ldb + 1, k).error_code == invalid_argument);
    CHECK(sptrsv_csr_multi(T, d_B.get(), ldb, d_B.get() + 3, ldb, k).error_code == invalid_argument);
    csr_destroy(T);

    // ---- IC-preconditioned CG
    CSRMatrix* A = grid_matrix(m, false);
    CHECK(csr_to_gpu(A) == 0);
    CudaBuffer<float> d_l(A->nnz);
    CHECK(ic0_csr(A, d_l.get()).error_code == 0);
    CSRMatrix wrap{};                                            // the factor over A's structure arrays: owns nothing
    wrap.num_rows = wrap.num_cols = n;
    wrap.nnz = A->nnz;
    wrap.d_row_ptrs = A->d_row_ptrs;
    wrap.d_col_indices = A->d_col_indices;
    wrap.d_values = d_l.get();
    const CSRMatrix* F = &wrap;
    for (int i = 0; i < n; ++i) {
        B[i * ldb + 2] = 0.0f;                                   // column 2: b = 0
        for (int j = 0; j < k; ++j) X0[i * ldx + j] = j == 1 ? 0.125f : 0.0f;
    }
    d_B.copyFromHost(B.data(), B.size());
    d_X.copyFromHost(X0.data(), X0.size());
    CGConfig cfg;
    cfg.tolerance = 1e-5f;
    cfg.engine = 0;
    CGResult results[5];
    CHECK(cg_solve_multi_ic(A, F, d_B.get(), ldb, d_X.get(), ldx, k, &cfg, results) == 0);
    d_X.copyToHost(X.data(), X.size());
    for (int j = 0; j < k; ++j) {
        for (int i = 0; i < n; ++i) {
            b[i] = B[i * ldb + j];
            x[i] = X0[i * ldx + j];
        }
        d_b.copyFromHost(b.data(), n);
        d_x.copyFromHost(x.data(), n);
        const CGResult ref = cg_solve_ic(A, F, d_b.get(), d_x.get(), &cfg);
        d_x.copyToHost(x.data(), n);
        const CGResult& r = results[j];
        CHECK(r.error_code == 0 && ref.error_code == 0 && r.converged == 1);
        CHECK(r.iterations == ref.iterations && r.converged == ref.converged && r.breakdown == ref.breakdown);
        CHECK(std::memcmp(&r.relative_residual, &ref.relative_residual, sizeof(float)) == 0);
        const int differ = rows_that_differ(X, ldx, j, x);
        CHECK(differ == 0);
        std::printf("cg_solve_multi_ic column %d: %d iterations, relative residual %.3g, %d rows differ\n", j,
                    r.iterations, r.relative_residual, differ);
    }
    CHECK(results[2].iterations == 0 && results[0].iterations > 0);
    CHECK(cg_solve_multi_ic(A, nullptr, d_B.get(), ldb, d_X.get(), ldx, k, &cfg, results) == invalid_argument);
    CHECK(results[4].error_code == invalid_argument);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
