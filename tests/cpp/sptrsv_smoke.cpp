// sptrsv_smoke.cpp — a C++ caller of the sparse triangular solve, written against the installed headers only
// (`#include "spmv/sptrsv.h"`, namespace spmv, CudaBuffer, direct struct-field access) and built with plain g++
// against include/ and libspmv_amd.so.  Needs a GPU to run.
#include "spmv/sptrsv.h"
#include "spmv/cuda_buffer.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

// 5-point Laplacian on an m x m grid plus a weak non-symmetric coupling (i, i + 7), unsorted columns in some rows
static CSRMatrix* grid_matrix(int m) {
    const int n = m * m;
    std::vector<int> ptr(1, 0), col;
    std::vector<float> val;
    for (int i = 0; i < n; ++i) {
        const int gx = i % m, gy = i / m;
        if (i % 3 == 0 && i + 7 < n) { col.push_back(i + 7); val.push_back(0.25f); }
        if (gy > 0) { col.push_back(i - m); val.push_back(-1.0f); }
        if (gx > 0) { col.push_back(i - 1); val.push_back(-1.0f); }
        col.push_back(i); val.push_back(4.0f + 0.001f * static_cast<float>(i % 13));
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

int main() {
    const int m = 40, n = m * m;
    CSRMatrix* A = grid_matrix(m);
    CHECK(csr_to_gpu(A) == 0);
    std::vector<float> b(n), want(n), got(n);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * static_cast<float>(i)) + 0.1f;
    CudaBuffer<float> d_b(n), d_x(n);
    d_b.copyFromHost(b.data(), n);

    std::vector<int> level_ptr(n + 1), order(n);
    for (int uplo = 0; uplo < 2; ++uplo) {
        int levels = 0, missing = 0;
        CHECK(sptrsv_levels(n, A->row_ptrs, A->col_indices, uplo, level_ptr.data(), order.data(), &levels, &missing) == 0);
        CHECK(missing == -1 && levels >= 2 * m - 1 && level_ptr[levels] == n);
        const SpTRSVResult ahead = sptrsv_analyze(A, uplo);
        CHECK(ahead.error_code == 0 && ahead.analysis_ms > 0.0f && ahead.num_levels == levels);
        for (int diag = 0; diag < 2; ++diag) {
            SpTRSVConfig cfg;
            cfg.uplo = uplo;
            cfg.diag = diag;
            cfg.ordered = 1;
            CHECK(sptrsv_cpu_csr(A, b.data(), want.data(), &cfg) == 0);
            SpTRSVResult r = sptrsv_csr(A, d_b.get(), d_x.get(), &cfg);
            CHECK(r.error_code == 0 && r.analysis_ms == 0.0f && r.num_levels == levels && r.lanes_per_row == 1);
            CHECK(r.launches >= 1 && r.launches < r.num_levels);
            d_x.copyToHost(got.data(), n);
            CHECK(std::memcmp(got.data(), want.data(), n * sizeof(float)) == 0);      // bit for bit

            cfg.ordered = 0;                                                          // lanes may reorder the sums
            r = sptrsv_csr(A, d_b.get(), d_x.get(), &cfg);
            CHECK(r.error_code == 0 && r.lanes_per_row >= 1 && r.lanes_per_row <= 64);
            d_x.copyToHost(got.data(), n);
            bool close = true;
            for (int i = 0; i < n; ++i) close = close && std::fabs(got[i] - want[i]) <= 1e-4f * (1.0f + std::fabs(want[i]));
            CHECK(close);

            CudaBuffer<float> d_inplace(n);                                           // b == x
            d_inplace.copyFromHost(b.data(), n);
            cfg.ordered = 1;
            CHECK(sptrsv_csr(A, d_inplace.get(), d_inplace.get(), &cfg).error_code == 0);
            d_inplace.copyToHost(got.data(), n);
            CHECK(std::memcmp(got.data(), want.data(), n * sizeof(float)) == 0);
        }
    }

    // argument checks through the C++ entry points
    SpTRSVConfig bad;
    bad.uplo = 5;
    CHECK(sptrsv_csr(nullptr, d_b.get(), d_x.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(sptrsv_csr(A, d_b.get(), d_x.get(), &bad).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(sptrsv_csr(A, d_b.get(), d_b.get() + 1).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(sptrsv_csr_async(A, d_b.get(), d_x.get(), nullptr, nullptr) == 0);
    CHECK(hipDeviceSynchronize() == hipSuccess);
    csr_invalidate_gpu_cache(A);
    CHECK(sptrsv_csr(A, d_b.get(), d_x.get()).analysis_ms > 0.0f);

    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
