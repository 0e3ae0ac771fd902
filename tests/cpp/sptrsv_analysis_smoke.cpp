// sptrsv_analysis_smoke.cpp — a C++ caller of sptrsv_analyze_device and sptrsv_schedule_get written against the
// installed headers only: `#include "spmv/*.h"`, namespace spmv, CudaBuffer.  On a 5-point Laplacian (48 x 48) it
// builds both schedules on the device, holds them to sptrsv_levels on the host arrays and to the host-built schedule
// int for int, then solves and factors on the device-built schedule.  Built with plain g++ against include/ and
// libspmv_amd.so by tests/test_gpu_sptrsv_analysis.py.  Needs a GPU.
#include "spmv/cuda_buffer.h"
#include "spmv/ic0.h"
#include "spmv/sptrsv.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static CSRMatrix* grid_matrix(int m) {
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

int main() {
    const int m = 48, n = m * m;
    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CSRMatrix* A = grid_matrix(m);
    CHECK(csr_to_gpu(A) == 0);
    for (int uplo = 0; uplo < 2; ++uplo) {
        std::vector<int> want_ptr(n + 1), want_order(n), got_ptr(n + 1, -1), got_order(n, -1), host_ptr(n + 1, -1),
            host_order(n, -1);
        int levels = 0, missing = 0;
        CHECK(sptrsv_levels(n, A->row_ptrs, A->col_indices, uplo, want_ptr.data(), want_order.data(), &levels,
                            &missing) == 0);
        SpTRSVScheduleInfo info{};
        CHECK(sptrsv_schedule_get(A, uplo, got_ptr.data(), got_order.data(), &info) == invalid_argument);
        CHECK(got_ptr[0] == -1 && got_order[0] == -1);

        const SpTRSVResult built = sptrsv_analyze_device(A, uplo);
        CHECK(built.error_code == 0 && built.analysis_ms > 0.0f && built.num_levels == levels);
        CHECK(sptrsv_analyze_device(A, uplo).analysis_ms == 0.0f);
        CHECK(sptrsv_analyze(A, uplo).analysis_ms == 0.0f);                   // the same cache
        CHECK(sptrsv_schedule_get(A, uplo, got_ptr.data(), got_order.data(), &info) == 0);
        CHECK(info.built_on_device == 1 && info.num_levels == levels && info.first_missing_diagonal == missing);
        CHECK(info.launches == built.launches && info.first_unsorted_row == -1 && info.one_sided_row == -1);
        CHECK(std::memcmp(got_ptr.data(), want_ptr.data(), (levels + 1) * sizeof(int)) == 0);
        CHECK(got_order == want_order);
        CHECK(sptrsv_schedule_get(A, uplo, nullptr, nullptr, nullptr) == 0);

        // a solve on the device-built schedule: the ordered rule, bit for bit
        std::vector<float> b(n), x(n), want(n);
        for (int i = 0; i < n; ++i) b[i] = 0.5f + static_cast<float>(i % 17);
        CudaBuffer<float> d_b(n), d_x(n);
        d_b.copyFromHost(b.data(), n);
        SpTRSVConfig cfg;
        cfg.uplo = uplo;
        cfg.ordered = 1;
        const SpTRSVResult solved = sptrsv_csr(A, d_b.get(), d_x.get(), &cfg);
        CHECK(solved.error_code == 0 && solved.analysis_ms == 0.0f && solved.launches == built.launches);
        d_x.copyToHost(x.data(), n);
        CHECK(sptrsv_cpu_csr(A, b.data(), want.data(), &cfg) == 0);
        CHECK(std::memcmp(x.data(), want.data(), n * sizeof(float)) == 0);

        // the host-built schedule of the same matrix
        csr_invalidate_gpu_cache(A);
        CHECK(sptrsv_schedule_get(A, uplo, nullptr, nullptr, nullptr) == invalid_argument);
        const SpTRSVResult host = sptrsv_analyze(A, uplo);
        SpTRSVScheduleInfo host_info{};
        CHECK(host.error_code == 0 && host.analysis_ms > 0.0f);
        CHECK(sptrsv_schedule_get(A, uplo, host_ptr.data(), host_order.data(), &host_info) == 0);
        CHECK(host_info.built_on_device == 0 && host_info.num_levels == info.num_levels &&
              host_info.launches == info.launches && host_info.triangle_nnz == info.triangle_nnz &&
              host_info.first_missing_diagonal == info.first_missing_diagonal &&
              host_info.first_unsorted_row == info.first_unsorted_row && host_info.one_sided_row == info.one_sided_row);
        CHECK(std::memcmp(host_ptr.data(), got_ptr.data(), (levels + 1) * sizeof(int)) == 0 && host_order == got_order);
        csr_invalidate_gpu_cache(A);
        std::printf("uplo %d: %d levels, %d launches, device analysis %.3f ms, host analysis %.3f ms\n", uplo,
                    built.num_levels, built.launches, built.analysis_ms, host.analysis_ms);
    }

    // IC(0) over a device-built LOWER schedule equals the host factor
    CHECK(sptrsv_analyze_device(A, SpTRSVConfig::LOWER).error_code == 0);
    CudaBuffer<float> d_l(A->nnz);
    const IC0Result factored = ic0_csr(A, d_l.get());
    CHECK(factored.error_code == 0 && factored.analysis_ms == 0.0f);
    std::vector<float> l(A->nnz), want_l(A->nnz);
    d_l.copyToHost(l.data(), l.size());
    int bad_pivot = 0;
    CHECK(ic0_cpu_csr(A, want_l.data(), &bad_pivot) == 0);
    CHECK(std::memcmp(l.data(), want_l.data(), l.size() * sizeof(float)) == 0);

    CHECK(sptrsv_analyze_device(nullptr, 0).error_code == invalid_argument);
    CHECK(sptrsv_analyze_device(A, 2).error_code == invalid_argument);
    CHECK(sptrsv_schedule_get(nullptr, 0, nullptr, nullptr, nullptr) == invalid_argument);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
