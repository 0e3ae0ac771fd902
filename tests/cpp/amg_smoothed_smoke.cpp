// amg_smoothed_smoke.cpp — a C++ caller of smoothed-aggregation AMG, written against the installed headers only
// (`#include "spmv/amg.h"`, namespace spmv, CudaBuffer, direct struct-field access) and built with plain g++ against
// include/ and libspmv_amd.so: set up both ways, look at a level's transfers, restrict and prolong by hand, solve,
// update, solve again.  Needs a GPU to run.
#include "spmv/amg.h"
#include "spmv/cg.h"
#include "spmv/cuda_buffer.h"

#include <cmath>
#include <cstdlib>
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

template <typename T>
static std::vector<T> download(const T* device, int count) {
    std::vector<T> host(static_cast<size_t>(count));
    CHECK(hipMemcpy(host.data(), device, host.size() * sizeof(T), hipMemcpyDeviceToHost) == hipSuccess);
    return host;
}

int main() {
    const int m = 32, n = m * m;
    CSRMatrix* A = laplacian(m);
    CHECK(csr_to_gpu(A) == 0);

    AMGHierarchy* plain = nullptr;
    CHECK(amg_setup(&plain, A).error_code == 0 && amg_is_smoothed(plain) == 0);
    AMGHierarchy* H = nullptr;
    const AMGResult s = amg_setup_smoothed(&H, A);
    CHECK(s.error_code == 0 && H != nullptr && s.levels == 3 && s.coarse_solver == 0 && s.bad_row == -1);
    CHECK(amg_is_smoothed(H) == 1 && amg_num_levels(H) == 3);
    CHECK(s.grid_complexity > 1.0 && s.operator_complexity > 1.0 && s.operator_complexity < 2.0 && s.setup_ms > 0.0f);
    std::printf("levels %d, grid complexity %.3f, operator complexity %.3f, setup %.2f ms\n", s.levels,
                s.grid_complexity, s.operator_complexity, s.setup_ms);

    // level 0: the map is still the aggregate map, and P is amg_prolongator_cpu_csr of it, bit for bit
    CSRMatrix view{}, P{}, PT{};
    const int* d_agg = nullptr;
    int count = 0;
    CHECK(amg_level(H, 0, &view, &d_agg, &count) == 0 && view.d_values == A->d_values && d_agg != nullptr);
    CHECK(amg_level_transfer(H, 0, &P, &PT) == 0);
    CHECK(P.num_rows == n && P.num_cols == count && PT.num_rows == count && PT.num_cols == n && P.nnz == PT.nnz);
    CHECK(P.nnz > n && !P.owns_device_memory && P.values == nullptr);
    CHECK(amg_level_transfer(H, 2, &P, &PT) == static_cast<int>(SpMVError::INVALID_DIMENSION));
    const std::vector<int> agg = download(d_agg, n);
    std::vector<int> want_agg(n);
    int want_count = 0;
    CHECK(amg_aggregate_cpu_csr(A, 0.08f, want_agg.data(), &want_count) == 0 && want_count == count && agg == want_agg);
    CSRMatrix* host_P = csr_create(0, 0, 0);
    CHECK(amg_prolongator_cpu_csr(host_P, A, agg.data(), count, 2.0f / 3.0f) == 0 && host_P->nnz == P.nnz);
    if (host_P->nnz == P.nnz) {
        const std::vector<int> cols = download(P.d_col_indices, P.nnz);
        const std::vector<float> vals = download(P.d_values, P.nnz);
        CHECK(std::memcmp(cols.data(), host_P->col_indices, cols.size() * sizeof(int)) == 0);
        CHECK(std::memcmp(vals.data(), host_P->values, vals.size() * sizeof(float)) == 0);
    }
    csr_destroy(host_P);

    std::vector<float> b(n), x(n, 0.0f), z(n), z2(n);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * static_cast<float>(i)) + 0.1f;
    CudaBuffer<float> d_b(n), d_x(n), d_z(n), d_fc(count), d_e(count);
    d_b.copyFromHost(b.data(), n);
    d_x.copyFromHost(x.data(), n);

    // the transfers by hand: with x = 0 the restriction is P^T b, and prolonging it back adds P P^T b to x
    CHECK(amg_restrict(H, 0, d_b.get(), d_x.get(), d_fc.get()) == 0);
    CHECK(amg_prolong(H, 0, d_fc.get(), d_x.get()) == 0);
    d_x.copyToHost(z.data(), n);
    double ppt = 0.0;
    for (int i = 0; i < n; ++i) ppt += static_cast<double>(z[i]) * b[i];
    CHECK(ppt > 0.0);                                            // b^T P P^T b = |P^T b|^2
    CHECK(amg_restrict(H, 2, d_b.get(), d_x.get(), d_fc.get()) == static_cast<int>(SpMVError::INVALID_DIMENSION));
    CHECK(amg_restrict(H, 0, d_b.get(), d_x.get(), d_b.get()) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(amg_prolong(H, 0, nullptr, d_x.get()) == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    d_x.copyFromHost(x.data(), n);

    // one cycle is a better approximation of the solve than the plain cycle, and the same bits twice
    CHECK(amg_apply(H, d_b.get(), d_z.get()) == 0);
    d_z.copyToHost(z.data(), n);
    CHECK(amg_apply(H, d_b.get(), d_z.get()) == 0);
    d_z.copyToHost(z2.data(), n);
    CHECK(std::memcmp(z.data(), z2.data(), n * sizeof(float)) == 0);
    const double after_one_cycle = residual(A, b, z);
    CHECK(amg_apply(plain, d_b.get(), d_z.get()) == 0);
    d_z.copyToHost(z2.data(), n);
    const double after_one_plain_cycle = residual(A, b, z2);
    CHECK(after_one_cycle < after_one_plain_cycle && after_one_plain_cycle < 1.0);

    CGConfig cfg;
    cfg.tolerance = 1e-6f;
    cfg.engine = 0;
    const CGResult smoothed = cg_solve_amg(A, H, d_b.get(), d_x.get(), &cfg);
    CHECK(smoothed.error_code == 0 && smoothed.converged == 1 && smoothed.breakdown == 0 && smoothed.iterations >= 1);
    d_x.copyToHost(x.data(), n);
    CHECK(residual(A, b, x) <= 4e-6);
    std::vector<float> zero(n, 0.0f);
    d_x.copyFromHost(zero.data(), n);
    const CGResult unsmoothed = cg_solve_amg(A, plain, d_b.get(), d_x.get(), &cfg);
    CHECK(unsmoothed.error_code == 0 && unsmoothed.converged == 1 && smoothed.iterations < unsmoothed.iterations);
    std::printf("residual after one cycle: smoothed %.3g, plain %.3g; iterations: smoothed %d, plain %d\n",
                after_one_cycle, after_one_plain_cycle, smoothed.iterations, unsmoothed.iterations);

    // new values in the same pattern: 2 A takes the same iterations (everything scales by a power of two; only the
    // fp64 Cholesky of the coarsest level may round another way)
    for (int j = 0; j < A->nnz; ++j) A->values[j] *= 2.0f;
    CHECK(hipMemcpy(A->d_values, A->values, A->nnz * sizeof(float), hipMemcpyHostToDevice) == hipSuccess);
    const AMGResult u = amg_update(H, A);
    CHECK(u.error_code == 0 && u.levels == 3 && u.operator_complexity == s.operator_complexity);
    d_x.copyFromHost(zero.data(), n);
    const CGResult again = cg_solve_amg(A, H, d_b.get(), d_x.get(), &cfg);
    CHECK(again.error_code == 0 && again.converged == 1 && std::abs(again.iterations - smoothed.iterations) <= 1);

    // the device-side builder, and the argument checks through the C++ entry points
    AMGHierarchy* D = nullptr;
    AMGSmoothing sm;
    sm.prolongator_weight = 0.5f;
    const AMGResult d = amg_setup_smoothed_device(&D, A, nullptr, &sm, 7u);
    CHECK(d.error_code == 0 && D != nullptr && amg_is_smoothed(D) == 1 && d.levels >= 2 && amg_setup_rounds(D, 0) >= 1);
    d_x.copyFromHost(zero.data(), n);
    const CGResult on_device_built = cg_solve_amg(A, D, d_b.get(), d_x.get(), &cfg);
    CHECK(on_device_built.error_code == 0 && on_device_built.converged == 1);
    amg_destroy(D);
    sm.strength_decay = 0.0f;
    AMGHierarchy* bad = reinterpret_cast<AMGHierarchy*>(0x10);
    CHECK(amg_setup_smoothed(&bad, A, nullptr, &sm).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT) && bad == nullptr);

    amg_destroy(H);
    amg_destroy(plain);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
