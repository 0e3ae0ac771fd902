// amg_smoke.cpp — a C++ caller of the aggregation AMG and the AMG-preconditioned CG, written against the installed
// headers only (`#include "spmv/amg.h"`, namespace spmv, CudaBuffer, direct struct-field access) and built with plain
// g++ against include/ and libspmv_amd.so: set up, look at the levels, apply, solve, update, solve again.  Needs a GPU
// to run.
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

int main() {
    const int m = 32, n = m * m;
    CSRMatrix* A = laplacian(m);
    CHECK(csr_to_gpu(A) == 0);

    AMGHierarchy* H = nullptr;
    AMGResult s = amg_setup(&H, A);
    CHECK(s.error_code == 0 && H != nullptr && s.levels == 3 && s.coarse_solver == 0 && s.bad_row == -1);
    CHECK(s.grid_complexity > 1.0 && s.operator_complexity > 1.0 && s.setup_ms > 0.0f);
    CHECK(amg_num_levels(H) == 3);
    std::printf("levels %d, grid complexity %.3f, operator complexity %.3f, setup %.2f ms\n", s.levels,
                s.grid_complexity, s.operator_complexity, s.setup_ms);

    // level 0 is a view over A; the host aggregation of A gives level 0's map
    CSRMatrix view{};
    const int* d_agg = nullptr;
    int count = 0;
    CHECK(amg_level(H, 0, &view, &d_agg, &count) == 0);
    CHECK(view.d_values == A->d_values && view.d_row_ptrs == A->d_row_ptrs && view.num_rows == n && d_agg != nullptr);
    CHECK(!view.owns_device_memory && !view.owns_host_memory && view.values == nullptr);
    std::vector<int> agg(n), want(n);
    int want_count = 0;
    CHECK(hipMemcpy(agg.data(), d_agg, n * sizeof(int), hipMemcpyDeviceToHost) == hipSuccess);
    CHECK(amg_aggregate_cpu_csr(A, 0.08f, want.data(), &want_count) == 0 && want_count == count && agg == want);
    CSRMatrix next{};
    CHECK(amg_level(H, 1, &next, nullptr, nullptr) == 0 && next.num_rows == count && next.num_cols == count);
    CHECK(amg_level(H, 2, &next, &d_agg, &count) == 0 && d_agg == nullptr && count == 0 && next.num_rows <= 64);
    CHECK(amg_level(H, 3, &next, nullptr, nullptr) == static_cast<int>(SpMVError::INVALID_DIMENSION));

    std::vector<float> b(n), x(n, 0.0f), z(n), z2(n);
    for (int i = 0; i < n; ++i) b[i] = std::sin(0.37f * static_cast<float>(i)) + 0.1f;
    CudaBuffer<float> d_b(n), d_x(n), d_z(n);
    d_b.copyFromHost(b.data(), n);
    d_x.copyFromHost(x.data(), n);

    // one cycle is a fair approximation of the solve, and the same bits twice
    CHECK(amg_apply(H, d_b.get(), d_z.get()) == 0);
    d_z.copyToHost(z.data(), n);
    CHECK(amg_apply(H, d_b.get(), d_z.get()) == 0);
    d_z.copyToHost(z2.data(), n);
    CHECK(std::memcmp(z.data(), z2.data(), n * sizeof(float)) == 0);
    const double after_one_cycle = residual(A, b, z);
    CHECK(after_one_cycle < 1.0);
    CHECK(amg_apply(H, d_b.get(), d_b.get()) == static_cast<int>(SpMVError::INVALID_ARGUMENT));

    CGConfig cfg;
    cfg.tolerance = 1e-6f;
    cfg.engine = 0;
    cfg.preconditioner = 99;                                    // not read by cg_solve_amg
    const CGResult amg = cg_solve_amg(A, H, d_b.get(), d_x.get(), &cfg);
    CHECK(amg.error_code == 0 && amg.converged == 1 && amg.breakdown == 0 && amg.iterations >= 1);
    d_x.copyToHost(x.data(), n);
    CHECK(residual(A, b, x) <= 4e-6);

    std::vector<float> zero(n, 0.0f);
    d_x.copyFromHost(zero.data(), n);
    cfg.preconditioner = CGConfig::JACOBI;
    const CGResult jacobi = cg_solve(A, d_b.get(), d_x.get(), &cfg);
    CHECK(jacobi.error_code == 0 && jacobi.converged == 1);
    CHECK(2 * amg.iterations <= jacobi.iterations);
    std::printf("residual after one cycle %.3g; iterations: AMG %d, Jacobi %d\n", after_one_cycle, amg.iterations,
                jacobi.iterations);

    // new values in the same pattern: 2 A takes the same iterations (everything scales by a power of two; only the
    // fp64 Cholesky of the coarsest level may round another way)
    for (int j = 0; j < A->nnz; ++j) A->values[j] *= 2.0f;
    CHECK(hipMemcpy(A->d_values, A->values, A->nnz * sizeof(float), hipMemcpyHostToDevice) == hipSuccess);
    const AMGResult u = amg_update(H, A);
    CHECK(u.error_code == 0 && u.levels == 3);
    d_x.copyFromHost(zero.data(), n);
    const CGResult again = cg_solve_amg(A, H, d_b.get(), d_x.get(), &cfg);
    CHECK(again.error_code == 0 && again.converged == 1 && std::abs(again.iterations - amg.iterations) <= 1);

    // argument checks through the C++ entry points
    CHECK(cg_solve_amg(A, nullptr, d_b.get(), d_x.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    AMGConfig lopsided;
    lopsided.post_sweeps = 2;
    AMGHierarchy* L = nullptr;
    CHECK(amg_setup(&L, A, &lopsided).error_code == 0 && L != nullptr);
    CHECK(cg_solve_amg(A, L, d_b.get(), d_x.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CHECK(amg_apply(L, d_b.get(), d_z.get()) == 0);
    amg_destroy(L);

    amg_destroy(H);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
