// eigs_smoke.cpp — a C++ caller of eigs_sym written the way the reference's tests are: `#include "spmv/*.h"`,
// namespace spmv, CudaBuffer.  The 5-point Laplacian of a 24 x 20 grid with the diagonal raised by 0.01 * row / n (a
// simple spectrum): the 4 largest and the 4 smallest eigenpairs, each checked against ||A y - theta y|| in fp64 on the
// host, the values printed for tests/test_gpu_eigs.py to compare with the Python call; then sym_eig_small on the host
// and on the device, an invariant subspace and the argument checks.  Built by build() with plain g++ against include/
// and libspmv_amd.so.  Needs a GPU.
#include "spmv/cuda_buffer.h"
#include "spmv/eigs.h"
#include "spmv/spmv.h"

#include <cmath>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;

static int g_failures = 0;
#define CHECK(cond) \
    do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static CSRMatrix* grid(int rows, int cols) {
    const int n = rows * cols;
    std::vector<int> rp(1, 0), ci;
    std::vector<float> va;
    for (int i = 0; i < rows; ++i) {
        for (int j = 0; j < cols; ++j) {
            const int row = i * cols + j;
            if (i > 0) { ci.push_back(row - cols); va.push_back(-1.0f); }
            if (j > 0) { ci.push_back(row - 1); va.push_back(-1.0f); }
            ci.push_back(row); va.push_back(4.0f + 0.01f * static_cast<float>(row) / static_cast<float>(n));
            if (j + 1 < cols) { ci.push_back(row + 1); va.push_back(-1.0f); }
            if (i + 1 < rows) { ci.push_back(row + cols); va.push_back(-1.0f); }
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

static double true_residual(const CSRMatrix* A, double theta, const float* y) {
    double sum = 0.0;
    for (int i = 0; i < A->num_rows; ++i) {
        double ay = 0.0;
        for (int k = A->row_ptrs[i]; k < A->row_ptrs[i + 1]; ++k) {
            ay += static_cast<double>(A->values[k]) * y[A->col_indices[k]];
        }
        sum += (ay - theta * y[i]) * (ay - theta * y[i]);
    }
    return std::sqrt(sum);
}

int main() {
    CSRMatrix* A = grid(24, 20);
    const int n = A->num_rows, k = 4;
    const long long ldv = n + 5;
    CHECK(csr_to_gpu(A) == 0);
    CudaBuffer<float> d_values(k), d_residuals(k), d_vectors(k * ldv);
    std::vector<float> values(k), residuals(k), vectors(k * ldv);
    for (int which = 0; which < 2; ++which) {
        EigsConfig cfg;
        cfg.num_values = k;
        cfg.which = which;
        cfg.engine = 0;
        const EigsResult r = eigs_sym(A, d_values.get(), d_vectors.get(), ldv, d_residuals.get(), nullptr, &cfg);
        CHECK(r.error_code == 0 && r.converged == k && r.breakdown == EigsResult::NONE);
        CHECK(r.iterations >= k && r.iterations <= 1000 && r.elapsed_ms > 0.0f);
        d_values.copyToHost(values.data(), k);
        d_residuals.copyToHost(residuals.data(), k);
        d_vectors.copyToHost(vectors.data(), k * ldv);
        for (int i = 0; i < k; ++i) {
            if (i > 0) CHECK(which == EigsConfig::LARGEST ? values[i - 1] > values[i] : values[i - 1] < values[i]);
            const double res = true_residual(A, values[i], vectors.data() + i * ldv);
            // the reported residual is the recomputed one: fp32 against fp64, a few units of fp32 rounding of the
            // row sums (|theta| <= 8, ||y|| = 1)
            CHECK(std::fabs(res - residuals[i]) <= 4e-6 && res <= 8.0 * 1.2e-5);
            CHECK(residuals[i] <= r.max_residual);
            std::printf("which %d value %d %.9g residual %.9g (true %.3g)\n", which, i, values[i], residuals[i], res);
        }
        std::printf("which %d: %d steps, %d restarts, %.3f ms\n", which, r.iterations, r.restarts, r.elapsed_ms);
    }
    // defaults (1 value, LARGEST, 1e-5) through a null config and without residuals
    CHECK(eigs_sym(A, d_values.get(), d_vectors.get(), ldv, nullptr, nullptr).converged == 1);

    // sym_eig_small: the device kernel and the host twin give the same bits
    {
        const int order = 33, ld = 35;
        std::vector<double> T(order * ld, 0.0), hv(order), hs(order * ld, 0.0), dv(order), ds(order * ld, 0.0);
        for (int i = 0; i < order; ++i) {
            for (int j = 0; j <= i; ++j) T[i * ld + j] = T[j * ld + i] = std::sin(1.0 + 3.0 * i + 0.7 * j * j);
        }
        CHECK(sym_eig_small(order, T.data(), ld, hv.data(), hs.data(), 0) == 0);
        CHECK(sym_eig_small(order, T.data(), ld, dv.data(), ds.data(), 1) == 0);
        CHECK(std::memcmp(hv.data(), dv.data(), order * sizeof(double)) == 0);
        CHECK(std::memcmp(hs.data(), ds.data(), order * ld * sizeof(double)) == 0);
    }
    // the identity: the space of any start vector is invariant after one step; one pair for three asked
    {
        const int m = 10;
        CSRMatrix* I = csr_create(m, m, m);
        for (int i = 0; i < m; ++i) {
            I->row_ptrs[i] = i;
            I->col_indices[i] = i;
            I->values[i] = 1.0f;
        }
        I->row_ptrs[m] = m;
        CHECK(csr_to_gpu(I) == 0);
        EigsConfig cfg;
        cfg.num_values = 3;
        const EigsResult r = eigs_sym(I, d_values.get(), d_vectors.get(), m, d_residuals.get(), nullptr, &cfg);
        d_values.copyToHost(values.data(), 3);
        CHECK(r.error_code == 0 && r.breakdown == EigsResult::INVARIANT_SUBSPACE && r.iterations == 1);
        CHECK(r.converged == 1 && std::fabs(values[0] - 1.0f) <= 1e-6f && std::isnan(values[1]) && std::isnan(values[2]));
        csr_destroy(I);
    }
    const int invalid_argument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
    CHECK(eigs_sym(nullptr, d_values.get(), d_vectors.get(), ldv, nullptr, nullptr).error_code == invalid_argument);
    CHECK(eigs_sym(A, d_values.get(), d_vectors.get(), n - 1, nullptr, nullptr).error_code == invalid_argument);
    EigsConfig bad;
    bad.num_values = 33;
    CHECK(eigs_sym(A, d_values.get(), d_vectors.get(), ldv, nullptr, nullptr, &bad).error_code == invalid_argument);
    csr_destroy(A);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
