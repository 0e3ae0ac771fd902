// multi_smoke.cpp — a C++ caller of spmv_csr_multi written the way the reference's tests are: `#include "spmv/*.h"`,
// namespace spmv, CudaBuffer.  Every column of Y is checked against spmv_cpu_csr on that column of X: bit for bit
// for SCALAR_CSR, within the reordered-sum bound for VECTOR_CSR / MERGE_PATH; padding columns stay untouched.
// Built with plain g++ against include/ and libspmv_amd.so by tests/test_gpu_spmv_multi.py.  Needs a GPU.
#include "spmv/spmv.h"
#include "spmv/bandwidth.h"
#include "spmv/cuda_buffer.h"
#include "spmv/test_utils.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;
using namespace spmv::test;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

// |got - want| <= 1e-5 * max(|want|, sum_j |a_ij x_j|)
static bool reordered_ok(const CSRMatrix* A, const float* x, const float* want, const float* got) {
    for (int i = 0; i < A->num_rows; ++i) {
        double abs_sum = 0.0;
        for (int j = A->row_ptrs[i]; j < A->row_ptrs[i + 1]; ++j) {
            abs_sum += std::fabs(static_cast<double>(A->values[j]) * x[A->col_indices[j]]);
        }
        const double scale = std::fmax(std::fabs(want[i]), abs_sum);
        if (std::fabs(static_cast<double>(want[i]) - got[i]) > 1e-5 * std::fmax(scale, 1e-30)) return false;
    }
    return true;
}

int main() {
    const uint32_t sentinel = 0x7FC0DEADu;
    RandomGenerator rng(7);
    for (int iter = 0; iter < 12; ++iter) {
        const int rows = rng.randInt(1, 300), cols = rng.randInt(1, 300);
        const int k = rng.randInt(1, 40);
        const int ldx = k + rng.randInt(0, 3), ldy = k + rng.randInt(0, 3);
        auto dense = generateRandomDenseMatrix(rows, cols, rng.randFloat(0.01f, 0.3f), rng);
        CSRMatrix* A = csr_create(0, 0, 0);
        csr_from_dense(A, dense.data(), rows, cols);
        CHECK(csr_to_gpu(A) == 0);

        std::vector<float> X(static_cast<size_t>(cols) * ldx);
        for (float& v : X) v = rng.randFloat(-1.0f, 1.0f);
        // the CPU path, one column at a time
        std::vector<std::vector<float>> want(k, std::vector<float>(rows));
        std::vector<std::vector<float>> xcol(k, std::vector<float>(cols));
        for (int j = 0; j < k; ++j) {
            for (int c = 0; c < cols; ++c) xcol[j][c] = X[static_cast<size_t>(c) * ldx + j];
            spmv_cpu_csr(A, xcol[j].data(), want[j].data());
        }

        CudaBuffer<float> d_X(X.size()), d_Y(static_cast<size_t>(rows) * ldy);
        d_X.copyFromHost(X.data(), X.size());
        std::vector<float> Y(static_cast<size_t>(rows) * ldy);
        for (auto kt : {SpMVConfig::SCALAR_CSR, SpMVConfig::VECTOR_CSR, SpMVConfig::MERGE_PATH}) {
            std::vector<uint32_t> init(Y.size(), sentinel);
            d_Y.copyFromHost(reinterpret_cast<const float*>(init.data()), init.size());
            SpMVConfig config;
            config.kernel_type = kt;
            const SpMVResult r = spmv_csr_multi(A, d_X.get(), ldx, d_Y.get(), ldy, k, &config, cols);
            CHECK(r.error_code == 0 && r.y == d_Y.get());
            d_Y.copyToHost(Y.data(), Y.size());
            std::vector<float> got(rows);
            for (int j = 0; j < k; ++j) {
                for (int i = 0; i < rows; ++i) got[i] = Y[static_cast<size_t>(i) * ldy + j];
                if (kt == SpMVConfig::SCALAR_CSR) {
                    CHECK(std::memcmp(got.data(), want[j].data(), rows * sizeof(float)) == 0);
                } else {
                    CHECK(reordered_ok(A, xcol[j].data(), want[j].data(), got.data()));
                }
            }
            for (int i = 0; i < rows; ++i) {
                for (int j = k; j < ldy; ++j) {
                    uint32_t bits;
                    std::memcpy(&bits, &Y[static_cast<size_t>(i) * ldy + j], sizeof(bits));
                    CHECK(bits == sentinel);
                }
            }
        }
        CHECK(spmv_csr_multi(A, d_X.get(), ldx, d_Y.get(), ldy, 0, nullptr).error_code ==
              static_cast<int>(SpMVError::INVALID_ARGUMENT));
        CHECK(spmv_csr_multi(A, d_X.get(), k - 1, d_Y.get(), ldy, k, nullptr).error_code ==
              static_cast<int>(SpMVError::INVALID_DIMENSION));
        csr_destroy(A);
    }
    const CSRMatrix* none = nullptr;
    CHECK(compute_bandwidth_csr_multi(none, 4, 1.0f).achieved_bandwidth_gb_s == 0.0f);
    std::printf(g_failures ? "multi_smoke: %d failure(s)\n" : "multi_smoke: all checks passed\n", g_failures);
    return g_failures ? 1 : 0;
}
