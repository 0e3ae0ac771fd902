// assemble_smoke.cpp — a C++ caller of the matrix assembly written the way the reference's tests are: `#include
// "spmv/*.h"`, namespace spmv, CudaBuffer.  Random triplets with repeats are assembled on the device in both modes and
// compared byte for byte with csr_from_coo_cpu; the values are refilled from a second array through the plan; and a
// CSR matrix goes back to triplets through csr_row_indices_gpu and comes back unchanged.  Built with plain g++ against
// include/ and libspmv_amd.so by tests/test_gpu_assemble.py.  Needs a GPU.
#include "spmv/assemble.h"
#include "spmv/cuda_buffer.h"
#include "spmv/test_utils.h"

#include <cstdio>
#include <cstring>
#include <vector>

using namespace spmv;
using namespace spmv::test;

static int g_failures = 0;
#define CHECK(cond) do { if (!(cond)) { ++g_failures; std::printf("FAIL %s:%d  %s\n", __FILE__, __LINE__, #cond); } } while (0)

static bool same(const CSRMatrix* got, const CSRMatrix* want) {
    if (got->num_rows != want->num_rows || got->num_cols != want->num_cols || got->nnz != want->nnz) return false;
    if (std::memcmp(got->row_ptrs, want->row_ptrs, sizeof(int) * (want->num_rows + 1)) != 0) return false;
    if (want->nnz == 0) return true;
    return std::memcmp(got->col_indices, want->col_indices, sizeof(int) * want->nnz) == 0 &&
           std::memcmp(got->values, want->values, sizeof(float) * want->nnz) == 0;
}

int main() {
    RandomGenerator rng(23);
    for (int iter = 0; iter < 8; ++iter) {
        const int rows = rng.randInt(1, 300), cols = rng.randInt(1, 300), n = rng.randInt(0, 20000);
        std::vector<int> r(n), c(n);
        std::vector<float> v(n), v2(n);
        for (int p = 0; p < n; ++p) {
            r[p] = rng.randInt(0, rows - 1);
            c[p] = rng.randInt(0, cols - 1);
            v[p] = rng.randFloat(-10.0f, 10.0f);
            v2[p] = rng.randFloat(-1e6f, 1e6f);
        }
        CudaBuffer<int> d_r(n), d_c(n);
        CudaBuffer<float> d_v(n), d_v2(n);
        if (n > 0) {
            d_r.copyFromHost(r.data(), n);
            d_c.copyFromHost(c.data(), n);
            d_v.copyFromHost(v.data(), n);
            d_v2.copyFromHost(v2.data(), n);
        }
        for (int mode : {static_cast<int>(COO_SUM), static_cast<int>(COO_KEEP)}) {
            CooConfig cfg;
            cfg.duplicates = mode;
            CSRMatrix* want = csr_create(0, 0, 0);
            CHECK(csr_from_coo_cpu(want, rows, cols, n, r.data(), c.data(), v.data(), &cfg) == 0);
            CSRMatrix* C = csr_create(0, 0, 0);
            CooPlan* plan = nullptr;
            const CooResult res = csr_from_coo_gpu(C, rows, cols, n, d_r.get(), d_c.get(), d_v.get(), &cfg, &plan);
            CHECK(res.error_code == 0 && plan != nullptr && res.nnz_out == want->nnz && res.combined == n - want->nnz);
            CHECK(res.tile_entries > 0 && C->owns_device_memory);
            CHECK(csr_from_gpu(C) == 0 && same(C, want));
            int p_rows = -1, p_cols = -1, p_n = -1, p_nnz = -1, p_mode = -1;
            CHECK(coo_plan_info(plan, &p_rows, &p_cols, &p_n, &p_nnz, &p_mode) == 0);
            CHECK(p_rows == rows && p_cols == cols && p_n == n && p_nnz == want->nnz && p_mode == mode);

            // new values into the same pattern
            CHECK(csr_from_coo_cpu(want, rows, cols, n, r.data(), c.data(), v2.data(), &cfg) == 0);
            CHECK(csr_coo_refill(plan, C, d_v2.get()) == 0);
            CHECK(csr_from_gpu(C) == 0 && same(C, want));
            CSRMatrix* wrong = csr_create(rows + 1, cols, 0);
            CHECK(csr_coo_refill(plan, wrong, d_v2.get()) == static_cast<int>(SpMVError::INVALID_DIMENSION));
            csr_destroy(wrong);

            // back to triplets and together again: the assembled matrix has sorted rows, so with COO_KEEP it returns
            CudaBuffer<int> d_back(C->nnz);
            CHECK(csr_row_indices_gpu(C, d_back.get()) == 0);
            CSRMatrix* again = csr_create(0, 0, 0);
            CooConfig keep;
            keep.duplicates = COO_KEEP;
            CHECK(csr_from_coo_gpu(again, rows, cols, C->nnz, d_back.get(), C->d_col_indices, C->d_values, &keep)
                      .error_code == 0);
            CHECK(csr_from_gpu(again) == 0 && same(again, want));
            csr_destroy(again);
            coo_plan_destroy(plan);
            csr_destroy(C);
            csr_destroy(want);
        }
    }
    coo_plan_destroy(nullptr);
    if (g_failures == 0) std::printf("all checks passed\n");
    return g_failures == 0 ? 0 : 1;
}
