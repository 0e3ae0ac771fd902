// sptrsv_cpu_csr_multi (include/spmv/sptrsv.h) and the host-side checks of sptrsv_csr_multi under AddressSanitizer +
// UndefinedBehaviorSanitizer: csrc/sptrsv_host.cpp is compiled into this executable with the sanitizers (make -C
// gpu-spmv_amd sanitize-sptrsv-multi), every array below is a heap allocation of exactly its size (the last row of B
// and X ends at column k, not at the leading dimension), and the rejected inputs are the ones that would walk off an
// array if a check came too late.  Run by tests/test_sptrsv_multi_host.py; needs no GPU.
#include "spmv/sptrsv.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

using namespace spmv;

static int failures = 0;
#define CHECK(cond)                                                              \
    do {                                                                         \
        if (!(cond)) {                                                           \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);        \
            ++failures;                                                          \
        }                                                                        \
    } while (0)

struct Host {
    std::vector<int> ptr, col;
    std::vector<float> val;
    CSRMatrix m{};
    Host(int rows, int cols, std::vector<int> p, std::vector<int> c, std::vector<float> v)
        : ptr(std::move(p)), col(std::move(c)), val(std::move(v)) {
        m.num_rows = rows;
        m.num_cols = cols;
        m.nnz = static_cast<int>(col.size());
        m.row_ptrs = ptr.data();
        m.col_indices = col.data();
        m.values = val.data();
    }
};

static const int kInvalidArgument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
static const int kInvalidDimension = static_cast<int>(SpMVError::INVALID_DIMENSION);
static const int kInvalidFormat = static_cast<int>(SpMVError::INVALID_FORMAT);

// a full matrix with entries on both sides of the diagonal, in shuffled storage order, one repeated diagonal entry
static Host band(int n) {
    std::vector<int> ptr{0}, col;
    std::vector<float> val;
    for (int i = 0; i < n; ++i) {
        if (i + 2 < n) col.push_back(i + 2), val.push_back(0.25f + 0.01f * (i % 7));
        if (i > 0) col.push_back(i - 1), val.push_back(-0.5f - 0.03f * (i % 5));
        col.push_back(i), val.push_back(2.0f + 0.125f * (i % 3));
        if (i > 2) col.push_back(i - 3), val.push_back(0.375f);
        if (i % 4 == 1) col.push_back(i), val.push_back(0.5f);
        if (i + 1 < n) col.push_back(i + 1), val.push_back(-0.75f);
        ptr.push_back(static_cast<int>(col.size()));
    }
    return Host(n, n, ptr, col, val);
}

static size_t span(int n, int ld, int k) { return static_cast<size_t>(n - 1) * ld + k; }

static void columns_equal_the_single_solve(int n, int k, int ldb, int ldx) {
    Host h = band(n);
    for (int uplo = 0; uplo < 2; ++uplo) {
        for (int diag = 0; diag < 2; ++diag) {
            SpTRSVConfig cfg;
            cfg.uplo = uplo;
            cfg.diag = diag;
            std::vector<float> B(span(n, ldb, k), -55.0f), X(span(n, ldx, k), -77.0f);
            for (int i = 0; i < n; ++i) {
                for (int j = 0; j < k; ++j) B[static_cast<size_t>(i) * ldb + j] = std::sin(0.3f * i + j) + 0.1f * j;
            }
            const std::vector<float> B0 = B;
            CHECK(sptrsv_cpu_csr_multi(&h.m, B.data(), ldb, X.data(), ldx, k, &cfg) == 0);
            CHECK(std::memcmp(B.data(), B0.data(), B.size() * sizeof(float)) == 0);
            for (int j = 0; j < k; ++j) {
                std::vector<float> b(n), x(n, -1.0f);
                for (int i = 0; i < n; ++i) b[i] = B[static_cast<size_t>(i) * ldb + j];
                CHECK(sptrsv_cpu_csr(&h.m, b.data(), x.data(), &cfg) == 0);
                int differ = 0;
                for (int i = 0; i < n; ++i) differ += std::memcmp(&x[i], &X[static_cast<size_t>(i) * ldx + j], 4) != 0;
                CHECK(differ == 0);
            }
            for (int i = 0; i + 1 < n; ++i) {
                for (int j = k; j < ldx; ++j) CHECK(X[static_cast<size_t>(i) * ldx + j] == -77.0f);
            }
            if (ldb == ldx) {           // in place
                std::vector<float> Y = B;
                CHECK(sptrsv_cpu_csr_multi(&h.m, Y.data(), ldb, Y.data(), ldb, k, &cfg) == 0);
                for (int i = 0; i < n; ++i) {
                    CHECK(std::memcmp(&Y[static_cast<size_t>(i) * ldb], &X[static_cast<size_t>(i) * ldx], 4 * k) == 0);
                }
            }
        }
    }
}

int main() {
    for (int k : {1, 3, 4, 5, 8, 9, 32}) {
        columns_equal_the_single_solve(1, k, k, k);
        columns_equal_the_single_solve(37, k, k, k);
        columns_equal_the_single_solve(37, k, k + 3, k + 1);
        columns_equal_the_single_solve(300, k, k + 2, k + 2);
    }
    {   // no rows: nothing is read or written
        Host h(0, 0, {0}, {}, {});
        float b = -55.0f, x = -77.0f;
        CHECK(sptrsv_cpu_csr_multi(&h.m, &b, 4, &x, 4, 4) == 0 && x == -77.0f);
    }
    // rejections, X untouched: the arrays hold exactly the span of a 3 x 2 system with ld = 2
    const auto rejected = [](Host& h, int ldb, int ldx, int k, int code) {
        std::vector<float> B(8, 1.0f), X(8, -77.0f);
        CHECK(sptrsv_cpu_csr_multi(&h.m, B.data(), ldb, X.data(), ldx, k) == code);
        for (float v : X) CHECK(v == -77.0f);
    };
    { Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4}); rejected(h, 2, 2, 0, kInvalidArgument); }
    { Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4}); rejected(h, 2, 2, 33, kInvalidArgument); }
    { Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4}); rejected(h, 1, 2, 2, kInvalidArgument); }
    { Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4}); rejected(h, 2, 1, 2, kInvalidArgument); }
    { Host h(2, 3, {0, 1, 2}, {0, 1}, {4, 4}); rejected(h, 2, 2, 2, kInvalidDimension); }
    { Host h(2, 3, {0, 1, 2}, {0, 1}, {4, 4}); rejected(h, 2, 2, 40, kInvalidArgument); }                       // k first
    { Host h(3, 3, {0, 1, 2, 4}, {0, 0, 1, 2}, {4, 1, 1, 4}); rejected(h, 2, 2, 2, kInvalidArgument); }         // no (1,1)
    { Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 7}, {4, 1, 4, 1, 4}); rejected(h, 2, 2, 2, kInvalidFormat); }     // column 7
    { Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, -1, 2}, {4, 1, 4, 1, 4}); rejected(h, 2, 2, 2, kInvalidFormat); }
    { Host h(3, 3, {0, 3, 1, 5}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4}); rejected(h, 2, 2, 2, kInvalidFormat); }     // decreasing
    { Host h(3, 3, {0, 1, 3, 9}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4}); rejected(h, 2, 2, 2, kInvalidFormat); }     // past nnz
    {
        Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4});
        std::vector<float> S(16, -77.0f);
        CHECK(sptrsv_cpu_csr_multi(nullptr, S.data(), 2, S.data() + 8, 2, 2) == kInvalidArgument);
        CHECK(sptrsv_cpu_csr_multi(&h.m, nullptr, 2, S.data(), 2, 2) == kInvalidArgument);
        CHECK(sptrsv_cpu_csr_multi(&h.m, S.data(), 2, nullptr, 2, 2) == kInvalidArgument);
        // overlap: the same array with another leading dimension, and a shifted one
        CHECK(sptrsv_cpu_csr_multi(&h.m, S.data(), 2, S.data(), 3, 2) == kInvalidArgument);
        CHECK(sptrsv_cpu_csr_multi(&h.m, S.data(), 2, S.data() + 5, 2, 2) == kInvalidArgument);
        CHECK(sptrsv_cpu_csr_multi(&h.m, S.data() + 5, 2, S.data(), 2, 2) == kInvalidArgument);
        for (float v : S) CHECK(v == -77.0f);
        CHECK(sptrsv_cpu_csr_multi(&h.m, S.data(), 2, S.data() + 6, 2, 2) == 0);                // 6 floats each: disjoint
        // the device entry points return before any device work
        CHECK(sptrsv_csr_multi(nullptr, S.data(), 2, S.data() + 8, 2, 2).error_code == kInvalidArgument);
        CHECK(sptrsv_csr_multi(&h.m, S.data(), 2, S.data() + 8, 2, 0).error_code == kInvalidArgument);
        CHECK(sptrsv_csr_multi(&h.m, S.data(), 1, S.data() + 8, 2, 2).error_code == kInvalidArgument);
        CHECK(sptrsv_csr_multi(&h.m, S.data(), 2, S.data() + 8, 2, 2).error_code == kInvalidFormat);   // host only
        CHECK(sptrsv_csr_multi_async(&h.m, S.data(), 2, S.data() + 8, 2, 33, nullptr, nullptr) == kInvalidArgument);
        h.m.values = nullptr;
        CHECK(sptrsv_cpu_csr_multi(&h.m, S.data(), 2, S.data() + 8, 2, 2) == kInvalidArgument);
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
