// The host side of smoothed aggregation (include/spmv/amg.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
// csrc/amg_host.cpp and the host twins amg_prolongator_cpu_csr calls (spgemm_host.cpp, csr_ops_host.cpp,
// csr_matrix.cpp) are compiled into this executable with the sanitizers (make -C gpu-spmv_amd sanitize-amg-smoothed),
// every array below is a heap allocation of exactly its size, and the rejected inputs are the ones that would walk
// off an array if a check came too late.  Run by tests/test_amg_smoothed_host.py; needs no GPU (every call returns
// before device work).
#include "spmv/amg.h"
#include "spmv/csr_ops.h"
#include "spmv/spgemm.h"

#include <cmath>
#include <cstdio>
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

// tridiag(-1, 2, -1)
static Host tridiagonal(int n) {
    std::vector<int> ptr(1, 0), col;
    std::vector<float> val;
    for (int i = 0; i < n; ++i) {
        if (i > 0) { col.push_back(i - 1); val.push_back(-1.0f); }
        col.push_back(i); val.push_back(2.0f);
        if (i + 1 < n) { col.push_back(i + 1); val.push_back(-1.0f); }
        ptr.push_back(static_cast<int>(col.size()));
    }
    return Host(n, n, ptr, col, val);
}

static void rejected(const CSRMatrix* A, const int* agg, int count, float weight, int code) {
    CSRMatrix* P = csr_create(1, 1, 1);
    P->row_ptrs[0] = 0; P->row_ptrs[1] = 1; P->col_indices[0] = 0; P->values[0] = 7.0f;
    CHECK(amg_prolongator_cpu_csr(P, A, agg, count, weight) == code);
    CHECK(P->num_rows == 1 && P->nnz == 1 && P->values[0] == 7.0f);
    csr_destroy(P);
}

int main() {
    {   // pairs, omega_p = 1/2: 3/4 in the row's own aggregate and 1/4 beside it
        Host a = tridiagonal(10);
        std::vector<int> agg(10);
        for (int i = 0; i < 10; ++i) agg[static_cast<size_t>(i)] = i / 2;
        CSRMatrix* P = csr_create(0, 0, 0);
        CHECK(amg_prolongator_cpu_csr(P, &a.m, agg.data(), 5, 0.5f) == 0);
        CHECK(P->num_rows == 10 && P->num_cols == 5 && P->nnz == 18);
        for (int i = 0; i < 10 && failures == 0; ++i) {
            for (int p = P->row_ptrs[i]; p < P->row_ptrs[i + 1]; ++p) {
                CHECK(P->values[p] == (P->col_indices[p] == i / 2 ? 0.75f : 0.25f));
                if (p > P->row_ptrs[i]) CHECK(P->col_indices[p] > P->col_indices[p - 1]);
            }
        }
        // a second call into the same P releases what the first one made
        CHECK(amg_prolongator_cpu_csr(P, &a.m, agg.data(), 5, 1.0f) == 0 && P->nnz == 18);
        csr_destroy(P);
    }
    {   // unsorted rows and a repeated column: the diagonal of row 1 is 3 + 1
        Host a(3, 3, {0, 3, 6, 8}, {1, 0, 1, 1, 0, 1, 2, 1}, {-1.0f, 4.0f, -0.5f, 3.0f, -1.5f, 1.0f, 4.0f, -2.0f});
        const std::vector<int> agg{0, 0, 1};
        CSRMatrix* P = csr_create(0, 0, 0);
        CHECK(amg_prolongator_cpu_csr(P, &a.m, agg.data(), 2, 2.0f / 3.0f) == 0);
        CHECK(P->num_rows == 3 && P->num_cols == 2 && P->nnz >= 3);
        for (int p = 0; p < P->nnz; ++p) CHECK(std::isfinite(P->values[p]) && P->col_indices[p] >= 0 && P->col_indices[p] < 2);
        csr_destroy(P);
    }
    {   // one row, one aggregate
        Host a(1, 1, {0, 1}, {0}, {3.0f});
        const std::vector<int> agg{0};
        CSRMatrix* P = csr_create(0, 0, 0);
        CHECK(amg_prolongator_cpu_csr(P, &a.m, agg.data(), 1, 0.5f) == 0 && P->nnz == 1 && P->values[0] == 0.5f);
        csr_destroy(P);
    }

    // rejections, P untouched
    Host good = tridiagonal(3);
    const std::vector<int> fine{0, 0, 1}, past{0, 0, 2}, negative{0, -1, 1};
    rejected(nullptr, fine.data(), 2, 0.5f, kInvalidArgument);
    rejected(&good.m, nullptr, 2, 0.5f, kInvalidArgument);
    CHECK(amg_prolongator_cpu_csr(nullptr, &good.m, fine.data(), 2, 0.5f) == kInvalidArgument);
    { Host x(2, 3, {0, 1, 2}, {0, 1}, {1, 1}); rejected(&x.m, fine.data(), 2, -1.0f, kInvalidDimension); }
    { Host x(3, 3, {0, 2, 3, 4}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(&x.m, fine.data(), 2, -1.0f, kInvalidFormat); }
    { Host x(3, 3, {0, 9, 3, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(&x.m, fine.data(), 2, 0.5f, kInvalidFormat); }
    { Host x(3, 3, {0, 2, 3, 5}, {0, 1, 1, 3, 2}, {2, -1, 2, -1, 2}); rejected(&x.m, fine.data(), 2, 0.5f, kInvalidFormat); }
    { Host x(3, 3, {0, 2, 3, 5}, {0, -1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(&x.m, fine.data(), 2, 0.5f, kInvalidFormat); }
    { Host x = tridiagonal(3); x.m.values = nullptr; rejected(&x.m, fine.data(), 2, 0.5f, kInvalidFormat); }
    for (float weight : {0.0f, 2.0f, -1.0f, NAN}) rejected(&good.m, fine.data(), 2, weight, kInvalidArgument);
    rejected(&good.m, fine.data(), 0, 0.5f, kInvalidArgument);
    rejected(&good.m, fine.data(), 1, 0.5f, kInvalidArgument);       // the map names aggregate 1
    rejected(&good.m, past.data(), 2, 0.5f, kInvalidArgument);
    rejected(&good.m, negative.data(), 2, 0.5f, kInvalidArgument);
    for (float diagonal : {0.0f, -2.0f, INFINITY, NAN}) {
        Host x = tridiagonal(3);
        x.val[3] = diagonal;                                          // row 1's (1, 1)
        rejected(&x.m, fine.data(), 2, 0.5f, kInvalidArgument);
    }
    { Host x(3, 3, {0, 2, 2, 4}, {0, 1, 1, 2}, {2, -1, -1, 2}); rejected(&x.m, fine.data(), 2, 0.5f, kInvalidArgument); }

    // amg_setup_smoothed's checks that come before any device work (the device pointers are never followed)
    {
        AMGHierarchy* H = reinterpret_cast<AMGHierarchy*>(0x10);
        CHECK(amg_setup_smoothed(&H, nullptr).error_code == kInvalidArgument && H == nullptr);
        CHECK(amg_setup_smoothed(nullptr, &good.m).error_code == kInvalidArgument);
        Host rect(2, 3, {0, 1, 2}, {0, 1}, {1, 1});
        CHECK(amg_setup_smoothed(&H, &rect.m).error_code == kInvalidDimension && H == nullptr);
        CHECK(amg_setup_smoothed(&H, &good.m).error_code == kInvalidFormat && H == nullptr);          // host arrays only
        int fake = 0;
        CSRMatrix dev = good.m;
        dev.d_row_ptrs = &fake;
        dev.d_col_indices = &fake;
        dev.d_values = reinterpret_cast<float*>(&fake);
        AMGConfig cfg;
        cfg.coarse_rows = 1025;
        AMGSmoothing sm;
        CHECK(amg_setup_smoothed(&H, &dev, &cfg, &sm).error_code == kInvalidArgument);
        cfg = AMGConfig();
        for (float weight : {0.0f, 2.0f, NAN}) {
            sm = AMGSmoothing();
            sm.prolongator_weight = weight;
            CHECK(amg_setup_smoothed(&H, &dev, &cfg, &sm).error_code == kInvalidArgument && H == nullptr);
        }
        for (float decay : {0.0f, 1.25f, -0.5f, NAN}) {
            sm = AMGSmoothing();
            sm.strength_decay = decay;
            CHECK(amg_setup_smoothed(&H, &dev, &cfg, &sm).error_code == kInvalidArgument && H == nullptr);
        }
        const std::vector<int> hole{0, 2, 2};
        const int* one[1] = {hole.data()};
        const AMGAggregates given{1, one};
        CHECK(amg_setup_smoothed(&H, &dev, nullptr, nullptr, &given).error_code == kInvalidArgument && H == nullptr);
        CHECK(amg_is_smoothed(nullptr) == 0);
        CHECK(amg_level_transfer(nullptr, 0, nullptr, nullptr) == kInvalidArgument);
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
