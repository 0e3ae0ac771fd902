// The host side of the aggregation AMG (include/spmv/amg.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
// csrc/amg_host.cpp is compiled into this executable with the sanitizers (make -C gpu-spmv_amd sanitize-amg), every
// array below is a heap allocation of exactly its size, and the rejected inputs are the ones that would walk off an
// array if a check came too late.  Run by tests/test_amg_host.py; needs no GPU (every call returns before device work).
#include "spmv/amg.h"
#include "spmv/cg.h"

#include <cmath>
#include <cstdio>
#include <set>
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

// 5-point Laplacian on an m x m grid
static Host laplacian(int m) {
    std::vector<int> ptr(1, 0), col;
    std::vector<float> val;
    for (int i = 0; i < m * m; ++i) {
        const int gx = i % m, gy = i / m;
        if (gy > 0) { col.push_back(i - m); val.push_back(-1.0f); }
        if (gx > 0) { col.push_back(i - 1); val.push_back(-1.0f); }
        col.push_back(i); val.push_back(4.0f);
        if (gx + 1 < m) { col.push_back(i + 1); val.push_back(-1.0f); }
        if (gy + 1 < m) { col.push_back(i + m); val.push_back(-1.0f); }
        ptr.push_back(static_cast<int>(col.size()));
    }
    return Host(m * m, m * m, ptr, col, val);
}

// every row in one aggregate, numbers dense, members of an aggregate connected through its first row
static void expect_partition(Host& a, float theta, int expected_count) {
    const int n = a.m.num_rows;
    std::vector<int> agg(static_cast<size_t>(n), -7);
    int count = -7;
    CHECK(amg_aggregate_cpu_csr(&a.m, theta, agg.data(), &count) == 0);
    CHECK(count >= 1 && count <= n);
    if (expected_count >= 0) CHECK(count == expected_count);
    std::set<int> seen;
    for (int i = 0; i < n; ++i) {
        CHECK(agg[i] >= 0 && agg[i] < count);
        seen.insert(agg[i]);
    }
    CHECK(static_cast<int>(seen.size()) == count);
    std::vector<int> again(static_cast<size_t>(n), -7);
    int count2 = -7;
    CHECK(amg_aggregate_cpu_csr(&a.m, theta, again.data(), &count2) == 0 && count2 == count && again == agg);
}

static void rejected(Host& a, float theta, int code) {
    std::vector<int> agg(static_cast<size_t>(a.m.num_rows > 0 ? a.m.num_rows : 1), -7);
    int count = -7;
    CHECK(amg_aggregate_cpu_csr(&a.m, theta, agg.data(), &count) == code);
    CHECK(count == -7);
    for (int v : agg) CHECK(v == -7);
}

int main() {
    { Host a = laplacian(16); expect_partition(a, 0.08f, 48); expect_partition(a, 0.0f, -1); expect_partition(a, 0.5f, 256); }
    { Host a = laplacian(5); expect_partition(a, 0.08f, -1); }
    {   // unsorted rows, a repeated column, a missing diagonal (counts as 0: everything non-zero is strong there)
        Host a(4, 4, {0, 3, 6, 8, 9}, {1, 0, 1, 0, 1, 3, 2, 3, 1},
               {-1.0f, 4.0f, -0.5f, -1.5f, 4.0f, -2.0f, 4.0f, 1.0f, -2.0f});
        expect_partition(a, 0.08f, -1);
    }
    { Host a(3, 3, {0, 1, 2, 3}, {0, 1, 2}, {1.0f, 2.0f, 3.0f}); expect_partition(a, 0.08f, 3); }
    { Host a(0, 0, {0}, {}, {}); std::vector<int> agg(1, -7); int count = -7;
      CHECK(amg_aggregate_cpu_csr(&a.m, 0.08f, agg.data(), &count) == 0 && count == 0 && agg[0] == -7); }
    {   // NaN and infinite values and diagonals: no comparison may index out of range
        Host a(3, 3, {0, 2, 4, 6}, {0, 1, 0, 1, 1, 2}, {NAN, -1.0f, -1.0f, INFINITY, -1.0f, 2.0f});
        expect_partition(a, 0.08f, -1);
    }

    // rejections, nothing written
    Host good(3, 3, {0, 2, 3, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2});
    { Host x(2, 3, {0, 1, 2}, {0, 1}, {1, 1}); rejected(x, 0.08f, kInvalidDimension); }
    { Host x(3, 3, {0, 2, 3, 4}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(x, 0.08f, kInvalidFormat); }
    { Host x(3, 3, {1, 2, 3, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(x, 0.08f, kInvalidFormat); }
    { Host x(3, 3, {0, 9, 3, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(x, 0.08f, kInvalidFormat); }
    { Host x(3, 3, {0, 3, 2, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(x, 0.08f, kInvalidFormat); }
    { Host x(3, 3, {0, 2, 3, 5}, {0, 1, 1, 3, 2}, {2, -1, 2, -1, 2}); rejected(x, 0.08f, kInvalidFormat); }
    { Host x(3, 3, {0, 2, 3, 5}, {0, -1, 1, 1, 2}, {2, -1, 2, -1, 2}); rejected(x, 0.08f, kInvalidFormat); }
    { Host x(3, 3, {0, 2, 3, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2}); x.m.values = nullptr; rejected(x, 0.08f, kInvalidFormat); }
    rejected(good, -0.25f, kInvalidArgument);
    rejected(good, NAN, kInvalidArgument);
    {
        int count = -7;
        std::vector<int> agg(3, -7);
        CHECK(amg_aggregate_cpu_csr(nullptr, 0.08f, agg.data(), &count) == kInvalidArgument);
        CHECK(amg_aggregate_cpu_csr(&good.m, 0.08f, nullptr, &count) == kInvalidArgument);
        CHECK(amg_aggregate_cpu_csr(&good.m, 0.08f, agg.data(), nullptr) == kInvalidArgument);
    }

    // amg_setup's checks that come before any device work (the matrices have no device arrays at all)
    {
        AMGHierarchy* H = reinterpret_cast<AMGHierarchy*>(0x10);
        CHECK(amg_setup(&H, nullptr).error_code == kInvalidArgument && H == nullptr);
        CHECK(amg_setup(nullptr, &good.m).error_code == kInvalidArgument);
        Host rect(2, 3, {0, 1, 2}, {0, 1}, {1, 1});
        CHECK(amg_setup(&H, &rect.m).error_code == kInvalidDimension && H == nullptr);
        Host none(0, 0, {0}, {}, {});
        CHECK(amg_setup(&H, &none.m).error_code == kInvalidDimension);
        CHECK(amg_setup(&H, &good.m).error_code == kInvalidFormat && H == nullptr);          // host arrays only
        int fake = 0;
        CSRMatrix dev = good.m;                    // device pointers that are never followed
        dev.d_row_ptrs = &fake;
        dev.d_col_indices = &fake;
        dev.d_values = reinterpret_cast<float*>(&fake);
        AMGConfig cfg;
        cfg.coarse_rows = 1025;
        CHECK(amg_setup(&H, &dev, &cfg).error_code == kInvalidArgument);
        cfg = AMGConfig();
        cfg.jacobi_weight = 2.0f;
        CHECK(amg_setup(&H, &dev, &cfg).error_code == kInvalidArgument);
        // caller-given maps: an entry out of range, an aggregate without members, a null map
        const std::vector<int> past{0, 1, 3}, hole{0, 2, 2}, fine{0, 0, 1}, second{0, 2};
        const int* one[1] = {past.data()};
        AMGAggregates given{1, one};
        CHECK(amg_setup(&H, &dev, nullptr, &given).error_code == kInvalidArgument);
        one[0] = hole.data();
        CHECK(amg_setup(&H, &dev, nullptr, &given).error_code == kInvalidArgument);
        one[0] = nullptr;
        CHECK(amg_setup(&H, &dev, nullptr, &given).error_code == kInvalidArgument);
        const int* two[2] = {fine.data(), second.data()};      // the second map is sized by the first: 2 entries
        given = AMGAggregates{2, two};
        CHECK(amg_setup(&H, &dev, nullptr, &given).error_code == kInvalidArgument && H == nullptr);
        given = AMGAggregates{-1, two};
        CHECK(amg_setup(&H, &dev, nullptr, &given).error_code == kInvalidArgument);
        CHECK(amg_update(nullptr, &dev).error_code == kInvalidArgument);
        CHECK(amg_num_levels(nullptr) == 0 && amg_level(nullptr, 0, nullptr, nullptr, nullptr) == kInvalidArgument);
        amg_destroy(nullptr);
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
