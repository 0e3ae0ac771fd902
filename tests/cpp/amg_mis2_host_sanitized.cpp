// amg_aggregate_mis2_cpu_csr (include/spmv/amg.h) under AddressSanitizer + UndefinedBehaviorSanitizer:
// csrc/amg_mis2_host.cpp is compiled into this executable with the sanitizers (make -C gpu-spmv_amd
// sanitize-amg-mis2), every array below is a heap allocation of exactly its size, and the rejected inputs are the ones
// that would walk off an array if a check came too late.  Run by tests/test_amg_mis2_host.py; needs no GPU.
#include "spmv/amg.h"

#include <cstdio>
#include <limits>
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

// vertex 0 joined to every other one
static Host star(int leaves) {
    std::vector<int> ptr(1, 0), col;
    std::vector<float> val;
    col.push_back(0); val.push_back(4.0f);
    for (int j = 1; j <= leaves; ++j) { col.push_back(j); val.push_back(-1.0f); }
    ptr.push_back(static_cast<int>(col.size()));
    for (int j = 1; j <= leaves; ++j) {
        col.push_back(0); val.push_back(-1.0f);
        col.push_back(j); val.push_back(2.0f);
        ptr.push_back(static_cast<int>(col.size()));
    }
    return Host(leaves + 1, leaves + 1, ptr, col, val);
}

// every row in one aggregate, the numbers dense, the round count within its bounds
static void expect_partition(Host& a, float theta, unsigned seed, int expected_count) {
    const int n = a.m.num_rows;
    std::vector<int> agg(static_cast<size_t>(n), -7);
    int count = -7, rounds = -7;
    CHECK(amg_aggregate_mis2_cpu_csr(&a.m, theta, seed, agg.data(), &count, &rounds) == 0);
    CHECK(count >= 1 && count <= n && rounds >= 1 && rounds <= n);
    if (expected_count >= 0) CHECK(count == expected_count);
    std::vector<char> used(static_cast<size_t>(count > 0 ? count : 1), 0);
    for (int i = 0; i < n; ++i) {
        CHECK(agg[i] >= 0 && agg[i] < count);
        if (agg[i] >= 0 && agg[i] < count) used[static_cast<size_t>(agg[i])] = 1;
    }
    for (int c = 0; c < count; ++c) CHECK(used[static_cast<size_t>(c)]);
    // the same ints from a second call, with and without the round count
    std::vector<int> again(static_cast<size_t>(n), -7);
    int count2 = -7;
    CHECK(amg_aggregate_mis2_cpu_csr(&a.m, theta, seed, again.data(), &count2, nullptr) == 0);
    CHECK(count2 == count && again == agg);
}

int main() {
    const unsigned seeds[] = {0u, 1u, 0xdeadbeefu};
    for (const unsigned seed : seeds) {
        Host grid = laplacian(9);
        expect_partition(grid, 0.08f, seed, -1);
        expect_partition(grid, 0.0f, seed, -1);
        expect_partition(grid, 0.5f, seed, 81);             // nothing is strong: all singletons
        Host wheel = star(130);
        expect_partition(wheel, 0.08f, seed, 1);            // one root reaches everything within two steps
        Host one(1, 1, {0, 1}, {0}, {3.0f});
        expect_partition(one, 0.08f, seed, 1);
        // unsorted rows, a repeated column, an explicit zero and a row without a diagonal
        Host messy(4, 4, {0, 4, 6, 9, 10}, {1, 0, 1, 3, 0, 1, 3, 2, 2, 0},
                   {-1.0f, 2.0f, -0.5f, 0.0f, -1.5f, 2.0f, -1.0f, 2.0f, 0.25f, -3.0f});
        expect_partition(messy, 0.08f, seed, -1);
    }

    // rejections, in the stated order, with nothing written
    Host a = laplacian(3);
    std::vector<int> agg(9, -7);
    int count = -7, rounds = -7;
    CHECK(amg_aggregate_mis2_cpu_csr(nullptr, 0.08f, 0u, agg.data(), &count, &rounds) == kInvalidArgument);
    CHECK(amg_aggregate_mis2_cpu_csr(&a.m, 0.08f, 0u, nullptr, &count, &rounds) == kInvalidArgument);
    CHECK(amg_aggregate_mis2_cpu_csr(&a.m, 0.08f, 0u, agg.data(), nullptr, &rounds) == kInvalidArgument);
    Host wide(2, 3, {0, 1, 2}, {0, 1}, {1.0f, 1.0f});
    CHECK(amg_aggregate_mis2_cpu_csr(&wide.m, -1.0f, 0u, agg.data(), &count, &rounds) == kInvalidDimension);
    Host short_end(3, 3, {0, 2, 3, 4}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2});
    Host late_start(3, 3, {1, 2, 3, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2});
    Host decreasing(3, 3, {0, 3, 2, 5}, {0, 1, 1, 1, 2}, {2, -1, 2, -1, 2});
    Host column_high(3, 3, {0, 2, 3, 5}, {0, 1, 1, 3, 2}, {2, -1, 2, -1, 2});
    Host column_low(3, 3, {0, 2, 3, 5}, {0, -1, 1, 1, 2}, {2, -1, 2, -1, 2});
    for (Host* bad : {&short_end, &late_start, &decreasing, &column_high, &column_low}) {
        CHECK(amg_aggregate_mis2_cpu_csr(&bad->m, -1.0f, 0u, agg.data(), &count, &rounds) == kInvalidFormat);
    }
    CSRMatrix no_host = a.m;
    no_host.row_ptrs = nullptr;
    CHECK(amg_aggregate_mis2_cpu_csr(&no_host, 0.08f, 0u, agg.data(), &count, &rounds) == kInvalidFormat);
    CHECK(amg_aggregate_mis2_cpu_csr(&a.m, -0.5f, 0u, agg.data(), &count, &rounds) == kInvalidArgument);
    CHECK(amg_aggregate_mis2_cpu_csr(&a.m, std::numeric_limits<float>::quiet_NaN(), 0u, agg.data(), &count, &rounds) ==
          kInvalidArgument);
    CHECK(count == -7 && rounds == -7);
    for (const int v : agg) CHECK(v == -7);

    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
