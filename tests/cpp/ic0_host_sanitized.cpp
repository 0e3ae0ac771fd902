// ic0_cpu_csr (include/spmv/ic0.h) under AddressSanitizer + UndefinedBehaviorSanitizer: csrc/factor0_host.cpp is compiled
// into this executable with the sanitizers (make -C gpu-spmv_amd sanitize-ic0), every array below is a heap
// allocation of exactly its size, and the rejected inputs are the ones that would walk off an array if a check came
// too late.  Run by tests/test_ic0_host.py; needs no GPU.
#include "spmv/ic0.h"

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

static void rejected(Host& h, int code) {
    std::vector<float> out(h.val.size(), -77.0f);
    int pivot = 55;
    CHECK(ic0_cpu_csr(&h.m, out.data(), &pivot) == code);
    for (float v : out) CHECK(v == -77.0f);
}

// A = L L^T, L lower bidiagonal with diagonal 2 and sub-diagonal 1: every step is exact
static void tridiagonal(int n) {
    std::vector<int> ptr{0}, col;
    std::vector<float> val, want;
    for (int i = 0; i < n; ++i) {
        if (i > 0) col.push_back(i - 1), val.push_back(2.0f), want.push_back(1.0f);
        col.push_back(i), val.push_back(i > 0 ? 5.0f : 4.0f), want.push_back(2.0f);
        if (i + 1 < n) col.push_back(i + 1), val.push_back(-9.0f), want.push_back(1.0f);   // A's upper values are not read
        ptr.push_back(static_cast<int>(col.size()));
    }
    Host h(n, n, ptr, col, val);
    std::vector<float> out(val.size(), -77.0f);
    int pivot = 55;
    CHECK(ic0_cpu_csr(&h.m, out.data(), &pivot) == 0 && pivot == -1);
    CHECK(std::memcmp(out.data(), want.data(), want.size() * sizeof(float)) == 0);
    CHECK(ic0_cpu_csr(&h.m, h.val.data(), nullptr) == 0);                                   // in place, no pivot
    CHECK(std::memcmp(h.val.data(), want.data(), want.size() * sizeof(float)) == 0);
}

int main() {
    tridiagonal(1);
    tridiagonal(2);
    tridiagonal(300);
    {   // dense 3 x 3: [[4,2,2],[2,5,3],[2,3,6]] = L L^T, L = [[2,0,0],[1,2,0],[1,1,2]]
        Host h(3, 3, {0, 3, 6, 9}, {0, 1, 2, 0, 1, 2, 0, 1, 2}, {4, 2, 2, 2, 5, 3, 2, 3, 6});
        std::vector<float> out(9, -77.0f);
        int pivot = 55;
        CHECK(ic0_cpu_csr(&h.m, out.data(), &pivot) == 0 && pivot == -1);
        const float want[9] = {2, 1, 1, 1, 2, 1, 1, 1, 2};
        CHECK(std::memcmp(out.data(), want, sizeof(want)) == 0);
    }
    {   // indefinite at row 1: w_11 = 1 - 4 = -3, l_11 = NaN, reported and not an error
        Host h(2, 2, {0, 2, 4}, {0, 1, 0, 1}, {1, 2, 2, 1});
        std::vector<float> out(4, -77.0f);
        int pivot = 55;
        CHECK(ic0_cpu_csr(&h.m, out.data(), &pivot) == 0 && pivot == 1 && std::isnan(out[3]));
    }
    {   // no rows
        Host h(0, 0, {0}, {}, {});
        float nothing = -77.0f;
        int pivot = 55;
        CHECK(ic0_cpu_csr(&h.m, &nothing, &pivot) == 0 && pivot == -1 && nothing == -77.0f);
    }
    // rejections, the output untouched
    { Host h(2, 3, {0, 1, 2}, {0, 1}, {4, 4}); rejected(h, kInvalidDimension); }
    { Host h(3, 3, {0, 2, 4, 6}, {0, 1, 1, 0, 1, 2}, {4, 1, 4, 1, 1, 4}); rejected(h, kInvalidArgument); }      // unsorted
    { Host h(3, 3, {0, 2, 5, 6}, {0, 1, 0, 1, 1, 2}, {4, 1, 1, 2, 2, 4}); rejected(h, kInvalidArgument); }      // repeated
    { Host h(3, 3, {0, 2, 3, 5}, {0, 1, 0, 1, 2}, {4, 1, 1, 1, 4}); rejected(h, kInvalidArgument); }            // no (1,1)
    { Host h(3, 3, {0, 1, 3, 5}, {0, 0, 1, 1, 2}, {4, 1, 4, 1, 4}); rejected(h, kInvalidArgument); }            // (1,0), (2,1) one-sided
    { Host h(3, 3, {0, 2, 3, 4}, {0, 2, 1, 2}, {4, 1, 4, 4}); rejected(h, kInvalidArgument); }                  // (0,2) one-sided
    { Host h(3, 3, {0, 2, 4, 6}, {0, 1, 0, 1, 1, 7}, {4, 1, 1, 4, 1, 4}); rejected(h, kInvalidFormat); }        // column 7
    { Host h(3, 3, {0, 2, 4, 6}, {0, 1, 0, 1, -1, 2}, {4, 1, 1, 4, 1, 4}); rejected(h, kInvalidFormat); }
    { Host h(3, 3, {0, 4, 2, 6}, {0, 1, 0, 1, 1, 2}, {4, 1, 1, 4, 1, 4}); rejected(h, kInvalidFormat); }        // decreasing
    { Host h(3, 3, {0, 2, 4, 9}, {0, 1, 0, 1, 1, 2}, {4, 1, 1, 4, 1, 4}); rejected(h, kInvalidFormat); }        // past nnz
    { Host h(3, 3, {-1, 2, 4, 6}, {0, 1, 0, 1, 1, 2}, {4, 1, 1, 4, 1, 4}); rejected(h, kInvalidFormat); }
    {
        Host h(2, 2, {0, 1, 2}, {0, 1}, {4, 4});
        float out[2] = {-77.0f, -77.0f};
        CHECK(ic0_cpu_csr(nullptr, out, nullptr) == kInvalidArgument);
        CHECK(ic0_cpu_csr(&h.m, nullptr, nullptr) == kInvalidArgument);
        h.m.values = nullptr;
        CHECK(ic0_cpu_csr(&h.m, out, nullptr) == kInvalidArgument && out[0] == -77.0f);
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
