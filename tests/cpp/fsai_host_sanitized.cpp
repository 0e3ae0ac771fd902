// fsai_cpu_csr (include/spmv/fsai.h) and the argument checks of fsai_csr / fsai_csr_numeric under AddressSanitizer +
// UndefinedBehaviorSanitizer: csrc/fsai_host.cpp is compiled into this executable with the sanitizers
// (make -C gpu-spmv_amd sanitize-fsai), every array below is a heap allocation of exactly its size, and the rejected
// inputs are the ones that would walk off an array if a check came too late.  Run by tests/test_fsai_host.py; needs no
// GPU.
#include "spmv/fsai.h"

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

static void rejected(Host& a, Host* s, int code) {
    CSRMatrix* G = csr_create(1, 1, 0);
    int bad = 55;
    CHECK(fsai_cpu_csr(G, &a.m, s ? &s->m : nullptr, &bad) == code);
    CHECK(G->num_rows == 1 && G->num_cols == 1 && G->nnz == 0 && bad == 55);
    csr_destroy(G);
}

// a dense m x m block A = L L^T, L = the all-ones lower triangle with 2 on the diagonal: G = L^-1 exactly
static void dense_block(int m) {
    std::vector<int> ptr{0}, col;
    std::vector<float> val;
    for (int i = 0; i < m; ++i) {
        for (int j = 0; j < m; ++j) {
            const int k = i < j ? i : j;                    // sum over the common columns: k ones, and the diagonal
            col.push_back(j);
            val.push_back(i == j ? static_cast<float>(k + 4) : static_cast<float>(k + 2));
        }
        ptr.push_back(static_cast<int>(col.size()));
    }
    Host h(m, m, ptr, col, val);
    CSRMatrix* G = csr_create(0, 0, 0);
    int bad = 55;
    CHECK(fsai_cpu_csr(G, &h.m, nullptr, &bad) == 0 && bad == -1);
    CHECK(G->num_rows == m && G->nnz == m * (m + 1) / 2);
    // L^-1: 1/2 on the diagonal, row i left of it -(1/2)^(i - j + 1)
    for (int i = 0; i < m && G->nnz == m * (m + 1) / 2; ++i) {
        for (int j = 0; j <= i; ++j) {
            const float g = G->values[G->row_ptrs[i] + j];
            CHECK(G->col_indices[G->row_ptrs[i] + j] == j);
            CHECK(g == (i == j ? 0.5f : -std::ldexp(1.0f, -(i - j + 1))));
        }
    }
    // the same matrix on the identity pattern, and into a G that holds something already
    std::vector<int> iptr, icol;
    for (int i = 0; i < m; ++i) iptr.push_back(i), icol.push_back(i);
    iptr.push_back(m);
    Host s(m, m, iptr, icol, std::vector<float>(m, 0.0f));
    s.m.values = nullptr;                                   // the pattern's values are never read
    CHECK(fsai_cpu_csr(G, &h.m, &s.m, nullptr) == 0 && G->nnz == m);
    for (int i = 0; i < m && G->nnz == m; ++i) {
        CHECK(G->values[i] == static_cast<float>(1.0 / std::sqrt(static_cast<double>(i + 4))));
    }
    csr_destroy(G);
}

int main() {
    dense_block(1);
    dense_block(2);
    dense_block(17);
    dense_block(64);
    {   // 65 entries in the last pattern row
        std::vector<int> ptr{0}, col;
        std::vector<float> val;
        for (int i = 0; i < 65; ++i) {
            for (int j = 0; j <= i; ++j) col.push_back(j), val.push_back(i == j ? 100.0f : 1.0f);
            ptr.push_back(static_cast<int>(col.size()));
        }
        Host h(65, 65, ptr, col, val);
        rejected(h, nullptr, kInvalidArgument);
    }
    {   // indefinite at row 1: w_11 = 1 - 4 = -3, g_11 = NaN, reported and not an error
        Host h(2, 2, {0, 2, 4}, {0, 1, 0, 1}, {1, 2, 2, 1});
        CSRMatrix* G = csr_create(0, 0, 0);
        int bad = 55;
        CHECK(fsai_cpu_csr(G, &h.m, nullptr, &bad) == 0 && bad == 1 && G->nnz == 3 && std::isnan(G->values[2]));
        csr_destroy(G);
    }
    {   // no rows
        Host h(0, 0, {0}, {}, {});
        CSRMatrix* G = csr_create(3, 3, 2);
        int bad = 55;
        CHECK(fsai_cpu_csr(G, &h.m, nullptr, &bad) == 0 && bad == -1 && G->num_rows == 0 && G->nnz == 0);
        csr_destroy(G);
    }
    // rejections, G untouched
    Host good(3, 3, {0, 2, 5, 7}, {0, 1, 0, 1, 2, 1, 2}, {4, 1, 1, 4, 1, 1, 4});
    { Host h(2, 3, {0, 1, 2}, {0, 1}, {4, 4}); rejected(h, nullptr, kInvalidDimension); }
    { Host s(2, 2, {0, 1, 2}, {0, 1}, {4, 4}); rejected(good, &s, kInvalidDimension); }
    { Host h(3, 3, {0, 2, 5, 7}, {0, 1, 1, 0, 2, 1, 2}, {4, 1, 4, 1, 1, 1, 4}); rejected(h, nullptr, kInvalidArgument); }  // unsorted
    { Host h(3, 3, {0, 2, 5, 7}, {0, 1, 0, 0, 2, 1, 2}, {4, 1, 1, 4, 1, 1, 4}); rejected(h, nullptr, kInvalidArgument); }  // repeated
    { Host s(3, 3, {0, 1, 2, 3}, {0, 0, 2}, {0, 0, 0}); rejected(good, &s, kInvalidArgument); }                            // no (1,1)
    { Host s(3, 3, {0, 1, 1, 2}, {0, 2}, {0, 0}); rejected(good, &s, kInvalidArgument); }                                  // empty row
    { Host h(3, 3, {0, 2, 5, 7}, {0, 1, 0, 1, 7, 1, 2}, {4, 1, 1, 4, 1, 1, 4}); rejected(h, nullptr, kInvalidFormat); }    // column 7
    { Host h(3, 3, {0, 2, 5, 7}, {0, 1, 0, -1, 2, 1, 2}, {4, 1, 1, 4, 1, 1, 4}); rejected(h, nullptr, kInvalidFormat); }
    { Host h(3, 3, {0, 5, 2, 7}, {0, 1, 0, 1, 2, 1, 2}, {4, 1, 1, 4, 1, 1, 4}); rejected(h, nullptr, kInvalidFormat); }    // decreasing
    { Host h(3, 3, {0, 2, 5, 9}, {0, 1, 0, 1, 2, 1, 2}, {4, 1, 1, 4, 1, 1, 4}); rejected(h, nullptr, kInvalidFormat); }    // past nnz
    { Host h(3, 3, {-1, 2, 5, 7}, {0, 1, 0, 1, 2, 1, 2}, {4, 1, 1, 4, 1, 1, 4}); rejected(h, nullptr, kInvalidFormat); }
    { Host s(3, 3, {0, 2, 5, 9}, {0, 1, 0, 1, 2, 1, 2}, {0, 0, 0, 0, 0, 0, 0}); rejected(good, &s, kInvalidFormat); }
    { Host s(3, 3, {0, 2, 5, 7}, {0, 1, 0, 1, 8, 1, 2}, {0, 0, 0, 0, 0, 0, 0}); rejected(good, &s, kInvalidFormat); }
    {
        CSRMatrix* G = csr_create(1, 1, 0);
        CHECK(fsai_cpu_csr(nullptr, &good.m, nullptr, nullptr) == kInvalidArgument);
        CHECK(fsai_cpu_csr(G, nullptr, nullptr, nullptr) == kInvalidArgument);
        CHECK(fsai_cpu_csr(&good.m, &good.m, nullptr, nullptr) == kInvalidArgument);
        Host h(3, 3, {0, 2, 5, 7}, {0, 1, 0, 1, 2, 1, 2}, {4, 1, 1, 4, 1, 1, 4});
        h.m.values = nullptr;
        CHECK(fsai_cpu_csr(G, &h.m, nullptr, nullptr) == kInvalidFormat);
        h.m.row_ptrs = nullptr;
        CHECK(fsai_cpu_csr(G, &good.m, &h.m, nullptr) == kInvalidFormat);
        // the device entry points return before they look at a device array
        CHECK(fsai_csr(nullptr, &good.m).error_code == kInvalidArgument);
        CHECK(fsai_csr(&good.m, &good.m).error_code == kInvalidArgument);
        CHECK(fsai_csr(G, &good.m).error_code == kInvalidFormat);                 // host arrays only
        CHECK(fsai_csr_numeric(G, nullptr).error_code == kInvalidArgument);
        CHECK(fsai_csr_numeric(G, &good.m).error_code == kInvalidDimension);
        CHECK(G->num_rows == 1 && G->nnz == 0);
        csr_destroy(G);
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
