// bsr_from_csr_cpu, bsr_to_csr_cpu, spmv_cpu_bsr and the BSR container (include/spmv/bsr.h, bsr_matrix.h) under
// AddressSanitizer + UndefinedBehaviorSanitizer: csrc/bsr_host.cpp and csrc/bsr_matrix.cpp are compiled into this
// executable with the sanitizers (make -C gpu-spmv_amd sanitize-bsr), every array below is a heap allocation of exactly
// its size, and the shapes are the ones whose last block row and block column are cut by the matrix's edge.  Run by
// tests/test_bsr_host.py; needs no GPU.
#include "spmv/bsr.h"

#include <algorithm>
#include <cstdio>
#include <cstring>
#include <limits>
#include <map>
#include <utility>
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
static const int kInvalidFormat = static_cast<int>(SpMVError::INVALID_FORMAT);

static bool same_bits(float x, float y) { return std::memcmp(&x, &y, sizeof(float)) == 0; }

// a deterministic sorted matrix: entry (i, j) is stored when (i * 7 + j * 3) % 5 < 2
static Host pattern(int rows, int cols) {
    std::vector<int> p{0}, c;
    std::vector<float> v;
    for (int i = 0; i < rows; ++i) {
        for (int j = 0; j < cols; ++j) {
            if ((i * 7 + j * 3) % 5 < 2) {
                c.push_back(j);
                v.push_back(static_cast<float>((i * 13 + j * 5) % 17 - 8) + 0.5f);
            }
        }
        p.push_back(static_cast<int>(c.size()));
    }
    return Host(rows, cols, p, c, v);
}

// the conversion by an ordered map of blocks, the product against spmv_cpu_csr, and the way back
static void expect_round_trip(Host& a, int b) {
    BSRMatrix* B = bsr_create(1, 1, 2, 1);
    CHECK(bsr_from_csr_cpu(B, &a.m, b) == 0);
    const int m = a.m.num_rows, n = a.m.num_cols;
    CHECK(B->num_rows == m && B->num_cols == n && B->block_dim == b && B->owns_host_memory);
    CHECK(B->num_block_rows == (m + b - 1) / b && B->num_block_cols == (n + b - 1) / b);
    std::map<std::pair<int, int>, std::vector<float>> want;
    for (int i = 0; i < m; ++i) {
        for (int p = a.ptr[i]; p < a.ptr[i + 1]; ++p) {
            std::vector<float>& block = want[{i / b, a.col[p] / b}];
            block.resize(static_cast<size_t>(b) * b, 0.0f);
            block[(i % b) * b + a.col[p] % b] = a.val[p];
        }
    }
    CHECK(B->num_blocks == static_cast<int>(want.size()));
    int at = 0, row = 0;
    for (const auto& kv : want) {
        while (row <= kv.first.first) CHECK(B->block_row_ptrs[row++] <= at);
        CHECK(at < B->num_blocks && B->block_cols[at] == kv.first.second);
        if (at < B->num_blocks) {
            for (int k = 0; k < b * b; ++k) CHECK(same_bits(B->values[static_cast<size_t>(at) * b * b + k], kv.second[k]));
        }
        ++at;
    }
    CHECK(B->block_row_ptrs[B->num_block_rows] == at);

    std::vector<float> x(n + 1), y_csr(m, -1.0f), y_bsr(m, -2.0f);    // (+ 1: spmv_cpu_csr returns at once for a null x)
    for (int j = 0; j < n; ++j) x[j] = static_cast<float>((j * 11) % 7 - 3) * 0.37f;
    spmv_cpu_csr(&a.m, x.data(), y_csr.data());
    spmv_cpu_bsr(B, x.data(), y_bsr.data());
    for (int i = 0; i < m; ++i) CHECK(same_bits(y_csr[i], y_bsr[i]));

    CSRMatrix* back = csr_create(1, 1, 1);
    CHECK(bsr_to_csr_cpu(back, B, 0) == 0 && back->nnz == a.m.nnz && back->num_rows == m && back->num_cols == n);
    if (back->nnz == a.m.nnz) {
        CHECK(std::memcmp(back->row_ptrs, a.ptr.data(), (static_cast<size_t>(m) + 1) * sizeof(int)) == 0);
        CHECK(a.m.nnz == 0 || std::memcmp(back->col_indices, a.col.data(), a.col.size() * sizeof(int)) == 0);
        CHECK(a.m.nnz == 0 || std::memcmp(back->values, a.val.data(), a.val.size() * sizeof(float)) == 0);
    }
    CHECK(bsr_to_csr_cpu(back, B, 1) == 0);
    long long inside = 0;
    for (int I = 0; I < B->num_block_rows; ++I) {
        for (int p = B->block_row_ptrs[I]; p < B->block_row_ptrs[I + 1]; ++p) {
            inside += static_cast<long long>(std::min(b, m - I * b)) * std::min(b, n - B->block_cols[p] * b);
        }
    }
    CHECK(back->nnz == inside);
    csr_destroy(back);
    bsr_destroy(B);
}

static void rejected(Host& a, int b, int code) {
    BSRMatrix* B = bsr_create(5, 7, 3, 0);
    CHECK(bsr_from_csr_cpu(B, &a.m, b) == code);
    CHECK(B->num_rows == 5 && B->num_cols == 7 && B->block_dim == 3 && B->num_blocks == 0 && B->block_row_ptrs[2] == 0);
    bsr_destroy(B);
}

int main() {
    const int dims[] = {2, 3, 4, 8};
    for (int b : dims) {
        const int shapes[][2] = {{1, 1}, {b, b}, {b + 1, 2 * b - 1}, {5 * b + 1, 6 * b}, {4 * b, 5 * b + b - 1}, {7 * b - 1, 9 * b + 1},
                                 {0, 5}, {5, 0}, {0, 0}, {37, 41}};
        for (const auto& s : shapes) {
            Host a = pattern(s[0], s[1]);
            expect_round_trip(a, b);
        }
        Host empty(3 * b, 2 * b, std::vector<int>(3 * b + 1, 0), {}, {});
        expect_round_trip(empty, b);
    }
    {   // special values arrive in place, padding is +0.0f, explicit zeros are entries of the block but not of the way back
        const float inf = std::numeric_limits<float>::infinity();
        Host a(3, 5, {0, 3, 4, 6}, {0, 1, 4, 2, 0, 3}, {-0.0f, 1e-40f, inf, 0.0f, 2.0f, -inf});
        BSRMatrix* B = bsr_create(0, 0, 2, 0);
        CHECK(bsr_from_csr_cpu(B, &a.m, 2) == 0 && B->num_blocks == 5);
        CHECK(same_bits(B->values[0], -0.0f) && same_bits(B->values[1], 1e-40f) && same_bits(B->values[2], 0.0f));
        CSRMatrix* back = csr_create(0, 0, 0);
        CHECK(bsr_to_csr_cpu(back, B, 0) == 0 && back->nnz == 4);          // -0.0f and 0.0f are dropped, 1e-40f is kept
        CHECK(bsr_to_csr_cpu(back, B, 1) == 0 && back->nnz == 2 * 5 + 4);    // rows 0 and 1 across all five columns, row 2 in two blocks
        csr_destroy(back);
        bsr_destroy(B);
    }

    // rejections, B untouched
    Host a(3, 4, {0, 1, 3, 4}, {0, 1, 3, 2}, {1, 2, 3, 4});
    for (int b : {0, 1, 5, 6, 7, 16, -2}) rejected(a, b, kInvalidArgument);
    { Host x(3, 4, {0, 1, 3, 4}, {0, 1, 1, 2}, {1, 2, 3, 4}); rejected(x, 2, kInvalidFormat); }       // equal pair
    { Host x(3, 4, {0, 1, 3, 4}, {0, 3, 1, 2}, {1, 2, 3, 4}); rejected(x, 3, kInvalidFormat); }       // descending pair
    { Host x(3, 4, {0, 1, 3, 4}, {0, 1, 4, 2}, {1, 2, 3, 4}); rejected(x, 4, kInvalidFormat); }       // column 4 of 4
    { Host x(3, 4, {0, 1, 3, 4}, {0, -1, 3, 2}, {1, 2, 3, 4}); rejected(x, 8, kInvalidFormat); }
    { Host x(3, 4, {0, 3, 1, 4}, {0, 1, 3, 2}, {1, 2, 3, 4}); rejected(x, 2, kInvalidFormat); }       // decreasing
    { Host x(3, 4, {0, 1, 3, 9}, {0, 1, 3, 2}, {1, 2, 3, 4}); rejected(x, 2, kInvalidFormat); }       // past nnz
    { Host x(3, 4, {0, 1, 3, 4}, {0, 1, 3, 2}, {1, 2, 3, 4}); x.m.values = nullptr; rejected(x, 2, kInvalidFormat); }
    {
        BSRMatrix* B = bsr_create(2, 2, 2, 0);
        CHECK(bsr_from_csr_cpu(nullptr, &a.m, 2) == kInvalidArgument);
        CHECK(bsr_from_csr_cpu(B, nullptr, 2) == kInvalidArgument);
        CHECK(bsr_from_csr_cpu(B, nullptr, 5) == kInvalidArgument);        // the null before the block size
        bsr_destroy(B);
        CHECK(bsr_create(-1, 2, 2, 0) == nullptr && bsr_create(2, 2, 5, 0) == nullptr && bsr_create(2, 2, 2, -1) == nullptr);
        CHECK(bsr_wrap_device(2, 2, 7, 0, nullptr, nullptr, nullptr) == nullptr);
        bsr_destroy(nullptr);
    }
    {   // BSR -> CSR: malformed block structures, A untouched
        CSRMatrix* A = csr_create(2, 3, 0);
        BSRMatrix* B = bsr_create(4, 6, 2, 3);
        const int ptr[] = {0, 2, 3}, col[] = {0, 2, 1};
        std::memcpy(B->block_row_ptrs, ptr, sizeof(ptr));
        std::memcpy(B->block_cols, col, sizeof(col));
        CHECK(bsr_to_csr_cpu(A, B, 1) == 0 && A->nnz == 12 && A->num_rows == 4 && A->num_cols == 6);
        CHECK(bsr_to_csr_cpu(A, B, 0) == 0 && A->nnz == 0 && A->row_ptrs[4] == 0);
        B->block_cols[1] = 3;                                              // block column 3 of 3
        CHECK(bsr_to_csr_cpu(A, B, 1) == kInvalidFormat && A->num_rows == 4);
        B->block_cols[1] = 0;                                              // not above its left neighbour
        CHECK(bsr_to_csr_cpu(A, B, 1) == kInvalidFormat);
        B->block_cols[1] = 2;
        B->block_row_ptrs[1] = 4;                                          // past the end
        CHECK(bsr_to_csr_cpu(A, B, 1) == kInvalidFormat);
        B->block_row_ptrs[1] = 2;
        B->num_block_cols = 2;                                             // a shape no BSR matrix has
        CHECK(bsr_to_csr_cpu(A, B, 1) == kInvalidFormat);
        B->num_block_cols = 3;
        CHECK(bsr_to_csr_cpu(nullptr, B, 1) == kInvalidArgument && bsr_to_csr_cpu(A, nullptr, 1) == kInvalidArgument);
        CHECK(bsr_to_csr_cpu(A, B, 1) == 0);
        bsr_destroy(B);
        csr_destroy(A);
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
