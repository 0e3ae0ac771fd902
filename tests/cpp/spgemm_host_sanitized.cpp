// spgemm_cpu_csr (include/spmv/spgemm.h) under AddressSanitizer + UndefinedBehaviorSanitizer: csrc/spgemm_host.cpp is
// compiled into this executable with the sanitizers (make -C gpu-spmv_amd sanitize-spgemm), every array below is a
// heap allocation of exactly its size, and the rejected inputs are the ones that would walk off an array if a check
// came too late.  Run by tests/test_spgemm_host.py; needs no GPU.
#include "spmv/spgemm.h"

#include <climits>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
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

// the product by an ordered map per row, in the documented order
static void expect_product(Host& a, Host& b) {
    CSRMatrix* c = csr_create(1, 1, 1);
    CHECK(spgemm_cpu_csr(c, &a.m, &b.m) == 0);
    CHECK(c->num_rows == a.m.num_rows && c->num_cols == b.m.num_cols && c->owns_host_memory);
    int at = 0;
    for (int i = 0; i < a.m.num_rows; ++i) {
        std::map<int, float> acc;
        for (int p = a.ptr[i]; p < a.ptr[i + 1]; ++p) {
            const int k = a.col[p];
            for (int q = b.ptr[k]; q < b.ptr[k + 1]; ++q) {
                const float product = a.val[p] * b.val[q];
                auto it = acc.emplace(b.col[q], 0.0f).first;
                it->second = it->second + product;
            }
        }
        CHECK(c->row_ptrs[i] == at);
        for (const auto& kv : acc) {
            CHECK(at < c->nnz && c->col_indices[at] == kv.first &&
                  std::memcmp(&c->values[at], &kv.second, sizeof(float)) == 0);
            ++at;
        }
    }
    CHECK(c->row_ptrs[a.m.num_rows] == at && c->nnz == at);
    csr_destroy(c);
}

static void rejected(Host& a, Host& b, int code) {
    CSRMatrix* c = csr_create(2, 3, 0);
    CHECK(spgemm_cpu_csr(c, &a.m, &b.m) == code);
    CHECK(c->num_rows == 2 && c->num_cols == 3 && c->nnz == 0 && c->row_ptrs[2] == 0);
    csr_destroy(c);
}

int main() {
    {   // a small product with unsorted A, a repeated entry of A and a cancellation
        Host a(3, 4, {0, 3, 3, 6}, {2, 0, 2, 3, 1, 0}, {1.5f, -2.0f, 0.25f, 1.0f, 3.0f, -1.0f});
        Host b(4, 5, {0, 2, 4, 5, 7}, {0, 4, 1, 4, 2, 0, 3}, {1.0f, 2.0f, 3.0f, -1.0f, 0.5f, 1.0f, 7.0f});
        expect_product(a, b);
    }
    {   // a row that touches the last column, and only it
        Host a(2, 2, {0, 1, 2}, {1, 0}, {2.0f, 3.0f});
        Host b(2, 70000, {0, 1, 3}, {69999, 0, 69999}, {1.0f, 1.0f, -1.0f});
        expect_product(a, b);
    }
    {   // A = [1, -1], B = [[1], [1]]: the cancelled entry is stored as +0.0f
        Host a(1, 2, {0, 2}, {0, 1}, {1.0f, -1.0f});
        Host b(2, 1, {0, 1, 2}, {0, 0}, {1.0f, 1.0f});
        CSRMatrix* c = csr_create(0, 0, 0);
        CHECK(spgemm_cpu_csr(c, &a.m, &b.m) == 0 && c->nnz == 1 && c->col_indices[0] == 0);
        const float zero = 0.0f;
        CHECK(std::memcmp(&c->values[0], &zero, sizeof(float)) == 0);
        csr_destroy(c);
    }
    // the empty shapes
    { Host a(0, 3, {0}, {}, {}); Host b(3, 4, {0, 1, 1, 2}, {3, 0}, {1.0f, 2.0f}); expect_product(a, b); }
    { Host a(2, 3, {0, 1, 2}, {1, 1}, {1.0f, 2.0f}); Host b(3, 0, {0, 0, 0, 0}, {}, {}); expect_product(a, b); }
    { Host a(2, 0, {0, 0, 0}, {}, {}); Host b(0, 4, {0}, {}, {}); expect_product(a, b); }
    { Host a(2, 3, {0, 0, 0}, {}, {}); Host b(3, 4, {0, 1, 1, 2}, {3, 0}, {1.0f, 2.0f}); expect_product(a, b); }
    { Host a(2, 3, {0, 1, 2}, {1, 1}, {1.0f, 2.0f}); Host b(3, 4, {0, 1, 1, 2}, {3, 0}, {1.0f, 2.0f}); expect_product(a, b); }

    // rejections, C untouched
    Host a(2, 3, {0, 2, 3}, {0, 2, 1}, {1, 2, 3});
    Host b(3, 4, {0, 1, 3, 4}, {0, 1, 3, 2}, {1, 2, 3, 4});
    { Host w(2, 4, {0, 1, 2}, {0, 1}, {1, 1}); rejected(a, w, kInvalidDimension); }
    { Host x(3, 4, {0, 1, 3, 4}, {0, 1, 1, 2}, {1, 2, 3, 4}); rejected(a, x, kInvalidFormat); }       // equal pair
    { Host x(3, 4, {0, 1, 3, 4}, {0, 3, 1, 2}, {1, 2, 3, 4}); rejected(a, x, kInvalidFormat); }       // descending pair
    { Host x(3, 4, {0, 1, 3, 4}, {0, 1, 4, 2}, {1, 2, 3, 4}); rejected(a, x, kInvalidFormat); }       // column 4 of 4
    { Host x(3, 4, {0, 1, 3, 4}, {0, -1, 3, 2}, {1, 2, 3, 4}); rejected(a, x, kInvalidFormat); }
    { Host x(3, 4, {0, 3, 1, 4}, {0, 1, 3, 2}, {1, 2, 3, 4}); rejected(a, x, kInvalidFormat); }       // decreasing
    { Host x(3, 4, {0, 1, 3, 9}, {0, 1, 3, 2}, {1, 2, 3, 4}); rejected(a, x, kInvalidFormat); }       // past nnz
    { Host x(3, 4, {-1, 1, 3, 4}, {0, 1, 3, 2}, {1, 2, 3, 4}); rejected(a, x, kInvalidFormat); }
    { Host x(2, 3, {0, 2, 3}, {0, 3, 1}, {1, 2, 3}); rejected(x, b, kInvalidFormat); }                // A points past B
    { Host x(2, 3, {0, 2, 3}, {0, -2, 1}, {1, 2, 3}); rejected(x, b, kInvalidFormat); }
    { Host x(2, 3, {0, 4, 3}, {0, 2, 1}, {1, 2, 3}); rejected(x, b, kInvalidFormat); }
    {
        Host x(2, 3, {0, 2, 3}, {0, 2, 1}, {1, 2, 3});
        x.m.values = nullptr;
        rejected(x, b, kInvalidFormat);
    }
    {
        CSRMatrix* c = csr_create(2, 3, 0);
        CHECK(spgemm_cpu_csr(nullptr, &a.m, &b.m) == kInvalidArgument);
        CHECK(spgemm_cpu_csr(c, nullptr, &b.m) == kInvalidArgument);
        CHECK(spgemm_cpu_csr(c, &a.m, nullptr) == kInvalidArgument);
        CHECK(spgemm_cpu_csr(&a.m, &a.m, &b.m) == kInvalidArgument);
        CHECK(spgemm_cpu_csr(&b.m, &a.m, &b.m) == kInvalidArgument);
        csr_destroy(c);
    }
    CHECK(spgemm_class_capacity(0) == -1 && spgemm_class_capacity(1) > 0);
    int cls = 1;
    while (spgemm_class_capacity(cls) != INT_MAX && cls < 9) ++cls;
    CHECK(cls < 9 && spgemm_class_capacity(cls + 1) == -1);
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
