// bsr_smoke.cpp — a C++ caller of include/spmv/bsr.h written against the public headers and CudaBuffer only: a 2-D
// elasticity-like matrix (three unknowns per grid node, full 3x3 blocks) goes CSR -> BSR on the device, both SpMV
// kernels run on it, new values are refilled into the same pattern, and the matrix comes back as CSR.  Compiled by
// __graft_entry__.build(), run by tests/test_gpu_bsr.py.
#include "spmv/bsr.h"
#include "spmv/bsr_matrix.h"
#include "spmv/csr_matrix.h"
#include "spmv/cuda_buffer.h"
#include "spmv/spmv.h"

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

static bool same_bsr(const BSRMatrix* x, const BSRMatrix* y) {
    const size_t values = static_cast<size_t>(x->num_blocks) * x->block_dim * x->block_dim;
    return x->num_rows == y->num_rows && x->num_cols == y->num_cols && x->block_dim == y->block_dim &&
           x->num_blocks == y->num_blocks &&
           std::memcmp(x->block_row_ptrs, y->block_row_ptrs, sizeof(int) * (x->num_block_rows + 1)) == 0 &&
           std::memcmp(x->block_cols, y->block_cols, sizeof(int) * x->num_blocks) == 0 &&
           std::memcmp(x->values, y->values, sizeof(float) * values) == 0;
}

int main() {
    // a side x side grid, five-point coupling between nodes, b unknowns per node: every block is full
    const int side = 40, b = 3, nodes = side * side, n = nodes * b;
    CSRMatrix* A = csr_create(n, n, 0);
    std::vector<int> cols;
    std::vector<float> vals;
    for (int node = 0; node < nodes; ++node) {
        const int gi = node / side, gj = node % side;
        int near[5], count = 0;
        if (gi > 0) near[count++] = node - side;
        if (gj > 0) near[count++] = node - 1;
        near[count++] = node;
        if (gj + 1 < side) near[count++] = node + 1;
        if (gi + 1 < side) near[count++] = node + side;
        for (int r = 0; r < b; ++r) {
            for (int k = 0; k < count; ++k) {
                for (int c = 0; c < b; ++c) {
                    cols.push_back(near[k] * b + c);
                    vals.push_back(near[k] == node ? (r == c ? 8.0f : 0.5f) : -0.25f * static_cast<float>(1 + (r + c) % 3));
                }
            }
            A->row_ptrs[node * b + r + 1] = static_cast<int>(cols.size());
        }
    }
    CSRMatrix* filled = csr_create(n, n, static_cast<int>(cols.size()));
    std::memcpy(filled->row_ptrs, A->row_ptrs, sizeof(int) * (n + 1));
    std::memcpy(filled->col_indices, cols.data(), sizeof(int) * cols.size());
    std::memcpy(filled->values, vals.data(), sizeof(float) * vals.size());
    csr_destroy(A);
    A = filled;
    CHECK(csr_to_gpu(A) == 0);

    long long counted = -1;
    CHECK(csr_block_count_gpu(A, b, &counted) == 0 && counted * b * b == A->nnz);     // fill 1: worth converting

    BSRMatrix* B = bsr_create(0, 0, 2, 0);
    BSRMatrix* H = bsr_create(0, 0, 2, 0);
    BsrBuildResult res;
    CHECK(bsr_from_csr_gpu(B, A, b, &res) == 0 && res.error_code == 0 && res.num_blocks == counted);
    CHECK(res.fill == 1.0f && res.max_block_row == 5 && res.lanes >= 1 && res.launches >= 4);
    CHECK(B->num_rows == n && B->block_dim == b && B->num_block_rows == nodes && B->owns_device_memory);
    CHECK(bsr_from_gpu(B) == 0 && bsr_from_csr_cpu(H, A, b) == 0 && same_bsr(B, H));

    std::vector<float> x(n), want(n), bsr_want(n), y(n);
    for (int j = 0; j < n; ++j) x[j] = 0.25f * static_cast<float>((j * 7) % 13 - 6);
    spmv_cpu_csr(A, x.data(), want.data());
    spmv_cpu_bsr(H, x.data(), bsr_want.data());
    CHECK(std::memcmp(want.data(), bsr_want.data(), sizeof(float) * n) == 0);
    CudaBuffer<float> d_x(n), d_y(n);
    d_x.copyFromHost(x.data(), n);

    SpMVResult r = spmv_bsr(B, d_x.get(), d_y.get(), nullptr, n);                    // CPU order
    CHECK(r.error_code == 0 && r.y == d_y.get() && r.elapsed_ms > 0.0f && r.bandwidth_gb_s > 0.0f);
    d_y.copyToHost(y.data(), n);
    CHECK(std::memcmp(y.data(), want.data(), sizeof(float) * n) == 0);

    SpMVConfig lanes;
    lanes.kernel_type = SpMVConfig::VECTOR_CSR;
    r = spmv_bsr(B, d_x.get(), d_y.get(), &lanes, n);                                // the lane-group kernel
    CHECK(r.error_code == 0 && r.gflops > 0.0f);
    d_y.copyToHost(y.data(), n);
    for (int i = 0; i < n; ++i) CHECK(std::fabs(y[i] - want[i]) <= 1e-5f * 40.0f);    // sum |a||x| per row is below 40

    // a time step later: new values over the same pattern
    for (int p = 0; p < A->nnz; ++p) A->values[p] *= 1.5f;
    CHECK(csr_to_gpu(A) == 0);
    const int* structure = B->d_block_cols;
    CHECK(bsr_from_csr_numeric(B, A, &res) == 0 && res.launches == 1 && B->d_block_cols == structure);
    CHECK(bsr_from_gpu(B) == 0 && bsr_from_csr_cpu(H, A, b) == 0 && same_bsr(B, H));

    // and back
    CSRMatrix* back = csr_create(0, 0, 0);
    CHECK(bsr_to_csr_gpu(back, B, 0) == 0 && csr_from_gpu(back) == 0 && back->nnz == A->nnz);
    CHECK(std::memcmp(back->row_ptrs, A->row_ptrs, sizeof(int) * (n + 1)) == 0);
    CHECK(std::memcmp(back->col_indices, A->col_indices, sizeof(int) * A->nnz) == 0);
    CHECK(std::memcmp(back->values, A->values, sizeof(float) * A->nnz) == 0);

    csr_destroy(back);
    bsr_destroy(H);
    bsr_destroy(B);
    csr_destroy(A);
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
