// cg_bsr_smoke.cpp — a C++ caller of cg_solve_bsr and the block-Jacobi routines written against the public headers and
// CudaBuffer only: a 2-D elasticity-like SPD matrix (three unknowns per grid node, full 3x3 blocks) goes CSR -> BSR on
// the device, the inverses of its diagonal blocks and their apply are compared with the host twins bit for bit, and
// A x = b is solved with all three preconditioners and checked by its true residual.  Compiled by
// __graft_entry__.build(), run by tests/test_gpu_cg_bsr.py.
#include "spmv/bsr.h"
#include "spmv/bsr_matrix.h"
#include "spmv/cg.h"
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

int main() {
    // a side x side grid, five-point coupling between nodes, b unknowns per node; symmetric and strictly diagonally
    // dominant (8 against 1 + 6), the unknowns of a node coupled by 3 off the diagonal of its block
    const int side = 40, b = 3, nodes = side * side, n = nodes * b;
    std::vector<int> ptr{0}, cols;
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
                    vals.push_back(near[k] == node ? (r == c ? 12.0f : 3.0f) : -0.25f * static_cast<float>(1 + (r + c) % 3));
                }
            }
            ptr.push_back(static_cast<int>(cols.size()));
        }
    }
    CSRMatrix* A = csr_create(n, n, static_cast<int>(cols.size()));
    std::memcpy(A->row_ptrs, ptr.data(), sizeof(int) * (n + 1));
    std::memcpy(A->col_indices, cols.data(), sizeof(int) * cols.size());
    std::memcpy(A->values, vals.data(), sizeof(float) * vals.size());
    CHECK(csr_to_gpu(A) == 0);
    BSRMatrix* B = bsr_create(0, 0, 2, 0);
    CHECK(bsr_from_csr_gpu(B, A, b) == 0 && bsr_from_gpu(B) == 0 && B->num_block_rows == nodes);

    // the inverses and their apply: device against host twin, bit for bit
    const size_t inv_count = static_cast<size_t>(nodes) * b * b;
    std::vector<float> inv(inv_count), inv_dev(inv_count), rhs(n), z(n), z_dev(n);
    for (int i = 0; i < n; ++i) rhs[i] = 0.125f * static_cast<float>((i * 7) % 13 - 6);
    CudaBuffer<float> d_inv(inv_count), d_b(n), d_x(n), d_z(n);
    d_b.copyFromHost(rhs.data(), n);
    CHECK(bsr_diag_inverse_cpu(B, inv.data()) == 0 && bsr_diag_inverse_gpu(B, d_inv.get()) == 0);
    d_inv.copyToHost(inv_dev.data(), inv_count);
    CHECK(std::memcmp(inv.data(), inv_dev.data(), sizeof(float) * inv_count) == 0);
    bsr_diag_apply_cpu(B, inv.data(), rhs.data(), z.data());
    CHECK(bsr_diag_apply(B, d_inv.get(), d_b.get(), d_z.get()) == 0);
    d_z.copyToHost(z_dev.data(), n);
    CHECK(std::memcmp(z.data(), z_dev.data(), sizeof(float) * n) == 0);

    // the three preconditioners
    std::vector<float> x(n), zero(n, 0.0f);
    std::vector<double> ax(n);
    int iterations[3] = {0, 0, 0};
    for (int precond : {CGConfig::NONE, CGConfig::JACOBI, CGConfig::BLOCK_JACOBI}) {
        CGConfig cfg;
        cfg.preconditioner = precond;
        cfg.tolerance = 1e-6f;
        d_x.copyFromHost(zero.data(), n);
        const CGResult res = cg_solve_bsr(B, d_b.get(), d_x.get(), &cfg);
        CHECK(res.error_code == 0 && res.converged == 1 && res.breakdown == 0 && res.iterations > 0);
        CHECK(res.relative_residual <= 1e-6f && res.elapsed_ms > 0.0f);
        iterations[precond] = res.iterations;
        d_x.copyToHost(x.data(), n);
        double rr = 0.0, bb = 0.0;
        for (int i = 0; i < n; ++i) {
            double s = 0.0;
            for (int p = A->row_ptrs[i]; p < A->row_ptrs[i + 1]; ++p) s += static_cast<double>(A->values[p]) * x[A->col_indices[p]];
            rr += (rhs[i] - s) * (rhs[i] - s);
            bb += static_cast<double>(rhs[i]) * rhs[i];
        }
        CHECK(std::sqrt(rr / bb) <= 4e-6);
    }
    CHECK(iterations[CGConfig::BLOCK_JACOBI] <= iterations[CGConfig::JACOBI]);
    std::printf("iterations: NONE %d JACOBI %d BLOCK_JACOBI %d\n", iterations[0], iterations[1], iterations[2]);

    CGConfig tiled;
    tiled.engine = 1;                                           // there is no tiled BSR engine
    CHECK(cg_solve_bsr(B, d_b.get(), d_x.get(), &tiled).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));
    CGConfig block;
    block.preconditioner = CGConfig::BLOCK_JACOBI;              // cg_solve keeps rejecting it
    CHECK(cg_solve(A, d_b.get(), d_x.get(), &block).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));

    bsr_destroy(B);
    csr_destroy(A);
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
