// bsr_ic_smoke.cpp — a C++ caller of bsr_ic0, sptrsv_bsr and cg_solve_bsr_ic written against the public headers and
// CudaBuffer only: a 2-D elasticity-like SPD matrix (three unknowns per grid node, full 3x3 blocks) goes CSR -> BSR on
// the device, its block IC(0) factor is compared with the host twin bit for bit, the ordered solves with theirs, and
// A x = b is solved with the factor and with BLOCK_JACOBI and checked by its true residual.  Compiled by
// __graft_entry__.build(), run by tests/test_gpu_bsr_ic.py.
#include "spmv/bsr.h"
#include "spmv/bsr_factor.h"
#include "spmv/bsr_matrix.h"
#include "spmv/cg.h"
#include "spmv/csr_matrix.h"
#include "spmv/cuda_buffer.h"

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
    // a side x side grid, five-point coupling between nodes, b unknowns per node: (Laplacian) (x) K + 0.05 I with
    // K[r][c] = min(r, c) + 1, weakly dominant, the unknowns of a node strongly coupled
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
                    const float kk = static_cast<float>((r < c ? r : c) + 1);
                    cols.push_back(near[k] * b + c);
                    vals.push_back(near[k] == node ? static_cast<float>(count - 1) * kk + (r == c ? 0.05f : 0.0f) : -kk);
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

    // the factor: device against host twin, bit for bit
    const size_t count = static_cast<size_t>(B->num_blocks) * b * b;
    std::vector<float> f(count), f_dev(count);
    int bad = 7;
    CHECK(bsr_ic0_cpu(B, f.data(), &bad) == 0 && bad == -1);
    CudaBuffer<float> d_f(count), d_b(n), d_x(n), d_y(n);
    const BsrIC0Result fr = bsr_ic0(B, d_f.get());
    CHECK(fr.error_code == 0 && fr.bad_pivot == -1 && fr.num_levels == 2 * side - 1 && fr.launches >= 1);
    CHECK(fr.analysis_ms > 0.0f && fr.elapsed_ms > 0.0f);
    d_f.copyToHost(f_dev.data(), count);
    CHECK(std::memcmp(f.data(), f_dev.data(), sizeof(float) * count) == 0);
    CHECK(bsr_ic0(B, d_f.get()).analysis_ms == 0.0f);

    // F over A's structure arrays serves both solves; ordered = 1 is the host twin's bits
    BSRMatrix* F = bsr_wrap_device(n, n, b, B->num_blocks, B->d_block_row_ptrs, B->d_block_cols, d_f.get());
    BSRMatrix Fh = *B;
    Fh.values = f.data();
    std::vector<float> rhs(n), y(n), y_dev(n);
    for (int i = 0; i < n; ++i) rhs[i] = 0.125f * static_cast<float>((i * 7) % 13 - 6);
    d_b.copyFromHost(rhs.data(), n);
    for (int uplo : {SpTRSVConfig::LOWER, SpTRSVConfig::UPPER}) {
        SpTRSVConfig cfg;
        cfg.uplo = uplo;
        cfg.ordered = 1;
        CHECK(sptrsv_cpu_bsr(&Fh, rhs.data(), y.data(), &cfg) == 0);
        const SpTRSVResult sr = sptrsv_bsr(F, d_b.get(), d_y.get(), &cfg);
        CHECK(sr.error_code == 0 && sr.lanes_per_row == 1 && sr.num_levels == 2 * side - 1);
        if (uplo == SpTRSVConfig::LOWER) CHECK(sr.analysis_ms == 0.0f);      // A's schedule
        d_y.copyToHost(y_dev.data(), n);
        CHECK(std::memcmp(y.data(), y_dev.data(), sizeof(float) * n) == 0);
    }

    // the solver, against BLOCK_JACOBI
    std::vector<float> x(n), zero(n, 0.0f);
    int iterations[2] = {0, 0};
    for (int with_ic : {0, 1}) {
        CGConfig cfg;
        cfg.preconditioner = CGConfig::BLOCK_JACOBI;
        cfg.tolerance = 1e-6f;
        cfg.max_iterations = 5000;
        d_x.copyFromHost(zero.data(), n);
        const CGResult res = with_ic ? cg_solve_bsr_ic(B, F, d_b.get(), d_x.get(), &cfg)
                                     : cg_solve_bsr(B, d_b.get(), d_x.get(), &cfg);
        CHECK(res.error_code == 0 && res.converged == 1 && res.breakdown == 0 && res.iterations > 0);
        CHECK(res.relative_residual <= 1e-6f && res.elapsed_ms > 0.0f);
        iterations[with_ic] = res.iterations;
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
    CHECK(2 * iterations[1] <= iterations[0]);
    std::printf("iterations: BLOCK_JACOBI %d block IC(0) %d\n", iterations[0], iterations[1]);

    CHECK(cg_solve_bsr_ic(B, nullptr, d_b.get(), d_x.get()).error_code == static_cast<int>(SpMVError::INVALID_ARGUMENT));

    bsr_destroy(F);
    bsr_destroy(B);
    csr_destroy(A);
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
