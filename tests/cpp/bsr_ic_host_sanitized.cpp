// bsr_ic0_cpu, sptrsv_cpu_bsr and the argument checks of bsr_ic0, sptrsv_bsr and cg_solve_bsr_ic (include/spmv/
// bsr_factor.h, cg.h) under AddressSanitizer + UndefinedBehaviorSanitizer: csrc/bsr_tri_host.cpp and the BSR host files
// it needs are compiled into this executable with the sanitizers (make -C gpu-spmv_amd sanitize-bsr-ic), every array
// below is a heap allocation of exactly its size, and the sizes are the ones whose last block is cut by the matrix's
// edge.  Run by tests/test_bsr_ic_host.py; needs no GPU.
#include "spmv/bsr_factor.h"
#include "spmv/cg.h"

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

static const int kInvalidArgument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
static const int kInvalidDimension = static_cast<int>(SpMVError::INVALID_DIMENSION);
static const int kInvalidFormat = static_cast<int>(SpMVError::INVALID_FORMAT);

// A = L L^T in integers for a block bidiagonal L: diagonal blocks unit lower triangular with ones below the diagonal
// (2 on the last diagonal entry), sub-diagonal blocks the identity.  IC(0) of a block tridiagonal matrix is its complete
// Cholesky factorisation, so the factor must come back exactly.  The arrays are exactly as long as the matrix needs.
struct Host {
    int n, b, nb;
    std::vector<int> ptr, col;
    std::vector<float> val;
    BSRMatrix m{};
    static int ld(int r, int c, int b) { return r == c ? (r == b - 1 ? 2 : 1) : (r > c ? 1 : 0); }
    bool in(int I, int r) const { return I * b + r < n; }
    // entry (r, c) of block (I, J) of L, rows and columns outside the matrix zero
    int l(int I, int J, int r, int c) const {
        if (!in(I, r) || !in(J, c)) return 0;
        if (I == J) return ld(r, c, b);
        if (I == J + 1) return r == c ? 1 : 0;
        return 0;
    }
    Host(int n_, int b_) : n(n_), b(b_), nb((n_ + b_ - 1) / b_) {
        ptr.push_back(0);
        for (int I = 0; I < nb; ++I) {
            for (int J = I - 1; J <= I + 1; ++J) {
                if (J < 0 || J >= nb) continue;
                col.push_back(J);
                for (int r = 0; r < b; ++r) {
                    for (int c = 0; c < b; ++c) {
                        int s = 0;
                        for (int K = 0; K < nb; ++K) {
                            for (int k = 0; k < b; ++k) s += l(I, K, r, k) * l(J, K, c, k);
                        }
                        val.push_back(static_cast<float>(s));
                    }
                }
            }
            ptr.push_back(static_cast<int>(col.size()));
        }
        m.num_rows = m.num_cols = n;
        m.block_dim = b;
        m.num_block_rows = m.num_block_cols = nb;
        m.num_blocks = static_cast<int>(col.size());
        m.block_row_ptrs = ptr.data();
        m.block_cols = col.data();
        m.values = val.data();
    }
};

int main() {
    for (int b : {2, 3, 4, 8}) {
        for (int tail = 0; tail < b; ++tail) {
            const int nb = 5, n = nb * b - tail;
            Host A(n, b);
            const size_t count = A.val.size();
            std::vector<float> f(count, -7.0f);
            int bad = 99;
            CHECK(bsr_ic0_cpu(&A.m, f.data(), &bad) == 0 && bad == -1);
            // off-diagonal blocks: L and its transpose, exactly
            for (int I = 0; I < nb; ++I) {
                for (int p = A.ptr[I]; p < A.ptr[I + 1]; ++p) {
                    const int J = A.col[p];
                    if (J == I) continue;
                    for (int r = 0; r < b; ++r) {
                        for (int c = 0; c < b; ++c) {
                            const int want = J < I ? A.l(I, J, r, c) : A.l(J, I, c, r);
                            CHECK(f[(static_cast<size_t>(p) * b + r) * b + c] == static_cast<float>(want));
                        }
                    }
                }
            }
            // in place gives the same bits
            std::vector<float> in_place(A.val);
            BSRMatrix M = A.m;
            M.values = in_place.data();
            CHECK(bsr_ic0_cpu(&M, in_place.data(), nullptr) == 0);
            CHECK(std::memcmp(in_place.data(), f.data(), count * sizeof(float)) == 0);

            // L^-T (L^-1 (A x)) == x for a small integer x, in and out of place
            BSRMatrix F = A.m;
            F.values = f.data();
            std::vector<float> x(static_cast<size_t>(n)), rhs(static_cast<size_t>(n)), y(static_cast<size_t>(n), -7.0f);
            for (int i = 0; i < n; ++i) x[i] = static_cast<float>((i * 5) % 7 - 3);
            for (int I = 0; I < nb; ++I) {
                for (int r = 0; r < b && I * b + r < n; ++r) {
                    float s = 0.0f;
                    for (int p = A.ptr[I]; p < A.ptr[I + 1]; ++p) {
                        for (int c = 0; c < b && A.col[p] * b + c < n; ++c) {
                            s += A.val[(static_cast<size_t>(p) * b + r) * b + c] * x[A.col[p] * b + c];
                        }
                    }
                    rhs[I * b + r] = s;
                }
            }
            SpTRSVConfig lower, upper;
            upper.uplo = SpTRSVConfig::UPPER;
            lower.ordered = upper.ordered = 1;
            CHECK(sptrsv_cpu_bsr(&F, rhs.data(), y.data(), &lower) == 0);
            CHECK(sptrsv_cpu_bsr(&F, y.data(), y.data(), &upper) == 0);
            for (int i = 0; i < n; ++i) CHECK(y[i] == x[i]);
            SpTRSVConfig unit = lower;
            unit.diag = SpTRSVConfig::UNIT;
            CHECK(sptrsv_cpu_bsr(&F, rhs.data(), y.data(), &unit) == 0);

            // a negative pivot is reported, not rejected
            Host N(n, b);
            N.val[0] = -4.0f;
            CHECK(bsr_ic0_cpu(&N.m, f.data(), &bad) == 0 && bad == 0);

            // rejections of the pattern
            if (nb > 1) {
                Host U(n, b);
                U.col[0] = 1;                                    // block row 0: columns 1, 1
                CHECK(bsr_ic0_cpu(&U.m, f.data(), &bad) == kInvalidArgument);
                CHECK(sptrsv_cpu_bsr(&U.m, rhs.data(), y.data(), &lower) == kInvalidArgument);
                Host R(n, b);
                R.col[1] = nb;                                   // out of range
                CHECK(bsr_ic0_cpu(&R.m, f.data(), &bad) == kInvalidFormat);
                CHECK(sptrsv_cpu_bsr(&R.m, rhs.data(), y.data(), &lower) == kInvalidFormat);
                Host P(n, b);
                P.ptr[1] = P.ptr[2] + 1;
                CHECK(bsr_ic0_cpu(&P.m, f.data(), &bad) == kInvalidFormat);
            }
        }
    }

    // argument checks: nothing below may be dereferenced
    Host A(7, 2);
    std::vector<float> f(A.val.size());
    float* fake_b = reinterpret_cast<float*>(0x600000);
    float* fake_x = reinterpret_cast<float*>(0x700000);
    float* fake_f = reinterpret_cast<float*>(0x800000);
    CHECK(bsr_ic0_cpu(nullptr, f.data(), nullptr) == kInvalidArgument);
    CHECK(bsr_ic0_cpu(&A.m, nullptr, nullptr) == kInvalidArgument);
    CHECK(bsr_ic0_cpu(&A.m, A.val.data() + 1, nullptr) == kInvalidArgument);
    {
        BSRMatrix R = A.m;
        R.num_cols = 5;
        R.num_block_cols = 3;
        CHECK(bsr_ic0_cpu(&R, f.data(), nullptr) == kInvalidDimension);
        CHECK(sptrsv_cpu_bsr(&R, f.data(), f.data(), nullptr) == kInvalidDimension);
        BSRMatrix N = A.m;
        N.values = nullptr;
        CHECK(bsr_ic0_cpu(&N, f.data(), nullptr) == kInvalidFormat);
        CHECK(sptrsv_cpu_bsr(&N, f.data(), f.data(), nullptr) == kInvalidFormat);
        // the device entry points: host arrays only is a missing device array
        CHECK(bsr_ic0(&A.m, fake_f).error_code == kInvalidFormat);
        CHECK(bsr_ic0(nullptr, fake_f).error_code == kInvalidArgument);
        CHECK(bsr_ic0_async(&A.m, nullptr, nullptr) == kInvalidArgument);
        CHECK(sptrsv_bsr(&A.m, fake_b, fake_x).error_code == kInvalidFormat);
        CHECK(sptrsv_bsr(&R, fake_b, fake_x).error_code == kInvalidDimension);
        CHECK(sptrsv_bsr_async(&A.m, nullptr, fake_x, nullptr, nullptr) == kInvalidArgument);
        CHECK(sptrsv_analyze_bsr(&A.m, 0).error_code == kInvalidFormat);
        BSRMatrix D = A.m;
        D.d_block_row_ptrs = reinterpret_cast<int*>(0x300000);
        D.d_block_cols = reinterpret_cast<int*>(0x400000);
        D.d_values = reinterpret_cast<float*>(0x500000);
        CHECK(bsr_ic0(&D, D.d_values + 1).error_code == kInvalidArgument);
        SpTRSVConfig cfg;
        cfg.uplo = 2;
        CHECK(sptrsv_bsr(&D, fake_b, fake_x, &cfg).error_code == kInvalidArgument);
        CHECK(sptrsv_bsr(&D, fake_x + 3, fake_x).error_code == kInvalidArgument);
        CHECK(sptrsv_analyze_bsr(&D, 2).error_code == kInvalidArgument);
        CGConfig any;
        any.preconditioner = 77;                                 // not read
        CHECK(cg_solve_bsr_ic(&D, nullptr, fake_b, fake_x, &any).error_code == kInvalidArgument);
        CHECK(cg_solve_bsr_ic(nullptr, &D, fake_b, fake_x).error_code == kInvalidArgument);
        CHECK(cg_solve_bsr_ic(&D, &R, fake_b, fake_x).error_code == kInvalidDimension);
        CHECK(cg_solve_bsr_ic(&D, &A.m, fake_b, fake_x).error_code == kInvalidFormat);
        any.engine = 1;
        CHECK(cg_solve_bsr_ic(&D, &D, fake_b, fake_x, &any).error_code == kInvalidArgument);
    }

    if (failures) {
        std::printf("%d checks failed\n", failures);
        return 1;
    }
    std::printf("all checks passed\n");
    return 0;
}
