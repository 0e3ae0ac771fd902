// The host side of include/spmv/eigs.h under AddressSanitizer + UndefinedBehaviorSanitizer: csrc/eigs_host.cpp
// (sym_eig_small's host twin and the argument checks of eigs_sym) is compiled into this executable with the
// sanitizers (make -C gpu-spmv_amd sanitize-eigs).  Every array below is a heap allocation of exactly its size, with
// leading dimensions larger than the order where the interface has one, and the device addresses given to the checks
// are fake: a check that dereferenced one would fault.  Run by tests/test_eigs_host.py; needs no GPU.
#include "eigs_impl.h"

#include <cmath>
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace spmv;
using namespace spmv::detail::eigs;

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

static double draw(uint64_t& state) {          // splitmix64 -> [-1, 1)
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    z ^= z >> 31;
    return static_cast<double>(z >> 11) * (1.0 / 4503599627370496.0) - 1.0;
}

// a random symmetric matrix of order n at leading dimension ld: T S = S Theta, S^T S = I, values ascending
static void decompose(int n, int ld) {
    uint64_t state = 1000u + n;
    std::vector<double> T(static_cast<size_t>(n) * ld, 7e77), values(n), vectors(static_cast<size_t>(n) * ld, -3.0);
    for (int i = 0; i < n; ++i) {
        for (int j = 0; j <= i; ++j) T[i * ld + j] = T[j * ld + i] = draw(state);
    }
    bool nothing = true;
    CHECK(sym_eig_small_check(n, T.data(), ld, values.data(), vectors.data(), &nothing) == 0 && nothing == (n == 0));
    if (n == 0) return;
    sym_eig_small_host(n, T.data(), ld, values.data(), vectors.data());
    double worst_res = 0.0, worst_ortho = 0.0;
    for (int a = 0; a < n; ++a) {
        if (a > 0) CHECK(values[a - 1] <= values[a]);
        for (int i = 0; i < n; ++i) {
            double r = -values[a] * vectors[a * ld + i];
            for (int j = 0; j < n; ++j) r += T[i * ld + j] * vectors[a * ld + j];
            worst_res = std::fmax(worst_res, std::fabs(r));
        }
        for (int b = 0; b < n; ++b) {
            double d = a == b ? -1.0 : 0.0;
            for (int i = 0; i < n; ++i) d += vectors[a * ld + i] * vectors[b * ld + i];
            worst_ortho = std::fmax(worst_ortho, std::fabs(d));
        }
        for (int i = n; i < ld; ++i) CHECK(vectors[a * ld + i] == -3.0);     // the padding is never written
    }
    CHECK(worst_res <= 1e-12 && worst_ortho <= 1e-12);
}

struct Header {
    CSRMatrix m{};
    Header(int rows, int cols, int nnz, uintptr_t rp, uintptr_t ci, uintptr_t va) {
        m.num_rows = rows;
        m.num_cols = cols;
        m.nnz = nnz;
        m.d_row_ptrs = reinterpret_cast<int*>(rp);
        m.d_col_indices = reinterpret_cast<int*>(ci);
        m.d_values = reinterpret_cast<float*>(va);
    }
};

static int check(const CSRMatrix* A, uintptr_t values, uintptr_t vectors, long long ldv, uintptr_t residuals,
                 uintptr_t v0, const EigsConfig& cfg, int* m = nullptr, bool* nothing = nullptr) {
    int basis = -1;
    bool none = false;
    const int status = eigs_check_arguments(A, reinterpret_cast<const float*>(values),
                                            reinterpret_cast<const float*>(vectors), ldv,
                                            reinterpret_cast<const float*>(residuals),
                                            reinterpret_cast<const float*>(v0), cfg, &basis, &none);
    if (m) *m = basis;
    if (nothing) *nothing = none;
    return status;
}

int main() {
    for (int n : {1, 2, 3, 7, 8, 9, 31, 32, 33, 63, 64}) {
        decompose(n, n);
        decompose(n, n + 3);
    }
    {   // [[2, 1], [1, 2]]: 1 and 3, vectors (1, -1) / sqrt 2 and (1, 1) / sqrt 2 up to sign
        const double T[4] = {2, 1, 1, 2};
        double values[2], vectors[4];
        sym_eig_small_host(2, T, 2, values, vectors);
        CHECK(std::fabs(values[0] - 1.0) <= 4e-15 && std::fabs(values[1] - 3.0) <= 4e-15);
        CHECK(std::fabs(std::fabs(vectors[0]) - std::sqrt(0.5)) <= 4e-16 && vectors[0] == -vectors[1]);
        CHECK(std::fabs(std::fabs(vectors[2]) - std::sqrt(0.5)) <= 4e-16 && vectors[2] == vectors[3]);
    }
    {   // the zero matrix and a diagonal one: no rotation, S = I, values sorted with ties by position
        const double T[9] = {5, 0, 0, 0, -1, 0, 0, 0, 5};
        double values[3], vectors[9];
        sym_eig_small_host(3, T, 3, values, vectors);
        CHECK(values[0] == -1.0 && values[1] == 5.0 && values[2] == 5.0);
        CHECK(vectors[1] == 1.0 && vectors[3] == 1.0 && vectors[8] == 1.0);
        const double Z[4] = {0, 0, 0, 0};
        sym_eig_small_host(2, Z, 2, values, vectors);
        CHECK(values[0] == 0.0 && values[1] == 0.0 && vectors[0] == 1.0 && vectors[3] == 1.0 && vectors[1] == 0.0);
    }
    {   // sym_eig_small's own checks
        double t = 1.0, v = 0.0, s = 0.0;
        bool nothing = false;
        CHECK(sym_eig_small_check(1, nullptr, 1, &v, &s, &nothing) == kInvalidArgument);
        CHECK(sym_eig_small_check(1, &t, 1, nullptr, &s, &nothing) == kInvalidArgument);
        CHECK(sym_eig_small_check(1, &t, 1, &v, nullptr, &nothing) == kInvalidArgument);
        CHECK(sym_eig_small_check(-1, &t, 1, &v, &s, &nothing) == kInvalidArgument);
        CHECK(sym_eig_small_check(65, &t, 65, &v, &s, &nothing) == kInvalidArgument);
        CHECK(sym_eig_small_check(2, &t, 1, &v, &s, &nothing) == kInvalidArgument);
        CHECK(sym_eig_small_check(0, &t, 0, &v, &s, &nothing) == 0 && nothing);
    }
    // eigs_sym's checks, in the header's order; every address is fake
    const uintptr_t VAL = 0x100000, VEC = 0x200000, RES = 0x300000, V0 = 0x400000;
    const uintptr_t RP = 0x500000, CI = 0x600000, VA = 0x700000;
    EigsConfig bad;
    bad.tolerance = -1.0f;
    Header D(100, 100, 300, RP, CI, VA);
    CHECK(check(nullptr, VAL, VEC, 100, RES, V0, bad) == kInvalidArgument);
    CHECK(check(&D.m, 0, VEC, 100, RES, V0, bad) == kInvalidArgument);
    CHECK(check(&D.m, VAL, 0, 100, RES, V0, bad) == kInvalidArgument);
    { Header R(5, 4, 0, RP, CI, VA); CHECK(check(&R.m, VAL, VEC, 5, 0, 0, bad) == kInvalidDimension); }
    { Header Z(0, 0, 0, 0, 0, 0); bool nothing = false; CHECK(check(&Z.m, VAL, VAL, -1, VAL, VAL, bad, nullptr, &nothing) == 0 && nothing); }
    { Header H(100, 100, 300, 0, CI, VA); CHECK(check(&H.m, VAL, VEC, 100, 0, 0, bad) == kInvalidFormat); }
    { Header H(100, 100, 300, RP, 0, VA); CHECK(check(&H.m, VAL, VEC, 100, 0, 0, bad) == kInvalidFormat); }
    { Header H(100, 100, 300, RP, CI, 0); CHECK(check(&H.m, VAL, VEC, 100, 0, 0, bad) == kInvalidFormat); }
    for (int k : {0, -1, 33, 101}) {
        EigsConfig cfg;
        cfg.num_values = k;
        cfg.basis = 65;                                                       // k is tested before the basis
        CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg) == kInvalidArgument);
    }
    for (int basis : {-1, 1, 4, 65}) {
        EigsConfig cfg;
        cfg.num_values = 4;
        cfg.basis = basis;
        CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg) == kInvalidArgument);
    }
    { EigsConfig cfg; cfg.tolerance = std::nan(""); CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg) == kInvalidArgument); }
    { EigsConfig cfg; cfg.max_iterations = -1; CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg) == kInvalidArgument); }
    { EigsConfig cfg; cfg.which = 2; CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg) == kInvalidArgument); }
    { EigsConfig cfg; cfg.engine = 2; CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg) == kInvalidArgument); }
    { EigsConfig cfg; cfg.engine = -2; CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg) == kInvalidArgument); }
    { EigsConfig cfg; CHECK(check(&D.m, VAL, VEC, 99, 0, 0, cfg) == kInvalidArgument); }
    {   // overlaps: k = 3, n = 100, ldv = 110: the vectors span 320 floats
        EigsConfig cfg;
        cfg.num_values = 3;
        CHECK(check(&D.m, VAL, VEC, 110, RES, V0, cfg) == 0);
        CHECK(check(&D.m, VAL, VEC, 110, VAL + 8, V0, cfg) == kInvalidArgument);
        CHECK(check(&D.m, VAL, VEC, 110, VAL + 12, V0, cfg) == 0);
        CHECK(check(&D.m, VEC + 4 * 319, VEC, 110, RES, V0, cfg) == kInvalidArgument);
        CHECK(check(&D.m, VEC + 4 * 320, VEC, 110, RES, V0, cfg) == 0);
        CHECK(check(&D.m, VAL, VEC, 110, VEC - 8, V0, cfg) == kInvalidArgument);
        CHECK(check(&D.m, VAL, VEC, 110, RES, VEC + 4 * 319, cfg) == kInvalidArgument);
        CHECK(check(&D.m, VAL, VEC, 110, RES, VEC - 4 * 100, cfg) == 0);
        CHECK(check(&D.m, VAL, VEC, 110, RES, VAL - 4 * 99, cfg) == kInvalidArgument);
        CHECK(check(&D.m, VAL, VEC, 110, RES, RES + 8, cfg) == kInvalidArgument);
    }
    {   // the basis that is used
        int m = 0;
        EigsConfig cfg;
        CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg, &m) == 0 && m == 20);
        cfg.num_values = 32;
        CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg, &m) == 0 && m == 64);
        cfg.num_values = 12;
        CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg, &m) == 0 && m == 24);
        cfg.basis = 13;
        CHECK(check(&D.m, VAL, VEC, 100, 0, 0, cfg, &m) == 0 && m == 13);
        Header S(5, 5, 5, RP, CI, VA);
        EigsConfig small;
        small.num_values = 5;
        CHECK(check(&S.m, VAL, VEC, 5, 0, 0, small, &m) == 0 && m == 5);
        Header One(1, 1, 1, RP, CI, VA);
        EigsConfig one;
        CHECK(check(&One.m, VAL, VEC, 1, 0, 0, one, &m) == 0 && m == 1);
    }
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
