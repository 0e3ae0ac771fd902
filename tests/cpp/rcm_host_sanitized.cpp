// The host side of the reverse Cuthill-McKee calls of include/spmv/reorder.h under AddressSanitizer +
// UndefinedBehaviorSanitizer: csrc/rcm_host.cpp (csr_rcm_cpu, csr_band_cpu and the argument checks of the device entry
// points) is compiled into this executable with the sanitizers (make -C gpu-spmv_amd sanitize-rcm).  Every array below
// is a heap allocation of exactly its size, and the device addresses given to the checks are fake: a check that
// dereferenced one would fault.  Run by tests/test_rcm_host.py; needs no GPU.
#include "rcm_impl.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <vector>

using namespace spmv;
using namespace spmv::detail::rcm;

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

static uint64_t draw(uint64_t& state) {          // splitmix64
    state += 0x9E3779B97F4A7C15ull;
    uint64_t z = state;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ull;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBull;
    return z ^ (z >> 31);
}

// a host matrix over vectors of exactly the right size
struct Host {
    std::vector<int> rp, ci;
    std::vector<float> va;
    CSRMatrix m{};
    Host(int rows, int cols, const std::vector<std::vector<int>>& lists) {
        rp.push_back(0);
        for (const auto& row : lists) {
            for (int c : row) {
                ci.push_back(c);
                va.push_back(static_cast<float>(ci.size()));
            }
            rp.push_back(static_cast<int>(ci.size()));
        }
        m.num_rows = rows;
        m.num_cols = cols;
        m.nnz = static_cast<int>(ci.size());
        m.row_ptrs = rp.data();
        m.col_indices = ci.empty() ? nullptr : ci.data();
        m.values = va.empty() ? nullptr : va.data();
    }
};

// orders A, checks that perm and inverse are inverse permutations; returns the lower band of P A P^T
static int order_and_check(const Host& A, const RcmConfig* cfg, int* components = nullptr, int* levels = nullptr) {
    const int n = A.m.num_rows;
    std::vector<int> perm(static_cast<size_t>(n), -7), inverse(static_cast<size_t>(n), -7);
    int count = -7, height = -7;
    CHECK(csr_rcm_cpu(&A.m, perm.data(), inverse.data(), &count, &height, cfg) == 0);
    std::vector<char> seen(static_cast<size_t>(n), 0);
    for (int i = 0; i < n; ++i) {
        CHECK(perm[i] >= 0 && perm[i] < n);
        if (perm[i] < 0 || perm[i] >= n) return -1;
        CHECK(!seen[perm[i]]);
        seen[perm[i]] = 1;
        CHECK(inverse[perm[i]] == i);
    }
    CHECK(count >= 1 && count <= n && height >= count && height <= n);
    if (components) *components = count;
    if (levels) *levels = height;
    int lower = 0;
    for (int i = 0; i < n; ++i) {
        for (int j = A.rp[i]; j < A.rp[i + 1]; ++j) lower = std::max(lower, inverse[i] - inverse[A.ci[j]]);
    }
    // null outputs for the counts are allowed
    CHECK(csr_rcm_cpu(&A.m, perm.data(), inverse.data(), nullptr, nullptr, cfg) == 0);
    return lower;
}

static Host grid(int side, uint64_t shuffle_seed) {
    const int n = side * side;
    std::vector<int> label(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) label[i] = i;
    uint64_t state = shuffle_seed;
    if (shuffle_seed) {
        for (int i = n - 1; i > 0; --i) std::swap(label[i], label[draw(state) % static_cast<uint64_t>(i + 1)]);
    }
    std::vector<std::vector<int>> rows(static_cast<size_t>(n));
    for (int y = 0; y < side; ++y) {
        for (int x = 0; x < side; ++x) {
            const int v = label[y * side + x];
            rows[v].push_back(v);
            if (x > 0) rows[v].push_back(label[y * side + x - 1]);
            if (x + 1 < side) rows[v].push_back(label[y * side + x + 1]);
            if (y > 0) rows[v].push_back(label[(y - 1) * side + x]);
            if (y + 1 < side) rows[v].push_back(label[(y + 1) * side + x]);
        }
    }
    for (auto& r : rows) std::sort(r.begin(), r.end());
    return Host(n, n, rows);
}

int main() {
    // ---- the ordering ----
    {
        const Host single(1, 1, {{0}});
        int components = 0, levels = 0;
        order_and_check(single, nullptr, &components, &levels);
        CHECK(components == 1 && levels == 1);
        const Host lone(4, 4, {{}, {1}, {}, {3}});
        order_and_check(lone, nullptr, &components, &levels);
        CHECK(components == 4 && levels == 4);
        const Host bidiagonal(6, 6, {{1}, {2}, {3}, {4}, {5}, {}});
        CHECK(order_and_check(bidiagonal, nullptr, &components, &levels) <= 1);
        CHECK(components == 1 && levels == 6);
        RcmConfig promised;
        promised.symmetric_pattern = 1;
        order_and_check(bidiagonal, &promised);                     // the broken promise: still a permutation
        RcmConfig plain;
        plain.peripheral = 0;
        order_and_check(bidiagonal, &plain);
    }
    for (uint64_t seed : {0ull, 1ull, 2ull}) {
        const Host g = grid(12, seed);
        int components = 0, levels = 0;
        const int lower = order_and_check(g, nullptr, &components, &levels);
        CHECK(components == 1 && lower <= 12 && levels == 23);      // from a corner: one level per anti-diagonal
        RcmConfig cfg;
        cfg.peripheral = 0;
        cfg.symmetric_pattern = 1;
        order_and_check(g, &cfg);
    }
    {   // random sparse rows, many components
        uint64_t state = 11;
        std::vector<std::vector<int>> rows(200);
        for (int i = 0; i < 200; ++i) {
            for (int k = 0; k < 2; ++k) {
                if (draw(state) % 3 == 0) rows[i].push_back(static_cast<int>(draw(state) % 200));
            }
            std::sort(rows[i].begin(), rows[i].end());
            rows[i].erase(std::unique(rows[i].begin(), rows[i].end()), rows[i].end());
        }
        const Host A(200, 200, rows);
        order_and_check(A, nullptr);
        RcmConfig cfg;
        cfg.symmetric_pattern = 1;
        order_and_check(A, &cfg);
    }

    // ---- csr_rcm_cpu's rejections, outputs untouched ----
    {
        const Host A(3, 3, {{0, 1}, {0, 1, 2}, {1, 2}});
        std::vector<int> perm(3, -7), inverse(3, -7);
        CHECK(csr_rcm_cpu(nullptr, perm.data(), inverse.data(), nullptr, nullptr) == kInvalidArgument);
        CHECK(csr_rcm_cpu(&A.m, nullptr, inverse.data(), nullptr, nullptr) == kInvalidArgument);
        CHECK(csr_rcm_cpu(&A.m, perm.data(), nullptr, nullptr, nullptr) == kInvalidArgument);
        const Host R(2, 3, {{0}, {2}});
        CHECK(csr_rcm_cpu(&R.m, perm.data(), inverse.data(), nullptr, nullptr) == kInvalidDimension);
        CSRMatrix empty{};
        int components = -7, levels = -7;
        CHECK(csr_rcm_cpu(&empty, perm.data(), inverse.data(), &components, &levels) == 0);
        CHECK(components == 0 && levels == 0);
        CSRMatrix bare = A.m;
        bare.row_ptrs = nullptr;
        CHECK(csr_rcm_cpu(&bare, perm.data(), inverse.data(), nullptr, nullptr) == kInvalidArgument);
        RcmConfig cfg;
        cfg.lanes_per_row = 3;
        CHECK(csr_rcm_cpu(&A.m, perm.data(), inverse.data(), nullptr, nullptr, &cfg) == kInvalidArgument);
        cfg = RcmConfig();
        cfg.peripheral = 2;
        CHECK(csr_rcm_cpu(&A.m, perm.data(), inverse.data(), nullptr, nullptr, &cfg) == kInvalidArgument);
        cfg = RcmConfig();
        cfg.reserved = 1;
        CHECK(csr_rcm_cpu(&A.m, perm.data(), inverse.data(), nullptr, nullptr, &cfg) == kInvalidArgument);
        const Host unsorted(3, 3, {{1, 0}, {0, 1, 2}, {1, 2}});
        CHECK(csr_rcm_cpu(&unsorted.m, perm.data(), inverse.data(), nullptr, nullptr) == kInvalidFormat);
        const Host repeated(3, 3, {{0, 0}, {0, 1, 2}, {1, 2}});
        CHECK(csr_rcm_cpu(&repeated.m, perm.data(), inverse.data(), nullptr, nullptr) == kInvalidFormat);
        const Host outside(3, 3, {{0, 3}, {0, 1, 2}, {1, 2}});
        CHECK(csr_rcm_cpu(&outside.m, perm.data(), inverse.data(), nullptr, nullptr) == kInvalidFormat);
        for (int i = 0; i < 3; ++i) CHECK(perm[i] == -7 && inverse[i] == -7);
    }

    // ---- csr_band_cpu ----
    {
        const Host A(4, 6, {{2, 0}, {}, {5}, {3, 1}});
        CsrBand band{-7, -7, -7};
        CHECK(csr_band_cpu(&A.m, &band) == 0);
        CHECK(band.lower == 2 && band.upper == 3 && band.profile == 2);
        const Host none(3, 3, {{}, {}, {}});
        CHECK(csr_band_cpu(&none.m, &band) == 0 && band.lower == 0 && band.upper == 0 && band.profile == 0);
        CSRMatrix empty{};
        CHECK(csr_band_cpu(&empty, &band) == 0 && band.profile == 0);
        band = CsrBand{-7, -7, -7};
        CHECK(csr_band_cpu(nullptr, &band) == kInvalidArgument && csr_band_cpu(&A.m, nullptr) == kInvalidArgument);
        const Host outside(2, 2, {{0, 2}, {1}});
        CHECK(csr_band_cpu(&outside.m, &band) == kInvalidFormat);
        CHECK(band.lower == -7 && band.upper == -7 && band.profile == -7);
    }

    // ---- the checks of the device entry points: none may touch a (fake) device address ----
    {
        int* const perm = reinterpret_cast<int*>(0x900000);
        int* const inverse = reinterpret_cast<int*>(0xA00000);
        CSRMatrix D{};
        D.num_rows = D.num_cols = 100;
        D.nnz = 300;
        D.d_row_ptrs = reinterpret_cast<int*>(0x500000);
        D.d_col_indices = reinterpret_cast<int*>(0x600000);
        D.d_values = reinterpret_cast<float*>(0x700000);
        RcmConfig bad;
        bad.lanes_per_row = 3;
        bad.peripheral = 5;
        bad.reserved = 9;
        bool nothing = true;
        CHECK(rcm_check(nullptr, perm, inverse, bad, &nothing) == kInvalidArgument);
        CHECK(rcm_check(&D, nullptr, inverse, bad, &nothing) == kInvalidArgument);
        CHECK(rcm_check(&D, perm, nullptr, bad, &nothing) == kInvalidArgument);
        CSRMatrix R = D;
        R.num_cols = 99;
        CHECK(rcm_check(&R, perm, inverse, bad, &nothing) == kInvalidDimension);
        CSRMatrix Z{};
        CHECK(rcm_check(&Z, perm, inverse, bad, &nothing) == 0 && nothing);
        CSRMatrix H = D;
        H.d_col_indices = nullptr;
        CHECK(rcm_check(&H, perm, inverse, bad, &nothing) == kInvalidFormat && !nothing);
        CHECK(rcm_check(&D, perm, inverse, bad, &nothing) == kInvalidArgument);
        RcmConfig cfg;
        CHECK(rcm_check(&D, perm, inverse, cfg, &nothing) == 0 && !nothing);
        cfg.peripheral = -1;
        CHECK(rcm_check(&D, perm, inverse, cfg, &nothing) == kInvalidArgument);
        cfg = RcmConfig();
        cfg.reserved = 1;
        CHECK(rcm_check(&D, perm, inverse, cfg, &nothing) == kInvalidArgument);
        CsrBand band{0, 0, 0};
        CHECK(band_check(nullptr, &band) == kInvalidArgument && band_check(&D, nullptr) == kInvalidArgument);
        CHECK(band_check(&H, &band) == kInvalidFormat && band_check(&D, &band) == 0);
    }

    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
