// The host side of include/spmv/assemble.h under AddressSanitizer + UndefinedBehaviorSanitizer: csrc/assemble_host.cpp
// (csr_from_coo_cpu, coo_plan_info and the argument checks of the device entry points) is compiled into this
// executable with the sanitizers (make -C gpu-spmv_amd sanitize-assemble).  Every array below is a heap allocation of
// exactly its size, and the device addresses given to the checks are fake: a check that dereferenced one would fault.
// Run by tests/test_assemble_host.py; needs no GPU.
#include "assemble_impl.h"

#include <algorithm>
#include <cstdint>
#include <cstdio>
#include <cstring>
#include <map>
#include <utility>
#include <vector>

using namespace spmv;
using namespace spmv::detail::assemble;

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

static uint32_t word(float v) {
    uint32_t w;
    std::memcpy(&w, &v, sizeof(w));
    return w;
}

static float from_word(uint32_t w) {
    float v;
    std::memcpy(&v, &w, sizeof(v));
    return v;
}

static void release(CSRMatrix& C) {
    if (C.owns_host_memory) {
        delete[] C.values;
        delete[] C.col_indices;
        delete[] C.row_ptrs;
    }
    C = CSRMatrix{};
}

// A[i, j] += v in source order over a map of lists, compared entry by entry with csr_from_coo_cpu
static void against_a_map(int num_rows, int num_cols, const std::vector<int>& rows, const std::vector<int>& cols,
                          const std::vector<float>& vals) {
    const int n = static_cast<int>(rows.size());
    std::map<std::pair<int, int>, std::vector<int>> cells;
    for (int p = 0; p < n; ++p) cells[{rows[p], cols[p]}].push_back(p);
    for (int mode : {static_cast<int>(COO_SUM), static_cast<int>(COO_KEEP)}) {
        CooConfig cfg;
        cfg.duplicates = mode;
        CSRMatrix C{};
        CHECK(csr_from_coo_cpu(&C, num_rows, num_cols, n, rows.data(), cols.data(), vals.data(), &cfg) == 0);
        CHECK(C.num_rows == num_rows && C.num_cols == num_cols && C.owns_host_memory);
        CHECK(C.nnz == (mode == COO_SUM ? static_cast<int>(cells.size()) : n));
        int out = 0;
        std::vector<int> count(static_cast<size_t>(num_rows) + 1, 0);
        for (const auto& cell : cells) {
            const std::vector<int>& places = cell.second;
            if (mode == COO_SUM) {
                float s = vals[places[0]];
                for (size_t e = 1; e < places.size(); ++e) s += vals[places[e]];
                uint32_t want = places.size() == 1 ? word(vals[places[0]]) : (s != s ? 0x7FC00000u : word(s));
                CHECK(out < C.nnz && C.col_indices[out] == cell.first.second && word(C.values[out]) == want);
                ++out;
                ++count[cell.first.first + 1];
            } else {
                for (int p : places) {
                    CHECK(out < C.nnz && C.col_indices[out] == cell.first.second && word(C.values[out]) == word(vals[p]));
                    ++out;
                    ++count[cell.first.first + 1];
                }
            }
        }
        CHECK(out == C.nnz);
        CHECK(C.row_ptrs[0] == 0);
        for (int r = 0; r < num_rows; ++r) CHECK(C.row_ptrs[r + 1] - C.row_ptrs[r] == count[r + 1]);
        // into a matrix that already owns arrays: they are replaced
        CHECK(csr_from_coo_cpu(&C, num_rows, num_cols, n, rows.data(), cols.data(), vals.data(), nullptr) == 0);
        CHECK(C.nnz == static_cast<int>(cells.size()));
        release(C);
    }
}

static void assembly() {
    uint64_t state = 7;
    {   // a small matrix with many repeats, empty first and last rows
        const int num_rows = 23, num_cols = 31, n = 4000;
        std::vector<int> rows(n), cols(n);
        std::vector<float> vals(n);
        for (int p = 0; p < n; ++p) {
            rows[p] = 2 + static_cast<int>(draw(state) % 19);
            cols[p] = static_cast<int>(draw(state) % num_cols);
            vals[p] = static_cast<float>(static_cast<int>(draw(state) % 2001) - 1000) / 7.0f;
        }
        against_a_map(num_rows, num_cols, rows, cols, vals);
    }
    {   // the widest key: 17 + 31 bits, entries at both extremes
        const int num_rows = (1 << 16) + 1, num_cols = 2147483647, n = 500;
        std::vector<int> rows(n), cols(n);
        std::vector<float> vals(n);
        for (int p = 0; p < n; ++p) {
            rows[p] = static_cast<int>(draw(state) % num_rows);
            cols[p] = static_cast<int>(draw(state) % num_cols);
            vals[p] = static_cast<float>(p);
        }
        rows[0] = rows[1] = num_rows - 1;
        cols[0] = cols[1] = num_cols - 1;
        rows[2] = cols[2] = 0;
        against_a_map(num_rows, num_cols, rows, cols, vals);
    }
    {   // bit patterns: a lone value is copied, the NaN of an addition has one spelling, order matters
        const std::vector<int> rows = {0, 0, 0, 1, 1, 2, 2, 2, 3, 3, 4, 4};
        const std::vector<int> cols = {0, 1, 2, 0, 0, 1, 1, 1, 2, 2, 0, 0};
        const std::vector<float> vals = {from_word(0x80000000u), from_word(0x7FC12345u), from_word(0x7F800001u),
                                         from_word(0x7F800000u), from_word(0xFF800000u),
                                         1e8f, 1.0f, -1e8f, 1.5f, -1.5f, from_word(0x00000001u), from_word(0x00000002u)};
        against_a_map(5, 3, rows, cols, vals);
        CSRMatrix C{};
        CHECK(csr_from_coo_cpu(&C, 5, 3, 12, rows.data(), cols.data(), vals.data(), nullptr) == 0 && C.nnz == 7);
        const uint32_t want[7] = {0x80000000u, 0x7FC12345u, 0x7F800001u, 0x7FC00000u, 0x00000000u, 0x00000000u,
                                  0x00000003u};
        for (int e = 0; e < 7 && e < C.nnz; ++e) CHECK(word(C.values[e]) == want[e]);
        release(C);
    }
    {   // nothing to assemble
        CSRMatrix C{};
        CHECK(csr_from_coo_cpu(&C, 4, 5, 0, nullptr, nullptr, nullptr, nullptr) == 0 && C.nnz == 0 && C.num_rows == 4);
        for (int r = 0; r <= 4; ++r) CHECK(C.row_ptrs[r] == 0);
        CHECK(C.values == nullptr && C.col_indices == nullptr);
        CHECK(csr_from_coo_cpu(&C, 0, 0, 0, nullptr, nullptr, nullptr, nullptr) == 0 && C.num_rows == 0);
        CHECK(C.row_ptrs[0] == 0);
        release(C);
    }
    {   // rejections, C as it was
        const std::vector<int> rows = {0, 1, 2}, cols = {2, 1, 0};
        const std::vector<float> vals = {1.0f, 2.0f, 3.0f};
        CSRMatrix C{};
        C.num_rows = -3;
        CooConfig bad;
        bad.reserved = 1;
        CHECK(csr_from_coo_cpu(nullptr, 3, 3, 3, rows.data(), cols.data(), vals.data(), nullptr) == kInvalidArgument);
        CHECK(csr_from_coo_cpu(&C, 3, 3, 3, nullptr, cols.data(), vals.data(), nullptr) == kInvalidArgument);
        CHECK(csr_from_coo_cpu(&C, 3, 3, 3, rows.data(), nullptr, vals.data(), nullptr) == kInvalidArgument);
        CHECK(csr_from_coo_cpu(&C, 3, 3, 3, rows.data(), cols.data(), nullptr, nullptr) == kInvalidArgument);
        CHECK(csr_from_coo_cpu(&C, -1, 3, 3, rows.data(), cols.data(), vals.data(), &bad) == kInvalidDimension);
        CHECK(csr_from_coo_cpu(&C, 3, -1, 3, rows.data(), cols.data(), vals.data(), nullptr) == kInvalidDimension);
        CHECK(csr_from_coo_cpu(&C, 3, 3, -1, rows.data(), cols.data(), vals.data(), nullptr) == kInvalidDimension);
        CHECK(csr_from_coo_cpu(&C, 3, 3, 3, rows.data(), cols.data(), vals.data(), &bad) == kInvalidArgument);
        bad.reserved = 0;
        bad.duplicates = 2;
        CHECK(csr_from_coo_cpu(&C, 3, 3, 3, rows.data(), cols.data(), vals.data(), &bad) == kInvalidArgument);
        CHECK(csr_from_coo_cpu(&C, 2, 3, 3, rows.data(), cols.data(), vals.data(), nullptr) == kInvalidFormat);
        CHECK(csr_from_coo_cpu(&C, 3, 2, 3, rows.data(), cols.data(), vals.data(), nullptr) == kInvalidFormat);
        const std::vector<int> negative = {0, -1, 2};
        CHECK(csr_from_coo_cpu(&C, 3, 3, 3, negative.data(), cols.data(), vals.data(), nullptr) == kInvalidFormat);
        CHECK(csr_from_coo_cpu(&C, 3, 3, 3, rows.data(), negative.data(), vals.data(), nullptr) == kInvalidFormat);
        CHECK(C.num_rows == -3 && C.row_ptrs == nullptr && !C.owns_host_memory);
    }
}

static void layout() {
    CHECK(index_bits(0) == 0 && index_bits(1) == 0 && index_bits(2) == 1 && index_bits(3) == 2 && index_bits(4) == 2);
    CHECK(index_bits(1 << 16) == 16 && index_bits((1 << 16) + 1) == 17 && index_bits(2147483647) == 31);
    CHECK(key_layout(1 << 16, 1 << 16).total_bits == 32 && key_layout(1 << 16, 1 << 16).narrow());
    CHECK(key_layout(1 << 16, (1 << 16) + 1).total_bits == 33 && !key_layout(1 << 16, (1 << 16) + 1).narrow());
    CHECK(key_layout((1 << 16) + 1, 2147483647).total_bits == 48);
    CHECK(key_layout(2147483647, 2147483647).total_bits == 62 && key_layout(1, 1).total_bits == 0);
    CHECK(kTileEntries == kSortThreads * kSortRounds && kTileEntries % 64 == 0);
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

static void checks() {
    const uintptr_t RP = 0x500000, CI = 0x600000, VA = 0x700000;
    const int* const rows = reinterpret_cast<const int*>(0x800000);
    const int* const cols = reinterpret_cast<const int*>(0x900000);
    const float* const vals = reinterpret_cast<const float*>(0xA00000);
    Header C(1, 1, 0, 0, 0, 0);
    CooConfig ok, bad;
    bad.reserved = 3;
    // csr_from_coo_gpu's order: nulls, sizes, config
    CHECK(build_check(&C.m, 3, 3, 5, rows, cols, vals, ok) == 0);
    CHECK(build_check(&C.m, 3, 3, 0, nullptr, nullptr, nullptr, ok) == 0);
    CHECK(build_check(nullptr, -1, 3, 5, rows, cols, vals, bad) == kInvalidArgument);
    CHECK(build_check(&C.m, -1, 3, 5, nullptr, cols, vals, bad) == kInvalidArgument);
    CHECK(build_check(&C.m, -1, 3, 5, rows, nullptr, vals, bad) == kInvalidArgument);
    CHECK(build_check(&C.m, -1, 3, 5, rows, cols, nullptr, bad) == kInvalidArgument);
    CHECK(build_check(&C.m, -1, 3, 5, rows, cols, vals, bad) == kInvalidDimension);
    CHECK(build_check(&C.m, 3, -1, 5, rows, cols, vals, bad) == kInvalidDimension);
    CHECK(build_check(&C.m, 3, 3, -5, rows, cols, vals, bad) == kInvalidDimension);
    CHECK(build_check(&C.m, 3, 3, 5, rows, cols, vals, bad) == kInvalidArgument);
    for (int mode : {-1, 2, 99}) {
        CooConfig cfg;
        cfg.duplicates = mode;
        CHECK(build_check(&C.m, 3, 3, 5, rows, cols, vals, cfg) == kInvalidArgument);
    }
    ok.duplicates = COO_KEEP;
    CHECK(build_check(&C.m, 3, 3, 5, rows, cols, vals, ok) == 0);

    // csr_coo_refill: a plan over fake device arrays
    CooPlan plan;
    plan.num_rows = 100;
    plan.num_cols = 50;
    plan.n = 900;
    plan.nnz_out = 300;
    plan.d_order = reinterpret_cast<int*>(0xB00000);
    plan.d_segments = reinterpret_cast<int*>(0xC00000);
    Header D(100, 50, 300, RP, CI, VA);
    CHECK(refill_check(&plan, &D.m, vals) == 0);
    CHECK(refill_check(nullptr, &D.m, vals) == kInvalidArgument);
    CHECK(refill_check(&plan, nullptr, vals) == kInvalidArgument);
    CHECK(refill_check(&plan, &D.m, nullptr) == kInvalidArgument);
    { Header W(101, 50, 300, RP, CI, VA); CHECK(refill_check(&plan, &W.m, vals) == kInvalidDimension); }
    { Header W(100, 51, 300, RP, CI, VA); CHECK(refill_check(&plan, &W.m, vals) == kInvalidDimension); }
    { Header W(100, 50, 299, RP, CI, VA); CHECK(refill_check(&plan, &W.m, vals) == kInvalidDimension); }
    { Header W(100, 50, 300, 0, CI, VA); CHECK(refill_check(&plan, &W.m, vals) == kInvalidFormat); }
    { Header W(100, 50, 300, RP, 0, VA); CHECK(refill_check(&plan, &W.m, vals) == kInvalidFormat); }
    { Header W(100, 50, 300, RP, CI, 0); CHECK(refill_check(&plan, &W.m, vals) == kInvalidFormat); }
    {   // an empty plan needs no values
        CooPlan empty;
        empty.num_rows = 4;
        empty.num_cols = 5;
        Header E(4, 5, 0, RP, 0, 0);
        CHECK(refill_check(&empty, &E.m, nullptr) == 0);
    }
    int got[5] = {-7, -7, -7, -7, -7};
    CHECK(coo_plan_info(nullptr, got, got + 1, got + 2, got + 3, got + 4) == kInvalidArgument && got[0] == -7);
    CHECK(coo_plan_info(&plan, got, got + 1, got + 2, got + 3, got + 4) == 0);
    CHECK(got[0] == 100 && got[1] == 50 && got[2] == 900 && got[3] == 300 && got[4] == COO_SUM);
    CHECK(coo_plan_info(&plan, nullptr, nullptr, nullptr, nullptr, nullptr) == 0);

    // csr_row_indices_gpu
    int* const out = reinterpret_cast<int*>(0xD00000);
    bool nothing = true;
    CHECK(row_indices_check(&D.m, out, &nothing) == 0 && !nothing);
    CHECK(row_indices_check(nullptr, out, &nothing) == kInvalidArgument);
    CHECK(row_indices_check(&D.m, nullptr, &nothing) == kInvalidArgument);
    { Header H(100, 50, 300, 0, CI, VA); CHECK(row_indices_check(&H.m, out, &nothing) == kInvalidFormat); }
    { Header H(100, 50, 300, RP, 0, VA); CHECK(row_indices_check(&H.m, out, &nothing) == kInvalidFormat); }
    { Header H(100, 50, 300, RP, CI, 0); CHECK(row_indices_check(&H.m, out, &nothing) == kInvalidFormat); }
    { Header H(-1, 50, 0, RP, 0, 0); CHECK(row_indices_check(&H.m, out, &nothing) == kInvalidFormat); }
    { Header H(0, 50, 3, RP, CI, VA); CHECK(row_indices_check(&H.m, out, &nothing) == kInvalidFormat); }
    { Header H(0, 50, 0, 0, 0, 0); CHECK(row_indices_check(&H.m, nullptr, &nothing) == 0 && nothing); }
    { Header H(100, 50, 0, RP, 0, 0); CHECK(row_indices_check(&H.m, nullptr, &nothing) == 0 && !nothing); }
}

int main() {
    assembly();
    layout();
    checks();
    if (failures == 0) std::printf("all checks passed\n");
    return failures == 0 ? 0 : 1;
}
