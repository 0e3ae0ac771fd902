// reorder_host.cpp — the host side of include/spmv/reorder.h that needs no device: csr_color_cpu,
// the definition of the colouring; csr_permute_cpu, the definition of the permuted matrix; and the argument checks
// of the device entry points in reorder.hip.
#include "reorder_impl.h"
#include "internal.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <utility>
#include <vector>

namespace spmv {
namespace detail {
namespace reorder {

namespace {

bool lanes_ok(int lanes) { return lanes == 0 || (lanes >= 1 && lanes <= 64 && (lanes & (lanes - 1)) == 0); }

bool spans_overlap(const float* a, long long na, const float* b, long long nb) {
    const uintptr_t a0 = reinterpret_cast<uintptr_t>(a), b0 = reinterpret_cast<uintptr_t>(b);
    return a0 < b0 + static_cast<uintptr_t>(nb) * sizeof(float) &&
           b0 < a0 + static_cast<uintptr_t>(na) * sizeof(float);
}

// csr_transpose_gpu's structure rule on host arrays
bool structure_ok(const CSRMatrix* A) {
    const int rows = A->num_rows;
    if (A->row_ptrs[0] != 0 || A->row_ptrs[rows] != A->nnz) return false;
    for (int i = 0; i < rows; ++i) {
        if (A->row_ptrs[i + 1] < A->row_ptrs[i]) return false;
    }
    for (int j = 0; j < A->nnz; ++j) {
        if (A->col_indices[j] < 0 || A->col_indices[j] >= A->num_cols) return false;
    }
    return true;
}

// null (the identity) or a permutation of [0, n)
bool is_permutation(const int* p, int n) {
    if (!p) return true;
    std::vector<char> seen(static_cast<size_t>(n), 0);
    for (int i = 0; i < n; ++i) {
        if (p[i] < 0 || p[i] >= n || seen[p[i]]) return false;
        seen[p[i]] = 1;
    }
    return true;
}

} // namespace

int color_check(const CSRMatrix* A, const int* d_colors, const ColorConfig& cfg, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_colors) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return 0;
    }
    // (not device_arrays_strict: a negative nnz fails here, there it counts as no entries)
    if (A->num_rows < 0 || A->nnz < 0 || !A->d_row_ptrs || (A->nnz > 0 && (!A->d_col_indices || !A->d_values))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    if (!lanes_ok(cfg.lanes_per_row)) return code(SpMVError::INVALID_ARGUMENT);
    if (cfg.reserved != 0) return code(SpMVError::INVALID_ARGUMENT);
    return 0;
}

int permute_check(const CSRMatrix* B, const CSRMatrix* A) {
    if (!B || !A) return code(SpMVError::INVALID_ARGUMENT);
    if (B == A) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    return 0;
}

int gather_check(const float* d_out, int ldo, const float* d_in, int ldi, const int* d_index, int n, int k,
                 bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!d_out || !d_in || !d_index || n < 0) return code(SpMVError::INVALID_ARGUMENT);
    if (k < 1 || k > kMaxGatherColumns) return code(SpMVError::INVALID_ARGUMENT);
    if (ldo < k || ldi < k) return code(SpMVError::INVALID_ARGUMENT);
    if (n == 0) {
        *nothing_to_do = true;
        return 0;
    }
    const long long rows = n - 1;
    if (spans_overlap(d_out, rows * ldo + k, d_in, rows * ldi + k)) return code(SpMVError::INVALID_ARGUMENT);
    return 0;
}

int ordering_check(int n, const int* d_colors, int num_colors, const int* d_perm, const int* d_inverse,
                   bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!d_colors || !d_perm || !d_inverse || n < 0 || num_colors < 0) return code(SpMVError::INVALID_ARGUMENT);
    if (n == 0) {
        *nothing_to_do = true;
        return 0;
    }
    if (num_colors == 0) return code(SpMVError::INVALID_ARGUMENT);      // every colour is out of range
    return 0;
}

} // namespace reorder
} // namespace detail

int csr_color_cpu(const CSRMatrix* A, int* colors, int* num_colors, int* rounds, const ColorConfig* config) {
    using namespace detail;
    using namespace detail::reorder;
    if (!A || !colors) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n == 0) {
        if (num_colors) *num_colors = 0;
        if (rounds) *rounds = 0;
        return code(SpMVError::SUCCESS);
    }
    if (n < 0 || A->nnz < 0 || !A->row_ptrs || (A->nnz > 0 && !A->col_indices)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const ColorConfig defaults;
    const ColorConfig& cfg = config ? *config : defaults;
    if (!lanes_ok(cfg.lanes_per_row) || cfg.reserved != 0) return code(SpMVError::INVALID_ARGUMENT);
    if (!structure_ok(A)) return code(SpMVError::INVALID_FORMAT);

    const int* rp = A->row_ptrs;
    const int* ci = A->col_indices;
    // the pattern of A^T, unless the caller promises that A's own is symmetric
    std::vector<int> trp, tci;
    if (!cfg.symmetric_pattern) {
        trp.assign(static_cast<size_t>(n) + 1, 0);
        tci.resize(static_cast<size_t>(A->nnz));
        for (int j = 0; j < A->nnz; ++j) ++trp[ci[j] + 1];
        for (int c = 0; c < n; ++c) trp[c + 1] += trp[c];
        std::vector<int> next(trp.begin(), trp.end() - 1);
        for (int i = 0; i < n; ++i) {
            for (int j = rp[i]; j < rp[i + 1]; ++j) tci[next[ci[j]]++] = i;
        }
    }

    // vertices in descending priority
    std::vector<uint64_t> order(static_cast<size_t>(n));
    for (int i = 0; i < n; ++i) {
        order[i] = (static_cast<uint64_t>(fmix32(static_cast<unsigned>(i) ^ cfg.seed)) << 32) | static_cast<unsigned>(i);
    }
    std::sort(order.begin(), order.end(), [](uint64_t a, uint64_t b) { return a > b; });

    std::vector<int> colour(static_cast<size_t>(n), -1), round(static_cast<size_t>(n), 0);
    std::vector<int> taken(static_cast<size_t>(n) + 1, -1);      // taken[c] == v: a higher neighbour of v holds c
    int colours = 0, last_round = 0;
    for (int step = 0; step < n; ++step) {
        const int v = static_cast<int>(order[step] & 0xffffffffu);
        int r = 0;
        auto visit = [&](const int* ptr, const int* col) {
            for (int j = ptr[v]; j < ptr[v + 1]; ++j) {
                const int u = col[j];
                if (u == v || !higher_priority(u, v, cfg.seed)) continue;
                taken[colour[u]] = v;
                r = std::max(r, round[u]);
            }
        };
        visit(rp, ci);
        if (!cfg.symmetric_pattern) visit(trp.data(), tci.data());
        int c = 0;
        while (taken[c] == v) ++c;
        colour[v] = c;
        round[v] = r + 1;
        colours = std::max(colours, c + 1);
        last_round = std::max(last_round, r + 1);
    }
    std::memcpy(colors, colour.data(), sizeof(int) * static_cast<size_t>(n));
    if (num_colors) *num_colors = colours;
    if (rounds) *rounds = last_round;
    return code(SpMVError::SUCCESS);
}

int csr_permute_cpu(CSRMatrix* B, const CSRMatrix* A, const int* row_perm, const int* col_inverse) {
    using namespace detail;
    using namespace detail::reorder;
    if (!B || !A || B == A) return code(SpMVError::INVALID_ARGUMENT);
    const int rows = A->num_rows, cols = A->num_cols, nnz = A->nnz;
    if (rows < 0 || cols < 0 || nnz < 0 || !A->row_ptrs || (nnz > 0 && (!A->col_indices || !A->values))) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    if (!structure_ok(A)) return code(SpMVError::INVALID_FORMAT);
    if (!is_permutation(row_perm, rows) || !is_permutation(col_inverse, cols)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }

    float* new_vals = nnz > 0 ? new float[nnz] : nullptr;
    int* new_cols = nnz > 0 ? new int[nnz] : nullptr;
    int* new_ptrs = new int[static_cast<size_t>(rows) + 1];
    std::vector<std::pair<int, int>> entries;                    // (new column, source position)
    int out = 0;
    new_ptrs[0] = 0;
    for (int i = 0; i < rows; ++i) {
        const int src = row_perm ? row_perm[i] : i;
        entries.clear();
        for (int j = A->row_ptrs[src]; j < A->row_ptrs[src + 1]; ++j) {
            const int c = A->col_indices[j];
            entries.emplace_back(col_inverse ? col_inverse[c] : c, j);
        }
        std::sort(entries.begin(), entries.end());               // positions are distinct: the stable order
        for (const auto& e : entries) {
            new_cols[out] = e.first;
            std::memcpy(&new_vals[out], &A->values[e.second], sizeof(float));     // the bits, whatever they are
            ++out;
        }
        new_ptrs[i + 1] = out;
    }

    csr_adopt_host(B, rows, cols, nnz, new_ptrs, new_cols, new_vals);
    return code(SpMVError::SUCCESS);
}

} // namespace spmv
