// assemble_host.cpp — the host side of include/spmv/assemble.h that needs no device:
// csr_from_coo_cpu, the definition of the assembled matrix; coo_plan_info; and the argument checks of the device
// entry points in assemble.hip.
#include "assemble_impl.h"
#include "internal.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace spmv {
namespace detail {
namespace assemble {

int build_check(const CSRMatrix* C, int num_rows, int num_cols, int n, const int* rows, const int* cols,
                const float* vals, const CooConfig& cfg) {
    if (!C || (n > 0 && (!rows || !cols || !vals))) return code(SpMVError::INVALID_ARGUMENT);
    if (num_rows < 0 || num_cols < 0 || n < 0) return code(SpMVError::INVALID_DIMENSION);
    if (cfg.duplicates != COO_SUM && cfg.duplicates != COO_KEEP) return code(SpMVError::INVALID_ARGUMENT);
    if (cfg.reserved != 0) return code(SpMVError::INVALID_ARGUMENT);
    return 0;
}

int refill_check(const CooPlan* plan, const CSRMatrix* C, const float* d_vals) {
    if (!plan || !C || (!d_vals && plan->n > 0)) return code(SpMVError::INVALID_ARGUMENT);
    if (C->num_rows != plan->num_rows || C->num_cols != plan->num_cols || C->nnz != plan->nnz_out) {
        return code(SpMVError::INVALID_DIMENSION);
    }
    // (not device_arrays_strict: no sign check, the sizes are the plan's; not lenient: d_row_ptrs also without rows)
    if (!C->d_row_ptrs || (C->nnz > 0 && (!C->d_col_indices || !C->d_values))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    return 0;
}

int row_indices_check(const CSRMatrix* A, const int* d_rows, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || (!d_rows && A->nnz > 0)) return code(SpMVError::INVALID_ARGUMENT);
    if (!device_arrays_lenient(A)) return code(SpMVError::INVALID_FORMAT);
    if (A->num_rows == 0) *nothing_to_do = true;
    return 0;
}

} // namespace assemble
} // namespace detail

int csr_from_coo_cpu(CSRMatrix* C, int num_rows, int num_cols, int n, const int* rows, const int* cols,
                     const float* vals, const CooConfig* config) {
    using namespace detail;
    const CooConfig defaults;
    const CooConfig& cfg = config ? *config : defaults;
    const int status = assemble::build_check(C, num_rows, num_cols, n, rows, cols, vals, cfg);
    if (status != 0) return status;
    for (int p = 0; p < n; ++p) {
        if (rows[p] < 0 || rows[p] >= num_rows || cols[p] < 0 || cols[p] >= num_cols) {
            return code(SpMVError::INVALID_FORMAT);
        }
    }

    // (key, position) pairs: positions are distinct, so the plain sort of the pairs is the stable sort of the keys
    const assemble::KeyLayout layout = assemble::key_layout(num_rows, num_cols);
    struct Slot {
        uint64_t key;
        int pos;
    };
    std::vector<Slot> slots(static_cast<size_t>(n));
    for (int p = 0; p < n; ++p) {
        slots[p] = Slot{(static_cast<uint64_t>(rows[p]) << layout.col_bits) | static_cast<uint64_t>(cols[p]), p};
    }
    std::sort(slots.begin(), slots.end(),
              [](const Slot& a, const Slot& b) { return a.key < b.key || (a.key == b.key && a.pos < b.pos); });

    int nnz = n;
    if (cfg.duplicates == COO_SUM) {
        nnz = 0;
        for (int t = 0; t < n; ++t) nnz += t == 0 || slots[t].key != slots[t - 1].key;
    }
    float* new_vals = nnz > 0 ? new float[nnz] : nullptr;
    int* new_cols = nnz > 0 ? new int[nnz] : nullptr;
    int* new_ptrs = new int[static_cast<size_t>(num_rows) + 1];
    std::fill(new_ptrs, new_ptrs + num_rows + 1, 0);
    int out = 0;
    for (int t = 0; t < n;) {
        int end = t + 1;
        if (cfg.duplicates == COO_SUM) {
            while (end < n && slots[end].key == slots[t].key) ++end;
        }
        new_cols[out] = cols[slots[t].pos];
        ++new_ptrs[rows[slots[t].pos] + 1];
        if (end == t + 1) {
            std::memcpy(&new_vals[out], &vals[slots[t].pos], sizeof(float));      // the bits, whatever they are
        } else {
            float s = vals[slots[t].pos];
            for (int u = t + 1; u < end; ++u) s += vals[slots[u].pos];
            if (s != s) {                                                         // the NaN of an addition: one spelling
                const uint32_t quiet = 0x7FC00000u;
                std::memcpy(&s, &quiet, sizeof(float));
            }
            std::memcpy(&new_vals[out], &s, sizeof(float));
        }
        ++out;
        t = end;
    }
    for (int r = 0; r < num_rows; ++r) new_ptrs[r + 1] += new_ptrs[r];

    csr_adopt_host(C, num_rows, num_cols, nnz, new_ptrs, new_cols, new_vals);
    return code(SpMVError::SUCCESS);
}

int coo_plan_info(const CooPlan* plan, int* num_rows, int* num_cols, int* n, int* nnz_out, int* duplicates) {
    if (!plan) return detail::code(SpMVError::INVALID_ARGUMENT);
    if (num_rows) *num_rows = plan->num_rows;
    if (num_cols) *num_cols = plan->num_cols;
    if (n) *n = plan->n;
    if (nnz_out) *nnz_out = plan->nnz_out;
    if (duplicates) *duplicates = plan->duplicates;
    return detail::code(SpMVError::SUCCESS);
}

} // namespace spmv
