// bsr_tri_host.cpp — the host side of include/spmv/bsr_factor.h: bsr_ic0_cpu and sptrsv_cpu_bsr,
// which define what the kernels of bsr_tri.hip compute, the argument checks of the device entry points (and of
// cg_solve_bsr_ic), the schedule of the block pattern, and the drivers.
// Compiled with -ffp-contract=off: the fused multiply-adds are bsr_tri_impl.h's explicit ones and nothing else, and
// every fp64 operation of the diagonal stage and every product and sum of the solve is a rounding of its own.
#include "bsr_impl.h"
#include "bsr_tri_impl.h"
#include "internal.h"
#include "level_driver.h"

#include <algorithm>
#include <cstdint>
#include <cstring>
#include <vector>

namespace spmv {

namespace detail {
namespace bsr {
namespace {

size_t value_count(const BSRMatrix* M) {
    return static_cast<size_t>(M->num_blocks) * M->block_dim * M->block_dim;
}

bool host_arrays(const BSRMatrix* M) {
    return shape_ok(M) && M->block_row_ptrs && (M->num_blocks == 0 || (M->block_cols && M->values));
}

// the block pattern on the host: row pointers inside [0, num_blocks] and not decreasing, block columns in
// [0, num_block_rows)
bool host_pattern_ok(const BSRMatrix* M) {
    const int nbr = M->num_block_rows;
    const int* ptr = M->block_row_ptrs;
    if (ptr[0] < 0 || ptr[nbr] > M->num_blocks) return false;
    for (int I = 0; I < nbr; ++I) {
        if (ptr[I + 1] < ptr[I]) return false;
    }
    for (int p = ptr[0]; p < ptr[nbr]; ++p) {
        if (M->block_cols[p] < 0 || M->block_cols[p] >= nbr) return false;
    }
    return true;
}

// the checks the two host twins and the device entry points share: null, square, no rows
int check_front(const BSRMatrix* M, const void* p, const void* q, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!M || !p || !q) return code(SpMVError::INVALID_ARGUMENT);
    if (M->num_rows != M->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (M->num_rows == 0) *nothing_to_do = true;
    return 0;
}

template <int B>
int ic0_cpu(const BSRMatrix* A, const std::vector<int>& diagonal, float* f) {
    constexpr int BB = B * B;
    const int n = A->num_rows, nbr = A->num_block_rows;
    const int* ptr = A->block_row_ptrs;
    const int* col = A->block_cols;
    const float* a = A->values;
    int bad = -1;
    // next[K]: the upper position of block row K that the next block row below it with a stored (I,K) mirrors into.
    // The pattern is symmetric and the block rows run in ascending I, so that position is (K,I).
    std::vector<int> next(static_cast<size_t>(nbr));
    for (int I = 0; I < nbr; ++I) next[I] = diagonal[I] + 1;
    for (int I = 0; I < nbr; ++I) {
        const int di = diagonal[I];
        const int size = std::min(B, n - I * B);
        if (f != a) {
            std::memcpy(f + static_cast<size_t>(ptr[I]) * BB, a + static_cast<size_t>(ptr[I]) * BB,
                        static_cast<size_t>(di + 1 - ptr[I]) * BB * sizeof(float));
        }
        float* wd = f + static_cast<size_t>(di) * BB;
        for (int pk = ptr[I]; pk < di; ++pk) {
            const int K = col[pk];
            const float* V = f + static_cast<size_t>(diagonal[K]) * BB;
            float* lk = f + static_cast<size_t>(pk) * BB;
            float L[BB];
            for (int r = 0; r < B; ++r) {
                float w[B];
                for (int c = 0; c < B; ++c) {
                    w[c] = lk[r * B + c];
                    L[r * B + c] = 0.0f;
                }
                if (r < size) ic_scale_row<B>(w, V, L + r * B);
            }
            std::memcpy(lk, L, sizeof(L));
            // the stored J of block row I with K < J < I that block row K also stores: both ascend, one merge; L_JK^T
            // is read from (K,J), where block row J put it when it finished
            int q = diagonal[K] + 1;
            const int q_end = ptr[K + 1];
            for (int t = pk + 1; t < di && q < q_end; ++t) {
                while (q < q_end && col[q] < col[t]) ++q;
                if (q < q_end && col[q] == col[t]) {
                    for (int r = 0; r < size; ++r) {
                        ic_update_row<B>(L + r * B, f + static_cast<size_t>(q) * BB,
                                         f + static_cast<size_t>(t) * BB + r * B);
                    }
                }
            }
            for (int r = 0; r < size; ++r) ic_diag_row<B>(L + r * B, L, r, wd + r * B);
            float* up = f + static_cast<size_t>(next[K]++) * BB;         // (K,I)
            for (int r = 0; r < B; ++r) {
                for (int m = 0; m < B; ++m) up[m * B + r] = L[r * B + m];
            }
        }
        double T[B * (B + 1) / 2];
        for (int r = 0; r < B; ++r) {
            for (int c = 0; c <= r; ++c) T[tri(r, c)] = r < size ? static_cast<double>(wd[r * B + c]) : 0.0;
        }
        if (!ic_diag_stage<B>(T, size) && bad < 0) bad = I;
        for (int r = 0; r < B; ++r) {
            for (int c = 0; c < B; ++c) wd[r * B + c] = ic_v_entry<B>(T, r, c, size);
        }
    }
    return bad;
}

template <int B>
void sptrsv_cpu(const BSRMatrix* F, const float* b, float* x, bool upper, bool unit) {
    constexpr int BB = B * B;
    const int n = F->num_rows, nbr = F->num_block_rows;
    const int* ptr = F->block_row_ptrs;
    const int* col = F->block_cols;
    for (int step = 0; step < nbr; ++step) {
        const int I = upper ? nbr - 1 - step : step;
        const int size = std::min(B, n - I * B);
        float s[B], t[B];
        for (int r = 0; r < B; ++r) s[r] = 0.0f;
        int d = -1;
        for (int p = ptr[I]; p < ptr[I + 1]; ++p) {
            const int J = col[p];
            if (J == I) d = p;
            if (upper ? J <= I : J >= I) continue;
            const float* v = F->values + static_cast<size_t>(p) * BB;
            for (int c = 0; c < B && J * B + c < n; ++c) {
                const float xc = x[J * B + c];
                for (int r = 0; r < size; ++r) s[r] = add_rn(s[r], mul_rn(v[r * B + c], xc));
            }
        }
        for (int r = 0; r < B; ++r) t[r] = r < size ? b[I * B + r] - s[r] : 0.0f;
        if (unit) {
            for (int r = 0; r < size; ++r) x[I * B + r] = t[r];
        } else {
            const float* V = F->values + static_cast<size_t>(d) * BB;
            for (int r = 0; r < size; ++r) x[I * B + r] = tri_diag_row<B>(V, t, r, size, upper);
        }
    }
}

// the checks of the device entry points after check_front, up to the schedule
int device_matrix_check(const BSRMatrix* M) {
    return device_arrays_ok(M) ? 0 : code(SpMVError::INVALID_FORMAT);
}

// sptrsv_bsr and sptrsv_bsr_async as an Op of level_driver.h
struct BlockSolve {
    const BSRMatrix* F;
    const float* d_b;
    float* d_x;
    SpTRSVConfig cfg;
    int prepare(hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) const {
        schedule->reset();
        *analysis_ms = 0.0f;
        bool nothing = false;
        int status = check_front(F, d_b, d_x, &nothing);
        if (status != 0 || nothing) return status;
        status = device_matrix_check(F);
        if (status != 0) return status;
        if (!config_ok(cfg)) return code(SpMVError::INVALID_ARGUMENT);
        if (partial_overlap(d_b, d_x, F->num_rows)) return code(SpMVError::INVALID_ARGUMENT);
        ScheduleRef found;
        status = tri_schedule_for(F, cfg.uplo, stream, &found, analysis_ms);
        if (status != 0) return status;
        // NON_UNIT reads the diagonal block, which the kernel finds by a binary search: the block columns must ascend
        if (cfg.diag == SpTRSVConfig::NON_UNIT &&
            (found->first_missing_diagonal >= 0 || found->first_unsorted_row >= 0)) {
            return code(SpMVError::INVALID_ARGUMENT);
        }
        *schedule = found;
        return 0;
    }
    int lanes(const SptrsvSchedule& schedule) const { return tri_lanes(schedule, cfg.ordered == 1); }
    hipError_t launch(const SptrsvSchedule& schedule, int lanes, hipStream_t stream) const {
        return launch_sptrsv_bsr(schedule, F, d_b, d_x, cfg.uplo, cfg.diag == SpTRSVConfig::UNIT, cfg.ordered == 1,
                                 lanes, stream);
    }
};

// bsr_ic0 and bsr_ic0_async
struct BlockFactor {
    const BSRMatrix* A;
    float* d_f;
    int prepare(hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) const {
        schedule->reset();
        *analysis_ms = 0.0f;
        bool nothing = false;
        int status = check_front(A, d_f, d_f, &nothing);
        if (status != 0 || nothing) return status;
        status = device_matrix_check(A);
        if (status != 0) return status;
        if (partial_overlap(A->d_values, d_f, static_cast<long long>(value_count(A)))) {
            return code(SpMVError::INVALID_ARGUMENT);
        }
        ScheduleRef found;
        status = tri_schedule_for(A, SpTRSVConfig::LOWER, stream, &found, analysis_ms);
        if (status != 0) return status;
        if (found->first_unsorted_row >= 0 || found->first_missing_diagonal >= 0 || found->one_sided_row >= 0) {
            return code(SpMVError::INVALID_ARGUMENT);
        }
        *schedule = found;
        return 0;
    }
    int lanes(const SptrsvSchedule& schedule) const { return tri_lanes(schedule, false); }
    hipError_t launch(const SptrsvSchedule& schedule, int lanes, hipStream_t stream, unsigned* d_pivot) const {
        return launch_bsr_ic0(schedule, A, A->d_values, d_f, lanes, d_pivot, stream);
    }
};

} // namespace

int tri_schedule_for(const BSRMatrix* M, int uplo, hipStream_t stream, ScheduleRef* out, float* analysis_ms) {
    CSRMatrix pattern{};                 // the block pattern is a CSR structure of num_block_rows rows
    pattern.num_rows = M->num_block_rows;
    pattern.num_cols = M->num_block_rows;
    pattern.nnz = M->num_blocks;
    pattern.d_row_ptrs = M->d_block_row_ptrs;
    pattern.d_col_indices = M->d_block_cols;
    pattern.d_values = M->d_values;      // never read: the analysis is structure only
    return sptrsv_schedule_for(&pattern, uplo, stream, out, analysis_ms);
}

int tri_lanes(const SptrsvSchedule& schedule, bool ordered) {
    if (ordered) return 1;
    if (int f = forced_lanes("bsr_tri_lanes")) return f;
    return pick_lanes_per_row(2.0f * static_cast<float>(schedule.triangle_nnz) /
                              static_cast<float>(std::max(schedule.num_rows, 1)));
}

int cg_ic_check(const BSRMatrix* A, const BSRMatrix* F) {
    if (!F) return code(SpMVError::INVALID_ARGUMENT);
    if (F->num_rows != F->num_cols || F->num_rows != A->num_rows || F->block_dim != A->block_dim) {
        return code(SpMVError::INVALID_DIMENSION);
    }
    return device_arrays_ok(F) ? 0 : code(SpMVError::INVALID_FORMAT);
}

} // namespace bsr
} // namespace detail

int bsr_ic0_cpu(const BSRMatrix* A, float* f_values, int* bad_pivot) {
    using namespace detail;
    using namespace detail::bsr;
    bool nothing = false;
    const int status = check_front(A, f_values, f_values, &nothing);
    if (status != 0) return status;
    if (nothing) {
        if (bad_pivot) *bad_pivot = -1;
        return 0;
    }
    if (!host_arrays(A)) return code(SpMVError::INVALID_FORMAT);
    if (partial_overlap(A->values, f_values, static_cast<long long>(value_count(A)))) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    if (!host_pattern_ok(A)) return code(SpMVError::INVALID_FORMAT);
    const int nbr = A->num_block_rows;
    const int* ptr = A->block_row_ptrs;
    const int* col = A->block_cols;
    std::vector<int> diagonal(static_cast<size_t>(nbr), -1);
    bool ascending = true;
    for (int I = 0; I < nbr; ++I) {
        for (int p = ptr[I]; p < ptr[I + 1]; ++p) {
            if (p > ptr[I] && col[p] <= col[p - 1]) ascending = false;
            if (col[p] == I) diagonal[I] = p;
        }
    }
    if (!ascending) return code(SpMVError::INVALID_ARGUMENT);
    for (int I = 0; I < nbr; ++I) {
        if (diagonal[I] < 0) return code(SpMVError::INVALID_ARGUMENT);
    }
    if (one_sided_row(nbr, ptr, col) >= 0) return code(SpMVError::INVALID_ARGUMENT);
    int bad = -1;
    switch (A->block_dim) {
        case 2:  bad = ic0_cpu<2>(A, diagonal, f_values); break;
        case 3:  bad = ic0_cpu<3>(A, diagonal, f_values); break;
        case 4:  bad = ic0_cpu<4>(A, diagonal, f_values); break;
        default: bad = ic0_cpu<8>(A, diagonal, f_values); break;
    }
    if (bad_pivot) *bad_pivot = bad;
    return 0;
}

int sptrsv_cpu_bsr(const BSRMatrix* F, const float* b, float* x, const SpTRSVConfig* config) {
    using namespace detail;
    using namespace detail::bsr;
    bool nothing = false;
    const int status = check_front(F, b, x, &nothing);
    if (status != 0 || nothing) return status;
    if (!host_arrays(F)) return code(SpMVError::INVALID_FORMAT);
    const SpTRSVConfig cfg = config_or_default(config);
    if (!config_ok(cfg)) return code(SpMVError::INVALID_ARGUMENT);
    if (partial_overlap(b, x, F->num_rows)) return code(SpMVError::INVALID_ARGUMENT);
    if (!host_pattern_ok(F)) return code(SpMVError::INVALID_FORMAT);
    const bool upper = cfg.uplo == SpTRSVConfig::UPPER;
    const bool unit = cfg.diag == SpTRSVConfig::UNIT;
    if (!unit) {                         // the device's rule: a diagonal block in every block row, found in ascending columns
        for (int I = 0; I < F->num_block_rows; ++I) {
            bool diagonal = false;
            for (int p = F->block_row_ptrs[I]; p < F->block_row_ptrs[I + 1]; ++p) {
                diagonal |= F->block_cols[p] == I;
                if (p > F->block_row_ptrs[I] && F->block_cols[p] <= F->block_cols[p - 1]) {
                    return code(SpMVError::INVALID_ARGUMENT);
                }
            }
            if (!diagonal) return code(SpMVError::INVALID_ARGUMENT);
        }
    }
    switch (F->block_dim) {
        case 2:  sptrsv_cpu<2>(F, b, x, upper, unit); break;
        case 3:  sptrsv_cpu<3>(F, b, x, upper, unit); break;
        case 4:  sptrsv_cpu<4>(F, b, x, upper, unit); break;
        default: sptrsv_cpu<8>(F, b, x, upper, unit); break;
    }
    return 0;
}

BsrIC0Result bsr_ic0(const BSRMatrix* A, float* d_f_values) {
    using namespace detail;
    return factor_result(timed_factor("spmv:bsr_ic0", bsr::BlockFactor{A, d_f_values}), &BsrIC0Result::bad_pivot);
}

int bsr_ic0_async(const BSRMatrix* A, float* d_f_values, hipStream_t stream) {
    return detail::launch_factor_async(detail::bsr::BlockFactor{A, d_f_values}, stream);
}

SpTRSVResult sptrsv_bsr(const BSRMatrix* F, const float* d_b, float* d_x, const SpTRSVConfig* config) {
    using namespace detail;
    return timed_solve("spmv:sptrsv_bsr", bsr::BlockSolve{F, d_b, d_x, config_or_default(config)});
}

int sptrsv_bsr_async(const BSRMatrix* F, const float* d_b, float* d_x, const SpTRSVConfig* config, hipStream_t stream) {
    using namespace detail;
    return launch_async(bsr::BlockSolve{F, d_b, d_x, config_or_default(config)}, stream);
}

SpTRSVResult sptrsv_analyze_bsr(const BSRMatrix* A, int uplo) {
    using namespace detail;
    using namespace detail::bsr;
    return analyze_levels(
        uplo,
        [&](bool* nothing) {
            const int status = check_front(A, A, A, nothing);
            return status != 0 || *nothing ? status : device_matrix_check(A);
        },
        [&](hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) {
            return tri_schedule_for(A, uplo, stream, schedule, analysis_ms);
        });
}

} // namespace spmv
