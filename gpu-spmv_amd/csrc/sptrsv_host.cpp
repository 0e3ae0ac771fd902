// sptrsv_host.cpp — host side of the sparse triangular solve (include/spmv/sptrsv.h): the level
// analysis, the schedule kept with the matrix, the host substitution sptrsv_cpu_csr and the entry points.  The
// kernels are in sptrsv.hip.  Built without FMA contraction: sptrsv_cpu_csr rounds the product, then the sum.
#include "internal.h"
#include "level_driver.h"
#include "spmv/sptrsv.h"

#include <algorithm>
#include <chrono>
#include <cstdint>
#include <vector>

namespace spmv {

namespace detail {
namespace {

// B and X of a k-wide solve (num_rows x k, leading dimensions ldb, ldx) overlap without being the solve in place
bool multi_overlap(const float* B, int ldb, const float* X, int ldx, int k, int num_rows) {
    if (B == X && ldb == ldx) return false;
    const long long rows = num_rows - 1;
    return spans_overlap(B, rows * ldb + k, X, rows * ldx + k);
}

} // namespace
} // namespace detail

int sptrsv_levels(int num_rows, const int* row_ptrs, const int* col_indices, int uplo, int* level_ptr, int* order,
                  int* num_levels, int* first_missing_diagonal) {
    using detail::code;
    if (num_rows < 0 || !row_ptrs || !level_ptr || !num_levels || (num_rows > 0 && !order) ||
        !detail::uplo_ok(uplo)) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const int n = num_rows;
    if (row_ptrs[0] < 0) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < n; ++i) {
        if (row_ptrs[i + 1] < row_ptrs[i]) return code(SpMVError::INVALID_FORMAT);
    }
    if (row_ptrs[n] > row_ptrs[0] && !col_indices) return code(SpMVError::INVALID_ARGUMENT);
    for (int j = row_ptrs[0]; j < row_ptrs[n]; ++j) {
        if (col_indices[j] < 0 || col_indices[j] >= n) return code(SpMVError::INVALID_FORMAT);
    }

    // level of every row, in the order the substitution visits them; `order` holds the levels until the sort
    const bool upper = uplo == SpTRSVConfig::UPPER;
    int missing = -1;
    int levels = 0;
    for (int step = 0; step < n; ++step) {
        const int i = upper ? n - 1 - step : step;
        int level = 0;
        bool diagonal = false;
        for (int j = row_ptrs[i]; j < row_ptrs[i + 1]; ++j) {
            const int c = col_indices[j];
            if (c == i) {
                diagonal = true;
            } else if (upper ? c > i : c < i) {
                level = std::max(level, order[c] + 1);
            }
        }
        order[i] = level;
        levels = std::max(levels, level + 1);
        if (!diagonal && (missing < 0 || i < missing)) missing = i;
    }

    // counting sort by level, rows ascending within a level
    std::vector<int> level_of(order, order + n);
    std::fill(level_ptr, level_ptr + levels + 1, 0);
    for (int i = 0; i < n; ++i) ++level_ptr[level_of[i] + 1];
    for (int l = 0; l < levels; ++l) level_ptr[l + 1] += level_ptr[l];
    std::vector<int> next(level_ptr, level_ptr + levels);
    for (int i = 0; i < n; ++i) order[next[level_of[i]]++] = i;

    *num_levels = levels;
    if (first_missing_diagonal) *first_missing_diagonal = missing;
    return code(SpMVError::SUCCESS);
}

int sptrsv_cpu_csr(const CSRMatrix* A, const float* b, float* x, const SpTRSVConfig* config) {
    using detail::code;
    if (!A || !b || !x) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n == 0) return code(SpMVError::SUCCESS);
    if (n < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values))) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const SpTRSVConfig cfg = detail::config_or_default(config);
    if (!detail::uplo_ok(cfg.uplo) || !detail::diag_ok(cfg.diag)) return code(SpMVError::INVALID_ARGUMENT);
    const bool upper = cfg.uplo == SpTRSVConfig::UPPER;
    const bool unit = cfg.diag == SpTRSVConfig::UNIT;
    const int* ptr = A->row_ptrs;
    const int* col = A->col_indices;
    // everything that can fail, before x is touched
    if (ptr[0] < 0 || ptr[n] > A->nnz) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < n; ++i) {
        if (ptr[i + 1] < ptr[i]) return code(SpMVError::INVALID_FORMAT);
    }
    bool every_diagonal = true;
    for (int i = 0; i < n; ++i) {
        bool diagonal = false;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            if (col[j] < 0 || col[j] >= n) return code(SpMVError::INVALID_FORMAT);
            diagonal |= col[j] == i;
        }
        every_diagonal &= diagonal;
    }
    if (!unit && !every_diagonal) return code(SpMVError::INVALID_ARGUMENT);

    for (int step = 0; step < n; ++step) {
        const int i = upper ? n - 1 - step : step;
        float s = 0.0f;
        float d = 0.0f;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            const int c = col[j];
            if (c == i) {
                d = d + A->values[j];
            } else if (upper ? c > i : c < i) {
                const float product = A->values[j] * x[c];
                s = s + product;
            }
        }
        x[i] = (b[i] - s) / (unit ? 1.0f : d);
    }
    return code(SpMVError::SUCCESS);
}

int sptrsv_cpu_csr_multi(const CSRMatrix* A, const float* B, int ldb, float* X, int ldx, int k,
                         const SpTRSVConfig* config) {
    using detail::code;
    if (!A || !B || !X) return code(SpMVError::INVALID_ARGUMENT);
    if (k < 1 || k > 32) return code(SpMVError::INVALID_ARGUMENT);
    if (ldb < k || ldx < k) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    const int n = A->num_rows;
    if (n == 0) return code(SpMVError::SUCCESS);
    if (n < 0 || !A->row_ptrs || (A->nnz > 0 && (!A->col_indices || !A->values))) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    const SpTRSVConfig cfg = detail::config_or_default(config);
    if (!detail::uplo_ok(cfg.uplo) || !detail::diag_ok(cfg.diag)) return code(SpMVError::INVALID_ARGUMENT);
    if (detail::multi_overlap(B, ldb, X, ldx, k, n)) return code(SpMVError::INVALID_ARGUMENT);
    const bool upper = cfg.uplo == SpTRSVConfig::UPPER;
    const bool unit = cfg.diag == SpTRSVConfig::UNIT;
    const int* ptr = A->row_ptrs;
    const int* col = A->col_indices;
    // everything that can fail, before X is touched
    if (ptr[0] < 0 || ptr[n] > A->nnz) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < n; ++i) {
        if (ptr[i + 1] < ptr[i]) return code(SpMVError::INVALID_FORMAT);
    }
    bool every_diagonal = true;
    for (int i = 0; i < n; ++i) {
        bool diagonal = false;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            if (col[j] < 0 || col[j] >= n) return code(SpMVError::INVALID_FORMAT);
            diagonal |= col[j] == i;
        }
        every_diagonal &= diagonal;
    }
    if (!unit && !every_diagonal) return code(SpMVError::INVALID_ARGUMENT);

    // sptrsv_cpu_csr's substitution with the row's entries walked once per column; the diagonal once per row
    for (int step = 0; step < n; ++step) {
        const int i = upper ? n - 1 - step : step;
        float d = 0.0f;
        for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
            if (col[j] == i) d = d + A->values[j];
        }
        const size_t row_b = static_cast<size_t>(i) * ldb, row_x = static_cast<size_t>(i) * ldx;
        for (int q = 0; q < k; ++q) {
            float s = 0.0f;
            for (int j = ptr[i]; j < ptr[i + 1]; ++j) {
                const int c = col[j];
                if (c != i && (upper ? c > i : c < i)) {
                    const float product = A->values[j] * X[static_cast<size_t>(c) * ldx + q];
                    s = s + product;
                }
            }
            X[row_x + q] = (B[row_b + q] - s) / (unit ? 1.0f : d);
        }
    }
    return code(SpMVError::SUCCESS);
}

namespace detail {

SptrsvSchedule::~SptrsvSchedule() {
    if (d_level_ptr) (void)hipFree(d_level_ptr);
    if (d_order) (void)hipFree(d_order);
}

namespace {

// One launch per group: a level wider than kSptrsvNarrowRows alone, consecutive narrower ones together.
void group_levels(const std::vector<int>& level_ptr, int num_levels, std::vector<SptrsvSchedule::Group>* groups) {
    groups->clear();
    bool open = false;       // the last group is a run that may take another narrow level
    for (int l = 0; l < num_levels; ++l) {
        const int rows = level_ptr[l + 1] - level_ptr[l];
        const bool narrow = rows <= kSptrsvNarrowRows;
        if (narrow && open && groups->back().level_end - groups->back().level_begin < kSptrsvMaxRunLevels) {
            groups->back().level_end = l + 1;
            groups->back().rows = std::max(groups->back().rows, rows);
        } else {
            groups->push_back({l, l + 1, rows});
            open = narrow;
        }
    }
}

bool matches(const ScheduleRef& s, const CSRMatrix* A, int uplo) {
    return s && s->row_ptrs == A->d_row_ptrs && s->cols == A->d_col_indices && s->nnz == A->nnz &&
           s->num_rows == A->num_rows && s->num_cols == A->num_cols && s->uplo == uplo;
}

// The host analysis: one read-back of the structure, sptrsv_levels, the statistics, the upload.  *level_ptr is left
// for the grouping.
int build_on_host(const CSRMatrix* A, int uplo, hipStream_t stream, SptrsvSchedule* built, std::vector<int>* level_ptr) {
    const int n = A->num_rows;
    const size_t nnz = static_cast<size_t>(std::max(A->nnz, 0));

    // one read-back of the structure (the device arrays are what the kernels walk; host arrays may be absent)
    std::vector<int> row_ptrs(static_cast<size_t>(n) + 1), cols(nnz);
    bool ok = hipMemcpyAsync(row_ptrs.data(), A->d_row_ptrs, row_ptrs.size() * sizeof(int), hipMemcpyDeviceToHost,
                             stream) == hipSuccess;
    if (ok && nnz > 0) {
        ok = hipMemcpyAsync(cols.data(), A->d_col_indices, nnz * sizeof(int), hipMemcpyDeviceToHost, stream) ==
             hipSuccess;
    }
    if (!ok || hipStreamSynchronize(stream) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MEMCPY);
    }
    if (row_ptrs[0] < 0 || row_ptrs[n] > A->nnz) return code(SpMVError::INVALID_FORMAT);
    for (int i = 0; i < n; ++i) {        // (before sptrsv_levels reads cols[row_ptrs[0] .. row_ptrs[n]))
        if (row_ptrs[i + 1] < row_ptrs[i]) return code(SpMVError::INVALID_FORMAT);
    }

    level_ptr->assign(static_cast<size_t>(n) + 1, 0);
    std::vector<int> order(static_cast<size_t>(n));
    int num_levels = 0, missing = -1;
    const int status = sptrsv_levels(n, row_ptrs.data(), cols.data(), uplo, level_ptr->data(), order.data(),
                                     &num_levels, &missing);
    if (status != 0) return status;

    built->num_levels = num_levels;
    built->first_missing_diagonal = missing;
    const bool upper = uplo == SpTRSVConfig::UPPER;
    for (int i = 0; i < n; ++i) {
        for (int j = row_ptrs[i]; j < row_ptrs[i + 1]; ++j) {
            built->triangle_nnz += upper ? cols[j] >= i : cols[j] <= i;
            if (j > row_ptrs[i] && cols[j] <= cols[j - 1] && built->first_unsorted_row < 0) {
                built->first_unsorted_row = i;
            }
        }
    }
    if (!upper && missing < 0 && built->first_unsorted_row < 0) {
        built->one_sided_row = one_sided_row(n, row_ptrs.data(), cols.data());
    }
    const size_t ptr_bytes = (static_cast<size_t>(num_levels) + 1) * sizeof(int);
    const size_t order_bytes = static_cast<size_t>(n) * sizeof(int);
    if (malloc_any_time(reinterpret_cast<void**>(&built->d_level_ptr), ptr_bytes) != hipSuccess ||
        malloc_any_time(reinterpret_cast<void**>(&built->d_order), order_bytes) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MALLOC);
    }
    if (hipMemcpyAsync(built->d_level_ptr, level_ptr->data(), ptr_bytes, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipMemcpyAsync(built->d_order, order.data(), order_bytes, hipMemcpyHostToDevice, stream) != hipSuccess ||
        hipStreamSynchronize(stream) != hipSuccess) {       // (the host vectors go away with this frame)
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MEMCPY);
    }
    return code(SpMVError::SUCCESS);
}

// A's schedule for `uplo` from its aux entry, built when it is not there or no longer matches A: on the device when
// the caller asks for it or SPMV_DEBUG holds sptrsv_analysis=device, else on the host.  *analysis_ms is the wall time
// of a build, 0 for a cache hit (of either origin).
int schedule_for(const CSRMatrix* A, int uplo, hipStream_t stream, ScheduleRef* out, float* analysis_ms,
                 bool on_device = false) {
    *analysis_ms = 0.0f;
    CsrAux* aux = aux_lookup(A->d_row_ptrs, true);
    std::lock_guard<std::mutex> guard(aux->sptrsv_lock);
    if (matches(aux->sptrsv[uplo], A, uplo)) {
        *out = aux->sptrsv[uplo];
        return code(SpMVError::SUCCESS);
    }
    aux->sptrsv[uplo].reset();
    const TraceRange range("spmv:sptrsv_analysis");
    const auto t0 = std::chrono::steady_clock::now();

    auto built = std::make_shared<SptrsvSchedule>();
    std::vector<int> level_ptr;
    const int status = on_device || debug_is("sptrsv_analysis", "device")
                           ? sptrsv_analysis_device(A, uplo, stream, built.get(), &level_ptr)
                           : build_on_host(A, uplo, stream, built.get(), &level_ptr);
    if (status != 0) return status;
    group_levels(level_ptr, built->num_levels, &built->groups);
    built->row_ptrs = A->d_row_ptrs;
    built->cols = A->d_col_indices;
    built->nnz = A->nnz;
    built->num_rows = A->num_rows;
    built->num_cols = A->num_cols;
    built->uplo = uplo;
    aux->sptrsv[uplo] = built;
    *out = built;
    *analysis_ms = std::max(std::chrono::duration<float, std::milli>(std::chrono::steady_clock::now() - t0).count(),
                            1e-6f);
    return code(SpMVError::SUCCESS);
}

// checks 1-4 of sptrsv.h, shared by the solve and sptrsv_analyze
int check_matrix(const CSRMatrix* A, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (A->num_rows != A->num_cols) return code(SpMVError::INVALID_DIMENSION);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return code(SpMVError::SUCCESS);
    }
    // (not device_arrays_strict: a negative nnz fails here, there it counts as no entries)
    if (A->num_rows < 0 || A->nnz < 0 || !A->d_row_ptrs || (A->nnz > 0 && (!A->d_col_indices || !A->d_values))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    return code(SpMVError::SUCCESS);
}

int lanes_for(const SptrsvSchedule& s, bool ordered) {
    if (ordered) return 1;
    if (int f = forced_lanes("sptrsv_lanes")) return f;
    return pick_lanes_per_row(static_cast<float>(s.triangle_nnz) / static_cast<float>(s.num_rows));
}

// Everything before the launches, from the dimension check on.  overlaps(): the arrays overlap in a way the solve
// does not allow (asked once A's dimensions are known to be sane).  On SUCCESS with *schedule null there is nothing
// to do (no rows).
template <class Overlaps>
int prepare_checked(const CSRMatrix* A, const SpTRSVConfig& cfg, hipStream_t stream, Overlaps&& overlaps,
                    ScheduleRef* schedule, float* analysis_ms) {
    bool nothing = false;
    const int status = check_matrix(A, &nothing);
    if (status != 0 || nothing) return status;
    if (!config_ok(cfg)) return code(SpMVError::INVALID_ARGUMENT);
    if (overlaps()) return code(SpMVError::INVALID_ARGUMENT);
    ScheduleRef found;
    const int analysed = schedule_for(A, cfg.uplo, stream, &found, analysis_ms);
    if (analysed != 0) return analysed;
    if (cfg.diag == SpTRSVConfig::NON_UNIT && found->first_missing_diagonal >= 0) {
        return code(SpMVError::INVALID_ARGUMENT);
    }
    *schedule = found;
    return code(SpMVError::SUCCESS);
}

constexpr int kMaxColumns = 32;

// sptrsv_csr and sptrsv_csr_async as an Op of level_driver.h
struct CsrSolve {
    const CSRMatrix* A;
    const float* d_b;
    float* d_x;
    SpTRSVConfig cfg;
    int prepare(hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) const {
        schedule->reset();
        *analysis_ms = 0.0f;
        if (!A || !d_b || !d_x) return code(SpMVError::INVALID_ARGUMENT);
        return prepare_checked(A, cfg, stream, [&] { return partial_overlap(d_b, d_x, A->num_rows); }, schedule,
                               analysis_ms);
    }
    int lanes(const SptrsvSchedule& schedule) const { return lanes_for(schedule, cfg.ordered == 1); }
    hipError_t launch(const SptrsvSchedule& schedule, int lanes, hipStream_t stream) const {
        return launch_sptrsv(schedule, A, d_b, d_x, cfg.uplo, cfg.diag == SpTRSVConfig::UNIT, cfg.ordered == 1, lanes,
                             stream);
    }
};

// sptrsv_csr_multi and sptrsv_csr_multi_async
struct CsrMultiSolve {
    const CSRMatrix* A;
    const float* d_B;
    int ldb;
    float* d_X;
    int ldx, k;
    SpTRSVConfig cfg;
    int prepare(hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) const {
        schedule->reset();
        *analysis_ms = 0.0f;
        // the checks that come before sptrsv_csr's
        if (!A || !d_B || !d_X) return code(SpMVError::INVALID_ARGUMENT);
        if (k < 1 || k > kMaxColumns) return code(SpMVError::INVALID_ARGUMENT);
        if (ldb < k || ldx < k) return code(SpMVError::INVALID_ARGUMENT);
        return prepare_checked(A, cfg, stream, [&] { return multi_overlap(d_B, ldb, d_X, ldx, k, A->num_rows); },
                               schedule, analysis_ms);
    }
    int lanes(const SptrsvSchedule& schedule) const { return lanes_for(schedule, cfg.ordered == 1); }
    hipError_t launch(const SptrsvSchedule& schedule, int lanes, hipStream_t stream) const {
        // the caller's arrays under sptrsv_multi.hip's addressing rule: the windows of w columns lie side by side in a row
        const int w = k <= 4 ? 4 : 8;
        return launch_sptrsv_multi(schedule, A, SptrsvMultiArrays{d_B, ldb, w, d_X, ldx, w, k, w}, cfg.uplo,
                                   cfg.diag == SpTRSVConfig::UNIT, cfg.ordered == 1, lanes, stream);
    }
};

} // namespace

int sptrsv_check_matrix(const CSRMatrix* A, bool* nothing_to_do) { return check_matrix(A, nothing_to_do); }

int sptrsv_schedule_for(const CSRMatrix* A, int uplo, hipStream_t stream, ScheduleRef* out, float* analysis_ms) {
    return schedule_for(A, uplo, stream, out, analysis_ms);
}

int sptrsv_lanes_for(const SptrsvSchedule& schedule) { return lanes_for(schedule, false); }

} // namespace detail

SpTRSVResult sptrsv_csr(const CSRMatrix* A, const float* d_b, float* d_x, const SpTRSVConfig* config) {
    using namespace detail;
    return timed_solve("spmv:sptrsv_csr", CsrSolve{A, d_b, d_x, config_or_default(config)});
}

int sptrsv_csr_async(const CSRMatrix* A, const float* d_b, float* d_x, const SpTRSVConfig* config,
                     hipStream_t stream) {
    using namespace detail;
    return launch_async(CsrSolve{A, d_b, d_x, config_or_default(config)}, stream);
}

SpTRSVResult sptrsv_csr_multi(const CSRMatrix* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                              const SpTRSVConfig* config) {
    using namespace detail;
    return timed_solve("spmv:sptrsv_csr_multi", CsrMultiSolve{A, d_B, ldb, d_X, ldx, k, config_or_default(config)});
}

int sptrsv_csr_multi_async(const CSRMatrix* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                           const SpTRSVConfig* config, hipStream_t stream) {
    using namespace detail;
    return launch_async(CsrMultiSolve{A, d_B, ldb, d_X, ldx, k, config_or_default(config)}, stream);
}

namespace detail {
namespace {

// sptrsv_analyze and sptrsv_analyze_device: the same checks in the same order, then the cache
SpTRSVResult analyze(const CSRMatrix* A, int uplo, bool on_device) {
    return analyze_levels(
        uplo,
        [&](bool* nothing) { return A ? check_matrix(A, nothing) : code(SpMVError::INVALID_ARGUMENT); },
        [&](hipStream_t stream, ScheduleRef* schedule, float* analysis_ms) {
            return schedule_for(A, uplo, stream, schedule, analysis_ms, on_device);
        });
}

} // namespace
} // namespace detail

SpTRSVResult sptrsv_analyze(const CSRMatrix* A, int uplo) { return detail::analyze(A, uplo, false); }

SpTRSVResult sptrsv_analyze_device(const CSRMatrix* A, int uplo) { return detail::analyze(A, uplo, true); }

int sptrsv_schedule_get(const CSRMatrix* A, int uplo, int* level_ptr, int* order, SpTRSVScheduleInfo* info) {
    using namespace detail;
    if (!A) return code(SpMVError::INVALID_ARGUMENT);
    if (!uplo_ok(uplo)) return code(SpMVError::INVALID_ARGUMENT);
    ScheduleRef schedule;
    if (CsrAux* aux = aux_lookup(A->d_row_ptrs, false)) {
        std::lock_guard<std::mutex> guard(aux->sptrsv_lock);
        if (matches(aux->sptrsv[uplo], A, uplo)) schedule = aux->sptrsv[uplo];
    }
    if (!schedule) return code(SpMVError::INVALID_ARGUMENT);
    // (a cached schedule is complete: its build waited for the stream)
    if ((level_ptr && hipMemcpy(level_ptr, schedule->d_level_ptr,
                                (static_cast<size_t>(schedule->num_levels) + 1) * sizeof(int),
                                hipMemcpyDeviceToHost) != hipSuccess) ||
        (order && hipMemcpy(order, schedule->d_order, static_cast<size_t>(schedule->num_rows) * sizeof(int),
                            hipMemcpyDeviceToHost) != hipSuccess)) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MEMCPY);
    }
    if (info) {
        copy_counts(*schedule, info);
        info->first_missing_diagonal = schedule->first_missing_diagonal;
        info->first_unsorted_row = schedule->first_unsorted_row;
        info->one_sided_row = schedule->one_sided_row;
        info->built_on_device = schedule->built_on_device ? 1 : 0;
        info->triangle_nnz = schedule->triangle_nnz;
    }
    return code(SpMVError::SUCCESS);
}

} // namespace spmv
