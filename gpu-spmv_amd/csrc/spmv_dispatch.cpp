// spmv_dispatch.cpp — host entry points spmv_csr / spmv_ell: validation,
// kernel choice, device-event timing, metric fill-in.
//
// Follows the reference's dispatcher contract (src/spmv_kernels.cu:215-326 for
// CSR, :328-420 for ELL): argument checks in the same order with the same
// error codes, nullptr config => {SCALAR_CSR, 256, false}, ELL_KERNEL passed to
// spmv_csr behaves as SCALAR_CSR, elapsed_ms is kernel-only event time, the
// call returns after the kernel completed, result.y aliases d_y.
// Documented deviations:
//   * a matrix with zero rows is a successful no-op (the reference's own
//     EmptyMatrix test expects this; its code returns INVALID_DIMENSION);
//   * nnz == 0 with rows > 0 succeeds and writes y = 0;
//   * the ELL non-padding count behind `gflops` is taken once on the device
//     and cached per matrix instead of an O(rows*K) host scan per call.
#include "internal.h"
#include "tiled.h"
#include "spmv/bandwidth.h"

#include <algorithm>
#include <atomic>
#include <cstdint>
#include <cstdlib>
#include <memory>
#include <mutex>
#include <utility>

namespace spmv {

namespace detail {

namespace {
thread_local hipStream_t g_stream = nullptr;
std::atomic<int> g_promote_after{-1};      // -1: not read from the environment yet
}

int tiled_promotion() {
    int v = g_promote_after.load(std::memory_order_relaxed);
    if (v < 0) {
        const char* env = std::getenv("SPMV_TILED_PROMOTE");
        v = env ? std::max(0, std::atoi(env)) : 4;
        if (env && env[0] == '1' && env[1] == '\0') v = 4;       // "1" = on, at the default threshold
        g_promote_after.store(v, std::memory_order_relaxed);
    }
    return v;
}

void set_tiled_promotion(int calls) { g_promote_after.store(std::max(0, calls), std::memory_order_relaxed); }

hipStream_t current_stream() { return g_stream; }

EventPair& thread_events() {
    thread_local EventPair pair;
    if (!pair.start) {
        if (hipEventCreate(&pair.start) != hipSuccess) pair.start = nullptr;
        if (hipEventCreate(&pair.stop) != hipSuccess) pair.stop = nullptr;
    }
    return pair;
}

namespace {

bool block_size_ok(const SpMVConfig* config) {
    return config->block_size > 0 && config->block_size <= 1024;
}

// shared front half of the sync and async CSR paths; returns SUCCESS when a launch should follow
int check_csr(const CSRMatrix* A, const float* d_x, float* d_y, int vec_size, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_x || !d_y) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return code(SpMVError::SUCCESS);
    }
    if (vec_size >= 0 && !spmv_validate_dimensions(A->num_cols, vec_size)) {
        return code(SpMVError::INVALID_DIMENSION);
    }
    // (not device_arrays_strict: no sign check, a negative num_rows passes as in the reference)
    if (!A->d_row_ptrs || (A->nnz > 0 && (!A->d_col_indices || !A->d_values))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    return code(SpMVError::SUCCESS);
}

hipError_t enqueue_csr(const CSRMatrix* A, const float* d_x, float* d_y,
                       const SpMVConfig* config, hipStream_t stream) {
    if (A->nnz == 0) return launch_fill_zero(d_y, A->num_rows, stream);

    // use_texture = "keep x on chip": on gfx950 that is the LDS-tiled engine (tiled.hip).
    // It replaces the row-parallel kernels that reorder sums anyway; SCALAR_CSR keeps its
    // CPU-order contract and never takes this route.
    // Without use_texture the same two kernels take it once the matrix HOLDS a plan (promotion, below; an enqueue
    // never builds one for them: the async entry points may be inside a graph capture).
    if (config->kernel_type == SpMVConfig::VECTOR_CSR || config->kernel_type == SpMVConfig::MERGE_PATH) {
        const PlanRef plan = config->use_texture ? tiled_plan_for(A, stream)
                                                 : (tiled_promotion() > 0 ? tiled_plan_if_cached(A) : PlanRef());
        if (plan) {
            const hipError_t e = tiled_spmv(*plan, d_x, d_y, stream);
            if (e != hipErrorOutOfMemory) return e;     // (no scratch for yet another stream: the direct kernels below)
        }
    }

    switch (config->kernel_type) {
        case SpMVConfig::VECTOR_CSR: {
            const float avg = static_cast<float>(A->nnz) / A->num_rows;
            if (config->use_texture) {          // small x: keep all of it in every CU's LDS
                if (const int grid = vector_ldsx_grid(A)) {
                    return launch_csr_vector_ldsx(A, d_x, d_y, pick_lanes_per_row(avg), grid, stream);
                }
            }
            return launch_csr_vector(A, d_x, d_y, pick_lanes_per_row(avg), stream);
        }
        case SpMVConfig::MERGE_PATH: {
            CsrAux* aux = aux_lookup(A->d_row_ptrs, true);
            return launch_csr_merge(A, aux, d_x, d_y, stream);
        }
        case SpMVConfig::SCALAR_CSR:
        default:
            return launch_csr_scalar(A, d_x, d_y, stream);
    }
}

// builds what enqueue_csr would otherwise build on first use (cached per matrix)
void prepare_csr(const CSRMatrix* A, const SpMVConfig* config, hipStream_t stream) {
    if (A->nnz == 0) return;
    const bool reorders = config->kernel_type == SpMVConfig::VECTOR_CSR || config->kernel_type == SpMVConfig::MERGE_PATH;
    if (config->use_texture && reorders && tiled_plan_for(A, stream)) return;
    // promotion: count the synchronous calls that spell a reordering kernel; past the threshold build the plan here,
    // in front of the timed region, like every other one-time preparation
    if (reorders && !config->use_texture && tiled_promotion() > 0 && tiled_eligible(A)) {
        CsrAux* aux = aux_lookup(A->d_row_ptrs, true);
        if (aux->reorder_calls.fetch_add(1, std::memory_order_relaxed) >= tiled_promotion() && aux->plan_replacements <= 2 &&
            tiled_plan_for(A, stream)) return;
        if (tiled_plan_if_cached(A)) return;
    }
    if (config->kernel_type == SpMVConfig::MERGE_PATH) (void)prepare_csr_merge(A, aux_lookup(A->d_row_ptrs, true), stream);
}

// front half of spmv_csr_multi / spmv_csr_multi_async, checks in the documented order (include/spmv/spmv.h)
int check_csr_multi(const CSRMatrix* A, const float* d_X, int ldx, const float* d_Y, int ldy, int k, int vec_size,
                    bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_X || !d_Y) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return code(SpMVError::SUCCESS);
    }
    if (k < 1) return code(SpMVError::INVALID_ARGUMENT);
    if (vec_size >= 0 && !spmv_validate_dimensions(A->num_cols, vec_size)) {
        return code(SpMVError::INVALID_DIMENSION);
    }
    if (ldx < k || ldy < k) return code(SpMVError::INVALID_DIMENSION);
    // (check_csr's rule: not device_arrays_strict, no sign check)
    if (!A->d_row_ptrs || (A->nnz > 0 && (!A->d_col_indices || !A->d_values))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    // the bytes a call reads from X and writes to Y (padding columns included between rows): disjoint
    const auto span = [k](const float* base, long long rows, long long ld) {
        const uintptr_t lo = reinterpret_cast<uintptr_t>(base);
        const uintptr_t bytes = rows > 0 ? static_cast<uintptr_t>(((rows - 1) * ld + k) * sizeof(float)) : 0;
        return std::make_pair(lo, lo + bytes);
    };
    const auto x = span(d_X, A->num_cols, ldx);
    const auto y = span(d_Y, A->num_rows, ldy);
    if (x.first < x.second && x.first < y.second && y.first < x.second) return code(SpMVError::INVALID_ARGUMENT);
    return code(SpMVError::SUCCESS);
}

// Multi calls never look at the tiled plan or the promotion count: use_texture is ignored here.
hipError_t enqueue_csr_multi(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                             const SpMVConfig* config, hipStream_t stream) {
    if (A->nnz == 0) return launch_csr_multi_zero(A, d_Y, ldy, k, stream);
    switch (config->kernel_type) {
        case SpMVConfig::VECTOR_CSR:
            return launch_csr_multi_vector(A, d_X, ldx, d_Y, ldy, k, stream);
        case SpMVConfig::MERGE_PATH:
            return launch_csr_multi_merge(A, aux_lookup(A->d_row_ptrs, true), d_X, ldx, d_Y, ldy, k, stream);
        case SpMVConfig::SCALAR_CSR:
        default:
            return launch_csr_multi_rows(A, d_X, ldx, d_Y, ldy, k, stream);
    }
}

// front half of spmv_csr_transpose / spmv_csr_transpose_async, checks in the documented order (include/spmv/spmv.h)
int check_csr_transpose(const CSRMatrix* A, const float* d_x, const float* d_y, int vec_size, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_x || !d_y) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_cols == 0) {
        *nothing_to_do = true;
        return code(SpMVError::SUCCESS);
    }
    if (vec_size >= 0 && !spmv_validate_dimensions(A->num_rows, vec_size)) {
        return code(SpMVError::INVALID_DIMENSION);
    }
    // (not device_arrays_lenient: entries without rows pass here and come out as y = 0)
    if (A->num_rows < 0 || A->num_cols < 0 || A->nnz < 0 ||
        (A->num_rows > 0 && (!A->d_row_ptrs || (A->nnz > 0 && (!A->d_col_indices || !A->d_values))))) {
        return code(SpMVError::INVALID_FORMAT);
    }
    return code(SpMVError::SUCCESS);
}

// A's device transpose from A's aux entry: built on the first call and again when A's arrays or shape no longer
// match what it was built from.  Null when there is nothing to transpose (no rows or no entries: y = 0).
int transpose_for(const CSRMatrix* A, hipStream_t stream, std::shared_ptr<CSRMatrix>* out) {
    out->reset();
    if (A->num_rows == 0 || A->nnz == 0) return code(SpMVError::SUCCESS);
    CsrAux* aux = aux_lookup(A->d_row_ptrs, true);
    std::lock_guard<std::mutex> guard(aux->transpose_lock);
    if (aux->transpose && aux->transpose_cols == A->d_col_indices && aux->transpose_vals == A->d_values &&
        aux->transpose_nnz == A->nnz && aux->transpose_rows == A->num_rows && aux->transpose_num_cols == A->num_cols) {
        *out = aux->transpose;
        return code(SpMVError::SUCCESS);
    }
    aux->transpose.reset();
    const TraceRange range("spmv:transpose_build");
    DeviceCsrArrays t;
    const int status = transpose_build(A, &t, stream);
    if (status != 0) return status;
    CSRMatrix* at = new CSRMatrix{};
    at->num_rows = A->num_cols;
    at->num_cols = A->num_rows;
    at->nnz = A->nnz;
    at->d_row_ptrs = t.row_ptrs;
    at->d_col_indices = t.col_indices;
    at->d_values = t.values;
    at->owns_device_memory = true;
    aux->transpose = std::shared_ptr<CSRMatrix>(at, [](CSRMatrix* m) {
        csr_free_gpu(m);        // (drops the transpose's own aux entry: merge partition, tiled plan)
        delete m;
    });
    aux->transpose_cols = A->d_col_indices;
    aux->transpose_vals = A->d_values;
    aux->transpose_nnz = A->nnz;
    aux->transpose_rows = A->num_rows;
    aux->transpose_num_cols = A->num_cols;
    *out = aux->transpose;
    return code(SpMVError::SUCCESS);
}

int check_ell(const ELLMatrix* A, const float* d_x, float* d_y, int vec_size, bool* nothing_to_do) {
    *nothing_to_do = false;
    if (!A || !d_x || !d_y) return code(SpMVError::INVALID_ARGUMENT);
    if (A->num_rows == 0) {
        *nothing_to_do = true;
        return code(SpMVError::SUCCESS);
    }
    if (vec_size >= 0 && !spmv_validate_dimensions(A->num_cols, vec_size)) {
        return code(SpMVError::INVALID_DIMENSION);
    }
    if (A->max_nnz_per_row > 0 && (!A->d_col_indices || !A->d_values)) {
        return code(SpMVError::INVALID_FORMAT);
    }
    return code(SpMVError::SUCCESS);
}

hipError_t enqueue_ell(const ELLMatrix* A, const float* d_x, float* d_y, const SpMVConfig* config,
                       hipStream_t stream) {
    if (A->max_nnz_per_row == 0) return launch_fill_zero(d_y, A->num_rows, stream);
    // use_texture: x through LDS tiles (gives up the default kernel's CPU summation order)
    if (config->use_texture) {
        if (const PlanRef plan = tiled_plan_for(A, stream)) {
            const hipError_t e = tiled_spmv(*plan, d_x, d_y, stream);
            if (e != hipErrorOutOfMemory) return e;
        }
    }
    return launch_ell(A, d_x, d_y, stream);
}

// runs `enqueue` between a cached event pair on `stream` and waits for it
template <typename Enqueue>
int timed(hipStream_t stream, float* elapsed_ms, Enqueue&& enqueue) {
    EventPair& ev = thread_events();
    if (!ev.start || !ev.stop) return code(SpMVError::KERNEL_LAUNCH);
    if (hipEventRecord(ev.start, stream) != hipSuccess) return code(SpMVError::KERNEL_LAUNCH);
    const hipError_t launched = enqueue();
    const hipError_t recorded = hipEventRecord(ev.stop, stream);
    const hipError_t waited = hipEventSynchronize(ev.stop);
    if (launched != hipSuccess || recorded != hipSuccess || waited != hipSuccess ||
        hipGetLastError() != hipSuccess) {
        return code(SpMVError::KERNEL_LAUNCH);
    }
    if (hipEventElapsedTime(elapsed_ms, ev.start, ev.stop) != hipSuccess) {
        return code(SpMVError::KERNEL_LAUNCH);
    }
    return code(SpMVError::SUCCESS);
}

} // namespace
} // namespace detail

void spmv_set_tiled_promotion(int calls) { detail::set_tiled_promotion(calls); }
int spmv_get_tiled_promotion() { return detail::tiled_promotion(); }

void spmv_set_stream(hipStream_t stream) { detail::g_stream = stream; }
hipStream_t spmv_get_stream() { return detail::g_stream; }

SpMVResult spmv_csr(const CSRMatrix* A, const float* d_x, float* d_y,
                    const SpMVConfig* config, int vec_size) {
    SpMVResult result;
    bool nothing = false;
    result.error_code = detail::check_csr(A, d_x, d_y, vec_size, &nothing);
    if (result.error_code != 0) return result;
    if (nothing) {
        result.y = d_y;
        return result;
    }

    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) {
        result.error_code = detail::code(SpMVError::KERNEL_LAUNCH);
        return result;
    }

    const detail::TraceRange range("spmv:spmv_csr");
    hipStream_t stream = detail::current_stream();
    // one-time auxiliary data (the LDS-tiled plan, the merge-path tile table) is built BEFORE the start
    // event: elapsed_ms / gflops / bandwidth_gb_s of the first call then mean what they mean on every later one
    // (the reference's timed region holds the kernel only, src/spmv_kernels.cu:258-262,296-297)
    detail::prepare_csr(A, config, stream);
    result.error_code = detail::timed(stream, &result.elapsed_ms, [&] {
        return detail::enqueue_csr(A, d_x, d_y, config, stream);
    });
    if (result.error_code != 0) return result;

    if (result.elapsed_ms > 0.0f) {
        result.gflops = (2.0f * A->nnz) / (result.elapsed_ms * 1e6f);
    }
    result.bandwidth_gb_s = compute_bandwidth_csr(A, result.elapsed_ms).achieved_bandwidth_gb_s;
    result.y = d_y;
    return result;
}

int spmv_csr_async(const CSRMatrix* A, const float* d_x, float* d_y,
                   const SpMVConfig* config, int vec_size, hipStream_t stream) {
    bool nothing = false;
    const int status = detail::check_csr(A, d_x, d_y, vec_size, &nothing);
    if (status != 0 || nothing) return status;
    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) return detail::code(SpMVError::KERNEL_LAUNCH);
    return detail::enqueue_csr(A, d_x, d_y, config, stream) == hipSuccess
         ? detail::code(SpMVError::SUCCESS) : detail::code(SpMVError::KERNEL_LAUNCH);
}

SpMVResult spmv_csr_multi(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                          const SpMVConfig* config, int vec_size) {
    SpMVResult result;
    bool nothing = false;
    result.error_code = detail::check_csr_multi(A, d_X, ldx, d_Y, ldy, k, vec_size, &nothing);
    if (result.error_code != 0) return result;
    if (nothing) {
        result.y = d_Y;
        return result;
    }

    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) {
        result.error_code = detail::code(SpMVError::KERNEL_LAUNCH);
        return result;
    }

    const detail::TraceRange range("spmv:spmv_csr_multi");
    hipStream_t stream = detail::current_stream();
    // the merge-path partition and this stream's k-wide carry slots, before the start event (as in spmv_csr)
    if (A->nnz > 0 && config->kernel_type == SpMVConfig::MERGE_PATH) {
        (void)detail::prepare_csr_multi_merge(A, detail::aux_lookup(A->d_row_ptrs, true), k, stream);
    }
    result.error_code = detail::timed(stream, &result.elapsed_ms, [&] {
        return detail::enqueue_csr_multi(A, d_X, ldx, d_Y, ldy, k, config, stream);
    });
    if (result.error_code != 0) return result;

    if (result.elapsed_ms > 0.0f) {
        result.gflops = static_cast<float>(2.0 * A->nnz * k / (result.elapsed_ms * 1e6));
    }
    result.bandwidth_gb_s = compute_bandwidth_csr_multi(A, k, result.elapsed_ms).achieved_bandwidth_gb_s;
    result.y = d_Y;
    return result;
}

int spmv_csr_multi_async(const CSRMatrix* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                         const SpMVConfig* config, int vec_size, hipStream_t stream) {
    bool nothing = false;
    const int status = detail::check_csr_multi(A, d_X, ldx, d_Y, ldy, k, vec_size, &nothing);
    if (status != 0 || nothing) return status;
    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) return detail::code(SpMVError::KERNEL_LAUNCH);
    return detail::enqueue_csr_multi(A, d_X, ldx, d_Y, ldy, k, config, stream) == hipSuccess
         ? detail::code(SpMVError::SUCCESS) : detail::code(SpMVError::KERNEL_LAUNCH);
}

SpMVResult spmv_csr_transpose(const CSRMatrix* A, const float* d_x, float* d_y,
                              const SpMVConfig* config, int vec_size) {
    SpMVResult result;
    bool nothing = false;
    result.error_code = detail::check_csr_transpose(A, d_x, d_y, vec_size, &nothing);
    if (result.error_code != 0) return result;
    if (nothing) {
        result.y = d_y;
        return result;
    }

    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) {
        result.error_code = detail::code(SpMVError::KERNEL_LAUNCH);
        return result;
    }

    const detail::TraceRange range("spmv:spmv_csr_transpose");
    hipStream_t stream = detail::current_stream();
    // the transpose and what spmv_csr would prepare for it, before the start event
    std::shared_ptr<CSRMatrix> AT;
    result.error_code = detail::transpose_for(A, stream, &AT);
    if (result.error_code != 0) return result;
    if (AT) detail::prepare_csr(AT.get(), config, stream);
    result.error_code = detail::timed(stream, &result.elapsed_ms, [&] {
        return AT ? detail::enqueue_csr(AT.get(), d_x, d_y, config, stream)
                  : detail::launch_fill_zero(d_y, A->num_cols, stream);
    });
    if (result.error_code != 0) return result;

    if (result.elapsed_ms > 0.0f) {
        result.gflops = (2.0f * A->nnz) / (result.elapsed_ms * 1e6f);
    }
    CSRMatrix shape{};                  // the byte model of spmv_csr on the transpose
    shape.num_rows = A->num_cols;
    shape.num_cols = A->num_rows;
    shape.nnz = A->nnz;
    result.bandwidth_gb_s = compute_bandwidth_csr(&shape, result.elapsed_ms).achieved_bandwidth_gb_s;
    result.y = d_y;
    return result;
}

int spmv_csr_transpose_async(const CSRMatrix* A, const float* d_x, float* d_y,
                             const SpMVConfig* config, int vec_size, hipStream_t stream) {
    bool nothing = false;
    int status = detail::check_csr_transpose(A, d_x, d_y, vec_size, &nothing);
    if (status != 0 || nothing) return status;
    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) return detail::code(SpMVError::KERNEL_LAUNCH);
    std::shared_ptr<CSRMatrix> AT;
    status = detail::transpose_for(A, stream, &AT);
    if (status != 0) return status;
    const hipError_t e = AT ? detail::enqueue_csr(AT.get(), d_x, d_y, config, stream)
                            : detail::launch_fill_zero(d_y, A->num_cols, stream);
    return e == hipSuccess ? detail::code(SpMVError::SUCCESS) : detail::code(SpMVError::KERNEL_LAUNCH);
}

SpMVResult spmv_ell(const ELLMatrix* A, const float* d_x, float* d_y,
                    const SpMVConfig* config, int vec_size) {
    SpMVResult result;
    bool nothing = false;
    result.error_code = detail::check_ell(A, d_x, d_y, vec_size, &nothing);
    if (result.error_code != 0) return result;
    if (nothing) {
        result.y = d_y;
        return result;
    }

    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) {
        result.error_code = detail::code(SpMVError::KERNEL_LAUNCH);
        return result;
    }

    const detail::TraceRange range("spmv:spmv_ell");
    hipStream_t stream = detail::current_stream();
    if (config->use_texture && A->max_nnz_per_row > 0) (void)detail::tiled_plan_for(A, stream);   // outside the timed region
    result.error_code = detail::timed(stream, &result.elapsed_ms, [&] {
        return detail::enqueue_ell(A, d_x, d_y, config, stream);
    });
    if (result.error_code != 0) return result;

    // gflops counts stored entries only (padding excluded), counted once per matrix
    long long stored = 0;
    if (A->d_col_indices) {
        detail::EllAux* aux = detail::ell_aux_lookup(A->d_col_indices, true);
        if (!aux->have_nnz) {
            if (detail::device_count_ell_nnz(A, &aux->actual_nnz, stream) == hipSuccess) {
                aux->have_nnz = true;
            }
        }
        stored = aux->actual_nnz;
    }
    if (result.elapsed_ms > 0.0f) {
        result.gflops = (2.0f * static_cast<float>(stored)) / (result.elapsed_ms * 1e6f);
    }
    result.bandwidth_gb_s = compute_bandwidth_ell(A, result.elapsed_ms).achieved_bandwidth_gb_s;
    result.y = d_y;
    return result;
}

int spmv_ell_async(const ELLMatrix* A, const float* d_x, float* d_y,
                   const SpMVConfig* config, int vec_size, hipStream_t stream) {
    bool nothing = false;
    const int status = detail::check_ell(A, d_x, d_y, vec_size, &nothing);
    if (status != 0 || nothing) return status;
    const SpMVConfig fallback;
    if (!config) config = &fallback;
    if (!detail::block_size_ok(config)) return detail::code(SpMVError::KERNEL_LAUNCH);
    return detail::enqueue_ell(A, d_x, d_y, config, stream) == hipSuccess
         ? detail::code(SpMVError::SUCCESS) : detail::code(SpMVError::KERNEL_LAUNCH);
}

} // namespace spmv
