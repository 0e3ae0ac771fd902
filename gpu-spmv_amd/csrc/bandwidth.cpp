// bandwidth.cpp — algorithmic-byte model and peak-bandwidth lookup.
//
// Byte counts as reference src/bandwidth.cpp:34-42 (CSR) and :66-75 (ELL).
// get_gpu_peak_bandwidth replaces the reference's clock*bus*2 DDR formula
// (:7-20, wrong for HBM) with a per-architecture table.
#include "internal.h"
#include "spmv/bandwidth.h"

#include <algorithm>
#include <cstring>

namespace spmv {

float get_gpu_peak_bandwidth() {
    static const float cached = [] {
        int dev = 0;
        hipDeviceProp_t prop;
        if (hipGetDevice(&dev) != hipSuccess ||
            hipGetDeviceProperties(&prop, dev) != hipSuccess) {
            return 8000.0f;   // no device visible: quote the build target (MI355X)
        }
        // spec HBM peaks, GB/s
        static const struct { const char* arch; float gbs; } table[] = {
            {"gfx950", 8000.0f},   // MI350X / MI355X, HBM3E
            {"gfx942", 5300.0f},   // MI300X
            {"gfx90a", 3276.8f},   // MI250X (both dies)
        };
        for (const auto& e : table) {
            if (std::strncmp(prop.gcnArchName, e.arch, std::strlen(e.arch)) == 0) return e.gbs;
        }
        // unknown part: HBM is double data rate on a wide bus
        const double gbs = 2.0 * prop.memoryClockRate * 1e3 * (prop.memoryBusWidth / 8.0) / 1e9;
        return static_cast<float>(std::min(std::max(gbs, 1.0), 9999.0));
    }();
    return cached;
}

namespace {

BandwidthMetrics from_bytes(double bytes, float elapsed_ms) {
    BandwidthMetrics m;
    m.achieved_bandwidth_gb_s = static_cast<float>(bytes / 1e9 / (elapsed_ms / 1e3));
    m.theoretical_bandwidth_gb_s = get_gpu_peak_bandwidth();
    if (m.theoretical_bandwidth_gb_s > 0.0f) {
        m.efficiency = std::min(m.achieved_bandwidth_gb_s / m.theoretical_bandwidth_gb_s, 1.0f);
    }
    return m;
}

} // namespace

BandwidthMetrics compute_bandwidth_csr(const CSRMatrix* A, float elapsed_ms) {
    if (!A || elapsed_ms <= 0.0f) return BandwidthMetrics();
    const double nnz = A->nnz, rows = A->num_rows, cols = A->num_cols;
    const double bytes = nnz * (sizeof(float) + sizeof(int))   // values + col_indices
                       + (rows + 1) * sizeof(int)              // row_ptrs
                       + cols * sizeof(float)                  // x, counted once
                       + rows * sizeof(float);                 // y
    return from_bytes(bytes, elapsed_ms);
}

BandwidthMetrics compute_bandwidth_csr_multi(const CSRMatrix* A, int k, float elapsed_ms) {
    if (!A || k < 1 || elapsed_ms <= 0.0f) return BandwidthMetrics();
    const double nnz = A->nnz, rows = A->num_rows, cols = A->num_cols;
    const double bytes = nnz * (sizeof(float) + sizeof(int))   // values + col_indices, read once for all k
                       + (rows + 1) * sizeof(int)              // row_ptrs
                       + k * cols * sizeof(float)              // X, counted once
                       + k * rows * sizeof(float);             // Y
    return from_bytes(bytes, elapsed_ms);
}

BandwidthMetrics compute_bandwidth_ell(const ELLMatrix* A, float elapsed_ms) {
    if (!A || elapsed_ms <= 0.0f) return BandwidthMetrics();
    const double slots = static_cast<double>(A->num_rows) * A->max_nnz_per_row;
    const double bytes = slots * (sizeof(float) + sizeof(int))
                       + static_cast<double>(A->num_cols) * sizeof(float)
                       + static_cast<double>(A->num_rows) * sizeof(float);
    return from_bytes(bytes, elapsed_ms);
}

BandwidthMetrics compute_bandwidth_bsr(const BSRMatrix* A, float elapsed_ms) {
    if (!A || elapsed_ms <= 0.0f) return BandwidthMetrics();
    const double b = A->block_dim;
    const double bytes = static_cast<double>(A->num_blocks) * (b * b * sizeof(float) + sizeof(int))   // blocks + block_cols
                       + (static_cast<double>(A->num_block_rows) + 1) * sizeof(int)                    // block_row_ptrs
                       + static_cast<double>(A->num_cols) * sizeof(float)                              // x, counted once
                       + static_cast<double>(A->num_rows) * sizeof(float);                             // y
    return from_bytes(bytes, elapsed_ms);
}

} // namespace spmv
