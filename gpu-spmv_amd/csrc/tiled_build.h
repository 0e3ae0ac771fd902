// tiled_build.h — the seam inside the LDS-tiled engine's plan builder: tiled_build.hip (build_plan: long rows, fold
// probe, phase-1 items) calls tiled_cells.hip (ranking, placing, scans, pass layout) through these.
#ifndef SPMV_AMD_TILED_BUILD_H
#define SPMV_AMD_TILED_BUILD_H

#include "tiled.h"

#include <chrono>
#include <cstdio>
#include <cstdlib>
#include <vector>

namespace spmv {
namespace detail {

// SPMV_TRACE=1: wall-clock time of each host phase of a plan build, on stderr
struct BuildTrace {
    bool on = std::getenv("SPMV_TRACE") != nullptr;
    std::chrono::steady_clock::time_point last = std::chrono::steady_clock::now();
    void mark(const char* phase) {
        if (!on) return;
        const auto now = std::chrono::steady_clock::now();
        std::fprintf(stderr, "[spmv trace] plan build: %-28s %8.3f ms\n", phase,
                     std::chrono::duration<double, std::milli>(now - last).count());
        last = now;
    }
};

// what build_cells leaves behind next to the plan's own arrays
struct BuiltCells {
    DevBuf<int> strip_begin;         // [num_strips + 1] first slot of every strip, on the device (the fold probe reads it)
    std::vector<int> host_strip;     // the same on the host (the phase-1 items are cut from it)
};

// The device passes of the build for a matrix's entries: fills plan->a_val / a_lcol / a_drow / cells_t / pass_first and
// the counts that go with them (plan->long_rows too, from a CSR source: unsorted).  Synchronises the stream.
hipError_t build_cells(const CSRMatrix* A, TiledPlan* plan, BuiltCells* out, hipStream_t s);
hipError_t build_cells(const ELLMatrix* A, TiledPlan* plan, BuiltCells* out, hipStream_t s);   // no long-row path
// plan->pass_desc and plan->pass_word for the finished cells (reads a_drow, which build_plan frees afterwards)
hipError_t layout_passes(TiledPlan* plan, hipStream_t s);

} // namespace detail
} // namespace spmv

#endif
