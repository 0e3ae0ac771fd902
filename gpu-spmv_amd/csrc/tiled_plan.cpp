// tiled_plan.cpp — which matrices the LDS-tiled engine takes and the plan shape (strip columns W, tile rows R) it
// gives them: pure host logic (tiled.hip describes the engine, tiled_build.hip builds the plan of this shape).
#include "tiled.h"
#include "tiled_layout.h"

#include <cstdlib>

namespace spmv {
namespace detail {

namespace {

constexpr long long kTargetRun = 128;        // wanted mean entries per cell (run length seen by phase 2)

} // namespace

// W / R for a matrix: as many row tiles as it takes to fill the chip several times over
// (phase 2 parallelism), strips wide enough that a cell's run averages >= ~128 entries
// (phase 2 reads one run per cell); when even the widest strip cannot give that (wide
// shards of a row-partitioned matrix), trade tiles for run length.
void choose_shape(long long num_rows, long long num_cols, long long nnz, int* strip_cols, int* tile_rows) {
    auto tiles_for = [&](int r) { return (num_rows + r - 1) / r; };
    auto strips_for = [&](int w) { return (num_cols + w - 1) / w; };
    int r = 8192;
    while (r > 1024 && tiles_for(r) < 1024) r >>= 1;
    int w = 4096;
    for (;;) {
        w = 4096;
        while (w < 32768 && nnz / (strips_for(w) * tiles_for(r)) < kTargetRun) w <<= 1;
        const bool long_enough = nnz / (strips_for(w) * tiles_for(r)) >= kTargetRun;
        // taller tiles lengthen the runs but cost phase-2 parallelism: keep >= ~600 tiles
        // (measured on a 1.25 M x 10 M shard: 611 tiles / 107-entry runs 88 us, 306 / 213 105 us)
        if (long_enough || r >= 8192 || tiles_for(2 * r) < 600) break;
        r <<= 1;
    }
    // Phase 2 keeps kResidentTiles workgroups on the chip at once (4 per CU while a tile is <= ~39 KiB);
    // tiles all cost the same, so a count just above a multiple of that leaves the chip nearly idle
    // for a whole extra round (C5 at R = 8192: 1221 tiles = 1.19 rounds).  Stretch the tiles so they
    // fill whole rounds (R need not be a power of two), or shrink them if stretching would not fit.
    {
        const long long tiles = tiles_for(r);
        const long long rounds = tiles / kResidentTiles;
        if (rounds >= 1 && tiles % kResidentTiles != 0) {
            auto snapped = [&](long long rounds_wanted) {
                const long long per_tile = (num_rows + rounds_wanted * kResidentTiles - 1) / (rounds_wanted * kResidentTiles);
                return static_cast<int>((per_tile + 63) / 64 * 64);
            };
            int stretched = snapped(rounds);
            r = stretched <= kMaxTileRows ? stretched : snapped(rounds + 1);
        }
    }
    // The strip width was chosen for the tile count before the snap; the snap usually halves the tiles (doubles
    // the runs), so a narrower strip may do now — half the LDS per phase-1 workgroup, twice the wavefronts per CU.
    // Narrow only while the runs stay comfortably long: C4 (1 M power-law rows) 16384 -> 8192 columns, runs
    // 361 -> 182: 44.0 -> 41.9 us; C5 at 8192 would have 128-slot runs: 503 -> 547 us (profiles/r02_shape_sweep.txt,
    // r02_c4_sweep.txt), hence the margin over kTargetRun.
    {
        constexpr long long kComfortableRun = 160;
        int narrower = 4096;
        while (narrower < w && nnz / (strips_for(narrower) * tiles_for(r)) < kComfortableRun) narrower <<= 1;
        w = narrower;
    }
    {   // SPMV_DEBUG=strip=W,tile=R: shape overrides for experiments and boundary-case tests
        const long long v = debug_number("strip", 0);
        if (v == 4096 || v == 8192 || v == 16384 || v == 32768) w = static_cast<int>(v);
        const long long t = debug_number("tile", 0);
        if (t >= 64 && t <= kMaxTileRows && t % 64 == 0) r = static_cast<int>(t);
    }
    *strip_cols = w;
    *tile_rows = r;
}

static bool eligible_dims(long long rows, long long cols, long long nnz) {
    static const bool enabled = [] {
        const char* env = std::getenv("SPMV_TILED");
        return !(env && env[0] == '0');
    }();
    // Everything wider than what one CU's LDS holds of x (<= 32768 columns: the x-in-LDS vector kernel).  Rounds 1-3 drew the line
    // at 65536 columns (a tie then: 69 vs 71 us on 1 M rows x 16); with round 4's engine it wins from the first column past the
    // LDS kernel's reach — 34000 columns: 43.7 against 65.5 us (1 M x 16), 92 against 150 us (4 M x 8); tools/crossover_probe.py,
    // profiles/r04_crossover.txt.  (SPMV_DEBUG=min_cols=1,min_nnz=1: tests force small matrices through the engine)
    const long long min_cols = debug_number("min_cols", 32769LL);
    const long long min_nnz = debug_number("min_nnz", 1LL << 20);
    if (!enabled || rows <= 0 || nnz < min_nnz || cols < min_cols) return false;
    int w = 0, r = 0;
    choose_shape(rows, cols, nnz, &w, &r);
    const long long strips = (cols + w - 1) / w;
    return strips <= kMaxBuildStrips && strips * ((rows + r - 1) / r) <= kMaxCells;
}

bool tiled_shape_for(long long rows, long long cols, long long nnz, int* strip_cols, int* tile_rows) {
    int w = 0, r = 0;
    if (rows > 0 && cols > 0 && nnz > 0) choose_shape(rows, cols, nnz, &w, &r);
    if (strip_cols) *strip_cols = w;
    if (tile_rows) *tile_rows = r;
    return eligible_dims(rows, cols, nnz);
}

bool tiled_eligible(const CSRMatrix* A) {
    return A && eligible_dims(A->num_rows, A->num_cols, A->nnz);
}

bool tiled_eligible(const ELLMatrix* A) {
    return A && eligible_dims(A->num_rows, A->num_cols, static_cast<long long>(A->num_rows) * A->max_nnz_per_row);
}

} // namespace detail
} // namespace spmv
