// tiled_layout.h — what the two sides of the LDS-tiled engine must agree on: the plan builder (tiled_cells.hip,
// tiled_build.hip, the shape rules of tiled_plan.cpp) writes a layout that the hot path (tiled.hip) walks.
#ifndef SPMV_AMD_TILED_LAYOUT_H
#define SPMV_AMD_TILED_LAYOUT_H

#include <cstddef>
#include <type_traits>

namespace spmv {
namespace detail {

// W (x columns per LDS strip) and R (y rows per LDS tile) are chosen per matrix
// (choose_shape, tiled_plan.cpp):
//   W in {4096, 8192, 16384, 32768} = 16 .. 128 KiB of static LDS in phase 1 (template instantiations)
//   R = any multiple of 64 in [64, kMaxTileRows]: dynamic LDS in phase 2
// Calls f(std::integral_constant<int, W>{}) for a plan's W.
template <class F>
auto with_strip_width(int strip_cols, F&& f) {
    switch (strip_cols) {
        case 4096:  return f(std::integral_constant<int, 4096>{});
        case 8192:  return f(std::integral_constant<int, 8192>{});
        case 16384: return f(std::integral_constant<int, 16384>{});
        default:    return f(std::integral_constant<int, 32768>{});
    }
}

constexpr int kSkip = 255;                  // row-delta byte: advance 255 rows, no entry
constexpr int kLongChunk = 512;       // entries per wavefront of the long-row path
constexpr long long kMaxCells = 1LL << 26;
constexpr long long kResidentTiles = 512;    // phase-2 workgroups resident at once: 256 CUs x 2 (a tile of doubles is <= 78 KiB)
constexpr int kMaxTileRows = 9984;           // 2 tiles of this many doubles (+ the reduction scratch) fit one CU's 160 KiB
constexpr int kMaxBuildStrips = 3072;

// ---- phase 2 as a list of PASSES laid out when the plan is built (round 4) ----
// A tile's slots are one run per strip (cell table); a wavefront of the tile's workgroup owns a contiguous share of the
// strips and walks its runs as ONE stream of slots, 256 per PASS whatever the run boundaries: a pass is up to kPassSegs
// SEGMENTS (the end of one run, whole short runs, the start of the next), 4 slots per lane.  Round 3 derived the segments
// inside the kernel, from the (begin, length) records of the runs — ~100 scalar instructions and ~18 branches per pass,
// and with 8 wavefronts per SIMD sharing one scalar issue slot every 4 cycles that was the kernel's bound: a phase 2 that
// only LOADS (no row rebuild, no LDS adds) took 192 us of the full kernel's 200, whatever the access pattern, the loads in
// flight or the source array (profiles/r04_phase2_bound.txt).  Everything the scalar code computed is a function of the
// plan alone, so it is computed ONCE, by pass_layout_kernel (tiled_cells.hip), into one 32-byte descriptor per pass:
//     base[k]  slot index lane 0 WOULD read if it belonged to segment k (a lane reads base + 4 * lane)
//     adj[k]   row of the slot in front of segment k's first slot (0 at a run's start) minus the sum of the delta bytes
//              of all lanes in front of the segment: row of a slot = adj[segment] + (wave-wide exclusive prefix of the lanes'
//              delta sums) + the in-lane prefix — no carry from pass to pass, nothing read back from the scan
//     geom     first lane of segments 1 and 2, lanes in use
// Beside the descriptors the builder writes the row deltas in PASS ORDER: pass_word[64 * p + l] holds the four delta
// bytes lane l of pass p adds (the word at a_drow + base[segment of l] + 4 l), and 0xFFFFFFFF — four skip markers — on
// the lanes past the pass's end.  A pass's deltas are then one aligned 256-byte block and a wavefront's passes are
// contiguous, where the slot-ordered bytes were one 256-byte piece per run at an arbitrary 4-byte offset whose first and
// last sectors were shared with the neighbouring tile's run and fetched twice whenever the two tiles did not meet in L2;
// the load no longer waits for the segment select, and add() needs no `lane < groups` select for the deltas.  The
// slot-ordered array (TiledPlan::a_drow) lives only while the plan is built.  Cost: the unused tail of every pass that
// is not full — the last pass of a (tile, wavefront), and passes closed by the three-segment limit — is stored as
// markers: for the 10 M x 16 bench plan 637 790 passes x 256 B = 163.27 MB against 161.14 MB of slot-ordered bytes
// (plan_bytes 1 798 181 216 -> 1 800 311 232), while phase 2's reads fell from 895.3 to 888.3 MB per step
// (profiles/aligned_streams_traffic_ab.txt; DESIGN §4.5 has the byte table).
// The hot loop is then: 8 v_readlane per pass, two loads, one wave scan, four ds_add_f64 — and passes are independent of
// each other, so the next ones' loads are always in flight.  Same slots, same rows, same fp64 adds as the round-3 form:
// bit-identical results (tests/tiled_small_shapes_worker.py: ~150 awkward shapes and the hand-picked run-length patterns —
// every boundary case of a pass — against the oracle).
constexpr int kPassSegs = 3;            // segments per pass: 2 / 3 / 4 measured 492 / 482 / 483 us on C5 in round 3
constexpr int kPassSlots = 256;         // slots per pass: four per lane
constexpr int kPassDepth = 3;           // passes in flight per wavefront (2 / 3 / 4: 158.7 / 157.0 / 156.9 us on C5)
constexpr int kReduceThreads = 1024;
constexpr int kReduceWaves = kReduceThreads / 64;

struct PassDesc {                       // 32 bytes = two 16-byte loads
    int base[kPassSegs];
    int adj[kPassSegs];
    unsigned int geom;                  // start[1] | start[2] << 8 | lanes in use << 16
    unsigned int reserved;
};
static_assert(sizeof(PassDesc) == 32, "a lane loads its pass descriptor as two 16-byte words");

// ---- phase 1's walk of a work item ----
// expand_slots starts at the 16-slot boundary at or below the item's first slot (begin & ~15: 16 products = one 64-byte
// sector) and masks the groups in front of `begin` exactly as those behind `end`.  Every full store instruction of a
// wavefront then writes 1 KB of whole sectors.  With the origin at begin & ~3 an instruction's 1 KB started at any
// 16-byte offset, and the non-temporal product stores do not merge partial sectors: a sector split between two
// instructions was written twice (WRITE_SIZE 653.6 -> 650.3 MB for 644.6 MB of products on the bench plan, phase 1
// 311.6 -> 307.8 us; the remaining 5.7 MB are not explained — profiles/aligned_streams_traffic_ab.txt).
// On a plan with packed columns (below) the origin is the 256-slot boundary at or below the first slot (begin & ~255):
// still a whole sector, and a wavefront's 256 slots are then one column block.

// ---- the local columns of a finished plan: 14 bits a slot in 448-byte blocks ----
// A local column is below strip_cols, so on every plan with strip_cols <= kPackedStripCols it has 14 bits, and phase 1
// reads it once per slot and step.  The placing passes, the fold probe and the pass layout work on the u16 array
// (TiledPlan::a_lcol); pack_cols_kernel (tiled_build.hip) then packs it as the last step of the build and the u16 array
// is freed, as a_drow is once pass_word holds its bytes.  The packed array (TiledPlan::a_cols14) is a sequence of BLOCKS
// of kColBlockSlots = 256 slots in kColBlockBytes = 448 bytes, seven whole 64-byte sectors; block b starts at byte 448 b:
//     bytes   0 .. 255   LOW plane: the low 8 bits of slot 256 b + i at byte i
//     bytes 256 .. 447   HIGH field: the high 6 bits of slot 256 b + i at bits 6 i .. 6 i + 5 of these 192 bytes,
//                        little-endian (bit k of the field is bit k % 8 of its byte k / 8)
// A lane of phase 1 owns the four slots q .. q + 3, q a multiple of 4: their low bytes are the aligned dword at byte
// (q & 255) of the block, their high bits the 24 bits that start at byte 256 + 3 ((q & 255) >> 2) — a 4-byte load at
// that (unaligned) address, of which the top byte belongs to the next lane.  A wavefront of phase 1 (64 lanes, 4 slots
// each) walks exactly one block per iteration.  Slots past the plan's last one hold zeros, and the allocation ends
// kColSlackBytes behind the last block, so that the 4-byte load of the last lane's high bits stays inside it.
// strip_cols == 32768 needs 15 bits: those plans keep the u16 array, as does every plan built under
// SPMV_DEBUG=cols=u16 (the A/B switch, and the tests' comparator).
constexpr int kPackedStripCols = 16384;
constexpr int kColBlockSlots = 256;
constexpr int kColBlockBytes = 448;
constexpr int kColLowBytes = 256;
constexpr int kColSlackBytes = 8;
inline long long packed_col_bytes(long long slots) {
    return (slots + kColBlockSlots - 1) / kColBlockSlots * kColBlockBytes + kColSlackBytes;
}

// ---- device side (the host-only tiled_plan.cpp reads the constants above) ----
#ifdef __HIP__
// byte at which the block of slot q starts / one slot's local column, decoded (edge loops, checksum: not the hot path)
__device__ __forceinline__ size_t col_block_byte(long long q) {
    return static_cast<size_t>(q >> 8) * kColBlockBytes;
}
__device__ __forceinline__ int packed_col_at(const unsigned char* __restrict__ cols14, long long k) {
    const unsigned char* block = cols14 + col_block_byte(k);
    const int i = static_cast<int>(k & (kColBlockSlots - 1));
    const int bit = 6 * i, shift = bit & 7;
    unsigned int field = block[kColLowBytes + (bit >> 3)];
    if (shift > 2) field |= static_cast<unsigned int>(block[kColLowBytes + (bit >> 3) + 1]) << 8;
    return static_cast<int>(block[i] | (((field >> shift) & 0x3Fu) << 8));
}
// the same for either form: exactly one of the two pointers is set
__device__ __forceinline__ int lcol_at(const unsigned short* __restrict__ a_lcol, const unsigned char* __restrict__ cols14,
                                       long long k) {
    return cols14 ? packed_col_at(cols14, k) : a_lcol[k];
}

// Workgroups are dealt round-robin over the 8 XCDs (blocks b and b + 8 share one, each XCD has its
// own L2).  Both phases hand every XCD a CONTIGUOUS range of the work list, walked in order:
// neighbours in the list then run on one XCD at about the same time and share what they both
// touch through its L2 — the x strip of consecutive phase-1 items, the 128-byte lines that
// adjacent runs of neighbouring tiles straddle in phase 2.  Returns -1 for the padding blocks of a
// grid rounded up to a multiple of 8.  (Speed only: correctness never depends on placement.
// Measured against the plain order on one box: C2 59.1 -> 55.0 us, C5 535.5 -> 530.1 us, 1/8 shard 84.5 -> 85.2 us.)
constexpr int kXcds = 8;
__device__ __forceinline__ int xcd_contiguous(int block, int count) {
    const int per_xcd = (count + kXcds - 1) / kXcds;
    const int which = (block % kXcds) * per_xcd + block / kXcds;
    return block / kXcds < per_xcd && which < count ? which : -1;
}
__host__ __device__ inline int xcd_grid(int count) { return (count + kXcds - 1) / kXcds * kXcds; }

// the strips (= runs of a tile) wavefront `wave` of a tile's workgroup owns
__device__ __forceinline__ void wave_runs(int num_strips, int wave, int* lo, int* hi) {
    const int per_wave = (num_strips + kReduceWaves - 1) / kReduceWaves;
    *lo = min(num_strips, wave * per_wave);
    *hi = min(num_strips, *lo + per_wave);
}
#endif

} // namespace detail
} // namespace spmv

#endif
