// assemble_impl.h — what assemble.hip and assemble_host.cpp share (include/spmv/assemble.h): the
// plan, the key layout and the argument checks that need no device.  Internal: not installed under include/.
#ifndef SPMV_AMD_ASSEMBLE_IMPL_H
#define SPMV_AMD_ASSEMBLE_IMPL_H

#include "spmv/assemble.h"

namespace spmv {

struct CooPlan {
    int  num_rows = 0, num_cols = 0;
    int  n = 0;                  // triplets
    int  nnz_out = 0;            // entries of the assembled matrix
    int  duplicates = COO_SUM;
    int* d_order = nullptr;      // [n] source position of every sorted slot
    int* d_segments = nullptr;   // [nnz_out + 1] first sorted slot of every entry; COO_SUM only
};

namespace detail {
namespace assemble {

// the sort's geometry: 4 wavefronts rank 16 rounds of 64 consecutive entries each
constexpr int kSortThreads = 256;
constexpr int kSortRounds = 16;
constexpr int kTileEntries = kSortThreads * kSortRounds;

// bits needed to write every value of [0, extent): 0 for an extent of 0 or 1
inline int index_bits(int extent) {
    int bits = 0;
    while (bits < 31 && (1LL << bits) < extent) ++bits;
    return bits;
}

// key = (row << col_bits) | col
struct KeyLayout {
    int col_bits;
    int total_bits;              // at most 62
    bool narrow() const { return total_bits <= 32; }
};
inline KeyLayout key_layout(int num_rows, int num_cols) {
    const int col_bits = index_bits(num_cols);
    return KeyLayout{col_bits, col_bits + index_bits(num_rows)};
}

// checks 1-3 of csr_from_coo_gpu and csr_from_coo_cpu (everything before the indices are read)
int build_check(const CSRMatrix* C, int num_rows, int num_cols, int n, const int* rows, const int* cols,
                const float* vals, const CooConfig& cfg);
// every check of csr_coo_refill
int refill_check(const CooPlan* plan, const CSRMatrix* C, const float* d_vals);
// the checks of csr_row_indices_gpu before the device pass; *nothing_to_do: no entries
int row_indices_check(const CSRMatrix* A, const int* d_rows, bool* nothing_to_do);

} // namespace assemble
} // namespace detail
} // namespace spmv

#endif
