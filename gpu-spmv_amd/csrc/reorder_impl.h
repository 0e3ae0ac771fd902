// reorder_impl.h — what reorder.hip and reorder_host.cpp share (include/spmv/reorder.h): the vertex
// priority, the length classes of csr_permute_gpu and the argument checks that need no device.  Internal: not
// installed under include/.
#ifndef SPMV_AMD_REORDER_IMPL_H
#define SPMV_AMD_REORDER_IMPL_H

#include "spmv/reorder.h"

#include <cstdint>

#if defined(__HIPCC__)
#define SPMV_REORDER_HD __host__ __device__ __forceinline__
#else
#define SPMV_REORDER_HD inline
#endif

namespace spmv {
namespace detail {
namespace reorder {

// the 32-bit finaliser of MurmurHash3: a bijection of the 32-bit integers
SPMV_REORDER_HD unsigned fmix32(unsigned h) {
    h ^= h >> 16;
    h *= 0x85ebca6bu;
    h ^= h >> 13;
    h *= 0xc2b2ae35u;
    h ^= h >> 16;
    return h;
}

// u comes before v in the colouring order: (fmix32(u ^ seed), u) > (fmix32(v ^ seed), v)
SPMV_REORDER_HD bool higher_priority(int u, int v, unsigned seed) {
    const unsigned hu = fmix32(static_cast<unsigned>(u) ^ seed), hv = fmix32(static_cast<unsigned>(v) ^ seed);
    return hu > hv || (hu == hv && u > v);
}

// csr_permute_gpu's row classes by length: a slice of kPermuteSlice lanes, a wavefront, one workgroup with the new
// columns in LDS; a matrix with a longer row takes the relabel-and-transpose-twice route as a whole
constexpr int kPermuteSlice = 8;
constexpr int kPermuteWave = 64;
constexpr int kPermuteLds = 4096;

constexpr int kMaxGatherColumns = 32;

// checks 1-6 of csr_color (everything before the device pass); *nothing_to_do: no rows
int color_check(const CSRMatrix* A, const int* d_colors, const ColorConfig& cfg, bool* nothing_to_do);
// the checks of csr_permute_gpu before the device passes
int permute_check(const CSRMatrix* B, const CSRMatrix* A);
// every check of permute_gather; *nothing_to_do: n == 0
int gather_check(const float* d_out, int ldo, const float* d_in, int ldi, const int* d_index, int n, int k,
                 bool* nothing_to_do);
// the checks of color_ordering before the device pass; *nothing_to_do: n == 0
int ordering_check(int n, const int* d_colors, int num_colors, const int* d_perm, const int* d_inverse,
                   bool* nothing_to_do);

} // namespace reorder
} // namespace detail
} // namespace spmv

#endif
