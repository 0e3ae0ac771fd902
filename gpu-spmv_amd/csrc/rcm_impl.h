// rcm_impl.h — what rcm.hip and rcm_host.cpp share (include/spmv/reorder.h): the limits of the level
// loop and the argument checks that need no device.  Internal: not installed under include/.
#ifndef SPMV_AMD_RCM_IMPL_H
#define SPMV_AMD_RCM_IMPL_H

#include "spmv/reorder.h"

namespace spmv {
namespace detail {
namespace rcm {

// a level of at most kNarrow vertices is numbered inside the one-workgroup run kernel, which takes at most kRunLevels
// levels per launch (that bounds one kernel's time); wider levels take the four grid-wide passes
constexpr int kNarrow = 256;
constexpr int kRunLevels = 512;
constexpr int kRoundsPerBatch = 8;      // rounds enqueued between two looks at the state

// the checks of csr_rcm before any device work; *nothing_to_do: no rows
int rcm_check(const CSRMatrix* A, const int* d_perm, const int* d_inverse, const RcmConfig& cfg, bool* nothing_to_do);
// the checks of csr_band_gpu before any device work
int band_check(const CSRMatrix* A, const CsrBand* out);

} // namespace rcm
} // namespace detail
} // namespace spmv

#endif
