// fsai_impl.h — what fsai.hip (device) and fsai_host.cpp (host twin, argument checks, driver) share: the arithmetic
// rule of include/spmv/fsai.h written once, with every fp64 operation rounded separately on both sides, and the interface
// between the driver and the launches.  Internal: not installed.
#ifndef SPMV_AMD_FSAI_IMPL_H
#define SPMV_AMD_FSAI_IMPL_H

#include "spmv/fsai.h"

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define FSAI_HD __host__ __device__ __forceinline__
#else
#include <hip/hip_runtime_api.h>
#define FSAI_HD inline
#endif

namespace spmv {
namespace detail {
namespace fsai {

// separately rounded fp64 arithmetic: the device intrinsics; on the host std::fma and the plain operators in a
// translation unit compiled with -ffp-contract=off (fsai_host.cpp)
#if defined(__HIP_DEVICE_COMPILE__)
FSAI_HD double fma_rn(double a, double b, double c) { return fma(a, b, c); }
FSAI_HD double div_rn(double a, double b) { return __ddiv_rn(a, b); }
FSAI_HD double sqrt_rn(double a) { return __dsqrt_rn(a); }
#else
FSAI_HD double fma_rn(double a, double b, double c) { return std::fma(a, b, c); }
FSAI_HD double div_rn(double a, double b) { return a / b; }
FSAI_HD double sqrt_rn(double a) { return std::sqrt(a); }
#endif

// position of (p, q), q <= p, in the packed lower triangle (0-based)
FSAI_HD int tri(int p, int q) { return p * (p + 1) / 2 + q; }

// Cholesky, entry (p, q), q <= p, of the packed triangle T that holds M where C is not finished yet: w before the root
// (p == q) or the division (p > q).  Reads rows p and q left of column q only: finished entries of C.
template <class Ptr>
FSAI_HD double cholesky_w(Ptr T, int p, int q) {
    double w = T[tri(p, q)];
    const int rp = tri(p, 0), rq = tri(q, 0);
    for (int k = 0; k < q; ++k) w = fma_rn(-T[rp + k], T[rq + k], w);
    return w;
}

// back substitution: the finished u_p from its accumulator t (u_{m-1}: t is not read), and one accumulation step
FSAI_HD double substitution_u(double t, double cpp, bool last) { return last ? div_rn(1.0, cpp) : div_rn(-t, cpp); }
FSAI_HD double substitution_t(double cqp, double uq, double t) { return fma_rn(cqp, uq, t); }

// the capacity classes of the kernel and the class a longest row of max_row takes (0: too long)
constexpr int kClasses[5] = {4, 8, 16, 32, 64};
inline int class_for(int max_row) {
    for (int c : kClasses) {
        if (max_row <= c) return c;
    }
    return 0;
}
inline bool is_class(long long c) { return c == 4 || c == 8 || c == 16 || c == 32 || c == 64; }

// ---- the device passes (fsai.hip); all enqueue on `s` and return the launch's error ----
// info words of the structure pass
enum Info { kBadFormat = 0, kUnsorted = 1, kNoDiagonal = 2, kMaxRow = 3, kLongRow = 4, kInfoWords = 5 };
// counts[i] = entries of row i of S on or left of the diagonal, counts[n] = 0; the flags of A and S into info
// (kLongRow, an unsigned minimum, preset to all ones, the others to zero)
hipError_t launch_structure_count(const CSRMatrix* A, const CSRMatrix* S, int* counts, unsigned* info, hipStream_t s);
// the columns j <= i of row i of S to g_cols[g_row_ptrs[i] ...]
hipError_t launch_structure_columns(const CSRMatrix* S, const int* g_row_ptrs, int* g_cols, hipStream_t s);
// the values of G on its pattern from A at row_class / lanes, then the scan of G's diagonal into *bad_row (an unsigned
// minimum, preset to all ones)
hipError_t launch_numeric(const CSRMatrix* A, int n, int g_nnz, const int* g_row_ptrs, const int* g_cols,
                          float* g_values, int row_class, int lanes, unsigned* bad_row, hipStream_t s);

} // namespace fsai
} // namespace detail
} // namespace spmv

#endif
