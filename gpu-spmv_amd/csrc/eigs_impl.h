// eigs_impl.h — what eigs.hip (device) and eigs_host.cpp (host twin, argument checks) share: the round-robin pairing
// and the rotation parameters of sym_eig_small's Jacobi rule (include/spmv/eigs.h), written once with every fp64
// operation rounded separately on both sides.  Internal: not installed.
#ifndef SPMV_AMD_EIGS_IMPL_H
#define SPMV_AMD_EIGS_IMPL_H

#include "spmv/eigs.h"

#include <cmath>

#if defined(__HIPCC__)
#include <hip/hip_runtime.h>
#define EIGS_HD __host__ __device__ __forceinline__
#else
#define EIGS_HD inline
#endif

namespace spmv {
namespace detail {
namespace eigs {

constexpr int kMaxOrder = 64;        // sym_eig_small's largest order = the largest basis
constexpr int kMaxValues = 32;
constexpr int kMaxSweeps = 30;

// separately rounded fp64 arithmetic: the device intrinsics; on the host plain operators in a translation unit
// compiled with -ffp-contract=off (eigs_host.cpp)
#if defined(__HIP_DEVICE_COMPILE__)
EIGS_HD double mul_rn(double a, double b) { return __dmul_rn(a, b); }
EIGS_HD double add_rn(double a, double b) { return __dadd_rn(a, b); }
EIGS_HD double div_rn(double a, double b) { return __ddiv_rn(a, b); }
EIGS_HD double sqrt_rn(double a) { return __dsqrt_rn(a); }
#else
EIGS_HD double mul_rn(double a, double b) { return a * b; }
EIGS_HD double add_rn(double a, double b) { return a + b; }
EIGS_HD double div_rn(double a, double b) { return a / b; }
EIGS_HD double sqrt_rn(double a) { return std::sqrt(a); }
#endif

// position i of round r among N (even) players: p < q
EIGS_HD void round_robin_pair(int r, int i, int N, int& p, int& q) {
    int a, b;
    if (i == 0) {
        a = r;
        b = N - 1;
    } else {
        a = (r + i) % (N - 1);
        b = (r - i + (N - 1)) % (N - 1);
    }
    p = a < b ? a : b;
    q = a < b ? b : a;
}

// the rotation that annihilates W[p][q] = apq (apq != 0)
EIGS_HD void rotation(double app, double aqq, double apq, double& c, double& s) {
    const double tau = div_rn(add_rn(aqq, -app), mul_rn(2.0, apq));
    const double root = sqrt_rn(add_rn(1.0, mul_rn(tau, tau)));
    const double t = div_rn(tau < 0.0 ? -1.0 : 1.0, add_rn(fabs(tau), root));
    c = div_rn(1.0, sqrt_rn(add_rn(1.0, mul_rn(t, t))));
    s = mul_rn(t, c);
}

// (x, y) <- (c x - s y, s x + c y)
EIGS_HD void rotate_pair(double c, double s, double& x, double& y) {
    const double nx = add_rn(mul_rn(c, x), -mul_rn(s, y));
    const double ny = add_rn(mul_rn(s, x), mul_rn(c, y));
    x = nx;
    y = ny;
}

// the host twin of the device kernel (eigs_host.cpp): arguments as sym_eig_small, already checked
void sym_eig_small_host(int n, const double* T, int ld, double* values, double* vectors);
// sym_eig_small's argument checks; *nothing_to_do: n == 0
int sym_eig_small_check(int n, const double* T, int ld, const double* values, const double* vectors,
                        bool* nothing_to_do);
// eigs_sym's argument checks in the header's order (no pointer into device memory is dereferenced); *m: the basis
// that is used; *nothing_to_do: num_rows == 0
int eigs_check_arguments(const CSRMatrix* A, const float* d_values, const float* d_vectors, long long ldv,
                         const float* d_residuals, const float* d_v0, const EigsConfig& cfg, int* m,
                         bool* nothing_to_do);

} // namespace eigs
} // namespace detail
} // namespace spmv

#endif
