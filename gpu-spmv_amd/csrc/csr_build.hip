// csr_build.hip — the device half of what the routines that build a CSR matrix share: the output
// arrays and their allocator, the hierarchical exclusive scan, the structure check, the row of every entry, and iota.
// The transpose, SpGEMM, the reordering, the assembly, FSAI, the device AMG setup, the level analysis and the CSR
// algebra call these; the host half (the hand-over to a CSRMatrix) is in csr_matrix.cpp.  No kernel here uses an atomic
// on a value or waits for another workgroup.
#include "internal.h"
#include "device_common.h"

#include <algorithm>
#include <vector>

namespace spmv {
namespace detail {

namespace {

using dev::capped_grid;
using dev::upper_bound;

constexpr int kThreads = 256;                 // 4 wavefronts per workgroup
constexpr int kScanTile = 4096;               // elements per workgroup of the scan

// exclusive scan of data[b*kScanTile ...] in place per workgroup b; sums[b] = the tile's total
__global__ __launch_bounds__(kThreads) void scan_tiles_kernel(int* __restrict__ data, long long n,
                                                              int* __restrict__ sums) {
    constexpr int kPer = kScanTile / kThreads;
    __shared__ int s[kScanTile];
    __shared__ int s_tot[kThreads];
    const long long base = blockIdx.x * static_cast<long long>(kScanTile);
    for (int j = threadIdx.x; j < kScanTile; j += kThreads) s[j] = base + j < n ? data[base + j] : 0;
    __syncthreads();
    int mine = 0;
#pragma unroll
    for (int j = 0; j < kPer; ++j) mine += s[threadIdx.x * kPer + j];
    s_tot[threadIdx.x] = mine;
    __syncthreads();
    for (int off = 1; off < kThreads; off <<= 1) {          // inclusive scan of the thread totals
        const int add = threadIdx.x >= off ? s_tot[threadIdx.x - off] : 0;
        __syncthreads();
        s_tot[threadIdx.x] += add;
        __syncthreads();
    }
    int run = s_tot[threadIdx.x] - mine;
#pragma unroll
    for (int j = 0; j < kPer; ++j) {
        const int v = s[threadIdx.x * kPer + j];
        s[threadIdx.x * kPer + j] = run;
        run += v;
    }
    if (threadIdx.x == kThreads - 1) sums[blockIdx.x] = run;
    __syncthreads();
    for (int j = threadIdx.x; j < kScanTile; j += kThreads) {
        if (base + j < n) data[base + j] = s[j];
    }
}

__global__ __launch_bounds__(kThreads) void scan_add_kernel(int* __restrict__ data, long long n,
                                                            const int* __restrict__ sums) {
    const long long i = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x;
    if (i < n) data[i] += sums[i / kScanTile];
}

// ---- structure: csr_transpose_gpu's rule; every writer stores the same 1 ----
__global__ __launch_bounds__(kThreads) void csr_validate_kernel(const int* __restrict__ rp, const int* __restrict__ ci,
                                                                int rows, int cols, long long nnz,
                                                                int* __restrict__ bad_flag) {
    const long long work = max(nnz, static_cast<long long>(rows) + 1);
    bool bad = false;
    for (long long i = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x; i < work;
         i += static_cast<long long>(gridDim.x) * kThreads) {
        if (i <= rows) {
            const int v = rp[i];
            if (i == 0 && v != 0) bad = true;
            if (i == rows && v != nnz) bad = true;
            if (i < rows && v > rp[i + 1]) bad = true;
        }
        if (i < nnz) {
            const int c = ci[i];
            if (c < 0 || c >= cols) bad = true;
        }
    }
    if (__any(bad) && (threadIdx.x & 63) == 0) *bad_flag = 1;
}

// row_of[p] = the row that holds entry p (row_ptrs validated: rp[0] == 0, non-decreasing, rp[rows] == nnz)
__global__ __launch_bounds__(kThreads) void expand_rows_kernel(const int* __restrict__ rp, int rows, long long nnz,
                                                               int* __restrict__ row_of) {
    __shared__ int s_first, s_last;
    const long long base = blockIdx.x * static_cast<long long>(kThreads);
    if (threadIdx.x == 0) s_first = upper_bound(rp, 0, rows + 1, base) - 1;
    if (threadIdx.x == 1) s_last = upper_bound(rp, 0, rows + 1, std::min(base + kThreads, nnz) - 1) - 1;
    __syncthreads();
    const long long p = base + threadIdx.x;
    if (p < nnz) row_of[p] = upper_bound(rp, s_first + 1, s_last + 2, p) - 1;
}

__global__ __launch_bounds__(kThreads) void iota_kernel(long long n, int* __restrict__ out) {
    for (long long i = blockIdx.x * static_cast<long long>(kThreads) + threadIdx.x; i < n;
         i += static_cast<long long>(gridDim.x) * kThreads) {
        out[i] = static_cast<int>(i);
    }
}

unsigned blocks_for(long long n, long long per) { return static_cast<unsigned>((n + per - 1) / per); }

hipError_t exclusive_scan(int* data, const std::vector<long long>& sizes, size_t level, int* sums, hipStream_t s) {
    const long long n = sizes[level];
    const unsigned tiles = blocks_for(n, kScanTile);
    scan_tiles_kernel<<<tiles, kThreads, 0, s>>>(data, n, sums);
    if (tiles == 1) return hipGetLastError();
    const hipError_t e = exclusive_scan(sums, sizes, level + 1, sums + sizes[level + 1], s);
    if (e != hipSuccess) return e;
    scan_add_kernel<<<blocks_for(n, kThreads), kThreads, 0, s>>>(data, n, sums);
    return hipGetLastError();
}

} // namespace

// ---- the output arrays ----
hipError_t DeviceCsrArrays::alloc(long long row_ptr_count, long long nnz) {
    const hipError_t e = hipMalloc(reinterpret_cast<void**>(&row_ptrs), static_cast<size_t>(row_ptr_count) * sizeof(int));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release();
        return e;
    }
    return alloc_entries(nnz);
}

hipError_t DeviceCsrArrays::alloc_entries(long long nnz) {
    if (nnz <= 0) return hipSuccess;
    hipError_t e = hipMalloc(reinterpret_cast<void**>(&col_indices), static_cast<size_t>(nnz) * sizeof(int));
    if (e == hipSuccess) e = hipMalloc(reinterpret_cast<void**>(&values), static_cast<size_t>(nnz) * sizeof(float));
    if (e != hipSuccess) {
        (void)hipGetLastError();
        release();
    }
    return e;
}

void DeviceCsrArrays::release() {
    if (row_ptrs) (void)hipFree(row_ptrs);
    if (col_indices) (void)hipFree(col_indices);
    if (values) (void)hipFree(values);
    *this = DeviceCsrArrays();
}

// ---- the scan: level sizes n, ceil(n / kScanTile), ... down to one element ----
std::vector<long long> device_scan_levels(long long n) {
    std::vector<long long> sizes{n};
    while (sizes.back() > 1) sizes.push_back((sizes.back() + kScanTile - 1) / kScanTile);
    return sizes;
}

long long device_scan_sums(const std::vector<long long>& levels) {
    long long sums = 1;
    for (size_t l = 1; l < levels.size(); ++l) sums += levels[l];
    return sums;
}

// a tile kernel per level below the top, an add kernel for all but the last of them
int device_scan_launches(const std::vector<long long>& levels) {
    return std::max(1, 2 * static_cast<int>(levels.size()) - 3);
}

hipError_t device_exclusive_scan(int* data, const std::vector<long long>& levels, int* sums, hipStream_t s) {
    return exclusive_scan(data, levels, 0, sums, s);
}

// ---- the structure check ----
hipError_t enqueue_validate(const CSRMatrix* A, int* d_flag, hipStream_t s) {
    const long long work = std::max<long long>(A->nnz, static_cast<long long>(A->num_rows) + 1);
    csr_validate_kernel<<<capped_grid(work, kThreads), kThreads, 0, s>>>(A->d_row_ptrs, A->d_col_indices, A->num_rows,
                                                                         A->num_cols, A->nnz, d_flag);
    return hipGetLastError();
}

int structure_checked(const CSRMatrix* A, hipStream_t s) {
    DevBuf<int> flag;
    if (dev_alloc(&flag, 1) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::CUDA_MALLOC);
    }
    int bad = 0;
    if (hipMemsetAsync(flag.get(), 0, sizeof(int), s) != hipSuccess ||
        enqueue_validate(A, flag.get(), s) != hipSuccess ||
        hipMemcpyAsync(&bad, flag.get(), sizeof(int), hipMemcpyDeviceToHost, s) != hipSuccess ||
        hipStreamSynchronize(s) != hipSuccess) {
        (void)hipGetLastError();
        return code(SpMVError::KERNEL_LAUNCH);
    }
    return bad ? code(SpMVError::INVALID_FORMAT) : 0;
}

// ---- small launchers ----
hipError_t launch_expand_rows(const int* rp, int rows, long long nnz, int* row_of, hipStream_t s) {
    expand_rows_kernel<<<blocks_for(nnz, kThreads), kThreads, 0, s>>>(rp, rows, nnz, row_of);
    return hipGetLastError();
}

hipError_t launch_iota(long long n, int* out, int grid, hipStream_t s) {
    iota_kernel<<<grid, kThreads, 0, s>>>(n, out);
    return hipGetLastError();
}

} // namespace detail
} // namespace spmv
