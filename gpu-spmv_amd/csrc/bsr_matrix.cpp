// bsr_matrix.cpp — BSR container (include/spmv/bsr_matrix.h): host construction, HBM upload and
// download, the non-owning device header, and the hand-over of the builders (bsr_impl.h), all with csr_matrix.cpp's
// ownership rules.
#include "bsr_impl.h"
#include "internal.h"

#include <algorithm>

namespace spmv {

namespace {

using detail::code;

size_t value_count(const BSRMatrix* m) {
    return static_cast<size_t>(m->num_blocks) * m->block_dim * m->block_dim;
}

void release_host(BSRMatrix* m) {
    if (m->owns_host_memory) {
        delete[] m->values;
        delete[] m->block_cols;
        delete[] m->block_row_ptrs;
    }
    m->values = nullptr;
    m->block_cols = nullptr;
    m->block_row_ptrs = nullptr;
}

void set_shape(BSRMatrix* m, int rows, int cols, int block_dim, int num_blocks) {
    m->num_rows = rows;
    m->num_cols = cols;
    m->block_dim = block_dim;
    m->num_block_rows = detail::bsr::blocks_along(rows, block_dim);
    m->num_block_cols = detail::bsr::blocks_along(cols, block_dim);
    m->num_blocks = num_blocks;
}

// (re)allocates uninitialised host arrays for the given shape
void adopt_shape(BSRMatrix* m, int rows, int cols, int block_dim, int num_blocks) {
    release_host(m);
    set_shape(m, rows, cols, block_dim, num_blocks);
    m->values = num_blocks > 0 ? new float[value_count(m)] : nullptr;
    m->block_cols = num_blocks > 0 ? new int[num_blocks] : nullptr;
    m->block_row_ptrs = new int[static_cast<size_t>(m->num_block_rows) + 1];
    m->owns_host_memory = true;
}

} // namespace

BSRMatrix* bsr_create(int rows, int cols, int block_dim, int num_blocks) {
    if (rows < 0 || cols < 0 || num_blocks < 0 || !bsr_block_dim_supported(block_dim)) return nullptr;
    BSRMatrix* m = new BSRMatrix{};
    m->owns_host_memory = true;   // so adopt_shape's release is a no-op on null arrays
    adopt_shape(m, rows, cols, block_dim, num_blocks);
    if (num_blocks > 0) {
        std::fill_n(m->values, value_count(m), 0.0f);
        std::fill_n(m->block_cols, num_blocks, 0);
    }
    std::fill_n(m->block_row_ptrs, static_cast<size_t>(m->num_block_rows) + 1, 0);
    m->owns_device_memory = false;
    return m;
}

void bsr_destroy(BSRMatrix* mat) {
    if (!mat) return;
    release_host(mat);
    if (mat->owns_device_memory) {
        bsr_free_gpu(mat);
    } else if (mat->d_block_row_ptrs) {
        detail::aux_drop(mat->d_block_row_ptrs);   // wrapped device arrays: drop only our side table
    }
    delete mat;
}

int bsr_to_gpu(BSRMatrix* mat) {
    if (!mat) return code(SpMVError::INVALID_ARGUMENT);
    bsr_free_gpu(mat);
    mat->owns_device_memory = true;   // set first so a partial failure is still freed

    struct Upload { void** dst; const void* src; size_t bytes; };
    const Upload plan[] = {
        {reinterpret_cast<void**>(&mat->d_values),         mat->values,         value_count(mat) * sizeof(float)},
        {reinterpret_cast<void**>(&mat->d_block_cols),     mat->block_cols,     static_cast<size_t>(mat->num_blocks) * sizeof(int)},
        {reinterpret_cast<void**>(&mat->d_block_row_ptrs), mat->block_row_ptrs,
         (static_cast<size_t>(mat->num_block_rows) + 1) * sizeof(int)},
    };
    for (const Upload& u : plan) {
        if (u.bytes == 0) continue;
        if (!u.src) {
            bsr_free_gpu(mat);
            return code(SpMVError::INVALID_ARGUMENT);
        }
        if (hipMalloc(u.dst, u.bytes) != hipSuccess) {
            bsr_free_gpu(mat);
            return detail::fail(SpMVError::CUDA_MALLOC);
        }
        if (hipMemcpy(*u.dst, u.src, u.bytes, hipMemcpyHostToDevice) != hipSuccess) {
            bsr_free_gpu(mat);
            return detail::fail(SpMVError::CUDA_MEMCPY);
        }
    }
    return code(SpMVError::SUCCESS);
}

int bsr_from_gpu(BSRMatrix* mat) {
    if (!mat || !mat->d_block_row_ptrs || !mat->block_row_ptrs) return code(SpMVError::INVALID_ARGUMENT);
    if (mat->num_blocks > 0 && mat->d_values && mat->d_block_cols && mat->values && mat->block_cols) {
        SPMV_HIP_CHECK_AS(hipMemcpy(mat->values, mat->d_values, value_count(mat) * sizeof(float), hipMemcpyDeviceToHost),
                          SpMVError::CUDA_MEMCPY);
        SPMV_HIP_CHECK_AS(hipMemcpy(mat->block_cols, mat->d_block_cols, static_cast<size_t>(mat->num_blocks) * sizeof(int),
                                    hipMemcpyDeviceToHost), SpMVError::CUDA_MEMCPY);
    }
    SPMV_HIP_CHECK_AS(hipMemcpy(mat->block_row_ptrs, mat->d_block_row_ptrs,
                                (static_cast<size_t>(mat->num_block_rows) + 1) * sizeof(int), hipMemcpyDeviceToHost),
                      SpMVError::CUDA_MEMCPY);
    return code(SpMVError::SUCCESS);
}

void bsr_free_gpu(BSRMatrix* mat) {
    if (!mat) return;
    if (mat->d_block_row_ptrs) detail::aux_drop(mat->d_block_row_ptrs);      // the schedules of the block pattern
    if (mat->owns_device_memory) {
        if (mat->d_values)         (void)hipFree(mat->d_values);
        if (mat->d_block_cols)     (void)hipFree(mat->d_block_cols);
        if (mat->d_block_row_ptrs) (void)hipFree(mat->d_block_row_ptrs);
    }
    mat->d_values = nullptr;
    mat->d_block_cols = nullptr;
    mat->d_block_row_ptrs = nullptr;
    mat->owns_device_memory = false;
}

BSRMatrix* bsr_wrap_device(int rows, int cols, int block_dim, int num_blocks, const int* d_block_row_ptrs,
                           const int* d_block_cols, const float* d_values) {
    if (rows < 0 || cols < 0 || num_blocks < 0 || !bsr_block_dim_supported(block_dim)) return nullptr;
    BSRMatrix* m = new BSRMatrix{};
    set_shape(m, rows, cols, block_dim, num_blocks);
    m->d_block_row_ptrs = const_cast<int*>(d_block_row_ptrs);
    m->d_block_cols = const_cast<int*>(d_block_cols);
    m->d_values = const_cast<float*>(d_values);
    return m;
}

void bsr_invalidate_gpu_cache(const BSRMatrix* mat) {
    if (mat && mat->d_block_row_ptrs) detail::aux_drop(mat->d_block_row_ptrs);
}

// ---- the hand-over of the builders (bsr_impl.h) ----
void detail::bsr::adopt_device(BSRMatrix* B, int rows, int cols, int block_dim, int num_blocks, int* d_block_row_ptrs,
                               int* d_block_cols, float* d_values) {
    bsr_free_gpu(B);
    adopt_shape(B, rows, cols, block_dim, num_blocks);
    B->d_block_row_ptrs = d_block_row_ptrs;
    B->d_block_cols = d_block_cols;
    B->d_values = d_values;
    B->owns_device_memory = true;
}

void detail::bsr::adopt_host(BSRMatrix* B, int rows, int cols, int block_dim, const std::vector<int>& block_row_ptrs,
                             const std::vector<int>& block_cols, const std::vector<float>& values) {
    const int num_blocks = static_cast<int>(block_cols.size());
    std::unique_ptr<float[]> new_vals(num_blocks > 0 ? new float[values.size()] : nullptr);
    std::unique_ptr<int[]> new_cols(num_blocks > 0 ? new int[block_cols.size()] : nullptr);
    std::unique_ptr<int[]> new_ptrs(new int[block_row_ptrs.size()]);
    std::copy(values.begin(), values.end(), new_vals.get());
    std::copy(block_cols.begin(), block_cols.end(), new_cols.get());
    std::copy(block_row_ptrs.begin(), block_row_ptrs.end(), new_ptrs.get());
    if (B->d_block_row_ptrs || B->d_block_cols || B->d_values) bsr_free_gpu(B);      // a device copy would be stale
    release_host(B);
    set_shape(B, rows, cols, block_dim, num_blocks);
    B->values = new_vals.release();
    B->block_cols = new_cols.release();
    B->block_row_ptrs = new_ptrs.release();
    B->owns_host_memory = true;
}

} // namespace spmv
