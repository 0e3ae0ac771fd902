/* spmv_c.h — C-ABI boundary of the MI355X-native SpMV library (libspmv_amd.so).
 *
 * The reference (LessUp/gpu-spmv) is a C++ library: free functions in
 * `namespace spmv` over plain structs (its include/spmv headers).  This header exports
 * the same entry points with C linkage — plain pointers, sizes and POD structs,
 * no C++ or torch types — so any FFI (ctypes, cgo, JNI, N-API) can bind them.
 * Every struct below has the byte layout of the reference's C++ struct of the
 * same name (x86-64 SysV), so a `spmv::CSRMatrix*` and a `spmv_c_csr*` are
 * interchangeable.  Each declaration cites the reference interface it replaces.
 *
 * Functions that return `int` return a spmv error code (0 = success, negative
 * values as reference include/spmv/common.h:13-23).  Results that the C++ API
 * returns by value come back through an `out` pointer.
 * Device pointers (`d_*`) are addresses in the current HIP device's memory.
 */
#ifndef SPMV_C_H
#define SPMV_C_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

/* ---- error codes: reference include/spmv/common.h:13-23 ---- */
enum {
    SPMV_C_SUCCESS = 0,
    SPMV_C_INVALID_DIMENSION = -1,
    SPMV_C_DEVICE_MALLOC = -2,
    SPMV_C_DEVICE_MEMCPY = -3,
    SPMV_C_KERNEL_LAUNCH = -4,
    SPMV_C_INVALID_FORMAT = -5,
    SPMV_C_FILE_IO = -6,
    SPMV_C_OUT_OF_MEMORY = -7,
    SPMV_C_INVALID_ARGUMENT = -8
};
/* reference include/spmv/common.h:26-39 (spmv_error_string) */
const char* spmv_c_error_string(int code);

/* ---- structs ---- */

/* reference include/spmv/csr_matrix.h:11-28 (72 bytes) */
typedef struct spmv_c_csr {
    int32_t num_rows, num_cols, nnz;
    float*   values;
    int32_t* col_indices;
    int32_t* row_ptrs;
    float*   d_values;
    int32_t* d_col_indices;
    int32_t* d_row_ptrs;
    uint8_t  owns_host_memory;
    uint8_t  owns_device_memory;
} spmv_c_csr;

/* reference include/spmv/ell_matrix.h:12-28 (56 bytes) */
typedef struct spmv_c_ell {
    int32_t num_rows, num_cols, max_nnz_per_row;
    float*   values;
    int32_t* col_indices;
    float*   d_values;
    int32_t* d_col_indices;
    uint8_t  owns_host_memory;
    uint8_t  owns_device_memory;
} spmv_c_ell;

/* reference include/spmv/csr_matrix.h:64-69 */
typedef struct spmv_c_csr_stats {
    float   avg_nnz_per_row;
    int32_t max_nnz_per_row;
    int32_t min_nnz_per_row;
    float   skewness;
} spmv_c_csr_stats;

/* reference include/spmv/spmv.h:11-24; kernel_type: 0 SCALAR_CSR, 1 VECTOR_CSR,
 * 2 MERGE_PATH, 3 ELL_KERNEL (12 bytes) */
typedef struct spmv_c_config {
    int32_t kernel_type;
    int32_t block_size;
    uint8_t use_texture;
} spmv_c_config;

/* reference include/spmv/spmv.h:27-36 (24 bytes) */
typedef struct spmv_c_result {
    float*  y;
    float   elapsed_ms;
    float   gflops;
    float   bandwidth_gb_s;
    int32_t error_code;
} spmv_c_result;

/* reference include/spmv/bandwidth.h:10-18 */
typedef struct spmv_c_bandwidth {
    float theoretical_bandwidth_gb_s;
    float achieved_bandwidth_gb_s;
    float efficiency;
} spmv_c_bandwidth;

/* reference include/spmv/pagerank.h:9-15 */
typedef struct spmv_c_pagerank_config {
    float   damping_factor;
    float   tolerance;
    int32_t max_iterations;
} spmv_c_pagerank_config;

/* reference include/spmv/pagerank.h:18-25 (24 bytes) */
typedef struct spmv_c_pagerank_result {
    float*  ranks;
    int32_t iterations;
    float   final_residual;
    uint8_t converged;
} spmv_c_pagerank_result;

/* reference include/spmv/pagerank.h:38-41 */
typedef struct spmv_c_topk_node {
    int32_t node_id;
    float   rank;
} spmv_c_topk_node;

/* ---- library / device ---- */
const char* spmv_c_version(void);
int spmv_c_device_count(void);                       /* 0 when no HIP device is visible */
int spmv_c_device_name(char* buf, size_t buf_len);   /* gcnArchName of the current device */
int spmv_c_set_device(int ordinal);
/* lets kernels of the current device store into memory of `peer_ordinal` (xGMI / PCIe peer access) */
int spmv_c_enable_peer_access(int peer_ordinal);
/* stream used by the synchronous entry points of the calling thread (NULL = null stream) */
void spmv_c_set_stream(void* hip_stream);

/* ---- device buffers: reference include/spmv/cuda_buffer.h:12-101 (CudaBuffer<T>) ---- */
int spmv_c_device_malloc(void** d_ptr, size_t bytes);            /* ctor / resize */
int spmv_c_device_free(void* d_ptr);                             /* dtor / release */
int spmv_c_memcpy_h2d(void* d_dst, const void* src, size_t bytes);   /* copyFromHost */
int spmv_c_memcpy_d2h(void* dst, const void* d_src, size_t bytes);   /* copyToHost */
int spmv_c_device_synchronize(void);
/* extension: share a spmv_c_device_malloc'ed buffer with another process on the same node
 * (hipIpcGetMemHandle / hipIpcOpenMemHandle); handles are 64 opaque bytes.  The opener maps the
 * buffer for ITS current device, so its kernels may load/store it directly (over xGMI when the
 * buffer lives on another GPU). */
int spmv_c_ipc_get_handle(void* d_ptr, unsigned char handle_out[64]);
int spmv_c_ipc_open_handle(const unsigned char handle[64], void** d_ptr_out);
int spmv_c_ipc_close(void* d_ptr);

/* ---- CSR container: reference include/spmv/csr_matrix.h:31-71 ---- */
spmv_c_csr* spmv_c_csr_create(int rows, int cols, int nnz);
void spmv_c_csr_destroy(spmv_c_csr* mat);
int spmv_c_csr_from_dense(spmv_c_csr* csr, const float* dense, int rows, int cols);
int spmv_c_csr_to_dense(const spmv_c_csr* csr, float* dense);
float spmv_c_csr_get_element(const spmv_c_csr* mat, int row, int col);
int spmv_c_csr_to_gpu(spmv_c_csr* mat);
int spmv_c_csr_from_gpu(spmv_c_csr* mat);
void spmv_c_csr_free_gpu(spmv_c_csr* mat);
/* extension: forget the cached auxiliary data after the device arrays were modified in place */
void spmv_c_csr_invalidate_gpu_cache(const spmv_c_csr* mat);
int spmv_c_csr_serialize(const spmv_c_csr* mat, const char* filename);
int spmv_c_csr_deserialize(spmv_c_csr* mat, const char* filename);
int spmv_c_csr_compute_stats(const spmv_c_csr* mat, spmv_c_csr_stats* out);
/* extension: a matrix header over device arrays the caller owns (no host arrays) */
spmv_c_csr* spmv_c_csr_wrap_device(int rows, int cols, int nnz, const int32_t* d_row_ptrs,
                                   const int32_t* d_col_indices, const float* d_values);

/* ---- ELL container: reference include/spmv/ell_matrix.h:31-66 ---- */
spmv_c_ell* spmv_c_ell_create(int rows, int cols, int max_nnz_per_row);
void spmv_c_ell_destroy(spmv_c_ell* mat);
int spmv_c_ell_from_dense(spmv_c_ell* ell, const float* dense, int rows, int cols);
int spmv_c_ell_from_csr(spmv_c_ell* ell, const spmv_c_csr* csr);
/* extension (device-side conversion, no host pass): see ell_from_csr_gpu in spmv/ell_matrix.h */
int spmv_c_ell_from_csr_gpu(spmv_c_ell* ell, const spmv_c_csr* csr);
/* extension (device-side transpose, deterministic): see csr_transpose_gpu in spmv/csr_matrix.h */
int spmv_c_csr_transpose_gpu(spmv_c_csr* AT, const spmv_c_csr* A);
int spmv_c_ell_to_dense(const spmv_c_ell* ell, float* dense);
float spmv_c_ell_get_element(const spmv_c_ell* mat, int row, int col);
int spmv_c_ell_to_gpu(spmv_c_ell* mat);
int spmv_c_ell_from_gpu(spmv_c_ell* mat);
void spmv_c_ell_free_gpu(spmv_c_ell* mat);
void spmv_c_ell_invalidate_gpu_cache(const spmv_c_ell* mat);
int spmv_c_ell_serialize(const spmv_c_ell* mat, const char* filename);
int spmv_c_ell_deserialize(spmv_c_ell* mat, const char* filename);
int spmv_c_ell_index(int row, int k, int num_rows);
spmv_c_ell* spmv_c_ell_wrap_device(int rows, int cols, int max_nnz_per_row,
                                   const int32_t* d_col_indices, const float* d_values);

/* ---- SpMV: reference include/spmv/spmv.h:39-54 ---- */
void spmv_c_cpu_csr(const spmv_c_csr* A, const float* x, float* y);      /* spmv_cpu_csr */
void spmv_c_cpu_ell(const spmv_c_ell* A, const float* x, float* y);      /* spmv_cpu_ell */
/* spmv_csr / spmv_ell: config may be NULL (defaults), vec_size < 0 skips the size check;
 * the return value equals out->error_code */
int spmv_c_spmv_csr(const spmv_c_csr* A, const float* d_x, float* d_y,
                    const spmv_c_config* config, int vec_size, spmv_c_result* out);
int spmv_c_spmv_ell(const spmv_c_ell* A, const float* d_x, float* d_y,
                    const spmv_c_config* config, int vec_size, spmv_c_result* out);
int spmv_c_auto_config(const spmv_c_csr* A, spmv_c_config* out);          /* spmv_auto_config */
int spmv_c_validate_dimensions(int num_cols, int vec_size);               /* 1 = match */
/* extension (spmv::spmv_set_tiled_promotion, include/spmv/spmv.h): after `calls` spmv_csr() calls that name
 * VECTOR_CSR / MERGE_PATH without use_texture on one large matrix, later ones run on the LDS-tiled engine
 * (default 4, 0 = never; the reference's callers never set use_texture: benchmarks/main.cu:52-56) */
void spmv_c_set_tiled_promotion(int calls);
int spmv_c_get_tiled_promotion(void);
/* extension: 1 when the matrix currently holds an LDS-tiled plan (built by the first
 * use_texture call / PageRank on a large matrix), 0 otherwise */
int spmv_c_csr_has_tiled_plan(const spmv_c_csr* A);
/* extension: what the LDS-tiled engine would do with a rows x cols matrix of nnz entries: returns 1
 * when it would take it (use_texture), and the strip width / tile height it would use (host logic) */
int spmv_c_tiled_shape(int64_t rows, int64_t cols, int64_t nnz, int32_t* strip_cols, int32_t* tile_rows);
/* extension: the plan a matrix currently holds — out[8] = strip_cols, tile_rows, num_strips, num_tiles,
 * slots in cells (entries + row-skip markers + padding), long rows, slots per lane per phase-2 load,
 * long-row limit; returns 0 if none */
int spmv_c_csr_tiled_info(const spmv_c_csr* A, int64_t out[8]);
/* extension: what the plan cost — out[4] = build time in ms (host wall clock, allocations included),
 * device bytes held (the local columns counted at two bytes a slot: see spmv_c_csr_tiled_col_bytes), slots in cells,
 * matrix entries in cells; returns 0 if the matrix has no plan */
int spmv_c_csr_tiled_stats(const spmv_c_csr* A, double out[4]);
/* position-weighted checksums of the plan's slot arrays (values, local columns, row deltas) and its cell table:
 * two builds of one matrix give the same four numbers (the layout is a pure function of the matrix).  1 = filled. */
int spmv_c_csr_tiled_checksum(const spmv_c_csr* A, uint64_t out[4]);
/* extension: 1 when the matrix's plan folded its values into one weight per column (every stored
 * entry of a column bit-identical: adjacency / column-stochastic matrices), so that the tiled engine
 * streams no values; 0 otherwise or without a plan.  SPMV_TILED_FOLD=0 at build time disables it. */
int spmv_c_csr_tiled_folded(const spmv_c_csr* A);
/* extension: the number of phase-1 work items of the matrix's plan (every strip's slots cut into equal pieces of
 * at most the item size; SPMV_DEBUG=item=N sets that size); -1 without a plan.  Read-only, for boundary-case tests. */
int spmv_c_csr_tiled_items(const spmv_c_csr* A);
/* extension: the device bytes the matrix's plan holds of local columns: 2 per slot, or, where the plan packed them to
 * 14 bits (strips of at most 16384 columns, unless SPMV_DEBUG=cols=u16), 448 for every 256 slots begun plus 8; -1
 * without a plan.  spmv_c_csr_tiled_stats counts two bytes per slot in its "bytes held" either way, so a packed plan's
 * footprint is that number - 2 * slots + this one. */
int64_t spmv_c_csr_tiled_col_bytes(const spmv_c_csr* A);
/* extension: the plan the LDS-tiled engine built from an ELL matrix's slabs (spmv_ell with use_texture), and the one
 * owned by the cached transpose of A (spmv_csr_transpose with use_texture) — out[10] = the eight numbers of
 * spmv_c_csr_tiled_info, then values folded (0 / 1) and the phase-1 item count; returns 0 if there is none (not
 * eligible, not built yet, or the build failed and the call took the direct kernels).  Read-only. */
int spmv_c_ell_tiled_info(const spmv_c_ell* E, int64_t out[10]);
int spmv_c_csr_transpose_tiled_info(const spmv_c_csr* A, int64_t out[10]);
/* extension: enqueue on a caller stream without timing or synchronisation */
int spmv_c_spmv_csr_async(const spmv_c_csr* A, const float* d_x, float* d_y,
                          const spmv_c_config* config, int vec_size, void* hip_stream);
int spmv_c_spmv_ell_async(const spmv_c_ell* A, const float* d_x, float* d_y,
                          const spmv_c_config* config, int vec_size, void* hip_stream);
/* extension (spmv::spmv_csr_multi, include/spmv/spmv.h): Y = A * X for k right-hand sides in one matrix pass;
 * X is num_cols x k, Y num_rows x k, row-major with leading dimensions ldx, ldy >= k; columns k..ldy-1 of Y are
 * never written.  The return value equals out->error_code (out may be NULL). */
int spmv_c_spmv_csr_multi(const spmv_c_csr* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                          const spmv_c_config* config, int vec_size, spmv_c_result* out);
int spmv_c_spmv_csr_multi_async(const spmv_c_csr* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                                const spmv_c_config* config, int vec_size, void* hip_stream);

/* extension (spmv::spmv_csr_transpose, include/spmv/spmv.h): y = A^T * x; d_x has num_rows entries, d_y num_cols.
 * The first call on a matrix builds and caches its device transpose.  The return value equals out->error_code. */
int spmv_c_spmv_csr_transpose(const spmv_c_csr* A, const float* d_x, float* d_y,
                              const spmv_c_config* config, int vec_size, spmv_c_result* out);
int spmv_c_spmv_csr_transpose_async(const spmv_c_csr* A, const float* d_x, float* d_y,
                                    const spmv_c_config* config, int vec_size, void* hip_stream);

/* ---- preconditioned conjugate gradient (extension; spmv::cg_solve, include/spmv/cg.h) ---- */
/* preconditioner: 0 NONE, 1 JACOBI; engine: -1 auto, 0 direct kernels, 1 tiled plan where eligible (16 bytes) */
typedef struct spmv_c_cg_config {
    float   tolerance;
    int32_t max_iterations;
    int32_t preconditioner;
    int32_t engine;
} spmv_c_cg_config;

/* 24 bytes */
typedef struct spmv_c_cg_result {
    int32_t error_code;
    int32_t iterations;
    float   relative_residual;
    int32_t converged;
    int32_t breakdown;
    float   elapsed_ms;
} spmv_c_cg_result;

/* Solves A x = b for a symmetric positive definite A on the device; d_b and d_x hold num_rows floats, d_x is the
 * initial guess on entry and the solution on exit.  config NULL = defaults (1e-6, 1000, JACOBI, auto).  Argument
 * checks and numerics as cg_solve in include/spmv/cg.h.  The return value equals out->error_code (out may be NULL). */
int spmv_c_cg_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_cg_config* config,
                    spmv_c_cg_result* out);

/* spmv_c_cg_solve for k right-hand sides (1..32) in one matrix pass per step: d_B and d_X are num_rows x k row-major
 * with leading dimensions ldb, ldx >= k; results holds k entries.  Column j is bit for bit spmv_c_cg_solve with
 * engine 0 on that column.  Checks and numerics as cg_solve_multi in include/spmv/cg.h.  Returns the error code. */
int spmv_c_cg_solve_multi(const spmv_c_csr* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                          const spmv_c_cg_config* config, spmv_c_cg_result* results);

/* the same iteration preconditioned by M = L L^T, L the lower triangle (with the stored diagonal) of the square
 * device matrix F and L^T its upper triangle (num_rows as A's; usually spmv_c_ic0_csr's output wrapped over A's
 * structure arrays).  config->preconditioner is not read.  Checks and numerics as cg_solve_ic in include/spmv/cg.h.
 * The return value equals out->error_code (out may be NULL). */
int spmv_c_cg_solve_ic(const spmv_c_csr* A, const spmv_c_csr* F, const float* d_b, float* d_x,
                       const spmv_c_cg_config* config, spmv_c_cg_result* out);

/* the same iteration preconditioned by a factorised sparse approximate inverse M^-1 = GT G: z = GT (G r), two direct
 * vector-CSR SpMVs per step (G usually spmv_c_fsai_csr's output, GT its spmv_c_csr_transpose_gpu).
 * config->preconditioner is not read.  Checks and numerics as cg_solve_fsai in include/spmv/cg.h.  The return value equals out->error_code
 * (out may be NULL). */
int spmv_c_cg_solve_fsai(const spmv_c_csr* A, const spmv_c_csr* G, const spmv_c_csr* GT, const float* d_b, float* d_x,
                         const spmv_c_cg_config* config, spmv_c_cg_result* out);

/* spmv_c_cg_solve_ic for k right-hand sides (1..32) in spmv_c_cg_solve_multi's layout: one matrix pass and one k-wide
 * launch sequence per triangular solve and step.  Column j is bit for bit spmv_c_cg_solve_ic with engine 0 on that
 * column.  Checks and numerics as cg_solve_multi_ic in include/spmv/cg.h.  Returns the error code. */
int spmv_c_cg_solve_multi_ic(const spmv_c_csr* A, const spmv_c_csr* F, const float* d_B, int ldb, float* d_X, int ldx,
                             int k, const spmv_c_cg_config* config, spmv_c_cg_result* results);

/* ---- Jacobi-preconditioned BiCGSTAB (extension; spmv::bicgstab_solve, include/spmv/bicgstab.h) ---- */
/* 16 bytes; the fields, defaults and meanings of spmv_c_cg_config */
typedef struct spmv_c_bicgstab_config {
    float   tolerance;
    int32_t max_iterations;
    int32_t preconditioner;
    int32_t engine;
} spmv_c_bicgstab_config;

/* breakdown: 0 none, 1 RHO (r^.r is 0 or not finite), 2 ALPHA (r^.v is 0 or not finite), 3 OMEGA (omega is 0 or
 * not finite) (24 bytes) */
typedef struct spmv_c_bicgstab_result {
    int32_t error_code;
    int32_t iterations;
    float   relative_residual;
    int32_t converged;
    int32_t breakdown;
    float   elapsed_ms;
} spmv_c_bicgstab_result;

/* Solves A x = b for a square non-singular A on the device; d_b and d_x hold num_rows floats, d_x is the initial
 * guess on entry and the solution on exit.  config NULL = defaults (1e-6, 1000, JACOBI, auto).  Argument checks and
 * numerics as bicgstab_solve in include/spmv/bicgstab.h.  The return value equals out->error_code (out may be NULL). */
int spmv_c_bicgstab_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_bicgstab_config* config,
                          spmv_c_bicgstab_result* out);

/* the same iteration right-preconditioned by M = L U, L the unit lower and U the upper triangle (with the stored
 * diagonal) of the square device matrix LU (num_rows as A's; usually spmv_c_ilu0_csr's output wrapped over A's
 * structure arrays).  config->preconditioner is not read.  Checks and numerics as bicgstab_solve_lu in
 * include/spmv/bicgstab.h.  The return value equals out->error_code (out may be NULL). */
int spmv_c_bicgstab_solve_lu(const spmv_c_csr* A, const spmv_c_csr* LU, const float* d_b, float* d_x,
                             const spmv_c_bicgstab_config* config, spmv_c_bicgstab_result* out);

/* ---- restarted GMRES(m) (extension; spmv::gmres_solve, include/spmv/gmres.h) ---- */
/* 20 bytes; restart in [1, 64]; the other fields as spmv_c_cg_config */
typedef struct spmv_c_gmres_config {
    float   tolerance;
    int32_t max_iterations;
    int32_t restart;
    int32_t preconditioner;
    int32_t engine;
} spmv_c_gmres_config;

/* breakdown: 0 none, 1 SINGULAR (the rotated Hessenberg column is 0), 2 NOT_FINITE; relative_residual and converged
 * come from b - A x recomputed with the returned x (28 bytes) */
typedef struct spmv_c_gmres_result {
    int32_t error_code;
    int32_t iterations;
    int32_t restarts;
    float   relative_residual;
    int32_t converged;
    int32_t breakdown;
    float   elapsed_ms;
} spmv_c_gmres_result;

/* Solves A x = b for a square non-singular A on the device by GMRES(restart); d_b and d_x hold num_rows floats, d_x is
 * the initial guess on entry and the solution on exit.  config NULL = defaults (1e-6, 1000, 30, JACOBI, auto).
 * Argument checks and numerics as gmres_solve in include/spmv/gmres.h.  The return value equals out->error_code (out
 * may be NULL). */
int spmv_c_gmres_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_gmres_config* config,
                       spmv_c_gmres_result* out);

/* the same iteration right-preconditioned by M = L U as spmv_c_bicgstab_solve_lu.  config->preconditioner is not read.
 * Checks and numerics as gmres_solve_lu in include/spmv/gmres.h.  The return value equals out->error_code (out may be
 * NULL). */
int spmv_c_gmres_solve_lu(const spmv_c_csr* A, const spmv_c_csr* LU, const float* d_b, float* d_x,
                          const spmv_c_gmres_config* config, spmv_c_gmres_result* out);

/* ---- MINRES for symmetric indefinite systems (extension; spmv::minres_solve, include/spmv/minres.h) ---- */
/* 20 bytes; solves (A - shift I) x = b; preconditioner 0 NONE / 1 JACOBI (M = |diag(A - shift I)|); the other fields
 * as spmv_c_cg_config */
typedef struct spmv_c_minres_config {
    float   tolerance;
    int32_t max_iterations;
    int32_t preconditioner;
    int32_t engine;
    float   shift;
} spmv_c_minres_config;

/* breakdown: 0 none, 1 PRECONDITIONER (r.M^-1 r < 0), 2 NOT_FINITE, 3 SINGULAR (gamma == 0).  relative_residual is the
 * recurrence's, in the M^-1-norm; true_relative_residual is ||b - (A - shift I) x||_2 / ||b||_2 recomputed from the
 * returned x (28 bytes) */
typedef struct spmv_c_minres_result {
    int32_t error_code;
    int32_t iterations;
    float   relative_residual;
    float   true_relative_residual;
    int32_t converged;
    int32_t breakdown;
    float   elapsed_ms;
} spmv_c_minres_result;

/* Solves (A - shift I) x = b for a square symmetric A, definite or not, on the device by preconditioned MINRES; d_b
 * and d_x hold num_rows floats, d_x is the initial guess on entry and the solution on exit.  config NULL = defaults
 * (1e-6, 1000, JACOBI, auto, 0).  Argument checks and numerics as minres_solve in include/spmv/minres.h.  The return
 * value equals out->error_code (out may be NULL). */
int spmv_c_minres_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_minres_config* config,
                        spmv_c_minres_result* out);

/* the same iteration preconditioned by M = L L^T from the factor matrix F as spmv_c_cg_solve_ic.
 * config->preconditioner is not read.  Checks and numerics as minres_solve_ic in include/spmv/minres.h.  The return
 * value equals out->error_code (out may be NULL). */
int spmv_c_minres_solve_ic(const spmv_c_csr* A, const spmv_c_csr* F, const float* d_b, float* d_x,
                           const spmv_c_minres_config* config, spmv_c_minres_result* out);

/* ---- extreme eigenpairs of a symmetric matrix (extension; spmv::eigs_sym, include/spmv/eigs.h) ---- */
/* 24 bytes; num_values in [1, 32]; which 0 LARGEST / 1 SMALLEST (algebraic); basis 0 (default) or in (num_values, 64] */
typedef struct spmv_c_eigs_config {
    int32_t num_values;
    int32_t which;
    int32_t basis;
    float   tolerance;
    int32_t max_iterations;
    int32_t engine;
} spmv_c_eigs_config;

/* breakdown: 0 none, 1 INVARIANT_SUBSPACE (fewer than num_values pairs exist in the start vector's Krylov space),
 * 2 NOT_FINITE; converged and max_residual come from A y - theta y recomputed with the returned pairs (28 bytes) */
typedef struct spmv_c_eigs_result {
    int32_t error_code;
    int32_t iterations;
    int32_t restarts;
    int32_t converged;
    int32_t breakdown;
    float   max_residual;
    float   elapsed_ms;
} spmv_c_eigs_result;

/* num_values eigenpairs at one end of the spectrum of the symmetric device matrix A by thick-restart Lanczos:
 * d_values num_values floats, vector i num_rows floats at d_vectors + i * ldv, d_residuals (may be NULL) num_values
 * floats, d_v0 (may be NULL) the start vector.  config NULL = defaults (1, LARGEST, 0, 1e-5, 1000, auto).  Argument
 * checks and numerics as eigs_sym in include/spmv/eigs.h.  The return value equals out->error_code (out may be NULL). */
int spmv_c_eigs_sym(const spmv_c_csr* A, float* d_values, float* d_vectors, int64_t ldv, float* d_residuals,
                    const float* d_v0, const spmv_c_eigs_config* config, spmv_c_eigs_result* out);

/* eigen-decomposition of the dense symmetric fp64 matrix T (host, order n <= 64, leading dimension ld) by the fixed
 * Jacobi rule of include/spmv/eigs.h: values ascending, eigenvector i at vectors + i * ld (host).  on_device != 0 runs
 * the one-workgroup device kernel instead of the host twin; both give the same bits.  Returns an SpMVError code. */
int spmv_c_sym_eig_small(int n, const double* T, int ld, double* values, double* vectors, int on_device);

/* ---- sparse triangular solve with level scheduling (extension; include/spmv/sptrsv.h) ---- */
/* uplo: 0 LOWER, 1 UPPER; diag: 0 NON_UNIT, 1 UNIT; ordered: 1 = one lane per row in the CPU's summation order
 * (bit-identical to spmv_c_sptrsv_cpu_csr), 0 = 1-64 lanes per row; reserved: 0 (16 bytes) */
typedef struct spmv_c_sptrsv_config {
    int32_t uplo;
    int32_t diag;
    int32_t ordered;
    int32_t reserved;
} spmv_c_sptrsv_config;

/* 24 bytes */
typedef struct spmv_c_sptrsv_result {
    int32_t error_code;
    int32_t num_levels;
    int32_t launches;
    int32_t lanes_per_row;
    float   analysis_ms;   /* 0 when the cached schedule was used */
    float   elapsed_ms;    /* the solve launches only */
} spmv_c_sptrsv_result;

/* Solves T x = b on the device, T the chosen triangle of the square matrix A (entries on the other side of the
 * diagonal are ignored); d_b and d_x hold num_rows floats and may be the same array.  config NULL = defaults (LOWER,
 * NON_UNIT, 0, 0).  Argument checks, analysis cache and numerics as sptrsv_csr in include/spmv/sptrsv.h.  The return
 * value equals out->error_code (out may be NULL). */
int spmv_c_sptrsv_csr(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                      spmv_c_sptrsv_result* out);
/* the same solve enqueued on a caller stream without timing or synchronisation (the first call per matrix and
 * triangle still analyses and synchronises that stream: call spmv_c_sptrsv_analyze first) */
int spmv_c_sptrsv_csr_async(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                            void* hip_stream);
/* builds and caches the schedule of A's uplo triangle ahead of a timed call; fills num_levels, launches, analysis_ms */
int spmv_c_sptrsv_analyze(const spmv_c_csr* A, int uplo, spmv_c_sptrsv_result* out);
/* the same with the analysis run on the device: no array of A crosses the bus (sptrsv_analyze_device in
 * include/spmv/sptrsv.h); analysis_ms is 0 when a schedule, however built, is already cached */
int spmv_c_sptrsv_analyze_device(const spmv_c_csr* A, int uplo, spmv_c_sptrsv_result* out);
/* what the cached schedule of (A, uplo) holds besides its arrays (32 bytes); one_sided_row: only its sign is shared
 * between the host and the device analysis */
typedef struct spmv_c_sptrsv_schedule_info {
    int32_t num_levels;
    int32_t launches;
    int32_t first_missing_diagonal;
    int32_t first_unsorted_row;
    int32_t one_sided_row;
    int32_t built_on_device;
    int64_t triangle_nnz;
} spmv_c_sptrsv_schedule_info;
/* copies the cached schedule of (A, uplo), of either origin, to host arrays: level_ptr (num_levels + 1 ints; room for
 * num_rows + 1), order (num_rows ints), info; each may be NULL.  Builds nothing: without a cached schedule it returns
 * INVALID_ARGUMENT and writes nothing (sptrsv_schedule_get in include/spmv/sptrsv.h) */
int spmv_c_sptrsv_schedule_get(const spmv_c_csr* A, int uplo, int32_t* level_ptr, int32_t* order,
                               spmv_c_sptrsv_schedule_info* info);
/* host forward / backward substitution on A's host arrays (b and x host arrays, may be the same); returns the error code */
int spmv_c_sptrsv_cpu_csr(const spmv_c_csr* A, const float* b, float* x, const spmv_c_sptrsv_config* config);
/* spmv_c_sptrsv_csr for k right-hand sides (1..32) in one launch sequence: d_B and d_X are num_rows x k row-major
 * with leading dimensions ldb, ldx >= k, and may be the same array when ldb == ldx.  Column j is bit for bit
 * spmv_c_sptrsv_csr on that column; num_levels, launches and lanes_per_row are the single call's.  Checks and
 * numerics as sptrsv_csr_multi in include/spmv/sptrsv.h.  The return value equals out->error_code (out may be NULL). */
int spmv_c_sptrsv_csr_multi(const spmv_c_csr* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                            const spmv_c_sptrsv_config* config, spmv_c_sptrsv_result* out);
/* the same enqueued on a caller stream without timing or synchronisation (spmv_c_sptrsv_csr_async's rules) */
int spmv_c_sptrsv_csr_multi_async(const spmv_c_csr* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                                  const spmv_c_sptrsv_config* config, void* hip_stream);
/* spmv_c_sptrsv_cpu_csr column by column on host arrays B and X (num_rows x k row-major; B == X with ldb == ldx is
 * allowed); returns the error code */
int spmv_c_sptrsv_cpu_csr_multi(const spmv_c_csr* A, const float* B, int ldb, float* X, int ldx, int k,
                                const spmv_c_sptrsv_config* config);
/* the level analysis as a pure host function: level_ptr[num_rows + 1], order[num_rows]; *first_missing_diagonal (may
 * be NULL) = lowest row without a stored diagonal entry, or -1 */
int spmv_c_sptrsv_levels(int num_rows, const int32_t* row_ptrs, const int32_t* col_indices, int uplo,
                         int32_t* level_ptr, int32_t* order, int32_t* num_levels, int32_t* first_missing_diagonal);

/* ---- ILU(0) factorisation over the LOWER level schedule (extension; include/spmv/ilu0.h) ---- */
/* 28 bytes */
typedef struct spmv_c_ilu0_result {
    int32_t error_code;
    int32_t num_levels;
    int32_t launches;
    int32_t lanes_per_row;
    int32_t zero_pivot;    /* lowest row whose u_ii is zero or not finite, or -1 */
    float   analysis_ms;   /* 0 when the cached schedule was used */
    float   elapsed_ms;    /* the factorisation launches only */
} spmv_c_ilu0_result;

/* Factors the square device matrix A (columns strictly ascending in every row, every diagonal stored) into
 * d_lu_values: nnz floats in A's pattern, L left of the diagonal (unit diagonal not stored), U on and right of it;
 * d_lu_values may be A's own device value array (in place).  Bit-identical to spmv_c_ilu0_cpu_csr.  Argument checks
 * and arithmetic as ilu0_csr in include/spmv/ilu0.h.  The return value equals out->error_code (out may be NULL). */
int spmv_c_ilu0_csr(const spmv_c_csr* A, float* d_lu_values, spmv_c_ilu0_result* out);
/* the same factorisation enqueued on a caller stream without timing, pivot scan or synchronisation */
int spmv_c_ilu0_csr_async(const spmv_c_csr* A, float* d_lu_values, void* hip_stream);
/* the factorisation on A's host arrays (lu_values: nnz floats, may be A's host values); *zero_pivot may be NULL */
int spmv_c_ilu0_cpu_csr(const spmv_c_csr* A, float* lu_values, int32_t* zero_pivot);

/* ---- IC(0) factorisation over the LOWER level schedule (extension; include/spmv/ic0.h) ---- */
/* 28 bytes */
typedef struct spmv_c_ic0_result {
    int32_t error_code;
    int32_t num_levels;
    int32_t launches;
    int32_t lanes_per_row;
    int32_t bad_pivot;     /* lowest row whose l_ii is not > 0 or not finite, or -1 */
    float   analysis_ms;   /* 0 when the cached schedule was used */
    float   elapsed_ms;    /* the factorisation launches only */
} spmv_c_ic0_result;

/* Factors the square device matrix A (columns strictly ascending in every row, every diagonal stored, a structurally
 * symmetric pattern; only the lower triangle's values are read) into d_l_values: nnz floats in A's pattern, L on and
 * left of the diagonal, L^T right of it; d_l_values may be A's own device value array (in place).  Bit-identical to
 * spmv_c_ic0_cpu_csr.  Argument checks and arithmetic as ic0_csr in include/spmv/ic0.h.  The return value equals
 * out->error_code (out may be NULL). */
int spmv_c_ic0_csr(const spmv_c_csr* A, float* d_l_values, spmv_c_ic0_result* out);
/* the same factorisation enqueued on a caller stream without timing, pivot scan or synchronisation */
int spmv_c_ic0_csr_async(const spmv_c_csr* A, float* d_l_values, void* hip_stream);
/* the factorisation on A's host arrays (l_values: nnz floats, may be A's host values); *bad_pivot may be NULL */
int spmv_c_ic0_cpu_csr(const spmv_c_csr* A, float* l_values, int32_t* bad_pivot);

/* ---- factorised sparse approximate inverse G ~ L^-1, A = L L^T (extension; include/spmv/fsai.h) ---- */
/* 32 bytes */
typedef struct spmv_c_fsai_result {
    int32_t error_code;
    int32_t nnz;            /* stored entries of G */
    int32_t max_row;        /* longest pattern row */
    int32_t row_class;      /* capacity class of the kernel: 4, 8, 16, 32 or 64 */
    int32_t lanes_per_row;
    int32_t bad_row;        /* lowest row whose g_ii is not > 0 or not finite, or -1 */
    int32_t long_row;       /* lowest row with more than 64 pattern entries, or -1 */
    float   elapsed_ms;     /* structure build + numeric kernel */
} spmv_c_fsai_result;

/* G = FSAI of the square device matrix A (rows strictly ascending; only the values on and left of the diagonal are
 * read) on the lower pattern of S (NULL: A; only S's structure is read).  G owns new device arrays afterwards (as
 * spmv_c_csr_transpose_gpu leaves AT); spmv_c_csr_from_gpu(G) fills its host arrays.  Bit-identical to
 * spmv_c_fsai_cpu_csr at every lane count and row class.  Checks and arithmetic as fsai_csr in include/spmv/fsai.h.
 * The return value equals out->error_code (out may be NULL). */
int spmv_c_fsai_csr(spmv_c_csr* G, const spmv_c_csr* A, const spmv_c_csr* S, spmv_c_fsai_result* out);
/* only G's device values again from a new A, on the pattern an earlier spmv_c_fsai_csr produced */
int spmv_c_fsai_csr_numeric(spmv_c_csr* G, const spmv_c_csr* A, spmv_c_fsai_result* out);
/* the same operation on host arrays, the definition of the arithmetic; G gets new host arrays; *bad_row may be NULL */
int spmv_c_fsai_cpu_csr(spmv_c_csr* G, const spmv_c_csr* A, const spmv_c_csr* S, int32_t* bad_row);

/* ---- sparse matrix-matrix product C = A*B (extension; include/spmv/spgemm.h) ---- */
/* 104 bytes */
typedef struct spmv_c_spgemm_result {
    int32_t error_code;
    int32_t nnz;                /* entries of C */
    int64_t products;           /* sum over A's entries of the length of the B row they point at */
    int32_t max_row_products;   /* clamped to INT32_MAX */
    int32_t max_row_nnz;
    int32_t symbolic_rows[8];   /* rows per accumulator class in the symbolic pass ([0] = rows without products) */
    int32_t numeric_rows[8];    /* the same for the numeric pass */
    int32_t lanes;              /* lanes that share one row of C */
    float   symbolic_ms;
    float   numeric_ms;
} spmv_c_spgemm_result;

/* C = A*B of two device matrices, bit-identical to spmv_c_spgemm_cpu_csr; B's columns strictly ascending in every
 * row.  C owns new device arrays afterwards (as spmv_c_csr_transpose_gpu leaves AT); spmv_c_csr_from_gpu(C) fills its
 * host arrays.  Checks and arithmetic as spgemm_csr in include/spmv/spgemm.h.  The return value equals
 * out->error_code (out may be NULL). */
int spmv_c_spgemm_csr(spmv_c_csr* C, const spmv_c_csr* A, const spmv_c_csr* B, spmv_c_spgemm_result* out);
/* only C's device values again, into the pattern an earlier spmv_c_spgemm_csr produced; the pattern is checked */
int spmv_c_spgemm_csr_numeric(spmv_c_csr* C, const spmv_c_csr* A, const spmv_c_csr* B, spmv_c_spgemm_result* out);
/* the product on host arrays, the definition of the arithmetic; C gets new host arrays */
int spmv_c_spgemm_cpu_csr(spmv_c_csr* C, const spmv_c_csr* A, const spmv_c_csr* B);
/* most distinct columns of a row in accumulator class cls (1-based); INT32_MAX for the dense class, -1 past it */
int spmv_c_spgemm_class_capacity(int cls);

/* ---- aggregation AMG and AMG-preconditioned CG (extension; include/spmv/amg.h, include/spmv/cg.h) ---- */
/* 28 bytes; the defaults of AMGConfig are 10, 64, 0.08, 1, 1, 2/3, 4 */
typedef struct spmv_c_amg_config {
    int32_t max_levels;      /* >= 1 */
    int32_t coarse_rows;     /* 1 .. 1024 */
    float   strength;        /* theta >= 0 */
    int32_t pre_sweeps;      /* >= 1 */
    int32_t post_sweeps;     /* >= 0 */
    float   jacobi_weight;   /* omega in (0, 2) */
    int32_t coarse_sweeps;   /* >= 1 */
} spmv_c_amg_config;
/* 48 bytes */
typedef struct spmv_c_amg_result {
    int32_t error_code;
    int32_t levels;
    int32_t coarse_solver;   /* 0 dense inverse, 1 Jacobi sweeps */
    int32_t bad_row;         /* -1 when no diagonal / pivot check failed */
    int32_t bad_level;
    double  grid_complexity;
    double  operator_complexity;
    float   setup_ms;
} spmv_c_amg_result;
typedef struct spmv_c_amg spmv_c_amg;             /* opaque: the hierarchy; one hierarchy serves one stream at a time */

/* Builds the hierarchy of the square device matrix A; *out is NULL on failure.  config may be NULL (the defaults).
 * aggregates may be NULL (the library aggregates), else aggregate_levels host arrays, aggregates[l][i] = the aggregate
 * of row i of level l.  Checks and arithmetic as amg_setup in include/spmv/amg.h.  The return value equals
 * result->error_code (result may be NULL). */
int spmv_c_amg_setup(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config, int aggregate_levels,
                     const int32_t* const* aggregates, spmv_c_amg_result* result);
/* new values in the same pattern: every level refilled, aggregates kept, nothing allocated again */
int spmv_c_amg_update(spmv_c_amg* H, const spmv_c_csr* A, spmv_c_amg_result* result);
void spmv_c_amg_destroy(spmv_c_amg* H);
int spmv_c_amg_num_levels(const spmv_c_amg* H);
/* level `level` as a non-owning device view; *d_aggregate (n_l ints on the device) is NULL on the coarsest level */
int spmv_c_amg_level(const spmv_c_amg* H, int level, spmv_c_csr* view, const int32_t** d_aggregate,
                     int32_t* num_aggregates);
/* d_z = one V-cycle on d_r from a zero guess */
int spmv_c_amg_apply(const spmv_c_amg* H, const float* d_r, float* d_z);
/* the aggregation of one level on A's host arrays: aggregate[num_rows], *num_aggregates */
int spmv_c_amg_aggregate_cpu_csr(const spmv_c_csr* A, float strength, int32_t* aggregate, int32_t* num_aggregates);
/* the MIS-2 aggregation of one level on A's host arrays, the definition of the device's: aggregate[num_rows] (-1 = a
 * vertex left free), *num_aggregates, *rounds (may be NULL) = the synchronous round count */
int spmv_c_amg_aggregate_mis2_cpu_csr(const spmv_c_csr* A, float strength, uint32_t seed, int32_t* aggregate,
                                      int32_t* num_aggregates, int32_t* rounds);
/* the same ints on the device: d_aggregate holds num_rows ints on the device; *rounds (may be NULL) = the rounds taken */
int spmv_c_amg_aggregate_mis2_gpu(const spmv_c_csr* A, float strength, uint32_t seed, int32_t* d_aggregate,
                                  int32_t* num_aggregates, int32_t* rounds);
/* amg_setup with every level's diagonal, aggregation (MIS-2 with `seed`) and P made on the device; checks and
 * arithmetic as amg_setup_device in include/spmv/amg.h.  The return value equals result->error_code. */
int spmv_c_amg_setup_device(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config, uint32_t seed,
                            spmv_c_amg_result* result);
/* rounds the root selection of level `level` took; 0 on the coarsest level and on a hierarchy spmv_c_amg_setup built */
int spmv_c_amg_setup_rounds(const spmv_c_amg* H, int level);
/* ---- smoothed aggregation (include/spmv/amg.h, "Smoothed aggregation") ---- */
/* 8 bytes; the defaults of AMGSmoothing are 2/3, 0.5 */
typedef struct spmv_c_amg_smoothing {
    float prolongator_weight;   /* omega_p in (0, 2) */
    float strength_decay;       /* in (0, 1]: theta_{l+1} = theta_l * strength_decay */
} spmv_c_amg_smoothing;
/* spmv_c_amg_setup with smoothed prolongators; smoothing may be NULL (the defaults) */
int spmv_c_amg_setup_smoothed(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config,
                              const spmv_c_amg_smoothing* smoothing, int aggregate_levels,
                              const int32_t* const* aggregates, spmv_c_amg_result* result);
/* spmv_c_amg_setup_device with smoothed prolongators */
int spmv_c_amg_setup_smoothed_device(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config,
                                     const spmv_c_amg_smoothing* smoothing, uint32_t seed, spmv_c_amg_result* result);
int spmv_c_amg_is_smoothed(const spmv_c_amg* H);   /* 0 for NULL */
/* P and P^T of level `level` as non-owning device views (either may be NULL) */
int spmv_c_amg_level_transfer(const spmv_c_amg* H, int level, spmv_c_csr* P_view, spmv_c_csr* PT_view);
/* the host definition of one level's smoothed P: aggregate[num_rows] in [0, num_aggregates) */
int spmv_c_amg_prolongator_cpu_csr(spmv_c_csr* P, const spmv_c_csr* A, const int32_t* aggregate, int num_aggregates,
                                   float weight);
/* d_f_coarse = P^T (d_f - A_l d_x) and d_x += P d_e on level `level`, device vectors */
int spmv_c_amg_restrict(const spmv_c_amg* H, int level, const float* d_f, const float* d_x, float* d_f_coarse);
int spmv_c_amg_prolong(const spmv_c_amg* H, int level, const float* d_e, float* d_x);
/* CG preconditioned by one V-cycle of H per iteration; config->preconditioner is not read.  Checks and numerics as
 * cg_solve_amg in include/spmv/cg.h. */
int spmv_c_cg_solve_amg(const spmv_c_csr* A, const spmv_c_amg* H, const float* d_b, float* d_x,
                        const spmv_c_cg_config* config, spmv_c_cg_result* out);

/* ---- multicolour reordering (extension; include/spmv/reorder.h) ---- */
/* seed of the vertex priorities; symmetric_pattern: 1 = only A's rows are walked (the caller's promise);
 * lanes_per_row: 0 = from the mean degree, else 1, 2, 4, ... 64; reserved: 0 (16 bytes) */
typedef struct spmv_c_color_config {
    uint32_t seed;
    int32_t  symmetric_pattern;
    int32_t  lanes_per_row;
    int32_t  reserved;
} spmv_c_color_config;
/* 20 bytes */
typedef struct spmv_c_color_result {
    int32_t error_code;
    int32_t num_colors;
    int32_t rounds;
    int32_t launches;
    float   elapsed_ms;
} spmv_c_color_result;

/* Colours the graph of the square device matrix A into d_colors (num_rows ints on the device): greedy first-fit in
 * descending (fmix32(i ^ seed), i) priority, the same ints as spmv_c_csr_color_cpu.  config may be NULL (0, 0, 0, 0).
 * Checks and algorithm as csr_color in include/spmv/reorder.h.  The return value equals out->error_code (out may be
 * NULL). */
int spmv_c_csr_color(const spmv_c_csr* A, int32_t* d_colors, const spmv_c_color_config* config,
                     spmv_c_color_result* out);
/* the definition on A's host arrays; *num_colors and *rounds (the synchronous round count) may be NULL */
int spmv_c_csr_color_cpu(const spmv_c_csr* A, int32_t* colors, int32_t* num_colors, int32_t* rounds,
                         const spmv_c_color_config* config);
/* the vertices sorted by (colour, index) on the device: d_perm[new] = old, d_inverse[old] = new; color_ptr (host,
 * num_colors + 1 ints) may be NULL */
int spmv_c_color_ordering(int n, const int32_t* d_colors, int num_colors, int32_t* d_perm, int32_t* d_inverse,
                          int32_t* color_ptr);
/* B = P A Q^T on the device with sorted rows: row i of B is row d_row_perm[i] of A, column j renamed d_col_inverse[j];
 * either array may be NULL (the identity).  B owns new device arrays afterwards (as spmv_c_csr_transpose_gpu leaves
 * AT).  Bit for bit spmv_c_csr_permute_cpu's result.  Checks as csr_permute_gpu in include/spmv/reorder.h. */
int spmv_c_csr_permute_gpu(spmv_c_csr* B, const spmv_c_csr* A, const int32_t* d_row_perm,
                           const int32_t* d_col_inverse);
/* the same on host arrays; B owns new host arrays */
int spmv_c_csr_permute_cpu(spmv_c_csr* B, const spmv_c_csr* A, const int32_t* row_perm, const int32_t* col_inverse);
/* d_out[i * ldo + j] = d_in[d_index[i] * ldi + j] for i < n, j < k (1..32), row-major with ldo, ldi >= k */
int spmv_c_permute_gather(float* d_out, int ldo, const float* d_in, int ldi, const int32_t* d_index, int n, int k);
/* the same enqueued on a caller stream without synchronisation */
int spmv_c_permute_gather_async(float* d_out, int ldo, const float* d_in, int ldi, const int32_t* d_index, int n,
                                int k, void* hip_stream);
/* colouring, ordering and B = P A P^T in one call; d_perm and d_inverse: num_rows ints each on the device.  The return
 * value equals out->error_code (out may be NULL). */
int spmv_c_multicolor_reorder(spmv_c_csr* B, const spmv_c_csr* A, int32_t* d_perm, int32_t* d_inverse,
                              const spmv_c_color_config* config, spmv_c_color_result* out);

/* ---- reverse Cuthill-McKee reordering (extension; include/spmv/reorder.h) ---- */
/* symmetric_pattern: 1 = only A's rows are walked (the caller's promise); peripheral: 1 = a pseudo-peripheral start
 * per component, 0 = the vertex of smallest (degree, index); lanes_per_row: 0 = from the mean degree, else 1, 2, 4,
 * ... 64; reserved: 0 (16 bytes).  NULL stands for (0, 1, 0, 0). */
typedef struct spmv_c_rcm_config {
    int32_t symmetric_pattern;
    int32_t peripheral;
    int32_t lanes_per_row;
    int32_t reserved;
} spmv_c_rcm_config;
/* 24 bytes */
typedef struct spmv_c_rcm_result {
    int32_t error_code;
    int32_t components;
    int32_t levels;
    int32_t sweeps;
    int32_t launches;
    float   elapsed_ms;
} spmv_c_rcm_result;
/* 16 bytes: max(i - j), max(j - i) over the stored entries, sum over the rows of i - min(i, smallest stored column) */
typedef struct spmv_c_csr_band {
    int32_t lower;
    int32_t upper;
    int64_t profile;
} spmv_c_csr_band;

/* The reverse Cuthill-McKee ordering of the square device matrix A (rows strictly ascending): d_perm[new] = old,
 * d_inverse[old] = new, num_rows ints each on the device; the same ints as spmv_c_csr_rcm_cpu.  Checks and algorithm as
 * csr_rcm in include/spmv/reorder.h.  The return value equals out->error_code (out may be NULL). */
int spmv_c_csr_rcm(const spmv_c_csr* A, int32_t* d_perm, int32_t* d_inverse, const spmv_c_rcm_config* config,
                   spmv_c_rcm_result* out);
/* the definition on A's host arrays; *components and *levels may be NULL */
int spmv_c_csr_rcm_cpu(const spmv_c_csr* A, int32_t* perm, int32_t* inverse, int32_t* components, int32_t* levels,
                       const spmv_c_rcm_config* config);
/* spmv_c_csr_rcm, then B = P A P^T (spmv_c_csr_permute_gpu) */
int spmv_c_rcm_reorder(spmv_c_csr* B, const spmv_c_csr* A, int32_t* d_perm, int32_t* d_inverse,
                       const spmv_c_rcm_config* config, spmv_c_rcm_result* out);
/* the band statistics of A's device arrays / host arrays: the same integers */
int spmv_c_csr_band_gpu(const spmv_c_csr* A, spmv_c_csr_band* out);
int spmv_c_csr_band_cpu(const spmv_c_csr* A, spmv_c_csr_band* out);

/* ---- matrix assembly (extension; include/spmv/assemble.h) ---- */
/* duplicates: 0 = equal (row, column) pairs are summed in source order, 1 = every triplet is kept; reserved: 0
 * (8 bytes) */
typedef struct spmv_c_coo_config {
    int32_t duplicates;
    int32_t reserved;
} spmv_c_coo_config;
/* 28 bytes; combined = n - nnz_out; passes = radix passes run; tile_entries = entries one workgroup sorts per pass */
typedef struct spmv_c_coo_result {
    int32_t error_code;
    int32_t nnz_out;
    int32_t combined;
    int32_t passes;
    int32_t tile_entries;
    int32_t launches;
    float   elapsed_ms;
} spmv_c_coo_result;
/* the sorted order of one assembly: 4 * n bytes on the device, plus 4 * (nnz_out + 1) when duplicates are summed */
typedef struct spmv_c_coo_plan spmv_c_coo_plan;

/* The definition on host arrays: C = the num_rows x num_cols matrix of the n triplets (rows[p], cols[p], vals[p]), in
 * any order, repeats allowed; stable order by (row, column), equal pairs summed left to right in fp32 from the first
 * value.  config may be NULL (0, 0).  C owns new host arrays.  Rule and checks as csr_from_coo_cpu in
 * include/spmv/assemble.h. */
int spmv_c_csr_from_coo_cpu(spmv_c_csr* C, int num_rows, int num_cols, int n, const int32_t* rows, const int32_t* cols,
                            const float* vals, const spmv_c_coo_config* config);
/* The same from device arrays on the device, bit for bit.  C owns new device arrays afterwards (as
 * spmv_c_csr_transpose_gpu leaves AT).  *plan (plan may be NULL) receives a plan for spmv_c_csr_coo_refill on success.
 * The return value equals out->error_code (out may be NULL).  Checks and algorithm as csr_from_coo_gpu in
 * include/spmv/assemble.h. */
int spmv_c_csr_from_coo_gpu(spmv_c_csr* C, int num_rows, int num_cols, int n, const int32_t* d_rows,
                            const int32_t* d_cols, const float* d_vals, const spmv_c_coo_config* config,
                            spmv_c_coo_plan** plan, spmv_c_coo_result* out);
/* only C's device values again, from a new value array in the same triplet order: one launch; drops C's cached
 * auxiliary data.  The plan does not re-check C's pattern. */
int spmv_c_csr_coo_refill(const spmv_c_coo_plan* plan, spmv_c_csr* C, const float* d_vals);
/* the same enqueued on a caller stream without synchronisation */
int spmv_c_csr_coo_refill_async(const spmv_c_coo_plan* plan, spmv_c_csr* C, const float* d_vals, void* hip_stream);
/* NULL is allowed */
void spmv_c_coo_plan_destroy(spmv_c_coo_plan* plan);
/* what a plan holds; any output pointer may be NULL */
int spmv_c_coo_plan_info(const spmv_c_coo_plan* plan, int32_t* num_rows, int32_t* num_cols, int32_t* n,
                         int32_t* nnz_out, int32_t* duplicates);
/* d_rows[p] = the row that stores entry p of the device matrix A (nnz ints on the device): CSR back to triplets */
int spmv_c_csr_row_indices_gpu(const spmv_c_csr* A, int32_t* d_rows);

/* ---- CSR algebra: C = alpha*A + beta*B, scaling, the diagonal in and out (extension; include/spmv/csr_ops.h) ---- */
/* 32 bytes; common = columns found in both matrices; launches = kernel launches of the call */
typedef struct spmv_c_csr_add_result {
    int32_t error_code;
    int32_t nnz;            /* entries of C */
    int32_t common;
    int32_t max_row_nnz;
    int32_t lanes;          /* lanes that share one row */
    int32_t launches;
    float   symbolic_ms;
    float   numeric_ms;
} spmv_c_csr_add_result;

/* C = alpha*A + beta*B of two device matrices with strictly ascending rows, bit-identical to spmv_c_csr_add_cpu: the
 * pattern is the union, cancelled entries are kept.  C owns new device arrays afterwards (as spmv_c_csr_transpose_gpu
 * leaves AT).  Rule and checks as csr_add in include/spmv/csr_ops.h.  The return value equals out->error_code (out
 * may be NULL). */
int spmv_c_csr_add(spmv_c_csr* C, float alpha, const spmv_c_csr* A, float beta, const spmv_c_csr* B,
                   spmv_c_csr_add_result* out);
/* only C's device values again, into the pattern an earlier spmv_c_csr_add produced: one launch; the pattern is
 * checked; drops C's cached auxiliary data */
int spmv_c_csr_add_numeric(spmv_c_csr* C, float alpha, const spmv_c_csr* A, float beta, const spmv_c_csr* B,
                           spmv_c_csr_add_result* out);
/* the sum on host arrays, the definition of the arithmetic; C gets new host arrays */
int spmv_c_csr_add_cpu(spmv_c_csr* C, float alpha, const spmv_c_csr* A, float beta, const spmv_c_csr* B);
/* out[p] = a[p] * (r[row] * c[col]), each product rounded to fp32; either scale may be NULL; d_values_out NULL or
 * A's own device values = in place (drops A's cached auxiliary data) */
int spmv_c_csr_scale_gpu(spmv_c_csr* A, const float* d_row_scale, const float* d_col_scale, float* d_values_out);
int spmv_c_csr_scale_cpu(const spmv_c_csr* A, const float* row_scale, const float* col_scale, float* values_out);
/* d_diag[i] = fp32 sum of row i's stored (i, i) entries in storage order, 0 where there is none (num_rows floats) */
int spmv_c_csr_diagonal_gpu(const spmv_c_csr* A, float* d_diag);
int spmv_c_csr_diagonal_cpu(const spmv_c_csr* A, float* diag);
/* D = the n x n diagonal matrix of d_diag, the identity when d_diag is NULL; zeros are kept */
int spmv_c_csr_diag_matrix_gpu(spmv_c_csr* D, int n, const float* d_diag);
int spmv_c_csr_diag_matrix_cpu(spmv_c_csr* D, int n, const float* diag);

/* ---- block CSR (BSR): container, CSR <-> BSR, SpMV (extension; include/spmv/bsr_matrix.h, include/spmv/bsr.h) ---- */
/* 80 bytes; square block_dim x block_dim blocks (2, 3, 4 or 8), row-major inside a block, block columns strictly
 * ascending inside a block row; positions outside the matrix hold +0.0f */
typedef struct spmv_c_bsr {
    int32_t  num_rows;
    int32_t  num_cols;
    int32_t  block_dim;
    int32_t  num_block_rows;
    int32_t  num_block_cols;
    int32_t  num_blocks;
    float*   values;            /* [num_blocks * block_dim * block_dim] */
    int32_t* block_cols;        /* [num_blocks] */
    int32_t* block_row_ptrs;    /* [num_block_rows + 1] */
    float*   d_values;
    int32_t* d_block_cols;
    int32_t* d_block_row_ptrs;
    uint8_t  owns_host_memory;
    uint8_t  owns_device_memory;
} spmv_c_bsr;

/* 32 bytes; fill = nnz / positions of the blocks inside the matrix; launches = kernel launches of the call */
typedef struct spmv_c_bsr_build_result {
    int32_t error_code;
    int32_t num_blocks;
    float   fill;
    int32_t max_block_row;
    int32_t lanes;          /* lanes that share one block row */
    int32_t launches;
    float   symbolic_ms;
    float   numeric_ms;
} spmv_c_bsr_build_result;

/* NULL on a negative size or an unsupported block_dim */
spmv_c_bsr* spmv_c_bsr_create(int rows, int cols, int block_dim, int num_blocks);
void spmv_c_bsr_destroy(spmv_c_bsr* mat);
int spmv_c_bsr_to_gpu(spmv_c_bsr* mat);
int spmv_c_bsr_from_gpu(spmv_c_bsr* mat);
void spmv_c_bsr_free_gpu(spmv_c_bsr* mat);
void spmv_c_bsr_invalidate_gpu_cache(const spmv_c_bsr* mat);
/* a matrix header over device arrays the caller owns (no host arrays) */
spmv_c_bsr* spmv_c_bsr_wrap_device(int rows, int cols, int block_dim, int num_blocks, const int32_t* d_block_row_ptrs,
                                   const int32_t* d_block_cols, const float* d_values);
/* CSR (strictly ascending rows) to BSR: the host twin is the definition, the device build has its ints and bits at
 * every lane count; B owns new arrays afterwards.  Rule and checks as bsr_from_csr_gpu in include/spmv/bsr.h.  The
 * return value equals out->error_code (out may be NULL). */
int spmv_c_bsr_from_csr_cpu(spmv_c_bsr* B, const spmv_c_csr* A, int block_dim);
int spmv_c_bsr_from_csr_gpu(spmv_c_bsr* B, const spmv_c_csr* A, int block_dim, spmv_c_bsr_build_result* out);
/* only B's device values again from a new A over the same pattern; an entry without a block is INVALID_FORMAT */
int spmv_c_bsr_from_csr_numeric(spmv_c_bsr* B, const spmv_c_csr* A, spmv_c_bsr_build_result* out);
/* the counting pass alone: *blocks = the blocks the build would store */
int spmv_c_csr_block_count_gpu(const spmv_c_csr* A, int block_dim, int64_t* blocks);
/* BSR back to CSR with sorted rows; keep_zeros == 0 drops the positions that hold +-0.0f */
int spmv_c_bsr_to_csr_gpu(spmv_c_csr* A, const spmv_c_bsr* B, int keep_zeros);
int spmv_c_bsr_to_csr_cpu(spmv_c_csr* A, const spmv_c_bsr* B, int keep_zeros);
void spmv_c_cpu_bsr(const spmv_c_bsr* A, const float* x, float* y);        /* spmv_cpu_bsr */
/* y = A x; SCALAR_CSR / ELL_KERNEL / NULL config: spmv_c_cpu_bsr's bits; VECTOR_CSR / MERGE_PATH: the lane-group kernel */
int spmv_c_spmv_bsr(const spmv_c_bsr* A, const float* d_x, float* d_y, const spmv_c_config* config, int vec_size,
                    spmv_c_result* out);
int spmv_c_spmv_bsr_async(const spmv_c_bsr* A, const float* d_x, float* d_y, const spmv_c_config* config,
                          int vec_size, void* hip_stream);
int spmv_c_compute_bandwidth_bsr(const spmv_c_bsr* A, float elapsed_ms, spmv_c_bandwidth* out);
/* the inverses of the diagonal blocks (num_block_rows * b * b floats, block I row-major) and z = D^-1 r by the ordered
 * sum; host twins and device paths give the same bits.  Rules and checks as in include/spmv/bsr.h. */
int spmv_c_bsr_diag_inverse_cpu(const spmv_c_bsr* A, float* inv);
int spmv_c_bsr_diag_inverse_gpu(const spmv_c_bsr* A, float* d_inv);
void spmv_c_bsr_diag_apply_cpu(const spmv_c_bsr* A, const float* inv, const float* r, float* z);
int spmv_c_bsr_diag_apply(const spmv_c_bsr* A, const float* d_inv, const float* d_r, float* d_z);
/* CG on a BSR matrix; config->preconditioner 0 NONE, 1 JACOBI, 2 BLOCK_JACOBI (this entry point only); engine -1 or 0.
 * Checks and numerics as cg_solve_bsr in include/spmv/cg.h.  Returns out->error_code (out may be NULL). */
int spmv_c_cg_solve_bsr(const spmv_c_bsr* A, const float* d_b, float* d_x, const spmv_c_cg_config* config,
                        spmv_c_cg_result* out);
/* Block IC(0) and the block triangular solves (include/spmv/bsr_factor.h, which holds the factor format, the arithmetic
 * and the checks).  f_values / d_f_values: num_blocks * b * b floats in A's block pattern, may be A's own values (in
 * place); spmv_c_bsr_wrap_device over A's structure arrays and d_f_values is the factor matrix F of both solves.  The
 * result of the factorisation has spmv_c_ic0_result's layout: lanes_per_row counts the lanes of a BLOCK row and
 * bad_pivot is a BLOCK row.  The device factor is bit for bit spmv_c_bsr_ic0_cpu; the solve with ordered = 1 is bit for
 * bit spmv_c_sptrsv_cpu_bsr.  Return values equal out->error_code (out may be NULL). */
int spmv_c_bsr_ic0_cpu(const spmv_c_bsr* A, float* f_values, int* bad_pivot);
int spmv_c_bsr_ic0(const spmv_c_bsr* A, float* d_f_values, spmv_c_ic0_result* out);
int spmv_c_bsr_ic0_async(const spmv_c_bsr* A, float* d_f_values, void* hip_stream);
int spmv_c_sptrsv_cpu_bsr(const spmv_c_bsr* F, const float* b, float* x, const spmv_c_sptrsv_config* config);
int spmv_c_sptrsv_bsr(const spmv_c_bsr* F, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                      spmv_c_sptrsv_result* out);
int spmv_c_sptrsv_bsr_async(const spmv_c_bsr* F, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                            void* hip_stream);
int spmv_c_sptrsv_analyze_bsr(const spmv_c_bsr* A, int uplo, spmv_c_sptrsv_result* out);
/* CG preconditioned with the block factor F (cg_solve_bsr_ic in include/spmv/cg.h); config->preconditioner is not read. */
int spmv_c_cg_solve_bsr_ic(const spmv_c_bsr* A, const spmv_c_bsr* F, const float* d_b, float* d_x,
                           const spmv_c_cg_config* config, spmv_c_cg_result* out);

/* ---- bandwidth model: reference include/spmv/bandwidth.h:21-27 ---- */
int spmv_c_compute_bandwidth_csr(const spmv_c_csr* A, float elapsed_ms, spmv_c_bandwidth* out);
int spmv_c_compute_bandwidth_ell(const spmv_c_ell* A, float elapsed_ms, spmv_c_bandwidth* out);
/* extension: the byte model of spmv_c_spmv_csr_multi, nnz*8 + (rows+1)*4 + k*cols*4 + k*rows*4 */
int spmv_c_compute_bandwidth_csr_multi(const spmv_c_csr* A, int k, float elapsed_ms, spmv_c_bandwidth* out);
float spmv_c_get_gpu_peak_bandwidth(void);

/* ---- PageRank: reference include/spmv/pagerank.h:29-43 ---- */
int spmv_c_pagerank(const spmv_c_csr* adj, const spmv_c_pagerank_config* config,
                    spmv_c_pagerank_result* out);
void spmv_c_pagerank_free(spmv_c_pagerank_result* result);
/* extension (the reference's pagerank(), include/spmv/pagerank.h:29-31, is single-device): the same call
 * with the CSR rows sharded over num_gpus devices of this process, equal-nnz row blocks, one RCCL all-gather
 * of the rank slices per iteration.  Needs the matrix's HOST arrays.  out->ranks == NULL when fewer than
 * num_gpus devices or no librccl are available.  Returns 0, or -8 for null arguments. */
int spmv_c_pagerank_multi_gpu(const spmv_c_csr* adj, const spmv_c_pagerank_config* config, int num_gpus,
                              spmv_c_pagerank_result* out);
/* extension: the row boundaries pagerank_multi_gpu uses — bounds[num_shards + 1], binary search on the host
 * row_ptrs for equal nnz */
int spmv_c_pagerank_shard_bounds(const int32_t* row_ptrs, int num_rows, int num_shards, int32_t* bounds);
void spmv_c_pagerank_top_k(const spmv_c_pagerank_result* result, int num_nodes, int k,
                           spmv_c_topk_node* top_k);

/* extension (spmv::pagerank_personalized, include/spmv/pagerank.h): personalized PageRank for k teleport vectors
 * (1..32) in one matrix pass per step.  d_V (read only) and d_R are num_rows x k row-major device arrays with leading
 * dimensions ldv, ldr >= k; results holds k entries (20 bytes each).  Column j is bit for bit the k = 1 call on that
 * column.  Checks and numerics as pagerank_personalized in include/spmv/pagerank.h.  Returns the error code. */
typedef struct spmv_c_personalized_result {
    int32_t error_code;
    int32_t iterations;
    float   final_residual;
    int32_t converged;
    float   elapsed_ms;
} spmv_c_personalized_result;
int spmv_c_pagerank_personalized(const spmv_c_csr* adj, const float* d_V, int ldv, float* d_R, int ldr, int k,
                                 const spmv_c_pagerank_config* config, spmv_c_personalized_result* results);
/* the same with column j teleporting uniformly to the nodes seed_nodes[seed_ptrs[j] .. seed_ptrs[j + 1]) (host
 * arrays): an empty set, a node out of range or a node twice in one set is -8 (INVALID_ARGUMENT) */
int spmv_c_pagerank_personalized_seeds(const spmv_c_csr* adj, const int32_t* seed_ptrs, const int32_t* seed_nodes,
                                       int k, float* d_R, int ldr, const spmv_c_pagerank_config* config,
                                       spmv_c_personalized_result* results);

/* ---- PageRank shard engine (extension: the row-sharded multi-GPU loop) ----
 * One rank owns A_local->num_rows consecutive rows of the n_global-node matrix (A_local: device
 * CSR, row_ptrs rebased to 0) and full-length device vectors of A_local->num_cols floats, which
 * the column indices address; its nodes sit at [row_offset, row_offset + num_rows) of those
 * vectors (num_cols may exceed n_global when slices carry padding, see pagerank_dist.py).
 * Per iteration: step -> reduce (partials into the slice tail) -> [all-gather] ->
 * commit_gathered; or with one rank: step -> reduce -> commit.  All calls enqueue on
 * `hip_stream` and return. */
typedef struct spmv_c_pr_shard spmv_c_pr_shard;   /* opaque */
typedef struct spmv_c_pr_status {                 /* device-side state, copied out */
    float   dangling_sum;
    float   final_residual;
    int32_t iterations;
    int32_t converged;
    int32_t done;
    int32_t reserved;
} spmv_c_pr_status;

/* d_dangling_mask (1 = dangling node, indexed like the rank vectors) must stay allocated for the shard's life.  It is a
 * property of the matrix: a shard that steps through the LDS-tiled engine on one contiguous slice reads it when it is
 * created and again at every spmv_c_pr_reset (one bit per local row is kept), so a mask filled or changed after the
 * creation takes effect with the next reset. */
spmv_c_pr_shard* spmv_c_pr_shard_create(const spmv_c_csr* A_local, int row_offset, int n_global,
                                        const uint8_t* d_dangling_mask);
/* the same for a CHUNKED vector layout (the overlapped exchange of pagerank_dist.py): local row i sits at
 * base + (i / piece) * block + i % piece — the vector is a sequence of blocks, block c holding piece c of every
 * rank back to back (base = rank * piece, block = world * piece), so that one in-place all-gather per block
 * delivers it while the blocks that have arrived are already being multiplied (spmv_c_pr_expand) */
spmv_c_pr_shard* spmv_c_pr_shard_create_chunked(const spmv_c_csr* A_local, int base, int piece, int block,
                                                int n_global, const uint8_t* d_dangling_mask);
void spmv_c_pr_shard_destroy(spmv_c_pr_shard* shard);
/* resets the iteration state; dangling_sum = dangling mass of the start vector */
int spmv_c_pr_reset(spmv_c_pr_shard* shard, float dangling_sum, void* hip_stream);
int spmv_c_pr_step(spmv_c_pr_shard* shard, const float* d_r_old, float* d_r_new, float damping,
                   void* hip_stream);
/* optional head start on the NEXT spmv_c_pr_step (same d_r_old): columns [0, cols_ready) of d_r_old are final,
 * the rest may still be arriving.  With the LDS-tiled engine the products of the entries in the strips inside
 * that range are computed now (each strip once; the following step does only what is left); otherwise a no-op.
 * spmv_c_pr_reset voids a head start. */
int spmv_c_pr_expand(spmv_c_pr_shard* shard, const float* d_r_old, int64_t cols_ready, void* hip_stream);
/* the same step, additionally storing every new value at the same offset of `num_peers` other
 * vectors (host array of device pointers: the peers' r_new buffers, IPC-mapped) — a push-style
 * all-gather over xGMI fused into the step's epilogue */
int spmv_c_pr_step_push(spmv_c_pr_shard* shard, const float* d_r_old, float* d_r_new, float damping,
                        float* const* peer_r_new, int num_peers, void* hip_stream);
int spmv_c_pr_reduce(spmv_c_pr_shard* shard, double* d_sums /*[2]*/, void* hip_stream);
int spmv_c_pr_commit(spmv_c_pr_shard* shard, const double* d_sums, float tolerance, void* hip_stream);
/* single rank: reduce + commit in one launch (no sums buffer leaves the engine) */
int spmv_c_pr_reduce_commit(spmv_c_pr_shard* shard, float tolerance, void* hip_stream);
/* single rank: spmv_c_pr_step followed by spmv_c_pr_reduce_commit, with the same results bit for bit.  On the
 * LDS-tiled engine the commit is DEFERRED: one workgroup at the head of the next step's first launch on the same
 * stream does it, so a loop of these calls pays two launches per step, not three.  Any other call on the shard
 * (status_get, expand, reduce, the commit forms, a push step, a step on another stream, destroy) first enqueues
 * the pending commit as a launch of its own on the stream it is given; spmv_c_pr_reset drops it.  Enqueue-only.
 * On a stream that is being captured into a hipGraph nothing is deferred (a commit pending when the capture ends
 * would be missing from the replays); flush (status_get) before a capture begins. */
int spmv_c_pr_step_commit(spmv_c_pr_shard* shard, const float* d_r_old, float* d_r_new, float damping,
                          float tolerance, void* hip_stream);
/* multi-rank commit without an all-reduce: rank p's two partial sums (as doubles) sit in the 16-byte
 * tail of its slice, d_gathered[p * stride + shard_len ...]; stride >= shard_len + 4, both even */
int spmv_c_pr_commit_gathered(spmv_c_pr_shard* shard, const float* d_gathered, int world, int64_t stride,
                              int64_t shard_len, float tolerance, void* hip_stream);
/* syncs — unless hip_stream is being captured into a hipGraph: then the (flush and the) copy are enqueued only,
 * and every replay fills `out`, which must be pinned host memory that outlives the graph */
int spmv_c_pr_status_get(spmv_c_pr_shard* shard, spmv_c_pr_status* out, void* hip_stream);
/* dangling-node detection on the device: accumulate this shard's column sums
 * (atomic adds into d_col_sums[n_global]); after the sums of all shards are
 * combined, mask[c] = (sum == 0). */
int spmv_c_pr_column_sums(const spmv_c_csr* A_local, float* d_col_sums, void* hip_stream);
int spmv_c_pr_mask_from_column_sums(const float* d_col_sums, int n, uint8_t* d_mask,
                                    uint64_t* d_count, void* hip_stream);
int spmv_c_fill(float* d_r, size_t n, float value, void* hip_stream);

/* ---- synthetic inputs generated in HBM (extension; numpy twin: gpu-spmv_amd/synth.py) ---- */
int spmv_c_gen_uniform_rows(uint64_t seed, int row_begin, int local_rows, int n_cols, int k,
                            int32_t* d_row_ptrs, int32_t* d_cols, float* d_vals, void* hip_stream);
/* the same entries as gen_uniform_rows(row_begin = 0), stored column-major (ELL, K = k, no padding) */
int spmv_c_gen_uniform_ell(uint64_t seed, int rows, int n_cols, int k, int32_t* d_cols, float* d_vals,
                           void* hip_stream);
int spmv_c_gen_stratified_rows(uint64_t seed, int row_begin, int local_rows, int n_cols,
                               const int32_t* d_row_ptrs, int32_t* d_cols, float* d_vals,
                               void* hip_stream);
int spmv_c_gen_vector(uint64_t seed, uint64_t tag, size_t n, float* d_x, void* hip_stream);
int spmv_c_count_columns(int64_t nnz, const int32_t* d_cols, int n_cols, int32_t* d_counts,
                         void* hip_stream);
int spmv_c_reciprocal_values(int64_t nnz, const int32_t* d_cols, const int32_t* d_counts,
                             float* d_vals, void* hip_stream);

#ifdef __cplusplus
}
#endif

#endif /* SPMV_C_H */
