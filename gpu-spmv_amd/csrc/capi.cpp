// capi.cpp — the extern "C" boundary declared in include/spmv_c.h: thin shims
// over the C++ API in namespace spmv (same struct layouts, checked below).
#include "internal.h"
#include "generators.h"
#include "pagerank_engine.h"
#include "tiled.h"
#include "spmv/bandwidth.h"
#include "spmv/bicgstab.h"
#include "spmv/gmres.h"
#include "spmv/minres.h"
#include "spmv/eigs.h"
#include "spmv/cg.h"
#include "spmv/pagerank.h"
#include "spmv/sptrsv.h"
#include "spmv/ic0.h"
#include "spmv/fsai.h"
#include "spmv/ilu0.h"
#include "spmv/spgemm.h"
#include "spmv/amg.h"
#include "spmv/reorder.h"
#include "spmv/assemble.h"
#include "spmv/csr_ops.h"
#include "spmv/bsr.h"
#include "spmv/bsr_factor.h"
#include "spmv_c.h"

#include <cstddef>
#include <cstring>
#include <vector>
#include <new>

using namespace spmv;

// ---- layout contracts: a C struct and its C++ twin must be byte-identical ----
static_assert(sizeof(spmv_c_csr) == sizeof(CSRMatrix) && sizeof(CSRMatrix) == 72, "CSRMatrix layout");
static_assert(offsetof(spmv_c_csr, d_values) == offsetof(CSRMatrix, d_values), "CSRMatrix layout");
static_assert(offsetof(spmv_c_csr, owns_host_memory) == offsetof(CSRMatrix, owns_host_memory), "CSRMatrix layout");
static_assert(offsetof(spmv_c_csr, owns_device_memory) == offsetof(CSRMatrix, owns_device_memory), "CSRMatrix layout");
static_assert(sizeof(spmv_c_ell) == sizeof(ELLMatrix) && sizeof(ELLMatrix) == 56, "ELLMatrix layout");
static_assert(sizeof(spmv_c_bsr) == sizeof(BSRMatrix) && sizeof(BSRMatrix) == 80, "BSRMatrix layout");
static_assert(offsetof(spmv_c_bsr, num_blocks) == offsetof(BSRMatrix, num_blocks) &&
              offsetof(spmv_c_bsr, values) == offsetof(BSRMatrix, values) &&
              offsetof(spmv_c_bsr, block_row_ptrs) == offsetof(BSRMatrix, block_row_ptrs) &&
              offsetof(spmv_c_bsr, d_values) == offsetof(BSRMatrix, d_values) &&
              offsetof(spmv_c_bsr, d_block_row_ptrs) == offsetof(BSRMatrix, d_block_row_ptrs) &&
              offsetof(spmv_c_bsr, owns_host_memory) == offsetof(BSRMatrix, owns_host_memory) &&
              offsetof(spmv_c_bsr, owns_device_memory) == offsetof(BSRMatrix, owns_device_memory), "BSRMatrix layout");
static_assert(sizeof(spmv_c_bsr_build_result) == sizeof(BsrBuildResult) && sizeof(BsrBuildResult) == 32, "BsrBuildResult layout");
static_assert(offsetof(spmv_c_bsr_build_result, error_code) == offsetof(BsrBuildResult, error_code) &&
              offsetof(spmv_c_bsr_build_result, num_blocks) == offsetof(BsrBuildResult, num_blocks) &&
              offsetof(spmv_c_bsr_build_result, fill) == offsetof(BsrBuildResult, fill) &&
              offsetof(spmv_c_bsr_build_result, max_block_row) == offsetof(BsrBuildResult, max_block_row) &&
              offsetof(spmv_c_bsr_build_result, lanes) == offsetof(BsrBuildResult, lanes) &&
              offsetof(spmv_c_bsr_build_result, launches) == offsetof(BsrBuildResult, launches) &&
              offsetof(spmv_c_bsr_build_result, symbolic_ms) == offsetof(BsrBuildResult, symbolic_ms) &&
              offsetof(spmv_c_bsr_build_result, numeric_ms) == offsetof(BsrBuildResult, numeric_ms), "BsrBuildResult layout");
static_assert(offsetof(spmv_c_ell, d_col_indices) == offsetof(ELLMatrix, d_col_indices), "ELLMatrix layout");
static_assert(offsetof(spmv_c_ell, owns_host_memory) == offsetof(ELLMatrix, owns_host_memory), "ELLMatrix layout");
static_assert(sizeof(spmv_c_config) == sizeof(SpMVConfig) && sizeof(SpMVConfig) == 12, "SpMVConfig layout");
static_assert(offsetof(spmv_c_config, use_texture) == offsetof(SpMVConfig, use_texture), "SpMVConfig layout");
static_assert(sizeof(spmv_c_result) == sizeof(SpMVResult) && sizeof(SpMVResult) == 24, "SpMVResult layout");
static_assert(sizeof(spmv_c_csr_stats) == sizeof(CSRStats) && sizeof(CSRStats) == 16, "CSRStats layout");
static_assert(sizeof(spmv_c_bandwidth) == sizeof(BandwidthMetrics) && sizeof(BandwidthMetrics) == 12, "BandwidthMetrics layout");
static_assert(sizeof(spmv_c_pagerank_config) == sizeof(PageRankConfig) && sizeof(PageRankConfig) == 12, "PageRankConfig layout");
static_assert(sizeof(spmv_c_pagerank_result) == sizeof(PageRankResult) && sizeof(PageRankResult) == 24, "PageRankResult layout");
static_assert(offsetof(spmv_c_pagerank_result, converged) == offsetof(PageRankResult, converged), "PageRankResult layout");
static_assert(sizeof(spmv_c_topk_node) == sizeof(TopKNode) && sizeof(TopKNode) == 8, "TopKNode layout");
static_assert(sizeof(spmv_c_pr_status) == sizeof(detail::PrState), "PrState layout");
static_assert(sizeof(spmv_c_cg_config) == sizeof(CGConfig) && sizeof(CGConfig) == 16, "CGConfig layout");
static_assert(offsetof(spmv_c_cg_config, max_iterations) == offsetof(CGConfig, max_iterations) &&
              offsetof(spmv_c_cg_config, preconditioner) == offsetof(CGConfig, preconditioner) &&
              offsetof(spmv_c_cg_config, engine) == offsetof(CGConfig, engine), "CGConfig layout");
static_assert(sizeof(spmv_c_personalized_result) == sizeof(PersonalizedResult) && sizeof(PersonalizedResult) == 20,
              "PersonalizedResult layout");
static_assert(offsetof(spmv_c_personalized_result, iterations) == offsetof(PersonalizedResult, iterations) &&
              offsetof(spmv_c_personalized_result, final_residual) == offsetof(PersonalizedResult, final_residual) &&
              offsetof(spmv_c_personalized_result, converged) == offsetof(PersonalizedResult, converged) &&
              offsetof(spmv_c_personalized_result, elapsed_ms) == offsetof(PersonalizedResult, elapsed_ms),
              "PersonalizedResult layout");
static_assert(sizeof(spmv_c_cg_result) == sizeof(CGResult) && sizeof(CGResult) == 24, "CGResult layout");
static_assert(offsetof(spmv_c_cg_result, iterations) == offsetof(CGResult, iterations) &&
              offsetof(spmv_c_cg_result, relative_residual) == offsetof(CGResult, relative_residual) &&
              offsetof(spmv_c_cg_result, converged) == offsetof(CGResult, converged) &&
              offsetof(spmv_c_cg_result, breakdown) == offsetof(CGResult, breakdown) &&
              offsetof(spmv_c_cg_result, elapsed_ms) == offsetof(CGResult, elapsed_ms), "CGResult layout");
static_assert(sizeof(spmv_c_gmres_config) == sizeof(GMRESConfig) && sizeof(GMRESConfig) == 20, "GMRESConfig layout");
static_assert(offsetof(spmv_c_gmres_config, max_iterations) == offsetof(GMRESConfig, max_iterations) &&
              offsetof(spmv_c_gmres_config, restart) == offsetof(GMRESConfig, restart) &&
              offsetof(spmv_c_gmres_config, preconditioner) == offsetof(GMRESConfig, preconditioner) &&
              offsetof(spmv_c_gmres_config, engine) == offsetof(GMRESConfig, engine), "GMRESConfig layout");
static_assert(sizeof(spmv_c_gmres_result) == sizeof(GMRESResult) && sizeof(GMRESResult) == 28, "GMRESResult layout");
static_assert(offsetof(spmv_c_gmres_result, iterations) == offsetof(GMRESResult, iterations) &&
              offsetof(spmv_c_gmres_result, restarts) == offsetof(GMRESResult, restarts) &&
              offsetof(spmv_c_gmres_result, relative_residual) == offsetof(GMRESResult, relative_residual) &&
              offsetof(spmv_c_gmres_result, converged) == offsetof(GMRESResult, converged) &&
              offsetof(spmv_c_gmres_result, breakdown) == offsetof(GMRESResult, breakdown) &&
              offsetof(spmv_c_gmres_result, elapsed_ms) == offsetof(GMRESResult, elapsed_ms), "GMRESResult layout");
static_assert(sizeof(spmv_c_minres_config) == sizeof(MinresConfig) && sizeof(MinresConfig) == 20,
              "MinresConfig layout");
static_assert(offsetof(spmv_c_minres_config, max_iterations) == offsetof(MinresConfig, max_iterations) &&
              offsetof(spmv_c_minres_config, preconditioner) == offsetof(MinresConfig, preconditioner) &&
              offsetof(spmv_c_minres_config, engine) == offsetof(MinresConfig, engine) &&
              offsetof(spmv_c_minres_config, shift) == offsetof(MinresConfig, shift), "MinresConfig layout");
static_assert(sizeof(spmv_c_minres_result) == sizeof(MinresResult) && sizeof(MinresResult) == 28,
              "MinresResult layout");
static_assert(offsetof(spmv_c_minres_result, iterations) == offsetof(MinresResult, iterations) &&
              offsetof(spmv_c_minres_result, relative_residual) == offsetof(MinresResult, relative_residual) &&
              offsetof(spmv_c_minres_result, true_relative_residual) ==
                  offsetof(MinresResult, true_relative_residual) &&
              offsetof(spmv_c_minres_result, converged) == offsetof(MinresResult, converged) &&
              offsetof(spmv_c_minres_result, breakdown) == offsetof(MinresResult, breakdown) &&
              offsetof(spmv_c_minres_result, elapsed_ms) == offsetof(MinresResult, elapsed_ms), "MinresResult layout");
static_assert(sizeof(spmv_c_eigs_config) == sizeof(EigsConfig) && sizeof(EigsConfig) == 24, "EigsConfig layout");
static_assert(offsetof(spmv_c_eigs_config, which) == offsetof(EigsConfig, which) &&
              offsetof(spmv_c_eigs_config, basis) == offsetof(EigsConfig, basis) &&
              offsetof(spmv_c_eigs_config, tolerance) == offsetof(EigsConfig, tolerance) &&
              offsetof(spmv_c_eigs_config, max_iterations) == offsetof(EigsConfig, max_iterations) &&
              offsetof(spmv_c_eigs_config, engine) == offsetof(EigsConfig, engine), "EigsConfig layout");
static_assert(sizeof(spmv_c_eigs_result) == sizeof(EigsResult) && sizeof(EigsResult) == 28, "EigsResult layout");
static_assert(offsetof(spmv_c_eigs_result, iterations) == offsetof(EigsResult, iterations) &&
              offsetof(spmv_c_eigs_result, restarts) == offsetof(EigsResult, restarts) &&
              offsetof(spmv_c_eigs_result, converged) == offsetof(EigsResult, converged) &&
              offsetof(spmv_c_eigs_result, breakdown) == offsetof(EigsResult, breakdown) &&
              offsetof(spmv_c_eigs_result, max_residual) == offsetof(EigsResult, max_residual) &&
              offsetof(spmv_c_eigs_result, elapsed_ms) == offsetof(EigsResult, elapsed_ms), "EigsResult layout");
static_assert(sizeof(spmv_c_bicgstab_config) == sizeof(BiCGStabConfig) && sizeof(BiCGStabConfig) == 16,
              "BiCGStabConfig layout");
static_assert(offsetof(spmv_c_bicgstab_config, max_iterations) == offsetof(BiCGStabConfig, max_iterations) &&
              offsetof(spmv_c_bicgstab_config, preconditioner) == offsetof(BiCGStabConfig, preconditioner) &&
              offsetof(spmv_c_bicgstab_config, engine) == offsetof(BiCGStabConfig, engine), "BiCGStabConfig layout");
static_assert(sizeof(spmv_c_bicgstab_result) == sizeof(BiCGStabResult) && sizeof(BiCGStabResult) == 24,
              "BiCGStabResult layout");
static_assert(offsetof(spmv_c_bicgstab_result, iterations) == offsetof(BiCGStabResult, iterations) &&
              offsetof(spmv_c_bicgstab_result, relative_residual) == offsetof(BiCGStabResult, relative_residual) &&
              offsetof(spmv_c_bicgstab_result, converged) == offsetof(BiCGStabResult, converged) &&
              offsetof(spmv_c_bicgstab_result, breakdown) == offsetof(BiCGStabResult, breakdown) &&
              offsetof(spmv_c_bicgstab_result, elapsed_ms) == offsetof(BiCGStabResult, elapsed_ms),
              "BiCGStabResult layout");
static_assert(sizeof(spmv_c_sptrsv_config) == sizeof(SpTRSVConfig) && sizeof(SpTRSVConfig) == 16, "SpTRSVConfig layout");
static_assert(offsetof(spmv_c_sptrsv_config, diag) == offsetof(SpTRSVConfig, diag) &&
              offsetof(spmv_c_sptrsv_config, ordered) == offsetof(SpTRSVConfig, ordered) &&
              offsetof(spmv_c_sptrsv_config, reserved) == offsetof(SpTRSVConfig, reserved), "SpTRSVConfig layout");
static_assert(sizeof(spmv_c_sptrsv_result) == sizeof(SpTRSVResult) && sizeof(SpTRSVResult) == 24, "SpTRSVResult layout");
static_assert(sizeof(spmv_c_sptrsv_schedule_info) == sizeof(SpTRSVScheduleInfo) && sizeof(SpTRSVScheduleInfo) == 32,
              "SpTRSVScheduleInfo layout");
static_assert(offsetof(spmv_c_sptrsv_schedule_info, launches) == offsetof(SpTRSVScheduleInfo, launches) &&
              offsetof(spmv_c_sptrsv_schedule_info, first_missing_diagonal) ==
                  offsetof(SpTRSVScheduleInfo, first_missing_diagonal) &&
              offsetof(spmv_c_sptrsv_schedule_info, first_unsorted_row) ==
                  offsetof(SpTRSVScheduleInfo, first_unsorted_row) &&
              offsetof(spmv_c_sptrsv_schedule_info, one_sided_row) == offsetof(SpTRSVScheduleInfo, one_sided_row) &&
              offsetof(spmv_c_sptrsv_schedule_info, built_on_device) == offsetof(SpTRSVScheduleInfo, built_on_device) &&
              offsetof(spmv_c_sptrsv_schedule_info, triangle_nnz) == offsetof(SpTRSVScheduleInfo, triangle_nnz) &&
              offsetof(SpTRSVScheduleInfo, triangle_nnz) == 24, "SpTRSVScheduleInfo layout");
static_assert(sizeof(spmv_c_ilu0_result) == sizeof(ILU0Result) && sizeof(ILU0Result) == 28, "ILU0Result layout");
static_assert(offsetof(spmv_c_ilu0_result, num_levels) == offsetof(ILU0Result, num_levels) &&
              offsetof(spmv_c_ilu0_result, launches) == offsetof(ILU0Result, launches) &&
              offsetof(spmv_c_ilu0_result, lanes_per_row) == offsetof(ILU0Result, lanes_per_row) &&
              offsetof(spmv_c_ilu0_result, zero_pivot) == offsetof(ILU0Result, zero_pivot) &&
              offsetof(spmv_c_ilu0_result, analysis_ms) == offsetof(ILU0Result, analysis_ms) &&
              offsetof(spmv_c_ilu0_result, elapsed_ms) == offsetof(ILU0Result, elapsed_ms), "ILU0Result layout");
static_assert(sizeof(spmv_c_ic0_result) == sizeof(IC0Result) && sizeof(IC0Result) == 28, "IC0Result layout");
static_assert(offsetof(spmv_c_ic0_result, num_levels) == offsetof(IC0Result, num_levels) &&
              offsetof(spmv_c_ic0_result, launches) == offsetof(IC0Result, launches) &&
              offsetof(spmv_c_ic0_result, lanes_per_row) == offsetof(IC0Result, lanes_per_row) &&
              offsetof(spmv_c_ic0_result, bad_pivot) == offsetof(IC0Result, bad_pivot) &&
              offsetof(spmv_c_ic0_result, analysis_ms) == offsetof(IC0Result, analysis_ms) &&
              offsetof(spmv_c_ic0_result, elapsed_ms) == offsetof(IC0Result, elapsed_ms), "IC0Result layout");
static_assert(sizeof(BsrIC0Result) == sizeof(IC0Result) && offsetof(BsrIC0Result, bad_pivot) == offsetof(IC0Result, bad_pivot) &&
              offsetof(BsrIC0Result, analysis_ms) == offsetof(IC0Result, analysis_ms) &&
              offsetof(BsrIC0Result, elapsed_ms) == offsetof(IC0Result, elapsed_ms), "BsrIC0Result layout");
static_assert(sizeof(spmv_c_fsai_result) == sizeof(FSAIResult) && sizeof(FSAIResult) == 32, "FSAIResult layout");
static_assert(offsetof(spmv_c_fsai_result, nnz) == offsetof(FSAIResult, nnz) &&
              offsetof(spmv_c_fsai_result, max_row) == offsetof(FSAIResult, max_row) &&
              offsetof(spmv_c_fsai_result, row_class) == offsetof(FSAIResult, row_class) &&
              offsetof(spmv_c_fsai_result, lanes_per_row) == offsetof(FSAIResult, lanes_per_row) &&
              offsetof(spmv_c_fsai_result, bad_row) == offsetof(FSAIResult, bad_row) &&
              offsetof(spmv_c_fsai_result, long_row) == offsetof(FSAIResult, long_row) &&
              offsetof(spmv_c_fsai_result, elapsed_ms) == offsetof(FSAIResult, elapsed_ms), "FSAIResult layout");
static_assert(offsetof(spmv_c_sptrsv_result, num_levels) == offsetof(SpTRSVResult, num_levels) &&
              offsetof(spmv_c_sptrsv_result, launches) == offsetof(SpTRSVResult, launches) &&
              offsetof(spmv_c_sptrsv_result, lanes_per_row) == offsetof(SpTRSVResult, lanes_per_row) &&
              offsetof(spmv_c_sptrsv_result, analysis_ms) == offsetof(SpTRSVResult, analysis_ms) &&
              offsetof(spmv_c_sptrsv_result, elapsed_ms) == offsetof(SpTRSVResult, elapsed_ms), "SpTRSVResult layout");

static_assert(sizeof(spmv_c_coo_config) == sizeof(CooConfig) && sizeof(CooConfig) == 8, "CooConfig layout");
static_assert(offsetof(spmv_c_coo_config, reserved) == offsetof(CooConfig, reserved), "CooConfig layout");
static_assert(sizeof(spmv_c_coo_result) == sizeof(CooResult) && sizeof(CooResult) == 28, "CooResult layout");
static_assert(offsetof(spmv_c_coo_result, nnz_out) == offsetof(CooResult, nnz_out) &&
              offsetof(spmv_c_coo_result, tile_entries) == offsetof(CooResult, tile_entries) &&
              offsetof(spmv_c_coo_result, elapsed_ms) == offsetof(CooResult, elapsed_ms), "CooResult layout");
static_assert(sizeof(spmv_c_csr_add_result) == sizeof(CsrAddResult) && sizeof(CsrAddResult) == 32, "CsrAddResult layout");
static_assert(offsetof(spmv_c_csr_add_result, error_code) == offsetof(CsrAddResult, error_code) &&
              offsetof(spmv_c_csr_add_result, nnz) == offsetof(CsrAddResult, nnz) &&
              offsetof(spmv_c_csr_add_result, common) == offsetof(CsrAddResult, common) &&
              offsetof(spmv_c_csr_add_result, max_row_nnz) == offsetof(CsrAddResult, max_row_nnz) &&
              offsetof(spmv_c_csr_add_result, lanes) == offsetof(CsrAddResult, lanes) &&
              offsetof(spmv_c_csr_add_result, launches) == offsetof(CsrAddResult, launches) &&
              offsetof(spmv_c_csr_add_result, symbolic_ms) == offsetof(CsrAddResult, symbolic_ms) &&
              offsetof(spmv_c_csr_add_result, numeric_ms) == offsetof(CsrAddResult, numeric_ms), "CsrAddResult layout");
static_assert(sizeof(spmv_c_color_config) == sizeof(ColorConfig) && sizeof(ColorConfig) == 16, "ColorConfig layout");
static_assert(offsetof(spmv_c_color_config, symmetric_pattern) == offsetof(ColorConfig, symmetric_pattern) &&
              offsetof(spmv_c_color_config, lanes_per_row) == offsetof(ColorConfig, lanes_per_row) &&
              offsetof(spmv_c_color_config, reserved) == offsetof(ColorConfig, reserved), "ColorConfig layout");
static_assert(sizeof(spmv_c_rcm_config) == sizeof(RcmConfig) && sizeof(RcmConfig) == 16, "RcmConfig layout");
static_assert(offsetof(spmv_c_rcm_config, peripheral) == offsetof(RcmConfig, peripheral) &&
              offsetof(spmv_c_rcm_config, lanes_per_row) == offsetof(RcmConfig, lanes_per_row) &&
              offsetof(spmv_c_rcm_config, reserved) == offsetof(RcmConfig, reserved), "RcmConfig layout");
static_assert(sizeof(spmv_c_rcm_result) == sizeof(RcmResult) && sizeof(RcmResult) == 24, "RcmResult layout");
static_assert(offsetof(spmv_c_rcm_result, components) == offsetof(RcmResult, components) &&
              offsetof(spmv_c_rcm_result, levels) == offsetof(RcmResult, levels) &&
              offsetof(spmv_c_rcm_result, sweeps) == offsetof(RcmResult, sweeps) &&
              offsetof(spmv_c_rcm_result, launches) == offsetof(RcmResult, launches) &&
              offsetof(spmv_c_rcm_result, elapsed_ms) == offsetof(RcmResult, elapsed_ms), "RcmResult layout");
static_assert(sizeof(spmv_c_csr_band) == sizeof(CsrBand) && sizeof(CsrBand) == 16 &&
              offsetof(spmv_c_csr_band, upper) == offsetof(CsrBand, upper) &&
              offsetof(spmv_c_csr_band, profile) == offsetof(CsrBand, profile), "CsrBand layout");
static_assert(sizeof(spmv_c_color_result) == sizeof(ColorResult) && sizeof(ColorResult) == 20, "ColorResult layout");
static_assert(offsetof(spmv_c_color_result, num_colors) == offsetof(ColorResult, num_colors) &&
              offsetof(spmv_c_color_result, rounds) == offsetof(ColorResult, rounds) &&
              offsetof(spmv_c_color_result, launches) == offsetof(ColorResult, launches) &&
              offsetof(spmv_c_color_result, elapsed_ms) == offsetof(ColorResult, elapsed_ms), "ColorResult layout");

static_assert(sizeof(spmv_c_spgemm_result) == sizeof(SpGEMMResult) && sizeof(SpGEMMResult) == 104, "SpGEMMResult layout");
static_assert(offsetof(spmv_c_spgemm_result, nnz) == offsetof(SpGEMMResult, nnz) &&
              offsetof(spmv_c_spgemm_result, products) == offsetof(SpGEMMResult, products) &&
              offsetof(spmv_c_spgemm_result, max_row_products) == offsetof(SpGEMMResult, max_row_products) &&
              offsetof(spmv_c_spgemm_result, max_row_nnz) == offsetof(SpGEMMResult, max_row_nnz) &&
              offsetof(spmv_c_spgemm_result, symbolic_rows) == offsetof(SpGEMMResult, symbolic_rows) &&
              offsetof(spmv_c_spgemm_result, numeric_rows) == offsetof(SpGEMMResult, numeric_rows) &&
              offsetof(spmv_c_spgemm_result, lanes) == offsetof(SpGEMMResult, lanes) &&
              offsetof(spmv_c_spgemm_result, symbolic_ms) == offsetof(SpGEMMResult, symbolic_ms) &&
              offsetof(spmv_c_spgemm_result, numeric_ms) == offsetof(SpGEMMResult, numeric_ms), "SpGEMMResult layout");

static_assert(sizeof(spmv_c_amg_config) == sizeof(AMGConfig) && sizeof(AMGConfig) == 28, "AMGConfig layout");
static_assert(offsetof(spmv_c_amg_config, strength) == offsetof(AMGConfig, strength) &&
              offsetof(spmv_c_amg_config, post_sweeps) == offsetof(AMGConfig, post_sweeps) &&
              offsetof(spmv_c_amg_config, jacobi_weight) == offsetof(AMGConfig, jacobi_weight) &&
              offsetof(spmv_c_amg_config, coarse_sweeps) == offsetof(AMGConfig, coarse_sweeps), "AMGConfig layout");
static_assert(sizeof(spmv_c_amg_smoothing) == sizeof(AMGSmoothing) && sizeof(AMGSmoothing) == 8 &&
              offsetof(spmv_c_amg_smoothing, strength_decay) == offsetof(AMGSmoothing, strength_decay),
              "AMGSmoothing layout");
static_assert(sizeof(spmv_c_amg_result) == sizeof(AMGResult) && sizeof(AMGResult) == 48, "AMGResult layout");
static_assert(offsetof(spmv_c_amg_result, bad_level) == offsetof(AMGResult, bad_level) &&
              offsetof(spmv_c_amg_result, grid_complexity) == offsetof(AMGResult, grid_complexity) &&
              offsetof(spmv_c_amg_result, operator_complexity) == offsetof(AMGResult, operator_complexity) &&
              offsetof(spmv_c_amg_result, setup_ms) == offsetof(AMGResult, setup_ms), "AMGResult layout");

namespace {

inline AMGHierarchy* cxx(spmv_c_amg* h) { return reinterpret_cast<AMGHierarchy*>(h); }
inline const AMGHierarchy* cxx(const spmv_c_amg* h) { return reinterpret_cast<const AMGHierarchy*>(h); }
inline CSRMatrix* cxx(spmv_c_csr* m) { return reinterpret_cast<CSRMatrix*>(m); }
inline const CSRMatrix* cxx(const spmv_c_csr* m) { return reinterpret_cast<const CSRMatrix*>(m); }
inline BSRMatrix* cxx(spmv_c_bsr* m) { return reinterpret_cast<BSRMatrix*>(m); }
inline const BSRMatrix* cxx(const spmv_c_bsr* m) { return reinterpret_cast<const BSRMatrix*>(m); }
inline ELLMatrix* cxx(spmv_c_ell* m) { return reinterpret_cast<ELLMatrix*>(m); }
inline const ELLMatrix* cxx(const spmv_c_ell* m) { return reinterpret_cast<const ELLMatrix*>(m); }
inline const SpMVConfig* cxx(const spmv_c_config* c) { return reinterpret_cast<const SpMVConfig*>(c); }
inline hipStream_t as_stream(void* s) { return static_cast<hipStream_t>(s); }

constexpr int kInvalidArgument = static_cast<int>(SpMVError::INVALID_ARGUMENT);
constexpr int kLaunch = static_cast<int>(SpMVError::KERNEL_LAUNCH);

inline int launch_code(hipError_t e) { return e == hipSuccess ? 0 : kLaunch; }

} // namespace

struct spmv_c_pr_shard {
    detail::PrShard shard;
};

extern "C" {

const char* spmv_c_error_string(int code) {
    return spmv_error_string(static_cast<SpMVError>(code));
}

const char* spmv_c_version(void) { return "spmv-amd 0.1 (gfx950)"; }

int spmv_c_device_count(void) {
    int n = 0;
    if (hipGetDeviceCount(&n) != hipSuccess) {
        (void)hipGetLastError();
        return 0;
    }
    return n;
}

int spmv_c_device_name(char* buf, size_t buf_len) {
    if (!buf || buf_len == 0) return kInvalidArgument;
    int dev = 0;
    hipDeviceProp_t prop;
    if (hipGetDevice(&dev) != hipSuccess || hipGetDeviceProperties(&prop, dev) != hipSuccess) {
        buf[0] = '\0';
        return kLaunch;
    }
    std::strncpy(buf, prop.gcnArchName, buf_len - 1);
    buf[buf_len - 1] = '\0';
    return 0;
}

int spmv_c_set_device(int ordinal) { return launch_code(hipSetDevice(ordinal)); }

int spmv_c_enable_peer_access(int peer_ordinal) {
    int current = 0;
    if (hipGetDevice(&current) != hipSuccess) return kLaunch;
    if (current == peer_ordinal) return 0;
    int can = 0;
    if (hipDeviceCanAccessPeer(&can, current, peer_ordinal) != hipSuccess || !can) {
        (void)hipGetLastError();
        return kInvalidArgument;
    }
    const hipError_t e = hipDeviceEnablePeerAccess(peer_ordinal, 0);
    if (e == hipSuccess || e == hipErrorPeerAccessAlreadyEnabled) {
        (void)hipGetLastError();
        return 0;
    }
    return kLaunch;
}

void spmv_c_set_stream(void* hip_stream) { spmv_set_stream(as_stream(hip_stream)); }

int spmv_c_device_malloc(void** d_ptr, size_t bytes) {
    if (!d_ptr) return kInvalidArgument;
    *d_ptr = nullptr;
    if (bytes == 0) return 0;
    return hipMalloc(d_ptr, bytes) == hipSuccess ? 0 : static_cast<int>(SpMVError::CUDA_MALLOC);
}

int spmv_c_device_free(void* d_ptr) {
    if (!d_ptr) return 0;
    return hipFree(d_ptr) == hipSuccess ? 0 : static_cast<int>(SpMVError::CUDA_MALLOC);
}

int spmv_c_memcpy_h2d(void* d_dst, const void* src, size_t bytes) {
    if (bytes == 0) return 0;
    if (!d_dst || !src) return kInvalidArgument;
    return hipMemcpy(d_dst, src, bytes, hipMemcpyHostToDevice) == hipSuccess
         ? 0 : static_cast<int>(SpMVError::CUDA_MEMCPY);
}

int spmv_c_memcpy_d2h(void* dst, const void* d_src, size_t bytes) {
    if (bytes == 0) return 0;
    if (!dst || !d_src) return kInvalidArgument;
    return hipMemcpy(dst, d_src, bytes, hipMemcpyDeviceToHost) == hipSuccess
         ? 0 : static_cast<int>(SpMVError::CUDA_MEMCPY);
}

int spmv_c_device_synchronize(void) { return launch_code(hipDeviceSynchronize()); }

static_assert(sizeof(hipIpcMemHandle_t) == 64, "IPC handle size");

int spmv_c_ipc_get_handle(void* d_ptr, unsigned char handle_out[64]) {
    if (!d_ptr || !handle_out) return kInvalidArgument;
    hipIpcMemHandle_t h;
    if (hipIpcGetMemHandle(&h, d_ptr) != hipSuccess) {
        (void)hipGetLastError();
        return kLaunch;
    }
    std::memcpy(handle_out, &h, sizeof(h));
    return 0;
}

int spmv_c_ipc_open_handle(const unsigned char handle[64], void** d_ptr_out) {
    if (!handle || !d_ptr_out) return kInvalidArgument;
    hipIpcMemHandle_t h;
    std::memcpy(&h, handle, sizeof(h));
    *d_ptr_out = nullptr;
    if (hipIpcOpenMemHandle(d_ptr_out, h, hipIpcMemLazyEnablePeerAccess) != hipSuccess) {
        (void)hipGetLastError();
        *d_ptr_out = nullptr;
        return kLaunch;
    }
    return 0;
}

int spmv_c_ipc_close(void* d_ptr) {
    if (!d_ptr) return 0;
    return launch_code(hipIpcCloseMemHandle(d_ptr));
}

// ---- CSR ----
spmv_c_csr* spmv_c_csr_create(int rows, int cols, int nnz) {
    return reinterpret_cast<spmv_c_csr*>(csr_create(rows, cols, nnz));
}
void spmv_c_csr_destroy(spmv_c_csr* mat) { csr_destroy(cxx(mat)); }
int spmv_c_csr_from_dense(spmv_c_csr* csr, const float* dense, int rows, int cols) {
    return csr_from_dense(cxx(csr), dense, rows, cols);
}
int spmv_c_csr_to_dense(const spmv_c_csr* csr, float* dense) { return csr_to_dense(cxx(csr), dense); }
float spmv_c_csr_get_element(const spmv_c_csr* mat, int row, int col) {
    return csr_get_element(cxx(mat), row, col);
}
int spmv_c_csr_to_gpu(spmv_c_csr* mat) { return csr_to_gpu(cxx(mat)); }
int spmv_c_csr_from_gpu(spmv_c_csr* mat) { return csr_from_gpu(cxx(mat)); }
void spmv_c_csr_free_gpu(spmv_c_csr* mat) { csr_free_gpu(cxx(mat)); }
void spmv_c_csr_invalidate_gpu_cache(const spmv_c_csr* mat) { csr_invalidate_gpu_cache(cxx(mat)); }
int spmv_c_csr_serialize(const spmv_c_csr* mat, const char* filename) {
    return csr_serialize(cxx(mat), filename);
}
int spmv_c_csr_deserialize(spmv_c_csr* mat, const char* filename) {
    return csr_deserialize(cxx(mat), filename);
}
int spmv_c_csr_compute_stats(const spmv_c_csr* mat, spmv_c_csr_stats* out) {
    if (!out) return kInvalidArgument;
    const CSRStats s = csr_compute_stats(cxx(mat));
    std::memcpy(out, &s, sizeof(s));
    return 0;
}

spmv_c_csr* spmv_c_csr_wrap_device(int rows, int cols, int nnz, const int32_t* d_row_ptrs,
                                   const int32_t* d_col_indices, const float* d_values) {
    if (rows < 0 || cols < 0 || nnz < 0) return nullptr;
    CSRMatrix* m = new (std::nothrow) CSRMatrix{};
    if (!m) return nullptr;
    m->num_rows = rows;
    m->num_cols = cols;
    m->nnz = nnz;
    m->d_row_ptrs = const_cast<int*>(d_row_ptrs);
    m->d_col_indices = const_cast<int*>(d_col_indices);
    m->d_values = const_cast<float*>(d_values);
    m->owns_host_memory = false;
    m->owns_device_memory = false;
    return reinterpret_cast<spmv_c_csr*>(m);
}

// ---- ELL ----
spmv_c_ell* spmv_c_ell_create(int rows, int cols, int k) {
    return reinterpret_cast<spmv_c_ell*>(ell_create(rows, cols, k));
}
void spmv_c_ell_destroy(spmv_c_ell* mat) { ell_destroy(cxx(mat)); }
int spmv_c_ell_from_dense(spmv_c_ell* ell, const float* dense, int rows, int cols) {
    return ell_from_dense(cxx(ell), dense, rows, cols);
}
int spmv_c_ell_from_csr(spmv_c_ell* ell, const spmv_c_csr* csr) { return ell_from_csr(cxx(ell), cxx(csr)); }
int spmv_c_ell_from_csr_gpu(spmv_c_ell* ell, const spmv_c_csr* csr) { return ell_from_csr_gpu(cxx(ell), cxx(csr)); }
int spmv_c_csr_transpose_gpu(spmv_c_csr* AT, const spmv_c_csr* A) { return csr_transpose_gpu(cxx(AT), cxx(A)); }
int spmv_c_ell_to_dense(const spmv_c_ell* ell, float* dense) { return ell_to_dense(cxx(ell), dense); }
float spmv_c_ell_get_element(const spmv_c_ell* mat, int row, int col) {
    return ell_get_element(cxx(mat), row, col);
}
int spmv_c_ell_to_gpu(spmv_c_ell* mat) { return ell_to_gpu(cxx(mat)); }
int spmv_c_ell_from_gpu(spmv_c_ell* mat) { return ell_from_gpu(cxx(mat)); }
void spmv_c_ell_free_gpu(spmv_c_ell* mat) { ell_free_gpu(cxx(mat)); }
void spmv_c_ell_invalidate_gpu_cache(const spmv_c_ell* mat) { ell_invalidate_gpu_cache(cxx(mat)); }
int spmv_c_ell_serialize(const spmv_c_ell* mat, const char* filename) {
    return ell_serialize(cxx(mat), filename);
}
int spmv_c_ell_deserialize(spmv_c_ell* mat, const char* filename) {
    return ell_deserialize(cxx(mat), filename);
}
int spmv_c_ell_index(int row, int k, int num_rows) { return ell_index(row, k, num_rows); }

spmv_c_ell* spmv_c_ell_wrap_device(int rows, int cols, int k, const int32_t* d_col_indices,
                                   const float* d_values) {
    if (rows < 0 || cols < 0 || k < 0) return nullptr;
    ELLMatrix* m = new (std::nothrow) ELLMatrix{};
    if (!m) return nullptr;
    m->num_rows = rows;
    m->num_cols = cols;
    m->max_nnz_per_row = k;
    m->d_col_indices = const_cast<int*>(d_col_indices);
    m->d_values = const_cast<float*>(d_values);
    m->owns_host_memory = false;
    m->owns_device_memory = false;
    return reinterpret_cast<spmv_c_ell*>(m);
}

// ---- SpMV ----
void spmv_c_cpu_csr(const spmv_c_csr* A, const float* x, float* y) { spmv_cpu_csr(cxx(A), x, y); }
void spmv_c_cpu_ell(const spmv_c_ell* A, const float* x, float* y) { spmv_cpu_ell(cxx(A), x, y); }

int spmv_c_spmv_csr(const spmv_c_csr* A, const float* d_x, float* d_y,
                    const spmv_c_config* config, int vec_size, spmv_c_result* out) {
    const SpMVResult r = spmv_csr(cxx(A), d_x, d_y, cxx(config), vec_size);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_spmv_ell(const spmv_c_ell* A, const float* d_x, float* d_y,
                    const spmv_c_config* config, int vec_size, spmv_c_result* out) {
    const SpMVResult r = spmv_ell(cxx(A), d_x, d_y, cxx(config), vec_size);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_auto_config(const spmv_c_csr* A, spmv_c_config* out) {
    if (!A || !out) return kInvalidArgument;
    const SpMVConfig c = spmv_auto_config(cxx(A));
    std::memset(out, 0, sizeof(*out));
    out->kernel_type = static_cast<int32_t>(c.kernel_type);
    out->block_size = c.block_size;
    out->use_texture = c.use_texture ? 1 : 0;
    return 0;
}

int spmv_c_validate_dimensions(int num_cols, int vec_size) {
    return spmv_validate_dimensions(num_cols, vec_size) ? 1 : 0;
}

void spmv_c_set_tiled_promotion(int calls) { spmv_set_tiled_promotion(calls); }
int spmv_c_get_tiled_promotion(void) { return spmv_get_tiled_promotion(); }

int spmv_c_csr_has_tiled_plan(const spmv_c_csr* A_c) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs) return 0;
    detail::CsrAux* aux = detail::aux_lookup(A->d_row_ptrs, false);
    return aux && aux->tiled ? 1 : 0;
}

int spmv_c_tiled_shape(int64_t rows, int64_t cols, int64_t nnz, int32_t* strip_cols, int32_t* tile_rows) {
    int w = 0, r = 0;
    const bool takes = detail::tiled_shape_for(rows, cols, nnz, &w, &r);
    if (strip_cols) *strip_cols = w;
    if (tile_rows) *tile_rows = r;
    return takes ? 1 : 0;
}

int spmv_c_csr_tiled_info(const spmv_c_csr* A_c, int64_t out[8]) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs || !out) return 0;
    detail::CsrAux* aux = detail::aux_lookup(A->d_row_ptrs, false);
    if (!aux || !aux->tiled) return 0;
    const detail::TiledPlan& p = *aux->tiled;
    const int64_t v[8] = {p.strip_cols, p.tile_rows, p.num_strips, p.num_tiles, p.nnz, p.num_long, 4 /* slots per lane per phase-2 pass */,
                          p.long_row};
    std::memcpy(out, v, sizeof(v));
    return 1;
}

int spmv_c_csr_tiled_stats(const spmv_c_csr* A_c, double out[4]) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs || !out) return 0;
    detail::CsrAux* aux = detail::aux_lookup(A->d_row_ptrs, false);
    if (!aux || !aux->tiled) return 0;
    const detail::TiledPlan& p = *aux->tiled;
    out[0] = p.build_ms;
    out[1] = static_cast<double>(p.plan_bytes);
    out[2] = static_cast<double>(p.nnz);
    out[3] = static_cast<double>(p.entries);
    return 1;
}

int spmv_c_csr_tiled_checksum(const spmv_c_csr* A_c, uint64_t out[4]) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs || !out) return 0;
    const detail::PlanRef plan = detail::tiled_plan_if_cached(A);
    if (!plan) return 0;
    unsigned long long sums[4] = {0, 0, 0, 0};
    if (detail::tiled_checksum(*plan, sums, detail::current_stream()) != hipSuccess) return 0;
    for (int i = 0; i < 4; ++i) out[i] = sums[i];
    return 1;
}

int spmv_c_csr_tiled_folded(const spmv_c_csr* A_c) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs) return 0;
    detail::CsrAux* aux = detail::aux_lookup(A->d_row_ptrs, false);
    return aux && aux->tiled && aux->tiled->col_weight ? 1 : 0;
}

int64_t spmv_c_csr_tiled_col_bytes(const spmv_c_csr* A_c) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs) return -1;
    detail::CsrAux* aux = detail::aux_lookup(A->d_row_ptrs, false);
    return aux && aux->tiled ? aux->tiled->col_bytes : -1;
}

int spmv_c_csr_tiled_items(const spmv_c_csr* A_c) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs) return -1;
    detail::CsrAux* aux = detail::aux_lookup(A->d_row_ptrs, false);
    return aux && aux->tiled ? aux->tiled->num_items : -1;
}

namespace {
// out[10] = the eight numbers of spmv_c_csr_tiled_info, then values folded (0 / 1) and the phase-1 item count
int plan_info10(const detail::TiledPlan& p, int64_t out[10]) {
    const int64_t v[10] = {p.strip_cols, p.tile_rows, p.num_strips, p.num_tiles, p.nnz, p.num_long, 4, p.long_row,
                           p.col_weight ? 1 : 0, p.num_items};
    std::memcpy(out, v, sizeof(v));
    return 1;
}
}  // namespace

int spmv_c_ell_tiled_info(const spmv_c_ell* E_c, int64_t out[10]) {
    const ELLMatrix* E = cxx(E_c);
    if (!E || !E->d_col_indices || !out) return 0;
    detail::EllAux* aux = detail::ell_aux_lookup(E->d_col_indices, false);
    return aux && aux->tiled ? plan_info10(*aux->tiled, out) : 0;
}

int spmv_c_csr_transpose_tiled_info(const spmv_c_csr* A_c, int64_t out[10]) {
    const CSRMatrix* A = cxx(A_c);
    if (!A || !A->d_row_ptrs || !out) return 0;
    detail::CsrAux* aux = detail::aux_lookup(A->d_row_ptrs, false);
    if (!aux) return 0;
    std::shared_ptr<CSRMatrix> at;
    {
        std::lock_guard<std::mutex> guard(aux->transpose_lock);
        at = aux->transpose;
    }
    if (!at || !at->d_row_ptrs) return 0;
    detail::CsrAux* at_aux = detail::aux_lookup(at->d_row_ptrs, false);
    return at_aux && at_aux->tiled ? plan_info10(*at_aux->tiled, out) : 0;
}

int spmv_c_spmv_csr_async(const spmv_c_csr* A, const float* d_x, float* d_y,
                          const spmv_c_config* config, int vec_size, void* hip_stream) {
    return spmv_csr_async(cxx(A), d_x, d_y, cxx(config), vec_size, as_stream(hip_stream));
}

int spmv_c_spmv_ell_async(const spmv_c_ell* A, const float* d_x, float* d_y,
                          const spmv_c_config* config, int vec_size, void* hip_stream) {
    return spmv_ell_async(cxx(A), d_x, d_y, cxx(config), vec_size, as_stream(hip_stream));
}

int spmv_c_spmv_csr_multi(const spmv_c_csr* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                          const spmv_c_config* config, int vec_size, spmv_c_result* out) {
    const SpMVResult r = spmv_csr_multi(cxx(A), d_X, ldx, d_Y, ldy, k, cxx(config), vec_size);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_spmv_csr_multi_async(const spmv_c_csr* A, const float* d_X, int ldx, float* d_Y, int ldy, int k,
                                const spmv_c_config* config, int vec_size, void* hip_stream) {
    return spmv_csr_multi_async(cxx(A), d_X, ldx, d_Y, ldy, k, cxx(config), vec_size, as_stream(hip_stream));
}

int spmv_c_spmv_csr_transpose(const spmv_c_csr* A, const float* d_x, float* d_y,
                              const spmv_c_config* config, int vec_size, spmv_c_result* out) {
    const SpMVResult r = spmv_csr_transpose(cxx(A), d_x, d_y, cxx(config), vec_size);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_spmv_csr_transpose_async(const spmv_c_csr* A, const float* d_x, float* d_y,
                                    const spmv_c_config* config, int vec_size, void* hip_stream) {
    return spmv_csr_transpose_async(cxx(A), d_x, d_y, cxx(config), vec_size, as_stream(hip_stream));
}

int spmv_c_cg_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_cg_config* config,
                    spmv_c_cg_result* out) {
    const CGResult r = cg_solve(cxx(A), d_b, d_x, reinterpret_cast<const CGConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_cg_solve_multi(const spmv_c_csr* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                          const spmv_c_cg_config* config, spmv_c_cg_result* results) {
    return cg_solve_multi(cxx(A), d_B, ldb, d_X, ldx, k, reinterpret_cast<const CGConfig*>(config),
                          reinterpret_cast<CGResult*>(results));
}

int spmv_c_cg_solve_multi_ic(const spmv_c_csr* A, const spmv_c_csr* F, const float* d_B, int ldb, float* d_X, int ldx,
                             int k, const spmv_c_cg_config* config, spmv_c_cg_result* results) {
    return cg_solve_multi_ic(cxx(A), cxx(F), d_B, ldb, d_X, ldx, k, reinterpret_cast<const CGConfig*>(config),
                             reinterpret_cast<CGResult*>(results));
}

int spmv_c_cg_solve_ic(const spmv_c_csr* A, const spmv_c_csr* F, const float* d_b, float* d_x,
                       const spmv_c_cg_config* config, spmv_c_cg_result* out) {
    const CGResult r = cg_solve_ic(cxx(A), cxx(F), d_b, d_x, reinterpret_cast<const CGConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_cg_solve_fsai(const spmv_c_csr* A, const spmv_c_csr* G, const spmv_c_csr* GT, const float* d_b, float* d_x,
                         const spmv_c_cg_config* config, spmv_c_cg_result* out) {
    const CGResult r = cg_solve_fsai(cxx(A), cxx(G), cxx(GT), d_b, d_x, reinterpret_cast<const CGConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_bicgstab_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_bicgstab_config* config,
                          spmv_c_bicgstab_result* out) {
    const BiCGStabResult r = bicgstab_solve(cxx(A), d_b, d_x, reinterpret_cast<const BiCGStabConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_bicgstab_solve_lu(const spmv_c_csr* A, const spmv_c_csr* LU, const float* d_b, float* d_x,
                             const spmv_c_bicgstab_config* config, spmv_c_bicgstab_result* out) {
    const BiCGStabResult r = bicgstab_solve_lu(cxx(A), cxx(LU), d_b, d_x,
                                               reinterpret_cast<const BiCGStabConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_gmres_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_gmres_config* config,
                       spmv_c_gmres_result* out) {
    const GMRESResult r = gmres_solve(cxx(A), d_b, d_x, reinterpret_cast<const GMRESConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_gmres_solve_lu(const spmv_c_csr* A, const spmv_c_csr* LU, const float* d_b, float* d_x,
                          const spmv_c_gmres_config* config, spmv_c_gmres_result* out) {
    const GMRESResult r = gmres_solve_lu(cxx(A), cxx(LU), d_b, d_x, reinterpret_cast<const GMRESConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_minres_solve(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_minres_config* config,
                        spmv_c_minres_result* out) {
    const MinresResult r = minres_solve(cxx(A), d_b, d_x, reinterpret_cast<const MinresConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_minres_solve_ic(const spmv_c_csr* A, const spmv_c_csr* F, const float* d_b, float* d_x,
                           const spmv_c_minres_config* config, spmv_c_minres_result* out) {
    const MinresResult r = minres_solve_ic(cxx(A), cxx(F), d_b, d_x, reinterpret_cast<const MinresConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_eigs_sym(const spmv_c_csr* A, float* d_values, float* d_vectors, int64_t ldv, float* d_residuals,
                    const float* d_v0, const spmv_c_eigs_config* config, spmv_c_eigs_result* out) {
    const EigsResult r = eigs_sym(cxx(A), d_values, d_vectors, ldv, d_residuals, d_v0,
                                  reinterpret_cast<const EigsConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_sym_eig_small(int n, const double* T, int ld, double* values, double* vectors, int on_device) {
    return sym_eig_small(n, T, ld, values, vectors, on_device);
}

int spmv_c_ilu0_csr(const spmv_c_csr* A, float* d_lu_values, spmv_c_ilu0_result* out) {
    const ILU0Result r = ilu0_csr(cxx(A), d_lu_values);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_ilu0_csr_async(const spmv_c_csr* A, float* d_lu_values, void* hip_stream) {
    return ilu0_csr_async(cxx(A), d_lu_values, as_stream(hip_stream));
}

int spmv_c_ilu0_cpu_csr(const spmv_c_csr* A, float* lu_values, int32_t* zero_pivot) {
    return ilu0_cpu_csr(cxx(A), lu_values, zero_pivot);
}

int spmv_c_ic0_csr(const spmv_c_csr* A, float* d_l_values, spmv_c_ic0_result* out) {
    const IC0Result r = ic0_csr(cxx(A), d_l_values);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_ic0_csr_async(const spmv_c_csr* A, float* d_l_values, void* hip_stream) {
    return ic0_csr_async(cxx(A), d_l_values, as_stream(hip_stream));
}

int spmv_c_ic0_cpu_csr(const spmv_c_csr* A, float* l_values, int32_t* bad_pivot) {
    return ic0_cpu_csr(cxx(A), l_values, bad_pivot);
}

int spmv_c_fsai_csr(spmv_c_csr* G, const spmv_c_csr* A, const spmv_c_csr* S, spmv_c_fsai_result* out) {
    const FSAIResult r = fsai_csr(cxx(G), cxx(A), cxx(S));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_fsai_csr_numeric(spmv_c_csr* G, const spmv_c_csr* A, spmv_c_fsai_result* out) {
    const FSAIResult r = fsai_csr_numeric(cxx(G), cxx(A));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_fsai_cpu_csr(spmv_c_csr* G, const spmv_c_csr* A, const spmv_c_csr* S, int32_t* bad_row) {
    return fsai_cpu_csr(cxx(G), cxx(A), cxx(S), bad_row);
}

int spmv_c_spgemm_csr(spmv_c_csr* C, const spmv_c_csr* A, const spmv_c_csr* B, spmv_c_spgemm_result* out) {
    SpGEMMResult r;
    const int status = spgemm_csr(cxx(C), cxx(A), cxx(B), &r);
    if (out) std::memcpy(out, &r, sizeof(r));
    return status;
}

int spmv_c_spgemm_csr_numeric(spmv_c_csr* C, const spmv_c_csr* A, const spmv_c_csr* B, spmv_c_spgemm_result* out) {
    SpGEMMResult r;
    const int status = spgemm_csr_numeric(cxx(C), cxx(A), cxx(B), &r);
    if (out) std::memcpy(out, &r, sizeof(r));
    return status;
}

int spmv_c_spgemm_cpu_csr(spmv_c_csr* C, const spmv_c_csr* A, const spmv_c_csr* B) {
    return spgemm_cpu_csr(cxx(C), cxx(A), cxx(B));
}

int spmv_c_spgemm_class_capacity(int cls) { return spgemm_class_capacity(cls); }

int spmv_c_amg_setup(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config, int aggregate_levels,
                     const int32_t* const* aggregates, spmv_c_amg_result* result) {
    const AMGAggregates given{aggregate_levels, aggregates};
    AMGHierarchy* H = nullptr;
    const AMGResult r = amg_setup(out ? &H : nullptr, cxx(A), reinterpret_cast<const AMGConfig*>(config),
                                  aggregates ? &given : nullptr);
    if (out) *out = reinterpret_cast<spmv_c_amg*>(H);
    if (result) std::memcpy(result, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_amg_update(spmv_c_amg* H, const spmv_c_csr* A, spmv_c_amg_result* result) {
    const AMGResult r = amg_update(cxx(H), cxx(A));
    if (result) std::memcpy(result, &r, sizeof(r));
    return r.error_code;
}

void spmv_c_amg_destroy(spmv_c_amg* H) { amg_destroy(cxx(H)); }

int spmv_c_amg_num_levels(const spmv_c_amg* H) { return amg_num_levels(cxx(H)); }

int spmv_c_amg_level(const spmv_c_amg* H, int level, spmv_c_csr* view, const int32_t** d_aggregate,
                     int32_t* num_aggregates) {
    return amg_level(cxx(H), level, cxx(view), d_aggregate, num_aggregates);
}

int spmv_c_amg_apply(const spmv_c_amg* H, const float* d_r, float* d_z) { return amg_apply(cxx(H), d_r, d_z); }

int spmv_c_amg_aggregate_cpu_csr(const spmv_c_csr* A, float strength, int32_t* aggregate, int32_t* num_aggregates) {
    return amg_aggregate_cpu_csr(cxx(A), strength, aggregate, num_aggregates);
}

int spmv_c_amg_aggregate_mis2_cpu_csr(const spmv_c_csr* A, float strength, uint32_t seed, int32_t* aggregate,
                                      int32_t* num_aggregates, int32_t* rounds) {
    return amg_aggregate_mis2_cpu_csr(cxx(A), strength, seed, aggregate, num_aggregates, rounds);
}

int spmv_c_amg_aggregate_mis2_gpu(const spmv_c_csr* A, float strength, uint32_t seed, int32_t* d_aggregate,
                                  int32_t* num_aggregates, int32_t* rounds) {
    return amg_aggregate_mis2_gpu(cxx(A), strength, seed, d_aggregate, num_aggregates, rounds);
}

int spmv_c_amg_setup_device(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config, uint32_t seed,
                            spmv_c_amg_result* result) {
    AMGHierarchy* H = nullptr;
    const AMGResult r = amg_setup_device(out ? &H : nullptr, cxx(A), reinterpret_cast<const AMGConfig*>(config), seed);
    if (out) *out = reinterpret_cast<spmv_c_amg*>(H);
    if (result) std::memcpy(result, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_amg_setup_rounds(const spmv_c_amg* H, int level) { return amg_setup_rounds(cxx(H), level); }

int spmv_c_amg_setup_smoothed(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config,
                              const spmv_c_amg_smoothing* smoothing, int aggregate_levels,
                              const int32_t* const* aggregates, spmv_c_amg_result* result) {
    const AMGAggregates given{aggregate_levels, aggregates};
    AMGHierarchy* H = nullptr;
    const AMGResult r = amg_setup_smoothed(out ? &H : nullptr, cxx(A), reinterpret_cast<const AMGConfig*>(config),
                                           reinterpret_cast<const AMGSmoothing*>(smoothing),
                                           aggregates ? &given : nullptr);
    if (out) *out = reinterpret_cast<spmv_c_amg*>(H);
    if (result) std::memcpy(result, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_amg_setup_smoothed_device(spmv_c_amg** out, const spmv_c_csr* A, const spmv_c_amg_config* config,
                                     const spmv_c_amg_smoothing* smoothing, uint32_t seed, spmv_c_amg_result* result) {
    AMGHierarchy* H = nullptr;
    const AMGResult r = amg_setup_smoothed_device(out ? &H : nullptr, cxx(A), reinterpret_cast<const AMGConfig*>(config),
                                                  reinterpret_cast<const AMGSmoothing*>(smoothing), seed);
    if (out) *out = reinterpret_cast<spmv_c_amg*>(H);
    if (result) std::memcpy(result, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_amg_is_smoothed(const spmv_c_amg* H) { return amg_is_smoothed(cxx(H)); }

int spmv_c_amg_level_transfer(const spmv_c_amg* H, int level, spmv_c_csr* P_view, spmv_c_csr* PT_view) {
    return amg_level_transfer(cxx(H), level, cxx(P_view), cxx(PT_view));
}

int spmv_c_amg_prolongator_cpu_csr(spmv_c_csr* P, const spmv_c_csr* A, const int32_t* aggregate, int num_aggregates,
                                   float weight) {
    return amg_prolongator_cpu_csr(cxx(P), cxx(A), aggregate, num_aggregates, weight);
}

int spmv_c_amg_restrict(const spmv_c_amg* H, int level, const float* d_f, const float* d_x, float* d_f_coarse) {
    return amg_restrict(cxx(H), level, d_f, d_x, d_f_coarse);
}

int spmv_c_amg_prolong(const spmv_c_amg* H, int level, const float* d_e, float* d_x) {
    return amg_prolong(cxx(H), level, d_e, d_x);
}

int spmv_c_cg_solve_amg(const spmv_c_csr* A, const spmv_c_amg* H, const float* d_b, float* d_x,
                        const spmv_c_cg_config* config, spmv_c_cg_result* out) {
    const CGResult r = cg_solve_amg(cxx(A), cxx(H), d_b, d_x, reinterpret_cast<const CGConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_sptrsv_csr(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                      spmv_c_sptrsv_result* out) {
    const SpTRSVResult r = sptrsv_csr(cxx(A), d_b, d_x, reinterpret_cast<const SpTRSVConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_sptrsv_csr_async(const spmv_c_csr* A, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                            void* hip_stream) {
    return sptrsv_csr_async(cxx(A), d_b, d_x, reinterpret_cast<const SpTRSVConfig*>(config), as_stream(hip_stream));
}

int spmv_c_sptrsv_analyze(const spmv_c_csr* A, int uplo, spmv_c_sptrsv_result* out) {
    const SpTRSVResult r = sptrsv_analyze(cxx(A), uplo);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_sptrsv_analyze_device(const spmv_c_csr* A, int uplo, spmv_c_sptrsv_result* out) {
    const SpTRSVResult r = sptrsv_analyze_device(cxx(A), uplo);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_sptrsv_schedule_get(const spmv_c_csr* A, int uplo, int32_t* level_ptr, int32_t* order,
                               spmv_c_sptrsv_schedule_info* info) {
    return sptrsv_schedule_get(cxx(A), uplo, level_ptr, order, reinterpret_cast<SpTRSVScheduleInfo*>(info));
}

int spmv_c_sptrsv_cpu_csr(const spmv_c_csr* A, const float* b, float* x, const spmv_c_sptrsv_config* config) {
    return sptrsv_cpu_csr(cxx(A), b, x, reinterpret_cast<const SpTRSVConfig*>(config));
}

int spmv_c_sptrsv_csr_multi(const spmv_c_csr* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                            const spmv_c_sptrsv_config* config, spmv_c_sptrsv_result* out) {
    const SpTRSVResult r = sptrsv_csr_multi(cxx(A), d_B, ldb, d_X, ldx, k,
                                            reinterpret_cast<const SpTRSVConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_sptrsv_csr_multi_async(const spmv_c_csr* A, const float* d_B, int ldb, float* d_X, int ldx, int k,
                                  const spmv_c_sptrsv_config* config, void* hip_stream) {
    return sptrsv_csr_multi_async(cxx(A), d_B, ldb, d_X, ldx, k, reinterpret_cast<const SpTRSVConfig*>(config),
                                  as_stream(hip_stream));
}

int spmv_c_sptrsv_cpu_csr_multi(const spmv_c_csr* A, const float* B, int ldb, float* X, int ldx, int k,
                                const spmv_c_sptrsv_config* config) {
    return sptrsv_cpu_csr_multi(cxx(A), B, ldb, X, ldx, k, reinterpret_cast<const SpTRSVConfig*>(config));
}

int spmv_c_sptrsv_levels(int num_rows,const int32_t* row_ptrs, const int32_t* col_indices, int uplo,
                         int32_t* level_ptr, int32_t* order, int32_t* num_levels, int32_t* first_missing_diagonal) {
    return sptrsv_levels(num_rows, row_ptrs, col_indices, uplo, level_ptr, order, num_levels, first_missing_diagonal);
}

// ---- multicolour reordering ----
int spmv_c_csr_color(const spmv_c_csr* A, int32_t* d_colors, const spmv_c_color_config* config,
                     spmv_c_color_result* out) {
    const ColorResult r = csr_color(cxx(A), d_colors, reinterpret_cast<const ColorConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_csr_color_cpu(const spmv_c_csr* A, int32_t* colors, int32_t* num_colors, int32_t* rounds,
                         const spmv_c_color_config* config) {
    return csr_color_cpu(cxx(A), colors, num_colors, rounds, reinterpret_cast<const ColorConfig*>(config));
}

int spmv_c_color_ordering(int n, const int32_t* d_colors, int num_colors, int32_t* d_perm, int32_t* d_inverse,
                          int32_t* color_ptr) {
    return color_ordering(n, d_colors, num_colors, d_perm, d_inverse, color_ptr);
}

int spmv_c_csr_permute_gpu(spmv_c_csr* B, const spmv_c_csr* A, const int32_t* d_row_perm,
                           const int32_t* d_col_inverse) {
    return csr_permute_gpu(cxx(B), cxx(A), d_row_perm, d_col_inverse);
}

int spmv_c_csr_permute_cpu(spmv_c_csr* B, const spmv_c_csr* A, const int32_t* row_perm, const int32_t* col_inverse) {
    return csr_permute_cpu(cxx(B), cxx(A), row_perm, col_inverse);
}

int spmv_c_permute_gather(float* d_out, int ldo, const float* d_in, int ldi, const int32_t* d_index, int n, int k) {
    return permute_gather(d_out, ldo, d_in, ldi, d_index, n, k);
}

int spmv_c_permute_gather_async(float* d_out, int ldo, const float* d_in, int ldi, const int32_t* d_index, int n,
                                int k, void* hip_stream) {
    return permute_gather_async(d_out, ldo, d_in, ldi, d_index, n, k, as_stream(hip_stream));
}

int spmv_c_multicolor_reorder(spmv_c_csr* B, const spmv_c_csr* A, int32_t* d_perm, int32_t* d_inverse,
                              const spmv_c_color_config* config, spmv_c_color_result* out) {
    const ColorResult r = multicolor_reorder(cxx(B), cxx(A), d_perm, d_inverse,
                                             reinterpret_cast<const ColorConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

// ---- reverse Cuthill-McKee reordering ----
int spmv_c_csr_rcm(const spmv_c_csr* A, int32_t* d_perm, int32_t* d_inverse, const spmv_c_rcm_config* config,
                   spmv_c_rcm_result* out) {
    const RcmResult r = csr_rcm(cxx(A), d_perm, d_inverse, reinterpret_cast<const RcmConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_csr_rcm_cpu(const spmv_c_csr* A, int32_t* perm, int32_t* inverse, int32_t* components, int32_t* levels,
                       const spmv_c_rcm_config* config) {
    return csr_rcm_cpu(cxx(A), perm, inverse, components, levels, reinterpret_cast<const RcmConfig*>(config));
}

int spmv_c_rcm_reorder(spmv_c_csr* B, const spmv_c_csr* A, int32_t* d_perm, int32_t* d_inverse,
                       const spmv_c_rcm_config* config, spmv_c_rcm_result* out) {
    const RcmResult r = rcm_reorder(cxx(B), cxx(A), d_perm, d_inverse, reinterpret_cast<const RcmConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_csr_band_gpu(const spmv_c_csr* A, spmv_c_csr_band* out) {
    return csr_band_gpu(cxx(A), reinterpret_cast<CsrBand*>(out));
}

int spmv_c_csr_band_cpu(const spmv_c_csr* A, spmv_c_csr_band* out) {
    return csr_band_cpu(cxx(A), reinterpret_cast<CsrBand*>(out));
}

// ---- matrix assembly ----
int spmv_c_csr_from_coo_cpu(spmv_c_csr* C, int num_rows, int num_cols, int n, const int32_t* rows, const int32_t* cols,
                            const float* vals, const spmv_c_coo_config* config) {
    return csr_from_coo_cpu(cxx(C), num_rows, num_cols, n, rows, cols, vals, reinterpret_cast<const CooConfig*>(config));
}

int spmv_c_csr_from_coo_gpu(spmv_c_csr* C, int num_rows, int num_cols, int n, const int32_t* d_rows,
                            const int32_t* d_cols, const float* d_vals, const spmv_c_coo_config* config,
                            spmv_c_coo_plan** plan, spmv_c_coo_result* out) {
    const CooResult r = csr_from_coo_gpu(cxx(C), num_rows, num_cols, n, d_rows, d_cols, d_vals,
                                         reinterpret_cast<const CooConfig*>(config),
                                         reinterpret_cast<CooPlan**>(plan));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

int spmv_c_csr_coo_refill(const spmv_c_coo_plan* plan, spmv_c_csr* C, const float* d_vals) {
    return csr_coo_refill(reinterpret_cast<const CooPlan*>(plan), cxx(C), d_vals);
}

int spmv_c_csr_coo_refill_async(const spmv_c_coo_plan* plan, spmv_c_csr* C, const float* d_vals, void* hip_stream) {
    return csr_coo_refill_async(reinterpret_cast<const CooPlan*>(plan), cxx(C), d_vals, as_stream(hip_stream));
}

void spmv_c_coo_plan_destroy(spmv_c_coo_plan* plan) { coo_plan_destroy(reinterpret_cast<CooPlan*>(plan)); }

int spmv_c_coo_plan_info(const spmv_c_coo_plan* plan, int32_t* num_rows, int32_t* num_cols, int32_t* n,
                         int32_t* nnz_out, int32_t* duplicates) {
    return coo_plan_info(reinterpret_cast<const CooPlan*>(plan), num_rows, num_cols, n, nnz_out, duplicates);
}

int spmv_c_csr_row_indices_gpu(const spmv_c_csr* A, int32_t* d_rows) { return csr_row_indices_gpu(cxx(A), d_rows); }

// ---- CSR algebra (include/spmv/csr_ops.h) ----
int spmv_c_csr_add(spmv_c_csr* C, float alpha, const spmv_c_csr* A, float beta, const spmv_c_csr* B,
                   spmv_c_csr_add_result* out) {
    CsrAddResult r;
    const int status = csr_add(cxx(C), alpha, cxx(A), beta, cxx(B), &r);
    if (out) std::memcpy(out, &r, sizeof(r));
    return status;
}

int spmv_c_csr_add_numeric(spmv_c_csr* C, float alpha, const spmv_c_csr* A, float beta, const spmv_c_csr* B,
                           spmv_c_csr_add_result* out) {
    CsrAddResult r;
    const int status = csr_add_numeric(cxx(C), alpha, cxx(A), beta, cxx(B), &r);
    if (out) std::memcpy(out, &r, sizeof(r));
    return status;
}

int spmv_c_csr_add_cpu(spmv_c_csr* C, float alpha, const spmv_c_csr* A, float beta, const spmv_c_csr* B) {
    return csr_add_cpu(cxx(C), alpha, cxx(A), beta, cxx(B));
}

int spmv_c_csr_scale_gpu(spmv_c_csr* A, const float* d_row_scale, const float* d_col_scale, float* d_values_out) {
    return csr_scale_gpu(cxx(A), d_row_scale, d_col_scale, d_values_out);
}

int spmv_c_csr_scale_cpu(const spmv_c_csr* A, const float* row_scale, const float* col_scale, float* values_out) {
    return csr_scale_cpu(cxx(A), row_scale, col_scale, values_out);
}

int spmv_c_csr_diagonal_gpu(const spmv_c_csr* A, float* d_diag) { return csr_diagonal_gpu(cxx(A), d_diag); }

int spmv_c_csr_diagonal_cpu(const spmv_c_csr* A, float* diag) { return csr_diagonal_cpu(cxx(A), diag); }

int spmv_c_csr_diag_matrix_gpu(spmv_c_csr* D, int n, const float* d_diag) {
    return csr_diag_matrix_gpu(cxx(D), n, d_diag);
}

int spmv_c_csr_diag_matrix_cpu(spmv_c_csr* D, int n, const float* diag) { return csr_diag_matrix_cpu(cxx(D), n, diag); }

// ---- bandwidth ----
int spmv_c_compute_bandwidth_csr(const spmv_c_csr* A, float elapsed_ms, spmv_c_bandwidth* out) {
    if (!out) return kInvalidArgument;
    const BandwidthMetrics m = compute_bandwidth_csr(cxx(A), elapsed_ms);
    std::memcpy(out, &m, sizeof(m));
    return 0;
}
int spmv_c_compute_bandwidth_ell(const spmv_c_ell* A, float elapsed_ms, spmv_c_bandwidth* out) {
    if (!out) return kInvalidArgument;
    const BandwidthMetrics m = compute_bandwidth_ell(cxx(A), elapsed_ms);
    std::memcpy(out, &m, sizeof(m));
    return 0;
}
float spmv_c_get_gpu_peak_bandwidth(void) { return get_gpu_peak_bandwidth(); }

int spmv_c_compute_bandwidth_csr_multi(const spmv_c_csr* A, int k, float elapsed_ms, spmv_c_bandwidth* out) {
    if (!out) return kInvalidArgument;
    const BandwidthMetrics m = compute_bandwidth_csr_multi(cxx(A), k, elapsed_ms);
    std::memcpy(out, &m, sizeof(m));
    return 0;
}

// ---- block CSR ----
spmv_c_bsr* spmv_c_bsr_create(int rows, int cols, int block_dim, int num_blocks) {
    return reinterpret_cast<spmv_c_bsr*>(bsr_create(rows, cols, block_dim, num_blocks));
}
void spmv_c_bsr_destroy(spmv_c_bsr* mat) { bsr_destroy(cxx(mat)); }
int spmv_c_bsr_to_gpu(spmv_c_bsr* mat) { return bsr_to_gpu(cxx(mat)); }
int spmv_c_bsr_from_gpu(spmv_c_bsr* mat) { return bsr_from_gpu(cxx(mat)); }
void spmv_c_bsr_free_gpu(spmv_c_bsr* mat) { bsr_free_gpu(cxx(mat)); }
void spmv_c_bsr_invalidate_gpu_cache(const spmv_c_bsr* mat) { bsr_invalidate_gpu_cache(cxx(mat)); }
spmv_c_bsr* spmv_c_bsr_wrap_device(int rows, int cols, int block_dim, int num_blocks, const int32_t* d_block_row_ptrs,
                                   const int32_t* d_block_cols, const float* d_values) {
    return reinterpret_cast<spmv_c_bsr*>(bsr_wrap_device(rows, cols, block_dim, num_blocks, d_block_row_ptrs,
                                                         d_block_cols, d_values));
}
int spmv_c_bsr_from_csr_cpu(spmv_c_bsr* B, const spmv_c_csr* A, int block_dim) {
    return bsr_from_csr_cpu(cxx(B), cxx(A), block_dim);
}
int spmv_c_bsr_from_csr_gpu(spmv_c_bsr* B, const spmv_c_csr* A, int block_dim, spmv_c_bsr_build_result* out) {
    BsrBuildResult r;
    const int status = bsr_from_csr_gpu(cxx(B), cxx(A), block_dim, &r);
    if (out) std::memcpy(out, &r, sizeof(r));
    return status;
}
int spmv_c_bsr_from_csr_numeric(spmv_c_bsr* B, const spmv_c_csr* A, spmv_c_bsr_build_result* out) {
    BsrBuildResult r;
    const int status = bsr_from_csr_numeric(cxx(B), cxx(A), &r);
    if (out) std::memcpy(out, &r, sizeof(r));
    return status;
}
int spmv_c_csr_block_count_gpu(const spmv_c_csr* A, int block_dim, int64_t* blocks) {
    long long count = 0;
    const int status = csr_block_count_gpu(cxx(A), block_dim, blocks ? &count : nullptr);
    if (status == 0) *blocks = count;
    return status;
}
int spmv_c_bsr_to_csr_gpu(spmv_c_csr* A, const spmv_c_bsr* B, int keep_zeros) {
    return bsr_to_csr_gpu(cxx(A), cxx(B), keep_zeros);
}
int spmv_c_bsr_to_csr_cpu(spmv_c_csr* A, const spmv_c_bsr* B, int keep_zeros) {
    return bsr_to_csr_cpu(cxx(A), cxx(B), keep_zeros);
}
void spmv_c_cpu_bsr(const spmv_c_bsr* A, const float* x, float* y) { spmv_cpu_bsr(cxx(A), x, y); }
int spmv_c_spmv_bsr(const spmv_c_bsr* A, const float* d_x, float* d_y, const spmv_c_config* config, int vec_size,
                    spmv_c_result* out) {
    const SpMVResult r = spmv_bsr(cxx(A), d_x, d_y, cxx(config), vec_size);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}
int spmv_c_spmv_bsr_async(const spmv_c_bsr* A, const float* d_x, float* d_y, const spmv_c_config* config,
                          int vec_size, void* hip_stream) {
    return spmv_bsr_async(cxx(A), d_x, d_y, cxx(config), vec_size, as_stream(hip_stream));
}
int spmv_c_compute_bandwidth_bsr(const spmv_c_bsr* A, float elapsed_ms, spmv_c_bandwidth* out) {
    if (!out) return kInvalidArgument;
    const BandwidthMetrics m = compute_bandwidth_bsr(cxx(A), elapsed_ms);
    std::memcpy(out, &m, sizeof(m));
    return 0;
}
int spmv_c_bsr_diag_inverse_cpu(const spmv_c_bsr* A, float* inv) { return bsr_diag_inverse_cpu(cxx(A), inv); }
int spmv_c_bsr_diag_inverse_gpu(const spmv_c_bsr* A, float* d_inv) { return bsr_diag_inverse_gpu(cxx(A), d_inv); }
void spmv_c_bsr_diag_apply_cpu(const spmv_c_bsr* A, const float* inv, const float* r, float* z) {
    bsr_diag_apply_cpu(cxx(A), inv, r, z);
}
int spmv_c_bsr_diag_apply(const spmv_c_bsr* A, const float* d_inv, const float* d_r, float* d_z) {
    return bsr_diag_apply(cxx(A), d_inv, d_r, d_z);
}
int spmv_c_cg_solve_bsr(const spmv_c_bsr* A, const float* d_b, float* d_x, const spmv_c_cg_config* config,
                        spmv_c_cg_result* out) {
    const CGResult r = cg_solve_bsr(cxx(A), d_b, d_x, reinterpret_cast<const CGConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}
int spmv_c_bsr_ic0_cpu(const spmv_c_bsr* A, float* f_values, int* bad_pivot) {
    return bsr_ic0_cpu(cxx(A), f_values, bad_pivot);
}
int spmv_c_bsr_ic0(const spmv_c_bsr* A, float* d_f_values, spmv_c_ic0_result* out) {
    const BsrIC0Result r = bsr_ic0(cxx(A), d_f_values);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}
int spmv_c_bsr_ic0_async(const spmv_c_bsr* A, float* d_f_values, void* hip_stream) {
    return bsr_ic0_async(cxx(A), d_f_values, as_stream(hip_stream));
}
int spmv_c_sptrsv_cpu_bsr(const spmv_c_bsr* F, const float* b, float* x, const spmv_c_sptrsv_config* config) {
    return sptrsv_cpu_bsr(cxx(F), b, x, reinterpret_cast<const SpTRSVConfig*>(config));
}
int spmv_c_sptrsv_bsr(const spmv_c_bsr* F, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                      spmv_c_sptrsv_result* out) {
    const SpTRSVResult r = sptrsv_bsr(cxx(F), d_b, d_x, reinterpret_cast<const SpTRSVConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}
int spmv_c_sptrsv_bsr_async(const spmv_c_bsr* F, const float* d_b, float* d_x, const spmv_c_sptrsv_config* config,
                            void* hip_stream) {
    return sptrsv_bsr_async(cxx(F), d_b, d_x, reinterpret_cast<const SpTRSVConfig*>(config), as_stream(hip_stream));
}
int spmv_c_sptrsv_analyze_bsr(const spmv_c_bsr* A, int uplo, spmv_c_sptrsv_result* out) {
    const SpTRSVResult r = sptrsv_analyze_bsr(cxx(A), uplo);
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}
int spmv_c_cg_solve_bsr_ic(const spmv_c_bsr* A, const spmv_c_bsr* F, const float* d_b, float* d_x,
                           const spmv_c_cg_config* config, spmv_c_cg_result* out) {
    const CGResult r = cg_solve_bsr_ic(cxx(A), cxx(F), d_b, d_x, reinterpret_cast<const CGConfig*>(config));
    if (out) std::memcpy(out, &r, sizeof(r));
    return r.error_code;
}

// ---- PageRank ----
int spmv_c_pagerank(const spmv_c_csr* adj, const spmv_c_pagerank_config* config,
                    spmv_c_pagerank_result* out) {
    if (!out) return kInvalidArgument;
    const PageRankResult r = pagerank(cxx(adj), reinterpret_cast<const PageRankConfig*>(config));
    std::memset(out, 0, sizeof(*out));
    out->ranks = r.ranks;
    out->iterations = r.iterations;
    out->final_residual = r.final_residual;
    out->converged = r.converged ? 1 : 0;
    return adj ? 0 : kInvalidArgument;
}

int spmv_c_pagerank_multi_gpu(const spmv_c_csr* adj, const spmv_c_pagerank_config* config, int num_gpus,
                              spmv_c_pagerank_result* out) {
    if (!out) return kInvalidArgument;
    const PageRankResult r = pagerank_multi_gpu(cxx(adj), reinterpret_cast<const PageRankConfig*>(config), num_gpus);
    std::memset(out, 0, sizeof(*out));
    out->ranks = r.ranks;
    out->iterations = r.iterations;
    out->final_residual = r.final_residual;
    out->converged = r.converged ? 1 : 0;
    return adj ? 0 : kInvalidArgument;
}

int spmv_c_pagerank_shard_bounds(const int32_t* row_ptrs, int num_rows, int num_shards, int32_t* bounds) {
    if (!row_ptrs || !bounds || num_rows < 0 || num_shards < 1) return kInvalidArgument;
    const std::vector<int> b = pagerank_shard_bounds(row_ptrs, num_rows, num_shards);
    std::copy(b.begin(), b.end(), bounds);
    return 0;
}

void spmv_c_pagerank_free(spmv_c_pagerank_result* result) {
    pagerank_free(reinterpret_cast<PageRankResult*>(result));
}

void spmv_c_pagerank_top_k(const spmv_c_pagerank_result* result, int num_nodes, int k,
                           spmv_c_topk_node* top_k) {
    pagerank_top_k(reinterpret_cast<const PageRankResult*>(result), num_nodes, k,
                   reinterpret_cast<TopKNode*>(top_k));
}

int spmv_c_pagerank_personalized(const spmv_c_csr* adj, const float* d_V, int ldv, float* d_R, int ldr, int k,
                                 const spmv_c_pagerank_config* config, spmv_c_personalized_result* results) {
    return pagerank_personalized(cxx(adj), d_V, ldv, d_R, ldr, k, reinterpret_cast<const PageRankConfig*>(config),
                                 reinterpret_cast<PersonalizedResult*>(results));
}

int spmv_c_pagerank_personalized_seeds(const spmv_c_csr* adj, const int32_t* seed_ptrs, const int32_t* seed_nodes,
                                       int k, float* d_R, int ldr, const spmv_c_pagerank_config* config,
                                       spmv_c_personalized_result* results) {
    return pagerank_personalized_seeds(cxx(adj), seed_ptrs, seed_nodes, k, d_R, ldr,
                                       reinterpret_cast<const PageRankConfig*>(config),
                                       reinterpret_cast<PersonalizedResult*>(results));
}

// ---- PageRank shard engine ----
spmv_c_pr_shard* spmv_c_pr_shard_create(const spmv_c_csr* A_local, int row_offset, int n_global,
                                        const uint8_t* d_dangling_mask) {
    return spmv_c_pr_shard_create_chunked(A_local, row_offset, 0x7fffffff, 0, n_global, d_dangling_mask);
}

spmv_c_pr_shard* spmv_c_pr_shard_create_chunked(const spmv_c_csr* A_local, int base, int piece, int block,
                                                int n_global, const uint8_t* d_dangling_mask) {
    const CSRMatrix* A = cxx(A_local);
    // the rank vector is indexed by column (num_cols long, possibly padded); n_global is the true node count
    if (!A || base < 0 || piece <= 0 || block < 0 || n_global <= 0 || !d_dangling_mask || n_global > A->num_cols ||
        (A->num_rows > 0 && !A->d_row_ptrs) ||
        (A->nnz > 0 && (!A->d_col_indices || !A->d_values))) {
        return nullptr;
    }
    detail::RowMap map;
    map.base = base;
    map.piece = piece;
    map.block = block;
    // every local row must land inside the vector, pieces must not overlap
    if (A->num_rows > 0) {
        const bool chunked = piece != 0x7fffffff;
        if (chunked && block < piece) return nullptr;
        const long long pieces = chunked ? (static_cast<long long>(A->num_rows) + piece - 1) / piece : 1;
        const long long last = map.at(static_cast<long long>(A->num_rows) - 1);
        if (last >= A->num_cols || (pieces > 1 && static_cast<long long>(base) + piece > block)) return nullptr;
    }
    spmv_c_pr_shard* h = new (std::nothrow) spmv_c_pr_shard();
    if (!h) return nullptr;
    detail::PrShard& sh = h->shard;
    sh.local_rows = A->num_rows;
    sh.map = map;
    sh.n_global = n_global;
    sh.nnz = A->nnz;
    sh.d_row_ptrs = A->d_row_ptrs;
    sh.d_cols = A->d_col_indices;
    sh.d_vals = A->d_values;
    sh.d_dangling = d_dangling_mask;
    const int partial_pairs = detail::pr_shard_prepare(&sh, detail::tiled_plan_for(A, nullptr));
    if (hipMalloc(reinterpret_cast<void**>(&sh.d_state), sizeof(detail::PrState)) != hipSuccess ||
        hipMalloc(reinterpret_cast<void**>(&sh.d_block_partials),
                  2 * sizeof(double) * static_cast<size_t>(partial_pairs)) != hipSuccess) {
        spmv_c_pr_shard_destroy(h);
        return nullptr;
    }
    // The tiled engine's phase 2 reads the flags of a contiguous slice as bits (DanglingBits, pagerank_engine.h): derived
    // here from the mask as it stands, and again by every spmv_c_pr_reset, for callers that fill the mask in between.
    // (SPMV_DEBUG=dangling=bytes keeps the shard on the byte mask: the A/B switch of profiles/aligned_streams_traffic_ab.txt.)
    if (sh.tiled && sh.local_rows > 0 && piece == 0x7fffffff && !detail::debug_is("dangling", "bytes")) {
        hipStream_t s = detail::current_stream();
        if (hipMalloc(reinterpret_cast<void**>(&sh.d_dangling_words),
                      sizeof(unsigned int) * detail::pr_dangling_words(sh.local_rows)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&sh.d_tile_dangling), sizeof(int) * static_cast<size_t>(sh.tiled->num_tiles)) != hipSuccess ||
            detail::pr_dangling_bits(&sh, s) != hipSuccess || hipStreamSynchronize(s) != hipSuccess) {
            (void)hipGetLastError();
            spmv_c_pr_shard_destroy(h);
            return nullptr;
        }
    }
    return h;
}

void spmv_c_pr_shard_destroy(spmv_c_pr_shard* h) {
    if (!h) return;
    if (h->shard.commit_pending) {          // the state dies with the shard, but the rule has no exception: flush
        (void)detail::pr_flush(h->shard, h->shard.pending_stream);
        (void)hipGetLastError();
    }
    if (h->shard.d_state) (void)hipFree(h->shard.d_state);
    if (h->shard.d_block_partials) (void)hipFree(h->shard.d_block_partials);
    if (h->shard.d_dangling_words) (void)hipFree(h->shard.d_dangling_words);
    if (h->shard.d_tile_dangling) (void)hipFree(h->shard.d_tile_dangling);
    delete h;
}

int spmv_c_pr_reset(spmv_c_pr_shard* h, float dangling_sum, void* hip_stream) {
    if (!h) return kInvalidArgument;
    detail::PrState fresh{};
    fresh.dangling_sum = dangling_sum;
    h->shard.expanded_strips = 0;          // a head start taken for a step that never ran is void
    h->shard.expanded_long = false;
    detail::pr_drop_pending(h->shard);     // ... and so is a commit that nobody asked to see
    if (detail::pr_dangling_bits(&h->shard, as_stream(hip_stream)) != hipSuccess) return kLaunch;
    // pageable source: the copy is staged before the call returns
    return hipMemcpyAsync(h->shard.d_state, &fresh, sizeof(fresh), hipMemcpyHostToDevice,
                          as_stream(hip_stream)) == hipSuccess
         ? 0 : static_cast<int>(SpMVError::CUDA_MEMCPY);
}

int spmv_c_pr_step(spmv_c_pr_shard* h, const float* d_r_old, float* d_r_new, float damping,
                   void* hip_stream) {
    if (!h || !d_r_old || !d_r_new) return kInvalidArgument;
    return launch_code(detail::pr_step(h->shard, d_r_old, d_r_new, damping, detail::PushTargets{},
                                       as_stream(hip_stream)));
}

int spmv_c_pr_step_commit(spmv_c_pr_shard* h, const float* d_r_old, float* d_r_new, float damping,
                          float tolerance, void* hip_stream) {
    if (!h || !d_r_old || !d_r_new) return kInvalidArgument;
    return launch_code(detail::pr_step_commit(h->shard, d_r_old, d_r_new, damping, tolerance, as_stream(hip_stream)));
}

int spmv_c_pr_expand(spmv_c_pr_shard* h, const float* d_r_old, int64_t cols_ready, void* hip_stream) {
    if (!h || !d_r_old) return kInvalidArgument;
    return launch_code(detail::pr_expand(h->shard, d_r_old, cols_ready, as_stream(hip_stream)));
}

int spmv_c_pr_step_push(spmv_c_pr_shard* h, const float* d_r_old, float* d_r_new, float damping,
                        float* const* peer_r_new, int num_peers, void* hip_stream) {
    if (!h || !d_r_old || !d_r_new || num_peers < 0 || num_peers > detail::kMaxPushPeers ||
        (num_peers > 0 && !peer_r_new)) {
        return kInvalidArgument;
    }
    detail::PushTargets push;
    for (int p = 0; p < num_peers; ++p) {
        if (!peer_r_new[p]) return kInvalidArgument;
        push.ptr[push.count++] = peer_r_new[p];
    }
    return launch_code(detail::pr_step(h->shard, d_r_old, d_r_new, damping, push, as_stream(hip_stream)));
}

int spmv_c_pr_reduce(spmv_c_pr_shard* h, double* d_sums, void* hip_stream) {
    if (!h || !d_sums) return kInvalidArgument;
    return launch_code(detail::pr_reduce(h->shard, d_sums, as_stream(hip_stream)));
}

int spmv_c_pr_commit(spmv_c_pr_shard* h, const double* d_sums, float tolerance, void* hip_stream) {
    if (!h || !d_sums) return kInvalidArgument;
    return launch_code(detail::pr_commit(h->shard, d_sums, tolerance, as_stream(hip_stream)));
}

int spmv_c_pr_reduce_commit(spmv_c_pr_shard* h, float tolerance, void* hip_stream) {
    if (!h) return kInvalidArgument;
    return launch_code(detail::pr_reduce_commit(h->shard, tolerance, as_stream(hip_stream)));
}

int spmv_c_pr_commit_gathered(spmv_c_pr_shard* h, const float* d_gathered, int world, int64_t stride,
                              int64_t shard_len, float tolerance, void* hip_stream) {
    if (!h || !d_gathered || world < 1 || stride < shard_len + 4 || (stride & 1) || (shard_len & 1)) {
        return kInvalidArgument;
    }
    return launch_code(detail::pr_commit_gathered(h->shard, d_gathered, world, stride, shard_len, tolerance,
                                                  as_stream(hip_stream)));
}

int spmv_c_pr_status_get(spmv_c_pr_shard* h, spmv_c_pr_status* out, void* hip_stream) {
    if (!h || !out) return kInvalidArgument;
    hipStream_t s = as_stream(hip_stream);
    if (detail::pr_flush(h->shard, s) != hipSuccess) return kLaunch;
    if (hipMemcpyAsync(out, h->shard.d_state, sizeof(*out), hipMemcpyDeviceToHost, s) != hipSuccess) {
        return static_cast<int>(SpMVError::CUDA_MEMCPY);
    }
    // A stream that is being captured cannot be waited for: the flush and the copy become nodes of the graph,
    // and `out` (pinned memory that outlives the graph) is filled by every replay.
    hipStreamCaptureStatus capturing = hipStreamCaptureStatusNone;
    if (hipStreamIsCapturing(s, &capturing) != hipSuccess) {
        (void)hipGetLastError();
        capturing = hipStreamCaptureStatusNone;
    }
    if (capturing == hipStreamCaptureStatusNone && hipStreamSynchronize(s) != hipSuccess) {
        return static_cast<int>(SpMVError::CUDA_MEMCPY);
    }
    return 0;
}

int spmv_c_pr_column_sums(const spmv_c_csr* A_local, float* d_col_sums, void* hip_stream) {
    const CSRMatrix* A = cxx(A_local);
    if (!A || !d_col_sums) return kInvalidArgument;
    return launch_code(detail::pr_column_sums(A->nnz, A->d_col_indices, A->d_values, A->num_cols,
                                              d_col_sums, as_stream(hip_stream)));
}

int spmv_c_pr_mask_from_column_sums(const float* d_col_sums, int n, uint8_t* d_mask,
                                    uint64_t* d_count, void* hip_stream) {
    if (!d_col_sums || !d_mask || !d_count || n < 0) return kInvalidArgument;
    return launch_code(detail::pr_mask_from_column_sums(
        d_col_sums, n, d_mask, reinterpret_cast<unsigned long long*>(d_count), as_stream(hip_stream)));
}

int spmv_c_fill(float* d_r, size_t n, float value, void* hip_stream) {
    if (n > 0 && !d_r) return kInvalidArgument;
    return launch_code(detail::pr_fill(d_r, n, value, as_stream(hip_stream)));
}

// ---- generators ----
int spmv_c_gen_uniform_rows(uint64_t seed, int row_begin, int local_rows, int n_cols, int k,
                            int32_t* d_row_ptrs, int32_t* d_cols, float* d_vals, void* hip_stream) {
    return detail::gen_uniform_rows(seed, row_begin, local_rows, n_cols, k, d_row_ptrs, d_cols,
                                    d_vals, as_stream(hip_stream));
}

int spmv_c_gen_uniform_ell(uint64_t seed, int rows, int n_cols, int k, int32_t* d_cols, float* d_vals,
                           void* hip_stream) {
    return detail::gen_uniform_ell(seed, rows, n_cols, k, d_cols, d_vals, as_stream(hip_stream));
}

int spmv_c_gen_stratified_rows(uint64_t seed, int row_begin, int local_rows, int n_cols,
                               const int32_t* d_row_ptrs, int32_t* d_cols, float* d_vals,
                               void* hip_stream) {
    return detail::gen_stratified_rows(seed, row_begin, local_rows, n_cols, d_row_ptrs, d_cols,
                                       d_vals, as_stream(hip_stream));
}

int spmv_c_gen_vector(uint64_t seed, uint64_t tag, size_t n, float* d_x, void* hip_stream) {
    return detail::gen_vector(seed, tag, n, d_x, as_stream(hip_stream));
}

int spmv_c_count_columns(int64_t nnz, const int32_t* d_cols, int n_cols, int32_t* d_counts,
                         void* hip_stream) {
    return detail::count_columns(nnz, d_cols, n_cols, d_counts, as_stream(hip_stream));
}

int spmv_c_reciprocal_values(int64_t nnz, const int32_t* d_cols, const int32_t* d_counts,
                             float* d_vals, void* hip_stream) {
    return detail::reciprocal_values(nnz, d_cols, d_counts, d_vals, as_stream(hip_stream));
}

} // extern "C"
