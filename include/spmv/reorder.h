// spmv/reorder.h — multicolour reordering: a device graph colouring, the permutation it defines, the symmetric
// permutation of a CSR matrix on the device, and the gather that carries vectors in and out of the new numbering.
//
// Why: sptrsv_csr, ilu0_csr, ic0_csr and the solvers built on them run over the level schedule of the matrix as it
// arrives, and a grid matrix in natural ordering has O(n^(1/2)) or O(n^(1/3)) levels, one launch each.  Colour the
// graph of A so that no two adjacent rows share a colour, renumber the rows colour by colour, and in P A P^T every
// dependency level of either triangle is a whole colour class: the level count falls to the number of colours.
// Nothing in the solvers, factorisations or schedules changes; they are handed a better-ordered matrix
// (gpu-spmv_amd/csrc/reorder.hip, reorder_host.cpp; the recipe is in INTEGRATION.md).
// The second half of the file is the ordering for the opposite need, locality: reverse Cuthill-McKee (csr_rcm,
// rcm_reorder) and the band statistics that show what it bought (csr_band_gpu).
#ifndef SPMV_REORDER_H
#define SPMV_REORDER_H

#include "common.h"
#include "csr_matrix.h"

namespace spmv {

struct ColorConfig {
    unsigned seed;           // of the vertex priorities
    int symmetric_pattern;   // 1: the caller promises that A stores (u, v) whenever it stores (v, u); only A is walked
    int lanes_per_row;       // lanes that share a row: 0 = from the mean degree, else 1, 2, 4, ... 64
    int reserved;            // 0
    ColorConfig() : seed(0u), symmetric_pattern(0), lanes_per_row(0), reserved(0) {}
};

struct ColorResult {
    int   error_code;    // SpMVError as int
    int   num_colors;    // 1 + the largest colour (0 for a matrix without rows)
    int   rounds;        // rounds in which some vertex took its colour
    int   launches;      // kernel launches of the call (the transpose build of symmetric_pattern = 0 not counted)
    float elapsed_ms;    // device-event time of the colouring itself: after the structure pass and the transpose build
    ColorResult() : error_code(0), num_colors(0), rounds(0), launches(0), elapsed_ms(0.0f) {}
};

// Colours the graph of the square matrix A (resident on the device) into d_colors (num_rows ints on the device).
//
// Graph: the vertices are the rows; u and v are adjacent when u != v and A stores (u, v) or (v, u).  Stored
// diagonals and repeated entries change nothing; the values are never read.  With symmetric_pattern = 0 the rows of A
// and of A^T are walked (the pattern of A^T is built by the device transpose and freed before the call returns).
// With symmetric_pattern = 1 only A's rows are walked: u counts as a neighbour of v only when row v stores u.  If the
// promise is broken the result is still DEFINED (it is what csr_color_cpu gives with the same config) but it may not
// be a proper colouring: two adjacent vertices may share a colour.
//
// Rule: the priority of vertex i is the pair (fmix32(i ^ seed), i), compared lexicographically, larger first, with
// fmix32(h): h ^= h >> 16; h *= 0x85ebca6b; h ^= h >> 13; h *= 0xc2b2ae35; h ^= h >> 16 (mod 2^32).  The colouring is
// greedy first-fit in descending priority: every vertex takes the smallest colour >= 0 that none of its
// higher-priority neighbours holds.  csr_color_cpu computes exactly that, sequentially, and is the definition;
// csr_color gives the same ints on every input, every run, every stream, every lanes_per_row and every seed.
//
// Device algorithm (Jones-Plassmann, in rounds): an uncoloured vertex takes its colour in a round in which every
// higher-priority neighbour already has one.  No workgroup waits for another; rounds are enqueued in batches and the
// count of vertices left is read once per batch.  result.rounds <= the synchronous round count csr_color_cpu reports
// (a vertex may see a neighbour's colour of the same round); it is not part of the bitwise contract.
//
// Checks, in this order; nothing is written to d_colors when one fails: null A or d_colors -> INVALID_ARGUMENT;
// num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS with 0 colours; missing device arrays (the rule
// of csr_transpose_gpu) -> INVALID_FORMAT; lanes_per_row not 0 or a power of two <= 64 -> INVALID_ARGUMENT;
// reserved != 0 -> INVALID_ARGUMENT; then ONE device pass over the structure: row_ptrs[0] == 0, non-decreasing,
// row_ptrs[num_rows] == nnz, every column in [0, num_rows), else INVALID_FORMAT.
// Runs on the library stream (spmv_set_stream) and returns after the colouring completed.
ColorResult csr_color(const CSRMatrix* A, int* d_colors, const ColorConfig* config = nullptr);

// The definition, on A's HOST arrays: colors[num_rows]; *num_colors and *rounds (either may be null) receive the
// number of colours and the round count of the synchronous algorithm (round(v) = 1 + the largest round of v's
// higher-priority neighbours, 1 without any; *rounds is the largest).  config->lanes_per_row is checked and otherwise
// ignored.  Checks: null A or colors -> INVALID_ARGUMENT; not square -> INVALID_DIMENSION; no rows -> SUCCESS; missing
// host arrays -> INVALID_ARGUMENT; lanes_per_row, reserved as above; malformed arrays (csr_color's structure rule) ->
// INVALID_FORMAT.  colors is untouched on any error.
int csr_color_cpu(const CSRMatrix* A, int* colors, int* num_colors, int* rounds, const ColorConfig* config = nullptr);

// The ordering a colouring defines, by a stable counting sort on the device: the vertices sorted by (colour, index),
// which makes it unique.  d_perm[new] = old and d_inverse[old] = new (n ints each, device); color_ptr (HOST,
// num_colors + 1 ints, may be null): the new indices [color_ptr[c], color_ptr[c + 1]) hold colour c.
// Checks: null d_colors / d_perm / d_inverse, n < 0 or num_colors < 0 -> INVALID_ARGUMENT; n == 0 -> SUCCESS
// (color_ptr all zero); a colour outside [0, num_colors) -> INVALID_ARGUMENT, found on the device before anything is
// written.  Runs on the library stream and returns after it completed.
int color_ordering(int n, const int* d_colors, int num_colors, int* d_perm, int* d_inverse, int* color_ptr);

// B = P A Q^T on the device with sorted rows: row i of B is row d_row_perm[i] of A with every column j renamed
// d_col_inverse[j], ordered by new column ascending; equal columns keep A's storage order.  Either array may be null:
// the identity.  A may be rectangular: d_row_perm has num_rows entries, d_col_inverse num_cols.  Values are copied,
// never combined: B is bit for bit csr_permute_cpu's (-0.0, NaN payloads, explicit zeros and duplicates kept).  With
// d_row_perm = perm and d_col_inverse = inverse of color_ordering this is P A P^T.  No atomics: the same bytes on every
// run.  B ends up as csr_transpose_gpu leaves AT: it owns new device arrays (what it owned before is released), its
// host arrays are allocated at the new size and hold no data until csr_from_gpu(B).
// Checks: null B or A -> INVALID_ARGUMENT; B == A -> INVALID_ARGUMENT; missing device arrays -> INVALID_FORMAT; then
// on the device, before B is touched: A's structure (csr_transpose_gpu's rule) -> INVALID_FORMAT; an array that is
// not a permutation (an index out of range or repeated) -> INVALID_ARGUMENT; allocation failure -> CUDA_MALLOC.
// Runs on the library stream and returns after the build completed.
int csr_permute_gpu(CSRMatrix* B, const CSRMatrix* A, const int* d_row_perm, const int* d_col_inverse);

// The same on HOST arrays (A's and the two index arrays): the definition of the order.  B owns new host arrays; a
// device copy it held is released.  Checks: null B or A, B == A, missing host arrays -> INVALID_ARGUMENT; malformed
// arrays -> INVALID_FORMAT; not a permutation -> INVALID_ARGUMENT; B is untouched on any error.
int csr_permute_cpu(CSRMatrix* B, const CSRMatrix* A, const int* row_perm, const int* col_inverse);

// out[i * ldo + j] = in[index[i] * ldi + j] for i < n, j < k: the rows of an n x k row-major array (spmv_csr_multi's
// layout, leading dimensions ldo, ldi >= k, 1 <= k <= 32) gathered through d_index, whose entries the caller
// guarantees to lie in [0, n).  With d_perm it forms P b, with d_inverse it brings x back.  Columns k..ldo-1 of d_out
// are never written.  Checks: null pointers, n < 0, k < 1 or k > 32, ldo < k or ldi < k -> INVALID_ARGUMENT; the
// ranges d_out[0, (n - 1) * ldo + k) and d_in[0, (n - 1) * ldi + k) overlapping -> INVALID_ARGUMENT; n == 0 ->
// SUCCESS.  Runs on the library stream and returns after it completed.
int permute_gather(float* d_out, int ldo, const float* d_in, int ldi, const int* d_index, int n, int k);

// The same enqueued on `stream` without a synchronisation.
int permute_gather_async(float* d_out, int ldo, const float* d_in, int ldi, const int* d_index, int n, int k,
                         hipStream_t stream);

// The three together: colours A (csr_color with `config`), orders the vertices (color_ordering into d_perm and
// d_inverse, num_rows ints each on the device) and forms B = P A P^T (csr_permute_gpu).  The result is csr_color's;
// error_code is that of the first step that failed, and B, d_perm and d_inverse are untouched unless all succeeded
// (d_perm and d_inverse may have been written when only the last step failed).  In B, sptrsv_analyze reports
// num_levels == num_colors for LOWER and for UPPER.  Checks: null B / A / d_perm / d_inverse -> INVALID_ARGUMENT;
// B == A -> INVALID_ARGUMENT; then csr_color's.
ColorResult multicolor_reorder(CSRMatrix* B, const CSRMatrix* A, int* d_perm, int* d_inverse,
                               const ColorConfig* config = nullptr);

// ---- reverse Cuthill-McKee: the ordering for locality (gpu-spmv_amd/csrc/rcm.hip, rcm_host.cpp) ----
// The multicolour ordering above shortens level schedules and pays with locality.  This one does the opposite: it
// pulls the entries of P A P^T towards the diagonal, so that the x gather of a row stays inside a few cache lines and
// the ILU(0) / IC(0) factors of a mesh that arrived in an arbitrary numbering are those of a banded matrix.

struct RcmConfig {
    int symmetric_pattern;   // as ColorConfig: 1 = only A's rows are walked (the caller promises a symmetric pattern)
    int peripheral;          // 1: a George-Liu pseudo-peripheral start per component; 0: start at the rule's minimum vertex
    int lanes_per_row;       // lanes that share a row: 0 = from the mean degree, else 1, 2, 4, ... 64
    int reserved;            // 0
    RcmConfig() : symmetric_pattern(0), peripheral(1), lanes_per_row(0), reserved(0) {}
};

struct RcmResult {           // 24 bytes
    int   error_code;    // SpMVError as int
    int   components;    // components numbered, every isolated vertex one of them
    int   levels;        // levels of the final level structures, summed over the components
    int   sweeps;        // level structures the device built, the search's included (isolated vertices need none)
    int   launches;      // kernel launches of the call's own loop (the builders of the symmetrised matrix not counted)
    float elapsed_ms;    // device-event time of that loop
    RcmResult() : error_code(0), components(0), levels(0), sweeps(0), launches(0), elapsed_ms(0.0f) {}
};

// The reverse Cuthill-McKee ordering of the square matrix A (resident on the device): d_perm[new] = old and
// d_inverse[old] = new (num_rows ints each on the device), color_ordering's conventions, so csr_permute_gpu and
// permute_gather take them unchanged.
//
// Input: every row's columns strictly ascending (csr_add's rule; csr_row_indices_gpu + csr_from_coo_gpu of
// spmv/assemble.h normalise a matrix that is not).  The values are never read.
// Graph: adj(v) = the columns u != v stored in row v and, with symmetric_pattern = 0, also the rows u != v that store
// v.  deg(v) = |adj(v)|, key(v) = (deg(v), v), compared lexicographically, smaller first.
// Rule (csr_rcm_cpu computes exactly this, sequentially, and is the definition): while some vertex is unnumbered, let
// r be the unnumbered vertex of smallest key.  With peripheral = 1: build the rooted level structure L(r) over the
// unnumbered vertices, let c be the vertex of smallest key in its last level, and if L(c) has more levels than L(r)
// set r = c and repeat; otherwise stop.  Then Cuthill-McKee from r: a queue that starts as (r); when u is dequeued its
// unnumbered neighbours are appended in ascending key.  The vertices are numbered in queue order, after those of the
// earlier components; the final order is the reverse of the whole sequence.  An isolated vertex is a component of its
// own, and the isolated vertices come first in index order (last after the reversal).  With symmetric_pattern = 1 and a
// pattern that is not symmetric the same words apply to the directed graph: the result is what csr_rcm_cpu gives, a
// permutation that need not reduce anything.
// csr_rcm gives the same ints on every input, every run, every stream and every lanes_per_row.
//
// Device algorithm: S = the pattern of A + A^T (csr_transpose_gpu, csr_add; A itself with symmetric_pattern = 1);
// D = the vertices by key, a stable counting sort by degree (color_ordering); S' = D S D^T (csr_permute_gpu), in whose
// numbering the smallest key is the smallest index and every row lists its neighbours in key order.  A level structure
// is then built level by level: an integer atomicMin gives every vertex of the next level its parent, the earliest
// position of the level before that stores it; every parent counts its children, a scan of the counts in position
// order gives each parent its slice of the next level, and a child's rank inside the slice is the count of its
// parent's children to its left in the row.  That is the queue order.  Runs of levels of at most 256 vertices are
// numbered by one workgroup in one launch, wider levels by four grid-wide launches each.  No workgroup waits for
// another.  Rounds are enqueued in batches and a small state is read back after each; the search's decisions are taken
// on the device.  Cost: the loop runs per component and per level, so a matrix with very many non-trivial components,
// or a very long thin one, costs launches and round trips in proportion; result.components and result.launches
// report it.  Nothing of size n or nnz crosses the bus.
//
// Checks, in this order; nothing is written to d_perm or d_inverse when one fails: null A / d_perm / d_inverse ->
// INVALID_ARGUMENT; num_rows != num_cols -> INVALID_DIMENSION; num_rows == 0 -> SUCCESS; missing device arrays ->
// INVALID_FORMAT; lanes_per_row not 0 or a power of two <= 64 -> INVALID_ARGUMENT; peripheral not 0 or 1 ->
// INVALID_ARGUMENT; reserved != 0 -> INVALID_ARGUMENT; then on the device: csr_color's structure rule, and every
// column strictly above its left neighbour, else INVALID_FORMAT.  A loop that stops making progress (it cannot) gives
// KERNEL_LAUNCH, never a hang.  Runs on the library stream and returns after the ordering completed.
RcmResult csr_rcm(const CSRMatrix* A, int* d_perm, int* d_inverse, const RcmConfig* config = nullptr);

// The definition, on A's HOST arrays: perm[num_rows], inverse[num_rows]; *components and *levels (either may be null)
// as in RcmResult.  config->lanes_per_row is checked and otherwise ignored.  Checks: null A / perm / inverse ->
// INVALID_ARGUMENT; not square -> INVALID_DIMENSION; no rows -> SUCCESS; missing host arrays -> INVALID_ARGUMENT;
// lanes_per_row, peripheral, reserved as above; malformed arrays or a row that is not strictly ascending ->
// INVALID_FORMAT.  perm and inverse are untouched on any error.
int csr_rcm_cpu(const CSRMatrix* A, int* perm, int* inverse, int* components, int* levels,
                const RcmConfig* config = nullptr);

// csr_rcm, then B = P A P^T (csr_permute_gpu).  The result is csr_rcm's; error_code is that of the first step that
// failed, and B is untouched unless both succeeded (d_perm and d_inverse have been written when only the permutation
// failed).  Checks: null B / A / d_perm / d_inverse -> INVALID_ARGUMENT; B == A -> INVALID_ARGUMENT; then csr_rcm's.
RcmResult rcm_reorder(CSRMatrix* B, const CSRMatrix* A, int* d_perm, int* d_inverse, const RcmConfig* config = nullptr);

// How far the stored entries of A lie from the diagonal: lower = max(i - j) and upper = max(j - i) over the stored
// entries (i, j) (0 without any), profile = the sum over the rows of i - min(i, smallest stored column of row i) (a
// row without entries adds 0).  A may be rectangular and its rows unsorted.  Integers throughout: the two calls agree
// exactly.  (Not to be confused with spmv/bandwidth.h, which models bytes moved.)
struct CsrBand {             // 16 bytes
    int lower;
    int upper;
    long long profile;
};
// A on the device.  Checks: null A or out -> INVALID_ARGUMENT; missing device arrays (csr_transpose_gpu's rule) ->
// INVALID_FORMAT; then the structure on the device -> INVALID_FORMAT; *out is written on SUCCESS only.  Runs on the
// library stream and returns after it completed.
int csr_band_gpu(const CSRMatrix* A, CsrBand* out);
// A's host arrays.  Checks: null A or out, negative sizes, missing host arrays -> INVALID_ARGUMENT; malformed arrays
// -> INVALID_FORMAT.
int csr_band_cpu(const CSRMatrix* A, CsrBand* out);

} // namespace spmv

#endif
