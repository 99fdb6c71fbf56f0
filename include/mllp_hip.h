/*
 * mllp_hip.h -- C ABI of libmllp_hip.so: the MI355X (gfx950) implementation of mllp's learned-LP
 * hot path (bipartite TransformerConv message passing over the LP constraint matrix, forward and
 * backward, fused BCE head, flat Adam).
 *
 * The reference (HAHHHD/mllp) has no FFI/plugin interface: it is pure Python on PyTorch +
 * PyTorch-Geometric.  The boundary a maintainer binds is therefore this
 * header, loaded with ctypes from the Python modules that keep the reference's names
 * (INTEGRATION.md shows the stub).  Each entry point cites the reference lines it replaces
 * (paths relative to the reference root).
 *
 * Conventions
 *   - every function returns 0 on success, a negative MLLP_E* code on failure;
 *     mllp_last_error() returns a thread-local message for the last failure on this thread.
 *   - "device pointer" arguments are caller-owned HIP device memory (e.g. torch tensors); the
 *     library never frees or reallocates them and allocates nothing after mllp_graph_create_*.
 *   - every launch is asynchronous on the hipStream_t passed as `stream` (void*; NULL = default
 *     stream); no entry point synchronises except mllp_graph_create_* / mllp_graph_export.
 *   - all launch functions are hipGraph-capturable (no malloc/free/sync inside).
 *   - the sparsity pattern of a mllp_graph_t is immutable after creation; its values change only through
 *     mllp_graph_set_values / mllp_graph_scale_values / mllp_graph_normalize / mllp_graph_plant_basis.  An internal scratch buffer is used by
 *     rows that are split over several workgroups: calls on ONE graph must be stream-ordered.
 *   - feature width is fixed at 16 (reference linear_program_methods.py:206-211), fp32 everywhere.
 *   - there is NO CPU fallback: without a HIP device every launch function fails with MLLP_EHIP.
 */
#ifndef MLLP_HIP_H
#define MLLP_HIP_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define MLLP_ABI_VERSION 6 /* 2: streamed SpMM copy, device-built tiled copies, mllp_gnn_train_step, mllp_graph_invalidate_inputs; 3: streamed copies of the attention sweeps (mllp_graph_*_stream_copy); 4: input gradients (mllp_gnn_backward_inputs); 5: AngleModel input gradients (mllp_angle_backward_inputs); 6: the predicted basis (mllp_topm_select, mllp_topm_select_dense); mllp_graph_set_values, _set_values_bytes and _scale_values arrived after 6 WITHOUT a bump: they are additions only (no existing export changed signature or meaning), so every caller built against 6 stays valid; a caller that needs them checks for the symbols; mllp_graph_normalize and mllp_normalize_row_tier likewise; mllp_graph_plant_basis, mllp_lp_certificate and mllp_lp_certificate_scratch_bytes likewise; mllp_basis_repair and mllp_basis_repair_scratch_bytes likewise */
#define MLLP_FEAT 16
#define MLLP_NUM_PARAMS 4721 /* GNNModel.state_dict(), SURVEY.md appendix A.2 */

#define MLLP_OK 0
#define MLLP_EINVAL (-1) /* bad argument (null pointer, shape mismatch, unsorted indices, ...) */
#define MLLP_EHIP (-2)   /* a HIP runtime call failed (message has hipGetErrorString) */
#define MLLP_ENOMEM (-3)
#define MLLP_ERANGE (-4) /* sizes exceed int32 indexing */

typedef struct mllp_graph mllp_graph_t;

const char* mllp_last_error(void);
int mllp_abi_version(void);

/* ------------------------------------------------------------------------------------------------
 * Graph: a block-diagonal batch of LP constraint matrices, resident in HBM in both orientations.
 * Replaces the per-step Python graph build `build_graph_from_weights_sets`
 * (linear_program_methods.py:89-103) and the batching rule `BipartiteData.__inc__`
 * (linear_program_methods.py:60-72): variable ids of instance k are offset by sum_{j<k} n_j,
 * constraint ids by sum_{j<k} m_j.  Built ONCE; the reference rebuilds it every step
 * (linear_program_experiment.py:124).
 * ---------------------------------------------------------------------------------------------- */

/* From host CSR pieces exactly as the reference loader returns them
 * (linear_program_data.py:75-77: scipy CSR indptr/indices/data per instance).
 *   indptr  : concatenation over instances of (m_k + 1) LOCAL row offsets (each block starts at 0)
 *   indices : concatenation of LOCAL column ids (row-major, sorted within a row, no duplicates)
 *   values  : float64 entries a_ij (cast to fp32 as linear_program_methods.py:100 does)
 *   tier_wave, tier_block : rows with more than tier_wave nonzeros are processed by one 64-lane
 *     wavefront, more than tier_block by 256-thread workgroups (one per chunk of at most
 *     4 * tier_block nonzeros; longer rows are split and merged); 0 = choose automatically.    */
int mllp_graph_create_host(int64_t n_inst, const int64_t* inst_m, const int64_t* inst_n,
                           const int64_t* indptr, const int32_t* indices, const double* values,
                           int32_t tier_wave, int32_t tier_block, mllp_graph_t** out);

/* From device arrays that already hold the batch in global ids, both orientations (CSR of A:
 * rows = constraints; CSR of A^T: rows = variables, row ids ascending within a column).  The
 * arrays are copied.  inst_ptr_m / inst_ptr_n are HOST arrays of n_inst + 1 offsets.           */
/* CSR(A) -> CSR(A^T) on the device (counting + scatter + per-column ordering by row id: the one stable transposition,
 * whatever order the scatter's atomics produced; mllp_amd/csrc/transpose.hip): the second orientation that
 * mllp_graph_create_device wants, for batches that were generated or loaded on the GPU.  All arrays are caller-owned
 * device memory: d_ptr [n_rows + 1], d_idx / d_val [nnz] (column ids ascending inside a row), outputs d_t_ptr
 * [n_cols + 1], d_t_idx / d_t_val [nnz].  Allocates scratch and synchronises `stream` (not a launch function).
 * The input is checked on the device first: d_ptr must ascend from 0 to nnz and the column ids of a row must be
 * strictly ascending and smaller than n_cols (no duplicate entries, which the per-column ordering could not keep
 * apart); anything else returns MLLP_EINVAL and writes nothing.                                                */
int mllp_csr_transpose_device(int64_t n_rows, int64_t n_cols, int64_t nnz, const int32_t* d_ptr, const int32_t* d_idx,
                              const float* d_val, int32_t* d_t_ptr, int32_t* d_t_idx, float* d_t_val, void* stream);

int mllp_graph_create_device(int64_t n_inst, const int64_t* inst_ptr_m, const int64_t* inst_ptr_n,
                             int64_t nnz,
                             const int32_t* d_csr_ptr, const int32_t* d_csr_idx, const float* d_csr_val,
                             const int32_t* d_csc_ptr, const int32_t* d_csc_idx, const float* d_csc_val,
                             int32_t tier_wave, int32_t tier_block, void* stream, mllp_graph_t** out);

int mllp_graph_destroy(mllp_graph_t* g);

/* dims[0..11] = M (constraints), N (variables), nnz, n_inst,
 *               group-tier rows / wave-tier rows / chunk work items for A (dst = constraints),
 *               the same three for A^T (dst = variables),
 *               rows split over several chunks for A, for A^T                                  */
int mllp_graph_dims(const mllp_graph_t* g, int64_t dims[12]);

/* Copy one device array of the graph back to host memory (synchronises; tests/debugging).
 * which: 0 csr_ptr(int32,M+1) 1 csr_idx(int32,nnz) 2 csr_val(f32,nnz)
 *        3 csc_ptr(int32,N+1) 4 csc_idx(int32,nnz) 5 csc_val(f32,nnz) 6 inv_n(f32,N)            */
int mllp_graph_export(const mllp_graph_t* g, int which, void* host_dst, int64_t capacity_bytes);

/* Which kernels the whole-model entry points (mllp_gnn_forward / _backward / _loss_step) use:
 *   0  by size (default): the fused latency-regime kernels below 32 M nonzeros (real Netlib: one sweep launch
 *      per conv forward, two backward, 16 rows per wavefront), the generic / LDS-tiled sweeps above;
 *   1  always the generic / LDS-tiled sweeps;   2  always the fused kernels.
 * Both paths compute the same quantities (tests compare them with each other and with the oracle).        */
int mllp_graph_set_path(mllp_graph_t* g, int path);

/* Grid of the fused sweeps (symbols added without an ABI bump: callers check for them, as for mllp_graph_set_values).
 * Process-wide cap on the workgroups of the fused sweeps, for graphs created AFTER the call:
 *   G = max(min(device CUs, STAT_BLOCKS_MAX = 256, limit) / 8, 1) * 8.
 * 0 means no limit.  It can only lower the grid: a limit above the device's CU count changes nothing, so every
 * workgroup stays resident as today.  Needs no GPU.  Negative: MLLP_EINVAL.  *previous (may be NULL) receives the
 * old value.  A graph keeps the limit it was created under, also when its fused arrays are built later by
 * mllp_graph_set_path(g, 2).  What it is for, and what it does not reproduce of a partitioned device: DESIGN.md. */
int mllp_set_fused_grid_limit(int64_t workgroups, int64_t* previous);

/* info = {G of this graph's fused sweeps, partitions (8), device CUs, the limit in force when it was created}.
 * A null argument is refused.  G is reported as the rule gives it even while the fused arrays are not built. */
int mllp_graph_fused_grid(const mllp_graph_t* g, int64_t info[4]);

/* INPUT CONTRACT of the whole-model entry points on the fused path: the graph keeps renumbered copies of d_x1, d_x2
 * and d_labels (and the layer-1 source features gathered beside the nonzeros), keyed on the POINTER VALUES -- the
 * model's inputs are data (linear_program_methods.py:90-91), constant for the life of a batch.  A caller that changes
 * their contents in place, or frees a buffer and gets the same address back for other data, must call
 * mllp_graph_invalidate_inputs before the next mllp_gnn_* call on this graph (the generic / tiled path reads the
 * pointers on every call and needs nothing).  Calls made while the stream is captured into a hipGraph re-make the
 * copies inside the capture and leave the cache empty.  A replay of such a hipGraph rewrites the graph's copies from ITS
 * buffers whenever the caller launches it, unseen by the library: from the first captured call on, and until
 * mllp_graph_destroy, every call on this graph re-makes the copies (up to five small launches) and the pointer cache is not
 * trusted again, so eager calls and replays on different buffers may alternate freely.  mllp_gnn_backward must follow an mllp_gnn_forward on the same
 * workspace with the same path (MLLP_EINVAL otherwise: the two paths lay the workspace out differently).          */
int mllp_graph_invalidate_inputs(mllp_graph_t* g);

/* New matrix values on the unchanged sparsity pattern, in place and on the device (mllp_amd/csrc/set_values.hip): what
 * a step on dL/da (mllp_gnn_backward_inputs), a family of LPs that share a pattern, or a row / column rescaling needs,
 * without building the batch again.
 *   d_val : nnz floats in the graph's CSR(A) order -- the order of mllp_graph_export(g, 2, ...) and of d_dvalues.
 * After the call EVERY array of the graph that holds values holds the new ones: both CSR orientations, the fused
 * path's renumbered entries (and the value half of its gathered layer-1 inputs, so bound inputs stay bound), every
 * streamed copy (geometries 0-4) and every library-built LDS-tiled copy, byte for byte what a fresh build from d_val
 * would hold; indices, pointers and padding are not touched.  Explicit zeros are values like any other; nothing inspects
 * the values.  Deterministic: gathers through int32 position maps, one writer per word, no atomics.
 * The maps (CSR(A^T) -> CSR(A), shared with mllp_gnn_backward_inputs, and one per re-blocked copy) are library-owned and
 * built lazily: the FIRST call, and the first call after a copy was built, allocate and synchronise `stream` (make
 * them outside a capture).  Every other call is a launch function: one device-to-device copy + one launch per array on
 * `stream` alone, no allocation, no synchronisation, hipGraph-capturable.  A map is freed with its copy (drop / rebuild)
 * and with the graph.  mllp_graph_set_values_bytes: bytes of the maps of the copies attached now, built or not yet.
 * The workspace record (RECORDS, below) is cleared: mllp_gnn_backward* needs a new mllp_gnn_forward (MLLP_EINVAL
 * otherwise; a captured call clears it when it is captured, not when it is replayed).  The folded weights are kept.
 * MLLP_EINVAL, before anything is written: null g or d_val; a caller-owned LDS-tiled copy is attached
 * (mllp_graph_attach_tiled) -- drop it or build it with mllp_graph_build_tiled.
 * mllp_graph_scale_values: a_ij <- (r_i a_ij) s_j in fp32, in that order, i the constraint and j the variable of the
 * nonzero; d_row_scale [M], d_col_scale [N], either may be NULL (all ones).  For positive r, s the LP (R A S, S c, R b)
 * has the optimal basis of (A, c, b): scaling x1 = c and x2 = b is the caller's business (they are the caller's
 * buffers, then mllp_graph_invalidate_inputs).  Works into a library-owned scratch array of nnz floats (allocated by the
 * first call, counted by _set_values_bytes from then on), then refreshes as mllp_graph_set_values does.         */
int mllp_graph_set_values(mllp_graph_t* g, const float* d_val, void* stream);
int mllp_graph_set_values_bytes(const mllp_graph_t* g, int64_t* bytes);
int mllp_graph_scale_values(mllp_graph_t* g, const float* d_row_scale, const float* d_col_scale, void* stream);

/* The reference's normalization of the resident batch, in place and on the device (mllp_amd/csrc/normalize.hip): the
 * stage that made the tensors the reference's loader reads (linear_program_data.py:58-80, `netlib_mps_norm`), whose rule
 * is restated in oracle/mps_norm.py `normalize`.  It puts a batch whose coefficients were made or changed on the device
 * (mllp_graph_create_device, _set_values, _scale_values, a step along dL/da) back on the distribution the weights were
 * trained on, without the host round trip and the rebuild.  In fp32:
 *   rows       q_i = sum_j a_ij^2,  s_i = 1 / sqrt(q_i), or 1 for an empty or all-zero row; then, with the cap enabled,
 *              where |b_i s_i| > rhs_cap:  s_i = rhs_cap / b_i -- SIGNED: a negative b_i flips the whole row, and every
 *              capped row ends at right-hand side +rhs_cap (an empty row with b_i beyond the cap included).
 *              rhs_cap <= 0, +inf or NaN disables the cap; the reference's value is 5.
 *   objective  t_k = 1 / ||x1[instance k]||_2, or 1 for a zero or empty objective.
 *   apply      x2_i <- b_i s_i,  x1_j <- c_j t_k,  a_ij <- s_i a_ij as mllp_graph_scale_values(g, s, NULL) does: every
 *              value-holding array of the graph is refreshed with the guarantees of mllp_graph_set_values (byte for byte a
 *              fresh build from the new values; the workspace record is cleared, so mllp_gnn_backward* needs a new
 *              mllp_gnn_forward; the folded weights are kept), and the graph's copies of the inputs are invalidated as by
 *              mllp_graph_invalidate_inputs, because d_x1 / d_x2 were just written.
 *   d_x1 [N], d_x2 [M] : the batch's objective coefficients and right-hand sides (the inputs of mllp_gnn_*), caller-owned.
 *   d_row_scale [M], d_obj_scale [n_inst] : receive the applied s_i and t_k (what carries duals or a solution back to the
 *              original units); NULL = library-owned scratch (M + n_inst floats, allocated by the first call and counted by
 *              mllp_graph_set_values_bytes from then on).
 *   flags      bit 0 = compute only: the scales are written (both output pointers are then required) and nothing else is
 *              written, invalidated or cleared.  Other bits must be 0.
 * Deterministic and batch-independent: no atomics, and the order in which a row's squares are added depends on that
 * row's nonzero count alone (mllp_normalize_row_tier: 0 = a 16-lane group up to 64 nonzeros, 1 = a wavefront up to 1024,
 * 2 = a workgroup), an objective's on n_k alone -- an instance gets the same bits alone and inside any batch.
 * A row whose |b_i| / ||row_i|| equals the cap to within fp32 rounding may fall on either side of the comparison; with
 * b_i < 0 the two sides differ by the sign of the row.
 * MLLP_EINVAL, before anything is written (d_x1 and d_x2 included): null g, d_x1 or d_x2; bit 0 with a null output;
 * unknown flag bits; a caller-owned LDS-tiled copy is attached (the condition of mllp_graph_set_values).
 * The FIRST call may allocate and synchronise like mllp_graph_set_values' (make it outside a capture); every later call
 * is a launch function: `stream` only, no allocation, no synchronisation, hipGraph-capturable (a captured call
 * invalidates and clears when it is captured, not when it is replayed).  Like _set_values it arrived after ABI 6 without
 * a bump: an addition only.                                                                                       */
int mllp_graph_normalize(mllp_graph_t* g, float* d_x1, float* d_x2, float rhs_cap, int flags, float* d_row_scale,
                         float* d_obj_scale, void* stream);
int mllp_normalize_row_tier(int64_t row_nnz, int* tier);

/* Planted-basis LPs: a labelled training batch made where the batch lives (mllp_amd/csrc/planted.hip).  The LP is that of
 * the normalized tensors, min c'x, Ax = b, x >= 0 with slack columns as ordinary columns; x1 = c, x2 = b, labels = 1 on
 * the m columns of the basis.  Given one pivot per row, a primal point, a dual point and dual slacks, the resident batch
 * is rewritten so that the pivots' columns are its unique optimal basis, in fp32:
 *   basic_j = 1 iff j is some row's pivot.
 *   row i, over its entries in CSR order:  off_i = sum |a_ij| and rest_i = sum a_ij xstar_j over the basic j != pivot[i];
 *              the pivot entry becomes copysign(dominance * off_i + floor, its old value);
 *              b_i = fma(new pivot value, xstar[pivot[i]], rest_i).  No other value changes by a bit.
 *   column j, over CSR(A^T) with the new values:  c_j = sum_i a_ij ystar_i + (basic_j ? 0 : slack_j);  labels_j = basic_j.
 * The basis matrix is strictly row-diagonally dominant under the pivot ordering, hence nonsingular with
 * ||B^-1||_inf <= 1 / min_i(|d_i| - off_i); with xstar > 0 on the basic and slack > 0 on the nonbasic columns the point
 * (xstar * basic, ystar) is primal and dual feasible and strictly complementary, so the basis is the unique optimum.
 * Nothing inspects xstar, ystar or slack: their signs are the caller's business (mllp_lp_certificate reports on them).
 *   d_pivot [M] int32 : the global column id of every row's pivot; the entry (i, pivot[i]) must exist in the pattern (rows
 *              ascending, as every builder of this library leaves them) and no column may be the pivot of two rows.
 *   d_xstar [N], d_ystar [M], d_slack [N] : inputs, never written.   dominance > 1, floor > 0, both finite.
 *   d_x1 [N], d_x2 [M], d_labels [N] : outputs, every element written; what they held does not matter.
 * A SETUP call, not a launch function: d_pivot is validated on the device first and `stream` is synchronised; a bad pivot
 * gives MLLP_EINVAL with a message before a byte of the caller's buffers or of the graph's values is written.  The new
 * values go through the library's scratch of nnz floats (that of mllp_graph_scale_values) and every value-holding array
 * of the graph is refreshed with the guarantees of mllp_graph_set_values; the graph's copies of the inputs are
 * invalidated as by mllp_graph_normalize.  Library scratch of N + M + 2 int32 is allocated by the first call and counted
 * by mllp_graph_set_values_bytes from then on.
 * MLLP_EINVAL before any HIP call: a null argument; dominance <= 1, floor <= 0 or either not finite; a caller-owned
 * LDS-tiled copy is attached (the condition of mllp_graph_set_values).
 * Deterministic and batch-independent: the sums take mllp_graph_normalize's three tiers and order, which depend on the
 * row's (column's) nonzero count alone; a term the rule leaves out is skipped in place.  No float atomics, one writer
 * per word.  Under the MEMORY CONTRACT below.  Added after ABI 6 without a bump, as mllp_graph_set_values was.
 *
 * mllp_lp_certificate: what a claimed optimal solution (x, y, basis) of the resident batch is worth, per instance, from
 * two sparse sweeps over the stored data -- the planted labels, Netlib's, or a solver's output.  A launch function:
 * `stream` only, no allocation, no synchronisation, hipGraph-capturable.
 *   d_x1 [N] = c, d_x2 [M] = b, d_x [N], d_y [M], d_basis [N] (0 = nonbasic, anything else = basic) : inputs.
 *   d_scratch : mllp_lp_certificate_scratch_bytes() bytes.     d_cert [n_inst, 6], per instance:
 *     0  max_i |sum_j a_ij x_j - b_i|             primal residual (0 without rows)
 *     1  min x_j over basic j                      (+inf without basic columns)
 *     2  max |x_j| over nonbasic j                 (0 without nonbasic columns)
 *     3  min (c_j - sum_i a_ij y_i) over nonbasic j   the smallest reduced cost (+inf without nonbasic columns)
 *     4  max |c_j - sum_i a_ij y_i| over basic j   complementarity (0 without basic columns)
 *     5  sum_j basis_j
 * The per-row and per-column sums take the fixed order above; the reductions over an instance are max / min.        */
int mllp_graph_plant_basis(mllp_graph_t* g, const int* d_pivot, const float* d_xstar, const float* d_ystar,
                           const float* d_slack, float dominance, float floor, float* d_x1, float* d_x2, float* d_labels,
                           void* stream);
int mllp_lp_certificate_scratch_bytes(const mllp_graph_t* g, int64_t* bytes);
int mllp_lp_certificate(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x, const float* d_y,
                        const float* d_basis, float* d_cert, void* d_scratch, void* stream);

/* Repair and solve a predicted basis (mllp_amd/csrc/basis.hip): per instance, a ranking of its columns ->
 * the best-ranked NONSINGULAR basis and its basic solution, whose outputs mllp_lp_certificate takes unchanged.  Added
 * after ABI 6 without a bump, as mllp_lp_certificate was.
 * THE RULE.  Instance k has m rows, n columns and the matrix A_k as the batch stores it now.  Its candidate list is its
 * segment of d_order: instance-local column ids, best first, ended by the first negative entry or by n entries.  Walk the
 * list in order, keeping a set of accepted columns, each with a pivot row of its own.  For a candidate j, with a = column
 * j of A_k:  amax = max_i |a_i|;  w = what is left of a in the rows not yet pivoted after eliminating the accepted columns
 * (the Schur-complement column);  r = max |w_i| over those rows.  Accept j iff amax > 0 and r > tol * amax; its pivot row
 * is the row attaining r, the lowest row index among equal values.  Stop after m acceptances or at the end of the list.
 * Greedy selection over a linear matroid: every accepted column is the best-ranked column independent of the
 * better-ranked accepted ones, so no nonsingular set is lexicographically better in the given ranking.  A repeated id
 * is rejected by the rule itself (its residual is zero up to rounding).  An id >= n ends the instance with code 3;
 * nothing out of bounds is read.  With rank == m:  x_j = (B^-1 b)_j on the accepted columns and 0 elsewhere,
 * y = B^-T c_B; otherwise the instance's x and y are zeros.  All in fp32; tol is a parameter of the rule (the customary
 * value is 2^-12, about sqrt(eps)).
 *   d_x1 [N] = c, d_x2 [M] = b : inputs, read only when d_x / d_y are asked for.   d_order [N] int32 : input.
 *   max_m     : instances with m > max_m are skipped (code 2, outputs defaulted); they cost no scratch.  Values above 8192
 *             mean 8192: the kernel keeps four vectors of m words in LDS (and at that size the transform is 256 MB).
 *   d_basis [N] float 0/1, d_col_of_row [M] int32 (the local id of the column whose pivot row this is, or -1),
 *   d_x [N], d_y [M], d_quality [n_inst, 2] : outputs, each may be NULL (not computed); d_x and d_y come together.
 *   d_status [n_inst, 4] int32, required : {rank, candidates examined, rejected among the first m candidates, code};
 *             code 0: rank == m;  1: the list ended below m;  2: skipped, m > max_m;  3: bad id.
 *   d_quality : {smallest accepted r / amax, largest rejected r / amax}; empty sets give +inf and 0 (the certificate's
 *             convention); a zero column counts as ratio 0.
 *   d_scratch : mllp_basis_repair_scratch_bytes(g, max_m) bytes: m^2 words for every instance with 192 < m <= max_m
 *             (smaller ones keep their transform in LDS); may be NULL when that is 0.
 * Every requested output is fully written for every instance, skipped ones included (zeros, -1, status).  A launch
 * function: `stream` only, no allocation, no synchronisation, hipGraph-capturable; one workgroup per instance.  It reads
 * the graph's plain CSR(A^T) only: paths and attached copies do not matter and are left alone.  No float atomics; every
 * sum has an order that depends on the instance alone, so the result is bitwise reproducible and the same for an
 * instance alone and inside any batch.  The transform is DENSE (m^2 words per instance): this is an evaluation and setup
 * call for m up to a few thousand, not a sparse LU.  Under the MEMORY CONTRACT below.
 * MLLP_EINVAL before any launch, nothing written: null g, d_order or d_status; one of d_x, d_y without the other; null
 * d_x1 or d_x2 with d_x and d_y asked for; null d_scratch with a non-zero scratch size; tol not finite or < 0; max_m < 0. */
int mllp_basis_repair_scratch_bytes(const mllp_graph_t* g, int64_t max_m, int64_t* bytes);
int mllp_basis_repair(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                      const int32_t* d_order /*[N], per instance segment, local ids*/, float tol, int64_t max_m,
                      float* d_basis /*[N] 0/1*/, int32_t* d_col_of_row /*[M] local id or -1*/,
                      float* d_x /*[N]*/, float* d_y /*[M]*/, int32_t* d_status /*[n_inst,4]*/,
                      float* d_quality /*[n_inst,2]*/, void* d_scratch, void* stream);

/* Pivot a basis to optimality (mllp_amd/csrc/simplex.hip): per instance, a basis mask -> dual simplex
 * pivots on shifted costs until the basis is primal feasible, then primal simplex pivots on the true costs until it is
 * optimal.  What it measures is the NUMBER OF PIVOTS between a (repaired) predicted basis and the optimum.  Added after
 * ABI 6 without a bump, as mllp_basis_repair was.
 * THE RULE.  The LP of instance k is the one mllp_lp_certificate judges: min c'x, A_k x = b, x >= 0, c = d_x1, b = d_x2, A_k
 * as the batch stores it now.  All arithmetic is fp32.
 *   Start.  d_start [N] is a mask (nonzero = basic).  Its columns in ascending order are factorized by the rule of
 *     mllp_basis_repair with `tol` (the list mllp_basis_repair gets from LPBatch.solve_basis).  A mask whose column count
 *     differs from m: code 3.  Rank < m: code 1.  Nothing is pivoted in either case.  Otherwise T = B^-1, row i of T
 *     belonging to the basic column col_of_row[i].
 *   Every iteration recomputes from the current T:  x_B = T b;  y = T' g_B;  d_j = g_j - a_j.y for the nonbasic columns,
 *     g the stage's cost vector.  Nothing is carried forward by updates except T itself.
 *   Stage D (dual simplex on shifted costs).  Before the first iteration d0 is computed with g = c and
 *     s_j = max(0, dshift - d0_j) for nonbasic j, 0 for basic j; ctilde = c + s stays fixed, so every nonbasic column starts
 *     at a reduced cost >= dshift (not 0: the entering ratios would all be tied at 0).  Leaving row: p minimises x_B, the
 *     lowest row among equal values.  x_B,p >= -ftol ends stage D; it is never re-entered.  With rho = row p of T and
 *     alpha_j = rho.a_j over the nonbasic j, the candidates are alpha_j < -ptol; none: code 4 (primal infeasible), stop.
 *     Entering: j minimises max(dtilde_j, 0) / (-alpha_j), the lowest j among equal ratios.
 *   Stage P (primal simplex on the true c).  Entering: j minimises d_j, the lowest j among equals (Dantzig).
 *     d_j >= -dtol: code 0 (optimal), stop.  w = T a_j; the candidates are the rows with w_i > ptol; none: code 5
 *     (unbounded), stop.  Leaving row: p minimises max(x_B,i, 0) / w_i, the lowest row among equals.
 *   Pivot, in either stage.  w = T a_j; row p of T is divided by w_p; T[i][:] -= w_i T[p][:] for i != p (the update of
 *     mllp_basis_repair, over all m stored columns); col_of_row[p] = j.
 *   Limits.  A pivot that would be number max_pivots + 1 ends the instance with code 6 (codes 0, 4 and 5 come first: they
 *     need no pivot).  m > max_m: code 2, as in mllp_basis_repair; values of max_m above 4096 mean 4096.
 *   Determinism.  Every argmin is ONE integer min over the keys {bits of the non-negative ratio, or the order-preserving
 *     key of x_B / d; index}.  Every sum has an order that depends on the instance alone (a column's entries in ascending
 *     row order; T b by ascending column; T' g_B by lanes, then the butterfly of the wavefront).  No float atomics.  An
 *     instance gives the same bits alone and inside any batch, with T in LDS or in scratch.
 * WHAT THE RULE DOES NOT CLAIM.  It has no anti-cycling device; pricing is Dantzig and there are no Harris ratios; T is
 * updated in product form and never refactorized.  It is an evaluation tool for up to a few hundred pivots on instances of
 * m up to a few thousand, not a production LP solver: degenerate LPs (most of Netlib) may stop with code 6.
 *   tol                        : mllp_basis_repair's, finite and >= 0.
 *   ftol, dtol, ptol, dshift   : finite and > 0; parameters of the rule in the units of the stored LP, like tol -- not
 *             measured bars.  (The Python defaults: ftol = dtol = ptol = 2^-10, dshift = 2^-4.)
 *   d_x1 [N] = c, d_x2 [M] = b, d_start [N] : inputs, never written; d_start must not overlap an output.
 *   d_basis [N] float 0/1, required : the basis at the stop for codes 0, 4, 5 and 6 (the kernel keeps it current and reads
 *             it back to tell basic from nonbasic columns).
 *   d_col_of_row [M] int32 or NULL : the local id of the basic column that owns row i of T at the stop.
 *   d_trace [n_inst, max_pivots, 2] int32 or NULL : {entering local column, leaving row} of every pivot, -1 past the end.
 *   d_status [n_inst, 4] int32, required : {code, stage-D pivots, stage-P pivots, rank of the start}.
 *             code 0: optimal;  1: the start is singular;  2: skipped, m > max_m;  3: the mask does not have m columns;
 *             4: primal infeasible;  5: unbounded;  6: max_pivots reached.  For codes 1, 2 and 3 the outputs are basis
 *             zeros, col_of_row -1, trace -1 (rank of the start: the rank found for code 1, 0 for codes 2 and 3).
 *   d_scratch : mllp_basis_simplex_scratch_bytes(g, max_m) bytes: for every instance with m <= max_m, n words (the shifts)
 *             and, with m > 192, m^2 words more (smaller ones keep T in LDS); may be NULL when that is 0.
 * x and y are deliberately not outputs: mllp_basis_repair on the final basis (LPBatch.solve_basis) gives them from a FRESH
 * factorization, which is also the refactorization the product-form T never gets.
 * Every requested output is fully written for every instance.  A launch function: `stream` only, no allocation, no
 * synchronisation, hipGraph-capturable; one workgroup per instance; six workgroup barriers per pivot.  It reads the
 * graph's plain CSR(A^T) only.  The kernel's six vectors of m words stay in LDS (6 * 4096 words = 96 KB: the row limit);
 * T is DENSE.  Under the MEMORY CONTRACT below.
 * MLLP_EINVAL before any launch, nothing written: null g, d_x1, d_x2, d_start, d_basis or d_status; tol not finite or < 0;
 * ftol, dtol, ptol or dshift not finite or <= 0; max_pivots < 0; max_m < 0; null d_scratch with a non-zero scratch size. */
int mllp_basis_simplex_scratch_bytes(const mllp_graph_t* g, int64_t max_m, int64_t* bytes);
int mllp_basis_simplex(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                       const float* d_start /*[N] mask*/, float tol, float ftol, float dtol, float ptol, float dshift,
                       int64_t max_pivots, int64_t max_m, float* d_basis /*[N] 0/1, required*/,
                       int32_t* d_col_of_row /*[M] or NULL*/, int32_t* d_trace /*[n_inst, max_pivots, 2] or NULL*/,
                       int32_t* d_status /*[n_inst, 4], required*/, void* d_scratch, void* stream);

/* The same pivots with two guards (mllp_amd/csrc/simplex.hip): Bland's rule once a stage stalls, and a fresh
 * factorization of the basis every refactor_every pivots.  Added after ABI 6 without a bump, as mllp_basis_simplex was.
 * Everything not named here is mllp_basis_simplex's: the arguments and their checks, codes 0-6 and the status words, the
 * scratch (mllp_basis_simplex_scratch_bytes; nothing more, and no LDS vector more), the limits 192 / 4096, one workgroup
 * per instance, the launch-function, memory and determinism contracts.
 * THE RULE is mllp_basis_simplex's with these additions.
 *   Degenerate pivot.  A stage-P pivot is degenerate iff the leaving row's x_B,p <= ftol; a stage-D pivot iff the entering
 *     column's shifted reduced cost dtilde_j <= dtol.  `stall` counts the consecutive degenerate pivots of the current
 *     stage: 0 at the start, 0 again after a pivot that is not degenerate and when stage D ends.
 *   Bland mode.  An iteration runs in Bland mode iff stall_pivots > 0 and stall >= stall_pivots when it begins.  Then
 *     Stage D, leaving row: among the rows with x_B,i < -ftol, the one whose basic column col_of_row[i] is lowest; none
 *       ends the stage (the same condition as outside Bland mode).
 *     Stage D, entering column: the candidates as always (alpha_j < -ptol); j minimises
 *       (dtilde_j > dtol ? dtilde_j : 0) / (-alpha_j), the lowest j among equal ratios.
 *     Stage P, entering column: the lowest j with d_j < -dtol; none: code 0 (the same condition).
 *     Stage P, leaving row: the candidates as always (w_i > ptol); the ratio is (x_B,i > ftol ? x_B,i : 0) / w_i, and among
 *       the rows whose ratio has the bits of the smallest one, the row whose col_of_row[i] is lowest.
 *     The clipping makes every degenerate candidate tie at an exact 0, in any precision; the ties are then broken by the
 *     index of the variable, which is Bland's rule.  Outside Bland mode every choice is mllp_basis_simplex's, bit for bit.
 *   Refactorization (refactor_every = R > 0).  After every pivot whose running number (stage-D + stage-P pivots so far) is
 *     a multiple of R, and before the next iteration, T is discarded and the current basis is factorized as the start was:
 *     its columns in ascending order, the rule of mllp_basis_repair with `tol`.  col_of_row becomes what that factorization
 *     assigns: rows change owners, so a later "lowest row among equals" may differ from the run that was not refactorized;
 *     that is part of the rule.  The shifts stay as they are.  Rank < m: code 7 (the basis could not be refactorized), stop:
 *     d_basis keeps that basis, d_col_of_row is -1, the trace keeps the pivots taken, status words 1-3 as for any stop.
 *   Equivalence.  With refactor_every == 0 and stall_pivots == 0 every output has the bits of mllp_basis_simplex's, and
 *     d_guard is zeros.
 * WHAT IT DOES NOT CLAIM.  No proof of termination in fp32 (Bland's argument needs exact ties, which the clipping gives
 * only up to the tolerances); no Harris ratio test, no steepest-edge pricing; T is still dense and explicit.
 *   refactor_every, stall_pivots : >= 0; 0 switches the guard off.
 *   d_guard [n_inst, 2] int32 or NULL : {refactorizations completed (one that ends in code 7 is not counted), pivots chosen
 *             in Bland mode}; fully written for every instance, zeros for codes 1, 2 and 3.
 * A pivot in Bland mode whose stage is P costs one workgroup barrier more (seven); every other pivot six; a
 * refactorization costs what the start's factorization costs.
 * MLLP_EINVAL before any launch, nothing written: what mllp_basis_simplex refuses; refactor_every < 0; stall_pivots < 0.   */
int mllp_basis_simplex_guarded(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                               const float* d_start /*[N] mask*/, float tol, float ftol, float dtol, float ptol, float dshift,
                               int64_t max_pivots, int64_t max_m, int64_t refactor_every, int64_t stall_pivots,
                               float* d_basis /*[N] 0/1, required*/, int32_t* d_col_of_row /*[M] or NULL*/,
                               int32_t* d_trace /*[n_inst, max_pivots, 2] or NULL*/, int32_t* d_status /*[n_inst, 4], required*/,
                               int32_t* d_guard /*[n_inst, 2] or NULL*/, void* d_scratch, void* stream);

/* Solve every instance by restarted PDHG (mllp_amd/csrc/pdhg.hip): a first-order method -- two sparse
 * matrix-vector products per iteration over the two resident orientations, no factorization, memory O(n + m) per instance,
 * no row limit.  Added after ABI 6 without a bump, as mllp_basis_simplex was.
 * THE RULE.  The LP of instance k is the one mllp_lp_certificate judges: min c'x, A_k x = b, x >= 0, c = d_x1, b = d_x2, A_k
 * as the batch stores it now.  All arithmetic is fp32; every operation is one of fadd, fsub, fmul, fma, fdiv, fsqrt, each
 * rounded to nearest, in the expressions written here; clip(t) = t > 0 ? t : 0 (a NaN gives 0).
 *   Step.  eta = step / sqrt(|A_k|_1 |A_k|_inf): the largest column sum and the largest row sum of |a_ij|, each a fadd
 *     chain in the order below; eta = fdiv(step, fsqrt(fmul(.,.))).  eta = step when that product is not > 0 (A_k has no
 *     nonzero entry).  Computed by the call itself, per instance.
 *   Start.  x = clip(x0), y = y0; a NULL d_x0 (d_y0) means zeros.
 *   Iteration.  s_j = sum_i a_ij y_i (fma chain);  g_j = fsub(c_j, s_j);  x+_j = clip(fsub(x_j, fmul(eta, g_j)));
 *     xbar_j = fsub(fadd(x+_j, x+_j), x_j);  t_i = sum_j a_ij xbar_j (fma chain);  y+_i = fadd(y_i, fmul(eta, fsub(b_i, t_i))).
 *     With check_every > 0 the sums xs += x+, ys += y+ (fadd) of the iterates since the last restart and their count cnt
 *     are kept.
 *   Check, after every check_every iterations.  (xa, ya) = (fdiv(xs_j, (float)cnt), fdiv(ys_i, (float)cnt)).  For a point
 *     z = (x, y):  primal(z) = max_i |fsub(sum_j a_ij x_j, b_i)| / (1 + |b|_inf);  dual(z) = max_j max(fsub(sum_i a_ij y_i,
 *     c_j), 0) / (1 + |c|_inf);  gap(z) = |fsub(c'x, b'y)| / fadd(fadd(1, |c'x|), |b'y|);  err(z) = the largest of the three.
 *     Every max keeps a NaN (it is an integer max over the patterns of non-negative floats).  The candidate is the average
 *     if err(avg) < err(cur), else the current iterate; e is its error.  e not finite: code 8, the output is the current
 *     iterate.  e <= eps: code 0, the output is the candidate.  Otherwise, if e <= fmul(beta, e_last) or
 *     25 cnt >= 9 (iterations so far): restart -- (x, y) <- candidate, e_last = e, sums and cnt cleared.  e_last is +inf at
 *     the start, so the first check restarts.
 *   Limit.  After max_iters iterations without code 0 or 8: code 6, the output is the current iterate (the candidate, when
 *     the check that falls on max_iters restarted) and its three errors are evaluated for d_kkt.  check_every == 0: no
 *     checks, no sums, no restarts -- plain PDHG for max_iters iterations, code 6.
 *   Order.  A row's (column's) terms are added in mllp_graph_normalize's three tiers, picked by the row's length alone
 *     (ordered_sum.h: up to 64 terms by 16 lanes, up to 1024 by a wavefront, longer by the workgroup of 1024 threads; lane
 *     l adds terms l, l + G, ... from 0, then the butterfly, then the binary tree over the wavefronts).  c'x and b'y: thread
 *     t adds j = t, t + 1024, ... (fma), then that butterfly and tree.  The average and the current iterate share every walk.
 * WHAT THE RULE DOES NOT CLAIM.  No diagonal preconditioning or equilibration; no adaptive step or primal weight; no
 * infeasibility detection (an infeasible or unbounded LP ends with code 6, or 8 once an iterate overflows); fp32 residuals
 * bottom out around 1e-6.  It is a BASELINE first-order solve: LPBatch.normalize's row scaling is the only conditioning it
 * gets, and on Netlib it needs tens of thousands of iterations where it converges at all.
 *   d_x1 [N] = c, d_x2 [M] = b : inputs.   d_x0 [N], d_y0 [M] : inputs or NULL; must not overlap an output.
 *   max_iters >= 0, check_every >= 0;  eps finite, >= 0;  step finite, in (0, 1];  beta finite, in (0, 1).
 *   max_lds_words : an instance keeps its five vectors (x, xbar, xs, y, ys: 3 n + 2 m words) in LDS when that is at most
 *             min(max_lds_words, limits[0]), in d_scratch otherwise, with the same bits either way; 0: every instance in
 *             scratch.  mllp_lp_pdhg_limits: {LDS words the kernel can give to vectors (36 864), threads per workgroup
 *             (1024)}; needs no GPU.
 *   d_x [N], d_y [M] : outputs, required.   d_status [n_inst, 4] int32, required : {code, iterations, restarts, 1 if the
 *             average was returned}; code 0: err <= eps;  6: max_iters reached;  8: the error was not finite.
 *   d_kkt [n_inst, 4] or NULL : {primal, dual, gap of the output -- the three terms of err --, eta}.
 *   d_scratch : mllp_lp_pdhg_scratch_bytes(g, max_lds_words) bytes: 3 n + 2 m words for every instance that does not fit
 *             LDS; may be NULL when that is 0.
 * Every requested output is fully written for every instance; n = 0 or m = 0 is legal.  A launch function: `stream` only,
 * no allocation, no synchronisation, hipGraph-capturable; one workgroup per instance, persistent over the iterations; two
 * workgroup barriers per iteration (two more per row of the workgroup tier), and the loop is bounded by max_iters and
 * nothing else.  It reads the graph's plain CSR(A) and CSR(A^T) only.  No float atomics, one writer per word: bitwise
 * reproducible, and the same bits for an instance alone and inside any batch.  Under the MEMORY CONTRACT below.
 * MLLP_EINVAL before any launch, nothing written: null g, d_x1, d_x2, d_x, d_y or d_status (before any HIP call);
 * max_iters < 0; check_every < 0; max_lds_words < 0; eps not finite or < 0; step not finite or outside (0, 1]; beta not
 * finite or outside (0, 1); null d_scratch with a non-zero scratch size; d_x0 or d_y0 overlapping an output.            */
int mllp_lp_pdhg_limits(int64_t limits[2]);
int mllp_lp_pdhg_scratch_bytes(const mllp_graph_t* g, int64_t max_lds_words, int64_t* bytes);
int mllp_lp_pdhg(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                 const float* d_x0 /*[N] or NULL*/, const float* d_y0 /*[M] or NULL*/, int64_t max_iters,
                 int64_t check_every, float eps, float step, float beta, int64_t max_lds_words, float* d_x /*[N]*/,
                 float* d_y /*[M]*/, int32_t* d_status /*[n_inst,4]*/, float* d_kkt /*[n_inst,4] or NULL*/,
                 void* d_scratch, void* stream);

/* Solve every instance by PRECONDITIONED restarted PDHG (mllp_amd/csrc/pdhg.hip): mllp_lp_pdhg's
 * iteration with diagonal scaling (Ruiz passes, an optional Pock-Chambolle pass) and a clamped primal weight, all computed
 * by the call itself.  Added after ABI 6 without a bump.  mllp_lp_pdhg is unchanged.
 * THE RULE.  The LP, the number format and clip are mllp_lp_pdhg's: fp32; fadd, fsub, fmul, fma, fdiv, fsqrt only, each
 * rounded to nearest, in the expressions written here.
 *   Scaling.  dr = 1 [m], dc = 1 [n];  s_ij = fmul(fmul(|a_ij|, dr_i), dc_j) -- this one expression from both orientations.
 *     A Ruiz pass (ruiz_passes of them): R_i = max_j s_ij, C_j = max_i s_ij, both from the same dr and dc, each an integer max
 *     over the bit patterns (exact in any order);  dr_i = fdiv(dr_i, fsqrt(R_i)) where R_i > 0, unchanged otherwise (an empty
 *     row, a NaN);  dc likewise from C.  The Pock-Chambolle pass (pock_chambolle != 0; alpha = 1) is the same update with
 *     R_i = sum_j s_ij, C_j = sum_i s_ij, fadd chains in the order below.  Finally tr_i = fmul(dr_i, dr_i), tc_j =
 *     fmul(dc_j, dc_j).
 *   Step.  eta = fdiv(step, fsqrt(fmul(|S|_1, |S|_inf))): the largest column sum and the largest row sum of the final s_ij,
 *     fadd chains;  eta = step when the product is not > 0.  This square root alone is taken by mllp_lp_pdhg's own
 *     instruction (the hardware's, within 1 ulp of the rounded one), which is what makes the neutral settings hold; every
 *     other fsqrt of this rule is correctly rounded, as every fdiv is.
 *   Weight. w0 = fdiv(|dc o c|_2, |dr o b|_2) when primal_weight != 0 and both norms are finite and > 0, else w0 = 1;
 *     each norm is fsqrt of the fma chain  q = fma(v, v, q), v = fmul(dc_j, c_j)  (fmul(dr_i, b_i)), in the order of c'x.
 *     w = w0;  tau = fdiv(eta, w), sigma = fmul(eta, w), formed again whenever w changes.
 *   Start, (xr, yr).  x = clip(x0), y = y0 as in mllp_lp_pdhg;  (xr, yr) = (x, y).
 *   Iteration.  s_j, g_j, xbar_j, t_i as in mllp_lp_pdhg;  x+_j = clip(fsub(x_j, fmul(fmul(tau, tc_j), g_j)));
 *     y+_i = fadd(y_i, fmul(fmul(sigma, tr_i), fsub(b_i, t_i))).  This is PDHG on the scaled LP written in the unscaled
 *     variables: no scaled matrix is stored.
 *   Check, stop, restart, limit.  mllp_lp_pdhg's, word for word: the errors are those of the ORIGINAL LP, so codes and
 *     d_kkt[0..2] mean the same in both calls.
 *   Weight update.  With primal_weight != 0, at a restart, after the candidate has become the iterate:
 *     dx = fsqrt(sum_j fma(d_j, fdiv(d_j, tc_j), .)), d_j = fsub(x_j, xr_j);  dy likewise with y, yr, tr;  the sums in the
 *     order of c'x.  If dx and dy are both finite and > 0:  w = min(max(fsqrt(fmul(w, fdiv(dy, dx))), fdiv(w0, weight_span)),
 *     fmul(w0, weight_span)).  Then (xr, yr) = (x, y), whether w moved or not.  A stop (code 0) does not update.
 *   Order.  mllp_lp_pdhg's: a row's (column's) terms in the three tiers picked by its length alone; sums over columns or rows
 *     by thread t adding j = t, t + 1024, ..., then the butterfly and the tree.
 *   Neutral settings.  ruiz_passes = 0, pock_chambolle = 0, primal_weight = 0 give tc = tr = 1, tau = sigma = eta and
 *     therefore the bits of mllp_lp_pdhg in d_x, d_y, d_status and d_kkt[0..3] (fmul by 1 and fdiv by 1 are exact).
 * WHAT THIS RULE STILL DOES NOT DO.  No adaptive step size (eta is fixed by the norms of S); no infeasibility detection (an
 * infeasible or unbounded LP ends with code 6 or 8); no feasibility polishing; fp32 residuals bottom out around 1e-6, and
 * the factors themselves can underflow or overflow on a badly scaled matrix (the iterate then turns not finite: code 8).
 *   d_x1, d_x2, d_x0, d_y0, max_iters, check_every, eps, step, beta, max_lds_words, d_x, d_y, d_status : as mllp_lp_pdhg.
 *   ruiz_passes in 0 .. 64;  pock_chambolle, primal_weight : 0 or not 0;  weight_span finite, >= 1 (1 keeps w = w0).
 *   d_dr [M], d_dc [N] or NULL : the factors dr and dc (before squaring).
 *   d_kkt [n_inst, 6] or NULL : {primal, dual, gap of the output, eta, w0, the final w}.
 *   d_scratch : mllp_lp_pdhg_scaled_scratch_bytes(g, max_lds_words) bytes: 2 n + 2 m words for EVERY instance (tc, xr, tr,
 *             yr: read once per finished row, as c and b are, never gathered) and 3 n + 2 m more for every instance whose
 *             five vectors do not fit LDS; may be NULL when that is 0 (a batch without rows and columns).
 *             mllp_lp_pdhg_scaled_limits: {LDS words (36 864), threads per workgroup (1024), largest ruiz_passes (64)}.
 * Every requested output is fully written for every instance; n = 0 or m = 0 is legal.  A launch function: `stream` only,
 * no allocation, no synchronisation, hipGraph-capturable; one workgroup per instance, persistent; the set-up takes
 * 2 (ruiz_passes + pock_chambolle + 1) sweeps, then two workgroup barriers per iteration as mllp_lp_pdhg.  No float atomics,
 * one writer per word: bitwise reproducible, the same bits in LDS and in scratch, alone and inside any batch.
 * mllp_lp_pdhg_scaled is under the MEMORY CONTRACT below as mllp_lp_pdhg is.
 * MLLP_EINVAL before any launch, nothing written: every refusal of mllp_lp_pdhg; ruiz_passes outside 0 .. 64; weight_span
 * not finite or < 1; d_x0 or d_y0 overlapping d_dr or d_dc.                                                               */
int mllp_lp_pdhg_scaled_limits(int64_t limits[3]);
int mllp_lp_pdhg_scaled_scratch_bytes(const mllp_graph_t* g, int64_t max_lds_words, int64_t* bytes);
int mllp_lp_pdhg_scaled(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                        const float* d_x0 /*[N] or NULL*/, const float* d_y0 /*[M] or NULL*/, int64_t max_iters,
                        int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes,
                        int32_t pock_chambolle, int32_t primal_weight, float weight_span, int64_t max_lds_words,
                        float* d_x /*[N]*/, float* d_y /*[M]*/, float* d_dr /*[M] or NULL*/, float* d_dc /*[N] or NULL*/,
                        int32_t* d_status /*[n_inst,4]*/, float* d_kkt /*[n_inst,6] or NULL*/, void* d_scratch,
                        void* stream);

/* Solve every instance by preconditioned, restarted HALPERN PDHG with reflection (mllp_amd/csrc/pdhg.hip):
 * mllp_lp_pdhg_scaled's scaling, step and weight, with the running average replaced by an anchored step,
 * z <- (k+1)/(k+2) (2 T(z) - z) + 1/(k+2) z_anchor, T one PDHG step, the anchor the last restart point (Lu and Yang's rHPDHG).
 * Added after ABI 6 without a bump.  mllp_lp_pdhg and mllp_lp_pdhg_scaled are unchanged.
 * THE RULE.  The LP, the number format and clip are mllp_lp_pdhg's: fp32; fadd, fsub, fmul, fma, fdiv, fsqrt only, each
 * rounded to nearest, in the expressions written here.
 *   Scaling, step, weight, start.  mllp_lp_pdhg_scaled's, word for word: dr, dc, tr, tc, eta, w0, w = w0, tau, sigma;
 *     x = clip(x0), y = y0.  In addition the anchor (xa, ya) = (x, y), the step's output (xh, yh) = (x, y), and k = 0.
 *   Iteration.  w1 = fdiv((float)(k + 1), (float)(k + 2)), w2 = fdiv(1, (float)(k + 2)), k the number of iterations since the
 *     last restart before this one; the conversions round to nearest (without restarts k may pass 2^24).
 *     s_j, g_j as in mllp_lp_pdhg;  xh_j = clip(fsub(x_j, fmul(fmul(tau, tc_j), g_j)));  xbar_j = fsub(fadd(xh_j, xh_j), x_j);
 *     p_j = reflect ? xbar_j : xh_j;  x_j <- fma(w1, p_j, fmul(w2, xa_j)).
 *     t_i = sum_j a_ij xbar_j;  yh_i = fadd(y_i, fmul(fmul(sigma, tr_i), fsub(b_i, t_i)));
 *     q_i = reflect ? fsub(fadd(yh_i, yh_i), y_i) : yh_i;  y_i <- fma(w1, q_i, fmul(w2, ya_i)).  Then k <- k + 1.
 *     Under reflection the iterate's x may be negative; the iterate is never an output.
 *   Check, after every check_every iterations.  ONE point, (xh, yh), with mllp_lp_pdhg's three errors of the ORIGINAL LP and
 *     its NaN-keeping maxima; e is the largest of the three.  e not finite: code 8.  e <= eps: code 0.  Otherwise, if
 *     e <= fmul(beta, e_last) or 25 k >= 9 (iterations so far): restart.  e_last is +inf at the start.
 *   Restart, in this order.  (x, y) <- (xh, yh).  With primal_weight != 0, mllp_lp_pdhg_scaled's weight update with
 *     d_j = fsub(x_j, xa_j) (y likewise, with ya).  (xa, ya) <- (x, y), whether the weight is on or not, moved or not.
 *     k <- 0, e_last = e, restarts + 1.
 *   Output.  Always (xh, yh): at code 0 and code 8 the point that was checked; at code 6 the last iteration's point (the
 *     start when max_iters == 0), with its errors evaluated.  check_every == 0: no checks and no restarts, code 6.
 *   Order.  mllp_lp_pdhg's.
 *   Identity with mllp_lp_pdhg_scaled.  At max_iters = 1, d_x and d_y are that call's at max_iters = 1, check_every = 0, bit
 *     for bit, for either reflect (the first step's output does not depend on w1, w2).  d_dr, d_dc, eta and w0 are that call's
 *     bits at any max_iters.
 * WHAT THIS RULE STILL DOES NOT DO.  No adaptive step size; no infeasibility detection (an infeasible or unbounded LP ends
 * with code 6 or 8); no feasibility polishing; fp32 residuals bottom out around 1e-6.  It changes how fast an instance
 * converges -- usually fewer iterations than mllp_lp_pdhg_scaled, on some instances more -- and it is no superset: on Netlib
 * at 1e-3 it solves four instances that call does not and misses four that it does; most instances that
 * stall there stall here.  An iteration costs 1 to 15 % more than that call's.  reflect = 0 is the unreflected Halpern
 * iteration, which is slower than mllp_lp_pdhg_scaled; it exists to pin the reflection in tests.
 *   d_x1 .. beta, ruiz_passes, pock_chambolle, primal_weight, weight_span, max_lds_words, d_x, d_y, d_dr, d_dc : as
 *             mllp_lp_pdhg_scaled.   reflect : 0 or not 0.
 *   d_status [n_inst, 4] int32, required : {code, iterations, restarts, 0}.
 *   d_kkt [n_inst, 6] or NULL : {primal, dual, gap of the output, eta, w0, the final w}.
 *   d_scratch : mllp_lp_pdhg_halpern_scratch_bytes(g, max_lds_words) bytes, which is mllp_lp_pdhg_scaled_scratch_bytes' closed
 *             form: the LDS image stays 3 n + 2 m words (x, xbar, xh, y, yh) and the anchor is that call's (xr, yr) in the
 *             2 n + 2 m side words.  mllp_lp_pdhg_halpern_limits: mllp_lp_pdhg_scaled_limits' three values.
 * Every requested output is fully written for every instance; n = 0 or m = 0 is legal.  A launch function: `stream` only,
 * no allocation, no synchronisation, hipGraph-capturable; one workgroup per instance, persistent; mllp_lp_pdhg_scaled's
 * set-up, then two workgroup barriers per iteration.  No float atomics, one writer per word: bitwise reproducible, the same
 * bits in LDS and in scratch, alone and inside any batch.
 * mllp_lp_pdhg_halpern is under the MEMORY CONTRACT below as mllp_lp_pdhg is.
 * MLLP_EINVAL before any launch, nothing written: every refusal of mllp_lp_pdhg_scaled, in its order and words, under this
 * call's name.                                                                                                            */
int mllp_lp_pdhg_halpern_limits(int64_t limits[3]);
int mllp_lp_pdhg_halpern_scratch_bytes(const mllp_graph_t* g, int64_t max_lds_words, int64_t* bytes);
int mllp_lp_pdhg_halpern(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                         const float* d_x0 /*[N] or NULL*/, const float* d_y0 /*[M] or NULL*/, int64_t max_iters,
                         int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes,
                         int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect,
                         int64_t max_lds_words, float* d_x /*[N]*/, float* d_y /*[M]*/, float* d_dr /*[M] or NULL*/,
                         float* d_dc /*[N] or NULL*/, int32_t* d_status /*[n_inst,4]*/, float* d_kkt /*[n_inst,6] or NULL*/,
                         void* d_scratch, void* stream);

/* mllp_lp_pdhg_halpern's rule across the whole device (mllp_amd/csrc/pdhg_wide.hip): the same solve as
 * ordinary kernel launches in stream order, every instance's rows and columns spread over as many workgroups as they need,
 * where mllp_lp_pdhg_halpern gives an instance one workgroup on one compute unit for the whole call.  Added after ABI 6
 * without a bump.  mllp_lp_pdhg, mllp_lp_pdhg_scaled and mllp_lp_pdhg_halpern are unchanged.
 * THE RULE is mllp_lp_pdhg_halpern's, word for word: the scaling, step, weight and start; the iteration with `reflect`; the
 * check, the restart, the weight update, the limit and the output; the order of every sum.  A row's sum depends on the row's
 * length alone and every maximum is an integer maximum, so WHICH workgroup sums a row does not reach a bit:
 *   Identity.  With iter_begin = 0 the outputs d_x, d_y, d_dr, d_dc, d_status and d_kkt are mllp_lp_pdhg_halpern's at
 *     max_iters = iter_end, bit for bit, for every instance, every rows_per_item and every batch composition.
 *   Execution.  A work item is rows_per_item consecutive rows of one instance's CSR(A), or columns of CSR(A^T), and one
 *     workgroup of 1024 threads runs it in the three tiers (a row of more than 1024 terms is summed by the workgroup that owns
 *     it).  One launch covers the items of every instance.  An iteration is two launches (the column sweep writes xh, xbar, x;
 *     the row sweep yh, y); a check is its two evaluation sweeps and one launch of one workgroup per instance, which does
 *     everything the rule sums in the order of c'x, and every decision; the set-up is 3 launches per scaling pass and 3 more;
 *     the end of a call is an evaluation and one launch that writes every output.  No kernel waits on another workgroup: no
 *     cooperative launch, no grid barrier, no flag; all ordering between phases is the stream's.  Across workgroups: one
 *     writer per word, and integer atomicMax on the patterns of non-negative floats.  No float atomics.
 *   rows_per_item : a positive multiple of 64 up to limits[3], or 0 for the default, limits[2].  It moves no bit.
 *   mllp_lp_pdhg_wide_limits: {threads per workgroup (1024), largest ruiz_passes (64), default rows_per_item (64), largest
 *             rows_per_item (4096)}; needs no GPU.
 *   iter_begin, iter_end : the call runs iterations iter_begin + 1 .. iter_end.  Checks fall on ABSOLUTE multiples of
 *             check_every.
 *     iter_begin == 0 : set-up and start, then the iterations.  d_scratch may hold anything.
 *     iter_begin > 0 : continues from the state that the previous call left in d_scratch -- a call on the same graph with the
 *             same options and the same d_scratch whose iter_end was this iter_begin; d_x0 and d_y0 are ignored.  Instances at
 *             code 0 or 8 stay as they are, instances at code 6 go on, and every call writes every requested output, d_dr and
 *             d_dc included (the factors are kept in the scratch).  The evaluation at the end of a call leaves the state of a
 *             code-6 instance untouched, so the calls (0, K1) then (K1, K2) give the bits of the call (0, K2), for any K1.
 *             An instance whose state does not say that a call ended exactly at iter_begin gets code 9, STALE STATE: its
 *             outputs are zeros, its status {9, 0, 0, 0}, its state is left as found.  The state is sixteen words of VALUES per
 *             instance (code, iterations, iteration of the last restart, restarts, e_last, w0, w, tau, sigma, eta, the two
 *             denominators): no index, offset or pointer that a kernel follows, so whatever d_scratch holds, no access leaves
 *             the buffers.
 *   d_x1 .. beta, ruiz_passes, pock_chambolle, primal_weight, weight_span, reflect, d_x, d_y, d_dr, d_dc, d_status, d_kkt : as
 *             mllp_lp_pdhg_halpern; d_status[.][0] may also be 9.
 *   d_scratch : mllp_lp_pdhg_wide_scratch_bytes(g, rows_per_item) bytes, which is 4 (21 n_inst + 6 N + 5 M): per instance
 *             the state and five words of the call's own (its flag, two maxima, the first work item of each orientation);
 *             x, xbar, xh, the anchor, tc and dc [N each]; y, yh, the anchor, tr and dr [M each].  May be NULL when that is 0.
 * Every requested output is fully written for every instance; n = 0 or m = 0 is legal.  A launch function: `stream` only, no
 * allocation, no host-to-device copy, no synchronisation, hipGraph-capturable (2 (iter_end - iter_begin) nodes and 3 per
 * check); the map from a workgroup to (instance, block) is made from inst_ptr_m / inst_ptr_n on the device by the call's
 * first kernel.  Bitwise reproducible, the same bits alone and inside any batch.
 * mllp_lp_pdhg_wide is under the MEMORY CONTRACT below as mllp_lp_pdhg is, and the state in d_scratch between a call and the call that continues it is state this header names.
 * MLLP_EINVAL before any launch, nothing written: every refusal of mllp_lp_pdhg_halpern that does not concern max_lds_words,
 * in its words, under this call's name (null arguments before any HIP call); iter_begin < 0; iter_end < iter_begin;
 * rows_per_item negative, above limits[3] or no multiple of 64.                                                            */
int mllp_lp_pdhg_wide_limits(int64_t limits[4]);
int mllp_lp_pdhg_wide_scratch_bytes(const mllp_graph_t* g, int64_t rows_per_item, int64_t* bytes);
int mllp_lp_pdhg_wide(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                      const float* d_x0 /*[N] or NULL*/, const float* d_y0 /*[M] or NULL*/, int64_t iter_begin,
                      int64_t iter_end, int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes,
                      int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect,
                      int64_t rows_per_item, float* d_x /*[N]*/, float* d_y /*[M]*/, float* d_dr /*[M] or NULL*/,
                      float* d_dc /*[N] or NULL*/, int32_t* d_status /*[n_inst,4]*/, float* d_kkt /*[n_inst,6] or NULL*/,
                      void* d_scratch, void* stream);

/* mllp_lp_pdhg_wide with CERTIFICATES OF INFEASIBILITY AND UNBOUNDEDNESS (mllp_amd/csrc/pdhg_wide.hip): codes 4
 * and 5, as mllp_basis_simplex reports them, for the first-order solver.  Added after ABI 6 without a bump.  mllp_lp_pdhg,
 * mllp_lp_pdhg_scaled, mllp_lp_pdhg_halpern and mllp_lp_pdhg_wide are unchanged.
 * The candidate ray costs nothing: the direction from the anchor to the step's output, (xh - xa, yh - ya), converges under
 * Halpern's iteration to the infimal displacement of the PDHG operator, which is zero for a solvable LP and a Farkas ray or a
 * recession ray otherwise.  No new vector, no change to the two sweeps of an iteration.
 * THE RULE is mllp_lp_pdhg_halpern's, word for word, with ONE step inserted into a check, after "e not finite: code 8" and
 * "e <= eps: code 0" and BEFORE the restart test, and only when ray_eps >= 0:
 *   Rays.  rx_j = fsub(xh_j, xa_j), ry_i = fsub(yh_i, ya_i).  At a check the anchor is the last restart point, or the start: it
 *     is always at least check_every iterations old.
 *   Objectives.  by = sum_i fma(b_i, ry_i, .), cx = sum_j fma(c_j, rx_j, .), both in the order of c'x.
 *   Residuals.  U = max_j max(sum_i a_ij ry_i, 0).  V = max(max_i |sum_j a_ij rx_j|, max_j max(-rx_j, 0)).  Each term of a sum is
 *     fma(a_ij, r, q) with the rounded difference as r; the sums run in the row tiers picked by length alone, as in every sweep
 *     of the rule; the maxima are integer maxima over the bit patterns and keep a NaN.
 *   Qualities.  qp = fdiv(U, by) when by is finite and > 0, otherwise +inf.  qd = fdiv(V, -cx) when cx is finite and < 0,
 *     otherwise +inf.  A comparison with a NaN is false.
 *   Decision.  qp <= ray_eps: code 4, primal infeasible, ry is the certificate.  Otherwise qd <= ray_eps: code 5, dual
 *     infeasible (unbounded if feasible), rx is the certificate.  Otherwise the restart test runs as before.  An instance at
 *     code 4 or 5 stops as one at code 0 does; its vectors and its anchor stay as they are.
 *   Off.  With ray_eps < 0 nothing is evaluated and nothing changes: the six outputs of mllp_lp_pdhg_wide have that call's bits.
 * WHAT A CERTIFICATE MEANS.  Code 4: every x >= 0 with A x = b satisfies b'ry = x'A'ry <= U |x|_1, so |x|_1 >= 1 / qp >=
 * 1 / ray_eps: no feasible point is smaller than that.  Code 5: along max(rx, 0) the cost falls by -cx while A x and the sign
 * constraints move by at most qd times that.  These are PDLP's two relative ray tests written for this LP form; they judge rays
 * of the ORIGINAL LP, so they do not depend on dr, dc or the weight.
 * NOT CLAIMED.  The persistent calls (mllp_lp_pdhg, mllp_lp_pdhg_scaled, mllp_lp_pdhg_halpern) get no detection.  Detection is
 * as slow as the displacement's convergence: an instance on which the iteration stalls may never produce a ray and still ends
 * with code 6.  A certificate is relative to ray_eps and is in fp32: a FEASIBLE LP all of whose feasible points have |x|_1 >=
 * 1 / ray_eps ends with code 4, truthfully and uselessly, so ray_eps has to lie below 1 / |x|_1 of the solutions expected
 * (at 2^-10 that stops 46 of the 97 feasible Netlib LPs).  Still no adaptive step size and no feasibility
 * polishing.
 *   d_x1 .. reflect, rows_per_item, d_x, d_y, d_dr, d_dc, d_kkt, iter_begin, iter_end : as mllp_lp_pdhg_wide.  d_x, d_y and d_kkt
 *             are always (xh, yh) and its errors, also at code 4 or 5.
 *   ray_eps : finite; negative: no detection.
 *   d_status [n_inst, 4] : {code, iterations, restarts, 0}; the code may be 0, 4, 5, 6, 8 or 9.
 *   d_ray_y [M] or NULL : ry for an instance at code 4, zeros otherwise.   d_ray_x [N] or NULL : rx at code 5, zeros otherwise.
 *             Both are recomputed from the frozen xh - xa, so they carry the bits of the deciding check.
 *   d_cert [n_inst, 4] or NULL : {qp, by, qd, cx} of the last check at which the instance evaluated its rays (a check that
 *             stops with code 0 or 8 does not), {+inf, 0, +inf, 0} if there was none, zeros for a stale instance.  The four
 *             values are kept in the state, so the calls (0, K1) then (K1, K2) give the bits of the call (0, K2) in every
 *             output, the new ones included.
 *   d_scratch : mllp_lp_pdhg_rays_scratch_bytes(g, rows_per_item) bytes, which is 4 (27 n_inst + 6 N + 5 M): mllp_lp_pdhg_wide's
 *             layout with six more words per instance BEHIND the vectors: two ray keys (the call's own) and the four cert words
 *             (state, values only).  A call with iter_begin > 0 also accepts an instance at code 4 or 5, which stays as it is.
 *             mllp_lp_pdhg_rays_limits: mllp_lp_pdhg_wide_limits' four values.
 * Every requested output is fully written for every instance; n = 0 or m = 0 is legal.  A launch function: `stream` only, no
 * allocation, no host-to-device copy, no synchronisation, hipGraph-capturable, with EXACTLY the launches of mllp_lp_pdhg_wide
 * for the same arguments: the rays ride in the check's two sweeps (a row is walked once for two accumulators, the point's and
 * the ray's: one load of the value and of the index per term, two gathers) and in the decision; they are no sweeps of their
 * own.  Bitwise reproducible, the same bits alone and inside any batch, for every rows_per_item.
 * mllp_lp_pdhg_rays is under the MEMORY CONTRACT below as mllp_lp_pdhg is, and the state in d_scratch between a call and the call that continues it is state this header names.
 * MLLP_EINVAL before any launch, nothing written: every refusal of mllp_lp_pdhg_wide, in its words, under this call's name;
 * ray_eps not finite; d_x0 or d_y0 overlapping d_ray_x, d_ray_y or d_cert.                                                  */
int mllp_lp_pdhg_rays_limits(int64_t limits[4]);
int mllp_lp_pdhg_rays_scratch_bytes(const mllp_graph_t* g, int64_t rows_per_item, int64_t* bytes);
int mllp_lp_pdhg_rays(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                      const float* d_x0 /*[N] or NULL*/, const float* d_y0 /*[M] or NULL*/, int64_t iter_begin,
                      int64_t iter_end, int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes,
                      int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect, float ray_eps,
                      int64_t rows_per_item, float* d_x /*[N]*/, float* d_y /*[M]*/, float* d_dr /*[M] or NULL*/,
                      float* d_dc /*[N] or NULL*/, float* d_ray_x /*[N] or NULL*/, float* d_ray_y /*[M] or NULL*/,
                      int32_t* d_status /*[n_inst,4]*/, float* d_kkt /*[n_inst,6] or NULL*/,
                      float* d_cert /*[n_inst,4] or NULL*/, void* d_scratch, void* stream);

/* mllp_lp_pdhg_rays with a SPECTRAL STEP SIZE (mllp_amd/csrc/pdhg_wide.hip): the step's denominator is an
 * estimate of |S|_2, S = diag(dr) A diag(dc), by power iteration on S'S, where every call before it takes the upper bound
 * sqrt(|S|_1 |S|_inf), which is 1.3 to 6.7 times |S|_2 on this project's data.  Added after ABI 6 without a bump.  mllp_lp_pdhg,
 * mllp_lp_pdhg_scaled, mllp_lp_pdhg_halpern, mllp_lp_pdhg_wide and mllp_lp_pdhg_rays are unchanged.
 * THE RULE is mllp_lp_pdhg_rays', word for word, with ONE step inserted into the set-up (iter_begin = 0), after the scaling and
 * the two norms |S|_1, |S|_inf and before eta is formed.  P = power_iters; fp32, every operation rounded to nearest, as written:
 *   Start.  h_j = 1 + ((j 2654435761 mod 2^32) >> 9) 2^-23, j the column's index INSIDE its instance: an exact fp32 value in
 *     [1, 2) whose bits do not depend on the batch, and no constant vector (A 1 = 0 for some Netlib matrices).
 *     nu_0 = fsqrt(sum_j fma(h_j, h_j, .)), v_j = fdiv(h_j, nu_0).
 *   Round r = 1 .. P.  u_i = fmul(dr_i, sum_j fma(a_ij, fmul(dc_j, v_j), .)), walking CSR(A);
 *     w_j = fmul(dc_j, sum_i fma(a_ij, fmul(dr_i, u_i), .)), walking CSR(A');
 *     nu_r = fsqrt(sum_j fma(w_j, w_j, .)), v_j = fdiv(w_j, nu_r).
 *     The row and column sums run in the tiers picked by the row's length alone, as every sweep of the rule; the sums over j
 *     of h^2 and w^2 run in the order of c'x (thread t adds t, t + 1024, ..., then the butterfly and the tree); every fsqrt is
 *     correctly rounded.  If nu_r (or nu_0) is not finite and > 0 the instance's estimate is VOID and its rounds end.
 *   Estimate.  sigma_est = fsqrt(nu_P), or 0 when void or P = 0.  In exact arithmetic sqrt(|S'S v|) <= |S|_2 for a unit v, and
 *     it is at least |S v|: a lower bound, the tighter of the two.
 *   Step.  L_bound = fsqrt(fmul(|S|_1, |S|_inf)) by mllp_lp_pdhg's own instruction, as before.  L = sigma_est if that is > 0 and
 *     <= L_bound, otherwise L = L_bound.  eta = fdiv(step, L); eta = step when the product is not > 0, as before.  w0, tau,
 *     sigma and everything else that depends on eta are formed as before.
 *   Identity.  With power_iters = 0 every output that mllp_lp_pdhg_rays has is that call's, bit for bit -- mllp_lp_pdhg_wide's
 *     with ray_eps < 0, and through it mllp_lp_pdhg_halpern's -- and d_norm is {0, L_bound}.
 * NOT CLAIMED.  sigma_est is a LOWER bound of |S|_2: a start vector nearly orthogonal to the leading singular space would make
 * the step too long.  The margin is `step` (0.9 against a smallest observed sigma_est / |S|_2 of 0.97 at P = 40); raise
 * power_iters or lower step where that is not enough.  Nothing is added for the persistent calls, and nothing is claimed about
 * the instances on which every rule so far stalls.
 *   d_x1 .. ray_eps, rows_per_item, d_x .. d_cert, iter_begin, iter_end : as mllp_lp_pdhg_rays.  d_kkt[.][3] is the eta in use.
 *   power_iters : 0 .. limits[4] (1024).  Ignored when iter_begin > 0: the set-up does not run and eta is the state's.
 *   d_norm [n_inst, 2] or NULL : {sigma_est, L_bound}; zeros for a stale instance.  Both are kept in the state, so every call
 *             writes them and the calls (0, K1) then (K1, K2) give the bits of the call (0, K2) in every output.
 *   d_scratch : mllp_lp_pdhg_spectral_scratch_bytes(g, rows_per_item) bytes, which is 4 (29 n_inst + 6 N + 5 M):
 *             mllp_lp_pdhg_rays' layout with two more words per instance BEHIND it (sigma_est and L_bound: state, values only;
 *             during the set-up the first holds nu_r).  v, u and w live in xbar and the two anchors, which the set-up does not
 *             read between the scaling and the start: no vector is added.
 *             mllp_lp_pdhg_spectral_limits: mllp_lp_pdhg_wide_limits' four values and the largest power_iters (1024).
 * Every requested output is fully written for every instance; n = 0 or m = 0 is legal (the estimate is void).  A launch
 * function: `stream` only, no allocation, no host-to-device copy, no synchronisation, hipGraph-capturable.  With power_iters = 0
 * it makes EXACTLY the launches of mllp_lp_pdhg_rays; with P > 0 and iter_begin = 0 the set-up makes 3 P + 1 more: one of one
 * workgroup per instance for the start vector, and per round the row sweep, the column sweep (the items of the iteration's
 * sweeps) and one of one workgroup per instance that normalises and records nu_r.  All are ordinary launches of 1024 threads
 * in stream order: no cooperative launch, no grid barrier, no float atomics, one writer per word.  Bitwise reproducible, the
 * same bits alone and inside any batch, for every rows_per_item.
 * mllp_lp_pdhg_spectral is under the MEMORY CONTRACT below as mllp_lp_pdhg is, and the state in d_scratch between a call and the call that continues it is state this header names.
 * MLLP_EINVAL before any launch, nothing written: every refusal of mllp_lp_pdhg_rays, in its words, under this call's name;
 * power_iters outside 0 .. 1024; d_x0 or d_y0 overlapping d_norm.                                                          */
int mllp_lp_pdhg_spectral_limits(int64_t limits[5]);
int mllp_lp_pdhg_spectral_scratch_bytes(const mllp_graph_t* g, int64_t rows_per_item, int64_t* bytes);
int mllp_lp_pdhg_spectral(const mllp_graph_t* g, const float* d_x1 /*c [N]*/, const float* d_x2 /*b [M]*/,
                          const float* d_x0 /*[N] or NULL*/, const float* d_y0 /*[M] or NULL*/, int64_t iter_begin,
                          int64_t iter_end, int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes,
                          int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect, float ray_eps,
                          int64_t power_iters, int64_t rows_per_item, float* d_x /*[N]*/, float* d_y /*[M]*/,
                          float* d_dr /*[M] or NULL*/, float* d_dc /*[N] or NULL*/, float* d_ray_x /*[N] or NULL*/,
                          float* d_ray_y /*[M] or NULL*/, int32_t* d_status /*[n_inst,4]*/,
                          float* d_kkt /*[n_inst,6] or NULL*/, float* d_cert /*[n_inst,4] or NULL*/,
                          float* d_norm /*[n_inst,2] or NULL*/, void* d_scratch, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Plain CSR SpMM (the roofline kernel named in BASELINE.json's metric):
 *   transpose == 0:  Y[M,16] = A   * H[N,16]       transpose == 1:  Y[N,16] = A^T * H[M,16]
 * This is the unweighted skeleton of the message passing in linear_program_methods.py:241-247
 * (gather source rows by edge, scale by a_ij, add into the destination row).
 * ---------------------------------------------------------------------------------------------- */
int mllp_spmm_csr_f32(const mllp_graph_t* g, int transpose, const float* d_H, float* d_Y, void* stream);
/* Opt-in bf16 feature image (SURVEY.md 8b `mllp_spmm_csr_f32/_bf16`, BASELINE.json configs[2] "bf16"): the same
 * product with H given as bf16 [n_src,16] (32-byte rows: half the H traffic and half the LDS image), fp32
 * values, fp32 accumulation, fp32 Y.  NOT the parity path: the result is the fp32 product of A with H rounded
 * to bf16 (relative error of an element of H up to 2^-8; the accumulation itself is exact-fp32 as above).
 * Runs on the LDS-tiled copy only (mllp_graph_attach_tiled, variant 0); MLLP_EINVAL without it.            */
int mllp_spmm_csr_bf16(const mllp_graph_t* g, int transpose, const void* d_H_bf16, float* d_Y, void* stream);

/* Streamed copy of one orientation for mllp_spmm_csr_f32 on large batches (rows of ~100+ nonzeros; layout and
 * rationale: mllp_amd/csrc/stream_layout.h).  The nonzeros are re-blocked ONCE into row tiles of at most 960 rows (never
 * across two LP instances) x 750-column blocks and stored in the order the kernel's wavefronts consume them, so that they stream HBM -> registers while LDS
 * holds two images of H (double-buffered by LDS-DMA).  Replaces the edge list the reference rebuilds every step
 * (linear_program_methods.py:89-103).  The copy is LIBRARY-owned device memory (these three are not launch functions:
 * they allocate, free and synchronise), ~8.6 bytes per nonzero; mllp_spmm_csr_f32 uses it when present.
 *   where: 0 = built on the device (counting + placement kernels), 1 = built by the host reference builder
 *          (same bytes; tests compare the two).
 *   mllp_graph_spmm_copy_info: info[0..7] = row tiles, (tile, block) pairs, 1 KB entry groups, entry slots (padding
 *          included; compare with nnz), bytes of the copy, microseconds the build took, rows per tile, columns per block
 *          | wavefronts per tile << 16.
 *   mllp_graph_export_spmm_copy (tests): which = 0 tile_blk (int32, tiles + 1), 1 blk_id (int32), 2 row records
 *          (int32 x 4 per (tile-block, wavefront, quad)), 3 entry stream (int32 x 4 per (group, lane)), 4 tile_row
 *          (int32, tiles + 1), 5 headers (int32 x 4 per (tile-block, wavefront)).                                 */
int mllp_graph_build_spmm_copy(mllp_graph_t* g, int transpose, int where, void* stream);
int mllp_graph_drop_spmm_copy(mllp_graph_t* g, int transpose);
int mllp_graph_spmm_copy_info(const mllp_graph_t* g, int transpose, int64_t info[8]);
int mllp_graph_export_spmm_copy(const mllp_graph_t* g, int transpose, int which, void* host_dst, int64_t capacity_bytes);

/* Streamed copies for the ATTENTION sweeps of the throughput regime (round 4; mllp_amd/csrc/stream_attn.hip): the same
 * layout and builders in other geometries, one library-owned copy per (orientation, geometry).  The four functions above
 * are these with geom = 0.
 *   geom 0  plain SpMM: 960-row tiles x 750-column blocks, four rows per quad (mllp_spmm_csr_f32)
 *   geom 1  attention forward sweep of a 16-channel TransformerConv whose DESTINATIONS are the rows of this orientation
 *           (transpose = 0: constraints, 1: variables): 480-row tiles x 720-column blocks, two rows per quad, 64-byte
 *           staged items.  When present, mllp_tconv_fwd and the mllp_gnn_* calls of the generic / tiled path use it in
 *           place of the LDS-tiled variant 1.
 *   geom 2  source-major backward sweep (rows of this orientation = the conv's SOURCE nodes): 312-column blocks of the
 *           160-byte destination records; replaces LDS-tiled variant 2.
 *   geom 3  destination-major backward sweep (rows = the conv's destinations): 432-column blocks; replaces variant 4.
 *   geom 4  the LAYER-1 sweeps (one input channel, destination-major forward and backward; mllp_amd/csrc/lane_stream.hip,
 *           layout lane_layout.h): 512-row tiles, ONE LANE PER ROW, 20 000-column blocks of 4-byte items (a whole instance
 *           of the synthetic batch); replaces LDS-tiled variant 3.  where = 1: host reference builder, same bytes.  Export: which = 0
 *           tile_blk, 1 tile_col (int32 x 2 per tile), 2 rows (int32 x 512 per tile), 3 column offsets (uint32 x 2 per
 *           (group, lane)), 4 tile_row, 5 headers (int32 x 2 per (tile-block, wavefront)), 6 values (float x 4 per
 *           (group, lane)); info[6] = 512 | 1 << 16 | 4 << 24.
 *   mllp_graph_stream_copy_info: info[0..5] as mllp_graph_spmm_copy_info; info[6] = row slots per tile | rows per quad
 *          << 16 | bytes per staged item << 24; info[7] = columns per block | wavefronts << 16 | padding groups << 24. */
int mllp_graph_build_stream_copy(mllp_graph_t* g, int transpose, int geom, int where, void* stream);
int mllp_graph_drop_stream_copy(mllp_graph_t* g, int transpose, int geom);
int mllp_graph_stream_copy_info(const mllp_graph_t* g, int transpose, int geom, int64_t info[8]);
int mllp_graph_export_stream_copy(const mllp_graph_t* g, int transpose, int geom, int which, void* host_dst,
                                  int64_t capacity_bytes);

/* Optional LDS-tiled copy of one orientation for large batches (rows of ~100+ nonzeros): the nonzeros
 * re-blocked into row tiles x column blocks so that source rows are read from LDS instead of L2.
 *   mllp_tiled_geometry: rows per tile, source nodes per column block, and the number of entries of one
 *     (tile, block) segment that fit the kernel's LDS window (longer segments take several windows).
 *   d_tile_blk [n_tiles+1]  first (tile, block) index of each row tile (a tile lists the contiguous
 *                           range of column blocks it touches)
 *   d_blk_id   [n_tb]       global column-block id of each (tile, block)
 *   d_ptr2     [n_tb * rows_per_tile + 1]  entry offsets: inside a (tile, block) the rows are ordered by their
 *                           number of entries in that block, descending (position k = k-th longest)
 *   d_perm     [n_tb * rows_per_tile]      row (inside its tile) of every sorted position
 *   d_ent      [nnz][2]     {byte offset of the column's staged item inside its block (64 * local column for
 *                           variants 0, 1, 4), fp32 value bits}, ordered by (tile, block, position); inside a row
 *                           round-robin over (local column mod 4) (LDS bank spreading)
 * The arrays are BORROWED: the caller keeps them alive while attached (n_tiles = 0 detaches).
 * variant 0 is the geometry of the plain SpMM (mllp_spmm_csr_f32 uses it when attached); variant 1 the attention
 * forward sweep with 16 channels (per-row query and softmax state in LDS, hence smaller column blocks); variant 2
 * the source-major attention backward sweep (attach it to the orientation whose ROWS are the conv's source nodes;
 * the staged items are the 160-byte backward records, d_ent[.][0] = 160 * local column); variant 3 the layer-1
 * (one channel) forward and destination-major backward sweeps (staged items are scalars, d_ent[.][0] = 4 * local
 * column); variant 4 the destination-major attention backward sweep with one lane per row: d_perm is the
 * identity (rows keep their order inside a tile, d_ptr2 their offsets) and the entries of every 64-row chunk of a
 * (tile, block) are ordered by step -- entry j of the rows that have one, in row order -- instead of row by row
 * (mllp_amd/graph.py::build_tiled_arrays builds every variant).  mllp_tconv_* / mllp_gnn_* use whichever
 * copies are attached and fall back to the generic sweeps (HIP as well) otherwise.                    */
int mllp_tiled_geometry(int variant, int32_t* rows_per_tile, int32_t* cols_per_block, int32_t* bundle_capacity);
int mllp_graph_attach_tiled(mllp_graph_t* g, int transpose, int variant, int64_t n_tiles, int64_t n_tb,
                            int32_t max_blocks_per_tile /* largest tile_blk[t+1]-tile_blk[t]; at most 255 */,
                            const int32_t* d_tile_blk, const int32_t* d_blk_id, const int32_t* d_ptr2,
                            const int32_t* d_perm, const int32_t* d_ent);
/* The same copies built by the library on the device from the graph's own CSR (counting passes + one placement pass,
 * mllp_amd/csrc/tiled_build.hip; not a launch function: allocates and synchronises `stream`).  The arrays are
 * library-owned: a later build / attach / detach of the same (orientation, variant) and mllp_graph_destroy free them.
 *   mllp_graph_tiled_info: info[0..4] = row tiles, (tile, block) pairs, most blocks in one tile, 1 if library-owned,
 *   longest (tile, block) segment in entries (0 for caller-built copies).
 *   mllp_graph_export_tiled (tests; a setup call beside mllp_graph_build_tiled, not a launch function): device-to-device copy of array `which` = 0 tile_blk, 1 blk_id, 2 ptr2, 3 perm,
 *   4 ent ((nnz + 1) x 2 int32); `count` int32 elements must equal the array's length.                       */
int mllp_graph_build_tiled(mllp_graph_t* g, int transpose, int variant, void* stream);
int mllp_graph_tiled_info(const mllp_graph_t* g, int transpose, int variant, int64_t info[5]);
int mllp_graph_export_tiled(const mllp_graph_t* g, int transpose, int variant, int which, int32_t* d_dst, int64_t count,
                            void* stream);

/* ------------------------------------------------------------------------------------------------
 * One torch_geometric.nn.TransformerConv((cin, cin), 16, edge_dim=1) followed by ReLU, as called at
 * linear_program_methods.py:241-247 (construction :206-211).  dst_is_var = 1 for the *_w2s convs
 * (source = constraints, destination = variables), 0 for *_s2w.
 *   d_conv_params : the conv's 9 tensors, flat, in state_dict order (lin_key.weight, lin_key.bias,
 *                   lin_query.weight, lin_query.bias, lin_value.weight, lin_value.bias,
 *                   lin_edge.weight, lin_skip.weight, lin_skip.bias): 144 floats (cin=1) or 1104.
 *   d_x_src [N_src, cin], d_x_dst [N_dst, cin], d_h_out [N_dst, 16] = relu(conv(...))
 *   d_ws : mllp_tconv_workspace_floats() floats; holds what backward needs (kept by the caller
 *          between forward and backward).
 * Backward: d_dh [N_dst,16] = dL/dh_out (overwritten with the ReLU-masked gradient);
 *   d_dx_dst [N_dst,cin], d_dx_src [N_src,cin] may be NULL (then not computed; with cin = 1 they are never
 *   computed here and never written: the whole model's input gradients are mllp_gnn_backward_inputs); accumulate bit 0 / bit 1 = add into d_dx_dst / d_dx_src
 *   instead of overwriting; d_param_grads: same layout as d_conv_params (overwritten).  An accumulate bit whose pointer is
 *   NULL is ignored.  No other output depends on accumulate or on which of the two pointers are given
 *   (tests/test_conv_options.py).
 * ---------------------------------------------------------------------------------------------- */
int mllp_tconv_workspace_floats(const mllp_graph_t* g, int dst_is_var, int cin, int64_t* n_floats);
int mllp_tconv_fwd(const mllp_graph_t* g, int dst_is_var, int cin, const float* d_conv_params,
                   const float* d_x_src, const float* d_x_dst, float* d_h_out, float* d_ws, void* stream);
int mllp_tconv_bwd(const mllp_graph_t* g, int dst_is_var, int cin, const float* d_conv_params,
                   const float* d_x_src, const float* d_x_dst, const float* d_h_out, float* d_ws,
                   float* d_dh, float* d_dx_dst, float* d_dx_src, int accumulate,
                   float* d_param_grads, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Whole model: GNNModel.forward (linear_program_methods.py:238-251) and its backward
 * (autograd in the reference: linear_program_experiment.py:141).
 *   d_params : MLLP_NUM_PARAMS floats, GNNModel.state_dict() order
 *   d_x1 [N] = objective coefficients (x1, methods.py:90), d_x2 [M] = right-hand sides (x2, :91)
 *   d_ws     : mllp_gnn_workspace_bytes() bytes, kept between forward and backward
 *   d_logits [N] : per-variable logits (methods.py:250-251)
 * MEMORY CONTRACT of every mllp_gnn_*, mllp_tconv_*, mllp_spmm_*, mllp_weighted_loss, mllp_balanced_pos_weight, mllp_topm_*,
 * mllp_graph_normalize, mllp_graph_plant_basis, mllp_lp_certificate, mllp_basis_repair, mllp_basis_simplex, mllp_lp_pdhg and mllp_optim_step call, for every buffer the caller owns (tests/test_memory_contract.py):
 *   1. A call's outputs do not depend on any byte that d_ws, or any other scratch or output buffer, held before the call:
 *      the buffers may be uninitialised, NaN included, and the same bits come out.  The only state carried between calls is
 *      what this header names: mllp_gnn_forward -> mllp_gnn_backward / _backward_inputs / _input_grads on the same workspace
 *      (mllp_gnn_loss_step_weighted leaves its forward's state likewise), mllp_gnn_train_step flags bit 0, and
 *      mllp_tconv_fwd -> mllp_tconv_bwd on the same d_ws.  The library keeps a record of each of the first two per graph
 *      (RECORDS below) and a call that would read carried state the record does not vouch for is refused, or (flags bit 0)
 *      makes the state again: a call either returns the bits it returns from a fresh workspace, or MLLP_EINVAL.
 *   2. A call writes nothing outside the documented extent of the buffers it is given -- for d_ws exactly
 *      mllp_gnn_workspace_bytes() (mllp_tconv_workspace_floats() floats) from the pointer -- and never writes an input:
 *      d_params (except in the train steps), d_x1, d_x2, d_labels, d_dlogits where it is an input, d_inst_weight,
 *      d_pos_weight, d_conv_params, d_x_src, d_x_dst, d_h_out in the backward, d_H.
 *   3. A call's outputs do not depend on any byte outside those extents (a kernel may read past the end of an array
 *      inside the caller's allocation only where what it reads cannot reach a result).
 *   4. Between whole calls that carry nothing the caller may do anything to the workspace: after mllp_gnn_loss_step and
 *      _loss_step_inputs (unless a backward call follows that the workspace record still allows: RECORDS),
 *      _loss_step_weighted (unless a backward call follows), _train_step_small, and after mllp_gnn_train_step when the next
 *      call passes flags 0.  The library cannot see such a write: a caller that clobbers a workspace whose forward it still
 *      means to use gets that garbage's gradients.
 *   RECORDS the library keeps per graph (tests/call_model.py states them as a model; tests/test_call_sequences.py walks
 *      every triple of whole-model calls against it).  They hold pointer VALUES and see only calls made on
 *      this graph: writing d_params or d_ws by other means between a forward and its backward is the caller's to avoid.
 *      Workspace record = {d_ws, path, d_params} of the mllp_gnn_forward whose activations d_ws holds.
 *        set by      mllp_gnn_forward (and so by mllp_gnn_loss_step_weighted, which calls it);
 *        required by mllp_gnn_backward, _backward_inputs and _input_grads: all three must be those of the call, else
 *                    MLLP_EINVAL with a message before any HIP call, nothing written.  The calls leave it as it is, so
 *                    several backward calls may follow one forward, each with the bits of the first;
 *        kept by     mllp_graph_set_path (a switch there and back changes nothing; a backward on the other path is refused)
 *                    and by mllp_gnn_loss_step / _loss_step_inputs given the record's workspace, path and parameters: the
 *                    step's forward writes the bits that are there (on the fused path it leaves layer 3's to that forward);
 *        cleared by  mllp_gnn_loss_step / _loss_step_inputs in every other case (another workspace, path or parameter
 *                    pointer: the step has rewritten the workspace with a forward that is not the recorded one),
 *                    mllp_gnn_train_step on both paths (it rewrites the workspace, then the parameters),
 *                    mllp_gnn_train_step_small, mllp_graph_set_values and the calls that end in it (_scale_values,
 *                    _normalize unless compute only, _plant_basis).
 *      Folded-weights record = {d_ws, d_params} of the fused mllp_gnn_train_step that left the NEXT step's folded weights.
 *        set by      mllp_gnn_train_step on the fused path;   honoured by the next one with flags bit 0, when both match;
 *        cleared by  every other whole-model call on the graph, the generic mllp_gnn_train_step and mllp_graph_set_path;
 *        kept by     mllp_graph_set_values and the calls built on it (the folded weights depend on the parameters alone).
 *   ALIGNMENT: d_ws, d_params, d_x1 and d_x2 of the mllp_gnn_* calls must be 16-byte aligned -- the workspace's fields,
 *      fc.weight and (on the lane-per-row copy of the layer-1 sweeps) four neighbouring source values are accessed in 16-byte
 *      pieces --, as must every pointer of mllp_tconv_fwd / _bwd except d_param_grads (rows of 16 floats; d_ws, d_conv_params)
 *      and d_H, d_Y of mllp_spmm_csr_f32.  A misaligned one is refused with MLLP_EINVAL and a message before any HIP call,
 *      nothing written.  d_logits, d_labels, d_loss, d_grads, d_dlogits, d_dx1, d_dx2, d_dvalues, d_scratch, the optimizer
 *      buffers, the per-instance arrays and the buffers of the loss-head, top-m, normalize, basis-repair, basis-simplex and PDHG calls need only the natural
 *      alignment of their element type.
 * mllp_gnn_backward: d_dlogits [N] -> d_grads [MLLP_NUM_PARAMS] (overwritten; the never-called
 *   gconv3_s2w block, methods.py:248, is written as zeros).
 * mllp_gnn_loss_step: forward + BCEWithLogitsLoss + backward in one call, loss =
 *   inv_batch * sum_k mean_i BCE(logit_i, label_i) over the instances k of this graph
 *   (linear_program_experiment.py:41,139-141 with batch size 1 and inv_batch = 1).
 *   d_labels [N] float 0/1; d_loss: 1 float.  The step rewrites d_ws with its own forward: the workspace record
 *   (RECORDS above) survives it only when it names this d_ws, the path in use and this d_params -- then a backward call
 *   may still follow the earlier mllp_gnn_forward, with the bits it has straight after it -- and is cleared otherwise.
 * mllp_gnn_backward: after mllp_gnn_forward on this d_ws, on the path in use, with this d_params pointer, and nothing since
 *   that clears the record (RECORDS); MLLP_EINVAL with a message otherwise, before any HIP call, nothing written.
 * ---------------------------------------------------------------------------------------------- */
int mllp_gnn_workspace_bytes(const mllp_graph_t* g, int64_t* bytes);
int mllp_gnn_forward(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                     void* d_ws, float* d_logits, void* stream);
int mllp_gnn_backward(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                      void* d_ws, const float* d_dlogits, float* d_grads, void* stream);
int mllp_gnn_loss_step(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                       const float* d_labels, float inv_batch, void* d_ws, float* d_logits,
                       float* d_loss, float* d_grads, void* stream);

/* Input gradients (reference: PyG's TransformerConv is plain autograd, so model(g) is differentiable in g.x1, g.x2 and
 * g.edge_attr as well as in the weights).  Call after mllp_gnn_forward on the GENERIC path (path 1, or path 0 at 32 M
 * nonzeros and above) on this workspace, with the graph still on a generic path; MLLP_EINVAL with a message when the
 * forward on d_ws ran on the fused path.  Runs mllp_gnn_backward, then a post-pass (mllp_amd/csrc/input_grads.hip) that
 * reads only what that backward leaves in the workspace and walks the plain CSR of A / A^T.
 *   d_grads [MLLP_NUM_PARAMS] : as mllp_gnn_backward, bit for bit; may be NULL, then the gradients go to d_scratch
 *   d_dx1 [N], d_dx2 [M], d_dvalues [nnz] : dL/dx1, dL/dx2, dL/da_ij in the CSR order of A (mllp_graph_export 2);
 *     each may be NULL (not computed, costs nothing).  Overwritten, not accumulated.  Bitwise reproducible: fixed
 *     launch order on `stream`, no float atomics.
 *   d_scratch : mllp_gnn_input_grads_scratch_bytes() bytes, used only when d_grads is NULL (may then be NULL).
 * A null graph, params, x1, x2, workspace or dlogits is rejected with a message before any HIP call.  All work is
 * queued on `stream`.  The first call on a graph with d_dvalues != NULL also builds the graph-owned map from A^T
 * positions to A positions (one hipMalloc of 4 * nnz bytes, freed by mllp_graph_destroy): make that first call
 * outside a hipGraph capture; later calls allocate nothing and can be captured.                                   */
int mllp_gnn_input_grads_scratch_bytes(const mllp_graph_t* g, int64_t* bytes);
int mllp_gnn_backward_inputs(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                             void* d_ws, const float* d_dlogits, float* d_grads, float* d_dx1, float* d_dx2,
                             float* d_dvalues, void* d_scratch, void* stream);

/* Input gradients on EITHER path (symbols added without an ABI bump: callers check for them, as for mllp_graph_set_values).
 * mllp_gnn_input_grads: call after mllp_gnn_forward on this workspace, on whichever path that forward used, with the
 *   graph still selecting that path and the d_params pointer of that forward; MLLP_EINVAL with a message, before anything
 *   is written, when the workspace record (RECORDS above) does not name d_ws, the path in use and d_params: no forward ran on
 *   d_ws, it ran on the other path or with another d_params, or a call that clears the record has run since
 *   (mllp_graph_set_values, a train step, a loss step with another path or other parameters).  Generic path: the call IS
 *   mllp_gnn_backward_inputs (same code, same bits).  Fused latency-regime path (the default below 32 M nonzeros): the
 *   fused backward, then a post-pass of four launches for the renumbered workspace (mllp_amd/csrc/fused_input_grads.hip).
 *   Arguments as mllp_gnn_backward_inputs; d_grads is bit for bit what mllp_gnn_backward writes on that path, and with
 *   d_grads == NULL the parameter gradients go to d_scratch (both NULL: MLLP_EINVAL).
 * mllp_gnn_loss_step_inputs: mllp_gnn_loss_step followed by the post-pass of the path in use.  d_logits, d_loss and
 *   d_grads are bit for bit those of mllp_gnn_loss_step on the same inputs and path; arguments as there.  It keeps or
 *   clears the workspace record exactly as mllp_gnn_loss_step does.
 * Both: d_dx1 [N], d_dx2 [M], d_dvalues [nnz] are in the caller's (original) node order, d_dvalues in the CSR order of A
 *   (mllp_graph_export 2); overwritten, not accumulated; each may be NULL, then it is not computed and its kernels are not
 *   launched (all three NULL: exactly mllp_gnn_backward / mllp_gnn_loss_step).  Bitwise reproducible: fixed launch
 *   order, a fixed summation order for every sum, no float atomics.  A null graph, params, x1, x2, workspace, dlogits
 *   or labels (loss step: also logits, loss, grads) is rejected with a message before any HIP call.  All work is queued on
 *   `stream`.  Nothing is allocated, except that the first call on a graph with d_dvalues != NULL builds the graph-owned
 *   map from A^T positions to A positions (one hipMalloc of 4 * nnz bytes): make that call outside a hipGraph capture;
 *   every later call can be captured.  The records of which path wrote the workspace and of the folded weights are left
 *   as mllp_gnn_backward / mllp_gnn_loss_step leave them.                                                           */
int mllp_gnn_input_grads(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                         void* d_ws, const float* d_dlogits, float* d_grads, float* d_dx1, float* d_dx2,
                         float* d_dvalues, void* d_scratch, void* stream);
int mllp_gnn_loss_step_inputs(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                              const float* d_labels, float inv_batch, void* d_ws, float* d_logits, float* d_loss,
                              float* d_grads, float* d_dx1, float* d_dx2, float* d_dvalues, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Weighted loss head (symbols added without an ABI bump: callers check for them, as for mllp_graph_set_values).
 * The reference's criterion is one unweighted nn.BCEWithLogitsLoss() per instance (linear_program_experiment.py:41,
 * 139-141); these calls put torch's BCEWithLogitsLoss(pos_weight=...) and a weight per instance between
 * mllp_gnn_forward and mllp_gnn_backward, in a kernel of their own (mllp_amd/csrc/weighted_loss.hip).  Per instance k of
 * the graph with n_k columns, pw_k = d_pos_weight[k] and w_k = d_inst_weight[k] (NULL array = all ones):
 *     sp_i = max(-z_i, 0) + log1p(exp(-|z_i|))
 *     l_i  = (1 - y_i) z_i + (1 + (pw_k - 1) y_i) sp_i              any label y_i in [0, 1]
 *     L_k  = (1 / n_k) sum_i l_i                                     0 for n_k = 0
 *     dz_i = (w_k / n_k) ((1 - y_i) - (1 + (pw_k - 1) y_i) (1 - sigmoid(z_i)))
 *     loss = sum_k w_k L_k
 * L_k is NOT multiplied by w_k: an instance with w_k = 0 gets dz = 0 and still reports its loss, which makes a masked
 * instance a held-out one.  w_k = inv_batch for every k and no pos_weight is the loss of mllp_gnn_loss_step (same value,
 * another summation order).
 * mllp_weighted_loss: d_logits, d_labels [N] in the caller's node order; d_inst_weight, d_pos_weight [n_inst] or NULL.
 *   Outputs, each may be NULL (not computed) but not all three (MLLP_EINVAL): d_dlogits [N] (what mllp_gnn_backward and
 *   mllp_gnn_input_grads take; must not overlap d_logits), d_inst_loss [n_inst] = L_k, d_loss [1].  One launch of one
 *   workgroup per instance, plus one launch of one workgroup for d_loss.  With d_loss but no d_inst_loss ONE workgroup
 *   takes the instances in turn -- same bits, slower: pass d_inst_loss where time matters.
 * mllp_balanced_pos_weight: d_pos_weight [n_inst] = (n_k - P_k) / P_k with P_k = sum_i y_i, the weight that gives the
 *   positives of an instance the total weight of its negatives; 1 where P_k = 0 or P_k = n_k (and for n_k = 0).  Labels
 *   are constant for a batch's life: call it once, not per step.
 * mllp_gnn_loss_step_weighted: mllp_gnn_forward, mllp_weighted_loss, mllp_gnn_backward on whichever path the graph
 *   selects.  d_logits [N] and d_grads [MLLP_NUM_PARAMS] are bit for bit what those calls write; d_dlogits [N] is
 *   required scratch and holds dz afterwards; d_loss, d_inst_loss, d_inst_weight, d_pos_weight may be NULL.  The
 *   workspace record is left as mllp_gnn_forward / mllp_gnn_backward leave it, so mllp_gnn_input_grads may follow.
 * All three: every sum has a fixed order that depends on n_k alone (loss: on n_inst alone, instance order), no float
 * atomics, so an instance gives the same L_k and dz bits alone and inside any batch, whichever outputs are asked for,
 * run after run.  A null graph, logits or labels (step: params, x1, x2, labels, workspace, logits, grads, dlogits;
 * balanced: labels, pos_weight) is rejected with a message before any HIP call.  Nothing is allocated; all work is
 * queued on `stream` (capturable).
 * ---------------------------------------------------------------------------------------------- */
int mllp_weighted_loss(const mllp_graph_t* g, const float* d_logits, const float* d_labels,
                       const float* d_inst_weight, const float* d_pos_weight, float* d_dlogits,
                       float* d_inst_loss, float* d_loss, void* stream);
int mllp_balanced_pos_weight(const mllp_graph_t* g, const float* d_labels, float* d_pos_weight, void* stream);
int mllp_gnn_loss_step_weighted(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                                const float* d_labels, const float* d_inst_weight, const float* d_pos_weight,
                                void* d_ws, float* d_logits, float* d_loss, float* d_inst_loss, float* d_grads,
                                float* d_dlogits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * Soft top-m loss head (symbols added without an ABI bump: callers check for them, as for mllp_weighted_loss).
 * The model predicts a basis: exactly m_k of instance k's n_k columns, m_k = the instance's row count in the graph.  This
 * head trains on probabilities that sum to m_k, where mllp_weighted_loss judges every column against logit 0.  Reference:
 * the (commented-out) gumbel_sinkhorn_topk(latent_vars, len(constrs), max_iter=cfg.sinkhorn_iter, tau=cfg.sinkhorn_tau,
 * sample_num, noise_fact, return_prob=True) of linear_program_experiment.py:126-137, whose module the reference does not
 * ship, and the lml projection it imports.  That call iterates Sinkhorn on a 2 x n transport problem (row masses n - m and
 * m, column masses 1, costs = the distances of a score to the anchors min and max, temperature sinkhorn_tau); its fixed point
 * is closed-form, p_i = sigmoid(2 z_i / sinkhorn_tau + nu) with the scalar nu fixed by sum_i p_i = m, and this head computes
 * that fixed point: tau here = sinkhorn_tau / 2.  (mllp_amd/csrc/topm_loss.hip)
 * Per instance k; pw_k, w_k as in mllp_weighted_loss (NULL = ones); tau > 0, sigma >= 0, S = n_samples.  ONE EVALUATION e
 * of the head with a perturbation eps_i (0 without noise), for 0 < m_k < n_k:
 *     a_i  = (z_i + sigma eps_i) / tau                       fp32: one product, one sum, one quotient (no noise: z_i / tau)
 *     nu_e : the root of F(nu) = sum_i sigmoid(a_i + nu) - m_k   (unique: F is increasing)
 *     u_i  = a_i + nu_e,  p_i = sigmoid(u_i),  q_i = p_i (1 - p_i),  Q = sum_i q_i
 *     l_i  = (1 - y_i) u_i + (1 + (pw_k - 1) y_i) softplus(-u_i)        mllp_weighted_loss's l_i at u instead of z
 *     L_e  = (1 / n_k) sum_i l_i
 *     g_i  = (1 / n_k) ((1 - y_i) - (1 + (pw_k - 1) y_i) (1 - p_i)),  G = sum_i g_i
 *     dz_i = (w_k / tau) (g_i - q_i G / Q)                   the implicit-function gradient of w_k L_e: nothing unrolled,
 *                                                            nothing saved.  (Computed as (w_k / tau / n_k) (n_k g_i -
 *                                                            q_i (n_k G) / Q); the quotient G / Q is taken as 0 when Q = 0.)
 *   n_samples == 0 ('soft-topk'): one evaluation with eps = 0; L_k = L_e, dz = dz_e.
 *   n_samples = S >= 1 ('gs-topk'): S evaluations with Gumbel noise; L_k = (sum_e L_e) / S and dz = (sum_e dz_e) / S, both
 *     added in sample order e = 0, 1, ... from the first term.
 *   m_k <= 0 or m_k >= n_k (no root; n_k = 0 included): L_k = 0, dz = 0, p = 0 (m_k <= 0) or 1, info = {0, 0, sum p - m_k, -1}.
 *   loss = sum_k w_k L_k, added as mllp_weighted_loss adds it (instance order from 0, one rounded product per term).
 * THE NOISE is a pure function of (seed, instance id, local column i, sample e), so an instance gives the same bits alone
 * and inside any batch.  id_k = d_inst_id ? d_inst_id[k] : k.  All arithmetic uint32:
 *     mix(x) = { x ^= x >> 16; x *= 0x7feb352d; x ^= x >> 15; x *= 0x846ca68b; x ^= x >> 16; }
 *     h      = mix( mix( mix(seed ^ (id_k * 0x9E3779B9)) + i ) + e * 0x85EBCA6B )
 *     t      = ((h >> 9) + 0.5) * 2^-23                      exact in fp32, in (0, 1)
 *     eps_i  = -log(-log t)                                   logf twice
 * THE ROOT (part of the bits).  c0 = logf(m / (n - m)); bracket lo = c0 - max_i a_i, hi = c0 - min_i a_i; start
 * nu = c0 - (sum_i a_i) / n clamped to [lo, hi].  Iteration t = 1, 2, ..., at most 64: F and Q at nu; stop if F == 0;
 * F < 0 moves lo to nu, otherwise hi; stop if hi is at most 2 ulp above lo; the Newton iterate nu - F / Q is taken when
 * Q > 0 and it lies strictly inside (lo, hi), the midpoint lo / 2 + hi / 2 otherwise; a Newton iterate that moves nu by
 * at most 2^-12 is taken and ends the iteration (|F''| <= Q, so what that last step leaves is below 2^-25, under the
 * rounding of F itself; a tighter test gains nothing and can chase that rounding for all 64 iterations).  nu, lo, hi and the count come
 * from the ordered sums below, so they are uniform in the instance's workgroup.
 * mllp_topm_loss: d_logits, d_labels [N] in the caller's node order; d_inst_weight, d_pos_weight, d_inst_id [n_inst] or
 *   NULL.  Outputs, each may be NULL (not computed) but not all five (MLLP_EINVAL): d_dlogits [N] (must not overlap
 *   d_logits), d_inst_loss [n_inst] = L_k, d_loss [1], d_prob [N] = p of the NOISE-FREE evaluation (the soft basis; sums to
 *   m_k), d_info [n_inst, 4] = {nu, Q, sum p - m_k of the noise-free evaluation, the largest iteration count over this
 *   call's evaluations of the instance}.  With S >= 1, d_prob or d_info cost one more (noise-free) evaluation; with S = 0
 *   nothing.  Also MLLP_EINVAL, with a message, before any HIP call, nothing written: tau not finite or <= 0, sigma not
 *   finite or < 0, n_samples < 0 (or above 2^20).  One launch of one workgroup of 1024 threads per instance, plus one of
 *   one workgroup for d_loss; with d_loss but no d_inst_loss ONE workgroup takes the instances in turn (same bits, slower).
 * mllp_topm_loss_limits: limits[0] = the column count up to which an instance's a_i stay in LDS between the passes (longer
 *   instances form them again from the logits in every pass: same bits, more time), limits[1] = threads of the workgroup.
 *   Needs no GPU.
 * mllp_topm_loss_math: d_y[i] = expf (which 0), log1pf (1) or logf (2) of d_x[i], i < n, as the head's translation unit
 *   compiles them: the one ingredient of the head's error bound that its code does not state (tests/test_topm_loss.py).
 * mllp_gnn_loss_step_topm: mllp_gnn_forward, mllp_topm_loss (no d_prob, no d_info), mllp_gnn_backward on whichever path
 *   the graph selects.  d_logits [N] and d_grads [MLLP_NUM_PARAMS] are bit for bit what those calls write; d_dlogits [N] is
 *   required scratch and holds dz afterwards; d_loss, d_inst_loss, d_inst_weight, d_pos_weight, d_inst_id may be NULL.  A
 *   bad tau, sigma or n_samples is refused before the forward.  The workspace record is left as mllp_gnn_forward /
 *   mllp_gnn_backward leave it, so mllp_gnn_input_grads may follow.
 * All: every sum (sum p, Q, sum l, G, sum a) is ordered_sum.h's over the 1024 threads as lanes -- thread t adds terms t,
 * t + 1024, ... from 0, then the butterfly, then the fixed tree over the wavefronts -- so it depends on n_k alone; no float
 * atomics, one writer per word.  An instance gives the same bits alone (with its d_inst_id) and inside any batch, whichever
 * outputs are asked for, run after run.  A null graph, logits or labels (step: as mllp_gnn_loss_step_weighted) is rejected
 * with a message before any HIP call.  Nothing is allocated; all work is queued on `stream` (capturable).
 * ---------------------------------------------------------------------------------------------- */
int mllp_topm_loss(const mllp_graph_t* g, const float* d_logits, const float* d_labels,
                   const float* d_inst_weight, const float* d_pos_weight, const int32_t* d_inst_id,
                   float tau, float sigma, int64_t n_samples, uint32_t seed,
                   float* d_dlogits, float* d_inst_loss, float* d_loss, float* d_prob, float* d_info, void* stream);
int mllp_topm_loss_limits(int64_t limits[2]);
int mllp_topm_loss_math(int which, int64_t n, const float* d_x, float* d_y, void* stream);
int mllp_gnn_loss_step_topm(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                            const float* d_labels, const float* d_inst_weight, const float* d_pos_weight,
                            const int32_t* d_inst_id, float tau, float sigma, int64_t n_samples, uint32_t seed,
                            void* d_ws, float* d_logits, float* d_loss, float* d_inst_loss, float* d_grads,
                            float* d_dlogits, void* stream);

/* ------------------------------------------------------------------------------------------------
 * torch.optim.Adam(lr, betas=(0.9, 0.999), eps=1e-8), no weight decay
 * (linear_program_experiment.py:119,143-144) on flat buffers.
 *   d_state: 4 floats on the device {step (as float, incremented by the kernel), lr, beta1, beta2};
 *            eps is passed by value.  grad_scale multiplies the gradient first (data-parallel
 *            averaging).  Parameters whose gradient is exactly 0 with zero moments do not move,
 *            which reproduces torch skipping `grad is None` parameters (gconv3_s2w).
 * ---------------------------------------------------------------------------------------------- */
int mllp_adam_step(float* d_params, const float* d_grads, float* d_exp_avg, float* d_exp_avg_sq,
                   float* d_state, float eps, float grad_scale, int64_t n, void* stream);

/* ------------------------------------------------------------------------------------------------
 * AdamW, global-norm gradient clipping and a learning-rate schedule on the flat buffers, all decided on the device
 * (mllp_amd/csrc/optim.hip): torch.optim.AdamW + torch.nn.utils.clip_grad_norm_ + a warm-up / cosine
 * LambdaLR, without a host round trip, so that a captured step replays with the schedule advancing.  A new entry point
 * beside mllp_adam_step, which is unchanged (symbols added without an ABI bump: callers check for them, as for
 * mllp_graph_set_values).
 *   d_state [8] = {step, lr_base, beta1, beta2, warmup W, total T, min_ratio r, 0}.  The first four words are
 *            mllp_adam_step's: a state of that call is continued by padding {0, 0, 0, 0}.  Only state[0] is ever written.
 *   d_scratch : mllp_optim_scratch_floats(n) floats (0 for n <= 16384: the pointer may then be NULL).
 *   d_info [4] or NULL = {||g||, c, lr_t, skipped}.
 * THE RULE.  All arithmetic is fp32; t = step + 1 is the step being taken.
 *   gradient  g_i = grad_scale * d_grads[i].
 *   norm      computed only when max_norm > 0 or d_info is given: ||g|| = sqrtf(sum_i g_i^2), every operation an explicit
 *             __fmaf_rn / __fadd_rn in a FIXED ORDER THAT DEPENDS ON n ALONE -- the order is the contract:
 *               slices of 4096 elements, slice s = [4096 s, min(n, 4096 (s + 1)));
 *               the partial P_s of a slice by one workgroup of 1024 threads: thread t adds its terms t, t + 1024, t + 2048,
 *               t + 3072 of the slice in that order, from 0 (acc = fmaf(g, g, acc)); the 64 lanes of a wavefront by the xor
 *               butterfly (1, 2, half-mirror, mirror inside 16 lanes, then 16 and 32), the 16 wavefronts by the fixed binary
 *               tree ((0 + 1) + (2 + 3)) + ... (ordered_sum.h);
 *               the total by the same pattern over the partials: thread t adds P_t, P_(t + 1024), ... in that order, from
 *               0, then butterfly and tree.
 *             No float atomics, one writer per word: the same bits on every run.
 *   clip      c = min(1, max_norm / (||g|| + 1e-6)) when max_norm > 0, else 1 (torch.nn.utils.clip_grad_norm_).
 *   skip      where a norm was computed and it is not finite (a NaN or Inf anywhere in the gradient, or an overflow of the
 *             sum), THE STEP IS SKIPPED: d_params, both moments and all of d_state keep their bits, d_info = {||g||, 0,
 *             lr_t, 1}.  This is deliberately NOT torch's behaviour, which scales by NaN and writes NaN into every weight.
 *             With max_norm == 0 and d_info == NULL nothing is inspected, as in mllp_adam_step.
 *   rate      lr_t = lr_base * t / W                                                       for W > 0 and t <= W;
 *             lr_t = lr_base * (r + (1 - r) * 0.5 * (1 + cosf(pi * min(1, (t - W) / (T - W)))))   otherwise, for T > W;
 *             lr_t = lr_base                                                               otherwise.
 *             W = T = 0 is mllp_adam_step's constant rate.  lr_t is never stored into state[1].
 *   decay     decoupled (torch.optim.AdamW): p_i <- p_i - (lr_t * weight_decay) * p_i (one fmaf), then Adam's update of
 *             mllp_adam_step with c * g_i and lr_t.  An element with g_i == 0 and both moments 0 is NOT TOUCHED AT ALL, and
 *             is not decayed either: the flat buffer cannot tell "grad is None" from 0 (gconv3_s2w), and this is what AdamW
 *             does to a parameter without a gradient.
 *   equivalence  with weight_decay = 0, max_norm = 0, W = T = 0 and d_info == NULL, d_params, both moments and state[0]
 *             get the bits mllp_adam_step gives them, at every n.
 * SHAPE.  n <= 16384: one launch of one workgroup (norm, barrier, update, tick).  Larger n: at most three launches -- the
 *   slice partials into d_scratch (not run when no norm is needed), the sliced update in which every workgroup adds the
 *   partials itself in the order above, a one-thread tick of the step counter.  Stream order between the launches is the
 *   only synchronisation.  A launch function: it works on `stream` only, allocates nothing, never synchronises and can be
 *   captured into a hipGraph.  Under the MEMORY CONTRACT above: d_scratch and d_info may hold anything, NaN included.
 * REFUSALS, MLLP_EINVAL with a message before any HIP call, nothing written: null d_params, d_grads, moments or d_state;
 *   n < 0 (or n >= 2^30); eps, grad_scale, weight_decay or max_norm not finite; weight_decay < 0; max_norm < 0; a null
 *   d_scratch when mllp_optim_scratch_floats(n) > 0.  W, T and r live on the device and CANNOT be checked by a launch
 *   function: the caller validates W >= 0, T >= 0, 0 <= r <= 1 where it fills the state (mllp_amd.trainer.FlatAdamW does).
 * mllp_optim_scratch_floats needs no GPU.
 * ---------------------------------------------------------------------------------------------- */
int mllp_optim_scratch_floats(int64_t n, int64_t* out);
int mllp_optim_step(float* d_params, const float* d_grads, float* d_exp_avg, float* d_exp_avg_sq, float* d_state,
                    float eps, float grad_scale, float weight_decay, float max_norm, float* d_scratch, float* d_info,
                    int64_t n, void* stream);

/* One whole training step of a single rank: mllp_gnn_loss_step followed by mllp_adam_step (grad_scale 1) on the
 * MLLP_NUM_PARAMS parameters -- the body of the reference's loop, linear_program_experiment.py:139-144 -- with the same
 * results bit for bit.  On the latency-regime path (batches below 32 M nonzeros) the end of the step runs as ONE launch:
 * reduction of the statistics, the gradients of the five convs, Adam, and the folded weights of the NEXT step, which
 * are left in the workspace.  flags bit 0: "the folded weights in d_ws are current" -- set it when the previous call on
 * this d_ws was mllp_gnn_train_step with these d_params and nothing else has written d_params since; the forward then
 * skips its weight-folding launch.  The library checks the claim against its folded-weights record (RECORDS above) and
 * folds the weights itself when the record does not match, so passing bit 0 always is safe.  The step clears the workspace
 * record on both paths: it rewrites d_ws and then d_params, so no backward call may follow an earlier forward across it.
 * With several ranks the gradient all-reduce sits between the two halves, so a
 * data-parallel caller keeps calling mllp_gnn_loss_step and mllp_adam_step.                                      */
int mllp_gnn_train_step(const mllp_graph_t* g, float* d_params, const float* d_x1, const float* d_x2,
                        const float* d_labels, float inv_batch, void* d_ws, float* d_logits, float* d_loss,
                        float* d_grads, float* d_exp_avg, float* d_exp_avg_sq, float* d_state, float eps, int flags,
                        void* stream);

/* The training step of a SMALL batch as one launch of one workgroup (small_step.hip): weight fold, the five convs forward,
 * fc + BCEWithLogits, the five convs backward, the parameter gradients and, with the three optimizer buffers given, Adam.
 * It is the step of the reference's own loop -- one LP, one Adam step, the next LP (linear_program_experiment.py:123-144)
 * -- for instances whose cost on the other paths is their launches.  The kernel reads the graph's plain arrays only
 * (CSR(A), CSR(A^T), 1 / n_k), so it runs on any graph whatever mllp_graph_set_path selected, and leaves the path alone.
 *   mllp_gnn_small_step_limits  limits = {max nodes M + N, max nonzeros, threads of the workgroup, LDS bytes}; needs no GPU.
 *                               Every graph with M + N <= 2048 and nnz <= 8192 is within the limits.
 *   mllp_gnn_small_step_fits    *fits = 1 when g is within the limits, else 0.
 *   mllp_gnn_train_step_small   arguments as mllp_gnn_train_step (no flags).  d_exp_avg == d_exp_avg_sq == d_state == NULL
 *                               selects the loss step: d_logits, d_loss, d_grads are written, d_params is not touched;
 *                               one or two of the three NULL is MLLP_EINVAL.  A graph beyond the limits is refused with
 *                               MLLP_EINVAL before any launch, nothing written; the message names the limit.  d_ws is the
 *                               buffer of mllp_gnn_workspace_bytes().  One launch on `stream`, no allocation, hipGraph-
 *                               capturable, bitwise reproducible.  The call forgets the forward and the folded weights the
 *                               library remembered for g: a later mllp_gnn_backward asks for a forward first, and a later
 *                               mllp_gnn_train_step folds its weights whatever flags bit 0 says.                       */
int mllp_gnn_small_step_limits(int64_t limits[4]);
int mllp_gnn_small_step_fits(const mllp_graph_t* g, int* fits);
int mllp_gnn_train_step_small(const mllp_graph_t* g, float* d_params, const float* d_x1, const float* d_x2,
                              const float* d_labels, float inv_batch, void* d_ws, float* d_logits, float* d_loss,
                              float* d_grads, float* d_exp_avg, float* d_exp_avg_sq, float* d_state, float eps,
                              void* stream);

/* ------------------------------------------------------------------------------------------------
 * Prediction + metrics (linear_program_experiment.py:146-151): per instance k, mark the m_k largest
 * logits, correct_k = |pred & basis|, f1_k = 2TP / (2TP + FP + FN).
 *   d_out [n_inst, 2] = {correct_k, f1_k}.   d_scratch: mllp_metrics_scratch_bytes() bytes.
 * ---------------------------------------------------------------------------------------------- */
int mllp_metrics_scratch_bytes(const mllp_graph_t* g, int64_t* bytes);
int mllp_topm_metrics(const mllp_graph_t* g, const float* d_logits, const float* d_labels,
                      void* d_scratch, float* d_out, void* stream);

/* ------------------------------------------------------------------------------------------------
 * The predicted basis itself, without labels (the reference forms this vector before it scores it:
 * `pred[pred_indices] = 1`, linear_program_experiment.py:146-148).  One workgroup per segment; order and tie rule
 * are those of mllp_topm_metrics: logits are compared by the key of their bit pattern (negative: all bits
 * flipped, otherwise: sign bit set), a total order in which -0.0 < +0.0 and every NaN has a place; the
 * min(m_k, n_k) largest keys are selected, and among keys EQUAL to the m-th largest the lowest indices win.
 * Each output may be NULL (not computed), but not all three:
 *   d_mask  uint8 [sum n_k]  1 where the variable is in the predicted basis, 0 elsewhere (every byte written)
 *   d_index int32 [sum m_k]  at offset sum_{j<k} m_j: the instance-LOCAL column indices of the selected variables,
 *                            ascending; slots past min(m_k, n_k) hold -1
 *   d_stats float [n_seg, 2] {threshold, runner_up} = the m-th largest logit and the largest logit NOT selected, both
 *                            with the bits they have in d_logits.  runner_up = -inf when every column is selected
 *                            (m_k >= n_k); threshold = +inf when nothing is (m_k = 0 or n_k = 0), and runner_up is then
 *                            the largest logit (-inf for an empty segment).  threshold - runner_up is a margin a caller
 *                            can read as confidence; equal bit patterns mean a tie was broken by index.
 * mllp_topm_select takes the segments and m_k from the graph (instances; m_k = constraints of instance k);
 * mllp_topm_select_dense is one segment of n logits with m to select (AngleModel: n = N - 1, m = basis_num).
 * No float arithmetic and no global atomics: results are bitwise reproducible.  A null graph or logits, all three
 * outputs NULL, or a negative n or m is rejected with a message before any HIP call.  Nothing is allocated; all
 * work is queued on `stream` (capturable).
 * ---------------------------------------------------------------------------------------------- */
int mllp_topm_select(const mllp_graph_t* g, const float* d_logits, uint8_t* d_mask, int32_t* d_index,
                     float* d_stats, void* stream);
int mllp_topm_select_dense(int64_t n, int64_t m, const float* d_logits, uint8_t* d_mask, int32_t* d_index,
                           float* d_stats, void* stream);

/* ------------------------------------------------------------------------------------------------
 * MPS -> the tensors the reference's loader reads (host only, no GPU needed).
 * Replaces the preprocessing that produced /root/reference/dataset/netlib_mps{,_norm}/<name>_{constrs.npz,
 * coefs.npy,rhs.npy} from /root/reference/netlib_mps/<name>.mps (input format: afiro.mps:1-83; consumer:
 * linear_program_data.py:58-80).  The reference ships the tensors but not the script; the rules (recovered from
 * the data, reproducing all 97 instances) are stated in mllp_amd/csrc/mps_reader.cpp and oracle/mps_norm.py.
 *   normalize == 0: the raw stage (A, c, b; one extra column per RANGES entry)
 *   normalize != 0: slack column per L / G row, rows scaled to unit 2-norm with the right-hand side capped at 5,
 *                   objective scaled to unit 2-norm.
 * dims[0..5] = m, n (all columns), nnz, structural columns, range columns, slack columns.
 * mllp_lp_export: any pointer may be null; indptr [m+1] int64, indices [nnz] int32 (ascending in a row),
 *   values [nnz], coefs [n], rhs [m] float64, slack_rows [slack columns] int32 (the row of each slack, in order:
 *   basis = [v ; c[slack_rows]] assembles the label vector from a solver's variable / constraint statuses).   */
typedef struct mllp_lp mllp_lp_t;
int mllp_mps_read(const char* path, int normalize, mllp_lp_t** out);
int mllp_lp_dims(const mllp_lp_t* lp, int64_t dims[6]);
int mllp_lp_export(const mllp_lp_t* lp, int64_t* indptr, int32_t* indices, double* values, double* coefs,
                   double* rhs, int32_t* slack_rows);
int mllp_lp_free(mllp_lp_t* lp);

/* ------------------------------------------------------------------------------------------------
 * `AngleModel` of the `angleNet` method (reference linear_program_methods.py:187-200, loop
 * linear_program_experiment.py:81-114): three TransformerConv layers (2 -> F, F -> F, and the same F -> F layer
 * again) + Linear(F, 1) on the COMPLETE directed graph over the N = n + 1 nodes of one instance, edge attribute =
 * cosine similarity (build_graph_from_Q_sets, :119-130).  Dense attention with a scalar edge bias:
 *   d_cos    [N, N]  cosine matrix, row = target node, column = source node; SYMMETRIC: every sweep reads the whole
 *                    matrix, the forward and the query sweep of the backward d_cos[i][j] for the edge j -> i, the key /
 *                    value sweep of the backward d_cos[j][i] (the forward alone of a non-symmetric matrix is the per-edge
 *                    model's); the diagonal may hold any FINITE value and is ignored: no self loops (an inf or NaN
 *                    there reaches the outputs through 0 * d_cos[i][i])
 *   d_x      [N, 2]  node features {coef, |Q row|}
 *   d_params flat fp32 in PyG state_dict order: gconv1, gconv2, gconv3 (each lin_key {W [F,C], b [F]}, lin_query,
 *            lin_value, lin_edge {W [F,1]}, lin_skip {W, b}; C = 2 for gconv1, F otherwise), fc {W [1,F], b [1]}
 *            (mllp_angle_num_params floats; gconv3 is never called by the reference's forward: its gradient is 0)
 *   d_ws     mllp_angle_workspace_floats floats, kept between forward and backward; may be uninitialised (whatever
 *            it holds, NaN included, the same bits come out); d_ws and d_params 16-byte aligned (they are read in 16-byte
 *            pieces; MLLP_EINVAL otherwise); d_logits, d_dx and d_dcos need only their natural 4-byte alignment
 *   forward : d_logits [N - 1] = fc(h)[:-1]            backward: d_dlogits [N - 1] -> d_grads (layout of d_params)
 * Hand-written kernels on the fp32 matrix cores (v_mfma_f32_16x16x4_f32): flash-attention-style forward / backward
 * sweeps that keep no N x N matrix in HBM (the backward recomputes the weights from the saved row max / row sum) and one
 * strided GEMM for the projections and their gradients; no BLAS library is linked or loaded.  feat_dim must be 16, 32,
 * 64, 128 or 256 (MLLP_EINVAL otherwise); N <= 46340; the workspace is O(N * feat_dim * ranges), ranges <= 32.       */
int mllp_angle_num_params(int feat_dim, int64_t* out);
int mllp_angle_workspace_floats(int64_t n_nodes, int feat_dim, int64_t* out);
int mllp_angle_forward(int64_t n_nodes, int feat_dim, const float* d_cos, const float* d_x, const float* d_params,
                       float* d_ws, float* d_logits, void* stream);
int mllp_angle_backward(int64_t n_nodes, int feat_dim, const float* d_cos, const float* d_x, const float* d_params,
                        float* d_ws, const float* d_dlogits, float* d_grads, void* stream);

/* Input gradients of AngleModel (reference: PyG's TransformerConv is plain autograd, so model(g) is differentiable in g.x
 * and g.edge_attr as well as in the weights).  Call after mllp_angle_forward on this workspace, as mllp_angle_backward.
 * Runs mllp_angle_backward; the BQ sweep of each of the three layer applications also writes the gradient of the edge
 * attributes of its pairs (dz_ij qe_i + p_ij u_i), and the first layer's backward also forms dL/dx.
 *   d_grads : as mllp_angle_backward, bit for bit; required
 *   d_dx [N, 2] : dL/d_x;  d_dcos [N, N] : dL/dA_ij, indexed as d_cos (row = target i, column = source j: the gradient of
 *     the reference's edge j -> i), diagonal written as 0.  Each may be NULL (not computed, costs nothing); both NULL is
 *     exactly mllp_angle_backward.  Overwritten, not accumulated.  Bitwise reproducible: fixed launch order on `stream`,
 *     the three layers' terms summed in a fixed order, no float atomics.
 *   The key / value sweep reads d_cos transposed (above): d_dcos and d_grads are the per-edge model's only for a symmetric d_cos.
 * A null cos, x, params, workspace, dlogits or grads, a bad size or a bad feat_dim is rejected with a message before any
 * HIP call.  All work is queued on `stream`; nothing is allocated.                                                     */
int mllp_angle_backward_inputs(int64_t n_nodes, int feat_dim, const float* d_cos, const float* d_x,
                               const float* d_params, float* d_ws, const float* d_dlogits, float* d_grads,
                               float* d_dx, float* d_dcos, void* stream);

#ifdef __cplusplus
}
#endif
#endif /* MLLP_HIP_H */
