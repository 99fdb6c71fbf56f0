// internal.h -- shared declarations of libmllp_hip.so (not part of the public ABI)
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include <algorithm>
#include <string>
#include <vector>

#include "../../include/mllp_hip.h"

namespace mllp {

constexpr int FEAT = 16;
constexpr int BLOCK = 256;     // threads per workgroup (4 wavefronts of 64)
constexpr int REC_W = 40;      // floats per destination record read by the source-major backward sweep
constexpr int STAT_TILES = 7;  // 16x16 outer-product tiles reduced over nodes per conv
constexpr int STAT_FLOATS = STAT_TILES * 256;
constexpr int STAT_BLOCKS_MAX = 256;

void set_error(const std::string& msg);
int fail(int code, const std::string& msg);
int hip_fail(hipError_t e, const char* what);

#define MLLP_HIP_TRY(expr)                                              \
    do {                                                                \
        hipError_t _e = (expr);                                         \
        if (_e != hipSuccess) return ::mllp::hip_fail(_e, #expr);       \
    } while (0)

// argument check of an extern "C" entry point: the message names the function
#define REQUIRE(cond, msg) \
    if (!(cond)) return ::mllp::fail(MLLP_EINVAL, std::string(__func__) + ": " + (msg))
// REQUIRE on behalf of the entry point `fn`, in a function that several entry points share: the message names that function
#define REQUIRE_FOR(fn, cond, msg) \
    if (!(cond)) return ::mllp::fail(MLLP_EINVAL, std::string(fn) + ": " + (msg))

// after a kernel launch: the launch error, if any, under the kernel's name
inline int check_launch(const char* what) {
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MLLP_OK : hip_fail(e, what);
}

// scratch device buffer of a builder, freed when it goes out of scope
template <class T>
struct DevBuf {
    T* p = nullptr;
    ~DevBuf() { if (p) (void)hipFree(p); }
    int alloc(size_t n) { return hipMalloc((void**)&p, std::max<size_t>(n, 1) * sizeof(T)) == hipSuccess ? 0 : 1; }
};

// One traversal orientation: destination-major CSR over the sparsity pattern of A (dst = constraint
// rows) or of A^T (dst = variable columns).  Rows are split in three tiers by nonzero count:
//   group tier: 16 lanes per row (4 rows per wavefront), wave tier: 64 lanes per row,
//   block tier: one 256-thread workgroup per row.
// optional LDS-tiled copy of an orientation (tiled_kernels.hip); arrays are borrowed from the caller
// (mllp_graph_attach_tiled) or owned by the library (mllp_graph_build_tiled: tiled_build.hip)
struct Tiled {
    int n_tiles = 0, n_tb = 0, max_nbt = 0, max_run = 0;   // max_run: longest (tile, block) segment (library-built copies)
    bool owned = false;
    const int* tile_blk = nullptr;   // [n_tiles + 1]
    const int* blk_id = nullptr;     // [n_tb]
    const int* ptr2 = nullptr;       // [n_tb * rows_per_tile + 1] offsets of the length-sorted positions
    const int* perm = nullptr;       // [n_tb * rows_per_tile] row of each sorted position
    const int* ent = nullptr;        // [nnz][2] {col_local * 64 (byte offset of the source row in the staged block), value bits}
    int* vmap = nullptr;             // [nnz] value map of mllp_graph_set_values (set_values.hip; library-built copies)
};
// variants of the LDS-tiled copy (mllp_graph_attach_tiled / _build_tiled): the sweep whose geometry each one has
constexpr int TILED_SPMM = 0;     // plain SpMM
constexpr int TILED_ATTN = 1;     // attention forward
constexpr int TILED_BSRC = 2;     // source-major attention backward (this orientation = its rows)
constexpr int TILED_SCALAR = 3;   // layer-1 (one channel) attention sweeps, destination-major
constexpr int TILED_BDST = 4;     // destination-major attention backward
constexpr int TILED_VARIANTS = 5;

// streamed copy of an orientation (stream_layout.h): library-owned device arrays, built by mllp_graph_build_spmm_copy
struct StreamCopy {
    int n_tiles = 0, n_tb = 0;
    int64_t n_groups = 0;       // groups of 2 steps, without the padding groups at the end
    int64_t step_slots = 0;     // 128 x groups: entry slots of the stream, padding included
    int* tile_row = nullptr;    // [n_tiles + 1]
    int* tile_blk = nullptr;    // [n_tiles + 1]
    int* blk_id = nullptr;      // [n_tb]
    int* rows = nullptr;        // [n_tb * 8 * 16] int4
    int* hdr = nullptr;         // [n_tb * 8] int4
    int* ent = nullptr;         // [(n_groups + S_K0) * 64 * S_ENT]
    int* vmap = nullptr;        // [(n_groups + S_K0) * 64 * 2] value map of mllp_graph_set_values (set_values.hip)
    double build_seconds = 0.0;
};

// lane-per-row streamed copy of one orientation for the layer-1 sweeps (lane_layout.h, lane_stream.hip)
struct LaneCopy {
    int n_tiles = 0, n_tb = 0;
    int64_t n_groups = 0;       // groups of 4 steps, without the padding groups at the end
    int64_t nnz = 0;
    int* tile_row = nullptr;    // [n_tiles + 1]
    int* tile_blk = nullptr;    // [n_tiles + 1]
    int* tile_col = nullptr;    // [n_tiles][2]
    int* rows = nullptr;        // [n_tiles][L1_R]
    int* whdr = nullptr;        // [n_tb][L1_NW][2]
    unsigned* offs = nullptr;   // [(n_groups + L1_PADG) * 64 * 2]
    float* vals = nullptr;      // [(n_groups + L1_PADG) * 64 * 4]
    int* vmap = nullptr;        // [(n_groups + L1_PADG) * 64 * 4] value map of mllp_graph_set_values (set_values.hip)
    double build_seconds = 0.0;
};

// One device array of a re-blocked copy: the copy's pointer member and its byte count, computed from the copy's counts.
// A copy kind's table lists its arrays in the order of their export index (mllp_graph_export_stream_copy /
// mllp_graph_export_tiled `which`); allocation, upload, export, free and the copy's byte count all read it.
struct CopyArray {
    void** p;
    int64_t bytes;
};
enum { SC_TILE_BLK, SC_BLK_ID, SC_ROWS, SC_ENT, SC_TILE_ROW, SC_HDR };                    // StreamCopy
enum { LC_TILE_BLK, LC_TILE_COL, LC_ROWS, LC_OFFS, LC_TILE_ROW, LC_WHDR, LC_VALS };       // LaneCopy
enum { TL_TILE_BLK, TL_BLK_ID, TL_PTR2, TL_PERM, TL_ENT };                                // Tiled
std::vector<CopyArray> stream_copy_arrays(StreamCopy& sc, int geom);        // stream_api.cpp (geom: STREAM_GEOM_*)
std::vector<CopyArray> lane_copy_arrays(LaneCopy& lc);                      // stream_api.cpp
std::vector<CopyArray> tiled_arrays(Tiled& tl, int variant, int64_t nnz);   // tiled_build.hip (nnz: of the graph)
int copy_alloc(const CopyArray& a);                        // hipMalloc of *a.p, at least 4 bytes
void copy_free(const std::vector<CopyArray>& arrays);      // hipFree of the non-null ones

// Sweep precedence: a streamed copy over the LDS-tiled copy of the same sweep over the generic kernels; for the layer-1
// sweeps the lane copy over the TILED_SCALAR copy.
struct Orient {
    LaneCopy lane1;                     // geometry 4: layer-1 sweeps, destination-major (lane_stream.hip)
    StreamCopy stream[4];               // by STREAM_GEOM_* (stream_layout.h; stream_spmm.hip, stream_attn.hip)
    Tiled tiled[TILED_VARIANTS];        // by TILED_* (tiled_kernels.hip)
    int n_dst = 0, n_src = 0;
    int* ptr = nullptr;    // [n_dst + 1]
    int* idx = nullptr;    // [nnz] source ids
    float* val = nullptr;  // [nnz] a_ij
    int* rows_group = nullptr;  // nullptr => identity (every row is in the group tier)
    int* rows_wave = nullptr;
    int* chunks = nullptr;      // [n_chunk] int4 {row, beg, end, slot}; slot < 0: the row's only chunk
    int* split = nullptr;       // [n_split] int4 {row, first_slot, n_chunks, 0}: rows cut into several chunks
    int n_group = 0, n_wave = 0, n_chunk = 0, n_split = 0, n_slots = 0;
    float* scratch = nullptr;   // [n_slots x SCRATCH_NS] partial states of this orientation's split rows
    int tier_wave = 0;          // rows with more nonzeros than this are skipped by the group tier
    bool short_rows = false;    // mean row length <= 16: group tier runs one nonzero slot per pass
};
// One orientation of the fused latency-regime path in RENUMBERED node ids (host_graph.h::HostFusedOrient)
struct FusedTiersDev {
    int n_block = 0, n_wave = 0, n_group = 0, n_base = 0;
};
constexpr int FUSED_NP = 8;     // partitions of the instances (host_graph.h::FUSED_PARTS): one per XCD
struct FusedOrient {
    int n_dst = 0, n_src = 0, nnz = 0;
    int* sptr = nullptr;        // [n_dst + 1]
    int* sent = nullptr;        // [nnz][2] {source id (renumbered), value bits}
    float* sax = nullptr;       // [nnz][2] {a_ij, x_src} of the bound layer-1 inputs (scalar node features are data)
    int row0[FUSED_NP + 1] = {};
    FusedTiersDev t16[FUSED_NP], t1[FUSED_NP];
    // items of every wavefront (host_graph.h::HostWaveLists), [FUSED_NP][nw][L]: 16-channel sweeps at one workgroup per
    // CU (lst16) and at two (lst16x2: fused_src16_kernel), 1-channel sweeps (lst1)
    int* lst16 = nullptr; int* lst16x2 = nullptr; int* lst1 = nullptr;
    int L16 = 0, L16x2 = 0, L1 = 0, nw16 = 0, nw16x2 = 0, nw1 = 0;
};
constexpr int SCRATCH_NS = 20;  // floats per partial-state slot of a split row

}  // namespace mllp

struct mllp_graph {
    // (tests/test_pdhg_rays_oracle.py::_sizes stands in for a graph with these four words alone, for refusals and closed forms
    // that read nothing else of it: keep them first, or change that stand-in with them)
    int64_t M = 0, N = 0, nnz = 0, n_inst = 0;
    mllp::Orient A;   // dst = constraints, src = variables
    mllp::Orient At;  // dst = variables,   src = constraints
    float* inv_n = nullptr;      // [N] 1 / n_k of the owning instance
    int* inst_ptr_n = nullptr;   // [n_inst + 1] device
    int* inst_ptr_m = nullptr;   // [n_inst + 1] device
    std::vector<int64_t> h_inst_ptr_n, h_inst_ptr_m;
    std::vector<int> h_csr_ptr, h_csc_ptr;     // host copies of the row pointers (the fused path is built from them)
    int tier_wave = 0, tier_block = 0, chunk_nnz = 0;
    int max_inst_n = 0;
    int n_cu = 256;              // grid size of the persistent fused kernels: the device's compute units, lowered by the
                                 // limit in force at creation (mllp_set_fused_grid_limit)
    int n_cu_dev = 256;          // compute units of the device
    int64_t grid_limit = 0;      // that limit (0: none), kept because the fused arrays may be built later (set_path(2))
    int path = 0;                // whole-model path: 0 = by size (fused below 32 M nonzeros), 1 = generic / tiled, 2 = fused
    // fused path: renumbered copies of both orientations, permutations, renumbered copies of the bound inputs
    bool fused_built = false;
    mllp::FusedOrient FA, FAt;   // FA: rows = constraints, FAt: rows = variables
    int* perm_v = nullptr;       // [N] renumbered variable id -> original
    int* perm_c = nullptr;       // [M]
    int* inv_v = nullptr;        // [N] original -> renumbered
    int* inv_c = nullptr;        // [M]
    float* inv_n_p = nullptr;    // [N] 1 / n_k in renumbered order
    unsigned long long* tail_sync = nullptr;   // [4] grid-barrier state of fused_tail_kernel {arrivals, launches, error word, -}
    unsigned* tail_err_host = nullptr;         // host-mapped word that the kernel raises when its barrier times out
    unsigned* tail_err_dev = nullptr;          // ... its device address
    float* x1_p = nullptr;       // [N] bound inputs in renumbered order
    float* x2_p = nullptr;       // [M]
    float* labels_p = nullptr;   // [N]
    const void* bound_x1 = nullptr;
    const void* bound_x2 = nullptr;
    const void* bound_labels = nullptr;
    bool bind_captured = false;  // a hipGraph captured on this graph re-makes the copies at every replay: the cache is never trusted again
    // the workspace record: the mllp_gnn_forward whose activations a workspace holds -- which buffer, on which whole-model
    // path (0 generic / tiled, 1 fused: the two lay the workspace out differently) and with which parameters.  The backward
    // calls run only when all three are those of the call (include/mllp_hip.h, RECORDS); forget_forward() clears it
    int ws_path = -1;
    const void* ws_ptr = nullptr;
    const void* ws_params = nullptr;
    // which {workspace, parameters} hold the folded weights that fused_tail_kernel left behind for the NEXT step
    // (mllp_gnn_train_step flags bit 0 is honoured only when both match; every other whole-model call, a path switch
    // and the generic branch of train_step clear the record)
    const void* folded_ws = nullptr;
    const void* folded_params = nullptr;
    // input gradients: CSR position in A of every nonzero of A^T, built on the first mllp_gnn_backward_inputs call that
    // asks for dL/da (in `allocs`)
    // (mllp_graph_set_values refreshes At.val through the same map and builds it when it runs first)
    int* at_pos = nullptr;
    float* scale_buf = nullptr;  // [nnz] the scaled values of mllp_graph_scale_values, made on its first call (in `allocs`)
    float* norm_scale = nullptr; // [M + n_inst] row and objective scales of mllp_graph_normalize calls that pass no output
                                 // array, made on its first call (in `allocs`)
    int* plant_ws = nullptr;     // [N + M + 2] mllp_graph_plant_basis (planted.hip): owner row of every column (-1: nonbasic), CSR
                                 // position of every row's pivot, the error words; made on its first call (in `allocs`)
    // second stream + events: the two convs of a layer (one per orientation) and the single-workgroup
    // finalize kernels run beside the main stream (fork/join by events, also under hipGraph capture)
    hipStream_t aux = nullptr;
    hipEvent_t ev[16] = {};
    std::vector<void*> allocs;   // everything to hipFree on destroy
};

namespace mllp {

// the workspace no longer holds the activations of a forward that a backward call may use
inline void forget_forward(mllp_graph* g) {
    g->ws_ptr = g->ws_params = nullptr;
    g->ws_path = -1;
}

// a device array that a graph makes on the first call that needs it and frees with itself (in `allocs`): a no-op once `slot`
// is set.  Allocates: the first such call is not for a capture
template <class T>
inline int graph_alloc_once(mllp_graph* g, T*& slot, size_t bytes) {
    if (slot) return MLLP_OK;
    void* p = nullptr;
    MLLP_HIP_TRY(hipMalloc(&p, bytes));
    g->allocs.push_back(p);
    slot = static_cast<T*>(p);
    return MLLP_OK;
}

// ---- per-conv parameter views into the flat state_dict-ordered buffer ---------------------------
struct ConvParams {
    const float *Wk, *bk, *Wq, *bq, *Wv, *bv, *we, *Ws, *bs;
};
constexpr int conv_param_count(int cin) { return 4 * FEAT * cin + 5 * FEAT; }

// ---- the model's layout: GNNModel.state_dict() order ---------------------
// the five convs that are used, then the never-called gconv3_s2w (its gradient is zero), then fc (weight [16], bias)
enum { CONV_1V, CONV_1C, CONV_2V, CONV_2C, CONV_3V };   // gconv1_w2s, gconv1_s2w, gconv2_w2s, gconv2_s2w, gconv3_w2s
constexpr int MODEL_CONVS = CONV_3V + 1;
struct ConvSpec {
    bool dst_is_var;    // w2s: destinations are the variables (walks A^T); s2w: the constraints (walks A)
    int cin;
};
constexpr ConvSpec MODEL_CONV[MODEL_CONVS] = {{true, 1}, {false, 1}, {true, 16}, {false, 16}, {true, 16}};
struct ConvOffsets {
    int at[MODEL_CONVS + 1];    // at[MODEL_CONVS]: the end of the used convs
};
constexpr ConvOffsets conv_offsets() {
    ConvOffsets o = {};
    for (int c = 0; c < MODEL_CONVS; ++c) o.at[c + 1] = o.at[c] + conv_param_count(MODEL_CONV[c].cin);
    return o;
}
constexpr ConvOffsets CONV_OFF = conv_offsets();
constexpr int OFF_UNUSED = CONV_OFF.at[MODEL_CONVS], LEN_UNUSED = conv_param_count(FEAT);   // gconv3_s2w
constexpr int OFF_FC = OFF_UNUSED + LEN_UNUSED;
constexpr int NUM_PARAMS = OFF_FC + FEAT + 1;
static_assert(CONV_OFF.at[CONV_1V] == 0 && CONV_OFF.at[CONV_1C] == 144 && CONV_OFF.at[CONV_2V] == 288 &&
                  CONV_OFF.at[CONV_2C] == 1392 && CONV_OFF.at[CONV_3V] == 2496,
              "conv offsets differ from GNNModel.state_dict()");
static_assert(OFF_UNUSED == 3600 && LEN_UNUSED == 1104 && OFF_FC == 4704, "gconv3_s2w / fc offsets differ from state_dict()");
static_assert(NUM_PARAMS == MLLP_NUM_PARAMS, "the layout's total differs from MLLP_NUM_PARAMS");
// conv c of a flat parameter or gradient buffer
template <class T>
inline T* conv_at(T* base, int c) { return base + CONV_OFF.at[c]; }

inline ConvParams conv_params_at(const float* base, int cin) {
    ConvParams p;
    const float* q = base;
    p.Wk = q; q += FEAT * cin;
    p.bk = q; q += FEAT;
    p.Wq = q; q += FEAT * cin;
    p.bq = q; q += FEAT;
    p.Wv = q; q += FEAT * cin;
    p.bv = q; q += FEAT;
    p.we = q; q += FEAT;
    p.Ws = q; q += FEAT * cin;
    p.bs = q;
    return p;
}

// folded weights written by the param_prep kernel (per conv; DERIVED_W floats, same layout for cin 1/16)
//   Pq [k][d]  = sum_c Wk[c][k] Wq[c][d] / 4      q'_i = Pq x_i + pq0   (logit scale 1/sqrt(16) folded in)
//   PqT[d][k]  = Pq[k][d]
//   WsT[d][o]  = Ws[o][d]          WvT[k][o] = Wv[o][k]
//   pq0[k]     = sum_c Wk[c][k] bq[c] / 4
//   Pt [d]     = sum_c we[c] Wq[c][d] / 4 ,  pt0 = <bq, we> / 4        t_i = <Pt, x_i> + pt0
//   Pb [d]     = sum_c bk[c] Wq[c][d] / 4                              (backward only)
constexpr int OFF_PQ = 0, OFF_PQT = 256, OFF_WST = 512, OFF_WVT = 768;
constexpr int OFF_PQ0 = 1024, OFF_PT = 1040, OFF_PB = 1056, OFF_PT0 = 1072;
constexpr int DERIVED_W = 1088;

// workspace of one conv (floats): what forward saves for backward + backward scratch
struct ConvWs {
    float* derived;  // [DERIVED_W]
    float* qp;       // [n_dst, cin]
    float* t;        // [n_dst]
    float* Z;        // [n_dst, cin]   normalised attention-weighted source sum
    float* aux;      // [n_dst, 4]     {u, rowmax, 1/(rowsum+1e-16), S}
    float* rec;      // [n_dst, REC_W] backward record (cin = 16) / [n_dst, 8] (cin = 1)
    float* dqp;      // [n_dst, cin]
    float* dsdt;     // [n_dst, 2]
    float* stats;    // [STAT_BLOCKS_MAX, STAT_FLOATS] per-workgroup partial statistics
    float* red;      // [STAT_FLOATS] the summed statistics (fused path)
};
// the one listing of the fields, each rounded up to 16 floats; *end: where the next workspace starts.  Carving from
// nullptr measures: conv_ws_floats is what it advances by
ConvWs conv_ws_carve(float* base, int64_t n_dst, int cin, float** end = nullptr);
int64_t conv_ws_floats(int64_t n_dst, int cin);

// workspace of the whole model (api.cpp::model_ws carves it)
struct ModelWs {
    ConvWs c[MODEL_CONVS];      // by CONV_*
    float *h1v, *h1c, *h2v, *h2c, *h3v;
    float *d3v, *d2v, *d2c, *d1v, *d1c;
    float *d1v_b, *d1c_b;       // second contributions to dL/dh1 (fused path: separate buffers instead of +=)
    float* head_partials;
    int64_t total;
};

// ---- launchers (sweep_kernels.hip / node_kernels.hip) -------------------------------------------
int launch_spmm(const Orient& o, const float* H, float* Y, float* scratch, hipStream_t s);
int build_stream_device(const Orient& o, int64_t nnz, const std::vector<int>& tile_row, StreamCopy& sc, hipStream_t s,
                        int geom = 0);   // stream_build.hip (geom: stream_layout.h::STREAM_GEOM_*)
void stream_copy_free(StreamCopy& sc);                                                  // stream_api.cpp
int build_tiled_device(const Orient& o, int64_t nnz, int variant, Tiled& out, hipStream_t s);   // tiled_build.hip
void tiled_free(Tiled& tl);                                                             // tiled_build.hip (owned arrays only)
int launch_spmm_stream(const StreamCopy& sc, int n_dst, int n_src, const float* H, float* Y, hipStream_t s);
struct ConvWs;
int launch_fwd16_stream(const StreamCopy& sc, int n_dst, int n_src, const float* conv_params, const ConvWs& w,
                        const float* x_src, const float* x_dst, float* h_out, hipStream_t s);      // stream_attn.hip
int launch_bwddst16_stream(const StreamCopy& sc, int n_dst, int n_src, const ConvWs& w, const float* x_src, const float* g,
                           float* dx_dst, int accumulate, hipStream_t s);
struct ConvWs;
int launch_fwd1_lane(const LaneCopy& lc, int n_dst, int n_src, const float* conv_params, const ConvWs& w, const float* x_src,
                     const float* x_dst, float* h_out, hipStream_t s);                              // lane_stream.hip
int launch_bwddst1_lane(const LaneCopy& lc, int n_dst, int n_src, const ConvWs& w, const float* x_src, hipStream_t s);
int build_lane_copy(const Orient& o, int64_t nnz, const std::vector<int64_t>& seg, LaneCopy& lc, hipStream_t s);
void lane_copy_free(LaneCopy& lc);
int launch_bwdsrc16_stream(const StreamCopy& sc, int n_rows, int n_cols, const float* rec, const float* x_rows, float* dx,
                           int accumulate, hipStream_t s);
int launch_spmm_tiled(const Tiled& tl, int n_dst, int n_src, const float* H, float* Y, hipStream_t s);
int launch_spmm_tiled_bf16(const Tiled& tl, int n_dst, int n_src, const void* H_bf16, float* Y, hipStream_t s);
struct ConvWs;
int launch_fwd16_tiled(const Tiled& tl, int n_dst, int n_src, const float* conv_params, const ConvWs& w,
                       const float* x_src, const float* x_dst, float* h_out, hipStream_t s);
int launch_fwd1_tiled(const Tiled& tl, int n_dst, int n_src, const float* conv_params, const ConvWs& w,
                      const float* x_src, const float* x_dst, float* h_out, hipStream_t s);
int launch_bwddst1_tiled(const Tiled& tl, int n_dst, int n_src, const ConvWs& w, const float* x_src, hipStream_t s);
int launch_bwddst16_tiled(const Tiled& tl, int n_dst, int n_src, const ConvWs& w, const float* x_src, const float* g,
                          float* dx_dst, int accumulate, hipStream_t s);
int launch_bwdsrc16_tiled(const Tiled& tl, int n_rows, int n_cols, const float* rec, const float* x_rows, float* dx,
                          int accumulate, hipStream_t s);
int tiled_geometry(int variant, int* rows_per_tile, int* cols_per_block, int* bundle_capacity);
int tiled_max_blocks_per_tile();
int launch_param_prep_batch(int n, const float* const* conv_params, const int* cin, float* const* derived, hipStream_t s);
int launch_finalize_batch(int n, const float* const* conv_params, const int* cin, const float* const* stats,
                          const int* n_stat_blocks, float* const* grads, float* zero, int n_zero, hipStream_t s);
int launch_param_prep(const float* conv_params, int cin, float* derived, hipStream_t s);
int launch_node_qp(const float* x_dst, int64_t n_dst, const float* derived, float* qp, float* t, hipStream_t s);
int launch_attn_fwd(const Orient& o, int cin, const float* conv_params, const ConvWs& w, const float* x_src,
                    const float* x_dst, float* h_out, float* scratch, hipStream_t s);
int launch_bwd_pre(int64_t n_dst, int cin, const float* conv_params, const ConvWs& w, const float* x_dst,
                   const float* h_out, float* dh, hipStream_t s);
int launch_attn_bwd_dst(const Orient& o, int cin, const float* conv_params, const ConvWs& w, const float* x_src,
                        const float* g, float* dx_dst, int accumulate, float* scratch, hipStream_t s);
int launch_attn_bwd_src(const Orient& o_src_major, const ConvWs& w, const float* x_src, float* dx_src,
                        int accumulate, float* scratch, hipStream_t s);
int launch_attn_bwd_src1(const Orient& o_src_major, const ConvWs& w, const float* x_src, float* dx_src,
                         int accumulate, float* scratch, hipStream_t s);
// input gradients (input_grads.hip): edge-parallel dL/da_ij of one conv walking the destination-major CSR `o`, stored
// (accumulate = 0) or added into dval[pos ? pos[e] : e]; the At -> A position map; dx_dst of both layer-1 convs
int launch_edge_grad(const Orient& o, int64_t nnz, int cin, const ConvWs& w, const float* x_src, const int* pos, float* dval,
                     int accumulate, hipStream_t s);
int build_csc_to_csr(const mllp_graph* g, int* pos, hipStream_t s);
int ensure_at_pos(mllp_graph* g, hipStream_t s);   // set_values.hip: g->at_pos, built once per graph (allocates)
int ensure_scale_buf(mllp_graph* g);               // set_values.hip: g->scale_buf [nnz], made once per graph (allocates)
// set_values.hip: a caller-owned LDS-tiled copy is attached; its values are in arrays the library may not write, so
// mllp_graph_set_values, _scale_values and _normalize refuse with this message
bool borrowed_tiled(const mllp_graph* g);
#define MLLP_BORROWED_TILED_MSG                                                                                         \
    "a caller-owned LDS-tiled copy is attached (mllp_graph_attach_tiled): its arrays are not the library's to write. " \
    "Drop it (n_tiles = 0) or build the copy with mllp_graph_build_tiled"
int launch_layer1_dst_grads(const ConvWs& wv, const float* gv, float* dx1, int64_t n, const ConvWs& wc, const float* gc,
                            float* dx2, int64_t m, hipStream_t s);
int launch_param_stats(int cin, int64_t n_dst, const ConvWs& w, const float* x_dst, const float* g, hipStream_t s);
int launch_finalize_conv(int cin, const float* conv_params, const float* stats, int n_stat_blocks, float* grads,
                         hipStream_t s);
int stat_blocks_for(int64_t n_dst);

// head: mode 0 = logits only, 1 = backward from given dlogits, 2 = fused BCE forward+backward
int launch_head(int mode, int64_t n, const float* h3v, const float* fc_w, const float* fc_b, const float* inv_n,
                const float* labels, float inv_batch, const float* dlogits_in, float* logits, float* dh3v,
                float* partials, hipStream_t s);
int launch_head_finalize(const float* partials, int n_blocks, float* grad_fc /*17*/, float* loss /*nullable*/,
                         hipStream_t s);
int head_blocks_for(int64_t n);
int launch_adam(float* p, const float* g, float* m, float* v, float* state, float eps, float gscale, int64_t n,
                hipStream_t s);
int launch_fill_zero(float* p, int64_t n, hipStream_t s);

// ---- one-launch step of a small batch (small_step.hip): one workgroup, the caller's workspace in model_ws layout ------
// The limits of mllp_gnn_small_step_limits, stated once.  Floor of the ABI: M + N <= 2048 and nnz <= 8192 is eligible.
constexpr int64_t SMALL_STEP_MAX_NODES = 8192, SMALL_STEP_MAX_NNZ = 16384;
constexpr int SMALL_STEP_THREADS = 1024, SMALL_STEP_LDS_BYTES = 63296;
int launch_small_step(const mllp_graph* g, float* params, const float* x1, const float* x2, const float* labels,
                      float inv_batch, const ModelWs& w, float* logits, float* loss, float* grads, float* m, float* v,
                      float* state, float eps, hipStream_t s);   // m == nullptr: gradients only
int launch_topm_metrics(const mllp_graph* g, const float* logits, const float* labels, void* scratch, float* out,
                        hipStream_t s);
// select.hip: ptr_n / ptr_m [n_seg + 1] device, or ptr_n == nullptr for ONE segment of n_dense logits, m_dense to select
int launch_topm_select(const int* ptr_n, const int* ptr_m, int64_t n_seg, int n_dense, int m_dense, const float* logits,
                       unsigned char* mask, int* index, float* stats, hipStream_t s);

// ---- basis repair (basis.hip): one workgroup per instance keeps the m x m transform T and four vectors of m words ------
// The threshold between T in LDS and T in the caller's scratch, stated once: 192^2 + 4 * 192 words = 150 528 bytes, beside
// the kernel's 400 bytes of static LDS, within the 160 KB of a workgroup.  The vectors stay in LDS above it, which bounds
// the instances the call runs: 4 * 8192 words = 128 KB.  (At m = 8192 T alone is 256 MB and the elimination 2.7e11 updates.)
constexpr int BASIS_LDS_MAX_M = 192;
constexpr int BASIS_MAX_M = 8192;
__host__ __device__ constexpr int64_t basis_repair_vec_words(int64_t m) { return 4 * m; }       // w, prow, crow, piv
__host__ __device__ constexpr int64_t basis_repair_words(int64_t m) { return m * m; }           // scratch of one instance: T

// ---- basis simplex (simplex.hip): the same transform, pivoted on; six vectors of m words, all in LDS ---------------------
// Constants of this kernel alone (basis repair keeps its own).  T in LDS up to 192 rows: 192^2 + 6 * 192 words = 152 064
// bytes, beside under 1 KB of static LDS, within the 160 KB of a workgroup.  Above it T is in the caller's scratch and the
// vectors bound the rows: 6 * 4096 words = 96 KB.  Every instance that runs also takes n words of scratch (the shifts).
constexpr int SIMPLEX_LDS_MAX_M = 192;
constexpr int SIMPLEX_MAX_M = 4096;
__host__ __device__ constexpr int64_t simplex_vec_words(int64_t m) { return 6 * m; }    // w, staged row / rho, col of row, x_B, y, g_B
__host__ __device__ constexpr int64_t simplex_words(int64_t m, int64_t n) {              // scratch of one instance: T, shifts
    return (m > SIMPLEX_LDS_MAX_M ? m * m : 0) + n;
}

// ---- restarted PDHG, plain and preconditioned (pdhg.hip): one workgroup per instance, five vectors of 3 n + 2 m words ------
// x, xbar, xs, y, ys (pdhg_words) live in LDS up to PDHG_LDS_WORDS words: 144 KB, beside under 1 KB of static LDS, within the
// 160 KB of a workgroup (92 of the 97 Netlib instances fit); longer instances keep them in the caller's scratch, the same bits
// either way.  1024 threads: a workgroup is alone on its CU at that LDS size, and the sweeps read A from L2 / HBM in every
// iteration, so the sixteen wavefronts are what hides that latency.  mllp_lp_pdhg_limits reports both.
// The preconditioned entry point runs the same kernel source, so its threshold and threads ARE these, and the same 92
// instances fit.  Its four more vectors tc, xr, tr, yr (pdhg_scaled_side_words) are gathered by no sweep: they are read once per
// finished row, as c and b are, and live in the caller's scratch for EVERY instance: in LDS they would raise an instance's
// image to 5 n + 4 m words and move 8 more Netlib instances out of LDS (84 fit) to save one cached, coalesced load per row.
// mllp_lp_pdhg_scaled_limits reports its three constants.
constexpr int64_t PDHG_LDS_WORDS = 36864;
constexpr int PDHG_THREADS = 1024;
constexpr int64_t PDHG_SCALED_LDS_WORDS = PDHG_LDS_WORDS;
constexpr int PDHG_SCALED_THREADS = PDHG_THREADS;
constexpr int PDHG_SCALED_MAX_RUIZ = 64;
__host__ __device__ constexpr int64_t pdhg_words(int64_t m, int64_t n) { return 3 * n + 2 * m; }   // x, 2x+ - x, xs, y, ys
__host__ __device__ constexpr int64_t pdhg_scaled_side_words(int64_t m, int64_t n) { return 2 * n + 2 * m; }   // tc, xr, tr, yr

// ---- soft top-m loss head (topm_loss.hip): one workgroup of TOPM_LOSS_T threads per instance, many passes per evaluation ---
// Where an instance's scaled (and perturbed) logits a_i live between the passes, by its column count n alone: up to
// TOPM_LOSS_LDS_MAX columns in LDS (64 KB; word t + 1024 j belongs to thread t alone); longer instances form a_i again
// from the logits in every pass.  Sixteen registers per thread hold as much, but the sixteen unrolled exp / log1p chains
// spill at the 128 VGPRs of a 1024-thread workgroup (146 VGPRs spilled when tried).  The sums take the columns in the
// same order in both tiers, so the threshold changes the time and never a bit.  mllp_topm_loss_limits reports it.
constexpr int TOPM_LOSS_T = 1024;
constexpr int TOPM_LOSS_LDS_MAX = 16 * TOPM_LOSS_T;
constexpr int TOPM_LOSS_MAX_ITER = 64;

// ---- fused latency-regime path of the whole model (fused_kernels.hip) ---------------------------------
// one whole-model call: the flat parameters, the carved workspace, the call's inputs (labels, logits: null where unused)
struct FusedModel {
    const float* P;
    const ModelWs& w;
    const float *x1, *x2, *labels;
    float inv_batch;
    float* logits;
};
// api.cpp: the per-conv launches of the whole model that both paths share (one launch each for the five convs)
int model_param_prep(const float* P, const ModelWs& w, hipStream_t s);
int model_finalize(const mllp_graph* g, const float* P, const ModelWs& w, bool reduced, float* grads, hipStream_t s);
int fused_graph_build(mllp_graph* g, const int* h_csr_ptr, const int* h_csc_ptr);   // allocates: creation / set_path only
int fused_grid(const mllp_graph* g);
int fused_refill_values(mllp_graph* g, hipStream_t s);   // sent of both orientations from A.val / At.val again (launches only)
int fused_bind(mllp_graph* g, const float* x1, const float* x2, const float* labels, hipStream_t s);
// head_mode 1: all three layers, logits (h3v kept).  2 (loss step): layers 1 and 2 only -- layer 3, the logits, BCE and the
// fc partials come from the first launch of fused_backward(premasked = true), which must follow on the same workspace
int fused_forward(mllp_graph* g, const FusedModel& m, int head_mode, hipStream_t s, bool skip_prep = false);
// d3v = dlogits (original variable order) x fc weight in renumbered order, fc gradient partials
int fused_head_backward(const mllp_graph* g, const FusedModel& m, const float* dlogits, hipStream_t s);
// premasked: after fused_forward(head_mode 2); the first launch runs layer 3's forward, the loss head and C3's
// destination-major backward per item (Z / aux of C3, h3v and d3v are not written).  Else d3v = dL/dh3v (unmasked, from
// fused_head_backward after a forward with head_mode 1) and the caller has produced the fc gradient itself
// adam != nullptr: the single-rank tail (reduce + gradients + Adam + the next step's folded weights in one launch)
struct FusedAdam {
    float *params, *m, *v, *state;
    float eps;
    int n;
};
int fused_backward(const mllp_graph* g, const FusedModel& m, bool premasked, float* grads, float* loss, hipStream_t s,
                   const FusedAdam* adam = nullptr);
// fused_input_grads.hip: dL/dx1, dL/dx2, dL/da_ij (caller's order; each may be null) from what fused_backward left in
// m.w; m.x1 / m.x2 are the caller's inputs.  Launches only: g->at_pos must exist when dval is wanted (ensure_at_pos)
int fused_input_grads(const mllp_graph* g, const FusedModel& m, float* dx1, float* dx2, float* dval, hipStream_t s);

}  // namespace mllp
