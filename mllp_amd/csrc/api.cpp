// api.cpp -- extern "C" entry points: one TransformerConv layer, the whole GNNModel
// (reference linear_program_methods.py:202-251), the fused loss step, Adam, metrics.
#include <algorithm>

#include "internal.h"

namespace mllp {

static inline int64_t up16(int64_t x) { return (x + 15) & ~int64_t(15); }

// Caller pointers that the kernels read or write in 16-byte pieces (include/mllp_hip.h, "Memory contract"): the workspace
// (every field is carved at a multiple of 16 floats), the parameters (the fused head reads fc.weight four floats at a time),
// x1 / x2 (the lane-per-row copy of the layer-1 sweeps loads four source values at once) and every [n, 16] node array of the
// single-conv and SpMM calls.  A null pointer is aligned: the null checks have their own message.
static inline bool al16(const void* p) { return (reinterpret_cast<uintptr_t>(p) & 15) == 0; }
#define REQUIRE_ALIGNED16(cond) REQUIRE(cond, "misaligned pointer: " #cond " (these are accessed in 16-byte pieces)")

ConvWs conv_ws_carve(float* base, int64_t n, int cin, float** end) {
    const int64_t recw = cin == 16 ? REC_W : 8;
    float* p = base;
    auto take = [&](int64_t floats) {
        float* q = p;
        p += up16(floats);
        return q;
    };
    ConvWs w;
    w.derived = take(DERIVED_W);
    w.qp = take(n * cin);
    w.t = take(n);
    w.Z = take(n * cin);
    w.aux = take(n * 4);
    w.rec = take(n * recw);
    w.dqp = take(n * cin);
    w.dsdt = take(n * 2);
    w.stats = take((int64_t)STAT_BLOCKS_MAX * STAT_FLOATS);
    w.red = take(STAT_FLOATS);
    if (end) *end = p;
    return w;
}

int64_t conv_ws_floats(int64_t n, int cin) {
    float* end;
    conv_ws_carve(nullptr, n, cin, &end);
    return end - (float*)nullptr;
}

static int conv_forward(const mllp_graph* g, bool dst_is_var, int cin, const float* cp, const ConvWs& w,
                        const float* x_src, const float* x_dst, float* h_out, hipStream_t s, bool prep = true) {
    const Orient& o = dst_is_var ? g->At : g->A;
    int rc;
    if (prep && (rc = launch_param_prep(cp, cin, w.derived, s))) return rc;
    if (cin == 16 && (rc = launch_node_qp(x_dst, o.n_dst, w.derived, w.qp, w.t, s))) return rc;
    return launch_attn_fwd(o, cin, cp, w, x_src, x_dst, h_out, o.scratch, s);
}

// fork: work queued on `to` after this point waits for everything queued on `from` so far (capturable)
static int fork_to(hipStream_t from, hipStream_t to, hipEvent_t ev) {
    MLLP_HIP_TRY(hipEventRecord(ev, from));
    MLLP_HIP_TRY(hipStreamWaitEvent(to, ev, 0));
    return MLLP_OK;
}

// ---- whole-model workspace ----------------------------------------------------------------------
constexpr int HEAD_PART_FLOATS = 1024 * 18;

static ModelWs model_ws(const mllp_graph* g, float* base) {
    const int64_t N = g->N, M = g->M;
    ModelWs w;
    float* p = base;
    auto buf = [&](int64_t n) {
        float* q = p;
        p += up16(n);
        return q;
    };
    for (int c = 0; c < MODEL_CONVS; ++c)
        w.c[c] = conv_ws_carve(p, MODEL_CONV[c].dst_is_var ? N : M, MODEL_CONV[c].cin, &p);
    w.h1v = buf(N * 16); w.h1c = buf(M * 16);
    w.h2v = buf(N * 16); w.h2c = buf(M * 16);
    w.h3v = buf(N * 16);
    w.d3v = buf(N * 16); w.d2v = buf(N * 16); w.d2c = buf(M * 16);
    w.d1v = buf(N * 16); w.d1c = buf(M * 16);
    w.d1v_b = buf(N * 16); w.d1c_b = buf(M * 16);
    w.head_partials = buf(HEAD_PART_FLOATS);
    w.total = p - base;
    return w;
}

// folded weights of all five convs in one launch (they only depend on the parameters)
int model_param_prep(const float* P, const ModelWs& w, hipStream_t s) {
    const float* cps[MODEL_CONVS];
    int cins[MODEL_CONVS];
    float* ders[MODEL_CONVS];
    for (int c = 0; c < MODEL_CONVS; ++c) { cps[c] = conv_at(P, c); cins[c] = MODEL_CONV[c].cin; ders[c] = w.c[c].derived; }
    return launch_param_prep_batch(MODEL_CONVS, cps, cins, ders, s);
}

// the five single-workgroup finalize kernels (and the zero gradient of the never-used gconv3_s2w) as ONE launch, from the
// per-workgroup partial statistics or (reduced: the fused path) from their sums
int model_finalize(const mllp_graph* g, const float* P, const ModelWs& w, bool reduced, float* grads, hipStream_t s) {
    const float* cps[MODEL_CONVS];
    const float* sts[MODEL_CONVS];
    float* grs[MODEL_CONVS];
    int cins[MODEL_CONVS], nbs[MODEL_CONVS];
    for (int c = 0; c < MODEL_CONVS; ++c) {
        cps[c] = conv_at(P, c); cins[c] = MODEL_CONV[c].cin; grs[c] = conv_at(grads, c);
        sts[c] = reduced ? w.c[c].red : w.c[c].stats;
        nbs[c] = reduced ? 1 : stat_blocks_for((MODEL_CONV[c].dst_is_var ? g->At : g->A).n_dst);
    }
    return launch_finalize_batch(MODEL_CONVS, cps, cins, sts, nbs, grs, grads + OFF_UNUSED, LEN_UNUSED, s);
}

static int model_forward_body(const mllp_graph* g, const float* P, const float* x1, const float* x2, const ModelWs& w,
                              hipStream_t s) {
    int rc;
    hipStream_t a = g->aux;
    auto conv = [&](int c, const float* x_src, const float* x_dst, float* h_out, hipStream_t st) {
        return conv_forward(g, MODEL_CONV[c].dst_is_var, MODEL_CONV[c].cin, conv_at(P, c), w.c[c], x_src, x_dst, h_out, st,
                            false);
    };
    if ((rc = model_param_prep(P, w, s))) return rc;
    // linear_program_methods.py:241-242  layer 1 (scalar inputs), both directions from the SAME inputs:
    // the w2s conv walks A^T, the s2w conv walks A -- independent, so they run on two streams
    if ((rc = fork_to(s, a, g->ev[0]))) return rc;
    if ((rc = conv(CONV_1V, x2, x1, w.h1v, s))) return rc;
    if ((rc = conv(CONV_1C, x1, x2, w.h1c, a))) return rc;
    if ((rc = fork_to(a, s, g->ev[1]))) return rc;       // join: layer 2 on s needs h1c
    if ((rc = fork_to(s, a, g->ev[2]))) return rc;       // ... and layer 2 on aux needs h1v
    // :244-245  layer 2 (simultaneous update: both read layer-1 outputs)
    if ((rc = conv(CONV_2V, w.h1c, w.h1v, w.h2v, s))) return rc;
    if ((rc = conv(CONV_2C, w.h1v, w.h1c, w.h2c, a))) return rc;
    if ((rc = fork_to(a, s, g->ev[3]))) return rc;       // join
    // :247  layer 3, variables only (gconv3_s2w is never called, :248)
    return conv(CONV_3V, w.h2c, w.h2v, w.h3v, s);
}

// One conv of the backward pass, cut at its dependency points so that the two streams can interleave convs:
//   pre   bwd_pre                        needs dh (complete), writes rec, masks dh in place
//   dst   destination-major sweep        needs pre; writes dq', ds, dt and dx_dst
//   src   source-major sweep             needs pre; writes dx_src                       (independent of dst)
//   stat  parameter statistics           needs dst
//   fin   single-workgroup finalize      needs stat
// dh is overwritten with the ReLU-masked gradient; dx_* may be null; acc bit0 -> dx_dst, bit1 -> dx_src
struct ConvBwd {
    const mllp_graph* g;
    bool dst_is_var;
    int cin;
    const float* cp;
    const ConvWs& w;
    const float *x_src, *x_dst, *h_out;
    float *dh, *dx_dst, *dx_src;
    int acc;
    float* param_grads;
    const Orient& o() const { return dst_is_var ? g->At : g->A; }
    const Orient& ot() const { return dst_is_var ? g->A : g->At; }
    int pre(hipStream_t s) const { return launch_bwd_pre(o().n_dst, cin, cp, w, x_dst, h_out, dh, s); }
    int dst(hipStream_t s) const {
        return launch_attn_bwd_dst(o(), cin, cp, w, x_src, dh, cin == 16 ? dx_dst : nullptr, acc & 1, o().scratch, s);
    }
    int src(hipStream_t s) const {
        if (cin != 16 || !dx_src) return MLLP_OK;
        return launch_attn_bwd_src(ot(), w, x_src, dx_src, (acc >> 1) & 1, ot().scratch, s);
    }
    int stat(hipStream_t s) const { return launch_param_stats(cin, o().n_dst, w, x_dst, dh, s); }
    int fin(hipStream_t s) const {
        return launch_finalize_conv(cin, cp, w.stats, stat_blocks_for(o().n_dst), param_grads, s);
    }
};

// Backward of the five convs on two streams (s = caller's stream, a = the graph's aux stream, already forked from s
// by the caller).  Dependencies (linear_program_methods.py:241-247 read backwards):
//   C3 (dst = variables)   dh = d3v;  dst -> d2v,  src -> d2c
//   C2V (dst = variables)  dh = d2v;  dst -> d1v,  src -> d1c        (overwrite)
//   C2C (dst = constraints) dh = d2c; dst -> d1c +=, src -> d1v +=   (after C2V's src / dst respectively: C2V runs its
//                          source-major sweep first so that C2C's destination-major sweep can start early)
//   C1V dh = d1v, C1C dh = d1c (inputs are data: no input gradients)
// On the Netlib batch no single sweep fills the GPU (2.5 waves per SIMD resident), so running the source-major sweep
// of a conv next to its destination-major one, and C2C next to C2V, shortens the step; every sweep of one
// orientation still runs alone on that orientation's scratch (the waits below guarantee it).
static int model_backward_body(const mllp_graph* g, const float* P, const float* x1, const float* x2,
                               const ModelWs& w, float* grads, hipStream_t s) {
    int rc;
    hipStream_t a = g->aux;
    auto conv = [&](int c, const float* x_src, const float* x_dst, float* h_out, float* dh, float* dx_dst, float* dx_src,
                    int acc) {
        return ConvBwd{g, MODEL_CONV[c].dst_is_var, MODEL_CONV[c].cin, conv_at(P, c), w.c[c], x_src, x_dst, h_out, dh,
                       dx_dst, dx_src, acc, conv_at(grads, c)};
    };
    const ConvBwd c3 = conv(CONV_3V, w.h2c, w.h2v, w.h3v, w.d3v, w.d2v, w.d2c, 0);
    const ConvBwd c2v = conv(CONV_2V, w.h1c, w.h1v, w.h2v, w.d2v, w.d1v, w.d1c, 0);
    const ConvBwd c2c = conv(CONV_2C, w.h1v, w.h1c, w.h2c, w.d2c, w.d1c, w.d1v, 3);
    const ConvBwd c1v = conv(CONV_1V, x2, x1, w.h1v, w.d1v, nullptr, nullptr, 0);
    const ConvBwd c1c = conv(CONV_1C, x1, x2, w.h1c, w.d1c, nullptr, nullptr, 0);
#define TRY(x) if ((rc = (x))) return rc
#define REC(e, st) TRY(hipEventRecord(g->ev[e], st) == hipSuccess ? MLLP_OK : fail(MLLP_EHIP, "event record"))
#define WAIT(st, e) TRY(hipStreamWaitEvent(st, g->ev[e], 0) == hipSuccess ? MLLP_OK : fail(MLLP_EHIP, "stream wait"))
    // stream s                                     stream a
    TRY(c3.pre(s));
    TRY(fork_to(s, a, g->ev[8]));                // rec of C3 ready
    TRY(c3.dst(s));  REC(9, s);                  // s: d2v
    TRY(c3.src(a));  REC(13, a);                 //                                          a: d2c
    TRY(c2v.pre(s));
    WAIT(s, 13);                                 // C3's src shares A's scratch with C2V's src
    TRY(c2v.src(s)); REC(11, s);                 // s: d1c (overwrite) first: C2C's dst waits for it
    TRY(c2v.dst(s)); REC(10, s);                 // s: d1v (overwrite)
    TRY(c2v.stat(s));
    TRY(c2c.pre(a));                             //                                          a: dh = d2c
    WAIT(a, 9);
    TRY(c3.stat(a));                             //                                          a: needs C3's dst
    WAIT(a, 11);
    TRY(c2c.dst(a)); REC(14, a);                 //                                          a: d1c +=
    WAIT(a, 10);
    TRY(c2c.src(a)); REC(12, a);                 //                                          a: d1v +=
    WAIT(s, 14);
    TRY(c2c.stat(s));                            // s: statistics of C2C (its dst ran on a)
    // layer 1: the two convs are independent (their inputs are data): one per stream
    WAIT(s, 12);
    TRY(c1v.pre(s));                             // s: dh = d1v (C2V dst + C2C src)
    TRY(c1v.dst(s));
    TRY(c1v.stat(s));
    TRY(c1c.pre(a));                             //                                          a: dh = d1c (C2V src + C2C dst)
    TRY(c1c.dst(a));
    TRY(c1c.stat(a));
#undef REC
#undef WAIT
    TRY(fork_to(a, s, g->ev[0]));            // join everything queued on aux
#undef TRY
    return model_finalize(g, P, w, false, grads, s);
}

// ---- fused latency-regime path ------------------------------------------------------------------------
static bool use_fused(const mllp_graph* g) {
    if (g->path == 1 || !g->fused_built) return false;
    if (g->path == 2) return true;
    return g->nnz < ((int64_t)32 << 20);     // the throughput regime keeps the generic / LDS-tiled sweeps
}

// the workspace record names this workspace, the path in use and these parameters: d_ws holds what a backward call with
// these arguments reads (internal.h; include/mllp_hip.h, RECORDS)
static bool forward_recorded(const mllp_graph* g, const void* d_ws, const void* d_params) {
    return g->ws_ptr == d_ws && g->ws_path == (use_fused(g) ? 1 : 0) && g->ws_params == d_params;
}
#define REQUIRE_FORWARD_PARAMS(g, d_params)                                                                                  \
    REQUIRE((g)->ws_params == (d_params), "the mllp_gnn_forward on this workspace ran with other parameters (another d_params " \
                                          "pointer): its activations are not those of this model")

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_spmm_csr_f32(const mllp_graph_t* g, int transpose, const float* d_H, float* d_Y, void* stream) {
    REQUIRE(g && d_H && d_Y, "null argument");
    REQUIRE_ALIGNED16(al16(d_H) && al16(d_Y));
    const Orient& o = transpose ? g->At : g->A;
    return launch_spmm(o, d_H, d_Y, o.scratch, (hipStream_t)stream);
}

extern "C" int mllp_spmm_csr_bf16(const mllp_graph_t* g, int transpose, const void* d_H_bf16, float* d_Y, void* stream) {
    REQUIRE(g && d_H_bf16 && d_Y, "null argument");
    const Orient& o = transpose ? g->At : g->A;
    const Tiled& tl = o.tiled[TILED_SPMM];
    REQUIRE(tl.n_tiles > 0 || o.n_dst == 0 || g->nnz == 0,
            "mllp_spmm_csr_bf16 runs on the LDS-tiled copy of the orientation (mllp_graph_attach_tiled, variant 0): attach it first");
    if (tl.n_tiles == 0) {     // no nonzeros: Y = 0
        if (o.n_dst > 0) MLLP_HIP_TRY(hipMemsetAsync(d_Y, 0, (size_t)o.n_dst * 16 * sizeof(float), (hipStream_t)stream));
        return MLLP_OK;
    }
    return launch_spmm_tiled_bf16(tl, o.n_dst, o.n_src, d_H_bf16, d_Y, (hipStream_t)stream);
}

extern "C" int mllp_graph_invalidate_inputs(mllp_graph_t* g) {
    REQUIRE(g, "null graph");
    g->bound_x1 = g->bound_x2 = g->bound_labels = nullptr;
    return MLLP_OK;
}

extern "C" int mllp_graph_set_path(mllp_graph_t* g, int path) {
    REQUIRE(g, "null graph");
    REQUIRE(path >= 0 && path <= 2, "path must be 0 (by size), 1 (generic / LDS-tiled sweeps) or 2 (fused latency-regime kernels)");
    if (path == 2 && !g->fused_built) {        // (allocates: not a launch function)
        const int rc = fused_graph_build(g, g->h_csr_ptr.data(), g->h_csc_ptr.data());
        if (rc) return rc;
    }
    g->path = path;
    g->folded_ws = g->folded_params = nullptr;      // the other path does not maintain the folded weights
    return MLLP_OK;
}

extern "C" int mllp_tiled_geometry(int variant, int32_t* rows_per_tile, int32_t* cols_per_block,
                                   int32_t* bundle_capacity) {
    REQUIRE(rows_per_tile && cols_per_block && bundle_capacity, "null argument");
    REQUIRE(variant >= 0 && variant <= 4, "variant must be 0 (SpMM), 1 (attention forward), 2 / 4 (attention backward, source- / destination-major) or 3 (layer-1 sweeps)");
    int a, b, c;
    tiled_geometry(variant, &a, &b, &c);
    *rows_per_tile = a; *cols_per_block = b; *bundle_capacity = c;
    return MLLP_OK;
}

extern "C" int mllp_graph_attach_tiled(mllp_graph_t* g, int transpose, int variant, int64_t n_tiles, int64_t n_tb,
                                       int32_t max_blocks_per_tile,
                                       const int32_t* d_tile_blk, const int32_t* d_blk_id, const int32_t* d_ptr2,
                                       const int32_t* d_perm, const int32_t* d_ent) {
    REQUIRE(g, "null graph");
    REQUIRE(variant >= 0 && variant <= 4, "variant must be 0 (SpMM), 1 (attention forward), 2 / 4 (attention backward, source- / destination-major) or 3 (layer-1 sweeps)");
    Orient& o = transpose ? g->At : g->A;
    Tiled& tl = o.tiled[variant];
    if (n_tiles == 0) {   // detach
        tiled_free(tl);
        return MLLP_OK;
    }
    REQUIRE(d_tile_blk && d_blk_id && d_ptr2 && d_perm && d_ent, "null array");
    int R, CB, CAP;
    tiled_geometry(variant, &R, &CB, &CAP);
    REQUIRE(n_tiles == (o.n_dst + R - 1) / R, "n_tiles must be ceil(rows / rows_per_tile)");
    REQUIRE(n_tb > 0 && n_tb * (int64_t)R < INT32_MAX, "bad (tile, block) count");
    REQUIRE(max_blocks_per_tile > 0 && max_blocks_per_tile <= tiled_max_blocks_per_tile(),
            "a row tile touches more column blocks than the kernel's table holds");
    tiled_free(tl);
    tl.n_tiles = (int)n_tiles; tl.n_tb = (int)n_tb; tl.max_nbt = max_blocks_per_tile;
    tl.tile_blk = d_tile_blk; tl.blk_id = d_blk_id; tl.ptr2 = d_ptr2; tl.perm = d_perm;
    tl.ent = d_ent;
    return MLLP_OK;
}

extern "C" int mllp_graph_build_tiled(mllp_graph_t* g, int transpose, int variant, void* stream) {
    REQUIRE(g, "null graph");
    REQUIRE(variant >= 0 && variant <= 4, "variant must be 0 (SpMM), 1 (attention forward), 2 / 4 (attention backward, source- / destination-major) or 3 (layer-1 sweeps)");
    Orient& o = transpose ? g->At : g->A;
    Tiled fresh;
    const int rc = build_tiled_device(o, g->nnz, variant, fresh, (hipStream_t)stream);
    if (rc) {
        tiled_free(fresh);
        return rc;
    }
    Tiled& tl = o.tiled[variant];
    tiled_free(tl);
    tl = fresh;
    return MLLP_OK;
}

extern "C" int mllp_graph_tiled_info(const mllp_graph_t* g, int transpose, int variant, int64_t* info) {
    REQUIRE(g && info, "null argument");
    REQUIRE(variant >= 0 && variant <= 4, "variant must be 0..4");
    const Tiled& tl = (transpose ? g->At : g->A).tiled[variant];
    info[0] = tl.n_tiles; info[1] = tl.n_tb; info[2] = tl.max_nbt; info[3] = tl.owned ? 1 : 0; info[4] = tl.max_run;
    return MLLP_OK;
}

extern "C" int mllp_graph_export_tiled(const mllp_graph_t* g, int transpose, int variant, int which, int32_t* d_dst,
                                       int64_t count, void* stream) {
    REQUIRE(g && d_dst, "null argument");
    REQUIRE(variant >= 0 && variant <= 4, "variant must be 0..4");
    Tiled& tl = const_cast<Tiled&>((transpose ? g->At : g->A).tiled[variant]);
    REQUIRE(tl.n_tiles > 0, "no tiled copy of this variant is attached");
    const std::vector<CopyArray> arrays = tiled_arrays(tl, variant, g->nnz);
    REQUIRE(which >= 0 && which < (int)arrays.size(), "which must be 0 (tile_blk), 1 (blk_id), 2 (ptr2), 3 (perm) or 4 (ent)");
    const CopyArray& a = arrays[which];
    REQUIRE(count * 4 == a.bytes, "count does not match the array's length");
    MLLP_HIP_TRY(hipMemcpyAsync(d_dst, *a.p, (size_t)a.bytes, hipMemcpyDeviceToDevice, (hipStream_t)stream));
    return MLLP_OK;
}

extern "C" int mllp_tconv_workspace_floats(const mllp_graph_t* g, int dst_is_var, int cin, int64_t* n_floats) {
    REQUIRE(g && n_floats, "null argument");
    REQUIRE(cin == 1 || cin == 16, "cin must be 1 or 16");
    *n_floats = conv_ws_floats(dst_is_var ? g->N : g->M, cin);
    return MLLP_OK;
}

extern "C" int mllp_tconv_fwd(const mllp_graph_t* g, int dst_is_var, int cin, const float* d_conv_params,
                              const float* d_x_src, const float* d_x_dst, float* d_h_out, float* d_ws, void* stream) {
    REQUIRE(g && d_conv_params && d_x_src && d_x_dst && d_h_out && d_ws, "null argument");
    REQUIRE(cin == 1 || cin == 16, "cin must be 1 or 16");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_conv_params) && al16(d_x_src) && al16(d_x_dst) && al16(d_h_out));
    ConvWs w = conv_ws_carve(d_ws, dst_is_var ? g->N : g->M, cin);
    return conv_forward(g, dst_is_var != 0, cin, d_conv_params, w, d_x_src, d_x_dst, d_h_out, (hipStream_t)stream);
}

extern "C" int mllp_tconv_bwd(const mllp_graph_t* g, int dst_is_var, int cin, const float* d_conv_params,
                              const float* d_x_src, const float* d_x_dst, const float* d_h_out, float* d_ws,
                              float* d_dh, float* d_dx_dst, float* d_dx_src, int accumulate, float* d_param_grads,
                              void* stream) {
    REQUIRE(g && d_conv_params && d_x_src && d_x_dst && d_h_out && d_ws && d_dh && d_param_grads, "null argument");
    REQUIRE(cin == 1 || cin == 16, "cin must be 1 or 16");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_conv_params) && al16(d_x_src) && al16(d_x_dst) && al16(d_h_out) && al16(d_dh) &&
                      al16(d_dx_dst) && al16(d_dx_src));
    ConvWs w = conv_ws_carve(d_ws, dst_is_var ? g->N : g->M, cin);
    const ConvBwd c{g, dst_is_var != 0, cin, d_conv_params, w, d_x_src, d_x_dst, d_h_out, d_dh, d_dx_dst, d_dx_src, accumulate,
                    d_param_grads};
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if ((rc = c.pre(s)) || (rc = c.dst(s)) || (rc = c.src(s)) || (rc = c.stat(s))) return rc;
    return c.fin(s);
}

extern "C" int mllp_gnn_workspace_bytes(const mllp_graph_t* g, int64_t* bytes) {
    REQUIRE(g && bytes, "null argument");
    *bytes = model_ws(g, nullptr).total * (int64_t)sizeof(float);
    return MLLP_OK;
}

extern "C" int mllp_gnn_forward(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                                void* d_ws, float* d_logits, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_ws && d_logits, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    hipStream_t s = (hipStream_t)stream;
    ModelWs w = model_ws(g, (float*)d_ws);
    int rc;
    mllp_graph* gm = const_cast<mllp_graph*>(g);          // (bookkeeping only: which path wrote which workspace)
    gm->ws_ptr = d_ws;
    gm->ws_path = use_fused(g) ? 1 : 0;
    gm->ws_params = d_params;
    gm->folded_ws = gm->folded_params = nullptr;
    if (use_fused(g))
        return fused_forward(gm, FusedModel{d_params, w, d_x1, d_x2, nullptr, 0.0f, d_logits}, 1, s);
    if ((rc = model_forward_body(g, d_params, d_x1, d_x2, w, s))) return rc;
    return launch_head(0, g->N, w.h3v, d_params + OFF_FC, d_params + OFF_FC + FEAT, g->inv_n, nullptr, 0.0f, nullptr,
                       d_logits, nullptr, w.head_partials, s);
}

extern "C" int mllp_gnn_backward(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                                 void* d_ws, const float* d_dlogits, float* d_grads, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_ws && d_dlogits && d_grads, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    hipStream_t s = (hipStream_t)stream;
    ModelWs w = model_ws(g, (float*)d_ws);
    int rc;
    // the two paths lay the workspace out differently (the fused one in renumbered node order): backward must follow
    // a forward of the same path on the same workspace
    REQUIRE(g->ws_ptr == d_ws && g->ws_path == (use_fused(g) ? 1 : 0),
            "no mllp_gnn_forward on this workspace with the current path (mllp_graph_set_path between forward and backward? "
            "A train step, mllp_graph_set_values, or a loss step with other parameters since the forward?)");
    REQUIRE_FORWARD_PARAMS(g, d_params);
    if (use_fused(g)) {      // (the node tensors of the fused path are in renumbered order: it has its own head kernel)
        const FusedModel m{d_params, w, d_x1, d_x2, nullptr, 0.0f, nullptr};
        if ((rc = fused_bind(const_cast<mllp_graph*>(g), d_x1, d_x2, nullptr, s))) return rc;
        if ((rc = fused_head_backward(g, m, d_dlogits, s))) return rc;
        return fused_backward(g, m, false, d_grads, nullptr, s);
    }
    if ((rc = launch_head(1, g->N, w.h3v, d_params + OFF_FC, d_params + OFF_FC + FEAT, g->inv_n, nullptr, 0.0f,
                          d_dlogits, nullptr, w.d3v, w.head_partials, s))) return rc;
    if ((rc = fork_to(s, g->aux, g->ev[1]))) return rc;
    if ((rc = launch_head_finalize(w.head_partials, head_blocks_for(g->N), d_grads + OFF_FC, nullptr, g->aux))) return rc;
    return model_backward_body(g, d_params, d_x1, d_x2, w, d_grads, s);
}

// Input gradients after the generic backward (post-pass on s; input_grads.hip, BwdSrc1Op).  Fixed order, no atomics:
//   dx1 = dx_dst(gconv1_w2s) + dx_src(gconv1_s2w),  dx2 = dx_dst(gconv1_s2w) + dx_src(gconv1_w2s)
//   dval = the edge terms of gconv1_s2w, gconv2_s2w (walking A), gconv1_w2s, gconv2_w2s, gconv3_w2s (walking A^T,
//          placed by g->at_pos); the first stores, the others add
static int input_grads_body(const mllp_graph* g, const float* x1, const float* x2, const ModelWs& w, float* dx1,
                            float* dx2, float* dval, hipStream_t s) {
    int rc;
    // dL/da of conv c from its destination-major walk: A in place, A^T through the position map
    auto edge = [&](int c, const float* x_src, int accumulate) {
        const bool t = MODEL_CONV[c].dst_is_var;
        return launch_edge_grad(t ? g->At : g->A, g->nnz, MODEL_CONV[c].cin, w.c[c], x_src, t ? g->at_pos : nullptr, dval,
                                accumulate, s);
    };
    if ((rc = launch_layer1_dst_grads(w.c[CONV_1V], w.d1v, dx1, g->N, w.c[CONV_1C], w.d1c, dx2, g->M, s))) return rc;
    if (dx1 && (rc = launch_attn_bwd_src1(g->At, w.c[CONV_1C], x1, dx1, 1, g->At.scratch, s))) return rc;
    if (dx2 && (rc = launch_attn_bwd_src1(g->A, w.c[CONV_1V], x2, dx2, 1, g->A.scratch, s))) return rc;
    if (!dval) return MLLP_OK;
    if ((rc = edge(CONV_1C, x1, 0)) || (rc = edge(CONV_2C, w.h1v, 1)) || (rc = edge(CONV_1V, x2, 1)) ||
        (rc = edge(CONV_2V, w.h1c, 1))) return rc;
    return edge(CONV_3V, w.h2c, 1);
}

extern "C" int mllp_gnn_loss_step(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                                  const float* d_labels, float inv_batch, void* d_ws, float* d_logits, float* d_loss,
                                  float* d_grads, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_labels && d_ws && d_logits && d_loss && d_grads, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    hipStream_t s = (hipStream_t)stream;
    ModelWs w = model_ws(g, (float*)d_ws);
    int rc;
    mllp_graph* gm = const_cast<mllp_graph*>(g);
    gm->folded_ws = gm->folded_params = nullptr;
    // the step rewrites the workspace with ITS forward (on the fused path all of it but layer 3's saved state, which a
    // recorded forward left).  After a recorded forward on this workspace, this path and these parameters those are the
    // bits that are there already and the record stays; after any other the workspace belongs to no forward
    if (!forward_recorded(g, d_ws, d_params)) forget_forward(gm);
    if (use_fused(g)) {
        const FusedModel m{d_params, w, d_x1, d_x2, d_labels, inv_batch, d_logits};
        if ((rc = fused_forward(const_cast<mllp_graph*>(g), m, 2, s))) return rc;
        return fused_backward(g, m, true, d_grads, d_loss, s);
    }
    if ((rc = model_forward_body(g, d_params, d_x1, d_x2, w, s))) return rc;
    if ((rc = launch_head(2, g->N, w.h3v, d_params + OFF_FC, d_params + OFF_FC + FEAT, g->inv_n, d_labels, inv_batch,
                          nullptr, d_logits, w.d3v, w.head_partials, s))) return rc;
    if ((rc = fork_to(s, g->aux, g->ev[1]))) return rc;
    if ((rc = launch_head_finalize(w.head_partials, head_blocks_for(g->N), d_grads + OFF_FC, d_loss, g->aux))) return rc;
    return model_backward_body(g, d_params, d_x1, d_x2, w, d_grads, s);
}

extern "C" int mllp_gnn_input_grads_scratch_bytes(const mllp_graph_t* g, int64_t* bytes) {
    REQUIRE(g && bytes, "null argument");
    *bytes = up16(MLLP_NUM_PARAMS) * (int64_t)sizeof(float);     // the parameter gradients when d_grads is null
    return MLLP_OK;
}

extern "C" int mllp_gnn_backward_inputs(const mllp_graph_t* g, const float* d_params, const float* d_x1,
                                        const float* d_x2, void* d_ws, const float* d_dlogits, float* d_grads,
                                        float* d_dx1, float* d_dx2, float* d_dvalues, void* d_scratch, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_ws && d_dlogits, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    REQUIRE(g->ws_ptr == d_ws, "no mllp_gnn_forward on this workspace");
    REQUIRE(g->ws_path == 0, "the forward on this workspace ran on the fused path: input gradients need the generic "
                             "sweeps (mllp_graph_set_path(g, 1) before mllp_gnn_forward)");
    REQUIRE(!use_fused(g), "the graph's path selects the fused kernels: set path 1 between the forward and this call");
    REQUIRE_FORWARD_PARAMS(g, d_params);
    REQUIRE(d_grads || d_scratch, "d_grads and d_scratch are both null (mllp_gnn_input_grads_scratch_bytes)");
    hipStream_t s = (hipStream_t)stream;
    mllp_graph* gm = const_cast<mllp_graph*>(g);
    int rc;
    if (d_dvalues && (rc = ensure_at_pos(gm, s))) return rc;      // once per graph (allocates: make the first such call uncaptured)
    float* grads = d_grads ? d_grads : (float*)d_scratch;
    if ((rc = mllp_gnn_backward(g, d_params, d_x1, d_x2, d_ws, d_dlogits, grads, stream))) return rc;
    return input_grads_body(g, d_x1, d_x2, model_ws(g, (float*)d_ws), d_dx1, d_dx2, d_dvalues, s);
}

// Input gradients on whichever path the forward on d_ws used.  Generic: mllp_gnn_backward_inputs itself.  Fused: the
// fused backward, then the post-pass for a renumbered workspace (fused_input_grads.hip).
extern "C" int mllp_gnn_input_grads(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                                    void* d_ws, const float* d_dlogits, float* d_grads, float* d_dx1, float* d_dx2,
                                    float* d_dvalues, void* d_scratch, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_ws && d_dlogits, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    REQUIRE(d_grads || d_scratch, "d_grads and d_scratch are both null (mllp_gnn_input_grads_scratch_bytes)");
    REQUIRE(g->ws_ptr == d_ws, "no mllp_gnn_forward on this workspace");
    REQUIRE(g->ws_path == (use_fused(g) ? 1 : 0),
            "the path was switched between the forward on this workspace and this call (mllp_graph_set_path)");
    REQUIRE_FORWARD_PARAMS(g, d_params);
    if (!use_fused(g))
        return mllp_gnn_backward_inputs(g, d_params, d_x1, d_x2, d_ws, d_dlogits, d_grads, d_dx1, d_dx2, d_dvalues, d_scratch,
                                        stream);
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (d_dvalues && (rc = ensure_at_pos(const_cast<mllp_graph*>(g), s))) return rc;      // once per graph (allocates: make the first such call uncaptured)
    float* grads = d_grads ? d_grads : (float*)d_scratch;
    if ((rc = mllp_gnn_backward(g, d_params, d_x1, d_x2, d_ws, d_dlogits, grads, stream))) return rc;
    const ModelWs w = model_ws(g, (float*)d_ws);
    return fused_input_grads(g, FusedModel{d_params, w, d_x1, d_x2, nullptr, 0.0f, nullptr}, d_dx1, d_dx2, d_dvalues, s);
}

// mllp_gnn_loss_step, then the post-pass of the path in use
extern "C" int mllp_gnn_loss_step_inputs(const mllp_graph_t* g, const float* d_params, const float* d_x1,
                                         const float* d_x2, const float* d_labels, float inv_batch, void* d_ws,
                                         float* d_logits, float* d_loss, float* d_grads, float* d_dx1, float* d_dx2,
                                         float* d_dvalues, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_labels && d_ws && d_logits && d_loss && d_grads, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    hipStream_t s = (hipStream_t)stream;
    int rc;
    if (d_dvalues && (rc = ensure_at_pos(const_cast<mllp_graph*>(g), s))) return rc;      // once per graph, as above
    if ((rc = mllp_gnn_loss_step(g, d_params, d_x1, d_x2, d_labels, inv_batch, d_ws, d_logits, d_loss, d_grads, stream)))
        return rc;
    const ModelWs w = model_ws(g, (float*)d_ws);
    if (use_fused(g))
        return fused_input_grads(g, FusedModel{d_params, w, d_x1, d_x2, d_labels, inv_batch, d_logits}, d_dx1, d_dx2,
                                 d_dvalues, s);
    return input_grads_body(g, d_x1, d_x2, w, d_dx1, d_dx2, d_dvalues, s);
}

extern "C" int mllp_gnn_train_step(const mllp_graph_t* g, float* d_params, const float* d_x1, const float* d_x2,
                                   const float* d_labels, float inv_batch, void* d_ws, float* d_logits, float* d_loss,
                                   float* d_grads, float* d_exp_avg, float* d_exp_avg_sq, float* d_state, float eps,
                                   int flags, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_labels && d_ws && d_logits && d_loss && d_grads, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    REQUIRE(d_exp_avg && d_exp_avg_sq && d_state, "null optimizer state");
    REQUIRE((flags & ~1) == 0, "flags: bit 0 = the folded weights in the workspace are current");
    hipStream_t s = (hipStream_t)stream;
    int rc;
    mllp_graph* gm = const_cast<mllp_graph*>(g);
    forget_forward(gm);      // the step rewrites the workspace and then the parameters: no backward call may follow it
    if (use_fused(g)) {
        ModelWs w = model_ws(g, (float*)d_ws);
        const FusedModel m{d_params, w, d_x1, d_x2, d_labels, inv_batch, d_logits};
        // bit 0 is the caller's claim that the parameters are unchanged since the last call; the library checks on its
        // side that the last whole-model call on this graph was a fused train_step on this workspace and these parameters
        const bool skip = (flags & 1) != 0 && gm->folded_ws == d_ws && gm->folded_params == d_params;
        gm->folded_ws = gm->folded_params = nullptr;
        if ((rc = fused_forward(gm, m, 2, s, skip))) return rc;
        const FusedAdam a = {d_params, d_exp_avg, d_exp_avg_sq, d_state, eps, (int)MLLP_NUM_PARAMS};
        if ((rc = fused_backward(g, m, true, d_grads, d_loss, s, &a))) return rc;
        gm->folded_ws = d_ws;
        gm->folded_params = d_params;
        return MLLP_OK;
    }
    gm->folded_ws = gm->folded_params = nullptr;
    // throughput regime: the same two calls a caller would make (the tail is 0.1 % of such a step)
    if ((rc = mllp_gnn_loss_step(g, d_params, d_x1, d_x2, d_labels, inv_batch, d_ws, d_logits, d_loss, d_grads, stream)))
        return rc;
    return launch_adam(d_params, d_grads, d_exp_avg, d_exp_avg_sq, d_state, eps, 1.0f, MLLP_NUM_PARAMS, s);
}

// ---- one-launch step of a small batch (small_step.hip) ---------------------------------------------------------------
extern "C" int mllp_gnn_small_step_limits(int64_t limits[4]) {
    REQUIRE(limits, "null argument");
    limits[0] = SMALL_STEP_MAX_NODES; limits[1] = SMALL_STEP_MAX_NNZ;
    limits[2] = SMALL_STEP_THREADS; limits[3] = SMALL_STEP_LDS_BYTES;
    return MLLP_OK;
}

// empty when g is within the limits, else the sentence that names the limit it exceeds
static std::string small_step_excess(const mllp_graph* g) {
    if (g->M + g->N > SMALL_STEP_MAX_NODES)
        return "the graph has " + std::to_string(g->M + g->N) + " nodes, the limit is " + std::to_string(SMALL_STEP_MAX_NODES);
    if (g->nnz > SMALL_STEP_MAX_NNZ)
        return "the graph has " + std::to_string(g->nnz) + " nonzeros, the limit is " + std::to_string(SMALL_STEP_MAX_NNZ);
    return std::string();
}

extern "C" int mllp_gnn_small_step_fits(const mllp_graph_t* g, int* fits) {
    REQUIRE(g && fits, "null argument");
    *fits = small_step_excess(g).empty() ? 1 : 0;
    return MLLP_OK;
}

extern "C" int mllp_gnn_train_step_small(const mllp_graph_t* g, float* d_params, const float* d_x1, const float* d_x2,
                                         const float* d_labels, float inv_batch, void* d_ws, float* d_logits,
                                         float* d_loss, float* d_grads, float* d_exp_avg, float* d_exp_avg_sq,
                                         float* d_state, float eps, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_labels && d_ws && d_logits && d_loss && d_grads, "null argument");
    REQUIRE_ALIGNED16(al16(d_ws) && al16(d_params) && al16(d_x1) && al16(d_x2));
    const int n_opt = (d_exp_avg != nullptr) + (d_exp_avg_sq != nullptr) + (d_state != nullptr);
    REQUIRE(n_opt == 0 || n_opt == 3, "optimizer state: give d_exp_avg, d_exp_avg_sq and d_state, or none of them (loss step)");
    const std::string excess = small_step_excess(g);
    REQUIRE(excess.empty(), excess + " (mllp_gnn_small_step_limits)");
    // the kernel lays the workspace out as the generic path does but saves less: nothing the library remembers about
    // this graph's workspace or folded weights holds afterwards
    mllp_graph* gm = const_cast<mllp_graph*>(g);
    forget_forward(gm);
    gm->folded_ws = gm->folded_params = nullptr;
    return launch_small_step(g, d_params, d_x1, d_x2, d_labels, inv_batch, model_ws(g, (float*)d_ws), d_logits, d_loss,
                             d_grads, d_exp_avg, d_exp_avg_sq, d_state, eps, (hipStream_t)stream);
}

extern "C" int mllp_adam_step(float* d_params, const float* d_grads, float* d_exp_avg, float* d_exp_avg_sq,
                              float* d_state, float eps, float grad_scale, int64_t n, void* stream) {
    REQUIRE(d_params && d_grads && d_exp_avg && d_exp_avg_sq && d_state, "null argument");
    REQUIRE(n > 0 && n < (int64_t)1 << 30, "bad parameter count");
    return launch_adam(d_params, d_grads, d_exp_avg, d_exp_avg_sq, d_state, eps, grad_scale, n, (hipStream_t)stream);
}

extern "C" int mllp_metrics_scratch_bytes(const mllp_graph_t* g, int64_t* bytes) {
    REQUIRE(g && bytes, "null argument");
    *bytes = 16;
    return MLLP_OK;
}

extern "C" int mllp_topm_metrics(const mllp_graph_t* g, const float* d_logits, const float* d_labels, void* d_scratch,
                                 float* d_out, void* stream) {
    REQUIRE(g && d_logits && d_labels && d_out, "null argument");
    return launch_topm_metrics(g, d_logits, d_labels, d_scratch, d_out, (hipStream_t)stream);
}

extern "C" int mllp_topm_select(const mllp_graph_t* g, const float* d_logits, uint8_t* d_mask, int32_t* d_index,
                                float* d_stats, void* stream) {
    REQUIRE(g && d_logits, "null argument");
    REQUIRE(d_mask || d_index || d_stats, "null outputs: at least one of mask, index, stats");
    return launch_topm_select(g->inst_ptr_n, g->inst_ptr_m, g->n_inst, 0, 0, d_logits, d_mask, d_index, d_stats,
                              (hipStream_t)stream);
}

extern "C" int mllp_topm_select_dense(int64_t n, int64_t m, const float* d_logits, uint8_t* d_mask, int32_t* d_index,
                                      float* d_stats, void* stream) {
    REQUIRE(n >= 0 && m >= 0, "bad size: n and m must not be negative");
    REQUIRE(d_logits, "null argument");
    REQUIRE(d_mask || d_index || d_stats, "null outputs: at least one of mask, index, stats");
    if (n > INT32_MAX || m > INT32_MAX) return fail(MLLP_ERANGE, "mllp_topm_select_dense: sizes exceed int32 indexing");
    return launch_topm_select(nullptr, nullptr, 1, (int)n, (int)m, d_logits, d_mask, d_index, d_stats,
                              (hipStream_t)stream);
}
