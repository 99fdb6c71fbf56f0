// set_values.hip -- new matrix values a_ij on an unchanged sparsity pattern (mllp_graph_set_values, _scale_values):
// every array of the graph that holds values is refreshed in place on the device, nothing is re-blocked.
//
//   A.val         one device-to-device copy: the caller's array is in CSR(A) order already
//   At.val        gather through at_pos (input_grads.hip: CSR(A) position of every nonzero of A^T), shared with the
//                 input-gradient post-pass and built by whichever of the two runs first
//   fused path    sent is filled from A.val / At.val by fused_fill_kernel (fused_kernels.hip), which simply runs again;
//                 the value half of sax is then copied from sent, so a cached binding of x1 / x2 stays valid
//   re-blocked    the streamed copies (geometries 0-3), the lane copy (geometry 4) and the library-built LDS-tiled
//   copies        copies store the values in the order their kernels consume them.  Each gets a VALUE MAP: for value
//                 word i of the copy, the CSR(A) position + 1 of the nonzero it holds, 0 for a padding slot.
//
// The maps are not written by a second set of builders.  The copy's own builder runs once more over an orientation
// whose value array holds, as bit patterns, the CSR(A) position + 1 of every nonzero (the builders move value bits
// verbatim and fill padding with 0), and the map is read back out of the value words of that scratch copy, which is
// freed again.  This happens on the first mllp_graph_set_values after a copy was built (allocates, synchronises);
// from then on a call is launches only:
//   sv_refresh<L>   dst[value_word<L>(i)] = val[map[i] - 1] for map[i] != 0: contiguous map read and (nearly)
//                   contiguous store, the gather from `val` is the random side.  One writer per word, no atomics.
// Map sizes (int32): lane copy 4 per (group, lane) = the size of `vals`; streamed copies 2 per (group, lane) = 2/3 of
// `ent`; tiled copies 1 per nonzero.
#include <vector>

#include "device_utils.h"
#include "host_stream.h"
#include "internal.h"
#include "lane_layout.h"
#include "stream_layout.h"

namespace mllp {

namespace {

// layout of the value words inside a copy's array, in 4-byte words
constexpr int VL_PLAIN = 0;     // every word (LaneCopy::vals)
constexpr int VL_TILED = 1;     // {offset, value} pairs (Tiled::ent)
constexpr int VL_STREAM = 2;    // {offsets, value, value} triples (StreamCopy::ent)
template <int L>
__device__ __forceinline__ int64_t value_word(int64_t i) {
    return L == VL_TILED ? 2 * i + 1 : L == VL_STREAM ? (i >> 1) * 3 + 1 + (i & 1) : i;
}

// out[e] = bits of (CSR(A) position of nonzero e) + 1; pos == nullptr: the orientation is A itself
__global__ __launch_bounds__(BLOCK) void sv_positions_kernel(const int* __restrict__ pos, int64_t n, int* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e < n) out[e] = (pos ? pos[e] : (int)e) + 1;
}

template <int L>
__global__ __launch_bounds__(BLOCK) void sv_extract_kernel(const int* __restrict__ words, int64_t n, int* __restrict__ map) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i < n) map[i] = words[value_word<L>(i)];
}

template <int L>
__global__ __launch_bounds__(BLOCK) void sv_refresh_kernel(const int* __restrict__ map, const float* __restrict__ val,
                                                           int64_t n, float* __restrict__ dst) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n) return;
    const int k = map[i];
    if (k) dst[value_word<L>(i)] = val[k - 1];
}

// dst[e] = val[pos[e]] (At.val: pos = at_pos, no padding)
__global__ __launch_bounds__(BLOCK) void sv_gather_kernel(const int* __restrict__ pos, const float* __restrict__ val, int64_t n,
                                                          float* __restrict__ dst) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e < n) dst[e] = val[pos[e]];
}

// the value half of sax = {a, x_src} of both fused orientations from the value bits of sent
__global__ __launch_bounds__(BLOCK) void sv_sax_kernel(const int2* __restrict__ sent_a, float* __restrict__ sax_a,
                                                       const int2* __restrict__ sent_t, float* __restrict__ sax_t, int64_t nnz) {
    const int64_t i = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (i >= 2 * nnz) return;
    const bool t = i >= nnz;
    const int64_t e = t ? i - nnz : i;
    (t ? sax_t : sax_a)[2 * e] = __int_as_float((t ? sent_t : sent_a)[e].y);
}

// out[e] = (r_i a_e) s_j in fp32, i / j the constraint / variable of nonzero e of CSR(A); a null scale is all ones
__global__ __launch_bounds__(BLOCK) void sv_scale_kernel(const int* __restrict__ ptr, const int* __restrict__ idx,
                                                         const float* __restrict__ val, int n_rows, int64_t nnz,
                                                         const float* __restrict__ rs, const float* __restrict__ cs,
                                                         float* __restrict__ out) {
    const int64_t e = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e >= nnz) return;
    const float r = rs ? rs[row_of(ptr, n_rows, (int)e)] : 1.0f;
    const float c = cs ? cs[idx[e]] : 1.0f;
    out[e] = __fmul_rn(__fmul_rn(r, val[e]), c);
}

inline dim3 grid_for(int64_t n) { return dim3((unsigned)((n + BLOCK - 1) / BLOCK)); }

template <int L>
int refresh(const int* map, const float* val, int64_t n, void* dst, hipStream_t s) {
    if (n == 0) return MLLP_OK;
    hipLaunchKernelGGL(sv_refresh_kernel<L>, grid_for(n), dim3(BLOCK), 0, s, map, val, n, static_cast<float*>(dst));
    return check_launch("set_values refresh");
}

// map = the value words of `words`, the value array of a scratch copy built over the position array
template <int L>
int extract(const void* words, int64_t n, int** map, hipStream_t s) {
    int* m = nullptr;
    MLLP_HIP_TRY(hipMalloc((void**)&m, (size_t)std::max<int64_t>(n, 1) * sizeof(int)));
    if (n > 0) hipLaunchKernelGGL(sv_extract_kernel<L>, grid_for(n), dim3(BLOCK), 0, s, static_cast<const int*>(words), n, m);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipStreamSynchronize(s);
    if (e != hipSuccess) {
        (void)hipFree(m);
        return hip_fail(e, "set_values: value map");
    }
    *map = m;
    return MLLP_OK;
}

// value words of the copies (the map sizes)
int64_t stream_words(StreamCopy& sc, int geom) { return stream_copy_arrays(sc, geom)[SC_ENT].bytes / 12 * 2; }
int64_t lane_words(LaneCopy& lc) { return lane_copy_arrays(lc)[LC_VALS].bytes / 4; }

bool maps_missing(const Orient& o) {
    for (const StreamCopy& sc : o.stream)
        if (sc.n_tiles > 0 && !sc.vmap) return true;
    if (o.lane1.n_tiles > 0 && !o.lane1.vmap) return true;
    for (const Tiled& tl : o.tiled)
        if (tl.n_tiles > 0 && !tl.vmap) return true;
    return false;
}

// the value maps that one orientation's attached copies still lack (not a launch path: allocates and synchronises)
int build_maps(mllp_graph* g, bool transpose, hipStream_t s) {
    Orient& o = transpose ? g->At : g->A;
    if (!maps_missing(o)) return MLLP_OK;
    const int64_t nnz = g->nnz;
    DevBuf<int> positions;
    if (positions.alloc((size_t)nnz)) return fail(MLLP_ENOMEM, "set_values: hipMalloc failed");
    hipLaunchKernelGGL(sv_positions_kernel, grid_for(nnz), dim3(BLOCK), 0, s, transpose ? g->at_pos : nullptr, nnz, positions.p);
    int rc;
    if ((rc = check_launch("set_values positions"))) return rc;
    Orient probe = o;                   // the same pattern with the positions where the values are (arrays shared, not owned)
    probe.val = reinterpret_cast<float*>(positions.p);
    const std::vector<int64_t>& seg = transpose ? g->h_inst_ptr_n : g->h_inst_ptr_m;
    for (int geom = 0; geom < STREAM_GEOMS; ++geom) {
        StreamCopy& sc = o.stream[geom];
        if (sc.n_tiles == 0 || sc.vmap) continue;
        StreamCopy t;
        rc = build_stream_device(probe, nnz, host_stream_tiles(seg.data(), (int64_t)seg.size() - 1, o.n_dst, geom), t, s, geom);
        if (!rc && (t.n_tiles != sc.n_tiles || t.n_tb != sc.n_tb || t.n_groups != sc.n_groups))
            rc = fail(MLLP_EINVAL, "set_values: the device builder does not reproduce the attached streamed copy");
        if (!rc) rc = extract<VL_STREAM>(t.ent, stream_words(sc, geom), &sc.vmap, s);
        stream_copy_free(t);
        if (rc) return rc;
    }
    if (o.lane1.n_tiles > 0 && !o.lane1.vmap) {
        LaneCopy& lc = o.lane1;
        LaneCopy t;
        rc = build_lane_copy(probe, nnz, seg, t, s);
        if (!rc && (t.n_tiles != lc.n_tiles || t.n_tb != lc.n_tb || t.n_groups != lc.n_groups))
            rc = fail(MLLP_EINVAL, "set_values: the device builder does not reproduce the attached lane copy");
        if (!rc) {                      // the scratch copy's value array IS the map
            lc.vmap = reinterpret_cast<int*>(t.vals);
            t.vals = nullptr;
        }
        lane_copy_free(t);
        if (rc) return rc;
    }
    for (int v = 0; v < TILED_VARIANTS; ++v) {
        Tiled& tl = o.tiled[v];
        if (tl.n_tiles == 0 || tl.vmap) continue;
        Tiled t;
        rc = build_tiled_device(probe, nnz, v, t, s);
        if (!rc && (t.n_tiles != tl.n_tiles || t.n_tb != tl.n_tb))
            rc = fail(MLLP_EINVAL, "set_values: the device builder does not reproduce the attached tiled copy");
        if (!rc) rc = extract<VL_TILED>(t.ent, nnz, &tl.vmap, s);
        tiled_free(t);
        if (rc) return rc;
    }
    return MLLP_OK;
}

int refresh_copies(Orient& o, int64_t nnz, const float* val, hipStream_t s) {
    int rc;
    for (int geom = 0; geom < STREAM_GEOMS; ++geom) {
        StreamCopy& sc = o.stream[geom];
        if (sc.n_tiles > 0 && (rc = refresh<VL_STREAM>(sc.vmap, val, stream_words(sc, geom), sc.ent, s))) return rc;
    }
    if (o.lane1.n_tiles > 0 && (rc = refresh<VL_PLAIN>(o.lane1.vmap, val, lane_words(o.lane1), o.lane1.vals, s))) return rc;
    for (Tiled& tl : o.tiled)
        if (tl.n_tiles > 0 && (rc = refresh<VL_TILED>(tl.vmap, val, nnz, const_cast<int*>(tl.ent), s))) return rc;
    return MLLP_OK;
}

}  // namespace

// a borrowed LDS-tiled copy holds values in arrays that are the caller's: nothing here may write them
bool borrowed_tiled(const mllp_graph* g) {
    for (const Orient* o : {&g->A, &g->At})
        for (const Tiled& tl : o->tiled)
            if (tl.n_tiles > 0 && !tl.owned) return true;
    return false;
}

int ensure_at_pos(mllp_graph* g, hipStream_t s) {
    if (g->at_pos || g->nnz == 0) return MLLP_OK;
    int* pos = nullptr;         // (the graph takes it once it is filled)
    if (int rc = graph_alloc_once(g, pos, (size_t)g->nnz * sizeof(int))) return rc;
    if (int rc = build_csc_to_csr(g, pos, s)) return rc;
    g->at_pos = pos;
    return MLLP_OK;
}

int ensure_scale_buf(mllp_graph* g) {
    return g->nnz == 0 ? MLLP_OK : graph_alloc_once(g, g->scale_buf, (size_t)g->nnz * sizeof(float));
}

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_graph_set_values_bytes(const mllp_graph_t* g, int64_t* bytes) {
    REQUIRE(g && bytes, "null argument");
    mllp_graph* gm = const_cast<mllp_graph*>(g);      // (the array tables take the copies by reference; nothing is written)
    int64_t words = g->nnz;                           // at_pos
    if (g->scale_buf) words += g->nnz;
    if (g->norm_scale) words += g->M + g->n_inst;     // (normalize.hip: not a map, counted here with the other scratch)
    if (g->plant_ws) words += g->N + g->M + 2;        // (planted.hip: likewise)
    for (Orient* o : {&gm->A, &gm->At}) {
        for (int geom = 0; geom < STREAM_GEOMS; ++geom)
            if (o->stream[geom].n_tiles > 0) words += stream_words(o->stream[geom], geom);
        if (o->lane1.n_tiles > 0) words += lane_words(o->lane1);
        for (const Tiled& tl : o->tiled)
            if (tl.n_tiles > 0 && tl.owned) words += g->nnz;
    }
    *bytes = words * 4;
    return MLLP_OK;
}

extern "C" int mllp_graph_set_values(mllp_graph_t* g, const float* d_val, void* stream) {
    REQUIRE(g && d_val, "null argument");
    REQUIRE(!borrowed_tiled(g), MLLP_BORROWED_TILED_MSG);
    hipStream_t s = (hipStream_t)stream;
    forget_forward(g);          // the workspace holds activations of the old values: backward needs a new forward
    const int64_t nnz = g->nnz;
    if (nnz == 0) return MLLP_OK;
    int rc;
    // first call, or a copy was built since the last one (allocates and synchronises: not inside a capture)
    if ((rc = ensure_at_pos(g, s))) return rc;
    if ((rc = build_maps(g, false, s)) || (rc = build_maps(g, true, s))) return rc;
    if (d_val != g->A.val) MLLP_HIP_TRY(hipMemcpyAsync(g->A.val, d_val, (size_t)nnz * sizeof(float), hipMemcpyDeviceToDevice, s));
    const float* val = g->A.val;
    hipLaunchKernelGGL(sv_gather_kernel, grid_for(nnz), dim3(BLOCK), 0, s, g->at_pos, val, nnz, g->At.val);
    if ((rc = check_launch("set_values A^T"))) return rc;
    if ((rc = refresh_copies(g->A, nnz, val, s)) || (rc = refresh_copies(g->At, nnz, val, s))) return rc;
    if (g->fused_built) {
        if ((rc = fused_refill_values(g, s))) return rc;
        hipLaunchKernelGGL(sv_sax_kernel, grid_for(2 * nnz), dim3(BLOCK), 0, s, reinterpret_cast<const int2*>(g->FA.sent), g->FA.sax,
                           reinterpret_cast<const int2*>(g->FAt.sent), g->FAt.sax, nnz);
        if ((rc = check_launch("set_values sax"))) return rc;
    }
    return MLLP_OK;
}

extern "C" int mllp_graph_scale_values(mllp_graph_t* g, const float* d_row_scale, const float* d_col_scale, void* stream) {
    REQUIRE(g, "null graph");
    REQUIRE(!borrowed_tiled(g), MLLP_BORROWED_TILED_MSG);
    hipStream_t s = (hipStream_t)stream;
    const int64_t nnz = g->nnz;
    if (nnz == 0) return mllp_graph_set_values(g, g->A.val, stream);
    if (int rc = ensure_scale_buf(g)) return rc;       // once per graph (allocates)
    hipLaunchKernelGGL(sv_scale_kernel, grid_for(nnz), dim3(BLOCK), 0, s, g->A.ptr, g->A.idx, g->A.val, (int)g->M, nnz,
                       d_row_scale, d_col_scale, g->scale_buf);
    if (int rc = check_launch("scale_values")) return rc;
    return mllp_graph_set_values(g, g->scale_buf, stream);
}
