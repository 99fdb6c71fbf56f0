// stream_api.cpp -- C ABI of the streamed copies (stream_layout.h, geometries 0-3; lane_layout.h, geometry 4): build
// (device kernels or the host reference builder), info, export, drop.  The copies are library-owned device memory, freed
// on rebuild / drop / graph destroy.
#include <chrono>
#include <vector>

#include "host_stream.h"
#include "internal.h"
#include "lane_layout.h"
#include "stream_layout.h"

namespace mllp {

static_assert(sizeof(Orient::stream) / sizeof(StreamCopy) == STREAM_GEOMS, "one slot per geometry");

namespace {
struct GeomInfo { int R, CB, NW, K0, RQ, ITEM; };
bool geom_info(int geom, GeomInfo* gi) {
    switch (geom) {
        case STREAM_GEOM_SPMM: *gi = {SpmmGeom::R, SpmmGeom::CB, SpmmGeom::NW, SpmmGeom::K0, SpmmGeom::RQ, SpmmGeom::ITEM}; return true;
        case STREAM_GEOM_ATTN: *gi = {AttnGeom::R, AttnGeom::CB, AttnGeom::NW, AttnGeom::K0, AttnGeom::RQ, AttnGeom::ITEM}; return true;
        case STREAM_GEOM_BSRC: *gi = {BsrcGeom::R, BsrcGeom::CB, BsrcGeom::NW, BsrcGeom::K0, BsrcGeom::RQ, BsrcGeom::ITEM}; return true;
        case STREAM_GEOM_BDST: *gi = {BdstGeom::R, BdstGeom::CB, BdstGeom::NW, BdstGeom::K0, BdstGeom::RQ, BdstGeom::ITEM}; return true;
        default: return false;
    }
}
}  // namespace

std::vector<CopyArray> stream_copy_arrays(StreamCopy& sc, int geom) {
    GeomInfo gi{};
    geom_info(geom, &gi);
    return {{(void**)&sc.tile_blk, ((int64_t)sc.n_tiles + 1) * 4},
            {(void**)&sc.blk_id, (int64_t)sc.n_tb * 4},
            {(void**)&sc.rows, (int64_t)sc.n_tb * gi.NW * 256},
            {(void**)&sc.ent, (sc.n_groups + gi.K0) * 64 * SpmmGeom::ENT * 4},
            {(void**)&sc.tile_row, ((int64_t)sc.n_tiles + 1) * 4},
            {(void**)&sc.hdr, (int64_t)sc.n_tb * gi.NW * 16}};
}

std::vector<CopyArray> lane_copy_arrays(LaneCopy& lc) {
    return {{(void**)&lc.tile_blk, ((int64_t)lc.n_tiles + 1) * 4},
            {(void**)&lc.tile_col, (int64_t)lc.n_tiles * 8},
            {(void**)&lc.rows, (int64_t)lc.n_tiles * L1_R * 4},
            {(void**)&lc.offs, (lc.n_groups + L1_PADG) * 64 * 8},
            {(void**)&lc.tile_row, ((int64_t)lc.n_tiles + 1) * 4},
            {(void**)&lc.whdr, (int64_t)lc.n_tb * L1_NW * 8},
            {(void**)&lc.vals, (lc.n_groups + L1_PADG) * 64 * 16}};
}

int copy_alloc(const CopyArray& a) {
    MLLP_HIP_TRY(hipMalloc(a.p, (size_t)std::max<int64_t>(a.bytes, 4)));
    return MLLP_OK;
}

void copy_free(const std::vector<CopyArray>& arrays) {
    for (const CopyArray& a : arrays)
        if (*a.p) (void)hipFree(*a.p);
}

// (the pointer members do not depend on the geometry)
void stream_copy_free(StreamCopy& sc) {
    copy_free(stream_copy_arrays(sc, STREAM_GEOM_SPMM));
    if (sc.vmap) (void)hipFree(sc.vmap);
    sc = StreamCopy();
}

void lane_copy_free(LaneCopy& lc) {
    copy_free(lane_copy_arrays(lc));
    if (lc.vmap) (void)hipFree(lc.vmap);
    lc = LaneCopy();
}

static int64_t copy_bytes(const std::vector<CopyArray>& arrays) {
    int64_t n = 0;
    for (const CopyArray& a : arrays) n += a.bytes;
    return n;
}

struct HostArray { const void* p; size_t bytes; };
template <class T>
static HostArray host_array(const std::vector<T>& v) { return {v.data(), v.size() * sizeof(T)}; }

// The host reference builder (host_stream.cpp) of the copy of geometry `geom` (0-3: into sc, 4: into lc): one download of
// the CSR, then every array of the copy's table uploaded from the host builder's array of the same index.
static int build_on_host(const Orient& o, int64_t nnz, const std::vector<int64_t>& seg, int geom, StreamCopy& sc,
                         LaneCopy& lc, hipStream_t s) {
    std::vector<int> ptr((size_t)o.n_dst + 1, 0), idx((size_t)std::max<int64_t>(nnz, 1));
    std::vector<float> val((size_t)std::max<int64_t>(nnz, 1));
    MLLP_HIP_TRY(hipStreamSynchronize(s));
    if (o.n_dst > 0) MLLP_HIP_TRY(hipMemcpy(ptr.data(), o.ptr, ((size_t)o.n_dst + 1) * 4, hipMemcpyDeviceToHost));
    if (nnz > 0) {
        MLLP_HIP_TRY(hipMemcpy(idx.data(), o.idx, (size_t)nnz * 4, hipMemcpyDeviceToHost));
        MLLP_HIP_TRY(hipMemcpy(val.data(), o.val, (size_t)nnz * 4, hipMemcpyDeviceToHost));
    }
    const int64_t n_seg = (int64_t)seg.size() - 1;
    std::string err;
    std::vector<CopyArray> arrays;
    std::vector<HostArray> host;
    HostStream hs;
    HostLane hl;
    if (geom == STREAM_GEOM_LANE1) {
        if (int rc = host_build_lane(ptr.data(), idx.data(), val.data(), o.n_dst, seg.data(), n_seg, &hl, &err)) return fail(rc, err);
        lc.n_tiles = hl.n_tiles; lc.n_tb = hl.n_tb; lc.n_groups = hl.n_groups; lc.nnz = nnz;
        arrays = lane_copy_arrays(lc);
        host = {host_array(hl.tile_blk), host_array(hl.tile_col), host_array(hl.rows), host_array(hl.offs),
                host_array(hl.tile_row), host_array(hl.whdr), host_array(hl.vals)};
    } else {
        if (int rc = host_build_stream(ptr.data(), idx.data(), val.data(), o.n_dst, o.n_src, seg.data(), n_seg, &hs, &err, 0, geom))
            return fail(rc, err);
        sc.n_tiles = hs.n_tiles; sc.n_tb = hs.n_tb; sc.n_groups = hs.n_groups; sc.step_slots = hs.step_slots;
        arrays = stream_copy_arrays(sc, geom);
        host = {host_array(hs.tile_blk), host_array(hs.blk_id), host_array(hs.rows), host_array(hs.ent),
                host_array(hs.tile_row), host_array(hs.hdr)};
    }
    for (size_t i = 0; i < arrays.size(); ++i) {
        if ((int64_t)host[i].bytes != arrays[i].bytes)
            return fail(MLLP_EINVAL, "host builder: array " + std::to_string(i) + " does not have the size of the copy's table");
        if (int rc = copy_alloc(arrays[i])) return rc;
        if (host[i].bytes) MLLP_HIP_TRY(hipMemcpy(*arrays[i].p, host[i].p, host[i].bytes, hipMemcpyHostToDevice));
    }
    return MLLP_OK;
}

}  // namespace mllp

using namespace mllp;

static bool valid_geom(int geom) {
    GeomInfo gi;
    return geom == STREAM_GEOM_LANE1 || geom_info(geom, &gi);
}

extern "C" int mllp_graph_build_stream_copy(mllp_graph_t* g, int transpose, int geom, int where, void* stream) {
    REQUIRE(g, "null graph");
    REQUIRE(where == 0 || where == 1, "where must be 0 (device builder) or 1 (host reference builder)");
    REQUIRE(valid_geom(geom), "geom must be 0 (plain SpMM), 1 (attention forward), 2 (source-major backward), 3 (destination-major backward) or 4 (lane-per-row copy of the layer-1 sweeps)");
    const bool lane = geom == STREAM_GEOM_LANE1;
    Orient& o = transpose ? g->At : g->A;
    if (lane) lane_copy_free(o.lane1);
    else stream_copy_free(o.stream[geom]);
    if (o.n_dst == 0) return MLLP_OK;
    const auto t0 = std::chrono::steady_clock::now();
    const hipStream_t s = (hipStream_t)stream;
    const std::vector<int64_t>& seg = transpose ? g->h_inst_ptr_n : g->h_inst_ptr_m;     // tiles stay inside an instance
    StreamCopy sc;
    LaneCopy lc;
    const int rc = where == 1 ? build_on_host(o, g->nnz, seg, geom, sc, lc, s)
                   : lane     ? build_lane_copy(o, g->nnz, seg, lc, s)
                              : build_stream_device(o, g->nnz, host_stream_tiles(seg.data(), (int64_t)seg.size() - 1, o.n_dst, geom),
                                                    sc, s, geom);
    if (rc) {
        stream_copy_free(sc);
        lane_copy_free(lc);
        return rc;
    }
    const double seconds = std::chrono::duration<double>(std::chrono::steady_clock::now() - t0).count();
    if (lane) {
        lc.build_seconds = seconds;
        o.lane1 = lc;
    } else {
        sc.build_seconds = seconds;
        o.stream[geom] = sc;
    }
    return MLLP_OK;
}

extern "C" int mllp_graph_drop_stream_copy(mllp_graph_t* g, int transpose, int geom) {
    REQUIRE(g, "null graph");
    REQUIRE(valid_geom(geom), "unknown geometry");
    Orient& o = transpose ? g->At : g->A;
    if (geom == STREAM_GEOM_LANE1) lane_copy_free(o.lane1);
    else stream_copy_free(o.stream[geom]);
    return MLLP_OK;
}

extern "C" int mllp_graph_stream_copy_info(const mllp_graph_t* g, int transpose, int geom, int64_t info[8]) {
    REQUIRE(g && info, "null argument");
    REQUIRE(valid_geom(geom), "unknown geometry");
    Orient& o = const_cast<Orient&>(transpose ? g->At : g->A);
    if (geom == STREAM_GEOM_LANE1) {
        LaneCopy& lc = o.lane1;
        info[0] = lc.n_tiles;
        info[1] = lc.n_tb;
        info[2] = lc.n_groups;
        info[3] = lc.n_groups * 64 * L1_GS;                     // entry slots of the stream, padding included
        info[4] = lc.n_tiles ? copy_bytes(lane_copy_arrays(lc)) : 0;
        info[5] = (int64_t)(lc.build_seconds * 1e6);
        info[6] = L1_R | (int64_t)1 << 16 | (int64_t)4 << 24;   // rows per tile, one row per lane, 4-byte items
        info[7] = (int64_t)L1_CB | (int64_t)L1_NW << 16 | (int64_t)L1_PADG << 24;
        return MLLP_OK;
    }
    GeomInfo gi;
    geom_info(geom, &gi);
    StreamCopy& sc = o.stream[geom];
    info[0] = sc.n_tiles;
    info[1] = sc.n_tb;
    info[2] = sc.n_groups;
    info[3] = sc.step_slots;
    info[4] = sc.n_tiles ? copy_bytes(stream_copy_arrays(sc, geom)) : 0;     // bytes of the copy
    info[5] = (int64_t)(sc.build_seconds * 1e6);                // microseconds the build took (host clock, synchronised)
    info[6] = gi.R | (int64_t)gi.RQ << 16 | (int64_t)gi.ITEM << 24;
    info[7] = gi.CB | gi.NW << 16 | (int64_t)gi.K0 << 24;
    return MLLP_OK;
}

extern "C" int mllp_graph_export_stream_copy(const mllp_graph_t* g, int transpose, int geom, int which, void* host_dst,
                                             int64_t capacity_bytes) {
    REQUIRE(g && host_dst, "null argument");
    REQUIRE(valid_geom(geom), "unknown geometry");
    Orient& o = const_cast<Orient&>(transpose ? g->At : g->A);
    std::vector<CopyArray> arrays;
    if (geom == STREAM_GEOM_LANE1) {
        REQUIRE(o.lane1.n_tiles > 0, "no lane-per-row copy of this orientation (mllp_graph_build_stream_copy, geometry 4)");
        arrays = lane_copy_arrays(o.lane1);
        REQUIRE(which >= 0 && which < (int)arrays.size(),
                "geometry 4 has arrays 0 (tile_blk), 1 (tile_col), 2 (rows), 3 (offs), 4 (tile_row), 5 (whdr), 6 (vals)");
    } else {
        REQUIRE(o.stream[geom].n_tiles > 0, "no streamed copy of this orientation and geometry (mllp_graph_build_stream_copy)");
        arrays = stream_copy_arrays(o.stream[geom], geom);
        REQUIRE(which >= 0 && which < (int)arrays.size(),
                "which must be 0 (tile_blk), 1 (blk_id), 2 (rows), 3 (ent), 4 (tile_row) or 5 (hdr)");
    }
    const CopyArray& a = arrays[which];
    REQUIRE(capacity_bytes >= a.bytes, "destination too small");
    MLLP_HIP_TRY(hipDeviceSynchronize());
    if (a.bytes > 0) MLLP_HIP_TRY(hipMemcpy(host_dst, *a.p, (size_t)a.bytes, hipMemcpyDeviceToHost));
    return MLLP_OK;
}

// the round-3 entry points: geometry 0
extern "C" int mllp_graph_build_spmm_copy(mllp_graph_t* g, int transpose, int where, void* stream) {
    return mllp_graph_build_stream_copy(g, transpose, STREAM_GEOM_SPMM, where, stream);
}
extern "C" int mllp_graph_drop_spmm_copy(mllp_graph_t* g, int transpose) {
    return mllp_graph_drop_stream_copy(g, transpose, STREAM_GEOM_SPMM);
}
extern "C" int mllp_graph_spmm_copy_info(const mllp_graph_t* g, int transpose, int64_t info[8]) {
    const int rc = mllp_graph_stream_copy_info(g, transpose, STREAM_GEOM_SPMM, info);
    if (rc == MLLP_OK) {      // (the round-3 meaning of the last two words)
        info[6] = S_R;
        info[7] = S_CB | S_NW << 16;
    }
    return rc;
}
extern "C" int mllp_graph_export_spmm_copy(const mllp_graph_t* g, int transpose, int which, void* host_dst,
                                           int64_t capacity_bytes) {
    return mllp_graph_export_stream_copy(g, transpose, STREAM_GEOM_SPMM, which, host_dst, capacity_bytes);
}
