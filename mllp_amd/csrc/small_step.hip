// small_step.hip -- the whole training step of a small batch in ONE launch of ONE workgroup (gfx950):
// weight fold, five convs forward, fc + BCEWithLogits, five convs backward, parameter gradients, optionally Adam.
// The step of the reference's own loop (linear_program_experiment.py:123-144: one LP, one Adam step, next LP) is bound by
// launches, not by work: the median Netlib instance has 4 756 nonzeros.  Here the kernel boundaries of the other paths are
// __syncthreads(); every tensor that one phase writes and a later one reads lives in the caller's workspace (the layout
// of api.cpp::model_ws) and stays in L2.
//
// Geometry: 1024 threads = 64 groups of 16 lanes.  A group owns one destination row at a time, lane c owns channel c
// (layer 1 runs the same code on its scalar inputs padded with zeros: the folded weights of a 1-channel conv are zero
// outside channel 0, param_prep_body writes them so).  Four rows per wavefront; a row longer than SM_LONG entries is left
// to a second round in which all 64 groups take one contiguous chunk each and group 0 merges the 64 partial states from
// LDS in chunk order.  No float atomics; every sum has a fixed order, so a step is bitwise reproducible.
// Arithmetic: oracle/spmm_form.py (conv_fwd, conv_bwd, gnn_forward_backward, adam_step), SURVEY.md appendix A.3 / A.4.
#include "device_utils.h"
#include "internal.h"
#include "node_bodies.h"

namespace mllp {

typedef float f32x4 __attribute__((ext_vector_type(4)));

constexpr int SM_T = SMALL_STEP_THREADS;    // finalize_conv_body needs 1024
constexpr int SM_NG = SM_T / 16;            // 16-lane groups
constexpr int SM_NW = SM_T / 64;            // wavefronts: partial statistics per conv
constexpr int SM_LONG = 128;                // a longer row is spread over the workgroup
constexpr int SM_LIST = (int)(SMALL_STEP_MAX_NNZ / SM_LONG) + 1;
constexpr int SM_PASSES = 13;               // 5 forward, 5 backward destination-major, 3 backward source-major
constexpr int SM_PART = 20;                 // floats of a group's partial row state

struct SmallLds {
    float fold[MODEL_CONVS][DERIVED_W];     // the folded weights of the five convs (internal.h::OFF_*)
    float part[SM_NG][SM_PART];
    int list[SM_LIST];
    int nlong[SM_PASSES + 2];         // (two more: the struct ends on 16 bytes)
};
static_assert(sizeof(SmallLds) + 5 * STAT_FLOATS * sizeof(float) == SMALL_STEP_LDS_BYTES, "SMALL_STEP_LDS_BYTES");
static_assert(SM_NW <= STAT_BLOCKS_MAX, "the partial statistics use the workspace's stats tiles");

struct SmallArgs {
    int N, M;
    const int *a_ptr, *a_idx;       // CSR(A): rows = constraints
    const float* a_val;
    const int *t_ptr, *t_idx;       // CSR(A^T): rows = variables
    const float* t_val;
    const float *inv_n, *x1, *x2, *labels;
    float inv_batch;
    float* params;
    ConvParams p[MODEL_CONVS];
    ModelWs w;
    float *logits, *loss, *grads;
    float *m, *v, *state;           // m == nullptr: loss step, the parameters stay
    float eps;
};

// one conv as the passes see it: the destination-major orientation, the opposite one, tensors
struct SConv {
    const int *ptr, *idx;
    const float* val;
    const int *optr, *oidx;
    const float* oval;
    int n_dst, n_src;
    ConvParams p;
    ConvWs w;
    const float* D;                 // folded weights, in LDS
    const float *x_src, *x_dst;
    float *h, *dh, *dx_dst, *dx_src;
};

__device__ __forceinline__ SConv small_conv(const SmallArgs& A, const SmallLds& lds, int c) {
    SConv s;
    s.D = lds.fold[c];
    const bool v = MODEL_CONV[c].dst_is_var;
    s.ptr = v ? A.t_ptr : A.a_ptr; s.idx = v ? A.t_idx : A.a_idx; s.val = v ? A.t_val : A.a_val;
    s.optr = v ? A.a_ptr : A.t_ptr; s.oidx = v ? A.a_idx : A.t_idx; s.oval = v ? A.a_val : A.t_val;
    s.n_dst = v ? A.N : A.M; s.n_src = v ? A.M : A.N;
    s.p = A.p[c];
    s.w = A.w.c[c];
    const ModelWs& w = A.w;
    // linear_program_methods.py:241-247 and its backward (api.cpp::model_backward_body)
    switch (c) {
    case CONV_1V: s.x_src = A.x2; s.x_dst = A.x1; s.h = w.h1v; s.dh = w.d1v; s.dx_dst = nullptr; s.dx_src = nullptr; break;
    case CONV_1C: s.x_src = A.x1; s.x_dst = A.x2; s.h = w.h1c; s.dh = w.d1c; s.dx_dst = nullptr; s.dx_src = nullptr; break;
    case CONV_2V: s.x_src = w.h1c; s.x_dst = w.h1v; s.h = w.h2v; s.dh = w.d2v; s.dx_dst = w.d1v; s.dx_src = w.d1c; break;
    case CONV_2C: s.x_src = w.h1v; s.x_dst = w.h1c; s.h = w.h2c; s.dh = w.d2c; s.dx_dst = w.d1c; s.dx_src = w.d1v; break;
    default:      s.x_src = w.h2c; s.x_dst = w.h2v; s.h = w.h3v; s.dh = w.d3v; s.dx_dst = w.d2v; s.dx_src = w.d2c; break;
    }
    return s;
}

// channel c of node `node` of a [n, CIN] tensor, a scalar tensor padded with zeros
template <int CIN>
__device__ __forceinline__ float ldn(const float* b, int node, int c) {
    if (CIN == 16) return b[(size_t)node * 16 + c];
    return c == 0 ? b[node] : 0.0f;
}
template <int CIN>
__device__ __forceinline__ void stn(float* b, int node, int c, float v) {
    if (CIN == 16) b[(size_t)node * 16 + c] = v;
    else if (c == 0) b[node] = v;
}
// the value of every lane of the 16-lane row (DPP row_share)
__device__ __forceinline__ void gather16(float v, float (&r)[16]) {
    r[0] = dpp_mov<0x150>(v);  r[1] = dpp_mov<0x151>(v);  r[2] = dpp_mov<0x152>(v);  r[3] = dpp_mov<0x153>(v);
    r[4] = dpp_mov<0x154>(v);  r[5] = dpp_mov<0x155>(v);  r[6] = dpp_mov<0x156>(v);  r[7] = dpp_mov<0x157>(v);
    r[8] = dpp_mov<0x158>(v);  r[9] = dpp_mov<0x159>(v);  r[10] = dpp_mov<0x15A>(v); r[11] = dpp_mov<0x15B>(v);
    r[12] = dpp_mov<0x15C>(v); r[13] = dpp_mov<0x15D>(v); r[14] = dpp_mov<0x15E>(v); r[15] = dpp_mov<0x15F>(v);
}

// rows longer than SM_LONG go on the pass's list (the order of the list does not reach any result: every row is
// computed on its own)
__device__ __forceinline__ bool defer_long(SmallLds& lds, int pass, int row, int len, int c) {
    if (len <= SM_LONG) return false;
    if (c == 0) lds.list[atomicAdd(&lds.nlong[pass], 1)] = row;
    return true;
}
// chunk of group `gid` of a row spread over the workgroup
__device__ __forceinline__ void chunk_of(int beg, int end, int gid, int* cb, int* ce) {
    const int chunk = (end - beg + SM_NG - 1) / SM_NG;
    *cb = min(beg + gid * chunk, end);
    *ce = min(*cb + chunk, end);
}

// ---- forward --------------------------------------------------------------------------------------------------------
struct FState {
    float m, L, u, z;       // running max, sum p, sum p a, sum p x_c
};
// entries [beg, end) of one row, four at a time (their loads leave together), online softmax in entry order
template <int CIN>
__device__ __forceinline__ void fwd_edges(const int* idx, const float* val, const float* X, int beg, int end, int c,
                                          float qp, float t, FState& s) {
    for (int e0 = beg; e0 < end; e0 += 4) {
        int id[4];
        float a[4], x[4], l[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = min(e0 + j, end - 1);
            id[j] = idx[e];
            a[j] = val[e];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = ldn<CIN>(X, id[j], c);
#pragma unroll
        for (int j = 0; j < 4; ++j) l[j] = e0 + j < end ? fmaf(a[j], t, row16_sum(qp * x[j])) : NEG_BIG;
        const float mn = fmaxf(fmaxf(s.m, fmaxf(l[0], l[1])), fmaxf(l[2], l[3]));
        const float sc = exp_acc(s.m - mn);
        s.L *= sc; s.u *= sc; s.z *= sc;
        s.m = mn;
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float p = exp_acc(l[j] - mn);     // exactly 0 for the padding of the last four
            s.L += p;
            s.u = fmaf(p, a[j], s.u);
            s.z = fmaf(p, x[j], s.z);
        }
    }
}

template <int CIN>
__device__ void fwd_pass(const SConv& cv, int pass, SmallLds& lds) {
    const int gid = threadIdx.x >> 4, c = threadIdx.x & 15;
    const float* D = cv.D;
    float pq[16], wv[16], ws[16];
    load_row16(D + OFF_PQ + c * 16, pq);                        // q'_c = <Pq[c][:], x> + pq0[c]
#pragma unroll
    for (int k = 0; k < 16; ++k) { wv[k] = D[OFF_WVT + k * 16 + c]; ws[k] = D[OFF_WST + k * 16 + c]; }
    const float pq0 = D[OFF_PQ0 + c], ptc = D[OFF_PT + c], pt0 = D[OFF_PT0];
    const float bs = cv.p.bs[c], bv = cv.p.bv[c], we = cv.p.we[c];

    float xg[16], qp, t;
    auto setup = [&](int r) {
        const float xd = ldn<CIN>(cv.x_dst, r, c);
        gather16(xd, xg);
        qp = dot16(pq, xg, pq0);
        t = row16_sum(ptc * xd) + pt0;
    };
    // o = relu(Wv Z + S bv + u we + Ws x + bs); what backward reads again: q', t, Z, {u, rowmax, rinv, S}
    auto finish = [&](int r, const FState& s) {
        const float rinv = 1.0f / (s.L + 1e-16f);
        const float S = s.L * rinv, un = s.u * rinv, zn = s.z * rinv;
        stn<CIN>(cv.w.qp, r, c, qp);
        stn<CIN>(cv.w.Z, r, c, zn);
        if (c == 0) {
            cv.w.t[r] = t;
            reinterpret_cast<float4*>(cv.w.aux)[r] = make_float4(un, s.L > 0.0f ? s.m : 0.0f, rinv, S);
        }
        float zg[16];
        gather16(zn, zg);
        float o = fmaf(un, we, fmaf(S, bv, bs));
        o = dot16(wv, zg, o);
        o = dot16(ws, xg, o);
        cv.h[(size_t)r * 16 + c] = fmaxf(o, 0.0f);
    };

    for (int r = gid; r < cv.n_dst; r += SM_NG) {
        const int beg = cv.ptr[r], end = cv.ptr[r + 1];
        if (defer_long(lds, pass, r, end - beg, c)) continue;
        setup(r);
        FState s = {NEG_BIG, 0.0f, 0.0f, 0.0f};
        fwd_edges<CIN>(cv.idx, cv.val, cv.x_src, beg, end, c, qp, t, s);
        finish(r, s);
    }
    __syncthreads();
    const int nl = lds.nlong[pass];
    for (int i = 0; i < nl; ++i) {
        const int r = lds.list[i];
        int cb, ce;
        chunk_of(cv.ptr[r], cv.ptr[r + 1], gid, &cb, &ce);
        setup(r);
        FState s = {NEG_BIG, 0.0f, 0.0f, 0.0f};
        fwd_edges<CIN>(cv.idx, cv.val, cv.x_src, cb, ce, c, qp, t, s);
        lds.part[gid][c] = s.z;
        if (c == 0) { lds.part[gid][16] = s.m; lds.part[gid][17] = s.L; lds.part[gid][18] = s.u; }
        __syncthreads();
        if (gid == 0) {
            FState tot = {NEG_BIG, 0.0f, 0.0f, 0.0f};
#pragma unroll 4
            for (int q = 0; q < SM_NG; ++q) tot.m = fmaxf(tot.m, lds.part[q][16]);
#pragma unroll 4
            for (int q = 0; q < SM_NG; ++q) {
                const float sc = exp_acc(lds.part[q][16] - tot.m);
                tot.L = fmaf(lds.part[q][17], sc, tot.L);
                tot.u = fmaf(lds.part[q][18], sc, tot.u);
                tot.z = fmaf(lds.part[q][c], sc, tot.z);
            }
            finish(r, tot);
        }
        __syncthreads();
    }
}

// ---- fc + BCEWithLogits + dL/dh3 (node_kernels.hip::head_kernel mode 2) -----------------------------------------------
__device__ void head_pass(const SmallArgs& A, SmallLds& lds) {
    const int gid = threadIdx.x >> 4, c = threadIdx.x & 15;
    const float w = A.params[OFF_FC + c], b = A.params[OFF_FC + FEAT];
    float accw = 0.0f, accb = 0.0f, accl = 0.0f;
    for (int i = gid; i < A.N; i += SM_NG) {
        const float hc = A.w.h3v[(size_t)i * 16 + c];
        const float z = row16_sum(hc * w) + b;
        const float y = A.labels[i];
        const float wn = A.inv_n[i] * A.inv_batch;
        const float e = expf(-fabsf(z));
        const float sig = z >= 0.0f ? 1.0f / (1.0f + e) : e / (1.0f + e);
        const float dz = wn * (sig - y);
        accl += wn * (fmaxf(z, 0.0f) - z * y + log1pf(e));
        accb += dz;
        accw = fmaf(dz, hc, accw);
        if (c == 0) A.logits[i] = z;
        A.w.d3v[(size_t)i * 16 + c] = dz * w;
    }
    lds.part[gid][c] = accw;
    if (c == 0) { lds.part[gid][16] = accb; lds.part[gid][17] = accl; }
    __syncthreads();
    if (threadIdx.x < 18) {
        float v = 0.0f;
#pragma unroll 4
        for (int q = 0; q < SM_NG; ++q) v += lds.part[q][threadIdx.x];
        if (threadIdx.x < 17) A.grads[OFF_FC + threadIdx.x] = v;
        else A.loss[0] = v;
    }
    __syncthreads();
}

// ---- backward, destination-major: ReLU mask, the row's record, dq', ds, dt, dL/dx_dst ----------------------------------
struct BState {
    float dq, ds, dt;
};
template <int CIN>
__device__ __forceinline__ void bwd_edges(const int* idx, const float* val, const float* X, int beg, int end, int c,
                                          float qp, float t, float m, float rinv, float gv, float ge, float cc, BState& s) {
    for (int e0 = beg; e0 < end; e0 += 4) {
        int id[4];
        float a[4], x[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = min(e0 + j, end - 1);
            id[j] = idx[e];
            a[j] = val[e];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) x[j] = ldn<CIN>(X, id[j], c);
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float l = fmaf(a[j], t, row16_sum(qp * x[j]));
            const float alpha = e0 + j < end ? exp_acc(l - m) * rinv : 0.0f;
            const float dl = alpha * (row16_sum(gv * x[j]) + fmaf(a[j], ge, cc));
            s.ds += dl;
            s.dt = fmaf(dl, a[j], s.dt);
            s.dq = fmaf(dl, x[j], s.dq);
        }
    }
}

// ACC: dL/dx_dst is added to what the buffer holds (the second contribution to dL/dh1)
template <int CIN, bool DX, bool ACC>
__device__ void bwd_pass(const SConv& cv, int pass, SmallLds& lds) {
    const int gid = threadIdx.x >> 4, c = threadIdx.x & 15;
    const float* D = cv.D;
    float wvt[16];
    load_row16(D + OFF_WVT + c * 16, wvt);                      // gv_c = sum_o g_o Wv[o][c]
    const float we = cv.p.we[c], bv = cv.p.bv[c];
    const float pb = D[OFF_PB + c], ptc = D[OFF_PT + c];

    float gk, qp, t, m, rinv, gv, ge, cc;
    auto setup = [&](int r, bool write) {
        const float hk = cv.h[(size_t)r * 16 + c];
        gk = hk > 0.0f ? cv.dh[(size_t)r * 16 + c] : 0.0f;
        if (write) cv.dh[(size_t)r * 16 + c] = gk;              // the masked gradient: the statistics read it
        float gr[16];
        gather16(gk, gr);
        gv = dot16(wvt, gr, 0.0f);
        ge = row16_sum(gk * we);
        const float gb = row16_sum(gk * bv);
        const float4 ax = reinterpret_cast<const float4*>(cv.w.aux)[r];     // {u, rowmax, rinv, S}
        const float Dn = row16_sum(gv * ldn<CIN>(cv.w.Z, r, c)) + gb * ax.w + ge * ax.x;
        cc = gb - Dn;
        qp = ldn<CIN>(cv.w.qp, r, c);
        t = cv.w.t[r];
        m = ax.y;
        rinv = ax.z;
    };
    auto finish = [&](int r, const BState& s) {
        stn<CIN>(cv.w.dqp, r, c, s.dq);
        if (c == 0) reinterpret_cast<float2*>(cv.w.dsdt)[r] = make_float2(s.ds, s.dt);
        if (CIN == 16) {        // record of the source-major sweep
            float* rec = cv.w.rec + (size_t)r * REC_W;
            rec[c] = qp;
            rec[16 + c] = gv;
            if (c < 8) {
                float v = 0.0f;
                v = c == 0 ? t : v;
                v = c == 1 ? m : v;
                v = c == 2 ? rinv : v;
                v = c == 3 ? ge : v;
                v = c == 4 ? cc : v;
                rec[32 + c] = v;
            }
        }
        if (DX) {               // dx_d = sum_o g_o Ws[o][d] + sum_k dq'_k Pq[k][d] + ds Pb[d] + dt Pt[d]
            float wst[16], pqt[16], gr[16], dg[16];
            load_row16(D + OFF_WST + c * 16, wst);
            load_row16(D + OFF_PQT + c * 16, pqt);
            gather16(gk, gr);
            gather16(s.dq, dg);
            float dx = dot16(wst, gr, 0.0f);
            dx = dot16(pqt, dg, dx);
            dx = fmaf(s.ds, pb, dx);
            dx = fmaf(s.dt, ptc, dx);
            float* out = cv.dx_dst + (size_t)r * 16 + c;
            *out = ACC ? *out + dx : dx;
        }
    };

    for (int r = gid; r < cv.n_dst; r += SM_NG) {
        const int beg = cv.ptr[r], end = cv.ptr[r + 1];
        if (defer_long(lds, pass, r, end - beg, c)) continue;
        setup(r, true);
        BState s = {0.0f, 0.0f, 0.0f};
        bwd_edges<CIN>(cv.idx, cv.val, cv.x_src, beg, end, c, qp, t, m, rinv, gv, ge, cc, s);
        finish(r, s);
    }
    __syncthreads();
    const int nl = lds.nlong[pass];
    for (int i = 0; i < nl; ++i) {
        const int r = lds.list[i];
        int cb, ce;
        chunk_of(cv.ptr[r], cv.ptr[r + 1], gid, &cb, &ce);
        setup(r, false);        // every group reads dh[r] before the barrier below; group 0 writes the masked row once, behind it
        BState s = {0.0f, 0.0f, 0.0f};
        bwd_edges<CIN>(cv.idx, cv.val, cv.x_src, cb, ce, c, qp, t, m, rinv, gv, ge, cc, s);
        lds.part[gid][c] = s.dq;
        if (c == 0) { lds.part[gid][16] = s.ds; lds.part[gid][17] = s.dt; }
        __syncthreads();
        if (gid == 0) {
            BState tot = {0.0f, 0.0f, 0.0f};
#pragma unroll 4
            for (int q = 0; q < SM_NG; ++q) {
                tot.dq += lds.part[q][c];
                tot.ds += lds.part[q][16];
                tot.dt += lds.part[q][17];
            }
            cv.dh[(size_t)r * 16 + c] = gk;
            finish(r, tot);
        }
        __syncthreads();
    }
}

// ---- backward, source-major (16 channels): dL/dx_src[j] = sum_i alpha_ij gv_i + dl_ij q'_i over the opposite orientation
__device__ __forceinline__ float src_edges(const int* idx, const float* val, const float* rec, int beg, int end, int c,
                                           float xj) {
    float acc = 0.0f;
    for (int e0 = beg; e0 < end; e0 += 4) {
        int id[4];
        float a[4], q[4], gv[4], cc[4];
        float4 sc[4];
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const int e = min(e0 + j, end - 1);
            id[j] = idx[e];
            a[j] = val[e];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float* r = rec + (size_t)id[j] * REC_W;
            q[j] = r[c];
            gv[j] = r[16 + c];
            sc[j] = ld4(r + 32);        // {t, rowmax, rinv, ge}
            cc[j] = r[36];
        }
#pragma unroll
        for (int j = 0; j < 4; ++j) {
            const float l = fmaf(a[j], sc[j].x, row16_sum(q[j] * xj));
            const float alpha = e0 + j < end ? exp_acc(l - sc[j].y) * sc[j].z : 0.0f;
            const float dl = alpha * (row16_sum(gv[j] * xj) + fmaf(a[j], sc[j].w, cc[j]));
            acc = fmaf(alpha, gv[j], acc);
            acc = fmaf(dl, q[j], acc);
        }
    }
    return acc;
}

template <bool ACC>
__device__ void src_pass(const SConv& cv, int pass, SmallLds& lds) {
    const int gid = threadIdx.x >> 4, c = threadIdx.x & 15;
    for (int j = gid; j < cv.n_src; j += SM_NG) {
        const int beg = cv.optr[j], end = cv.optr[j + 1];
        if (defer_long(lds, pass, j, end - beg, c)) continue;
        const float acc = src_edges(cv.oidx, cv.oval, cv.w.rec, beg, end, c, cv.x_src[(size_t)j * 16 + c]);
        float* out = cv.dx_src + (size_t)j * 16 + c;
        *out = ACC ? *out + acc : acc;
    }
    __syncthreads();
    const int nl = lds.nlong[pass];
    for (int i = 0; i < nl; ++i) {
        const int j = lds.list[i];
        int cb, ce;
        chunk_of(cv.optr[j], cv.optr[j + 1], gid, &cb, &ce);
        lds.part[gid][c] = src_edges(cv.oidx, cv.oval, cv.w.rec, cb, ce, c, cv.x_src[(size_t)j * 16 + c]);
        __syncthreads();
        if (gid == 0) {
            float acc = 0.0f;
#pragma unroll 4
            for (int q = 0; q < SM_NG; ++q) acc += lds.part[q][c];
            float* out = cv.dx_src + (size_t)j * 16 + c;
            *out = ACC ? *out + acc : acc;
        }
        __syncthreads();
    }
}

// ---- parameter statistics: the seven 16x16 tiles of node_kernels.hip::param_stats16_kernel, one partial per wavefront ----
//   T0 g x^T   T1 g Z^T   T2 g e^T   T3 dq' x^T   T4 dq' e^T   T5 sc x^T   T6 sc e^T     e = [1, S, u], sc = [ds, dt]
template <int CIN>
__device__ void stats_pass(const SConv& cv) {
    const int lane = threadIdx.x & 63, wave = threadIdx.x >> 6;
    const int r = lane & 15, kq = lane >> 4;
    const int n = cv.n_dst;
    f32x4 acc[STAT_TILES];
#pragma unroll
    for (int i = 0; i < STAT_TILES; ++i) acc[i] = (f32x4){0.0f, 0.0f, 0.0f, 0.0f};
    constexpr int CH = 4;       // chunks of 4 nodes whose loads leave together
    const int npass = (n + 4 * CH - 1) / (4 * CH);
    for (int ps = wave; ps < npass; ps += SM_NW) {
        float ag[CH], adq[CH], asc[CH], bx[CH], bz[CH], be[CH];
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            const int node = (ps * CH + k) * 4 + kq;
            ag[k] = adq[k] = asc[k] = bx[k] = bz[k] = be[k] = 0.0f;
            if (node < n) {
                ag[k] = cv.dh[(size_t)node * 16 + r];
                adq[k] = ldn<CIN>(cv.w.dqp, node, r);
                bx[k] = ldn<CIN>(cv.x_dst, node, r);
                bz[k] = ldn<CIN>(cv.w.Z, node, r);
                const float2 sd = reinterpret_cast<const float2*>(cv.w.dsdt)[node];
                const float4 ax = reinterpret_cast<const float4*>(cv.w.aux)[node];
                asc[k] = r == 0 ? sd.x : (r == 1 ? sd.y : 0.0f);
                be[k] = r == 0 ? 1.0f : (r == 1 ? ax.w : (r == 2 ? ax.x : 0.0f));
            }
        }
#pragma unroll
        for (int k = 0; k < CH; ++k) {
            acc[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag[k], bx[k], acc[0], 0, 0, 0);
            acc[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag[k], bz[k], acc[1], 0, 0, 0);
            acc[2] = __builtin_amdgcn_mfma_f32_16x16x4f32(ag[k], be[k], acc[2], 0, 0, 0);
            acc[3] = __builtin_amdgcn_mfma_f32_16x16x4f32(adq[k], bx[k], acc[3], 0, 0, 0);
            acc[4] = __builtin_amdgcn_mfma_f32_16x16x4f32(adq[k], be[k], acc[4], 0, 0, 0);
            acc[5] = __builtin_amdgcn_mfma_f32_16x16x4f32(asc[k], bx[k], acc[5], 0, 0, 0);
            acc[6] = __builtin_amdgcn_mfma_f32_16x16x4f32(asc[k], be[k], acc[6], 0, 0, 0);
        }
    }
    // finalize_conv_body sums the SM_NW partials in its fixed order
    float* out = cv.w.stats + (size_t)wave * STAT_FLOATS;
#pragma unroll
    for (int i = 0; i < STAT_TILES; ++i)
#pragma unroll
        for (int j = 0; j < 4; ++j) out[i * 256 + (kq * 4 + j) * 16 + r] = acc[i][j];
}

__global__ __launch_bounds__(SM_T) void small_step_kernel(SmallArgs A) {
    __shared__ SmallLds lds;
    if (threadIdx.x < SM_PASSES) lds.nlong[threadIdx.x] = 0;
    for (int k = threadIdx.x; k < LEN_UNUSED; k += SM_T) A.grads[OFF_UNUSED + k] = 0.0f;     // gconv3_s2w is never called
    if (threadIdx.x < BLOCK) {
#pragma unroll
        for (int c = 0; c < MODEL_CONVS; ++c) param_prep_body(A.p[c], MODEL_CONV[c].cin, lds.fold[c]);
    }
    __syncthreads();
    // every pass ends behind a __syncthreads(): what it wrote to the workspace is there for the next one
    fwd_pass<1>(small_conv(A, lds, CONV_1V), 0, lds);
    fwd_pass<1>(small_conv(A, lds, CONV_1C), 1, lds);
    fwd_pass<16>(small_conv(A, lds, CONV_2V), 2, lds);
    fwd_pass<16>(small_conv(A, lds, CONV_2C), 3, lds);
    fwd_pass<16>(small_conv(A, lds, CONV_3V), 4, lds);
    head_pass(A, lds);
    bwd_pass<16, true, false>(small_conv(A, lds, CONV_3V), 5, lds);     // d2v =
    src_pass<false>(small_conv(A, lds, CONV_3V), 10, lds);              // d2c =
    bwd_pass<16, true, false>(small_conv(A, lds, CONV_2V), 6, lds);     // d1v =
    src_pass<false>(small_conv(A, lds, CONV_2V), 11, lds);              // d1c =
    bwd_pass<16, true, true>(small_conv(A, lds, CONV_2C), 7, lds);      // d1c +=
    src_pass<true>(small_conv(A, lds, CONV_2C), 12, lds);               // d1v +=
    bwd_pass<1, false, false>(small_conv(A, lds, CONV_1V), 8, lds);
    bwd_pass<1, false, false>(small_conv(A, lds, CONV_1C), 9, lds);
    stats_pass<1>(small_conv(A, lds, CONV_1V));
    stats_pass<1>(small_conv(A, lds, CONV_1C));
    stats_pass<16>(small_conv(A, lds, CONV_2V));
    stats_pass<16>(small_conv(A, lds, CONV_2C));
    stats_pass<16>(small_conv(A, lds, CONV_3V));
    __syncthreads();
#pragma unroll
    for (int c = 0; c < MODEL_CONVS; ++c)
        finalize_conv_body(MODEL_CONV[c].cin, A.p[c], A.w.c[c].stats, SM_NW, A.grads + CONV_OFF.at[c]);
    __syncthreads();
    if (A.m) adam_body(A.params, A.grads, A.m, A.v, A.state, A.eps, 1.0f, NUM_PARAMS);
}

int launch_small_step(const mllp_graph* g, float* params, const float* x1, const float* x2, const float* labels,
                      float inv_batch, const ModelWs& w, float* logits, float* loss, float* grads, float* m, float* v,
                      float* state, float eps, hipStream_t s) {
    SmallArgs A;
    A.N = (int)g->N; A.M = (int)g->M;
    A.a_ptr = g->A.ptr; A.a_idx = g->A.idx; A.a_val = g->A.val;
    A.t_ptr = g->At.ptr; A.t_idx = g->At.idx; A.t_val = g->At.val;
    A.inv_n = g->inv_n; A.x1 = x1; A.x2 = x2; A.labels = labels;
    A.inv_batch = inv_batch;
    A.params = params;
    for (int c = 0; c < MODEL_CONVS; ++c) A.p[c] = conv_params_at(conv_at(params, c), MODEL_CONV[c].cin);
    A.w = w;
    A.logits = logits; A.loss = loss; A.grads = grads;
    A.m = m; A.v = v; A.state = state; A.eps = eps;
    hipLaunchKernelGGL(small_step_kernel, dim3(1), dim3(SM_T), 0, s, A);
    return check_launch("small_step");
}

}  // namespace mllp
