// fused_input_grads.hip -- gradients of the whole model with respect to its inputs after the FUSED latency-regime
// backward (mllp_gnn_input_grads, mllp_gnn_loss_step_inputs): dL/dx1, dL/dx2 and dL/da_ij as a post-pass of four launches.
// The fused path keeps every node tensor of the workspace in RENUMBERED node order (fused_graph_build); its copies of
// the matrix keep each original row's entries in order, so this pass walks the plain CSR of A / A^T in the caller's
// order and reaches the node tensors through inv_v / inv_c.  It reads what fused_forward + fused_backward leave behind:
//   h1v, h1c, h2c; the 40-float records of C3, C2V, C2C; Z, aux and the folded weights of the layer-1 convs; the complete
//   ReLU-masked layer-1 output gradients d1v_b / d1c_b; the renumbered copies of the bound inputs (x1_p / x2_p).
// The arithmetic is that of input_grads.hip / BwdSrc1Op; nothing here is shared with the training step.
//
//   rec1      one node kernel, both layer-1 convs: the record {q', gv, t, rowmax, rinv, ge, c, <Ws, g>} of every
//             destination node (fused_bwd1_kernel keeps these in registers and never stores them).  The first seven are
//             the layout edge_grad1_kernel reads; slot 7, which that layout leaves unused, carries the skip term of dx_dst.
//   layer1    dx1 and dx2 in one launch.  Variable j is a destination of gconv1_w2s and a source of gconv1_s2w, and both
//             terms walk row j of A^T: dx_dst = <Ws, g> + Pq dq' + ds Pb + dt Pt with dq', ds, dt summed over the row, and
//             dx_src = sum_i dl_ij q'_i + alpha_ij gv_i over the records of the row's constraints.  One writer per
//             element stores dx_dst + dx_src.  (Constraints likewise, on the rows of A.)
//             Rows by nonzero count: up to FUSED_T1[1] a 16-lane group, up to FUSED_T1[2] a wavefront, above that the
//             workgroup (four wavefront sums added in wavefront order).  The tier and the lane of every term follow
//             from the row's own length, so the order of every sum depends on that row alone.
//   edge_a    dL/da of gconv1_s2w and gconv2_s2w, one quad per nonzero of A: stores t(1C) + t(2C).
//   edge_at   dL/da of gconv1_w2s, gconv2_w2s, gconv3_w2s, one quad per nonzero of A^T: adds the three, in that order, at
//             the nonzero's position in A (g->at_pos).  The fixed order of the generic pass, in two launches.
#include "device_utils.h"
#include "host_graph.h"
#include "internal.h"

namespace mllp {

namespace {

constexpr int IG_GROUP_MAX = FUSED_T1[1];    // longest row of a 16-lane group
constexpr int IG_WAVE_MAX = FUSED_T1[2];     // longest row of a wavefront
constexpr int IG_ROWS = BLOCK / 16;          // rows per workgroup of the layer-1 walk

// ---- layer-1 records ---------------------------------------------------------------------------------------------
struct Rec1Job {
    const float* __restrict__ x;      // [n] destination feature, renumbered (x1_p / x2_p)
    const float* __restrict__ g;      // [n, 16] complete ReLU-masked gradient of the conv's output (d1v_b / d1c_b)
    const float* __restrict__ Z;      // [n]
    const float* __restrict__ aux;    // [n, 4] {u, rowmax, rinv, S}
    const float* __restrict__ D;      // folded weights
    ConvParams p;
    float* __restrict__ rec;          // [n, 8]
    int n, blocks;
};

__global__ __launch_bounds__(BLOCK) void fused_ig_rec1_kernel(Rec1Job v, Rec1Job c) {
    const bool first = (int)blockIdx.x < v.blocks;
    const Rec1Job& a = first ? v : c;
    const int k = (first ? (int)blockIdx.x : (int)blockIdx.x - v.blocks) * BLOCK + (int)threadIdx.x;
    if (k >= a.n) return;
    float gr[16], w[16];
    load_row16(a.g + (size_t)k * 16, gr);
    load_row16(a.p.Wv, w);                            // cin = 1: Wv[o][0]
    const float gv = dot16(w, gr, 0.0f);
    load_row16(a.p.we, w);
    const float ge = dot16(w, gr, 0.0f);
    load_row16(a.p.bv, w);
    const float gb = dot16(w, gr, 0.0f);
    load_row16(a.p.Ws, w);
    const float gs = dot16(w, gr, 0.0f);
    const float x = a.x[k], Zn = a.Z[k];
    const float4 ax = ld4(a.aux + (size_t)k * 4);
    const float Dn = gv * Zn + gb * ax.w + ge * ax.x;      // as bwd1_row of fused_kernels.hip
    const float cc = gb - Dn;
    const float qp = fmaf(a.D[OFF_PQ], x, a.D[OFF_PQ0]), t = fmaf(a.D[OFF_PT], x, a.D[OFF_PT0]);
    float4* r = reinterpret_cast<float4*>(a.rec + (size_t)k * 8);
    r[0] = make_float4(qp, gv, t, ax.y);
    r[1] = make_float4(ax.z, ge, cc, gs);
}

// ---- dx1 / dx2: destination and source term of the two layer-1 convs in one walk of the node's row ----------------
struct L1Job {
    const int* __restrict__ ptr;        // plain CSR of the orientation whose rows are this job's nodes (caller's order)
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const int* __restrict__ inv_row;    // original -> renumbered id of the rows / of the columns
    const int* __restrict__ inv_col;
    const float* __restrict__ x_row;    // the caller's input of the rows / of the columns (original order)
    const float* __restrict__ x_col;
    const float* __restrict__ rec_dst;  // [n, 8] records of the layer-1 conv whose DESTINATIONS are the rows
    const float* __restrict__ rec_src;  // [n_col, 8] records of the conv whose SOURCES are the rows (its destinations: the columns)
    const float* __restrict__ D;        // folded weights of the former
    float* __restrict__ dx;             // [n] (nullptr: not wanted, blocks = 0)
    int n, blocks;
};

struct L1Row {
    float qp, gv, t, mx, rinv, ge, cc, x;
};
struct L1Sum {
    float dq, ds, dt, sx;
};

// the terms of nonzeros beg + lane, beg + lane + step, ... of one row, added in that order
__device__ __forceinline__ L1Sum l1_walk(const L1Job& J, const L1Row& R, int beg, int end, int lane, int step) {
    L1Sum s = {0.0f, 0.0f, 0.0f, 0.0f};
    for (int e = beg + lane; e < end; e += step) {
        const int col = J.idx[e];
        const float a = J.val[e];
        const float xs = J.x_col[col];
        const float* rs = J.rec_src + (size_t)J.inv_col[col] * 8;
        const float4 s0 = ld4(rs), s1 = ld4(rs + 4);
        // the row as a destination (bwd1_row)
        const float l = fmaf(R.qp, xs, a * R.t);
        const float al = exp_acc(l - R.mx) * R.rinv;
        const float dl = al * fmaf(R.gv, xs, fmaf(a, R.ge, R.cc));
        s.ds += dl;
        s.dt = fmaf(dl, a, s.dt);
        s.dq = fmaf(dl, xs, s.dq);
        // the row as a source of the column's conv (BwdSrc1Op): dl q' + alpha gv
        const float l2 = fmaf(s0.x, R.x, a * s0.z);
        const float al2 = exp_acc(l2 - s0.w) * s1.x;
        const float dl2 = al2 * fmaf(s0.y, R.x, fmaf(a, s1.y, s1.z));
        s.sx += fmaf(dl2, s0.x, al2 * s0.y);
    }
    return s;
}

__device__ __forceinline__ float l1_finish(const L1Job& J, float gs, const L1Sum& s) {
    float x = gs;                                   // <Ws, g>
    x = fmaf(J.D[OFF_PQ], s.dq, x);
    x = fmaf(s.ds, J.D[OFF_PB], x);
    x = fmaf(s.dt, J.D[OFF_PT], x);
    return x + s.sx;                                // dx_dst + dx_src
}

__device__ __forceinline__ L1Row l1_row(const L1Job& J, int row, float* gs) {
    const float* r = J.rec_dst + (size_t)J.inv_row[row] * 8;
    const float4 r0 = ld4(r), r1 = ld4(r + 4);
    *gs = r1.w;
    return L1Row{r0.x, r0.y, r0.z, r0.w, r1.x, r1.y, r1.z, J.x_row[row]};
}

__global__ __launch_bounds__(BLOCK) void fused_ig_layer1_kernel(L1Job v, L1Job c) {
    __shared__ float4 merge[BLOCK / 64];
    const bool first = (int)blockIdx.x < v.blocks;
    const L1Job& J = first ? v : c;
    const int row0 = (first ? (int)blockIdx.x : (int)blockIdx.x - v.blocks) * IG_ROWS;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    {   // rows of the group tier: 16 lanes each
        const int row = row0 + (tid >> 4);
        const bool have = row < J.n;
        const int beg = have ? J.ptr[row] : 0, end = have ? J.ptr[row + 1] : 0;
        const bool mine = have && end - beg <= IG_GROUP_MAX;
        float gs = 0.0f;
        L1Sum s = {0.0f, 0.0f, 0.0f, 0.0f};
        if (mine) {
            const L1Row R = l1_row(J, row, &gs);
            s = l1_walk(J, R, beg, end, tid & 15, 16);
        }
        s.dq = row16_sum(s.dq); s.ds = row16_sum(s.ds); s.dt = row16_sum(s.dt); s.sx = row16_sum(s.sx);
        if (mine && (tid & 15) == 0) J.dx[row] = l1_finish(J, gs, s);
        if (!__syncthreads_or(have && !mine)) return;       // no longer row among the workgroup's 16
    }
    // rows of the wave tier: wavefront w takes those among its own four rows
    for (int q = 0; q < 4; ++q) {
        const int row = row0 + wave * 4 + q;
        if (row >= J.n) break;
        const int beg = J.ptr[row], end = J.ptr[row + 1];
        if (end - beg <= IG_GROUP_MAX || end - beg > IG_WAVE_MAX) continue;       // (wave-uniform)
        float gs;
        const L1Row R = l1_row(J, row, &gs);
        L1Sum s = l1_walk(J, R, beg, end, lane, 64);
        s.dq = group_sum<64>(s.dq); s.ds = group_sum<64>(s.ds); s.dt = group_sum<64>(s.dt); s.sx = group_sum<64>(s.sx);
        if (lane == 0) J.dx[row] = l1_finish(J, gs, s);
    }
    // rows of the block tier: the whole workgroup, the four wavefront sums added in wavefront order
    for (int q = 0; q < IG_ROWS; ++q) {
        const int row = row0 + q;
        if (row >= J.n) break;
        const int beg = J.ptr[row], end = J.ptr[row + 1];
        if (end - beg <= IG_WAVE_MAX) continue;                                    // (uniform over the workgroup)
        float gs;
        const L1Row R = l1_row(J, row, &gs);
        L1Sum s = l1_walk(J, R, beg, end, tid, BLOCK);
        s.dq = group_sum<64>(s.dq); s.ds = group_sum<64>(s.ds); s.dt = group_sum<64>(s.dt); s.sx = group_sum<64>(s.sx);
        if (lane == 0) merge[wave] = make_float4(s.dq, s.ds, s.dt, s.sx);
        __syncthreads();
        if (tid == 0) {
            L1Sum t = {0.0f, 0.0f, 0.0f, 0.0f};
            for (int w = 0; w < BLOCK / 64; ++w) {
                const float4 m = merge[w];
                t.dq += m.x; t.ds += m.y; t.dt += m.z; t.sx += m.w;
            }
            J.dx[row] = l1_finish(J, gs, t);
        }
        __syncthreads();
    }
}

// ---- edge terms --------------------------------------------------------------------------------------------------
// dl t + alpha ge of one nonzero: layer 1 (8-float record, scalar source feature) ...
__device__ __forceinline__ float edge_term1(const float* __restrict__ rec, float x, float av) {
    const float4 s0 = ld4(rec), s1 = ld4(rec + 4);
    const float l = fmaf(s0.x, x, av * s0.z);
    const float alpha = exp_acc(l - s0.w) * s1.x;
    const float dl = alpha * fmaf(s0.y, x, fmaf(av, s1.y, s1.z));
    return fmaf(dl, s0.z, alpha * s1.y);
}
// ... and 16 channels: lane `part` of the quad owns channels 4 part .. 4 part + 3 (edge_grad16_kernel); every lane of
// the quad gets the term
__device__ __forceinline__ float edge_term16(const float* __restrict__ r, const float* __restrict__ xrow, float av, int part) {
    const float4 qp = ld4(r + 4 * part), gv = ld4(r + 16 + 4 * part);
    const float4 s0 = ld4(r + 32);                  // {t, rowmax, rinv, ge}
    const float cc = r[36];
    const float4 x = ld4(xrow + 4 * part);
    const float l = fmaf(av, s0.x, quad_sum(dot4(qp, x)));
    const float alpha = exp_acc(l - s0.y) * s0.z;
    const float dl = alpha * (quad_sum(dot4(gv, x)) + fmaf(av, s0.w, cc));
    return fmaf(dl, s0.x, alpha * s0.w);
}

struct EdgeJob {
    const int* __restrict__ ptr;        // plain CSR of the orientation (caller's order)
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const int* __restrict__ inv_row;
    const int* __restrict__ inv_col;
    const float* __restrict__ x_col;    // the caller's input of the columns: layer 1's source feature
    const float* __restrict__ rec1;     // [n_row, 8] layer-1 conv of this orientation
    const float* __restrict__ rec2;     // [n_row, REC_W] layer-2 conv, sources h_a
    const float* __restrict__ rec3;     // [n_row, REC_W] layer-3 conv, sources h_b (A^T only)
    const float* __restrict__ h_a;      // [n_col, 16] renumbered
    const float* __restrict__ h_b;
    const int* __restrict__ pos;        // A^T only: position in A of every nonzero
    float* __restrict__ dval;           // [nnz] CSR order of A
    int n_row, nnz;
};

// one quad per nonzero; idle quads of the last workgroup redo the last nonzero (the quad reductions need every lane)
__global__ __launch_bounds__(BLOCK) void fused_ig_edge_a_kernel(EdgeJob a) {
    const int part = threadIdx.x & 3;
    const int64_t e64 = (int64_t)blockIdx.x * (BLOCK / 4) + (threadIdx.x >> 2);
    const bool ok = e64 < a.nnz;
    const int e = ok ? (int)e64 : a.nnz - 1;
    const int kr = a.inv_row[row_of(a.ptr, a.n_row, e)];
    const int col = a.idx[e];
    const float av = a.val[e];
    const int kc = a.inv_col[col];
    float v = edge_term1(a.rec1 + (size_t)kr * 8, a.x_col[col], av);                              // gconv1_s2w stores
    v = v + edge_term16(a.rec2 + (size_t)kr * REC_W, a.h_a + (size_t)kc * 16, av, part);         // gconv2_s2w adds
    if (ok && part == 0) a.dval[e] = v;
}

__global__ __launch_bounds__(BLOCK) void fused_ig_edge_at_kernel(EdgeJob a) {
    const int part = threadIdx.x & 3;
    const int64_t e64 = (int64_t)blockIdx.x * (BLOCK / 4) + (threadIdx.x >> 2);
    const bool ok = e64 < a.nnz;
    const int e = ok ? (int)e64 : a.nnz - 1;
    const int kr = a.inv_row[row_of(a.ptr, a.n_row, e)];
    const int col = a.idx[e];
    const float av = a.val[e];
    const int kc = a.inv_col[col];
    const int p = a.pos[e];
    const float t1 = edge_term1(a.rec1 + (size_t)kr * 8, a.x_col[col], av);
    const float t2 = edge_term16(a.rec2 + (size_t)kr * REC_W, a.h_a + (size_t)kc * 16, av, part);
    const float t3 = edge_term16(a.rec3 + (size_t)kr * REC_W, a.h_b + (size_t)kc * 16, av, part);
    if (ok && part == 0) {
        float v = a.dval[p];        // gconv1_s2w + gconv2_s2w (fused_ig_edge_a_kernel)
        v = v + t1;                 // gconv1_w2s
        v = v + t2;                 // gconv2_w2s
        v = v + t3;                 // gconv3_w2s
        a.dval[p] = v;
    }
}

}  // namespace

// After fused_backward on this workspace.  m.x1 / m.x2 are the caller's inputs (original order); the renumbered copies
// g->x1_p / g->x2_p are those fused_bind made of them.  Launches only; g->at_pos must exist when dval is wanted.
int fused_input_grads(const mllp_graph* g, const FusedModel& m, float* dx1, float* dx2, float* dval, hipStream_t s) {
    if (!dx1 && !dx2 && !dval) return MLLP_OK;
    const ModelWs& w = m.w;
    const ConvWs &w1v = w.c[CONV_1V], &w1c = w.c[CONV_1C];
    const int N = (int)g->N, M = (int)g->M;
    auto blocks_for = [](int64_t n, int per) { return (int)((n + per - 1) / per); };
    int rc;
    {
        Rec1Job v{g->x1_p, w.d1v_b, w1v.Z, w1v.aux, w1v.derived, conv_params_at(conv_at(m.P, CONV_1V), 1), w1v.rec, N,
                  blocks_for(N, BLOCK)};
        Rec1Job c{g->x2_p, w.d1c_b, w1c.Z, w1c.aux, w1c.derived, conv_params_at(conv_at(m.P, CONV_1C), 1), w1c.rec, M,
                  blocks_for(M, BLOCK)};
        if (v.blocks + c.blocks > 0) {
            hipLaunchKernelGGL(fused_ig_rec1_kernel, dim3((unsigned)(v.blocks + c.blocks)), dim3(BLOCK), 0, s, v, c);
            if ((rc = check_launch("fused_ig_rec1"))) return rc;
        }
    }
    if (dx1 || dx2) {
        // variables: destinations of gconv1_w2s, sources of gconv1_s2w, rows of A^T; constraints: the mirror image
        L1Job v{g->At.ptr, g->At.idx, g->At.val, g->inv_v, g->inv_c, m.x1, m.x2, w1v.rec, w1c.rec, w1v.derived, dx1, N,
                dx1 ? blocks_for(N, IG_ROWS) : 0};
        L1Job c{g->A.ptr, g->A.idx, g->A.val, g->inv_c, g->inv_v, m.x2, m.x1, w1c.rec, w1v.rec, w1c.derived, dx2, M,
                dx2 ? blocks_for(M, IG_ROWS) : 0};
        if (v.blocks + c.blocks > 0) {
            hipLaunchKernelGGL(fused_ig_layer1_kernel, dim3((unsigned)(v.blocks + c.blocks)), dim3(BLOCK), 0, s, v, c);
            if ((rc = check_launch("fused_ig_layer1"))) return rc;
        }
    }
    if (!dval || g->nnz == 0) return MLLP_OK;
    const unsigned eb = (unsigned)blocks_for(g->nnz, BLOCK / 4);
    EdgeJob a{g->A.ptr, g->A.idx, g->A.val, g->inv_c, g->inv_v, m.x1, w1c.rec, w.c[CONV_2C].rec, nullptr, w.h1v, nullptr,
              nullptr, dval, M, (int)g->nnz};
    hipLaunchKernelGGL(fused_ig_edge_a_kernel, dim3(eb), dim3(BLOCK), 0, s, a);
    if ((rc = check_launch("fused_ig_edge_a"))) return rc;
    EdgeJob t{g->At.ptr, g->At.idx, g->At.val, g->inv_v, g->inv_c, m.x2, w1v.rec, w.c[CONV_2V].rec, w.c[CONV_3V].rec,
              w.h1c, w.h2c, g->at_pos, dval, N, (int)g->nnz};
    hipLaunchKernelGGL(fused_ig_edge_at_kernel, dim3(eb), dim3(BLOCK), 0, s, t);
    return check_launch("fused_ig_edge_at");
}

}  // namespace mllp
