// input_grads.hip -- gradients of the whole model with respect to its inputs (mllp_gnn_backward_inputs): dL/dx1,
// dL/dx2 and dL/da_ij, as a post-pass after the generic backward.  Everything here reads what that backward leaves in
// each conv's workspace (the records `rec`, the folded weights, dq' / ds / dt, the ReLU-masked output gradient) and
// walks the plain CSR of either orientation, so the result does not depend on which re-blocked copies are attached.
//
//   edge_grad     one conv's term of dL/da_ij = dl_ij t_i + alpha_ij ge_i, one nonzero per quad (16 channels) or per
//                 lane (layer 1).  With the forward's final softmax statistics in the record every nonzero is
//                 independent: the mapping is edge-parallel, so a 6 184-nonzero row costs what 6 184 short rows cost,
//                 and no partial states are merged.  The row of a nonzero is found by binary search in ptr.
//   csc_to_csr    CSR position in A of every nonzero of A^T (exact int32, built once per graph): the w2s convs walk
//                 A^T, and their terms land in A's order through it, without atomics.
//   layer1_dst    dx_dst of the two layer-1 convs from dq', ds, dt of their destination-major sweeps:
//                 dx_i = <Ws, g_i> + Pq dq'_i + ds_i Pb + dt_i Pt.
// (dx_src of the layer-1 convs is the source-major sweep BwdSrc1Op of sweep_kernels.hip.)
#include "device_utils.h"
#include "internal.h"

namespace mllp {

struct EdgeArgs {
    const int* __restrict__ ptr;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ X;     // [n_src, cin] source features of the conv
    const float* __restrict__ rec;   // [n_dst, REC_W] (cin = 16) or [n_dst, 8] (cin = 1)
    const int* __restrict__ pos;     // nullptr: the orientation is A itself
    float* __restrict__ dval;        // [nnz] in the CSR order of A
    int n_dst, nnz, accumulate;
};

// 16 channels: lane `part` of a quad owns channels 4 part .. 4 part + 3 of the gathered 64-byte source row (Fwd16Op)
__global__ __launch_bounds__(BLOCK) void edge_grad16_kernel(EdgeArgs a) {
    const int part = threadIdx.x & 3;
    const int64_t e64 = (int64_t)blockIdx.x * (BLOCK / 4) + (threadIdx.x >> 2);
    const bool ok = e64 < a.nnz;
    const int e = ok ? (int)e64 : a.nnz - 1;        // the quad reductions need every lane: idle quads redo the last
    const int row = row_of(a.ptr, a.n_dst, e);
    const int col = a.idx[e];
    const float av = a.val[e];
    const float* r = a.rec + (size_t)row * REC_W;
    const float4 qp = ld4(r + 4 * part), gv = ld4(r + 16 + 4 * part);
    const float4 s0 = ld4(r + 32);                  // {t, rowmax, rinv, ge}
    const float cc = r[36];
    const float4 x = ld4(a.X + (size_t)col * 16 + 4 * part);
    const float l = fmaf(av, s0.x, quad_sum(dot4(qp, x)));
    const float alpha = exp_acc(l - s0.y) * s0.z;
    const float dl = alpha * (quad_sum(dot4(gv, x)) + fmaf(av, s0.w, cc));
    const float v = fmaf(dl, s0.x, alpha * s0.w);
    if (ok && part == 0) {
        const int p = a.pos ? a.pos[e] : e;
        a.dval[p] = a.accumulate ? a.dval[p] + v : v;
    }
}

// 1 channel (layer 1): one lane per nonzero, records {q', gv, t, rowmax, rinv, ge, c, 0}
__global__ __launch_bounds__(BLOCK) void edge_grad1_kernel(EdgeArgs a) {
    const int64_t e64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e64 >= a.nnz) return;
    const int e = (int)e64;
    const int row = row_of(a.ptr, a.n_dst, e);
    const float x = a.X[a.idx[e]];
    const float av = a.val[e];
    const float4 s0 = ld4(a.rec + (size_t)row * 8);
    const float4 s1 = ld4(a.rec + (size_t)row * 8 + 4);
    const float l = fmaf(s0.x, x, av * s0.z);
    const float alpha = exp_acc(l - s0.w) * s1.x;
    const float dl = alpha * fmaf(s0.y, x, fmaf(av, s1.y, s1.z));
    const float v = fmaf(dl, s0.z, alpha * s1.y);
    const int p = a.pos ? a.pos[e] : e;
    a.dval[p] = a.accumulate ? a.dval[p] + v : v;
}

int launch_edge_grad(const Orient& o, int64_t nnz, int cin, const ConvWs& w, const float* x_src, const int* pos,
                     float* dval, int accumulate, hipStream_t s) {
    if (nnz == 0) return MLLP_OK;
    EdgeArgs a{o.ptr, o.idx, o.val, x_src, w.rec, pos, dval, o.n_dst, (int)nnz, accumulate};
    const int per = cin == 16 ? BLOCK / 4 : BLOCK;
    const int64_t blocks = (nnz + per - 1) / per;
    if (cin == 16)
        hipLaunchKernelGGL(edge_grad16_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, a);
    else
        hipLaunchKernelGGL(edge_grad1_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, a);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MLLP_OK : hip_fail(e, "edge_grad");
}

// ---- CSR position in A of every nonzero of A^T ------------------------------------------------------------------
// nonzero e of A^T sits in row j (a variable) and column i (a constraint); its position in A is the place of j among
// the strictly ascending column ids of A's row i (binary search): exact for any nnz, no float round trip
__global__ __launch_bounds__(BLOCK) void csc_to_csr_kernel(const int* __restrict__ tptr, const int* __restrict__ tidx,
                                                           int n_var, const int* __restrict__ ptr,
                                                           const int* __restrict__ idx, int nnz, int* __restrict__ pos) {
    const int64_t e64 = (int64_t)blockIdx.x * BLOCK + threadIdx.x;
    if (e64 >= nnz) return;
    const int e = (int)e64;
    const int j = row_of(tptr, n_var, e);
    const int i = tidx[e];
    int lo = ptr[i], hi = ptr[i + 1];
    while (lo < hi) {
        const int mid = (lo + hi) >> 1;
        if (idx[mid] < j) lo = mid + 1;
        else hi = mid;
    }
    pos[e] = lo;
}

int build_csc_to_csr(const mllp_graph* g, int* pos, hipStream_t s) {
    if (g->nnz == 0) return MLLP_OK;
    const int64_t blocks = (g->nnz + BLOCK - 1) / BLOCK;
    hipLaunchKernelGGL(csc_to_csr_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, g->At.ptr, g->At.idx, g->At.n_dst,
                       g->A.ptr, g->A.idx, (int)g->nnz, pos);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MLLP_OK : hip_fail(e, "csc_to_csr");
}

// ---- dx_dst of the two layer-1 convs, one thread per destination node --------------------------------------------
struct L1Dst {
    const float* __restrict__ g;      // [n, 16] ReLU-masked output gradient
    const float* __restrict__ dqp;    // [n]
    const float* __restrict__ dsdt;   // [n, 2]
    const float* __restrict__ D;      // folded weights
    float* __restrict__ dx;           // [n] (nullptr: not wanted)
    int n, blocks;
};

__global__ __launch_bounds__(BLOCK) void layer1_dst_kernel(L1Dst v, L1Dst c) {
    const bool first = (int)blockIdx.x < v.blocks;
    const L1Dst& a = first ? v : c;
    const int i = ((first ? (int)blockIdx.x : (int)blockIdx.x - v.blocks) * BLOCK) + (int)threadIdx.x;
    if (!a.dx || i >= a.n) return;
    float gr[16], ws[16];
    load_row16(a.g + (size_t)i * 16, gr);
    load_row16(a.D + OFF_WST, ws);                    // WsT[0][o] = Ws[o][0]
    const float2 sd = reinterpret_cast<const float2*>(a.dsdt)[i];
    float x = dot16(ws, gr, 0.0f);
    x = fmaf(a.D[OFF_PQ], a.dqp[i], x);
    x = fmaf(sd.x, a.D[OFF_PB], x);
    x = fmaf(sd.y, a.D[OFF_PT], x);
    a.dx[i] = x;
}

int launch_layer1_dst_grads(const ConvWs& wv, const float* gv, float* dx1, int64_t n, const ConvWs& wc, const float* gc,
                            float* dx2, int64_t m, hipStream_t s) {
    L1Dst v{gv, wv.dqp, wv.dsdt, wv.derived, dx1, (int)n, dx1 ? (int)((n + BLOCK - 1) / BLOCK) : 0};
    L1Dst c{gc, wc.dqp, wc.dsdt, wc.derived, dx2, (int)m, dx2 ? (int)((m + BLOCK - 1) / BLOCK) : 0};
    const int64_t blocks = (int64_t)v.blocks + c.blocks;
    if (blocks == 0) return MLLP_OK;
    hipLaunchKernelGGL(layer1_dst_kernel, dim3((unsigned)blocks), dim3(BLOCK), 0, s, v, c);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MLLP_OK : hip_fail(e, "layer1_dst");
}

}  // namespace mllp
