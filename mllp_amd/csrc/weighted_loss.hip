// weighted_loss.hip -- the loss head between mllp_gnn_forward and mllp_gnn_backward as a kernel of its own
// (mllp_weighted_loss, mllp_balanced_pos_weight, mllp_gnn_loss_step_weighted): torch's BCEWithLogitsLoss(pos_weight) per
// instance, a weight per instance on top, and the per-instance losses themselves.  Reference: the criterion and its use in
// linear_program_experiment.py:41,139-141, which knows one unweighted loss.  Per instance k with n_k columns,
// pw_k = d_pos_weight[k], w_k = d_inst_weight[k] (each 1 when its array is NULL):
//
//   sp_i = max(-z_i, 0) + log1p(exp(-|z_i|))                        softplus(-z_i)
//   l_i  = (1 - y_i) z_i + (1 + (pw_k - 1) y_i) sp_i
//   L_k  = (1 / n_k) sum_i l_i                                      (0 for n_k = 0; NOT multiplied by w_k)
//   dz_i = (w_k / n_k) ((1 - y_i) - (1 + (pw_k - 1) y_i) sigma(-z_i))
//   loss = sum_k w_k L_k
//
//   weighted_loss_kernel        one workgroup of 1024 threads per instance (the geometry of select.hip: an instance is one
//                               contiguous segment, a Netlib batch has fewer instances than the device has CUs, and sixteen
//                               wavefronts hide the latency of the two loads under the exp / log1p chain)
//   weighted_loss_total_kernel  loss: one workgroup, the products w_k L_k staged 256 at a time and added by one thread
//   balanced_pos_weight_kernel  pw_k = (n_k - P_k) / P_k with P_k = sum_i y_i, 1 where P_k is 0 or n_k
//
// The summation order is ordered_sum.h's with all 1024 threads as the lanes: thread t adds l_t, l_(t + 1024), ... (eight of
// them per round, their loads issued together: the order is that of one per round), then the butterfly and the tree over
// the sixteen wavefronts.  All of it depends on n_k alone, so an instance gives the same L_k and dz bits alone and inside
// any batch, whichever outputs are asked for.  loss starts from 0 and adds w_k L_k (one rounded product, one rounded sum)
// for k = 0, 1, ... in instance order.  No atomics; one writer per word.
//
// sigma(-z) is formed as head_kernel (node_kernels.hip) forms sigma(z): from e = exp(-|z|) <= 1, so nothing overflows;
// it is computed directly, not as 1 - sigma(z), which would lose it entirely above z = 17.
#include "ordered_sum.h"

namespace mllp {

namespace {

constexpr int WL_T = 1024, WL_W = WL_T / 64;
constexpr int WL_U = 8;                 // columns of a thread whose loads are in flight together
constexpr int WL_TOTAL_T = 256;

// L_k of the segment [beg, beg + n) in every thread; dz (when given) written on the way
__device__ __forceinline__ float wl_instance(int beg, int n, float w, float pw, const float* __restrict__ z,
                                             const float* __restrict__ y, float* __restrict__ dz, float* part) {
    const float pwm1 = pw - 1.0f;
    const float nf = (float)n;
    const float wn = n > 0 ? __fdiv_rn(w, nf) : 0.0f;
    float acc = 0.0f;
    // WL_U columns of the thread per round, their loads issued together (the walk of a long instance is a chain of load
    // latencies otherwise); the sum takes them in the same order as one column per round would
    for (int64_t i0 = threadIdx.x; i0 < n; i0 += WL_T * WL_U) {      // (64 bits: i0 + 7 * 1024 may pass 2^31 before n does)
        float zv[WL_U], yv[WL_U];
#pragma unroll
        for (int u = 0; u < WL_U; ++u) {
            const int64_t i = i0 + u * WL_T;
            zv[u] = i < n ? z[beg + i] : 0.0f;
            yv[u] = i < n ? y[beg + i] : 0.0f;
        }
#pragma unroll
        for (int u = 0; u < WL_U; ++u) {
            const int64_t i = i0 + u * WL_T;
            if (i >= n) continue;
            const float zi = zv[u], yi = yv[u];
            const float e = expf(-fabsf(zi));
            const float sneg = zi >= 0.0f ? e / (1.0f + e) : 1.0f / (1.0f + e);      // sigma(-z) = 1 - sigma(z)
            const float c = 1.0f + pwm1 * yi, omy = 1.0f - yi;
            const float sp = fmaxf(-zi, 0.0f) + log1pf(e);
            acc = __fadd_rn(acc, omy * zi + c * sp);
            if (dz) dz[beg + i] = wn * (omy - c * sneg);
        }
    }
    const float s = block_tree_sum<WL_W>(acc, part);
    return n > 0 ? __fdiv_rn(s, nf) : 0.0f;
}

// serial == 0: workgroup k takes instance k.  serial != 0 (loss wanted without a place for the L_k): ONE workgroup takes
// the instances in turn and adds the loss as weighted_loss_total_kernel does.
__global__ __launch_bounds__(WL_T) void weighted_loss_kernel(const int* __restrict__ ptr_n, int n_inst, int serial,
                                                             const float* __restrict__ z, const float* __restrict__ y,
                                                             const float* __restrict__ inst_w, const float* __restrict__ pos_w,
                                                             float* __restrict__ dz, float* __restrict__ inst_loss,
                                                             float* __restrict__ loss) {
    __shared__ float part[WL_W];
    const int k0 = serial ? 0 : (int)blockIdx.x, k1 = serial ? n_inst : k0 + 1;
    float total = 0.0f;
    for (int k = k0; k < k1; ++k) {
        const int beg = ptr_n[k], n = ptr_n[k + 1] - beg;
        const float w = inst_w ? inst_w[k] : 1.0f, pw = pos_w ? pos_w[k] : 1.0f;
        const float L = wl_instance(beg, n, w, pw, z, y, dz, part);
        if (threadIdx.x == 0 && inst_loss) inst_loss[k] = L;
        total = __fadd_rn(total, __fmul_rn(w, L));
    }
    if (serial && threadIdx.x == 0) loss[0] = total;
}

__global__ __launch_bounds__(WL_TOTAL_T) void weighted_loss_total_kernel(const float* __restrict__ inst_loss,
                                                                         const float* __restrict__ inst_w, int n_inst,
                                                                         float* __restrict__ loss) {
    __shared__ float prod[WL_TOTAL_T];
    float total = 0.0f;
    for (int base = 0; base < n_inst; base += WL_TOTAL_T) {
        const int k = base + (int)threadIdx.x;
        if (k < n_inst) prod[threadIdx.x] = __fmul_rn(inst_w ? inst_w[k] : 1.0f, inst_loss[k]);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(WL_TOTAL_T, n_inst - base);
            for (int j = 0; j < m; ++j) total = __fadd_rn(total, prod[j]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = total;
}

__global__ __launch_bounds__(WL_T) void balanced_pos_weight_kernel(const int* __restrict__ ptr_n, const float* __restrict__ y,
                                                                   float* __restrict__ pos_w) {
    __shared__ float part[WL_W];
    const int k = blockIdx.x, beg = ptr_n[k], n = ptr_n[k + 1] - beg;
    float acc = 0.0f;
    for (int i = threadIdx.x; i < n; i += WL_T) acc = __fadd_rn(acc, y[beg + i]);
    const float P = block_tree_sum<WL_W>(acc, part), nf = (float)n;
    if (threadIdx.x == 0) pos_w[k] = (P > 0.0f && P < nf) ? __fdiv_rn(nf - P, P) : 1.0f;
}

}  // namespace

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_weighted_loss(const mllp_graph_t* g, const float* d_logits, const float* d_labels,
                                  const float* d_inst_weight, const float* d_pos_weight, float* d_dlogits,
                                  float* d_inst_loss, float* d_loss, void* stream) {
    REQUIRE(g && d_logits && d_labels, "null argument");
    REQUIRE(d_dlogits || d_inst_loss || d_loss, "null outputs: at least one of dlogits, inst_loss, loss");
    hipStream_t s = (hipStream_t)stream;
    const int n_inst = (int)g->n_inst;
    const bool serial = d_loss && !d_inst_loss;
    if (serial) {
        // the L_k have no place to go: the instances in turn, the loss added on the way.  dlogits of such a call come
        // from the same launch (same code per instance, same bits).
        hipLaunchKernelGGL(weighted_loss_kernel, dim3(1), dim3(WL_T), 0, s, g->inst_ptr_n, n_inst, 1, d_logits, d_labels,
                           d_inst_weight, d_pos_weight, d_dlogits, nullptr, d_loss);
        return check_launch("weighted_loss (serial)");
    }
    if (n_inst > 0) {
        hipLaunchKernelGGL(weighted_loss_kernel, dim3((unsigned)n_inst), dim3(WL_T), 0, s, g->inst_ptr_n, n_inst, 0, d_logits,
                           d_labels, d_inst_weight, d_pos_weight, d_dlogits, d_inst_loss, nullptr);
        if (int rc = check_launch("weighted_loss")) return rc;
    }
    if (!d_loss) return MLLP_OK;
    hipLaunchKernelGGL(weighted_loss_total_kernel, dim3(1), dim3(WL_TOTAL_T), 0, s, d_inst_loss, d_inst_weight, n_inst,
                       d_loss);
    return check_launch("weighted_loss total");
}

extern "C" int mllp_balanced_pos_weight(const mllp_graph_t* g, const float* d_labels, float* d_pos_weight, void* stream) {
    REQUIRE(g && d_labels && d_pos_weight, "null argument");
    if (g->n_inst <= 0) return MLLP_OK;
    hipLaunchKernelGGL(balanced_pos_weight_kernel, dim3((unsigned)g->n_inst), dim3(WL_T), 0, (hipStream_t)stream,
                       g->inst_ptr_n, d_labels, d_pos_weight);
    return check_launch("balanced_pos_weight");
}

// mllp_gnn_forward, the loss head above, mllp_gnn_backward: the public calls themselves, so the workspace record is
// exactly what a caller of the two would leave (mllp_gnn_input_grads may follow)
extern "C" int mllp_gnn_loss_step_weighted(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                                           const float* d_labels, const float* d_inst_weight, const float* d_pos_weight,
                                           void* d_ws, float* d_logits, float* d_loss, float* d_inst_loss, float* d_grads,
                                           float* d_dlogits, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_labels && d_ws && d_logits && d_grads, "null argument");
    REQUIRE(((reinterpret_cast<uintptr_t>(d_ws) | reinterpret_cast<uintptr_t>(d_params) | reinterpret_cast<uintptr_t>(d_x1) |
              reinterpret_cast<uintptr_t>(d_x2)) & 15) == 0,
            "misaligned pointer: d_ws, d_params, d_x1 and d_x2 are accessed in 16-byte pieces");
    REQUIRE(d_dlogits, "null d_dlogits: the step needs [N] floats of scratch between its loss head and its backward");
    int rc;
    if ((rc = mllp_gnn_forward(g, d_params, d_x1, d_x2, d_ws, d_logits, stream))) return rc;
    if ((rc = mllp_weighted_loss(g, d_logits, d_labels, d_inst_weight, d_pos_weight, d_dlogits, d_inst_loss, d_loss, stream)))
        return rc;
    return mllp_gnn_backward(g, d_params, d_x1, d_x2, d_ws, d_dlogits, d_grads, stream);
}
