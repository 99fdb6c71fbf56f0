// normalize.hip -- the reference's normalization of a resident batch (mllp_graph_normalize): every constraint row scaled
// to unit 2-norm, or to right-hand side +rhs_cap where unit norm would leave |b_i| above the cap (SIGNED: s_i = cap / b_i,
// a negative b_i flips the row), the objective of every instance scaled to unit 2-norm.  The rule is oracle/mps_norm.py's
// `normalize`; the consumer of such tensors is the reference's loader (linear_program_data.py:58-80).  All in fp32.
//
//   RowScale           s_i (and x2_i <- b_i s_i): an op of ordered_sum.h's three-tier sweep over CSR(A), the row's sum of
//                      squares with one fma per term
//   norm_obj_kernel    t_k (and x1_j <- c_j t_k): one workgroup per instance, the block tier's order
//   values             a_ij <- s_i a_ij by mllp_graph_scale_values (set_values.hip): every copy refreshed as by
//                      mllp_graph_set_values, byte for byte what a fresh build from the scaled values would hold
//
// The summation order is ordered_sum.h's: an instance normalizes to the same bits alone and inside any batch.
#include <cmath>

#include "ordered_sum.h"

namespace mllp {

namespace {

__device__ __forceinline__ float inv_norm(float q) { return q > 0.0f ? __fdiv_rn(1.0f, __fsqrt_rn(q)) : 1.0f; }

// the row scale: q_i = sum_j a_ij^2, then one lane makes s_i of it; cap <= 0: no cap
struct RowScale {
    using Acc = float;
    struct Row {};
    const float* __restrict__ val;
    float* __restrict__ x2;
    float cap;
    int write;
    float* __restrict__ scale;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const {
        const float v = val[e];
        q = __fmaf_rn(v, v, q);
    }
    __device__ __forceinline__ void finish(int r, const Row&, float q) const {
        const float b = x2[r];
        float s = inv_norm(q);
        if (cap > 0.0f && fabsf(__fmul_rn(b, s)) > cap) s = __fdiv_rn(cap, b);
        scale[r] = s;
        if (write) x2[r] = __fmul_rn(b, s);
    }
};

__global__ __launch_bounds__(BLOCK) void norm_obj_kernel(const int* __restrict__ inst_ptr_n, float* __restrict__ x1, int write,
                                                         float* __restrict__ scale) {
    __shared__ float part[BLOCK / 64];
    const int k = blockIdx.x, beg = inst_ptr_n[k], n = inst_ptr_n[k + 1] - beg;
    float q = 0.0f;
    for (int j = threadIdx.x; j < n; j += BLOCK) {
        const float v = x1[beg + j];
        q = __fmaf_rn(v, v, q);
    }
    const float t = inv_norm(block_tree_sum<BLOCK / 64>(q, part));
    if (threadIdx.x == 0) scale[k] = t;
    if (write)
        for (int j = threadIdx.x; j < n; j += BLOCK) x1[beg + j] = __fmul_rn(x1[beg + j], t);
}

}  // namespace

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_normalize_row_tier(int64_t row_nnz, int* tier) {
    REQUIRE(tier, "null argument");
    REQUIRE(row_nnz >= 0, "row_nnz must not be negative");
    *tier = row_tier(row_nnz);
    return MLLP_OK;
}

extern "C" int mllp_graph_normalize(mllp_graph_t* g, float* d_x1, float* d_x2, float rhs_cap, int flags, float* d_row_scale,
                                    float* d_obj_scale, void* stream) {
    REQUIRE(g && d_x1 && d_x2, "null argument");
    REQUIRE((flags & ~1) == 0, "unknown flag bits (bit 0: compute only)");
    const bool compute_only = (flags & 1) != 0;
    REQUIRE(!compute_only || (d_row_scale && d_obj_scale), "compute only (flags bit 0) with a null output: both d_row_scale and d_obj_scale are required");
    REQUIRE(!borrowed_tiled(g), MLLP_BORROWED_TILED_MSG);
    hipStream_t s = (hipStream_t)stream;
    // the scales of calls that pass no output array
    if (int rc = graph_alloc_once(g, g->norm_scale, (size_t)std::max<int64_t>(g->M + g->n_inst, 1) * sizeof(float))) return rc;
    float* rs = d_row_scale ? d_row_scale : g->norm_scale;
    float* os = d_obj_scale ? d_obj_scale : g->norm_scale + g->M;
    const float cap = std::isfinite(rhs_cap) && rhs_cap > 0.0f ? rhs_cap : 0.0f;
    const int write = compute_only ? 0 : 1;
    if (int rc = launch_tier_sweep(g->A.ptr, g->M, RowScale{g->A.val, d_x2, cap, write, rs}, s, "normalize rows")) return rc;
    hipLaunchKernelGGL(norm_obj_kernel, dim3((unsigned)g->n_inst), dim3(BLOCK), 0, s, g->inst_ptr_n, d_x1, write, os);
    if (int rc = check_launch("normalize objective")) return rc;
    if (compute_only) return MLLP_OK;
    if (int rc = mllp_graph_scale_values(g, rs, nullptr, stream)) return rc;
    return mllp_graph_invalidate_inputs(g);     // x1 / x2 were just written
}
