// normalize.hip -- the reference's normalization of a resident batch (mllp_graph_normalize): every constraint row scaled
// to unit 2-norm, or to right-hand side +rhs_cap where unit norm would leave |b_i| above the cap (SIGNED: s_i = cap / b_i,
// a negative b_i flips the row), the objective of every instance scaled to unit 2-norm.  The rule is oracle/mps_norm.py's
// `normalize`; the consumer of such tensors is the reference's loader (linear_program_data.py:58-80).  All in fp32.
//
//   norm_rows_kernel   s_i (and x2_i <- b_i s_i): one workgroup per NORM_ROWS consecutive rows of CSR(A), three tiers by the
//                      row's nonzero count alone (norm_tier):
//                        group  len <= 64     the 16 lanes of the row's DPP row
//                        wave   len <= 1024   one wavefront (the workgroup's four take the block's long rows in turn)
//                        block  longer        the whole workgroup, the four wavefronts' sums added as (0 + 1) + (2 + 3)
//   norm_obj_kernel    t_k (and x1_j <- c_j t_k): one workgroup per instance, the block tier's order
//   values             a_ij <- s_i a_ij by mllp_graph_scale_values (set_values.hip): every copy refreshed as by
//                      mllp_graph_set_values, byte for byte what a fresh build from the scaled values would hold
//
// SUMMATION ORDER.  In a tier of G lanes, lane l adds a_l^2, a_(l+G)^2, ... in that order with one fma each, starting from
// 0; the lanes are then added by the xor butterfly of device_utils.h::group_sum (1, 2, half-mirror, mirror, 16, 32), whose
// pair sums are symmetric, so every lane holds the same bits.  Which tier, how many terms a lane adds and the tree depend
// on the row's LENGTH only -- not on the row's position in its workgroup, its neighbours, the batch or the graph's own
// tiers -- so an instance normalizes to the same bits alone and inside any batch.  No atomics; one writer per word.
#include <cmath>

#include "device_utils.h"
#include "internal.h"

namespace mllp {

namespace {

constexpr int NORM_ROWS = BLOCK / 16;       // rows per workgroup: one 16-lane group each
constexpr int NORM_GROUP_MAX = 64;          // longest row of the group tier (4 terms per lane)
constexpr int NORM_WAVE_MAX = 1024;         // ... of the wave tier (16 terms per lane)

__host__ __device__ constexpr int norm_tier(int64_t len) { return len <= NORM_GROUP_MAX ? 0 : len <= NORM_WAVE_MAX ? 1 : 2; }

// lane `l` of G: a[l]^2 + a[l + G]^2 + ... in that order
template <int G>
__device__ __forceinline__ float strided_squares(const float* __restrict__ a, int len, int l) {
    float q = 0.0f;
    for (int j = l; j < len; j += G) {
        const float v = a[j];
        q = __fmaf_rn(v, v, q);
    }
    return q;
}

// the whole workgroup over a[0, len): every thread returns the sum (two barriers; `part` is reusable afterwards)
__device__ __forceinline__ float block_squares(const float* __restrict__ a, int len, float* part) {
    const float q = group_sum<64>(strided_squares<BLOCK>(a, len, threadIdx.x));
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = q;
    __syncthreads();
    const float total = __fadd_rn(__fadd_rn(part[0], part[1]), __fadd_rn(part[2], part[3]));
    __syncthreads();
    return total;
}

__device__ __forceinline__ float inv_norm(float q) { return q > 0.0f ? __fdiv_rn(1.0f, __fsqrt_rn(q)) : 1.0f; }

// one row's scale from its sum of squares (one lane); cap <= 0: no cap
__device__ __forceinline__ void finish_row(int r, float q, float cap, float* __restrict__ x2, int write, float* __restrict__ scale) {
    const float b = x2[r];
    float s = inv_norm(q);
    if (cap > 0.0f && fabsf(__fmul_rn(b, s)) > cap) s = __fdiv_rn(cap, b);
    scale[r] = s;
    if (write) x2[r] = __fmul_rn(b, s);
}

__global__ __launch_bounds__(BLOCK) void norm_rows_kernel(const int* __restrict__ ptr, const float* __restrict__ val, int n_rows,
                                                          float* __restrict__ x2, float cap, int write,
                                                          float* __restrict__ scale) {
    __shared__ int s_ptr[NORM_ROWS + 1];
    __shared__ float part[BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * NORM_ROWS;
    const int n_here = min(NORM_ROWS, n_rows - row0);
    if (tid <= NORM_ROWS) s_ptr[tid] = ptr[row0 + min(tid, n_here)];       // (rows past the end: empty)
    __syncthreads();
    {   // group tier: row `tid / 16` (a row of another tier runs the same code over no terms)
        const int k = tid >> 4, beg = s_ptr[k], len = s_ptr[k + 1] - beg;
        const bool mine = k < n_here && norm_tier(len) == 0;
        const float q = group_sum<16>(strided_squares<16>(val + beg, mine ? len : 0, tid & 15));
        if (mine && (tid & 15) == 0) finish_row(row0 + k, q, cap, x2, write, scale);
    }
    for (int k = wave; k < n_here; k += BLOCK / 64) {       // wave tier (k is uniform in the wavefront)
        const int beg = s_ptr[k], len = s_ptr[k + 1] - beg;
        if (norm_tier(len) != 1) continue;
        const float q = group_sum<64>(strided_squares<64>(val + beg, len, lane));
        if (lane == 0) finish_row(row0 + k, q, cap, x2, write, scale);
    }
    for (int k = 0; k < n_here; ++k) {                      // block tier (k is uniform in the workgroup)
        const int beg = s_ptr[k], len = s_ptr[k + 1] - beg;
        if (norm_tier(len) != 2) continue;
        const float q = block_squares(val + beg, len, part);
        if (tid == 0) finish_row(row0 + k, q, cap, x2, write, scale);
    }
}

__global__ __launch_bounds__(BLOCK) void norm_obj_kernel(const int* __restrict__ inst_ptr_n, float* __restrict__ x1, int write,
                                                         float* __restrict__ scale) {
    __shared__ float part[BLOCK / 64];
    const int k = blockIdx.x, beg = inst_ptr_n[k], n = inst_ptr_n[k + 1] - beg;
    const float t = inv_norm(block_squares(x1 + beg, n, part));
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
    *tier = norm_tier(row_nnz);
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
    if (!g->norm_scale) {       // once per graph (allocates): the scales of calls that pass no output array
        void* p = nullptr;
        MLLP_HIP_TRY(hipMalloc(&p, (size_t)std::max<int64_t>(g->M + g->n_inst, 1) * sizeof(float)));
        g->allocs.push_back(p);
        g->norm_scale = static_cast<float*>(p);
    }
    float* rs = d_row_scale ? d_row_scale : g->norm_scale;
    float* os = d_obj_scale ? d_obj_scale : g->norm_scale + g->M;
    const float cap = std::isfinite(rhs_cap) && rhs_cap > 0.0f ? rhs_cap : 0.0f;
    const int write = compute_only ? 0 : 1;
    if (g->M > 0) {
        hipLaunchKernelGGL(norm_rows_kernel, dim3((unsigned)((g->M + NORM_ROWS - 1) / NORM_ROWS)), dim3(BLOCK), 0, s, g->A.ptr,
                           g->A.val, (int)g->M, d_x2, cap, write, rs);
        if (int rc = check_launch("normalize rows")) return rc;
    }
    hipLaunchKernelGGL(norm_obj_kernel, dim3((unsigned)g->n_inst), dim3(BLOCK), 0, s, g->inst_ptr_n, d_x1, write, os);
    if (int rc = check_launch("normalize objective")) return rc;
    if (compute_only) return MLLP_OK;
    if (int rc = mllp_graph_scale_values(g, rs, nullptr, stream)) return rc;
    return mllp_graph_invalidate_inputs(g);     // x1 / x2 were just written
}
