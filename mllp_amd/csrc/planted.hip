// planted.hip -- labelled LPs made where the batch lives (mllp_graph_plant_basis), and the two sparse sweeps that certify a
// claimed optimal solution of the resident batch (mllp_lp_certificate).  The LP is that of the normalized tensors:
// min c'x, Ax = b, x >= 0; x1 = c, x2 = b, labels = 1 on the basis.  All in fp32.
//
//   plant_validate_kernel  one thread per row: the pivot's column is inside the batch, the entry (i, pivot[i]) exists
//                          (binary search in the ascending row -> ppos[i], its CSR position), and no column is claimed by two
//                          rows (integer atomicCAS on owner[j]; only the error word depends on who wins).  Library scratch only.
//   plant rows             off_i = sum |a_ij|, rest_i = sum a_ij xstar_j over the basic j != pivot[i]; the pivot entry becomes
//                          copysign(dominance off_i + floor, old value), b_i = fma(pivot value, xstar[pivot[i]], rest_i).  The
//                          new value array (every other value copied bit for bit) goes to the graph's scratch of nnz floats
//   values                 mllp_graph_set_values from that scratch: every copy refreshed
//   plant cols             c_j = sum_i a_ij ystar_i (+ slack_j off the basis) over column j of the refreshed CSR(A^T);
//                          labels_j = basic_j
//   certificate            row sweep |sum_j a_ij x_j - b_i| -> scratch[0, M), column sweep c_j - sum_i a_ij y_i ->
//                          scratch[M, M + N), then one workgroup per instance takes the six figures
//
// The summation order of every sweep is ordered_sum.h's (a term that the rule leaves out is skipped in place), so an
// instance gets the same bits alone and inside any batch.  No float atomics; one writer per word.
#include <climits>
#include <cmath>

#include "ordered_sum.h"

namespace mllp {

namespace {

constexpr int PL_ERR_ABSENT = 1, PL_ERR_TWICE = 2, PL_ERR_RANGE = 4;

// ---- planting -----------------------------------------------------------------------------------------------------------
// err[0]: PL_ERR_* bits, err[1]: the lowest offending row
__global__ __launch_bounds__(BLOCK) void plant_validate_kernel(const int* __restrict__ ptr, const int* __restrict__ idx, int n_rows,
                                                               int n_cols, const int* __restrict__ pivot, int* __restrict__ owner,
                                                               int* __restrict__ ppos, int* __restrict__ err) {
    const int i = blockIdx.x * BLOCK + threadIdx.x;
    if (i >= n_rows) return;
    const int p = pivot[i];
    int bad = 0;
    if (p < 0 || p >= n_cols) bad = PL_ERR_RANGE;
    else {
        int lo = ptr[i], hi = ptr[i + 1];                   // first position with idx >= p in the ascending row
        const int end = hi;
        while (lo < hi) {
            const int mid = lo + ((hi - lo) >> 1);
            if (idx[mid] < p) lo = mid + 1;
            else hi = mid;
        }
        if (lo < end && idx[lo] == p) ppos[i] = lo;
        else bad = PL_ERR_ABSENT;
        if (atomicCAS(&owner[p], -1, i) != -1) bad |= PL_ERR_TWICE;
    }
    if (bad) {
        atomicOr(&err[0], bad);
        atomicMin(&err[1], i);
    }
}

struct PlantRows {
    using Acc = Sum2;           // {off_i, rest_i}
    struct Row {
        int p, pos;
    };
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const int* __restrict__ pivot;
    const int* __restrict__ ppos;
    const int* __restrict__ owner;
    const float* __restrict__ xstar;
    float dominance, floor;
    float* __restrict__ out;        // [nnz] the new values
    float* __restrict__ x2;
    __device__ __forceinline__ Row row(int r) const { return {pivot[r], ppos[r]}; }
    __device__ __forceinline__ void term(const Row& rc, int e, Sum2& v) const {
        const int j = idx[e];
        const float a = val[e];
        if (e != rc.pos) out[e] = a;
        if (j != rc.p && owner[j] >= 0) {
            v.a = __fadd_rn(v.a, fabsf(a));
            v.b = __fmaf_rn(a, xstar[j], v.b);
        }
    }
    __device__ __forceinline__ void finish(int r, const Row& rc, const Sum2& v) const {
        const float d = copysignf(__fadd_rn(__fmul_rn(dominance, v.a), floor), val[rc.pos]);
        out[rc.pos] = d;
        x2[r] = __fmaf_rn(d, xstar[rc.p], v.b);
    }
};

struct PlantCols {
    using Acc = float;
    struct Row {};
    const int* __restrict__ idx;    // CSR(A^T): the constraint of every nonzero
    const float* __restrict__ val;
    const int* __restrict__ owner;
    const float* __restrict__ ystar;
    const float* __restrict__ slack;
    float* __restrict__ x1;
    float* __restrict__ labels;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& v) const { v = __fmaf_rn(val[e], ystar[idx[e]], v); }
    __device__ __forceinline__ void finish(int j, const Row&, float v) const {
        const bool basic = owner[j] >= 0;
        x1[j] = basic ? v : __fadd_rn(v, slack[j]);
        labels[j] = basic ? 1.0f : 0.0f;
    }
};

// ---- certificate --------------------------------------------------------------------------------------------------------
// out[r] = |sum_j a_rj x_j - b_r| (rows = 1: CSR(A)) or c_r - sum_i a_ir y_i (rows = 0: CSR(A^T))
struct CertSweep {
    using Acc = float;
    struct Row {};
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ x;    // the source vector
    const float* __restrict__ rhs;  // b (rows) or c (columns)
    int rows;
    float* __restrict__ out;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& v) const { v = __fmaf_rn(val[e], x[idx[e]], v); }
    __device__ __forceinline__ void finish(int r, const Row&, float v) const {
        out[r] = rows ? fabsf(__fsub_rn(v, rhs[r])) : __fsub_rn(rhs[r], v);
    }
};

constexpr int CERT_FIELDS = 6, CERT_EXTREMA = 5;    // five maxima / minima, then the basis count

// one workgroup per instance.  The max / min are exact whatever the order; the sum of the mask takes the block tier's order
__global__ __launch_bounds__(BLOCK) void cert_reduce_kernel(const int* __restrict__ inst_ptr_m, const int* __restrict__ inst_ptr_n,
                                                            const float* __restrict__ row_res, const float* __restrict__ red,
                                                            const float* __restrict__ x, const float* __restrict__ basis,
                                                            float* __restrict__ cert) {
    __shared__ float part[BLOCK / 64][CERT_EXTREMA];
    __shared__ float count_part[BLOCK / 64];
    const int k = blockIdx.x, tid = threadIdx.x;
    const float inf = __builtin_huge_valf();
    float f[CERT_EXTREMA] = {0.0f, inf, 0.0f, inf, 0.0f}, count = 0.0f;
    for (int i = inst_ptr_m[k] + tid, end = inst_ptr_m[k + 1]; i < end; i += BLOCK) f[0] = fmaxf(f[0], row_res[i]);
    for (int j = inst_ptr_n[k] + tid, end = inst_ptr_n[k + 1]; j < end; j += BLOCK) {
        const float m = basis[j], xj = x[j], rc = red[j];
        if (m != 0.0f) {
            f[1] = fminf(f[1], xj);
            f[4] = fmaxf(f[4], fabsf(rc));
        } else {
            f[2] = fmaxf(f[2], fabsf(xj));
            f[3] = fminf(f[3], rc);
        }
        count = __fadd_rn(count, m);
    }
    f[0] = group_max<64>(f[0]);
    f[1] = group_min<64>(f[1]);
    f[2] = group_max<64>(f[2]);
    f[3] = group_min<64>(f[3]);
    f[4] = group_max<64>(f[4]);
    if ((tid & 63) == 0)
        for (int c = 0; c < CERT_EXTREMA; ++c) part[tid >> 6][c] = f[c];
    count = block_tree_sum<BLOCK / 64>(count, count_part);      // (its barriers publish `part` as well)
    if (tid < CERT_EXTREMA) {
        const float a = part[0][tid], b = part[1][tid], c = part[2][tid], d = part[3][tid];
        const bool is_min = tid == 1 || tid == 3;
        cert[(int64_t)k * CERT_FIELDS + tid] = is_min ? fminf(fminf(a, b), fminf(c, d)) : fmaxf(fmaxf(a, b), fmaxf(c, d));
    } else if (tid == CERT_EXTREMA) {
        cert[(int64_t)k * CERT_FIELDS + tid] = count;
    }
}

}  // namespace

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_graph_plant_basis(mllp_graph_t* g, const int* d_pivot, const float* d_xstar, const float* d_ystar,
                                      const float* d_slack, float dominance, float floor, float* d_x1, float* d_x2,
                                      float* d_labels, void* stream) {
    REQUIRE(g && d_pivot && d_xstar && d_ystar && d_slack && d_x1 && d_x2 && d_labels, "null argument");
    REQUIRE(std::isfinite(dominance) && dominance > 1.0f, "dominance must be finite and above 1");
    REQUIRE(std::isfinite(floor) && floor > 0.0f, "floor must be finite and above 0");
    REQUIRE(!borrowed_tiled(g), MLLP_BORROWED_TILED_MSG);
    hipStream_t s = (hipStream_t)stream;
    const int M = (int)g->M, N = (int)g->N;
    int rc;
    // owner [N], ppos [M], the error words [2]
    if ((rc = graph_alloc_once(g, g->plant_ws, (size_t)(g->N + g->M + 2) * sizeof(int)))) return rc;
    if ((rc = ensure_scale_buf(g))) return rc;
    int* owner = g->plant_ws;
    int* ppos = owner + N;
    int* err = ppos + M;
    // ---- validation: library scratch only; the caller's buffers and the graph's values are untouched on refusal
    if (N > 0) MLLP_HIP_TRY(hipMemsetAsync(owner, 0xFF, (size_t)N * sizeof(int), s));       // -1: unclaimed
    MLLP_HIP_TRY(hipMemsetAsync(err, 0, sizeof(int), s));
    MLLP_HIP_TRY(hipMemsetAsync(err + 1, 0x7F, sizeof(int), s));
    if (M > 0) {
        hipLaunchKernelGGL(plant_validate_kernel, dim3((unsigned)((M + BLOCK - 1) / BLOCK)), dim3(BLOCK), 0, s, g->A.ptr, g->A.idx,
                           M, N, d_pivot, owner, ppos, err);
        if ((rc = check_launch("plant_basis validate"))) return rc;
    }
    int h_err[2] = {0, 0};
    MLLP_HIP_TRY(hipMemcpyAsync(h_err, err, sizeof(h_err), hipMemcpyDeviceToHost, s));
    MLLP_HIP_TRY(hipStreamSynchronize(s));
    if (h_err[0]) {
        std::string why;
        if (h_err[0] & PL_ERR_RANGE) why += " a pivot is outside the batch's columns;";
        if (h_err[0] & PL_ERR_ABSENT) why += " a pivot entry (i, pivot[i]) is absent from its row's pattern;";
        if (h_err[0] & PL_ERR_TWICE) why += " a column is the pivot of two rows (pivot must be injective);";
        return fail(MLLP_EINVAL, std::string(__func__) + ":" + why + " first offending row " + std::to_string(h_err[1]) +
                                     "; nothing was written");
    }
    // ---- rows: the new values into the scratch, b into d_x2
    const PlantRows rows = {g->A.idx, g->A.val, d_pivot, ppos, owner, d_xstar, dominance, floor, g->scale_buf, d_x2};
    if ((rc = launch_tier_sweep(g->A.ptr, M, rows, s, "plant_basis rows"))) return rc;
    if ((rc = mllp_graph_set_values(g, g->nnz ? g->scale_buf : g->A.val, stream))) return rc;
    // ---- columns over the refreshed CSR(A^T): c into d_x1, the mask into d_labels
    const PlantCols cols = {g->At.idx, g->At.val, owner, d_ystar, d_slack, d_x1, d_labels};
    if ((rc = launch_tier_sweep(g->At.ptr, N, cols, s, "plant_basis columns"))) return rc;
    return mllp_graph_invalidate_inputs(g);     // x1 / x2 / labels were just written
}

extern "C" int mllp_lp_certificate_scratch_bytes(const mllp_graph_t* g, int64_t* bytes) {
    REQUIRE(g && bytes, "null argument");
    *bytes = std::max<int64_t>(g->M + g->N, 1) * (int64_t)sizeof(float);
    return MLLP_OK;
}

extern "C" int mllp_lp_certificate(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x, const float* d_y,
                                   const float* d_basis, float* d_cert, void* d_scratch, void* stream) {
    REQUIRE(g && d_x1 && d_x2 && d_x && d_y && d_basis && d_cert && d_scratch, "null argument");
    hipStream_t s = (hipStream_t)stream;
    const int M = (int)g->M, N = (int)g->N;
    float* row_res = static_cast<float*>(d_scratch);
    float* red = row_res + M;
    int rc;
    if ((rc = launch_tier_sweep(g->A.ptr, M, CertSweep{g->A.idx, g->A.val, d_x, d_x2, 1, row_res}, s, "lp_certificate rows"))) return rc;
    if ((rc = launch_tier_sweep(g->At.ptr, N, CertSweep{g->At.idx, g->At.val, d_y, d_x1, 0, red}, s, "lp_certificate columns")))
        return rc;
    if (g->n_inst > 0) {
        hipLaunchKernelGGL(cert_reduce_kernel, dim3((unsigned)g->n_inst), dim3(BLOCK), 0, s, g->inst_ptr_m, g->inst_ptr_n, row_res, red,
                           d_x, d_basis, d_cert);
        if ((rc = check_launch("lp_certificate reduce"))) return rc;
    }
    return MLLP_OK;
}
