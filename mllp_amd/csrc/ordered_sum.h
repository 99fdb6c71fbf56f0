// ordered_sum.h -- the one fixed-order sum behind every result that promises the same bits for an instance alone and inside
// any batch: the row sweeps of normalize.hip and planted.hip, the per-instance sums of weighted_loss.hip.
//
// SUMMATION ORDER.  A row's (column's, instance's) terms are added by G lanes: lane l adds terms l, l + G, ... in that
// order, starting from 0 (a term that the rule leaves out is skipped in place).  The lanes are then added by the xor
// butterfly of device_utils.h::group_sum (1, 2, half-mirror, mirror inside 16 lanes, then 16 and 32 across the wavefront),
// whose pair sums are symmetric, so every lane holds the same bits; the wavefronts of a workgroup by the fixed binary tree
// ((0 + 1) + (2 + 3)) + ... over one LDS word each (block_tree_sum).  A sweep picks G by the row's LENGTH alone (row_tier):
//   group  up to TIER_GROUP_MAX terms   the 16 lanes of the row's DPP row (4 terms per lane at most)
//   wave   up to TIER_WAVE_MAX          one wavefront (the workgroup's four take the block's long rows in turn)
//   block  longer                       the whole workgroup
// Nothing depends on the row's position in its workgroup, its neighbours, the batch or the graph's own tiers.  No float
// atomics; one writer per word.  Every sum is an explicit __fadd_rn / __fmaf_rn: the order is the contract.
#pragma once
#include "device_utils.h"
#include "internal.h"

namespace mllp {

constexpr int SWEEP_ROWS = BLOCK / 16;      // rows per workgroup of a sweep: one 16-lane group each
constexpr int TIER_GROUP_MAX = 64;          // longest row of the group tier
constexpr int TIER_WAVE_MAX = 1024;         // ... of the wave tier (16 terms per lane)

__host__ __device__ constexpr int row_tier(int64_t len) { return len <= TIER_GROUP_MAX ? 0 : len <= TIER_WAVE_MAX ? 1 : 2; }

// an accumulator is a float or two of them that share a row's walk
struct Sum2 {
    float a, b;
};

template <int G>
__device__ __forceinline__ Sum2 group_sum(Sum2 v) {
    return {group_sum<G>(v.a), group_sum<G>(v.b)};
}
__device__ __forceinline__ float ordered_add(float x, float y) { return __fadd_rn(x, y); }
__device__ __forceinline__ Sum2 ordered_add(Sum2 x, Sum2 y) { return {__fadd_rn(x.a, y.a), __fadd_rn(x.b, y.b)}; }

// the sum of v over a workgroup of NW wavefronts, in every thread (two barriers; `part` [NW] is reusable afterwards)
template <int NW, class T>
__device__ __forceinline__ T block_tree_sum(T v, T* part) {
    v = group_sum<64>(v);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
    __syncthreads();
    T t[NW];
#pragma unroll
    for (int w = 0; w < NW; ++w) t[w] = part[w];
#pragma unroll
    for (int s = 1; s < NW; s <<= 1) {
#pragma unroll
        for (int w = 0; w < NW; w += 2 * s) t[w] = ordered_add(t[w], t[w + s]);
    }
    __syncthreads();
    return t[0];
}

// lane `l` of G over the row's terms l, l + G, ... in that order
template <int G, class Op>
__device__ __forceinline__ typename Op::Acc strided_terms(const Op& op, const typename Op::Row& rc, int beg, int len, int l) {
    typename Op::Acc v = {};
    for (int j = l; j < len; j += G) op.term(rc, beg + j, v);
    return v;
}

// One sweep over a CSR orientation in the three tiers.  Op: Acc (float or Sum2), Row row(r) (what a row's terms share),
// term(row, e, acc) adds nonzero e, finish(r, row, acc) is run by ONE lane of the row
template <class Op>
__global__ __launch_bounds__(BLOCK) void tier_sweep_kernel(const int* __restrict__ ptr, int n_rows, Op op) {
    using Acc = typename Op::Acc;
    __shared__ int s_ptr[SWEEP_ROWS + 1];
    __shared__ Acc part[BLOCK / 64];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = blockIdx.x * SWEEP_ROWS;
    const int n_here = min(SWEEP_ROWS, n_rows - row0);
    if (tid <= SWEEP_ROWS) s_ptr[tid] = ptr[row0 + min(tid, n_here)];      // (rows past the end: empty)
    __syncthreads();
    {   // group tier: row `tid / 16`.  Every lane reaches the butterfly: a row of another tier runs it over no terms
        const int k = tid >> 4, beg = s_ptr[k], len = s_ptr[k + 1] - beg;
        const bool mine = k < n_here && row_tier(len) == 0;
        const typename Op::Row rc = op.row(row0 + (mine ? k : 0));
        const Acc q = group_sum<16>(strided_terms<16>(op, rc, beg, mine ? len : 0, tid & 15));
        if (mine && (tid & 15) == 0) op.finish(row0 + k, rc, q);
    }
    for (int k = wave; k < n_here; k += BLOCK / 64) {       // wave tier (k is uniform in the wavefront)
        const int beg = s_ptr[k], len = s_ptr[k + 1] - beg;
        if (row_tier(len) != 1) continue;
        const typename Op::Row rc = op.row(row0 + k);
        const Acc q = group_sum<64>(strided_terms<64>(op, rc, beg, len, lane));
        if (lane == 0) op.finish(row0 + k, rc, q);
    }
    for (int k = 0; k < n_here; ++k) {                      // block tier (k is uniform in the workgroup: the barriers need it)
        const int beg = s_ptr[k], len = s_ptr[k + 1] - beg;
        if (row_tier(len) != 2) continue;
        const typename Op::Row rc = op.row(row0 + k);
        const Acc q = block_tree_sum<BLOCK / 64>(strided_terms<BLOCK>(op, rc, beg, len, tid), part);
        if (tid == 0) op.finish(row0 + k, rc, q);
    }
}

// rows [0, n_rows) of the orientation whose row pointers are `ptr`; no rows, no launch
template <class Op>
inline int launch_tier_sweep(const int* ptr, int64_t n_rows, const Op& op, hipStream_t s, const char* what) {
    if (n_rows <= 0) return MLLP_OK;
    hipLaunchKernelGGL(tier_sweep_kernel<Op>, dim3((unsigned)((n_rows + SWEEP_ROWS - 1) / SWEEP_ROWS)), dim3(BLOCK), 0, s, ptr,
                       (int)n_rows, op);
    return check_launch(what);
}

}  // namespace mllp
