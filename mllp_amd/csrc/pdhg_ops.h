// pdhg_ops.h -- what the two executions of PDHG share: pdhg.hip, which gives an instance one persistent
// workgroup, and pdhg_wide.hip, which cuts an instance into items across the device.  The bar between the two is bit equality
// (DESIGN.md 4.25), so what a sweep does with a term and with a finished row is written ONCE, here: the status codes, the
// helpers on the bit patterns of floats, the workgroup's integer maxima, how the lanes of a row are combined (BySum, ByMax),
// and the operators of the set-up walks (ScaledAbs; ScaledProd, the power round of mllp_lp_pdhg_spectral, which only
// pdhg_wide.hip instantiates) and of a Halpern iteration (HalpernCol, HalpernRow).  An operator says
//   Acc, Row, By    the accumulator, what a row's lanes hold of the row beside it, how the lanes are combined
//   row(r)          that Row;  term(rc, e, q): entry e into the accumulator;  finish(r, rc, q): the row's result, by ONE lane
// and knows nothing of who walks the rows.
//
// NOT here: the walkers.  pdhg.hip's wg_sweep and pdhg_wide.hip's item_sweep run the same three tiers of ordered_sum.h over the
// same operators, but place the block tier differently -- wg_sweep walks one range behind ALL chunks of the instance (its
// workgroup sees every row, so the range is found once per call), item_sweep takes a vote of the workgroup per chunk (an item
// knows only its own rows) -- and a walker that did both would change pdhg_kernel's six instruction streams, which are held
// (AbsSum beside ScaledAbs is what folding near-duplicates costs there).  Each file also keeps the operators
// that only it instantiates: AbsSum, ColStep, RowStep and EvalSweep in pdhg.hip, EvalOne and EvalPair in pdhg_wide.hip.
//
// Everything is in the unnamed namespace of the translation unit that includes it, as the definitions were before they moved.
#pragma once
#include <type_traits>

#include "ordered_sum.h"

namespace mllp {

namespace {

// what a call says of an instance (include/mllp_hip.h).  4, 5 and 9 are the wide calls' alone
constexpr int PD_CODE_OPTIMAL = 0, PD_CODE_INFEASIBLE = 4, PD_CODE_UNBOUNDED = 5, PD_CODE_LIMIT = 6, PD_CODE_NOT_FINITE = 8,
              PD_CODE_STALE = 9;

__device__ __forceinline__ unsigned abs_bits(float v) { return __float_as_uint(v) & 0x7fffffffu; }
// the key of max(v, 0) that keeps a NaN
__device__ __forceinline__ unsigned pos_bits(float v) { return (v > 0.0f || v != v) ? abs_bits(v) : 0u; }
__device__ __forceinline__ float clip0(float t) { return t > 0.0f ? t : 0.0f; }
// max of two non-negative floats (or NaN) by their patterns
__device__ __forceinline__ float nn_max(float a, float b) {
    const unsigned ka = abs_bits(a), kb = abs_bits(b);
    return __uint_as_float(ka > kb ? ka : kb);
}
__device__ __forceinline__ bool finite_bits(float v) { return (__float_as_uint(v) & 0x7f800000u) != 0x7f800000u; }
// the correctly rounded square root (__fsqrt_rn is the hardware's approximation, within 1 ulp: numpy's differs from it)
__device__ __forceinline__ float sqrt_rn(float v) { return __builtin_sqrtf(v); }
__device__ __forceinline__ bool finite_pos(float v) { return finite_bits(v) && v > 0.0f; }

// the maxima of K integers over the workgroup, in every thread (two barriers; `s` [NW * K] is reusable afterwards)
template <int NW, int K>
__device__ __forceinline__ void block_max_u32(unsigned (&v)[K], unsigned* s) {
#pragma unroll
    for (int q = 0; q < K; ++q) {
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) {
            const unsigned u = (unsigned)__shfl_xor((int)v[q], o, 64);
            v[q] = u > v[q] ? u : v[q];
        }
    }
    if ((threadIdx.x & 63) == 0) {
#pragma unroll
        for (int q = 0; q < K; ++q) s[(threadIdx.x >> 6) * K + q] = v[q];
    }
    __syncthreads();
#pragma unroll
    for (int q = 0; q < K; ++q) {
        unsigned best = 0u;
#pragma unroll
        for (int w = 0; w < NW; ++w) best = s[w * K + q] > best ? s[w * K + q] : best;
        v[q] = best;
    }
    __syncthreads();
}

// How a sweep combines the lanes of a row: the ordered sum (every sweep of an iteration and of a check) ...
struct BySum {
    template <int G, class T>
    static __device__ __forceinline__ T group(T v) { return group_sum<G>(v); }
    template <int NW, class T>
    static __device__ __forceinline__ T block(T v, T* part) { return block_tree_sum<NW>(v, part); }
};
// ... or the max of non-negative floats by their patterns: exact in any order, keeps a NaN
struct ByMax {
    template <int G>
    static __device__ __forceinline__ float group(float v) {
        unsigned k = __float_as_uint(v);
#pragma unroll
        for (int o = 1; o < G; o <<= 1) {
            const unsigned u = (unsigned)__shfl_xor((int)k, o, 64);
            k = u > k ? u : k;
        }
        return __uint_as_float(k);
    }
    template <int NW>
    static __device__ __forceinline__ float block(float v, float* part) {
        v = group<64>(v);
        if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = v;
        __syncthreads();
        float best = 0.0f;
#pragma unroll
        for (int w = 0; w < NW; ++w) best = nn_max(best, part[w]);
        __syncthreads();
        return best;
    }
};

struct NoRow {};
struct OwnFactor {
    float d;
};

// a set-up walk of one orientation over s_e = fmul(fmul(|a_e|, dr_i), dc_j): a row's max (MAX) or its fadd chain.  `own`:
// the factors of this orientation's rows, `other`: those the walk gathers; ROWS says which of the two is dr, so that both
// orientations form the product in the same order.  The result goes to out[r] (unless null) and into the largest so far
template <bool ROWS, bool MAX>
struct ScaledAbs {
    using Acc = float;
    using Row = OwnFactor;
    using By = std::conditional_t<MAX, ByMax, BySum>;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    int off;
    const float *own, *other;
    float* out;
    unsigned* best;
    __device__ __forceinline__ Row row(int r) const { return {own[r]}; }
    __device__ __forceinline__ void term(const Row& rc, int e, float& q) const {
        const float o = other[idx[e] - off], a = fabsf(val[e]);
        const float s = ROWS ? __fmul_rn(__fmul_rn(a, rc.d), o) : __fmul_rn(__fmul_rn(a, o), rc.d);
        q = MAX ? nn_max(q, s) : __fadd_rn(q, s);
    }
    __device__ __forceinline__ void finish(int r, const Row&, float q) const {
        if (out) out[r] = q;
        const unsigned k = abs_bits(q);
        *best = k > *best ? k : *best;
    }
};

// a power round's walk of one orientation (mllp_lp_pdhg_spectral): the product of the matrix with a gathered vector `g` that
// already carries the OTHER side's factor (fmul(dc_j, v_j) for rows, fmul(dr_i, u_i) for columns: ONE gather per term), an fma
// chain, times this row's own factor.  ROWS: out_i = fmul(dr_i, u_i) with u_i = fmul(dr_i, sum) -- what the column walk
// gathers; columns: out_j = w_j = fmul(dc_j, sum)
template <bool ROWS>
struct ScaledProd {
    using Acc = float;
    using Row = OwnFactor;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    int off;
    const float *own, *g;
    float* out;
    __device__ __forceinline__ Row row(int r) const { return {own[r]}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const { q = __fmaf_rn(val[e], g[idx[e] - off], q); }
    __device__ __forceinline__ void finish(int r, const Row& rc, float q) const {
        const float p = __fmul_rn(rc.d, q);
        out[r] = ROWS ? __fmul_rn(rc.d, p) : p;
    }
};

// the column sweep of a Halpern iteration: the step's output to xh, its reflection to xb (what the row sweep gathers), and
// the iterate to w1 p + w2 anchor.  One writer per word: x_j, xb_j, xh_j of its own j
struct HalpernCol {
    using Acc = float;
    using Row = NoRow;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ c;       // of the instance's first column
    const float *tc, *xa;              // the column's step factor, the anchor
    int row0;
    float tau, w1, w2;
    bool reflect;
    float *x, *xb, *xh;
    const float* y;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const { q = __fmaf_rn(val[e], y[idx[e] - row0], q); }
    __device__ __forceinline__ void finish(int j, const Row&, float s) const {
        const float g = __fsub_rn(c[j], s), xo = x[j];
        const float xn = clip0(__fsub_rn(xo, __fmul_rn(__fmul_rn(tau, tc[j]), g)));
        const float xf = __fsub_rn(__fadd_rn(xn, xn), xo);
        xh[j] = xn;
        xb[j] = xf;
        x[j] = __fmaf_rn(w1, reflect ? xf : xn, __fmul_rn(w2, xa[j]));
    }
};

// the row sweep of a Halpern iteration: y_i, yh_i of its own i
struct HalpernRow {
    using Acc = float;
    using Row = NoRow;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ b;       // of the instance's first row
    const float *tr, *ya;              // the row's step factor, the anchor
    int col0;
    float sigma, w1, w2;
    bool reflect;
    float *y, *yh;
    const float* xb;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const { q = __fmaf_rn(val[e], xb[idx[e] - col0], q); }
    __device__ __forceinline__ void finish(int i, const Row&, float t) const {
        const float yo = y[i];
        const float yn = __fadd_rn(yo, __fmul_rn(__fmul_rn(sigma, tr[i]), __fsub_rn(b[i], t)));
        yh[i] = yn;
        y[i] = __fmaf_rn(w1, reflect ? __fsub_rn(__fadd_rn(yn, yn), yo) : yn, __fmul_rn(w2, ya[i]));
    }
};

}  // namespace

}  // namespace mllp
