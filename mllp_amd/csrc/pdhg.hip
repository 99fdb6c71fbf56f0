// pdhg.hip -- restarted PDHG on every instance of the resident batch: mllp_lp_pdhg, its diagonally
// preconditioned form with a clamped primal weight, mllp_lp_pdhg_scaled, and the preconditioned form whose
// iteration is Halpern's anchored step with reflection, mllp_lp_pdhg_halpern.  The rules are stated in
// include/mllp_hip.h.  ONE kernel source, instantiated on the entry point's argument struct (S = Args::scaled,
// H = Args::halpern), and one host path.  A first-order solve of  min c'x, A_k x = b, x >= 0  that needs two sparse matrix-vector products per
// iteration and no factorization: memory O(n + m) per instance, no row limit.
//
// One workgroup per instance, persistent over the iterations (the structure of basis.hip and simplex.hip, for the same
// reason: no cross-workgroup synchronisation, no atomics, the same bits alone and inside any batch).  Per iteration
//   column sweep over CSR(A^T)   s_j = sum_i a_ij y_i;  x+_j = max(0, x_j - eta (c_j - s_j));  xbar_j = 2 x+_j - x_j;  xs_j += x+_j
//   barrier
//   row sweep over CSR(A)        t_i = sum_j a_ij xbar_j;  y+_i = y_i + eta (b_i - t_i);  ys_i += y+_i
//   barrier
// Every row (column) sum takes ordered_sum.h's order, picked by the row's length alone: up to 64 terms the 16 lanes of a
// DPP row, up to 1024 one wavefront, longer the whole workgroup (wg_sweep below is tier_sweep_kernel's body for a
// workgroup that walks ALL rows of its instance instead of 16 of them).  One lane finishes a row: one writer per word.
//
// A check (every check_every iterations) evaluates the average and the current iterate in ONE walk of each orientation
// (Sum2), the four max-norms as integer maxima over the bit patterns of non-negative floats (exact in any order, and a
// NaN -- whose pattern is above +inf's -- is never lost), the four dot products through block_tree_sum.  Every thread then
// holds the same bits of both errors, so stop / restart / which candidate are taken alike by all wavefronts: a decision
// that differed between two of them would leave a barrier unmatched.
//
// What S adds; all of it is compiled out of mllp_lp_pdhg's instantiations:
//   set-up     dr [m], dc [n] by ruiz_passes passes on the maxima and an optional one on the sums of
//              s_ij = fmul(fmul(|a_ij|, dr_i), dc_j) -- ONE expression, walked from both orientations, so CSR(A) and
//              CSR(A^T) see the same bits; then tr = dr^2, tc = dc^2, eta from the sums of the final s_ij, w0 from two norms
//   iteration  x+_j = clip(x_j - (tau tc_j)(c_j - s_j)),  y+_i = y_i + (sigma tr_i)(b_i - t_i):  preconditioned PDHG written in
//              the unscaled variables -- no scaled matrix is stored; one more load and one more multiply per finished row
//   restart    the weight w moves to sqrt(w dy / dx), clamped to [w0 / span, w0 span]; tau = eta / w, sigma = eta w
// The checks evaluate the ORIGINAL LP either way, in the same expressions and order.
//
// What H changes (H implies S); all of it is compiled out of the other four instantiations:
//   iteration  the step's output goes to xh_j (yh_i), which take the words of xs (ys), and the iterate moves to
//              w1 p + w2 anchor, p the reflected point 2 xh - x (or xh), w1 = (k + 1) / (k + 2), w2 = 1 / (k + 2), k the
//              iterations since the last restart; the anchor is S's (xr, yr): one more cached load per finished row
//   check      ONE point, (xh, yh), which is also the output; no average, no choice between two candidates
//   restart    (x, y) <- (xh, yh), S's weight update from the anchor, and the anchor moves whether the weight is on or not.
//              xr, yr are then read by the lane that finishes a row, not by the thread that wrote them: a barrier ends it
//
// WHERE THE VECTORS LIVE.  x, xbar, xs, y, ys (3 n + 2 m words) are gathered through idx in every sweep and live in LDS
// (IN_LDS) when they fit min(max_lds_words, PDHG_LDS_WORDS), in the caller's scratch otherwise -- the same code instantiated
// twice, the same bits either way.  S's tc, xr, tr, yr (2 n + 2 m words) are read once per finished row by the lane that
// finishes it -- the access pattern of c and b -- and ALWAYS live in the caller's scratch: sharing the LDS image would take
// 5 n + 4 m words and move instances out of LDS to save one cached load per row.  During the set-up the same words hold dc,
// C, dr, R.
//
// The four instantiations of mllp_lp_pdhg and mllp_lp_pdhg_scaled are instruction for instruction what the two files they came from compiled to.
// That holds the kernel's text to two habits: a value that S changes is DEFINED once, through a ternary on S or an accessor of
// Args, never set and then overwritten under `if constexpr`; and one deliberate duplicate stays, AbsSum beside ScaledAbs (a
// ScaledAbs with unit factors folded at compile time moves all four streams).
//
// WHAT IS DEFINED WHERE.  pdhg_ops.h, shared with pdhg_wide.hip: the status codes, the bit helpers,
// block_max_u32, BySum and ByMax, and the operators that both executions instantiate -- ScaledAbs, HalpernCol, HalpernRow.
// This file: the walker of a persistent workgroup (wg_sweep), the operators that only this kernel instantiates (AbsSum, ColStep,
// RowStep, EvalSweep), the kernel and its host path.
#include <cmath>
#include <string>

#include "lp_launch.h"
#include "ordered_sum.h"
#include "pdhg_ops.h"

namespace mllp {

namespace {

// One sweep of a workgroup over the n_rows rows of ITS instance in the three tiers of ordered_sum.h.  ptr: the row
// pointers of the instance's first row; [lo2, hi2): a range that holds every row of the block tier (uniform in the
// workgroup: the block tier has barriers).  Op as in tier_sweep_kernel, and Op::By combines the lanes.  No barrier at the end
template <int NT, class Op>
__device__ __forceinline__ void wg_sweep(const int* __restrict__ ptr, int n_rows, int lo2, int hi2, const Op& op,
                                         typename Op::Acc* part) {
    using Acc = typename Op::Acc;
    using By = typename Op::By;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int r0 = 0; r0 < n_rows; r0 += NT / 16) {           // (r0 is uniform in the workgroup)
        const int r = r0 + (tid >> 4);
        const bool in = r < n_rows;
        const int beg = in ? ptr[r] : 0, len = in ? ptr[r + 1] - beg : 0;
        {   // group tier: every lane reaches the butterfly; a row of another tier runs it over no terms
            const bool mine = in && row_tier(len) == 0;
            const typename Op::Row rc = op.row(mine ? r : 0);
            const Acc q = By::template group<16>(strided_terms<16>(op, rc, beg, mine ? len : 0, tid & 15));
            if (mine && (tid & 15) == 0) op.finish(r, rc, q);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {                        // wave tier: the wavefront's four rows in turn
            const int b4 = __shfl(beg, 16 * g, 64), l4 = __shfl(len, 16 * g, 64);
            if (row_tier(l4) != 1) continue;                 // (uniform in the wavefront)
            const int r4 = r0 + (tid >> 6) * 4 + g;
            const typename Op::Row rc = op.row(r4);
            const Acc q = By::template group<64>(strided_terms<64>(op, rc, b4, l4, lane));
            if (lane == 0) op.finish(r4, rc, q);
        }
    }
    for (int r = lo2; r < hi2; ++r) {                        // block tier
        const int beg = ptr[r], len = ptr[r + 1] - beg;
        if (row_tier(len) != 2) continue;
        const typename Op::Row rc = op.row(r);
        const Acc q = By::template block<NT / 64>(strided_terms<NT>(op, rc, beg, len, tid), part);
        if (tid == 0) op.finish(r, rc, q);
    }
}

// sum_e |a_e| of a row; the largest over the rows this lane finished (mllp_lp_pdhg's set-up: the deliberate duplicate of
// ScaledAbs with unit factors, see the head of the file)
struct AbsSum {
    using Acc = float;
    using Row = NoRow;
    using By = BySum;
    const float* __restrict__ val;
    unsigned* best;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const { q = __fadd_rn(q, fabsf(val[e])); }
    __device__ __forceinline__ void finish(int, const Row&, float q) const {
        const unsigned k = abs_bits(q);
        *best = k > *best ? k : *best;
    }
};

// the column sweep of an iteration; S: the step of column j is tau tc_j (tc is null otherwise)
template <bool S>
struct ColStep {
    using Acc = float;
    using Row = NoRow;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ c;       // of the instance's first column
    const float* tc;
    int row0;
    float tau;
    bool sums;
    float *x, *xb, *xs;
    const float* y;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const { q = __fmaf_rn(val[e], y[idx[e] - row0], q); }
    __device__ __forceinline__ void finish(int j, const Row&, float s) const {
        const float g = __fsub_rn(c[j], s), xo = x[j];
        const float xn = clip0(__fsub_rn(xo, __fmul_rn(S ? __fmul_rn(tau, tc[j]) : tau, g)));
        x[j] = xn;
        xb[j] = __fsub_rn(__fadd_rn(xn, xn), xo);
        if (sums) xs[j] = __fadd_rn(xs[j], xn);
    }
};

// the row sweep of an iteration; S: the step of row i is sigma tr_i (tr is null otherwise)
template <bool S>
struct RowStep {
    using Acc = float;
    using Row = NoRow;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ b;       // of the instance's first row
    const float* tr;
    int col0;
    float sigma;
    bool sums;
    float *y, *ys;
    const float* xb;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const { q = __fmaf_rn(val[e], xb[idx[e] - col0], q); }
    __device__ __forceinline__ void finish(int i, const Row&, float t) const {
        const float yn = __fadd_rn(y[i], __fmul_rn(S ? __fmul_rn(sigma, tr[i]) : sigma, __fsub_rn(b[i], t)));
        y[i] = yn;
        if (sums) ys[i] = __fadd_rn(ys[i], yn);
    }
};

// a check's walk of one orientation: the product with the average (a) and with the current iterate (b) of the OTHER
// side's vector, then the residual against `rhs`: |.| for rows (primal), max(., 0) for columns (dual)
template <bool ROWS>
struct EvalSweep {
    using Acc = Sum2;
    using Row = NoRow;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ rhs;
    int off;
    bool with_avg;
    float cntf;
    const float *v, *vs;               // the current vector and the sum of its iterates
    unsigned *best_a, *best_b;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, Sum2& q) const {
        const int i = idx[e] - off;
        const float a = val[e], cur = v[i], avg = with_avg ? __fdiv_rn(vs[i], cntf) : cur;
        q.a = __fmaf_rn(a, avg, q.a);
        q.b = __fmaf_rn(a, cur, q.b);
    }
    __device__ __forceinline__ void finish(int r, const Row&, Sum2 q) const {
        const float t = rhs[r], da = __fsub_rn(q.a, t), db = __fsub_rn(q.b, t);
        const unsigned ka = ROWS ? abs_bits(da) : pos_bits(da), kb = ROWS ? abs_bits(db) : pos_bits(db);
        *best_a = ka > *best_a ? ka : *best_a;
        *best_b = kb > *best_b ? kb : *best_b;
    }
};

// The kernel's arguments, one struct per entry point.  The fields of PdhgArgs are fields of ScaledArgs under the same
// names (pdhg_args fills them by name), and HalpernArgs is ScaledArgs with `reflect` (scaled_options fills both); `scaled` is
// the kernel's S, `halpern` its H, kkt_words a row of d_kkt, and the two accessors are what the shared text reads of ScaledArgs'
// own fields outside `if constexpr (S)`.
struct PdhgArgs {
    static constexpr bool scaled = false;
    static constexpr bool halpern = false;
    static constexpr int kkt_words = 4;
    const int* __restrict__ ptr_m;
    const int* __restrict__ ptr_n;
    const int* __restrict__ a_ptr;      // CSR(A)
    const int* __restrict__ a_idx;
    const float* __restrict__ a_val;
    const int* __restrict__ at_ptr;     // CSR(A^T)
    const int* __restrict__ at_idx;
    const float* __restrict__ at_val;
    const float* __restrict__ c;
    const float* __restrict__ b;
    const float* x0;
    const float* y0;
    long long max_iters, check_every, lim;
    float eps, step, beta;
    float* x;
    float* y;
    int* status;
    float* kkt;
    float* scratch;
    __device__ bool weigh() const { return false; }
    __device__ float weight_span() const { return 1.0f; }
};

struct ScaledArgs {
    static constexpr bool scaled = true;
    static constexpr bool halpern = false;
    static constexpr int kkt_words = 6;
    const int* __restrict__ ptr_m;
    const int* __restrict__ ptr_n;
    const int* __restrict__ a_ptr;      // CSR(A)
    const int* __restrict__ a_idx;
    const float* __restrict__ a_val;
    const int* __restrict__ at_ptr;     // CSR(A^T)
    const int* __restrict__ at_idx;
    const float* __restrict__ at_val;
    const float* __restrict__ c;
    const float* __restrict__ b;
    const float* x0;
    const float* y0;
    long long max_iters, check_every, lim;
    float eps, step, beta, span;
    int ruiz_passes, pock_chambolle, primal_weight;
    float* x;
    float* y;
    float* dr;
    float* dc;
    int* status;
    float* kkt;
    float* scratch;
    __device__ bool weigh() const { return primal_weight != 0; }
    __device__ float weight_span() const { return span; }
};

struct HalpernArgs {
    static constexpr bool scaled = true;
    static constexpr bool halpern = true;
    static constexpr int kkt_words = 6;
    const int* __restrict__ ptr_m;
    const int* __restrict__ ptr_n;
    const int* __restrict__ a_ptr;      // CSR(A)
    const int* __restrict__ a_idx;
    const float* __restrict__ a_val;
    const int* __restrict__ at_ptr;     // CSR(A^T)
    const int* __restrict__ at_idx;
    const float* __restrict__ at_val;
    const float* __restrict__ c;
    const float* __restrict__ b;
    const float* x0;
    const float* y0;
    long long max_iters, check_every, lim;
    float eps, step, beta, span;
    int ruiz_passes, pock_chambolle, primal_weight, reflect;
    float* x;
    float* y;
    float* dr;
    float* dc;
    int* status;
    float* kkt;
    float* scratch;
    __device__ bool weigh() const { return primal_weight != 0; }
    __device__ float weight_span() const { return span; }
};

struct PdhgErr {
    float p, d, g;      // primal, dual, gap
    __device__ __forceinline__ float worst() const { return nn_max(nn_max(p, d), g); }
};

template <bool IN_LDS, int NT, class Args>
__global__ __launch_bounds__(NT) void pdhg_kernel(const Args A) {
    constexpr bool S = Args::scaled, H = Args::halpern;
    static_assert(S || !H, "the Halpern iteration keeps its anchor in the scaled call's side words");
    constexpr int NW = NT / 64;
    extern __shared__ float pd_lds[];
    __shared__ Sum2 s_part2[NW];
    __shared__ float s_part[NW];
    __shared__ unsigned s_key[NW * 4];
    __shared__ long long s_off[NW];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = A.ptr_m[k], m = A.ptr_m[k + 1] - row0;
    const int col0 = A.ptr_n[k], n = A.ptr_n[k + 1] - col0;
    if ((pdhg_words(m, n) <= A.lim) != IN_LDS) return;      // the other launch's instance
    const float inf = __builtin_huge_valf();
    // This instance's piece of the scratch: behind those of the earlier instances (integer sum: exact).  S: every instance
    // takes its 2 n + 2 m side words there, and its five vectors too when they do not fit LDS; otherwise only the instances
    // whose vectors do not fit take one
    long long off = 0;
    if constexpr (S || !IN_LDS) {
        for (int j = tid; j < k; j += NT) {
            const long long mj = A.ptr_m[j + 1] - A.ptr_m[j], nj = A.ptr_n[j + 1] - A.ptr_n[j];
            if constexpr (S) {
                off += pdhg_scaled_side_words(mj, nj) + (pdhg_words(mj, nj) > A.lim ? pdhg_words(mj, nj) : 0);
            } else {
                const long long w = pdhg_words(mj, nj);
                if (w > A.lim) off += w;
            }
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) off += __shfl_xor(off, o, 64);
        if (lane == 0) s_off[wave] = off;
        __syncthreads();
        off = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) off += s_off[v];
    }
    float* side = A.scratch + off;
    float* tc = S ? side : nullptr;         // [n] dc, then dc^2                              (these four: S only)
    float* xr = S ? tc + n : nullptr;       // [n] the set-up's C, then x at the last restart (H: the anchor)
    float* tr = S ? xr + n : nullptr;       // [m] dr, then dr^2
    float* yr = S ? tr + m : nullptr;       // [m] the set-up's R, then y at the last restart
    float* base = IN_LDS ? pd_lds : S ? yr + m : side;
    float* x = base;                // [n] the iterate
    float* xb = x + n;              // [n] 2 x+ - x
    float* xs = xb + n;             // [n] the sum of the iterates since the last restart; H: xh, the last step's output
    float* y = xs + n;              // [m]
    float* ys = y + m;              // [m] likewise; H: yh
    const int* a_ptr = A.a_ptr + row0;
    const int* at_ptr = A.at_ptr + col0;
    const float* c = A.c + col0;
    const float* b = A.b + row0;
    const bool sums = A.check_every > 0;    // (H: no sums -- whether there are checks)
    const bool weigh = A.weigh();

    // ---- start: the clipped start, the norms of b and c, where the block tier's rows are ----
    unsigned kn[2] = {0u, 0u};      // ||b||inf, ||c||inf
    unsigned kr[4] = {0u, 0u, 0u, 0u};      // block tier: {~first, last + 1} of the columns, of the rows
    for (int j = tid; j < n; j += NT) {
        kn[1] = max(kn[1], abs_bits(c[j]));
        x[j] = A.x0 ? clip0(A.x0[col0 + j]) : 0.0f;
        if constexpr (H) xs[j] = x[j];
        else if (sums) xs[j] = 0.0f;
        if constexpr (S) tc[j] = 1.0f;
        if (row_tier(at_ptr[j + 1] - at_ptr[j]) == 2) {
            kr[0] = max(kr[0], (unsigned)(0x7fffffff - j));
            kr[1] = max(kr[1], (unsigned)(j + 1));
        }
    }
    for (int i = tid; i < m; i += NT) {
        kn[0] = max(kn[0], abs_bits(b[i]));
        y[i] = A.y0 ? A.y0[row0 + i] : 0.0f;
        if constexpr (H) ys[i] = y[i];
        else if (sums) ys[i] = 0.0f;
        if constexpr (S) tr[i] = 1.0f;
        if (row_tier(a_ptr[i + 1] - a_ptr[i]) == 2) {
            kr[2] = max(kr[2], (unsigned)(0x7fffffff - i));
            kr[3] = max(kr[3], (unsigned)(i + 1));
        }
    }
    block_max_u32<NW, 4>(kr, s_key);
    block_max_u32<NW, 2>(kn, s_key);        // (also: every x_j and y_i, S: dc_j and dr_i, is written)
    const int c_lo = kr[1] ? 0x7fffffff - (int)kr[0] : 0, c_hi = (int)kr[1];
    const int r_lo = kr[3] ? 0x7fffffff - (int)kr[2] : 0, r_hi = (int)kr[3];
    const float den_p = __fadd_rn(1.0f, __uint_as_float(kn[0])), den_d = __fadd_rn(1.0f, __uint_as_float(kn[1]));

    // ---- the step eta; S: first the scaling, then the weight's start ----
    unsigned ka[2] = {0u, 0u};      // the largest column result, the largest row result of the last walk
    if constexpr (S) {
        // C and R from the SAME dr, dc, then both updated (tc holds dc, tr holds dr until they are squared)
        auto walk = [&](auto is_max, float* out_c, float* out_r) {
            constexpr bool MAX = decltype(is_max)::value;
            ka[0] = ka[1] = 0u;
            wg_sweep<NT>(at_ptr, n, c_lo, c_hi, ScaledAbs<false, MAX>{A.at_idx, A.at_val, row0, tc, tr, out_c, &ka[0]}, s_part);
            wg_sweep<NT>(a_ptr, m, r_lo, r_hi, ScaledAbs<true, MAX>{A.a_idx, A.a_val, col0, tr, tc, out_r, &ka[1]}, s_part);
        };
        const int passes = A.ruiz_passes + (A.pock_chambolle ? 1 : 0);
        for (int p = 0; p < passes; ++p) {      // (uniform in the workgroup)
            if (p < A.ruiz_passes) walk(std::true_type{}, xr, yr);
            else walk(std::false_type{}, xr, yr);
            __syncthreads();
            for (int j = tid; j < n; j += NT) {
                const float v = xr[j];
                if (v > 0.0f) tc[j] = __fdiv_rn(tc[j], sqrt_rn(v));
            }
            for (int i = tid; i < m; i += NT) {
                const float v = yr[i];
                if (v > 0.0f) tr[i] = __fdiv_rn(tr[i], sqrt_rn(v));
            }
            __syncthreads();
        }
        walk(std::false_type{}, nullptr, nullptr);      // ||S||1 (largest column sum), ||S||inf (largest row sum) of the final s_ij
    } else {
        // ||A||1 (largest column sum), ||A||inf (largest row sum)
        wg_sweep<NT>(at_ptr, n, c_lo, c_hi, AbsSum{A.at_val, &ka[0]}, s_part);
        wg_sweep<NT>(a_ptr, m, r_lo, r_hi, AbsSum{A.a_val, &ka[1]}, s_part);
    }
    float eta;
    {
        block_max_u32<NW, 2>(ka, s_key);
        const float prod = __fmul_rn(__uint_as_float(ka[0]), __uint_as_float(ka[1]));
        eta = prod > 0.0f ? __fdiv_rn(A.step, __fsqrt_rn(prod)) : A.step;      // (the hardware's root for both: the neutral settings' bits)
    }
    float w0 = 1.0f;
    if constexpr (S) {
        // the weight's start, the factors' squares, the restart point (thread t owns words t, t + NT, ... of all of them)
        Sum2 nn = {0.0f, 0.0f};     // |dc o c|^2, |dr o b|^2
        for (int j = tid; j < n; j += NT) {
            const float d = tc[j], v = __fmul_rn(d, c[j]);
            nn.a = __fmaf_rn(v, v, nn.a);
            if (A.dc) A.dc[col0 + j] = d;
            tc[j] = __fmul_rn(d, d);
            xr[j] = x[j];
        }
        for (int i = tid; i < m; i += NT) {
            const float d = tr[i], v = __fmul_rn(d, b[i]);
            nn.b = __fmaf_rn(v, v, nn.b);
            if (A.dr) A.dr[row0 + i] = d;
            tr[i] = __fmul_rn(d, d);
            yr[i] = y[i];
        }
        nn = block_tree_sum<NW>(nn, s_part2);       // (its barriers: tc, tr are written before a sweep's lane reads them)
        const float nc = sqrt_rn(nn.a), nb = sqrt_rn(nn.b);
        if (weigh && finite_pos(nc) && finite_pos(nb)) w0 = __fdiv_rn(nc, nb);
    }
    // the weight w and its clamp, the two steps: both are eta without S, and w never moves
    const float w_lo = __fdiv_rn(w0, A.weight_span()), w_hi = __fmul_rn(w0, A.weight_span());
    float w = w0, tau = S ? __fdiv_rn(eta, w) : eta, sigma = S ? __fmul_rn(eta, w) : eta;

    long long cnt = 0;
    // both points of a check (with_avg) or the point (px, py) alone, in every thread (barriers inside)
    auto evaluate = [&](bool with_avg, PdhgErr& avg, PdhgErr& cur) {
        const float *px = H ? xs : x, *py = H ? ys : y;     // H: the point is the step's output
        const float cntf = (float)cnt;
        unsigned key[4] = {0u, 0u, 0u, 0u};     // primal avg, primal cur, dual avg, dual cur
        wg_sweep<NT>(a_ptr, m, r_lo, r_hi, EvalSweep<true>{A.a_idx, A.a_val, b, col0, with_avg, cntf, px, xs, &key[0], &key[1]}, s_part2);
        wg_sweep<NT>(at_ptr, n, c_lo, c_hi, EvalSweep<false>{A.at_idx, A.at_val, c, row0, with_avg, cntf, py, ys, &key[2], &key[3]}, s_part2);
        Sum2 cx = {0.0f, 0.0f}, by = {0.0f, 0.0f};
        for (int j = tid; j < n; j += NT) {
            const float v = px[j], a = with_avg ? __fdiv_rn(xs[j], cntf) : v;
            cx.a = __fmaf_rn(c[j], a, cx.a);
            cx.b = __fmaf_rn(c[j], v, cx.b);
        }
        for (int i = tid; i < m; i += NT) {
            const float v = py[i], a = with_avg ? __fdiv_rn(ys[i], cntf) : v;
            by.a = __fmaf_rn(b[i], a, by.a);
            by.b = __fmaf_rn(b[i], v, by.b);
        }
        cx = block_tree_sum<NW>(cx, s_part2);
        by = block_tree_sum<NW>(by, s_part2);
        block_max_u32<NW, 4>(key, s_key);
        auto gap = [](float p, float d) {
            return __fdiv_rn(fabsf(__fsub_rn(p, d)), __fadd_rn(__fadd_rn(1.0f, fabsf(p)), fabsf(d)));
        };
        avg = {__fdiv_rn(__uint_as_float(key[0]), den_p), __fdiv_rn(__uint_as_float(key[2]), den_d), gap(cx.a, by.a)};
        cur = {__fdiv_rn(__uint_as_float(key[1]), den_p), __fdiv_rn(__uint_as_float(key[3]), den_d), gap(cx.b, by.b)};
    };

    // ---- the iterations: bounded by max_iters and nothing else ----
    int code = -1, restarts = 0, avg_out = 0;
    long long it = 0, since = 0;
    float e_last = inf;
    PdhgErr out = {0.0f, 0.0f, 0.0f};
    while (it < A.max_iters) {
        if constexpr (H) {
            // The Halpern iteration, whole, ahead of the text of the other two rules (which an `else` or a shared restart would
            // move: DESIGN.md 4.24).  cnt is the rule's k; both weights come from the integer, alike in every thread
            const float w1 = __fdiv_rn((float)(cnt + 1), (float)(cnt + 2)), w2 = __fdiv_rn(1.0f, (float)(cnt + 2));
            const bool reflect = A.reflect != 0;
            wg_sweep<NT>(at_ptr, n, c_lo, c_hi, HalpernCol{A.at_idx, A.at_val, c, tc, xr, row0, tau, w1, w2, reflect, x, xb, xs, y}, s_part);
            __syncthreads();
            wg_sweep<NT>(a_ptr, m, r_lo, r_hi, HalpernRow{A.a_idx, A.a_val, b, tr, yr, col0, sigma, w1, w2, reflect, y, ys, xb}, s_part);
            __syncthreads();
            ++it;
            ++cnt;
            if (!sums || ++since < A.check_every) continue;
            since = 0;
            PdhgErr unused, at;
            evaluate(false, unused, at);        // ONE point: (xh, yh), which is the output as it stands
            const float e = at.worst();
            if (!finite_bits(e) || e <= A.eps) {
                code = finite_bits(e) ? PD_CODE_OPTIMAL : PD_CODE_NOT_FINITE;
                out = at;
                break;
            }
            if (!(e <= __fmul_rn(A.beta, e_last) || 25 * cnt >= 9 * it)) continue;
            ++restarts;
            e_last = e;
            cnt = 0;
            // The restart: (x, y) <- (xh, yh); how far that is from the anchor, in the metric of the scaled variables, for the
            // weight; the anchor moves there with or without the weight.  Thread t owns words t, t + NT, ... of all of them
            Sum2 dd = {0.0f, 0.0f};
            for (int j = tid; j < n; j += NT) {
                const float v = xs[j], d = __fsub_rn(v, xr[j]);
                dd.a = __fmaf_rn(d, __fdiv_rn(d, tc[j]), dd.a);
                x[j] = xr[j] = v;
            }
            for (int i = tid; i < m; i += NT) {
                const float v = ys[i], d = __fsub_rn(v, yr[i]);
                dd.b = __fmaf_rn(d, __fdiv_rn(d, tr[i]), dd.b);
                y[i] = yr[i] = v;
            }
            __syncthreads();        // the next sweep reads x, y, xr, yr from the lanes that finish rows, not from their writers
            if (!weigh) continue;
            dd = block_tree_sum<NW>(dd, s_part2);       // (every thread gets the tree's bits: the same w, tau, sigma in all)
            const float dx = sqrt_rn(dd.a), dy = sqrt_rn(dd.b);
            if (finite_pos(dx) && finite_pos(dy)) {
                const float raw = sqrt_rn(__fmul_rn(w, __fdiv_rn(dy, dx)));
                const float up = raw > w_lo ? raw : w_lo;
                w = up < w_hi ? up : w_hi;
                tau = __fdiv_rn(eta, w);
                sigma = __fmul_rn(eta, w);
            }
            continue;
        }
        wg_sweep<NT>(at_ptr, n, c_lo, c_hi, ColStep<S>{A.at_idx, A.at_val, c, tc, row0, tau, sums, x, xb, xs, y}, s_part);
        __syncthreads();
        wg_sweep<NT>(a_ptr, m, r_lo, r_hi, RowStep<S>{A.a_idx, A.a_val, b, tr, col0, sigma, sums, y, ys, xb}, s_part);
        __syncthreads();
        ++it;
        if (!sums) continue;
        ++cnt;
        if (++since < A.check_every) continue;
        since = 0;
        PdhgErr avg, cur;
        evaluate(true, avg, cur);
        const float ea = avg.worst(), ec = cur.worst();
        const bool use_avg = ea < ec;
        const float e = use_avg ? ea : ec;
        if (!finite_bits(e)) {
            code = PD_CODE_NOT_FINITE;
            out = cur;
            break;
        }
        const bool stop = e <= A.eps;
        if (!stop && !(e <= __fmul_rn(A.beta, e_last) || 25 * cnt >= 9 * it)) continue;
        // the candidate becomes the iterate: the output of code 0, the start of the next period otherwise
        const float cntf = (float)cnt;
        for (int j = tid; j < n; j += NT) {
            if (use_avg) x[j] = __fdiv_rn(xs[j], cntf);
            xs[j] = 0.0f;
        }
        for (int i = tid; i < m; i += NT) {
            if (use_avg) y[i] = __fdiv_rn(ys[i], cntf);
            ys[i] = 0.0f;
        }
        __syncthreads();
        if (stop) {
            code = PD_CODE_OPTIMAL;
            avg_out = use_avg ? 1 : 0;
            out = use_avg ? avg : cur;
            break;
        }
        ++restarts;
        e_last = e;
        cnt = 0;
        if constexpr (S) {
            if (!weigh) continue;
            // the weight: how far the restart moved in each space, in the metric of the scaled variables.  Every thread gets
            // the tree's bits, so every thread holds the same w, tau and sigma
            Sum2 dd = {0.0f, 0.0f};
            for (int j = tid; j < n; j += NT) {
                const float v = x[j], d = __fsub_rn(v, xr[j]);
                dd.a = __fmaf_rn(d, __fdiv_rn(d, tc[j]), dd.a);
                xr[j] = v;
            }
            for (int i = tid; i < m; i += NT) {
                const float v = y[i], d = __fsub_rn(v, yr[i]);
                dd.b = __fmaf_rn(d, __fdiv_rn(d, tr[i]), dd.b);
                yr[i] = v;
            }
            dd = block_tree_sum<NW>(dd, s_part2);
            const float dx = sqrt_rn(dd.a), dy = sqrt_rn(dd.b);
            if (finite_pos(dx) && finite_pos(dy)) {
                const float raw = sqrt_rn(__fmul_rn(w, __fdiv_rn(dy, dx)));
                const float up = raw > w_lo ? raw : w_lo;
                w = up < w_hi ? up : w_hi;
                tau = __fdiv_rn(eta, w);
                sigma = __fmul_rn(eta, w);
            }
        }
    }
    if (code < 0) {
        code = PD_CODE_LIMIT;
        PdhgErr unused;
        evaluate(false, unused, out);
    }
    for (int j = tid; j < n; j += NT) A.x[col0 + j] = (H ? xs : x)[j];
    for (int i = tid; i < m; i += NT) A.y[row0 + i] = (H ? ys : y)[i];
    if (tid == 0) {
        int* st = A.status + 4 * (size_t)k;
        st[0] = code;
        st[1] = (int)min(it, (long long)0x7fffffff);
        st[2] = restarts;
        st[3] = avg_out;
        if (A.kkt) {
            float* q = A.kkt + Args::kkt_words * (size_t)k;
            q[0] = out.p; q[1] = out.d; q[2] = out.g; q[3] = eta;
            if constexpr (S) { q[4] = w0; q[5] = w; }
        }
    }
}

// side: every instance takes its side words in the scratch
LpPlan pdhg_plan(const mllp_graph_t* g, int64_t max_lds_words, bool side) {
    // the largest 3 n + 2 m that runs with its five vectors in LDS
    const int64_t lim = std::min<int64_t>(max_lds_words, PDHG_LDS_WORDS);
    return lp_plan(g, [=](int64_t m, int64_t n) {
        const int64_t w = pdhg_words(m, n);
        return LpInstance{w <= lim, true, (side ? pdhg_scaled_side_words(m, n) : 0) + (w <= lim ? 0 : w), w};
    });
}

bool overlaps(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

// The checks that every entry point makes first, and the arguments that every kernel takes.
template <class Args>
int pdhg_args(const char* fn, const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0,
              int64_t max_iters, int64_t check_every, float eps, float step, float beta, int64_t max_lds_words, float* d_x,
              float* d_y, int32_t* d_status, float* d_kkt, void* d_scratch, Args* args) {
    REQUIRE_FOR(fn, g && d_x1 && d_x2 && d_x && d_y && d_status, "null argument (g, d_x1, d_x2, d_x, d_y and d_status are required)");
    REQUIRE_FOR(fn, max_iters >= 0, "max_iters must not be negative");
    REQUIRE_FOR(fn, check_every >= 0, "check_every must not be negative");
    REQUIRE_FOR(fn, max_lds_words >= 0, "max_lds_words must not be negative");
    REQUIRE_FOR(fn, std::isfinite(eps) && eps >= 0.0f, "eps must be finite and not negative");
    REQUIRE_FOR(fn, std::isfinite(step) && step > 0.0f && step <= 1.0f, "step must be in (0, 1]");
    REQUIRE_FOR(fn, std::isfinite(beta) && beta > 0.0f && beta < 1.0f, "beta must be in (0, 1)");
    Args& a = *args = Args{};
    a.ptr_m = g->inst_ptr_m; a.ptr_n = g->inst_ptr_n;
    a.a_ptr = g->A.ptr; a.a_idx = g->A.idx; a.a_val = g->A.val;
    a.at_ptr = g->At.ptr; a.at_idx = g->At.idx; a.at_val = g->At.val;
    a.c = d_x1; a.b = d_x2; a.x0 = d_x0; a.y0 = d_y0;
    a.max_iters = (long long)max_iters; a.check_every = (long long)check_every;
    a.lim = (long long)std::min<int64_t>(max_lds_words, PDHG_LDS_WORDS);
    a.eps = eps; a.step = step; a.beta = beta;
    a.x = d_x; a.y = d_y; a.status = d_status; a.kkt = d_kkt; a.scratch = static_cast<float*>(d_scratch);
    return MLLP_OK;
}

// The rest of a call, after the entry point's own checks: the plan, the scratch and overlap checks, and a launch per address
// space of the five vectors that has an instance.  Errors of HIP carry the entry point's name without its prefix.
template <class Args>
int pdhg_launch(const char* fn, const mllp_graph_t* g, const Args& args, void* stream) {
    const LpPlan plan = pdhg_plan(g, args.lim, Args::scaled);
    REQUIRE_FOR(fn, plan.words == 0 || args.scratch, std::string("null d_scratch (") + fn + "_scratch_bytes is not 0)");
    const float *dr = nullptr, *dc = nullptr;
    if constexpr (Args::scaled) { dr = args.dr; dc = args.dc; }
    const struct {
        const void* p;
        int64_t bytes;
    } outs[] = {{args.x, g->N * 4}, {args.y, g->M * 4}, {dr, g->M * 4}, {dc, g->N * 4}, {args.status, g->n_inst * 16},
                {args.kkt, g->n_inst * 4 * Args::kkt_words}};
    for (const auto& o : outs)
        REQUIRE_FOR(fn, !overlaps(args.x0, g->N * 4, o.p, o.bytes) && !overlaps(args.y0, g->M * 4, o.p, o.bytes),
                    "d_x0 or d_y0 overlaps an output");
    if (g->n_inst <= 0) return MLLP_OK;
    hipStream_t s = (hipStream_t)stream;
    const std::string name = fn + sizeof("mllp_") - 1;
    int rc = MLLP_OK;
    if (plan.any_lds)
        rc = lp_launch<pdhg_kernel<true, PDHG_THREADS, Args>, PDHG_THREADS>(name, " (LDS)", g->n_inst, lp_lds_bytes(PDHG_LDS_WORDS),
                                                                            lp_lds_bytes(plan.lds_extent), s, args);
    if (!rc && plan.any_glb)    // (no dynamic LDS: no limit to raise)
        rc = lp_launch<pdhg_kernel<false, PDHG_THREADS, Args>, PDHG_THREADS>(name, " (scratch)", g->n_inst, 0, 0, s, args);
    return rc;
}

// The options that mllp_lp_pdhg_scaled adds to mllp_lp_pdhg's, and mllp_lp_pdhg_halpern takes too: their checks, after pdhg_args'.
template <class Args>
int scaled_options(const char* fn, int64_t ruiz_passes, int32_t pock_chambolle, int32_t primal_weight, float weight_span, float* d_dr,
                   float* d_dc, Args* args) {
    REQUIRE_FOR(fn, ruiz_passes >= 0 && ruiz_passes <= PDHG_SCALED_MAX_RUIZ, "ruiz_passes must be in 0 .. 64");
    REQUIRE_FOR(fn, std::isfinite(weight_span) && weight_span >= 1.0f, "weight_span must be finite and at least 1");
    args->span = weight_span;
    args->ruiz_passes = (int)ruiz_passes;
    args->pock_chambolle = pock_chambolle != 0;
    args->primal_weight = primal_weight != 0;
    args->dr = d_dr;
    args->dc = d_dc;
    return MLLP_OK;
}

int pdhg_scaled_limits(const char* fn, int64_t* limits) {
    REQUIRE_FOR(fn, limits, "null argument");
    limits[0] = PDHG_SCALED_LDS_WORDS;
    limits[1] = PDHG_SCALED_THREADS;
    limits[2] = PDHG_SCALED_MAX_RUIZ;
    return MLLP_OK;
}

int pdhg_scratch_bytes(const char* fn, const mllp_graph_t* g, int64_t max_lds_words, bool side, int64_t* bytes) {
    REQUIRE_FOR(fn, g && bytes, "null argument");
    REQUIRE_FOR(fn, max_lds_words >= 0, "max_lds_words must not be negative");
    *bytes = pdhg_plan(g, max_lds_words, side).words * (int64_t)sizeof(float);
    return MLLP_OK;
}

}  // namespace

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_lp_pdhg_limits(int64_t* limits) {
    REQUIRE(limits, "null argument");
    limits[0] = PDHG_LDS_WORDS;
    limits[1] = PDHG_THREADS;
    return MLLP_OK;
}

extern "C" int mllp_lp_pdhg_scaled_limits(int64_t* limits) { return pdhg_scaled_limits(__func__, limits); }

extern "C" int mllp_lp_pdhg_halpern_limits(int64_t* limits) { return pdhg_scaled_limits(__func__, limits); }

extern "C" int mllp_lp_pdhg_scratch_bytes(const mllp_graph_t* g, int64_t max_lds_words, int64_t* bytes) {
    return pdhg_scratch_bytes(__func__, g, max_lds_words, false, bytes);
}

extern "C" int mllp_lp_pdhg_scaled_scratch_bytes(const mllp_graph_t* g, int64_t max_lds_words, int64_t* bytes) {
    return pdhg_scratch_bytes(__func__, g, max_lds_words, true, bytes);
}

extern "C" int mllp_lp_pdhg_halpern_scratch_bytes(const mllp_graph_t* g, int64_t max_lds_words, int64_t* bytes) {
    return pdhg_scratch_bytes(__func__, g, max_lds_words, true, bytes);
}

extern "C" int mllp_lp_pdhg(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0,
                            int64_t max_iters, int64_t check_every, float eps, float step, float beta, int64_t max_lds_words,
                            float* d_x, float* d_y, int32_t* d_status, float* d_kkt, void* d_scratch, void* stream) {
    PdhgArgs args;
    if (int rc = pdhg_args(__func__, g, d_x1, d_x2, d_x0, d_y0, max_iters, check_every, eps, step, beta, max_lds_words, d_x, d_y,
                           d_status, d_kkt, d_scratch, &args))
        return rc;
    return pdhg_launch(__func__, g, args, stream);
}

extern "C" int mllp_lp_pdhg_scaled(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0,
                                   int64_t max_iters, int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes,
                                   int32_t pock_chambolle, int32_t primal_weight, float weight_span, int64_t max_lds_words,
                                   float* d_x, float* d_y, float* d_dr, float* d_dc, int32_t* d_status, float* d_kkt,
                                   void* d_scratch, void* stream) {
    ScaledArgs args;
    if (int rc = pdhg_args(__func__, g, d_x1, d_x2, d_x0, d_y0, max_iters, check_every, eps, step, beta, max_lds_words, d_x, d_y,
                           d_status, d_kkt, d_scratch, &args))
        return rc;
    if (int rc = scaled_options(__func__, ruiz_passes, pock_chambolle, primal_weight, weight_span, d_dr, d_dc, &args)) return rc;
    return pdhg_launch(__func__, g, args, stream);
}

extern "C" int mllp_lp_pdhg_halpern(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0,
                                    int64_t max_iters, int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes,
                                    int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect,
                                    int64_t max_lds_words, float* d_x, float* d_y, float* d_dr, float* d_dc, int32_t* d_status,
                                    float* d_kkt, void* d_scratch, void* stream) {
    HalpernArgs args;
    if (int rc = pdhg_args(__func__, g, d_x1, d_x2, d_x0, d_y0, max_iters, check_every, eps, step, beta, max_lds_words, d_x, d_y,
                           d_status, d_kkt, d_scratch, &args))
        return rc;
    if (int rc = scaled_options(__func__, ruiz_passes, pock_chambolle, primal_weight, weight_span, d_dr, d_dc, &args)) return rc;
    args.reflect = reflect != 0;
    return pdhg_launch(__func__, g, args, stream);
}
