// pdhg_wide.hip -- mllp_lp_pdhg_halpern's rule run across the whole device: mllp_lp_pdhg_wide.  The rule is
// stated in include/mllp_hip.h under mllp_lp_pdhg_halpern and is followed word for word; what changes is WHO runs it.  The
// persistent kernel of pdhg.hip gives an instance one workgroup for the whole call; here an instance's rows (columns) are cut
// into items of rows_per_item consecutive rows, one workgroup of 1024 threads each, and the call is a sequence of ordinary
// launches in stream order.  No kernel waits on another workgroup: every ordering between two phases is the stream's.
//
// TWO KINDS OF KERNEL.
//   sweep     grid = the items of every instance of the batch, of one orientation.  A workgroup finds its (instance, block)
//             by a search of the first-item table that the call's first kernel made from inst_ptr_m / inst_ptr_n, and sums its
//             rows in ordered_sum.h's three tiers exactly as pdhg.hip's wg_sweep does: a row's bits depend on its length alone,
//             so it does not matter which workgroup owns it.  One lane finishes a row: one writer per word.  The maxima (the
//             two norms of the set-up's last walk, the two residuals of an evaluation) are integer maxima over the patterns of
//             non-negative floats, reduced in the workgroup and then by ONE atomicMax per workgroup on a state word.
//   instance  grid = n_inst, one workgroup of 1024 threads per instance: everything the rule sums "in the order of c'x"
//             (thread t adds t, t + 1024, ..., then the butterfly and the tree) and every decision.
// A call:   prep (instance);  iter_begin == 0: per scaling pass {column walk, row walk (sweeps), update (instance)}, the last
//           walk of both orientations (sweeps), start (instance);  per iteration {column sweep, row sweep};  after every
//           check_every-th iteration (absolute) {row evaluation, column evaluation (sweeps), decide (instance)};  at the end
//           {row evaluation, column evaluation, finish (instance)}.
//
// STATE.  16 words per instance at the head of the caller's scratch (WS_* below), all of them VALUES: no index, offset or
// pointer that a kernel follows.  Every address is formed from inst_ptr_m / inst_ptr_n, blockIdx and the arguments, so whatever
// the state holds no access leaves the buffers.  A call with iter_begin > 0 accepts an instance only when its state says that the
// previous call ended exactly at iter_begin (code 0, 6 or 8); otherwise the instance is stale for this call (flag, not state:
// the state is left as found), its sweeps return at once and finish writes zeros and code 9.
//
// mllp_lp_pdhg_rays is the same call with certificates of infeasibility and unboundedness.  Its first and last
// kernel are the wide call's bodies with their additions under `if constexpr (RAYS)` (prep_body, finish_body: the entry points
// are one-line wrappers), and with ray_eps >= 0 it has its own three kernels of a check, further down, whose restart is the
// wide call's (wide_restart); every launch of a call has its counterpart in the other call, so the two make the same number of
// launches.  A value that RAYS changes is DEFINED once, never set and then overwritten (DESIGN.md 4.22's habit).
//
// mllp_lp_pdhg_spectral is the rays call whose set-up estimates |S|_2 by power iteration between the last walk
// and the start: spec_init, then per round spec_product<rows>, spec_product<columns>, spec_normalize -- 3 P + 1 launches, none
// at P = 0 -- and spec_start / spec_finish, which are the wide start and the rays finish with the estimate (start_body<SPEC>) and
// d_norm.  Its two state words lie BEHIND the rays' words.
//
// WHAT IS DEFINED WHERE.  pdhg_ops.h, shared with pdhg.hip: the status codes, the bit helpers, block_max_u32,
// BySum and ByMax, ScaledAbs, ScaledProd, HalpernCol, HalpernRow -- the iteration and the set-up walks are written once.
// This file: the walker of an item (item_sweep: pdhg.hip's wg_sweep places the block tier differently, see pdhg_ops.h) and the
// operators that only these kernels instantiate.  EvalOne walks ONE point with a float accumulator, which is the `cur` half of
// pdhg.hip's Sum2 walk (EvalSweep): the two halves of a Sum2 never meet.
#include <cmath>
#include <string>

#include "internal.h"
#include "ordered_sum.h"
#include "pdhg_ops.h"

namespace mllp {

namespace {

constexpr int WD_THREADS = 1024;
constexpr int WD_NW = WD_THREADS / 64;
constexpr int WD_CHUNK = WD_THREADS / 16;          // rows that a workgroup takes at a time: one 16-lane group each
constexpr int64_t WD_ROWS_DEFAULT = 64, WD_ROWS_MAX = 4096;
constexpr int64_t WD_MAX_RUIZ = 64;

// the state's words (int or float, by the name)
enum {
    WS_CODE = 0,        // 6 while the instance runs (what it ends with at the limit), 0 or 8 once it stopped
    WS_IT_LO, WS_IT_HI,         // iterations done by the instance (it stops counting at code 0 or 8)
    WS_REACHED_LO, WS_REACHED_HI,       // iter_end of the call that wrote the state last
    WS_LAST_LO, WS_LAST_HI,     // the iteration of the last restart: the rule's k is the iteration number minus this
    WS_RESTARTS,
    WS_E_LAST, WS_W0, WS_W, WS_TAU, WS_SIGMA, WS_ETA,
    WS_DEN_P, WS_DEN_D,         // 1 + |b|inf, 1 + |c|inf
    WS_WORDS
};
// per instance behind the state: the call's flag, the four maxima, the first item of each orientation
enum { WX_FLAG = 0, WX_KEY_COL, WX_KEY_ROW, WX_FIRST_N, WX_FIRST_M, WX_WORDS };
constexpr int WD_RUN = 1, WD_IDLE = 2, WD_STALE = 3;
constexpr int64_t WD_INST_WORDS = WS_WORDS + WX_WORDS;

__host__ __device__ constexpr int64_t wide_words(int64_t n_inst, int64_t M, int64_t N) { return WD_INST_WORDS * n_inst + 6 * N + 5 * M; }

// pdhg.hip's wg_sweep for the rows [rb, re) of an instance (ptr: the row pointers of the instance's first row), re - rb any
// number: WD_CHUNK rows at a time, and a chunk's rows of the block tier behind its other rows -- a vote of the workgroup says
// whether it has one, so that every thread takes the barriers of that tier or none does.  No barrier at the end
template <class Op>
__device__ __forceinline__ void item_sweep(const int* __restrict__ ptr, int rb, int re, const Op& op, typename Op::Acc* part) {
    using By = typename Op::By;
    using Acc = typename Op::Acc;
    const int tid = threadIdx.x, lane = tid & 63;
    for (int r0 = rb; r0 < re; r0 += WD_CHUNK) {             // (r0 is uniform in the workgroup)
        const int r = r0 + (tid >> 4);
        const bool in = r < re;
        const int beg = in ? ptr[r] : 0, len = in ? ptr[r + 1] - beg : 0;
        {   // group tier: every lane reaches the butterfly; a row of another tier runs it over no terms
            const bool mine = in && row_tier(len) == 0;
            const typename Op::Row rc = op.row(mine ? r : rb);
            const Acc q = By::template group<16>(strided_terms<16>(op, rc, beg, mine ? len : 0, tid & 15));
            if (mine && (tid & 15) == 0) op.finish(r, rc, q);
        }
#pragma unroll
        for (int g = 0; g < 4; ++g) {                        // wave tier: the wavefront's four rows in turn
            const int b4 = __shfl(beg, 16 * g, 64), l4 = __shfl(len, 16 * g, 64);
            if (row_tier(l4) != 1) continue;                 // (uniform in the wavefront; a row past `re` has no terms)
            const int r4 = r0 + (tid >> 6) * 4 + g;
            const typename Op::Row rc = op.row(r4);
            const Acc q = By::template group<64>(strided_terms<64>(op, rc, b4, l4, lane));
            if (lane == 0) op.finish(r4, rc, q);
        }
        if (!__syncthreads_or(in && row_tier(len) == 2)) continue;
        const int r1 = min(r0 + WD_CHUNK, re);
        for (int q2 = r0; q2 < r1; ++q2) {                   // block tier
            const int b2 = ptr[q2], l2 = ptr[q2 + 1] - b2;
            if (row_tier(l2) != 2) continue;
            const typename Op::Row rc = op.row(q2);
            const Acc q = By::template block<WD_NW>(strided_terms<WD_THREADS>(op, rc, b2, l2, tid), part);
            if (tid == 0) op.finish(q2, rc, q);
        }
    }
}

// an evaluation's walk of one orientation: the product with the OTHER side's point, then the residual against `rhs`: |.| for
// rows (primal), max(., 0) for columns (dual).  The `cur` half of pdhg.hip's EvalSweep
template <bool ROWS>
struct EvalOne {
    using Acc = float;
    using Row = NoRow;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ rhs;
    int off;
    const float* v;
    unsigned* best;
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, float& q) const { q = __fmaf_rn(val[e], v[idx[e] - off], q); }
    __device__ __forceinline__ void finish(int r, const Row&, float q) const {
        const float d = __fsub_rn(q, rhs[r]);
        const unsigned k = ROWS ? abs_bits(d) : pos_bits(d);
        *best = k > *best ? k : *best;
    }
};

// What every kernel takes.  Nothing here comes from the state
struct WideArgs {
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
    long long iter_begin, iter_end, check_every;
    float eps, step, beta, span;
    int primal_weight, reflect, rows, n_inst;
    long long M, N;
    float* x_out;
    float* y_out;
    float* dr_out;
    float* dc_out;
    int* status;
    float* kkt;
    float* scratch;
};

// where an instance's words are.  The vectors are indexed like c and b: by the batch's column (row) number
struct WideView {
    int k, row0, m, col0, n;
    int* st;            // the state [WS_WORDS]
    int* ex;            // flag, keys, first items [WX_WORDS]
    float *x, *xb, *xh, *xa, *tc, *dc;      // [n] the iterate, 2 xh - x, the step's output, the anchor (set-up: C), dc^2, dc
    float *y, *yh, *ya, *tr, *dr;           // [m] likewise (set-up: R in ya)
};

__device__ __forceinline__ WideView wide_view(const WideArgs& A, int k) {
    WideView v;
    v.k = k;
    v.row0 = A.ptr_m[k]; v.m = A.ptr_m[k + 1] - v.row0;
    v.col0 = A.ptr_n[k]; v.n = A.ptr_n[k + 1] - v.col0;
    int* words = reinterpret_cast<int*>(A.scratch);
    v.st = words + WD_INST_WORDS * (long long)k;
    v.ex = v.st + WS_WORDS;
    float* cols = A.scratch + WD_INST_WORDS * (long long)A.n_inst;
    float* rows = cols + 6 * A.N;
    v.x = cols + v.col0; v.xb = v.x + A.N; v.xh = v.xb + A.N; v.xa = v.xh + A.N; v.tc = v.xa + A.N; v.dc = v.tc + A.N;
    v.y = rows + v.row0; v.yh = v.y + A.M; v.ya = v.yh + A.M; v.tr = v.ya + A.M; v.dr = v.tr + A.M;
    return v;
}

__device__ __forceinline__ long long get64(const int* st, int lo) {
    return (long long)(((unsigned long long)(unsigned)st[lo + 1] << 32) | (unsigned)st[lo]);
}
__device__ __forceinline__ void put64(int* st, int lo, long long v) {
    st[lo] = (int)(unsigned)((unsigned long long)v & 0xffffffffull);
    st[lo + 1] = (int)(unsigned)((unsigned long long)v >> 32);
}
__device__ __forceinline__ float stf(const int* st, int w) { return __int_as_float(st[w]); }

// mllp_lp_pdhg_rays: six more words per instance BEHIND the vectors of the wide layout (which stays as it is): the two ray keys,
// which are the call's own as the two keys above are, and the four cert words {qp, b'ry, qd, c'rx} of the last check that
// evaluated the rays, which are STATE (values only) and travel from one call to the next
enum { RX_KEY_U = 0, RX_KEY_V, RX_QP, RX_BY, RX_QD, RX_CX, RX_WORDS };

__host__ __device__ constexpr int64_t rays_words(int64_t n_inst, int64_t M, int64_t N) { return wide_words(n_inst, M, N) + RX_WORDS * n_inst; }

// what the rays' kernels take beside WideArgs (whose layout every kernel of the wide call depends on)
struct RayArgs {
    float ray_eps;
    float* ray_x;
    float* ray_y;
    float* cert;
};

__device__ __forceinline__ int* ray_words(const WideArgs& A, int k) {
    return reinterpret_cast<int*>(A.scratch) + wide_words(A.n_inst, A.M, A.N) + RX_WORDS * (long long)k;
}

// mllp_lp_pdhg_spectral: two more words per instance BEHIND the rays' words, both STATE (values only): the
// estimate sigma_est (0: void, or power_iters = 0) and the bound sqrt(|S|_1 |S|_inf), which every call writes to d_norm.  During
// the set-up the first word is the power iteration's own: nu of the last round (|h|_2 before the first), 0 once void
enum { SX_SIGMA = 0, SX_BOUND, SX_WORDS };
constexpr int64_t WD_MAX_POWER = 1024;

__host__ __device__ constexpr int64_t spectral_words(int64_t n_inst, int64_t M, int64_t N) { return rays_words(n_inst, M, N) + SX_WORDS * n_inst; }

// what mllp_lp_pdhg_spectral takes beside the rays' arguments (host only: the kernels get them as arguments of their own)
struct SpecArgs {
    int64_t power_iters;
    float* norm;
};

__device__ __forceinline__ int* spec_words(const WideArgs& A, int k) {
    return reinterpret_cast<int*>(A.scratch) + rays_words(A.n_inst, A.M, A.N) + SX_WORDS * (long long)k;
}

// the workgroup's item: the instance k with first[k] <= blockIdx.x < first[k + 1] (the table is made by wide_prep of THIS call
// from inst_ptr alone; thread t looks at instances t, t + 1024, ..., so the search costs one round of loads and two barriers),
// and the block inside it.  False, for the whole workgroup: no item (cannot happen with the grid the host computes from the
// same offsets; whatever the table holds, k is an instance and the block lies inside its rows)
template <bool COLS>
__device__ __forceinline__ bool wide_item(const WideArgs& A, int* k_out, int* rb, int* re) {
    __shared__ int s_k;
    const int* first = reinterpret_cast<const int*>(A.scratch) + WS_WORDS + (COLS ? WX_FIRST_N : WX_FIRST_M);
    const int item = (int)blockIdx.x;
    if (threadIdx.x == 0) s_k = -1;
    __syncthreads();
    for (int t = threadIdx.x; t < A.n_inst; t += WD_THREADS) {
        const int f = first[WD_INST_WORDS * (long long)t];
        const int nxt = t + 1 < A.n_inst ? first[WD_INST_WORDS * (long long)(t + 1)] : 0x7fffffff;
        if (f <= item && item < nxt) s_k = t;
    }
    __syncthreads();
    const int lo = s_k;
    if (lo < 0) return false;
    const int* p = COLS ? A.ptr_n : A.ptr_m;
    const int rows = p[lo + 1] - p[lo];
    const long long blk = (long long)item - first[WD_INST_WORDS * (long long)lo];
    if (blk < 0 || blk * A.rows >= rows) return false;
    *k_out = lo;
    *rb = (int)(blk * A.rows);
    *re = min(rows, *rb + A.rows);
    return true;
}

// the workgroup's largest key into the state word, by one thread
__device__ __forceinline__ void publish_max(unsigned best, int* word, unsigned* s_key) {
    unsigned v[1] = {best};
    block_max_u32<WD_NW, 1>(v, s_key);
    if (threadIdx.x == 0 && v[0]) atomicMax(reinterpret_cast<unsigned*>(word), v[0]);
}

// ---- the call's first kernel: the item table, the flags; iter_begin == 0: the start and the state.  RAYS: it also knows codes
// 4 and 5, clears the ray keys and starts the cert ----
template <bool RAYS>
__device__ __forceinline__ void prep_body(const WideArgs A) {
    __shared__ unsigned s_key[WD_NW * 2];
    __shared__ long long s_off[WD_NW * 2];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const WideView V = wide_view(A, k);
    int* rw = RAYS ? ray_words(A, k) : nullptr;
    // the items of the earlier instances (integer sums: exact)
    long long fn = 0, fm = 0;
    for (int j = tid; j < k; j += WD_THREADS) {
        fn += (A.ptr_n[j + 1] - A.ptr_n[j] + A.rows - 1) / A.rows;
        fm += (A.ptr_m[j + 1] - A.ptr_m[j] + A.rows - 1) / A.rows;
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        fn += __shfl_xor(fn, o, 64);
        fm += __shfl_xor(fm, o, 64);
    }
    if (lane == 0) { s_off[wave * 2] = fn; s_off[wave * 2 + 1] = fm; }
    __syncthreads();
    if (tid == 0) {
        fn = fm = 0;
        for (int w = 0; w < WD_NW; ++w) { fn += s_off[w * 2]; fm += s_off[w * 2 + 1]; }
        V.ex[WX_FIRST_N] = (int)fn;
        V.ex[WX_FIRST_M] = (int)fm;
        V.ex[WX_KEY_COL] = 0;
        V.ex[WX_KEY_ROW] = 0;
        if constexpr (RAYS) {
            rw[RX_KEY_U] = 0;
            rw[RX_KEY_V] = 0;
        }
    }
    if (A.iter_begin > 0) {
        // which codes a continued call accepts; anything else, or a state that did not end at iter_begin, is stale
        if (tid == 0) {
            const int code = V.st[WS_CODE];
            const bool known = code == PD_CODE_OPTIMAL || code == PD_CODE_LIMIT || code == PD_CODE_NOT_FINITE ||
                               (RAYS && (code == PD_CODE_INFEASIBLE || code == PD_CODE_UNBOUNDED));
            V.ex[WX_FLAG] = !known || get64(V.st, WS_REACHED_LO) != A.iter_begin ? WD_STALE : code == PD_CODE_LIMIT ? WD_RUN : WD_IDLE;
        }
        return;
    }
    // the clipped start, which is also the step's output so far; unit factors; the norms of b and c
    const float* c = A.c + V.col0;
    const float* b = A.b + V.row0;
    unsigned kn[2] = {0u, 0u};      // ||b||inf, ||c||inf
    for (int j = tid; j < V.n; j += WD_THREADS) {
        kn[1] = max(kn[1], abs_bits(c[j]));
        const float v = A.x0 ? clip0(A.x0[V.col0 + j]) : 0.0f;
        V.x[j] = v;
        V.xh[j] = v;
        V.dc[j] = 1.0f;
    }
    for (int i = tid; i < V.m; i += WD_THREADS) {
        kn[0] = max(kn[0], abs_bits(b[i]));
        const float v = A.y0 ? A.y0[V.row0 + i] : 0.0f;
        V.y[i] = v;
        V.yh[i] = v;
        V.dr[i] = 1.0f;
    }
    block_max_u32<WD_NW, 2>(kn, s_key);
    if (tid == 0) {
        V.ex[WX_FLAG] = WD_RUN;
        V.st[WS_CODE] = PD_CODE_LIMIT;
        put64(V.st, WS_IT_LO, 0);
        put64(V.st, WS_REACHED_LO, -1);     // (no call has ended on this state yet)
        put64(V.st, WS_LAST_LO, 0);
        V.st[WS_RESTARTS] = 0;
        V.st[WS_E_LAST] = __float_as_int(__builtin_huge_valf());
        V.st[WS_DEN_P] = __float_as_int(__fadd_rn(1.0f, __uint_as_float(kn[0])));
        V.st[WS_DEN_D] = __float_as_int(__fadd_rn(1.0f, __uint_as_float(kn[1])));
        if constexpr (RAYS) {
            rw[RX_QP] = __float_as_int(__builtin_huge_valf());      // no check has evaluated the rays
            rw[RX_BY] = 0;
            rw[RX_QD] = __float_as_int(__builtin_huge_valf());
            rw[RX_CX] = 0;
        }
    }
}
__global__ __launch_bounds__(WD_THREADS) void wide_prep(const WideArgs A) { prep_body<false>(A); }
__global__ __launch_bounds__(WD_THREADS) void rays_prep(const WideArgs A) { prep_body<true>(A); }

// ---- the set-up's walks.  MAX: a Ruiz pass, else the sums; LAST: no result per row, the largest into the keys ----
template <bool COLS, bool MAX, bool LAST>
__global__ __launch_bounds__(WD_THREADS) void wide_scale_walk(const WideArgs A) {
    __shared__ float s_part[WD_NW];
    __shared__ unsigned s_key[WD_NW];
    int k, rb, re;
    if (!wide_item<COLS>(A, &k, &rb, &re)) return;
    const WideView V = wide_view(A, k);
    unsigned best = 0u;
    if constexpr (COLS)
        item_sweep(A.at_ptr + V.col0, rb, re, ScaledAbs<false, MAX>{A.at_idx, A.at_val, V.row0, V.dc, V.dr, LAST ? nullptr : V.xa, &best}, s_part);
    else
        item_sweep(A.a_ptr + V.row0, rb, re, ScaledAbs<true, MAX>{A.a_idx, A.a_val, V.col0, V.dr, V.dc, LAST ? nullptr : V.ya, &best}, s_part);
    if constexpr (LAST) publish_max(best, V.ex + (COLS ? WX_KEY_COL : WX_KEY_ROW), s_key);
}

// after a pass's two walks: both factors from the SAME C and R
__global__ __launch_bounds__(WD_THREADS) void wide_scale_update(const WideArgs A) {
    const WideView V = wide_view(A, blockIdx.x);
    for (int j = threadIdx.x; j < V.n; j += WD_THREADS) {
        const float v = V.xa[j];
        if (v > 0.0f) V.dc[j] = __fdiv_rn(V.dc[j], sqrt_rn(v));
    }
    for (int i = threadIdx.x; i < V.m; i += WD_THREADS) {
        const float v = V.ya[i];
        if (v > 0.0f) V.dr[i] = __fdiv_rn(V.dr[i], sqrt_rn(v));
    }
}

// after the last walk: eta, the weight's start, the factors' squares, the anchor.  SPEC (mllp_lp_pdhg_spectral): the step's
// denominator is the power iteration's estimate where that is finite, positive and not above the bound; the two go to the state
template <bool SPEC>
__device__ __forceinline__ void start_body(const WideArgs A, long long power_iters) {
    __shared__ Sum2 s_part2[WD_NW];
    const int tid = threadIdx.x;
    const WideView V = wide_view(A, blockIdx.x);
    const float* c = A.c + V.col0;
    const float* b = A.b + V.row0;
    const float prod = __fmul_rn(__int_as_float(V.ex[WX_KEY_COL]), __int_as_float(V.ex[WX_KEY_ROW]));
    int* sw = SPEC ? spec_words(A, blockIdx.x) : nullptr;
    float bound = 0.0f, est = 0.0f, eta;
    if constexpr (SPEC) {
        const float nu = power_iters > 0 ? stf(sw, SX_SIGMA) : 0.0f;        // (read before thread 0 writes: the tree's barriers lie between)
        bound = __fsqrt_rn(prod);
        est = finite_pos(nu) ? sqrt_rn(nu) : 0.0f;
        eta = prod > 0.0f ? __fdiv_rn(A.step, est > 0.0f && est <= bound ? est : bound) : A.step;
    } else {
        eta = prod > 0.0f ? __fdiv_rn(A.step, __fsqrt_rn(prod)) : A.step;      // (the hardware's root, as pdhg.hip takes it)
    }
    Sum2 nn = {0.0f, 0.0f};     // |dc o c|^2, |dr o b|^2
    for (int j = tid; j < V.n; j += WD_THREADS) {
        const float d = V.dc[j], v = __fmul_rn(d, c[j]);
        nn.a = __fmaf_rn(v, v, nn.a);
        V.tc[j] = __fmul_rn(d, d);
        V.xa[j] = V.x[j];
    }
    for (int i = tid; i < V.m; i += WD_THREADS) {
        const float d = V.dr[i], v = __fmul_rn(d, b[i]);
        nn.b = __fmaf_rn(v, v, nn.b);
        V.tr[i] = __fmul_rn(d, d);
        V.ya[i] = V.y[i];
    }
    nn = block_tree_sum<WD_NW>(nn, s_part2);        // (its barriers: every thread has read the keys before thread 0 clears them)
    const float nc = sqrt_rn(nn.a), nb = sqrt_rn(nn.b);
    float w0 = 1.0f;
    if (A.primal_weight && finite_pos(nc) && finite_pos(nb)) w0 = __fdiv_rn(nc, nb);
    if (tid == 0) {
        V.st[WS_ETA] = __float_as_int(eta);
        V.st[WS_W0] = __float_as_int(w0);
        V.st[WS_W] = __float_as_int(w0);
        V.st[WS_TAU] = __float_as_int(__fdiv_rn(eta, w0));
        V.st[WS_SIGMA] = __float_as_int(__fmul_rn(eta, w0));
        V.ex[WX_KEY_COL] = 0;
        V.ex[WX_KEY_ROW] = 0;
        if constexpr (SPEC) {
            sw[SX_SIGMA] = __float_as_int(est);
            sw[SX_BOUND] = __float_as_int(bound);
        }
    }
}
__global__ __launch_bounds__(WD_THREADS) void wide_start(const WideArgs A) { start_body<false>(A, 0); }
__global__ __launch_bounds__(WD_THREADS) void spec_start(const WideArgs A, long long power_iters) { start_body<true>(A, power_iters); }

// ---- mllp_lp_pdhg_spectral's power iteration on S'S, S = diag(dr) A diag(dc), between the last walk and the start.  xb holds
// fmul(dc_j, v_j), ya holds fmul(dr_i, u_i), xa holds w: the three are free here (xa and ya were the scaling's C and R, xb is
// not read before the first column sweep writes it).  An instance whose word is 0 is void: its kernels return at once ----
// the start vector: h_j = 1 + ((j 2654435761 mod 2^32) >> 9) 2^-23, j inside the instance; v = h / |h|_2
__global__ __launch_bounds__(WD_THREADS) void spec_init(const WideArgs A) {
    __shared__ float s_part[WD_NW];
    const int tid = threadIdx.x;
    const WideView V = wide_view(A, blockIdx.x);
    float q = 0.0f;
    for (int j = tid; j < V.n; j += WD_THREADS) {
        const float h = __uint_as_float(0x3f800000u | (((unsigned)j * 2654435761u) >> 9));
        q = __fmaf_rn(h, h, q);
    }
    const float nh = sqrt_rn(block_tree_sum<WD_NW>(q, s_part));
    const bool good = finite_pos(nh);
    for (int j = tid; good && j < V.n; j += WD_THREADS) {
        const float h = __uint_as_float(0x3f800000u | (((unsigned)j * 2654435761u) >> 9));
        V.xb[j] = __fmul_rn(V.dc[j], __fdiv_rn(h, nh));
    }
    if (tid == 0) spec_words(A, blockIdx.x)[SX_SIGMA] = good ? __float_as_int(nh) : 0;
}

// a round's two sweeps: rows, u = dr o (A (dc o v)), stored with dr once more; then columns, w = dc o (A' (dr o u))
template <bool COLS>
__global__ __launch_bounds__(WD_THREADS) void spec_product(const WideArgs A) {
    __shared__ float s_part[WD_NW];
    int k, rb, re;
    if (!wide_item<COLS>(A, &k, &rb, &re)) return;
    const WideView V = wide_view(A, k);
    if (spec_words(A, k)[SX_SIGMA] == 0) return;        // (uniform in the workgroup: no kernel of this launch writes the word)
    if constexpr (COLS)
        item_sweep(A.at_ptr + V.col0, rb, re, ScaledProd<false>{A.at_idx, A.at_val, V.row0, V.dc, V.ya, V.xa}, s_part);
    else
        item_sweep(A.a_ptr + V.row0, rb, re, ScaledProd<true>{A.a_idx, A.a_val, V.col0, V.dr, V.xb, V.ya}, s_part);
}

// a round's end: nu = |w|_2 in the order of c'x, v = w / nu (stored as fmul(dc_j, v_j)); nu not finite and positive: void
__global__ __launch_bounds__(WD_THREADS) void spec_normalize(const WideArgs A) {
    __shared__ float s_part[WD_NW];
    const int tid = threadIdx.x;
    const WideView V = wide_view(A, blockIdx.x);
    int* sw = spec_words(A, blockIdx.x);
    if (sw[SX_SIGMA] == 0) return;      // (every thread reads it before the tree's barriers, thread 0 writes it behind them)
    float q = 0.0f;
    for (int j = tid; j < V.n; j += WD_THREADS) q = __fmaf_rn(V.xa[j], V.xa[j], q);
    const float nu = sqrt_rn(block_tree_sum<WD_NW>(q, s_part));
    const bool good = finite_pos(nu);
    for (int j = tid; good && j < V.n; j += WD_THREADS) V.xb[j] = __fmul_rn(V.dc[j], __fdiv_rn(V.xa[j], nu));
    if (tid == 0) sw[SX_SIGMA] = good ? __float_as_int(nu) : 0;
}

// ---- an iteration's two sweeps.  `it`: the iterations done before this one ----
template <bool COLS>
__global__ __launch_bounds__(WD_THREADS) void wide_step(const WideArgs A, long long it) {
    __shared__ float s_part[WD_NW];
    int k, rb, re;
    if (!wide_item<COLS>(A, &k, &rb, &re)) return;
    const WideView V = wide_view(A, k);
    if (V.ex[WX_FLAG] != WD_RUN || V.st[WS_CODE] != PD_CODE_LIMIT) return;
    const long long cnt = it - get64(V.st, WS_LAST_LO);         // the rule's k
    const float w1 = __fdiv_rn((float)(cnt + 1), (float)(cnt + 2)), w2 = __fdiv_rn(1.0f, (float)(cnt + 2));
    const bool reflect = A.reflect != 0;
    if constexpr (COLS)
        item_sweep(A.at_ptr + V.col0, rb, re,
                   HalpernCol{A.at_idx, A.at_val, A.c + V.col0, V.tc, V.xa, V.row0, stf(V.st, WS_TAU), w1, w2, reflect, V.x, V.xb, V.xh, V.y}, s_part);
    else
        item_sweep(A.a_ptr + V.row0, rb, re,
                   HalpernRow{A.a_idx, A.a_val, A.b + V.row0, V.tr, V.ya, V.col0, stf(V.st, WS_SIGMA), w1, w2, reflect, V.y, V.yh, V.xb}, s_part);
}

// ---- an evaluation's two sweeps of (xh, yh).  FINAL: every instance that is not stale, else the running ones ----
template <bool ROWS, bool FINAL>
__global__ __launch_bounds__(WD_THREADS) void wide_eval(const WideArgs A) {
    __shared__ float s_part[WD_NW];
    __shared__ unsigned s_key[WD_NW];
    int k, rb, re;
    if (!wide_item<!ROWS>(A, &k, &rb, &re)) return;
    const WideView V = wide_view(A, k);
    const int flag = V.ex[WX_FLAG];
    if (FINAL ? flag == WD_STALE : (flag != WD_RUN || V.st[WS_CODE] != PD_CODE_LIMIT)) return;
    unsigned best = 0u;
    if constexpr (ROWS)
        item_sweep(A.a_ptr + V.row0, rb, re, EvalOne<true>{A.a_idx, A.a_val, A.b + V.row0, V.col0, V.xh, &best}, s_part);
    else
        item_sweep(A.at_ptr + V.col0, rb, re, EvalOne<false>{A.at_idx, A.at_val, A.c + V.col0, V.row0, V.yh, &best}, s_part);
    publish_max(best, V.ex + (ROWS ? WX_KEY_ROW : WX_KEY_COL), s_key);
}

struct WideErr {
    float p, d, g;
    __device__ __forceinline__ float worst() const { return nn_max(nn_max(p, d), g); }
};

// the three errors of a point from the keys of its two evaluation sweeps and s = (c'x, b'y)
__device__ __forceinline__ WideErr wide_err(const WideView& V, unsigned key_p, unsigned key_d, float cx, float by) {
    const float gap = __fdiv_rn(fabsf(__fsub_rn(cx, by)), __fadd_rn(__fadd_rn(1.0f, fabsf(cx)), fabsf(by)));
    return {__fdiv_rn(__uint_as_float(key_p), stf(V.st, WS_DEN_P)), __fdiv_rn(__uint_as_float(key_d), stf(V.st, WS_DEN_D)), gap};
}

// the three errors of (xh, yh) from the keys of the two evaluation sweeps, in every thread; clears the keys
__device__ __forceinline__ WideErr wide_errors(const WideArgs& A, const WideView& V, Sum2* s_part2) {
    const int tid = threadIdx.x;
    const float* c = A.c + V.col0;
    const float* b = A.b + V.row0;
    const unsigned key_p = (unsigned)V.ex[WX_KEY_ROW], key_d = (unsigned)V.ex[WX_KEY_COL];
    Sum2 s = {0.0f, 0.0f};      // c'x, b'y
    for (int j = tid; j < V.n; j += WD_THREADS) s.a = __fmaf_rn(c[j], V.xh[j], s.a);
    for (int i = tid; i < V.m; i += WD_THREADS) s.b = __fmaf_rn(b[i], V.yh[i], s.b);
    s = block_tree_sum<WD_NW>(s, s_part2);          // (its barriers: every thread has read the keys)
    if (tid == 0) {
        V.ex[WX_KEY_ROW] = 0;
        V.ex[WX_KEY_COL] = 0;
    }
    return wide_err(V, key_p, key_d, s.a, s.b);
}

// A check's restart, by every thread of the instance's workgroup: (x, y) <- (xh, yh), how far that is from the anchor in the
// metric of the scaled variables, the anchor moves there; then thread 0 writes the state: the restart's count, error and
// iteration, and with primal_weight the weight moved to sqrt(w dy / dx), clamped to [w0 / span, w0 span], and the two steps.
// restarts, w0, w, eta: the state as every thread read it before any of it was written
__device__ __forceinline__ void wide_restart(const WideArgs& A, const WideView& V, long long it, float e, int restarts, float w0, float w,
                                             float eta, Sum2* s_part2) {
    const int tid = threadIdx.x;
    Sum2 dd = {0.0f, 0.0f};
    for (int j = tid; j < V.n; j += WD_THREADS) {
        const float v = V.xh[j], d = __fsub_rn(v, V.xa[j]);
        dd.a = __fmaf_rn(d, __fdiv_rn(d, V.tc[j]), dd.a);
        V.x[j] = V.xa[j] = v;
    }
    for (int i = tid; i < V.m; i += WD_THREADS) {
        const float v = V.yh[i], d = __fsub_rn(v, V.ya[i]);
        dd.b = __fmaf_rn(d, __fdiv_rn(d, V.tr[i]), dd.b);
        V.y[i] = V.ya[i] = v;
    }
    dd = block_tree_sum<WD_NW>(dd, s_part2);
    if (tid != 0) return;
    V.st[WS_RESTARTS] = restarts + 1;
    V.st[WS_E_LAST] = __float_as_int(e);
    put64(V.st, WS_LAST_LO, it);
    if (!A.primal_weight) return;
    const float dx = sqrt_rn(dd.a), dy = sqrt_rn(dd.b);
    if (finite_pos(dx) && finite_pos(dy)) {
        const float w_lo = __fdiv_rn(w0, A.span), w_hi = __fmul_rn(w0, A.span);
        const float raw = sqrt_rn(__fmul_rn(w, __fdiv_rn(dy, dx)));
        const float up = raw > w_lo ? raw : w_lo;
        const float wn = up < w_hi ? up : w_hi;
        V.st[WS_W] = __float_as_int(wn);
        V.st[WS_TAU] = __float_as_int(__fdiv_rn(eta, wn));
        V.st[WS_SIGMA] = __float_as_int(__fmul_rn(eta, wn));
    }
}

// ---- a check's decision, after its two sweeps.  `it`: the iterations done ----
__global__ __launch_bounds__(WD_THREADS) void wide_decide(const WideArgs A, long long it) {
    __shared__ Sum2 s_part2[WD_NW];
    const int tid = threadIdx.x;
    const WideView V = wide_view(A, blockIdx.x);
    if (V.ex[WX_FLAG] != WD_RUN || V.st[WS_CODE] != PD_CODE_LIMIT) return;
    // the state, in every thread, before thread 0 writes any of it (the barriers of wide_errors lie between)
    const long long cnt = it - get64(V.st, WS_LAST_LO);
    const float e_last = stf(V.st, WS_E_LAST), w0 = stf(V.st, WS_W0), w = stf(V.st, WS_W), eta = stf(V.st, WS_ETA);
    const int restarts = V.st[WS_RESTARTS];
    const WideErr at = wide_errors(A, V, s_part2);
    const float e = at.worst();
    if (!finite_bits(e) || e <= A.eps) {
        if (tid == 0) {
            V.st[WS_CODE] = finite_bits(e) ? PD_CODE_OPTIMAL : PD_CODE_NOT_FINITE;
            put64(V.st, WS_IT_LO, it);
        }
        return;
    }
    if (!(e <= __fmul_rn(A.beta, e_last) || 25 * cnt >= 9 * it)) return;
    wide_restart(A, V, it, e, restarts, w0, w, eta, s_part2);
}

// ---- the call's last kernel, after the final evaluation's sweeps: every output of every instance.  RAYS: also the rays (from
// the frozen xh - xa, so with the bits of the deciding check) and the cert words.  A stale instance gets zeros and code 9 ----
template <bool RAYS>
__device__ __forceinline__ void finish_body(const WideArgs A, const RayArgs R) {
    __shared__ Sum2 s_part2[WD_NW];
    const int tid = threadIdx.x;
    const WideView V = wide_view(A, blockIdx.x);
    const bool stale = V.ex[WX_FLAG] == WD_STALE;       // (uniform in the workgroup: a word that this call's prep wrote)
    const int code = stale ? PD_CODE_STALE : V.st[WS_CODE];
    WideErr out = {0.0f, 0.0f, 0.0f};
    if (!stale) out = wide_errors(A, V, s_part2);
    for (int j = tid; j < V.n; j += WD_THREADS) {
        A.x_out[V.col0 + j] = stale ? 0.0f : V.xh[j];
        if (A.dc_out) A.dc_out[V.col0 + j] = stale ? 0.0f : V.dc[j];
        if constexpr (RAYS)
            if (R.ray_x) R.ray_x[V.col0 + j] = code == PD_CODE_UNBOUNDED ? __fsub_rn(V.xh[j], V.xa[j]) : 0.0f;
    }
    for (int i = tid; i < V.m; i += WD_THREADS) {
        A.y_out[V.row0 + i] = stale ? 0.0f : V.yh[i];
        if (A.dr_out) A.dr_out[V.row0 + i] = stale ? 0.0f : V.dr[i];
        if constexpr (RAYS)
            if (R.ray_y) R.ray_y[V.row0 + i] = code == PD_CODE_INFEASIBLE ? __fsub_rn(V.yh[i], V.ya[i]) : 0.0f;
    }
    if (tid != 0) return;
    int* st = A.status + 4 * (size_t)V.k;
    float* q = A.kkt ? A.kkt + 6 * (size_t)V.k : nullptr;
    float* ce = RAYS && R.cert ? R.cert + 4 * (size_t)V.k : nullptr;
    if (stale) {
        st[0] = PD_CODE_STALE; st[1] = 0; st[2] = 0; st[3] = 0;
        if (q) q[0] = q[1] = q[2] = q[3] = q[4] = q[5] = 0.0f;
        if (ce) ce[0] = ce[1] = ce[2] = ce[3] = 0.0f;
        return;
    }
    if (code == PD_CODE_LIMIT) put64(V.st, WS_IT_LO, A.iter_end);
    put64(V.st, WS_REACHED_LO, A.iter_end);
    st[0] = code;
    st[1] = (int)min(get64(V.st, WS_IT_LO), (long long)0x7fffffff);
    st[2] = V.st[WS_RESTARTS];
    st[3] = 0;
    if (q) {
        q[0] = out.p; q[1] = out.d; q[2] = out.g;
        q[3] = stf(V.st, WS_ETA); q[4] = stf(V.st, WS_W0); q[5] = stf(V.st, WS_W);
    }
    if (ce) {
        const int* rw = ray_words(A, V.k);
        ce[0] = stf(rw, RX_QP); ce[1] = stf(rw, RX_BY); ce[2] = stf(rw, RX_QD); ce[3] = stf(rw, RX_CX);
    }
}
__global__ __launch_bounds__(WD_THREADS) void wide_finish(const WideArgs A) { finish_body<false>(A, RayArgs{}); }
__global__ __launch_bounds__(WD_THREADS) void rays_finish(const WideArgs A, const RayArgs R) { finish_body<true>(A, R); }
// mllp_lp_pdhg_spectral: the rays' last kernel, then d_norm from the state (zeros for a stale instance)
__global__ __launch_bounds__(WD_THREADS) void spec_finish(const WideArgs A, const RayArgs R, float* norm) {
    finish_body<true>(A, R);
    if (threadIdx.x != 0 || !norm) return;
    const bool stale = wide_view(A, blockIdx.x).ex[WX_FLAG] == WD_STALE;
    const int* sw = spec_words(A, blockIdx.x);
    norm[2 * (size_t)blockIdx.x] = stale ? 0.0f : stf(sw, SX_SIGMA);
    norm[2 * (size_t)blockIdx.x + 1] = stale ? 0.0f : stf(sw, SX_BOUND);
}

// =====================================================================================================================
// mllp_lp_pdhg_rays: a check with certificates of infeasibility and unboundedness.  The candidate ray
// is the direction from the anchor to the step's output, (rx, ry) = (xh - xa, yh - ya), which Halpern's iteration drives to the
// infimal displacement of the PDHG operator: zero for a solvable LP, a Farkas or recession ray otherwise.  Nothing is stored for
// it: a check's two sweeps walk every row once for TWO accumulators, the point's and the ray's (pdhg.hip's EvalSweep pair,
// with zero right-hand sides for the ray), and the decision adds b'ry, c'rx and max(-rx) to the walk that forms c'x and b'y.
// With ray_eps < 0 the host launches the three kernels of a check above instead, so that nothing is evaluated.  The call's first
// and last kernel are prep_body and finish_body with RAYS, above; the restart is wide_restart, as in wide_decide.
// =====================================================================================================================
// an evaluation's walk for the point v and the ray fsub(v, va) at once: one load of the value and of the index per term, two
// gathers.  The point's residual is EvalOne's; the ray's has no right-hand side: |A rx| for rows, max(A'ry, 0) for columns
template <bool ROWS>
struct EvalPair {
    using Acc = Sum2;       // a: the point, b: the ray
    using Row = NoRow;
    using By = BySum;
    const int* __restrict__ idx;
    const float* __restrict__ val;
    const float* __restrict__ rhs;
    int off;
    const float *v, *va;
    unsigned* best;         // [2]: the point's key, the ray's
    __device__ __forceinline__ Row row(int) const { return {}; }
    __device__ __forceinline__ void term(const Row&, int e, Sum2& q) const {
        const float a = val[e];
        const int i = idx[e] - off;
        const float p = v[i];
        q.a = __fmaf_rn(a, p, q.a);
        q.b = __fmaf_rn(a, __fsub_rn(p, va[i]), q.b);
    }
    __device__ __forceinline__ void finish(int r, const Row&, Sum2 q) const {
        const float d = __fsub_rn(q.a, rhs[r]);
        const unsigned k = ROWS ? abs_bits(d) : pos_bits(d), kr = ROWS ? abs_bits(q.b) : pos_bits(q.b);
        best[0] = k > best[0] ? k : best[0];
        best[1] = kr > best[1] ? kr : best[1];
    }
};

// ---- a check's two sweeps of (xh, yh) and of the ray, for the running instances.  Two integer maxima per workgroup ----
template <bool ROWS>
__global__ __launch_bounds__(WD_THREADS) void rays_eval(const WideArgs A) {
    __shared__ Sum2 s_part2[WD_NW];
    __shared__ unsigned s_key[WD_NW * 2];
    int k, rb, re;
    if (!wide_item<!ROWS>(A, &k, &rb, &re)) return;
    const WideView V = wide_view(A, k);
    if (V.ex[WX_FLAG] != WD_RUN || V.st[WS_CODE] != PD_CODE_LIMIT) return;
    unsigned best[2] = {0u, 0u};
    if constexpr (ROWS)
        item_sweep(A.a_ptr + V.row0, rb, re, EvalPair<true>{A.a_idx, A.a_val, A.b + V.row0, V.col0, V.xh, V.xa, best}, s_part2);
    else
        item_sweep(A.at_ptr + V.col0, rb, re, EvalPair<false>{A.at_idx, A.at_val, A.c + V.col0, V.row0, V.yh, V.ya, best}, s_part2);
    block_max_u32<WD_NW, 2>(best, s_key);
    if (threadIdx.x != 0) return;
    int* rw = ray_words(A, k);
    if (best[0]) atomicMax(reinterpret_cast<unsigned*>(V.ex + (ROWS ? WX_KEY_ROW : WX_KEY_COL)), best[0]);
    if (best[1]) atomicMax(reinterpret_cast<unsigned*>(rw + (ROWS ? RX_KEY_V : RX_KEY_U)), best[1]);
}

// ---- a check's decision with the rays: wide_decide with the ray step between "e <= eps" and the restart test ----
__global__ __launch_bounds__(WD_THREADS) void rays_decide(const WideArgs A, const RayArgs R, long long it) {
    __shared__ Sum2 s_part2[WD_NW];
    __shared__ unsigned s_key[WD_NW];
    const int tid = threadIdx.x;
    const WideView V = wide_view(A, blockIdx.x);
    if (V.ex[WX_FLAG] != WD_RUN || V.st[WS_CODE] != PD_CODE_LIMIT) return;
    int* rw = ray_words(A, blockIdx.x);
    const long long cnt = it - get64(V.st, WS_LAST_LO);
    const float e_last = stf(V.st, WS_E_LAST), w0 = stf(V.st, WS_W0), w = stf(V.st, WS_W), eta = stf(V.st, WS_ETA);
    const int restarts = V.st[WS_RESTARTS];
    const float* c = A.c + V.col0;
    const float* b = A.b + V.row0;
    const unsigned key_p = (unsigned)V.ex[WX_KEY_ROW], key_d = (unsigned)V.ex[WX_KEY_COL];
    const unsigned key_u = (unsigned)rw[RX_KEY_U], key_v = (unsigned)rw[RX_KEY_V];
    // one walk: c'x and b'y of the point, c'rx and b'ry of the ray, the largest -rx
    Sum2 s = {0.0f, 0.0f}, r = {0.0f, 0.0f};
    unsigned neg[1] = {0u};
    for (int j = tid; j < V.n; j += WD_THREADS) {
        const float xh = V.xh[j], rx = __fsub_rn(xh, V.xa[j]);
        s.a = __fmaf_rn(c[j], xh, s.a);
        r.a = __fmaf_rn(c[j], rx, r.a);
        const unsigned kn = pos_bits(-rx);
        neg[0] = kn > neg[0] ? kn : neg[0];
    }
    for (int i = tid; i < V.m; i += WD_THREADS) {
        const float yh = V.yh[i];
        s.b = __fmaf_rn(b[i], yh, s.b);
        r.b = __fmaf_rn(b[i], __fsub_rn(yh, V.ya[i]), r.b);
    }
    s = block_tree_sum<WD_NW>(s, s_part2);          // (its barriers: every thread has read the four keys)
    r = block_tree_sum<WD_NW>(r, s_part2);
    block_max_u32<WD_NW, 1>(neg, s_key);
    if (tid == 0) {
        V.ex[WX_KEY_ROW] = 0;
        V.ex[WX_KEY_COL] = 0;
        rw[RX_KEY_U] = 0;
        rw[RX_KEY_V] = 0;
    }
    const float e = wide_err(V, key_p, key_d, s.a, s.b).worst();
    if (!finite_bits(e) || e <= A.eps) {
        if (tid == 0) {
            V.st[WS_CODE] = finite_bits(e) ? PD_CODE_OPTIMAL : PD_CODE_NOT_FINITE;
            put64(V.st, WS_IT_LO, it);
        }
        return;
    }
    // the rays: qp = U / b'ry, qd = V / -c'rx; a comparison with a NaN is false
    const float cx = r.a, by = r.b, inf = __builtin_huge_valf();
    const float U = __uint_as_float(key_u), Vr = __uint_as_float(key_v > neg[0] ? key_v : neg[0]);
    const float qp = finite_bits(by) && by > 0.0f ? __fdiv_rn(U, by) : inf;
    const float qd = finite_bits(cx) && cx < 0.0f ? __fdiv_rn(Vr, -cx) : inf;
    if (tid == 0) {
        rw[RX_QP] = __float_as_int(qp);
        rw[RX_BY] = __float_as_int(by);
        rw[RX_QD] = __float_as_int(qd);
        rw[RX_CX] = __float_as_int(cx);
    }
    if (qp <= R.ray_eps || qd <= R.ray_eps) {
        if (tid == 0) {
            V.st[WS_CODE] = qp <= R.ray_eps ? PD_CODE_INFEASIBLE : PD_CODE_UNBOUNDED;
            put64(V.st, WS_IT_LO, it);
        }
        return;
    }
    if (!(e <= __fmul_rn(A.beta, e_last) || 25 * cnt >= 9 * it)) return;
    wide_restart(A, V, it, e, restarts, w0, w, eta, s_part2);
}

bool overlaps(const void* a, int64_t a_bytes, const void* b, int64_t b_bytes) {
    if (!a || !b || a_bytes <= 0 || b_bytes <= 0) return false;
    const uintptr_t a0 = (uintptr_t)a, b0 = (uintptr_t)b;
    return a0 < b0 + (uintptr_t)b_bytes && b0 < a0 + (uintptr_t)a_bytes;
}

int wide_rows(const char* fn, int64_t rows_per_item, int64_t* rows) {
    REQUIRE_FOR(fn, rows_per_item >= 0 && rows_per_item <= WD_ROWS_MAX && rows_per_item % 64 == 0,
                "rows_per_item must be 0 or a multiple of 64 up to 4096");
    *rows = rows_per_item ? rows_per_item : WD_ROWS_DEFAULT;
    return MLLP_OK;
}

// the items of one orientation, from the host copy of the instance offsets
int64_t wide_items(const std::vector<int64_t>& p, int64_t n_inst, int64_t rows) {
    int64_t items = 0;
    for (int64_t k = 0; k < n_inst && k + 1 < (int64_t)p.size(); ++k) items += (p[k + 1] - p[k] + rows - 1) / rows;
    return items;
}

// the scratch's words of the three calls: each layout is the one before it with words behind
int64_t call_words(const mllp_graph_t* g, bool rays, bool spec) {
    return spec ? spectral_words(g->n_inst, g->M, g->N) : rays ? rays_words(g->n_inst, g->M, g->N) : wide_words(g->n_inst, g->M, g->N);
}

// a launch of the entry point `fn` ("mllp_" + what an error names it by)
template <class... KArgs, class... Args>
int wide_go(void (*kernel)(KArgs...), const char* fn, const char* what, int64_t grid, hipStream_t s, const Args&... args) {
    if (grid <= 0) return MLLP_OK;
    hipLaunchKernelGGL(kernel, dim3((unsigned)grid), dim3(WD_THREADS), 0, s, args...);
    const hipError_t e = hipGetLastError();
    return e == hipSuccess ? MLLP_OK : hip_fail(e, (std::string(fn + 5) + " (" + what + ")").c_str());
}

// mllp_lp_pdhg_wide (rays == nullptr) and mllp_lp_pdhg_rays: the refusals, the arguments and the launches.  The two calls make
// the same launches in the same order; with rays the first and the last kernel are the rays' own, and with ray_eps >= 0 so are
// the three of a check.  mllp_lp_pdhg_spectral (spec != nullptr, which comes with rays): the rays call's launches with its own
// start and finish, and 3 P + 1 more between the last walk and the start when P = power_iters > 0
int wide_call(const char* fn, const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0, int64_t iter_begin,
              int64_t iter_end, int64_t check_every, float eps, float step, float beta, int64_t ruiz_passes, int32_t pock_chambolle,
              int32_t primal_weight, float weight_span, int32_t reflect, const RayArgs* rays, const SpecArgs* spec, int64_t rows_per_item,
              float* d_x, float* d_y, float* d_dr, float* d_dc, int32_t* d_status, float* d_kkt, void* d_scratch, void* stream) {
    REQUIRE_FOR(fn, g && d_x1 && d_x2 && d_x && d_y && d_status, "null argument (g, d_x1, d_x2, d_x, d_y and d_status are required)");
    REQUIRE_FOR(fn, iter_begin >= 0, "iter_begin must not be negative");
    REQUIRE_FOR(fn, iter_end >= iter_begin, "iter_end must not be below iter_begin");
    REQUIRE_FOR(fn, check_every >= 0, "check_every must not be negative");
    REQUIRE_FOR(fn, std::isfinite(eps) && eps >= 0.0f, "eps must be finite and not negative");
    REQUIRE_FOR(fn, std::isfinite(step) && step > 0.0f && step <= 1.0f, "step must be in (0, 1]");
    REQUIRE_FOR(fn, std::isfinite(beta) && beta > 0.0f && beta < 1.0f, "beta must be in (0, 1)");
    REQUIRE_FOR(fn, ruiz_passes >= 0 && ruiz_passes <= WD_MAX_RUIZ, "ruiz_passes must be in 0 .. 64");
    REQUIRE_FOR(fn, std::isfinite(weight_span) && weight_span >= 1.0f, "weight_span must be finite and at least 1");
    REQUIRE_FOR(fn, !rays || std::isfinite(rays->ray_eps), "ray_eps must be finite (negative: no detection)");
    REQUIRE_FOR(fn, !spec || (spec->power_iters >= 0 && spec->power_iters <= WD_MAX_POWER), "power_iters must be in 0 .. 1024");
    int64_t rows;
    if (int rc = wide_rows(fn, rows_per_item, &rows)) return rc;
    const int64_t words = call_words(g, rays != nullptr, spec != nullptr);
    REQUIRE_FOR(fn, words == 0 || d_scratch, std::string("null d_scratch (") + fn + "_scratch_bytes is not 0)");
    const struct {
        const void* p;
        int64_t bytes;
    } outs[] = {{d_x, g->N * 4}, {d_y, g->M * 4}, {d_dr, g->M * 4}, {d_dc, g->N * 4}, {d_status, g->n_inst * 16}, {d_kkt, g->n_inst * 24},
                {rays ? rays->ray_x : nullptr, g->N * 4}, {rays ? rays->ray_y : nullptr, g->M * 4}, {rays ? rays->cert : nullptr, g->n_inst * 16},
                {spec ? spec->norm : nullptr, g->n_inst * 8}};
    for (const auto& o : outs)
        REQUIRE_FOR(fn, !overlaps(d_x0, g->N * 4, o.p, o.bytes) && !overlaps(d_y0, g->M * 4, o.p, o.bytes), "d_x0 or d_y0 overlaps an output");
    if (g->n_inst <= 0) return MLLP_OK;

    WideArgs a{};
    a.ptr_m = g->inst_ptr_m; a.ptr_n = g->inst_ptr_n;
    a.a_ptr = g->A.ptr; a.a_idx = g->A.idx; a.a_val = g->A.val;
    a.at_ptr = g->At.ptr; a.at_idx = g->At.idx; a.at_val = g->At.val;
    a.c = d_x1; a.b = d_x2; a.x0 = d_x0; a.y0 = d_y0;
    a.iter_begin = (long long)iter_begin; a.iter_end = (long long)iter_end; a.check_every = (long long)check_every;
    a.eps = eps; a.step = step; a.beta = beta; a.span = weight_span;
    a.primal_weight = primal_weight != 0; a.reflect = reflect != 0; a.rows = (int)rows; a.n_inst = (int)g->n_inst;
    a.M = (long long)g->M; a.N = (long long)g->N;
    a.x_out = d_x; a.y_out = d_y; a.dr_out = d_dr; a.dc_out = d_dc; a.status = d_status; a.kkt = d_kkt;
    a.scratch = static_cast<float*>(d_scratch);
    const bool detect = rays && rays->ray_eps >= 0.0f;
    const RayArgs r = rays ? *rays : RayArgs{};

    hipStream_t s = (hipStream_t)stream;
    const int64_t K = g->n_inst;
    const int64_t items_n = wide_items(g->h_inst_ptr_n, K, rows), items_m = wide_items(g->h_inst_ptr_m, K, rows);
    int rc = rays ? wide_go(rays_prep, fn, "prep", K, s, a) : wide_go(wide_prep, fn, "prep", K, s, a);
    if (!rc && iter_begin == 0) {
        for (int64_t p = 0; !rc && p < ruiz_passes + (pock_chambolle ? 1 : 0); ++p) {
            if (p < ruiz_passes) {
                rc = wide_go(wide_scale_walk<true, true, false>, fn, "scaling, columns", items_n, s, a);
                if (!rc) rc = wide_go(wide_scale_walk<false, true, false>, fn, "scaling, rows", items_m, s, a);
            } else {
                rc = wide_go(wide_scale_walk<true, false, false>, fn, "scaling, columns", items_n, s, a);
                if (!rc) rc = wide_go(wide_scale_walk<false, false, false>, fn, "scaling, rows", items_m, s, a);
            }
            if (!rc) rc = wide_go(wide_scale_update, fn, "scaling, update", K, s, a);
        }
        if (!rc) rc = wide_go(wide_scale_walk<true, false, true>, fn, "norm, columns", items_n, s, a);
        if (!rc) rc = wide_go(wide_scale_walk<false, false, true>, fn, "norm, rows", items_m, s, a);
        const long long P = spec ? (long long)spec->power_iters : 0;
        if (!rc && P > 0) rc = wide_go(spec_init, fn, "power, start", K, s, a);
        for (long long r = 0; !rc && r < P; ++r) {
            rc = wide_go(spec_product<false>, fn, "power, rows", items_m, s, a);
            if (!rc) rc = wide_go(spec_product<true>, fn, "power, columns", items_n, s, a);
            if (!rc) rc = wide_go(spec_normalize, fn, "power, norm", K, s, a);
        }
        if (!rc) rc = spec ? wide_go(spec_start, fn, "start", K, s, a, P) : wide_go(wide_start, fn, "start", K, s, a);
    }
    for (long long it = (long long)iter_begin; !rc && it < (long long)iter_end; ++it) {
        rc = wide_go(wide_step<true>, fn, "columns", items_n, s, a, it);
        if (!rc) rc = wide_go(wide_step<false>, fn, "rows", items_m, s, a, it);
        if (rc || check_every == 0 || (it + 1) % check_every) continue;
        if (detect) {
            rc = wide_go(rays_eval<true>, fn, "check, rows", items_m, s, a);
            if (!rc) rc = wide_go(rays_eval<false>, fn, "check, columns", items_n, s, a);
            if (!rc) rc = wide_go(rays_decide, fn, "check", K, s, a, r, it + 1);
        } else {
            rc = wide_go(wide_eval<true, false>, fn, "check, rows", items_m, s, a);
            if (!rc) rc = wide_go(wide_eval<false, false>, fn, "check, columns", items_n, s, a);
            if (!rc) rc = wide_go(wide_decide, fn, "check", K, s, a, it + 1);
        }
    }
    if (!rc) rc = wide_go(wide_eval<true, true>, fn, "evaluation, rows", items_m, s, a);
    if (!rc) rc = wide_go(wide_eval<false, true>, fn, "evaluation, columns", items_n, s, a);
    if (!rc)
        rc = spec   ? wide_go(spec_finish, fn, "finish", K, s, a, r, spec->norm)
             : rays ? wide_go(rays_finish, fn, "finish", K, s, a, r)
                    : wide_go(wide_finish, fn, "finish", K, s, a);
    return rc;
}

}  // namespace

}  // namespace mllp

using namespace mllp;

static int wide_limits(const char* fn, int64_t* limits) {
    REQUIRE_FOR(fn, limits, "null argument");
    limits[0] = WD_THREADS;
    limits[1] = WD_MAX_RUIZ;
    limits[2] = WD_ROWS_DEFAULT;
    limits[3] = WD_ROWS_MAX;
    return MLLP_OK;
}

static int wide_scratch_bytes(const char* fn, const mllp_graph_t* g, int64_t rows_per_item, bool rays, bool spec, int64_t* bytes) {
    REQUIRE_FOR(fn, g && bytes, "null argument");
    int64_t rows;
    if (int rc = wide_rows(fn, rows_per_item, &rows)) return rc;
    *bytes = call_words(g, rays, spec) * (int64_t)sizeof(float);
    return MLLP_OK;
}

extern "C" int mllp_lp_pdhg_wide_limits(int64_t* limits) { return wide_limits(__func__, limits); }
extern "C" int mllp_lp_pdhg_rays_limits(int64_t* limits) { return wide_limits(__func__, limits); }
extern "C" int mllp_lp_pdhg_spectral_limits(int64_t* limits) {
    if (int rc = wide_limits(__func__, limits)) return rc;
    limits[4] = WD_MAX_POWER;
    return MLLP_OK;
}

extern "C" int mllp_lp_pdhg_wide_scratch_bytes(const mllp_graph_t* g, int64_t rows_per_item, int64_t* bytes) {
    return wide_scratch_bytes(__func__, g, rows_per_item, false, false, bytes);
}
extern "C" int mllp_lp_pdhg_rays_scratch_bytes(const mllp_graph_t* g, int64_t rows_per_item, int64_t* bytes) {
    return wide_scratch_bytes(__func__, g, rows_per_item, true, false, bytes);
}
extern "C" int mllp_lp_pdhg_spectral_scratch_bytes(const mllp_graph_t* g, int64_t rows_per_item, int64_t* bytes) {
    return wide_scratch_bytes(__func__, g, rows_per_item, true, true, bytes);
}

extern "C" int mllp_lp_pdhg_wide(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0,
                                 int64_t iter_begin, int64_t iter_end, int64_t check_every, float eps, float step, float beta,
                                 int64_t ruiz_passes, int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect,
                                 int64_t rows_per_item, float* d_x, float* d_y, float* d_dr, float* d_dc, int32_t* d_status, float* d_kkt,
                                 void* d_scratch, void* stream) {
    return wide_call(__func__, g, d_x1, d_x2, d_x0, d_y0, iter_begin, iter_end, check_every, eps, step, beta, ruiz_passes, pock_chambolle,
                     primal_weight, weight_span, reflect, nullptr, nullptr, rows_per_item, d_x, d_y, d_dr, d_dc, d_status, d_kkt, d_scratch, stream);
}

extern "C" int mllp_lp_pdhg_rays(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0,
                                 int64_t iter_begin, int64_t iter_end, int64_t check_every, float eps, float step, float beta,
                                 int64_t ruiz_passes, int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect,
                                 float ray_eps, int64_t rows_per_item, float* d_x, float* d_y, float* d_dr, float* d_dc, float* d_ray_x,
                                 float* d_ray_y, int32_t* d_status, float* d_kkt, float* d_cert, void* d_scratch, void* stream) {
    const RayArgs rays{ray_eps, d_ray_x, d_ray_y, d_cert};
    return wide_call(__func__, g, d_x1, d_x2, d_x0, d_y0, iter_begin, iter_end, check_every, eps, step, beta, ruiz_passes, pock_chambolle,
                     primal_weight, weight_span, reflect, &rays, nullptr, rows_per_item, d_x, d_y, d_dr, d_dc, d_status, d_kkt, d_scratch, stream);
}

extern "C" int mllp_lp_pdhg_spectral(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_x0, const float* d_y0,
                                     int64_t iter_begin, int64_t iter_end, int64_t check_every, float eps, float step, float beta,
                                     int64_t ruiz_passes, int32_t pock_chambolle, int32_t primal_weight, float weight_span, int32_t reflect,
                                     float ray_eps, int64_t power_iters, int64_t rows_per_item, float* d_x, float* d_y, float* d_dr,
                                     float* d_dc, float* d_ray_x, float* d_ray_y, int32_t* d_status, float* d_kkt, float* d_cert,
                                     float* d_norm, void* d_scratch, void* stream) {
    const RayArgs rays{ray_eps, d_ray_x, d_ray_y, d_cert};
    const SpecArgs spec{power_iters, d_norm};
    return wide_call(__func__, g, d_x1, d_x2, d_x0, d_y0, iter_begin, iter_end, check_every, eps, step, beta, ruiz_passes, pock_chambolle,
                     primal_weight, weight_span, reflect, &rays, &spec, rows_per_item, d_x, d_y, d_dr, d_dc, d_status, d_kkt, d_scratch, stream);
}

