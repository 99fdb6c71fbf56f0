// simplex.hip -- a basis mask -> the optimal basis by dual, then primal simplex pivots on the explicit inverse
// (mllp_basis_simplex; the rule is stated in include/mllp_hip.h, the design in DESIGN.md 4.15).
//
// One workgroup per instance.  The start is factorized exactly as basis.hip does it (the same gather, keys, staged row and
// update, duplicated here so that basis_repair_kernel stays what it is); with rank m every column of T has been pivoted, so
// from then on T = B^-1 is a full m x m matrix, row i belonging to the basic column crow[i].  An iteration:
//   S1  g_B[i] = g[crow[i]];  x_B[p] = sum_c T[p][c] b_c, c ascending, a thread per p; stage D: the leaving row is the
//       integer min over {order key of x_B[p], p}.                                                             barrier
//   S2  y_c = sum_p T[p][c] g_B[p], a wavefront per c: lane l adds p = l, l + 64, ..., then group_sum<64>; stage D: rho =
//       row p of T, into the staged row's storage.                                                             barrier
//   S3  pricing, a thread per nonbasic column over its CSR(A^T) entries (ascending row): d_j = g_j - a_j.y and, stage D,
//       alpha_j = a_j.rho; the key {bits of the ratio | order key of d_j, j} reduced by wave shuffles, one LDS word per
//       wavefront.  No per-column array.                                                                       barrier
//   S4  w = T a_j, a thread per row (repair's gather); stage P: the ratio test, key {bits of max(x_B,i, 0) / w_i, i}.
//                                                                                                              barrier
//   S5  the staged row: row p of T (stage D: rho) divided by w_p.                                              barrier
//   S6  T[i][:] -= w_i * staged row for i != p, row p = the staged row: a column per wavefront, rows over the lanes; then
//       crow[p] = j, d_basis and the trace follow (one thread).                                                barrier
// Six barriers per pivot in either stage.  T is COLUMN-MAJOR (element (i, c) at c * m + i): S1, S4 and S6 walk i with the
// lanes.  IN_LDS: T in LDS up to SIMPLEX_LDS_MAX_M rows, in the caller's scratch above -- the same code, instantiated twice,
// each with one address space for T.  The six vectors are in LDS in both.  The shifts s [n] are in scratch: read once per
// iteration, coalesced.  Whether a column is basic is read from d_basis, which the kernel keeps current.
// No float atomics; every sum has an order that depends on the instance alone: the same bits alone and inside any batch.
//
// mllp_basis_simplex_guarded is the same kernel source, instantiated on its own argument struct, and the
// same host path.  In Bland mode -- after stall_pivots degenerate pivots of a stage, the same in every thread -- the
// reductions of S1, S3 and S4 take other keys ({basic column, row}, {column}, clipped ratios), and S4 of stage P a second
// reduction (the lowest basic column among the bit-equal smallest ratios: a seventh barrier, in that iteration only); after
// every refactor_every pivots the factorization of the start runs again on d_basis, in place.  All of that is compiled out of
// mllp_basis_simplex's instantiations.  One deliberate duplicate is left: those instantiations factorize the start by inline
// text, not through sx_factorize, because any function form of it changes their instruction streams.
#include <cmath>
#include <string>
#include <type_traits>

#include "device_utils.h"
#include "internal.h"
#include "lp_launch.h"

namespace mllp {

namespace {

constexpr int SX_T_LDS = 256, SX_T_GLB = 1024;      // threads of a workgroup, T in LDS / in scratch
constexpr int SX_UNROLL = 4;
constexpr int SX_OPTIMAL = 0, SX_SINGULAR = 1, SX_SKIPPED = 2, SX_BAD_MASK = 3, SX_INFEASIBLE = 4, SX_UNBOUNDED = 5, SX_LIMIT = 6,
              SX_REFACTOR = 7;      // (mllp_basis_simplex_guarded only)
constexpr unsigned long long SX_NONE = ~0ull;       // the key of an empty candidate set

__device__ __forceinline__ unsigned long long sx_wave_max(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = (unsigned long long)__shfl_xor((long long)v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}
__device__ __forceinline__ unsigned long long sx_wave_min(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = (unsigned long long)__shfl_xor((long long)v, o, 64);
        v = u < v ? u : v;
    }
    return v;
}
// min over the workgroup, the same word in every thread.  One barrier; `slot` [NW] is free again after the NEXT barrier.
template <int NW>
__device__ __forceinline__ unsigned long long sx_block_min(unsigned long long v, unsigned long long* slot) {
    v = sx_wave_min(v);
    if ((threadIdx.x & 63) == 0) slot[threadIdx.x >> 6] = v;
    __syncthreads();
    v = SX_NONE;
#pragma unroll
    for (int q = 0; q < NW; ++q) v = slot[q] < v ? slot[q] : v;
    return v;
}
// unsigned keys in the order of the floats (-0.0 below +0.0), and back
__device__ __forceinline__ unsigned sx_order_key(float d) {
    const unsigned u = __float_as_uint(d);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sx_key_value(unsigned k) {
    return __uint_as_float((k & 0x80000000u) ? (k & 0x7fffffffu) : ~k);
}

// The rule of mllp_basis_repair on a mask's columns in ascending order (basis.hip): T = B^-1 in place from an implicit
// identity, whatever T held, and the rank.  `mask` is the start, or d_basis at a refactorization, when x_B -- which
// piv aliases --, w and the staged row are dead.  crow [m]: the column whose row this is.  Every thread of the workgroup.
// (`mask` is not __restrict__: d_basis is written by this kernel between two calls.)
template <int NT>
__device__ __forceinline__ int sx_factorize(const float* mask, const int* __restrict__ at_ptr, const int* __restrict__ at_idx,
                                            const float* __restrict__ at_val, float tol, int row0, int col0, int m, int n, float* T,
                                            float* w, float* prow, int* crow, int* piv, unsigned long long (*s_fkey)[NT / 64]) {
    constexpr int NW = NT / 64;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    for (int i = tid; i < m; i += NT) crow[i] = -1;
    __syncthreads();
    int rank = 0, par = 0;
    for (int j = 0; j < n && rank < m; ++j) {
        if (mask[col0 + j] == 0.0f) continue;
        const int beg = at_ptr[col0 + j], end = at_ptr[col0 + j + 1];
        float amax = 0.0f;
        for (int e = beg; e < end; ++e) amax = fmaxf(amax, fabsf(at_val[e]));
        unsigned long long best = 0ull;             // (every row that is not pivoted has a key above 0)
        for (int i = tid; i < m; i += NT) {
            float acc = 0.0f;
            for (int e = beg; e < end; ++e) {
                const int r = at_idx[e] - row0;
                const float a = at_val[e];
                if (crow[r] >= 0) acc = __fmaf_rn(a, T[(size_t)r * m + i], acc);
                else if (r == i) acc = __fadd_rn(acc, a);
            }
            w[i] = acc;
            if (crow[i] < 0) {
                const unsigned long long key = ((unsigned long long)__float_as_uint(fabsf(acc)) << 32) | (unsigned)(0x7fffffff - i);
                best = key > best ? key : best;
            }
        }
        best = sx_wave_max(best);
        if (lane == 0) s_fkey[par][wave] = best;
        __syncthreads();        // (also: every w_i is written)
        best = 0ull;
#pragma unroll
        for (int v = 0; v < NW; ++v) best = s_fkey[par][v] > best ? s_fkey[par][v] : best;
        par ^= 1;               // (this buffer is written again two candidates on: a barrier lies between)
        const float r = __uint_as_float((unsigned)(best >> 32));
        const int p = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
        if (!(amax > 0.0f && r > __fmul_rn(tol, amax))) continue;     // (no barrier: nobody reads another thread's w_i)
        const float wp = w[p];
        for (int q = tid; q <= rank; q += NT)
            prow[q] = q < rank ? __fdiv_rn(T[(size_t)piv[q] * m + p], wp) : __fdiv_rn(1.0f, wp);
        __syncthreads();
        for (int q = wave; q <= rank; q += NW) {    // a column per wavefront, the rows over its lanes
            const float pc = prow[q];
            const bool fresh = q == rank;           // column p was e_p until now
            if (!fresh && pc == 0.0f) continue;
            float* col = T + (size_t)(fresh ? p : piv[q]) * m;
            for (int i0 = lane; i0 < m; i0 += 64 * SX_UNROLL) {
                float tv[SX_UNROLL], wv[SX_UNROLL];
#pragma unroll
                for (int u = 0; u < SX_UNROLL; ++u) {
                    const int i = i0 + 64 * u;
                    wv[u] = i < m ? w[i] : 0.0f;
                    tv[u] = (i < m && !fresh) ? col[i] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < SX_UNROLL; ++u) {
                    const int i = i0 + 64 * u;
                    if (i >= m) continue;
                    if (i == p) col[i] = pc;
                    else if (fresh || wv[u] != 0.0f) col[i] = __fmaf_rn(-wv[u], pc, tv[u]);
                }
            }
        }
        if (tid == 0) {
            piv[rank] = p;
            crow[p] = j;
        }
        ++rank;
        __syncthreads();
    }
    return rank;
}

struct SimplexArgs {
    const int* __restrict__ ptr_m;
    const int* __restrict__ ptr_n;
    const int* __restrict__ at_ptr;     // CSR(A^T)
    const int* __restrict__ at_idx;
    const float* __restrict__ at_val;
    const float* __restrict__ c;
    const float* __restrict__ b;
    const float* __restrict__ start;
    float tol, ftol, dtol, ptol, dshift;
    long long max_pivots, max_m;
    float* basis;
    int* col_of_row;
    int* trace;
    int* status;
    float* scratch;
};

// mllp_basis_simplex_guarded: the same, and the two guards
struct SimplexGuardedArgs : SimplexArgs {
    long long refactor_every, stall_pivots;
    int* guard;
};

// The one kernel of both entry points.  Args = SimplexGuardedArgs adds Bland's rule after stall_pivots degenerate pivots of a
// stage and a fresh factorization every refactor_every pivots; with Args = SimplexArgs every guard is
// discarded at compile time, and what is left is mllp_basis_simplex's rule.  A change meant for one entry point is held to
// leaving the other's instantiations instruction for instruction what they were (tools/kernel_streams.py).
template <bool IN_LDS, int NT, class Args>
__global__ __launch_bounds__(NT) void basis_simplex_kernel(const Args A) {
    constexpr bool G = std::is_same<Args, SimplexGuardedArgs>::value;
    constexpr int NW = NT / 64;
    extern __shared__ float sx_lds[];
    __shared__ unsigned long long s_fkey[2][NW];    // the factorization's pivot search
    __shared__ unsigned long long s_key[3][NW];     // leaving row (D), pricing, ratio test (P)
    __shared__ long long s_off[NW];
    __shared__ int s_cnt[NW];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = A.ptr_m[k], m = A.ptr_m[k + 1] - row0;
    const int col0 = A.ptr_n[k], n = A.ptr_n[k + 1] - col0;
    if ((m <= SIMPLEX_LDS_MAX_M) != IN_LDS) return;     // the other launch's instance
    int* st = A.status + 4 * (size_t)k;
    auto write_guard = [&](long long refactorizations, long long bland) {      // (one thread)
        if constexpr (G)
            if (A.guard) { A.guard[2 * (size_t)k] = (int)refactorizations; A.guard[2 * (size_t)k + 1] = (int)bland; }
    };
    // defaults of the outputs; a running instance writes them again behind at least one barrier
    for (int j = tid; j < n; j += NT) A.basis[col0 + j] = 0.0f;
    if (A.trace) {
        int* tr = A.trace + 2 * (size_t)k * (size_t)A.max_pivots;
        for (long long q = tid; q < 2 * A.max_pivots; q += NT) tr[q] = -1;
    }
    int count = 0;
    if ((long long)m <= A.max_m) {
        for (int j = tid; j < n; j += NT) count += A.start[col0 + j] != 0.0f;
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) count += __shfl_xor(count, o, 64);
        if (lane == 0) s_cnt[wave] = count;
        __syncthreads();
        count = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) count += s_cnt[v];
    }
    if ((long long)m > A.max_m || count != m) {
        for (int i = tid; i < m; i += NT)
            if (A.col_of_row) A.col_of_row[row0 + i] = -1;
        if (tid == 0) { st[0] = (long long)m > A.max_m ? SX_SKIPPED : SX_BAD_MASK; st[1] = 0; st[2] = 0; st[3] = 0; write_guard(0, 0); }
        return;
    }
    // this instance's piece of the scratch: behind those of the earlier instances that may run (integer sum: exact)
    long long off = 0;
    for (int j = tid; j < k; j += NT) {
        const long long mj = A.ptr_m[j + 1] - A.ptr_m[j], nj = A.ptr_n[j + 1] - A.ptr_n[j];
        if (mj <= A.max_m) off += simplex_words(mj, nj);
    }
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) off += __shfl_xor(off, o, 64);
    if (lane == 0) s_off[wave] = off;
    __syncthreads();
    off = 0;
#pragma unroll
    for (int v = 0; v < NW; ++v) off += s_off[v];
    float* T;                                       // [m][m] column-major
    float* w;                                       // [m] T a_j
    float* sh;                                      // [n] the shifts of stage D
    if constexpr (IN_LDS) {
        T = sx_lds;
        w = sx_lds + (size_t)m * m;
        sh = A.scratch + off;
    } else {
        T = A.scratch + off;
        w = sx_lds;
        sh = A.scratch + off + (size_t)m * m;
    }
    float* prow = w + m;                            // [m] the staged pivot row; rho (row p of T) before it in stage D
    int* crow = reinterpret_cast<int*>(prow + m);   // [m] local column whose row this is, or -1
    float* xB = reinterpret_cast<float*>(crow + m); // [m] T b
    int* piv = reinterpret_cast<int*>(xB);          //     (the factorization's pivoted rows in order, before there is an x_B)
    float* yv = xB + m;                             // [m] T' g_B
    float* gB = yv + m;                             // [m] the stage's costs of the basic columns
    // ---- the start: the rule of mllp_basis_repair on the mask's columns in ascending order (basis.hip) ----------------------
    int rank;
    if constexpr (G) {
        rank = sx_factorize<NT>(A.start, A.at_ptr, A.at_idx, A.at_val, A.tol, row0, col0, m, n, T, w, prow, crow, piv, s_fkey);
    } else {
        // sx_factorize's text once more, on purpose: with the start factorized through any function the plain instantiations
        // are scheduled and allocated differently from here on, and measured 2.4 % and 3.4 % slower.  The
        // one duplicate left in this file; a change to either copy goes into both.
        for (int i = tid; i < m; i += NT) crow[i] = -1;
        __syncthreads();
        rank = 0;
        int par = 0;
        for (int j = 0; j < n && rank < m; ++j) {
            if (A.start[col0 + j] == 0.0f) continue;
            const int beg = A.at_ptr[col0 + j], end = A.at_ptr[col0 + j + 1];
            float amax = 0.0f;
            for (int e = beg; e < end; ++e) amax = fmaxf(amax, fabsf(A.at_val[e]));
            unsigned long long best = 0ull;             // (every row that is not pivoted has a key above 0)
            for (int i = tid; i < m; i += NT) {
                float acc = 0.0f;
                for (int e = beg; e < end; ++e) {
                    const int r = A.at_idx[e] - row0;
                    const float a = A.at_val[e];
                    if (crow[r] >= 0) acc = __fmaf_rn(a, T[(size_t)r * m + i], acc);
                    else if (r == i) acc = __fadd_rn(acc, a);
                }
                w[i] = acc;
                if (crow[i] < 0) {
                    const unsigned long long key = ((unsigned long long)__float_as_uint(fabsf(acc)) << 32) | (unsigned)(0x7fffffff - i);
                    best = key > best ? key : best;
                }
            }
            best = sx_wave_max(best);
            if (lane == 0) s_fkey[par][wave] = best;
            __syncthreads();        // (also: every w_i is written)
            best = 0ull;
#pragma unroll
            for (int v = 0; v < NW; ++v) best = s_fkey[par][v] > best ? s_fkey[par][v] : best;
            par ^= 1;               // (this buffer is written again two candidates on: a barrier lies between)
            const float r = __uint_as_float((unsigned)(best >> 32));
            const int p = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
            if (!(amax > 0.0f && r > __fmul_rn(A.tol, amax))) continue;     // (no barrier: nobody reads another thread's w_i)
            const float wp = w[p];
            for (int q = tid; q <= rank; q += NT)
                prow[q] = q < rank ? __fdiv_rn(T[(size_t)piv[q] * m + p], wp) : __fdiv_rn(1.0f, wp);
            __syncthreads();
            for (int q = wave; q <= rank; q += NW) {    // a column per wavefront, the rows over its lanes
                const float pc = prow[q];
                const bool fresh = q == rank;           // column p was e_p until now
                if (!fresh && pc == 0.0f) continue;
                float* col = T + (size_t)(fresh ? p : piv[q]) * m;
                for (int i0 = lane; i0 < m; i0 += 64 * SX_UNROLL) {
                    float tv[SX_UNROLL], wv[SX_UNROLL];
#pragma unroll
                    for (int u = 0; u < SX_UNROLL; ++u) {
                        const int i = i0 + 64 * u;
                        wv[u] = i < m ? w[i] : 0.0f;
                        tv[u] = (i < m && !fresh) ? col[i] : 0.0f;
                    }
#pragma unroll
                    for (int u = 0; u < SX_UNROLL; ++u) {
                        const int i = i0 + 64 * u;
                        if (i >= m) continue;
                        if (i == p) col[i] = pc;
                        else if (fresh || wv[u] != 0.0f) col[i] = __fmaf_rn(-wv[u], pc, tv[u]);
                    }
                }
            }
            if (tid == 0) {
                piv[rank] = p;
                crow[p] = j;
            }
            ++rank;
            __syncthreads();
        }
    }
    if (rank < m) {
        for (int i = tid; i < m; i += NT)
            if (A.col_of_row) A.col_of_row[row0 + i] = -1;
        if (tid == 0) { st[0] = SX_SINGULAR; st[1] = 0; st[2] = 0; st[3] = rank; write_guard(0, 0); }
        return;
    }
    for (int i = tid; i < m; i += NT) A.basis[col0 + crow[i]] = 1.0f;

    // y = T' g_B: a wavefront per column of T
    auto dual = [&]() {
        for (int cc = wave; cc < m; cc += NW) {
            const float* col = T + (size_t)cc * m;
            float acc = 0.0f;
            for (int p = lane; p < m; p += 64) acc = __fmaf_rn(col[p], gB[p], acc);
            acc = group_sum<64>(acc);
            if (lane == 0) yv[cc] = acc;
        }
    };

    // ---- the shifts: s_j = max(0, dshift - d0_j) off the basis, 0 on it, d0 the reduced costs of c ------------------------
    for (int i = tid; i < m; i += NT) gB[i] = A.c[col0 + crow[i]];
    __syncthreads();            // (also: d_basis holds the start)
    dual();
    __syncthreads();
    for (int j = tid; j < n; j += NT) {
        float s = 0.0f;
        if (A.basis[col0 + j] == 0.0f) {
            float ay = 0.0f;
            for (int e = A.at_ptr[col0 + j]; e < A.at_ptr[col0 + j + 1]; ++e) ay = __fmaf_rn(A.at_val[e], yv[A.at_idx[e] - row0], ay);
            const float t = __fsub_rn(A.dshift, __fsub_rn(A.c[col0 + j], ay));
            s = t > 0.0f ? t : 0.0f;
        }
        sh[j] = s;
    }
    __syncthreads();

    // ---- the pivots ---------------------------------------------------------------------------------------------------------
    int stage = 0, code = SX_LIMIT;
    long long nD = 0, nP = 0;
    int* tr = A.trace ? A.trace + 2 * (size_t)k * (size_t)A.max_pivots : nullptr;
    // the consecutive degenerate pivots of the stage, the pivots until the next refactorization, the two counts
    long long stall = 0, until = 0, nRef = 0, nBl = 0;
    if constexpr (G) until = A.refactor_every;
    while (true) {
        bool bland = false;         // the same in every thread: a property of the instance; never, without the guards
        if constexpr (G) bland = A.stall_pivots > 0 && stall >= A.stall_pivots;
        // S1
        for (int i = tid; i < m; i += NT) {
            const int j = crow[i];
            const float g = A.c[col0 + j];
            gB[i] = stage == 0 ? __fadd_rn(g, sh[j]) : g;
        }
        unsigned long long best = SX_NONE;
        for (int p = tid; p < m; p += NT) {
            float acc = 0.0f;
#pragma unroll 8
            for (int cc = 0; cc < m; ++cc) acc = __fmaf_rn(T[(size_t)cc * m + p], A.b[row0 + cc], acc);
            xB[p] = acc;
            unsigned long long key = ((unsigned long long)sx_order_key(acc) << 32) | (unsigned)p;
            if (bland)              // Bland: the infeasible row whose basic column is lowest
                key = acc < -A.ftol ? ((unsigned long long)(unsigned)crow[p] << 32) | (unsigned)p : SX_NONE;
            best = key < best ? key : best;
        }
        int p = -1;
        if (stage == 0) {
            best = sx_block_min<NW>(best, s_key[0]);
            if (bland ? best == SX_NONE : (best == SX_NONE || !(sx_key_value((unsigned)(best >> 32)) < -A.ftol))) {
                stall = 0;
                stage = 1;          // primal feasible: stage D is over for good; S1 once more with the true costs
                continue;           // (nothing S1 writes is read before its barrier, and s_key[0] is not written again)
            }
            p = (int)(unsigned)(best & 0xffffffffull);
        } else {
            __syncthreads();
        }
        // S2
        dual();
        if (stage == 0)
            for (int cc = tid; cc < m; cc += NT) prow[cc] = T[(size_t)cc * m + p];
        __syncthreads();
        // S3
        best = SX_NONE;
        for (int j = tid; j < n; j += NT) {
            if (A.basis[col0 + j] != 0.0f) continue;
            const int beg = A.at_ptr[col0 + j], end = A.at_ptr[col0 + j + 1];
            float ay = 0.0f, ar = 0.0f;
            for (int e = beg; e < end; ++e) {
                const int r = A.at_idx[e] - row0;
                const float a = A.at_val[e];
                ay = __fmaf_rn(a, yv[r], ay);
                if (stage == 0) ar = __fmaf_rn(a, prow[r], ar);
            }
            float g = A.c[col0 + j];
            if (stage == 0) g = __fadd_rn(g, sh[j]);
            const float d = __fsub_rn(g, ay);
            unsigned long long key = SX_NONE;
            if (stage == 0) {
                // (Bland: every degenerate candidate ties at an exact 0, and the lowest j wins)
                if (ar < -A.ptol)
                    key = ((unsigned long long)__float_as_uint(__fdiv_rn(bland ? (d > A.dtol ? d : 0.0f) : (d > 0.0f ? d : 0.0f), -ar)) << 32) | (unsigned)j;
            } else {
                key = ((unsigned long long)sx_order_key(d) << 32) | (unsigned)j;
                if (bland)          // Bland: the lowest j that prices out
                    key = d < -A.dtol ? (unsigned long long)(unsigned)j : SX_NONE;
            }
            best = key < best ? key : best;
        }
        best = sx_block_min<NW>(best, s_key[1]);
        if (stage == 0 && best == SX_NONE) { code = SX_INFEASIBLE; break; }
        if (stage == 1 && (bland ? best == SX_NONE : (best == SX_NONE || !(sx_key_value((unsigned)(best >> 32)) < -A.dtol)))) { code = SX_OPTIMAL; break; }
        const int j = (int)(unsigned)(best & 0xffffffffull);
        // S4
        const int beg = A.at_ptr[col0 + j], end = A.at_ptr[col0 + j + 1];
        best = SX_NONE;
        for (int i = tid; i < m; i += NT) {
            float acc = 0.0f;
            for (int e = beg; e < end; ++e) acc = __fmaf_rn(A.at_val[e], T[(size_t)(A.at_idx[e] - row0) * m + i], acc);
            w[i] = acc;
            if (stage == 1 && acc > A.ptol) {
                const float x = xB[i];
                const unsigned long long key =
                    ((unsigned long long)__float_as_uint(__fdiv_rn(bland ? (x > A.ftol ? x : 0.0f) : (x > 0.0f ? x : 0.0f), acc)) << 32) | (unsigned)i;
                best = key < best ? key : best;
            }
        }
        if (stage == 1) {
            best = sx_block_min<NW>(best, s_key[2]);
            if (best == SX_NONE) { code = SX_UNBOUNDED; break; }
            p = (int)(unsigned)(best & 0xffffffffull);
            if (bland) {            // among the rows whose ratio has the smallest ratio's bits, the lowest basic column: one barrier more
                const unsigned bits = (unsigned)(best >> 32);
                best = SX_NONE;
                for (int i = tid; i < m; i += NT) {
                    const float wi = w[i], x = xB[i];
                    if (wi > A.ptol && __float_as_uint(__fdiv_rn(x > A.ftol ? x : 0.0f, wi)) == bits) {
                        const unsigned long long key = ((unsigned long long)(unsigned)crow[i] << 32) | (unsigned)i;
                        best = key < best ? key : best;
                    }
                }
                best = sx_block_min<NW>(best, s_fkey[0]);    // (the factorization's words: idle between factorizations)
                if (best != SX_NONE) p = (int)(unsigned)(best & 0xffffffffull);     // (the first pass's row is among them)
            }
        } else {
            __syncthreads();
        }
        if (nD + nP >= A.max_pivots) { code = SX_LIMIT; break; }
        bool degenerate = false;
        if constexpr (G)
            if (A.stall_pivots > 0) {
                if (stage == 1) {
                    degenerate = xB[p] <= A.ftol;
                } else {            // dtilde_j again, in pricing's order: the same bits
                    float ay = 0.0f;
                    for (int e = beg; e < end; ++e) ay = __fmaf_rn(A.at_val[e], yv[A.at_idx[e] - row0], ay);
                    degenerate = __fsub_rn(__fadd_rn(A.c[col0 + j], sh[j]), ay) <= A.dtol;
                }
            }
        // S5
        const float wp = w[p];
        for (int cc = tid; cc < m; cc += NT) prow[cc] = __fdiv_rn(stage == 0 ? prow[cc] : T[(size_t)cc * m + p], wp);
        __syncthreads();
        // S6
        for (int cc = wave; cc < m; cc += NW) {     // a column per wavefront, the rows over its lanes
            const float pc = prow[cc];
            if (pc == 0.0f) continue;               // (row p holds a zero here already; every other row keeps its bits)
            float* col = T + (size_t)cc * m;
            for (int i0 = lane; i0 < m; i0 += 64 * SX_UNROLL) {
                float tv[SX_UNROLL], wv[SX_UNROLL];
#pragma unroll
                for (int u = 0; u < SX_UNROLL; ++u) {
                    const int i = i0 + 64 * u;
                    wv[u] = i < m ? w[i] : 0.0f;
                    tv[u] = i < m ? col[i] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < SX_UNROLL; ++u) {
                    const int i = i0 + 64 * u;
                    if (i >= m) continue;
                    if (i == p) col[i] = pc;
                    else if (wv[u] != 0.0f) col[i] = __fmaf_rn(-wv[u], pc, tv[u]);
                }
            }
        }
        if (tid == 0) {
            A.basis[col0 + crow[p]] = 0.0f;
            A.basis[col0 + j] = 1.0f;
            crow[p] = j;
            if (tr) { tr[2 * (nD + nP)] = j; tr[2 * (nD + nP) + 1] = p; }
        }
        if (stage == 0) ++nD;
        else ++nP;
        __syncthreads();
        if constexpr (G) {
            stall = degenerate ? stall + 1 : 0;
            nBl += bland;
            if (A.refactor_every > 0 && --until == 0) {
                // discard T: the current basis, factorized as the start was (x_B, w and the staged row are dead here)
                until = A.refactor_every;
                if (sx_factorize<NT>(A.basis, A.at_ptr, A.at_idx, A.at_val, A.tol, row0, col0, m, n, T, w, prow, crow, piv, s_fkey) < m) { code = SX_REFACTOR; break; }
                ++nRef;
            }
        }
    }
    for (int i = tid; i < m; i += NT)
        if (A.col_of_row) A.col_of_row[row0 + i] = (G && code == SX_REFACTOR) ? -1 : crow[i];
    if (tid == 0) { st[0] = code; st[1] = (int)nD; st[2] = (int)nP; st[3] = m; write_guard(nRef, nBl); }
}

LpPlan simplex_plan(const mllp_graph_t* g, int64_t max_m) {
    max_m = std::min<int64_t>(max_m, SIMPLEX_MAX_M);
    return lp_plan(g, [=](int64_t m, int64_t n) { return LpInstance{m <= SIMPLEX_LDS_MAX_M, m <= max_m, simplex_words(m, n), m}; });
}

// The checks that both entry points make first, and the arguments that both kernels take.
int simplex_args(const char* fn, const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_start, float tol, float ftol,
                 float dtol, float ptol, float dshift, int64_t max_pivots, int64_t max_m, float* d_basis, int32_t* d_col_of_row,
                 int32_t* d_trace, int32_t* d_status, void* d_scratch, SimplexArgs* args) {
    REQUIRE_FOR(fn, g && d_x1 && d_x2 && d_start && d_basis && d_status,
                "null argument (g, d_x1, d_x2, d_start, d_basis and d_status are required)");
    REQUIRE_FOR(fn, std::isfinite(tol) && tol >= 0.0f, "tol must be finite and not negative");
    REQUIRE_FOR(fn, std::isfinite(ftol) && ftol > 0.0f && std::isfinite(dtol) && dtol > 0.0f && std::isfinite(ptol) && ptol > 0.0f &&
                        std::isfinite(dshift) && dshift > 0.0f,
                "ftol, dtol, ptol and dshift must be finite and positive");
    REQUIRE_FOR(fn, max_pivots >= 0, "max_pivots must not be negative");
    REQUIRE_FOR(fn, max_m >= 0, "max_m must not be negative");
    *args = {g->inst_ptr_m, g->inst_ptr_n, g->At.ptr, g->At.idx, g->At.val, d_x1, d_x2, d_start, tol, ftol, dtol, ptol, dshift,
             (long long)max_pivots, (long long)std::min<int64_t>(max_m, SIMPLEX_MAX_M), d_basis, d_col_of_row, d_trace, d_status,
             static_cast<float*>(d_scratch)};
    return MLLP_OK;
}

// The rest of a call, after the entry point's own checks: the plan, the scratch check, and a launch per address space of T
// that has an instance.
template <class Args>
int simplex_launch(const char* fn, const mllp_graph_t* g, const Args& args, void* stream) {
    const LpPlan plan = simplex_plan(g, args.max_m);
    REQUIRE_FOR(fn, plan.words == 0 || args.scratch, "null d_scratch (mllp_basis_simplex_scratch_bytes is not 0)");
    if (g->n_inst <= 0) return MLLP_OK;
    hipStream_t s = (hipStream_t)stream;
    const std::string name = fn + sizeof("mllp_") - 1;
    // a launch's dynamic LDS, its largest instance having m rows: the six vectors, and T where it lives there
    constexpr auto lds = [](bool in_lds, int64_t m) { return lp_lds_bytes((in_lds ? m * m : 0) + simplex_vec_words(m)); };
    int rc = MLLP_OK;
    if (plan.any_lds)
        rc = lp_launch<basis_simplex_kernel<true, SX_T_LDS, Args>, SX_T_LDS>(name, " (LDS)", g->n_inst, lds(true, SIMPLEX_LDS_MAX_M),
                                                                             lds(true, plan.lds_extent), s, args);
    if (!rc && plan.any_glb)
        rc = lp_launch<basis_simplex_kernel<false, SX_T_GLB, Args>, SX_T_GLB>(name, " (scratch)", g->n_inst, lds(false, SIMPLEX_MAX_M),
                                                                              lds(false, plan.glb_extent), s, args);
    return rc;
}

}  // namespace

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_basis_simplex_scratch_bytes(const mllp_graph_t* g, int64_t max_m, int64_t* bytes) {
    REQUIRE(g && bytes, "null argument");
    REQUIRE(max_m >= 0, "max_m must not be negative");
    *bytes = simplex_plan(g, max_m).words * (int64_t)sizeof(float);
    return MLLP_OK;
}

extern "C" int mllp_basis_simplex(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_start, float tol,
                                  float ftol, float dtol, float ptol, float dshift, int64_t max_pivots, int64_t max_m,
                                  float* d_basis, int32_t* d_col_of_row, int32_t* d_trace, int32_t* d_status, void* d_scratch,
                                  void* stream) {
    SimplexArgs args;
    if (int rc = simplex_args(__func__, g, d_x1, d_x2, d_start, tol, ftol, dtol, ptol, dshift, max_pivots, max_m, d_basis, d_col_of_row,
                              d_trace, d_status, d_scratch, &args))
        return rc;
    return simplex_launch(__func__, g, args, stream);
}

extern "C" int mllp_basis_simplex_guarded(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const float* d_start,
                                          float tol, float ftol, float dtol, float ptol, float dshift, int64_t max_pivots,
                                          int64_t max_m, int64_t refactor_every, int64_t stall_pivots, float* d_basis,
                                          int32_t* d_col_of_row, int32_t* d_trace, int32_t* d_status, int32_t* d_guard,
                                          void* d_scratch, void* stream) {
    SimplexGuardedArgs args;
    if (int rc = simplex_args(__func__, g, d_x1, d_x2, d_start, tol, ftol, dtol, ptol, dshift, max_pivots, max_m, d_basis, d_col_of_row,
                              d_trace, d_status, d_scratch, &args))
        return rc;
    REQUIRE(refactor_every >= 0 && stall_pivots >= 0, "refactor_every and stall_pivots must not be negative");
    args.refactor_every = (long long)refactor_every;
    args.stall_pivots = (long long)stall_pivots;
    args.guard = d_guard;
    return simplex_launch(__func__, g, args, stream);
}
