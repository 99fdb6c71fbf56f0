// basis.hip -- a ranking of an instance's columns -> the best-ranked nonsingular basis and its basic solution
// (mllp_basis_repair; the rule is stated in include/mllp_hip.h, the design in DESIGN.md 4.13).
//
// One workgroup per instance.  The workgroup keeps the explicit transform T (m x m) of a Gauss-Jordan elimination with
// the rule's pivoting, such that T a is what is left of a column a after eliminating the accepted ones:
//   per candidate   w_i = sum_e a_e T[i][row_e] over the column's entries in CSR(A^T) order (ascending row), one thread per
//                   row i; amax = max |a_e|; {r, pivot row} = the largest |w_i| over the rows not yet pivoted, lowest row
//                   among equals -- ONE integer max over the keys {bits of |w_i|, ~i}, exact in any order.  One barrier.
//   on acceptance   row p of T is divided by w_p and staged (prow), then T[i][:] -= w_i prow for i != p.  Two more barriers.
//   at the end      x[col of row p] = sum_c T[p][c] b_c, c ascending, one thread per p;  y_c = sum_p T[p][c] cB_p, one
//                   wavefront per c: lane l adds p = l, l + 64, ... in that order, then the butterfly of group_sum<64>.
//
// T is COLUMN-MAJOR (element (i, c) at c * m + i): the w gather, the update and both final sums walk i with the lanes, so
// every access is coalesced (global) or conflict-free (LDS).  Column c of T is the unit vector e_c until row c is pivoted;
// such a column is never stored or read, so T needs no initialisation (nothing depends on what the storage held) and the
// update touches (rank + 1) x m elements, not m x m.  A column whose staged factor is exactly 0 and a row whose w_i is
// exactly 0 are left alone: they would be rewritten with the bits they hold.
//
// IN_LDS: T lives in LDS when m <= BASIS_LDS_MAX_M, in the caller's scratch otherwise -- the same code, instantiated twice,
// each with one address space for T.  The four vectors (w, prow, col of row, pivoted rows in order) are in LDS in both: they
// are read once per column of every update, and from global memory each of those reads is a round trip on the critical
// path (m = 1200: 331 ms with the vectors in scratch, 151 ms with them in LDS).  That bounds m by BASIS_MAX_M.
// No float atomics; every sum has an order that depends on the instance alone: the same bits alone and inside any batch.
#include <cmath>

#include "device_utils.h"
#include "internal.h"
#include "lp_launch.h"

namespace mllp {

namespace {

constexpr int BR_T_LDS = 256, BR_T_GLB = 1024;      // threads of a workgroup, T in LDS / in scratch
constexpr int BR_SKIPPED = 2, BR_BAD_ID = 3;
constexpr int BR_UNROLL = 4;

__device__ __forceinline__ unsigned long long wave_max_u64(unsigned long long v) {
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long u = (unsigned long long)__shfl_xor((long long)v, o, 64);
        v = u > v ? u : v;
    }
    return v;
}

struct RepairArgs {
    const int* __restrict__ ptr_m;
    const int* __restrict__ ptr_n;
    const int* __restrict__ at_ptr;     // CSR(A^T)
    const int* __restrict__ at_idx;
    const float* __restrict__ at_val;
    const float* __restrict__ c;
    const float* __restrict__ b;
    const int* __restrict__ order;
    float tol;
    long long max_m;
    float* basis;
    int* col_of_row;
    float* x;
    float* y;
    int* status;
    float* quality;
    float* scratch;
};

template <bool IN_LDS, int NT>
__global__ __launch_bounds__(NT) void basis_repair_kernel(const RepairArgs A) {
    constexpr int NW = NT / 64;
    extern __shared__ float br_lds[];
    __shared__ unsigned long long s_key[2][NW];
    __shared__ long long s_off[NW];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int row0 = A.ptr_m[k], m = A.ptr_m[k + 1] - row0;
    const int col0 = A.ptr_n[k], n = A.ptr_n[k + 1] - col0;
    if ((m <= BASIS_LDS_MAX_M) != IN_LDS) return;       // the other launch's instance
    const float inf = __builtin_huge_valf();
    // defaults of the column outputs; the accepted columns are written again behind at least one barrier
    for (int j = tid; j < n; j += NT) {
        if (A.basis) A.basis[col0 + j] = 0.0f;
        if (A.x) A.x[col0 + j] = 0.0f;
    }
    if ((long long)m > A.max_m) {
        for (int i = tid; i < m; i += NT) {
            if (A.col_of_row) A.col_of_row[row0 + i] = -1;
            if (A.y) A.y[row0 + i] = 0.0f;
        }
        if (tid == 0) {
            int* st = A.status + 4 * (size_t)k;
            st[0] = 0; st[1] = 0; st[2] = 0; st[3] = BR_SKIPPED;
            if (A.quality) { A.quality[2 * (size_t)k] = inf; A.quality[2 * (size_t)k + 1] = 0.0f; }
        }
        return;
    }
    float* T;                                       // [m][m] column-major
    float* w;                                       // [m] the candidate's eliminated column; c_B at the end
    if constexpr (IN_LDS) {
        T = br_lds;
        w = br_lds + (size_t)m * m;
    } else {
        // this instance's piece of the scratch: behind those of the earlier instances that take one (integer sum: exact)
        long long off = 0;
        for (int j = tid; j < k; j += NT) {
            const long long mj = A.ptr_m[j + 1] - A.ptr_m[j];
            if (mj > BASIS_LDS_MAX_M && mj <= A.max_m) off += basis_repair_words(mj);
        }
#pragma unroll
        for (int o = 1; o < 64; o <<= 1) off += __shfl_xor(off, o, 64);
        if (lane == 0) s_off[wave] = off;
        __syncthreads();
        off = 0;
#pragma unroll
        for (int v = 0; v < NW; ++v) off += s_off[v];
        T = A.scratch + off;
        w = br_lds;
    }
    float* prow = w + m;                            // [m] the staged pivot row, by position in piv
    int* crow = reinterpret_cast<int*>(prow + m);   // [m] local column whose pivot row this is, or -1
    int* piv = crow + m;                            // [m] the pivoted rows in order of acceptance
    for (int i = tid; i < m; i += NT) crow[i] = -1;
    __syncthreads();

    int rank = 0, examined = 0, rejected = 0, code = 1, par = 0;
    float qmin = inf, qmax = 0.0f;
    const int* ord = A.order + col0;
    for (int t = 0; t < n && rank < m; ++t) {
        const int j = ord[t];
        if (j < 0) break;
        if (j >= n) { code = BR_BAD_ID; break; }
        ++examined;
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
        best = wave_max_u64(best);
        if (lane == 0) s_key[par][wave] = best;
        __syncthreads();        // (also: every w_i is written)
        best = 0ull;
#pragma unroll
        for (int v = 0; v < NW; ++v) best = s_key[par][v] > best ? s_key[par][v] : best;
        par ^= 1;               // (this buffer is written again two candidates on: a barrier lies between)
        const float r = __uint_as_float((unsigned)(best >> 32));
        const int p = 0x7fffffff - (int)(unsigned)(best & 0xffffffffull);
        const float ratio = amax > 0.0f ? __fdiv_rn(r, amax) : 0.0f;
        if (!(amax > 0.0f && r > __fmul_rn(A.tol, amax))) {
            if (t < m) ++rejected;
            qmax = fmaxf(qmax, ratio);
            continue;           // (no barrier: nobody reads another thread's w_i of a rejected candidate)
        }
        qmin = fminf(qmin, ratio);
        const float wp = w[p];
        for (int q = tid; q <= rank; q += NT)
            prow[q] = q < rank ? __fdiv_rn(T[(size_t)piv[q] * m + p], wp) : __fdiv_rn(1.0f, wp);
        __syncthreads();
        for (int q = wave; q <= rank; q += NW) {    // a column per wavefront, the rows over its lanes
            const float pc = prow[q];
            const bool fresh = q == rank;           // column p was e_p until now
            if (!fresh && pc == 0.0f) continue;
            float* col = T + (size_t)(fresh ? p : piv[q]) * m;
            for (int i0 = lane; i0 < m; i0 += 64 * BR_UNROLL) {     // BR_UNROLL independent loads in flight per lane
                float tv[BR_UNROLL], wv[BR_UNROLL];
#pragma unroll
                for (int u = 0; u < BR_UNROLL; ++u) {
                    const int i = i0 + 64 * u;
                    wv[u] = i < m ? w[i] : 0.0f;
                    tv[u] = (i < m && !fresh) ? col[i] : 0.0f;
                }
#pragma unroll
                for (int u = 0; u < BR_UNROLL; ++u) {
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
    if (rank == m) code = 0;
    if (tid == 0) {
        int* st = A.status + 4 * (size_t)k;
        st[0] = rank; st[1] = examined; st[2] = rejected; st[3] = code;
        if (A.quality) { A.quality[2 * (size_t)k] = qmin; A.quality[2 * (size_t)k + 1] = qmax; }
    }
    for (int i = tid; i < m; i += NT) {
        const int j = crow[i];
        if (A.col_of_row) A.col_of_row[row0 + i] = j;
        if (A.basis && j >= 0) A.basis[col0 + j] = 1.0f;
    }
    if (!A.x) return;
    if (rank < m) {
        for (int i = tid; i < m; i += NT) A.y[row0 + i] = 0.0f;
        return;
    }
    for (int i = tid; i < m; i += NT) w[i] = A.c[col0 + crow[i]];
    __syncthreads();
    for (int p = tid; p < m; p += NT) {
        float acc = 0.0f;
#pragma unroll 8
        for (int cc = 0; cc < m; ++cc) acc = __fmaf_rn(T[(size_t)cc * m + p], A.b[row0 + cc], acc);
        A.x[col0 + crow[p]] = acc;
    }
    for (int cc = wave; cc < m; cc += NW) {
        const float* col = T + (size_t)cc * m;
        float acc = 0.0f;
        for (int p = lane; p < m; p += 64) acc = __fmaf_rn(col[p], w[p], acc);
        acc = group_sum<64>(acc);
        if (lane == 0) A.y[row0 + cc] = acc;
    }
}

LpPlan repair_plan(const mllp_graph_t* g, int64_t max_m) {
    max_m = std::min<int64_t>(max_m, BASIS_MAX_M);
    return lp_plan(g, [=](int64_t m, int64_t) {
        const bool in_lds = m <= BASIS_LDS_MAX_M;
        return LpInstance{in_lds, m <= max_m, in_lds ? 0 : basis_repair_words(m), m};
    });
}

}  // namespace

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_basis_repair_scratch_bytes(const mllp_graph_t* g, int64_t max_m, int64_t* bytes) {
    REQUIRE(g && bytes, "null argument");
    REQUIRE(max_m >= 0, "max_m must not be negative");
    *bytes = repair_plan(g, max_m).words * (int64_t)sizeof(float);
    return MLLP_OK;
}

extern "C" int mllp_basis_repair(const mllp_graph_t* g, const float* d_x1, const float* d_x2, const int32_t* d_order, float tol,
                                 int64_t max_m, float* d_basis, int32_t* d_col_of_row, float* d_x, float* d_y, int32_t* d_status,
                                 float* d_quality, void* d_scratch, void* stream) {
    REQUIRE(g && d_order && d_status, "null argument (g, d_order and d_status are required)");
    REQUIRE((d_x == nullptr) == (d_y == nullptr), "d_x and d_y come together");
    REQUIRE(!d_x || (d_x1 && d_x2), "null d_x1 or d_x2 with d_x and d_y asked for");
    REQUIRE(std::isfinite(tol) && tol >= 0.0f, "tol must be finite and not negative");
    REQUIRE(max_m >= 0, "max_m must not be negative");
    const LpPlan plan = repair_plan(g, max_m);
    REQUIRE(plan.words == 0 || d_scratch, "null d_scratch (mllp_basis_repair_scratch_bytes is not 0)");
    if (g->n_inst <= 0) return MLLP_OK;
    hipStream_t s = (hipStream_t)stream;
    max_m = std::min<int64_t>(max_m, BASIS_MAX_M);
    const RepairArgs args = {g->inst_ptr_m, g->inst_ptr_n, g->At.ptr, g->At.idx, g->At.val, d_x1, d_x2, d_order, tol, (long long)max_m,
                             d_basis, d_col_of_row, d_x, d_y, d_status, d_quality, static_cast<float*>(d_scratch)};
    // a launch's dynamic LDS, its largest instance having m rows: the four vectors, and T where it lives there
    constexpr auto lds = [](bool in_lds, int64_t m) { return lp_lds_bytes((in_lds ? m * m : 0) + basis_repair_vec_words(m)); };
    int rc = MLLP_OK;
    if (plan.any_lds)
        rc = lp_launch<basis_repair_kernel<true, BR_T_LDS>, BR_T_LDS>("basis_repair", " (LDS)", g->n_inst, lds(true, BASIS_LDS_MAX_M),
                                                                      lds(true, plan.lds_extent), s, args);
    if (!rc && plan.any_glb)
        rc = lp_launch<basis_repair_kernel<false, BR_T_GLB>, BR_T_GLB>("basis_repair", " (scratch)", g->n_inst, lds(false, BASIS_MAX_M),
                                                                       lds(false, plan.glb_extent), s, args);
    return rc;
}
