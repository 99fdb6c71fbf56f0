// select.hip -- the predicted basis itself (mllp_topm_select, mllp_topm_select_dense): per segment (instance) the
// m largest logits as a 0/1 mask, as an ascending index list, and the pair {threshold, runner-up}.
//
//   topm_select    one workgroup per segment.  The order and the tie rule are those of topm_metrics_kernel
//                  (node_kernels.hip): keys are orderable(logit) -- a total order over bit patterns, -0.0 < +0.0 --,
//                  the min(m, n) largest keys are selected, and among keys equal to the threshold the lowest indices
//                  win.  The threshold comes from the same 4-pass radix select (8 bits per pass); one ordered
//                  compaction pass over the 1024-thread chunks follows (wave ballots + a scan over the 16 wavefront
//                  counts), which gives every selected column its rank, so the index list is written in ascending
//                  order without a sort and without atomics on global memory.
//
// The select is a copy of the forty lines of the metrics kernel, not a shared header: that kernel is tuned and pinned by
// the profiles, and its device code stays byte for byte what it was.  The two traps recorded there hold here as well:
// the top byte's histogram is wave-aggregated (plain LDS atomics serialise 64 lanes on a handful of addresses), and the
// 256 bins are walked by four wavefronts, not by one thread.
//
// Every result is a function of the input alone: integer counts, keys mapped back to the float bits they came from, no
// float arithmetic at all, no dependence on launch or arrival order.
#include "internal.h"

namespace mllp {

__device__ __forceinline__ unsigned sel_key(float f) {          // = orderable() of node_kernels.hip
    const unsigned u = __float_as_uint(f);
    return (u & 0x80000000u) ? ~u : (u | 0x80000000u);
}
__device__ __forceinline__ float sel_unkey(unsigned k) {        // the float whose key is k, bit for bit
    return __uint_as_float((k & 0x80000000u) ? (k ^ 0x80000000u) : ~k);
}

constexpr int SEL_T = 1024, SEL_W = SEL_T / 64;

// ptr_n == nullptr: one segment of n_dense logits, m_dense to select, index list at offset 0
__global__ __launch_bounds__(SEL_T) void topm_select_kernel(const int* __restrict__ ptr_n, const int* __restrict__ ptr_m,
                                                            int n_dense, int m_dense, const float* __restrict__ logits,
                                                            unsigned char* __restrict__ mask_out,
                                                            int* __restrict__ index_out, float* __restrict__ stats) {
    __shared__ unsigned hist[256];
    __shared__ unsigned s_prefix, s_need, s_wtot[4];
    __shared__ unsigned s_cnt[2][SEL_W];
    __shared__ unsigned s_max[SEL_W];
    const int k = blockIdx.x, tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    int beg = 0, n = n_dense, m_slots = m_dense, slot0 = 0;
    if (ptr_n) {
        beg = ptr_n[k];
        n = ptr_n[k + 1] - beg;
        slot0 = ptr_m[k];
        m_slots = ptr_m[k + 1] - slot0;
    }
    const int m = min(m_slots, n);
    const float* z = logits + beg;
    unsigned char* mk = mask_out ? mask_out + beg : nullptr;
    int* ix = index_out ? index_out + slot0 : nullptr;
    if (ix)
        for (int j = max(m, 0) + tid; j < m_slots; j += SEL_T) ix[j] = -1;      // slots past min(m, n)

    unsigned thr = 0u, need_eq = 0u;
    if (m > 0) {
        if (tid == 0) { s_prefix = 0u; s_need = (unsigned)m; }
        unsigned kmask = 0u;
        for (int pass = 3; pass >= 0; --pass) {
            const int shift = pass * 8;
            if (tid < 256) hist[tid] = 0u;
            __syncthreads();
            const unsigned prefix = s_prefix, need = s_need;
            if (pass == 3) {
                // sign + 7 exponent bits: a handful of distinct values -- one LDS atomic per distinct bin of a wavefront
                for (int i0 = 0; i0 < n; i0 += SEL_T) {
                    const int i = i0 + tid;
                    const bool have = i < n;
                    const unsigned bin = have ? (sel_key(z[i]) >> 24) : 0u;
                    unsigned long long todo = __ballot(have);
                    while (todo) {
                        const int leader = __builtin_amdgcn_readfirstlane(__ffsll((long long)todo) - 1);
                        const unsigned b = (unsigned)__builtin_amdgcn_readlane((int)bin, leader);
                        const unsigned long long same = __ballot(have && bin == b) & todo;
                        if (lane == leader) atomicAdd(&hist[b], (unsigned)__popcll(same));
                        todo &= ~same;
                    }
                }
            } else {
                for (int i = tid; i < n; i += SEL_T) {
                    const unsigned key = sel_key(z[i]);
                    if ((key & kmask) == prefix) atomicAdd(&hist[(key >> shift) & 255u], 1u);
                }
            }
            __syncthreads();
            // the bin that holds the need-th largest key: suffix sums over the 256 bins in four wavefronts
            unsigned h = 0u, sfx = 0u;
            if (tid < 256) {
                h = hist[tid];
                sfx = h;
                for (int o = 1; o < 64; o <<= 1) {
                    const unsigned v = __shfl_down(sfx, o, 64);
                    if (lane + o < 64) sfx += v;
                }
                if (lane == 0) s_wtot[wave] = sfx;
            }
            __syncthreads();
            if (tid < 256) {
                unsigned above = 0u;
                for (int w = wave + 1; w < 4; ++w) above += s_wtot[w];
                const unsigned ge = sfx + above, gt = ge - h;      // keys of this prefix with bin >= tid / > tid
                if (ge >= need && gt < need) {                     // exactly one bin
                    s_need = need - gt;
                    s_prefix = prefix | ((unsigned)tid << shift);
                }
            }
            kmask |= 255u << shift;
            __syncthreads();
        }
        thr = s_prefix;
        need_eq = s_need;      // how many keys equal to thr belong to the selection (>= 1), the lowest indices first
    }

    // ordered compaction: a column is selected if key > thr, or key == thr and fewer than need_eq equal keys precede it.
    // Its rank in the index list = (# greater keys before it) + min(# equal keys before it, need_eq).  Per chunk of 1024
    // columns: two ballots per wavefront, the wavefront's two counts packed in one word (each <= 64, a chunk's <= 1024),
    // and every thread sums the 16 words.  s_cnt is double-buffered, so one barrier per chunk is enough: a wavefront
    // writes buffer p again only behind the next chunk's barrier, which it passes after its reads of this chunk.
    // With m <= 0 nothing is selected (thr / need_eq unused): the pass writes the zero mask and finds the largest key.
    unsigned run_gt = 0u, run_eq = 0u;
    unsigned best = 0u;            // largest key NOT selected that this thread has seen
    bool any_out = false;
    int par = 0;
    for (int base = 0; base < n; base += SEL_T, par ^= 1) {
        const int i = base + tid;
        const bool have = i < n;
        const unsigned key = have ? sel_key(z[i]) : 0u;
        const bool gt = have && m > 0 && key > thr, eq = have && m > 0 && key == thr;
        const unsigned long long bg = __ballot(gt), be = __ballot(eq);
        const unsigned long long below = (1ull << lane) - 1ull;
        if (lane == 0) s_cnt[par][wave] = (unsigned)__popcll(bg) | ((unsigned)__popcll(be) << 16);
        __syncthreads();
        unsigned off = 0u, total = 0u;
#pragma unroll
        for (int w = 0; w < SEL_W; ++w) {
            const unsigned c = s_cnt[par][w];
            if (w < wave) off += c;
            total += c;
        }
        const unsigned gt_before = run_gt + (off & 0xffffu) + (unsigned)__popcll(bg & below);
        const unsigned eq_before = run_eq + (off >> 16) + (unsigned)__popcll(be & below);
        const bool sel = gt || (eq && eq_before < need_eq);
        if (have) {
            if (mk) mk[i] = sel ? 1 : 0;
            if (sel) {
                if (ix) ix[gt_before + min(eq_before, need_eq)] = i;
            } else {
                best = any_out ? max(best, key) : key;
                any_out = true;
            }
        }
        run_gt += total & 0xffffu;
        run_eq += total >> 16;
    }
    if (!stats) return;
    // runner-up: the largest key not selected (none when m >= n).  Key 0 is a legal key, and the smallest: a thread
    // without an unselected column contributes 0, which cannot exceed the true maximum when one exists.
    for (int o = 32; o > 0; o >>= 1) best = max(best, (unsigned)__shfl_xor((int)best, o, 64));
    if (lane == 0) s_max[wave] = best;
    __syncthreads();
    if (tid == 0) {
        unsigned b = 0u;
        for (int w = 0; w < SEL_W; ++w) b = max(b, s_max[w]);
        const float ninf = __uint_as_float(0xff800000u), pinf = __uint_as_float(0x7f800000u);
        stats[2 * k] = m > 0 ? sel_unkey(thr) : pinf;
        stats[2 * k + 1] = n > max(m, 0) ? sel_unkey(b) : ninf;
    }
}

int launch_topm_select(const int* ptr_n, const int* ptr_m, int64_t n_seg, int n_dense, int m_dense, const float* logits,
                       unsigned char* mask, int* index, float* stats, hipStream_t s) {
    if (n_seg <= 0) return MLLP_OK;
    hipLaunchKernelGGL(topm_select_kernel, dim3((unsigned)n_seg), dim3(SEL_T), 0, s, ptr_n, ptr_m, n_dense, m_dense, logits,
                       mask, index, stats);
    hipError_t e = hipGetLastError();
    return e == hipSuccess ? MLLP_OK : hip_fail(e, "topm_select");
}

}  // namespace mllp
