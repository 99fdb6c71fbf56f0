// topm_loss.hip -- the soft top-m loss head (mllp_topm_loss, mllp_topm_loss_limits, mllp_topm_loss_math,
// mllp_gnn_loss_step_topm): probabilities that sum to m_k per instance, and the weighted BCE of weighted_loss.hip taken at
// them.  Reference: the commented-out gumbel_sinkhorn_topk(latent_vars, len(constrs), ..., return_prob=True) of
// linear_program_experiment.py:126-137 and the lml projection it imports; the fixed point of that 2 x n transport problem
// is p_i = sigma(a_i + nu) with sum_i p_i = m (include/mllp_hip.h states the rule in full).
//
//   topm_loss_kernel        one workgroup of 1024 threads per instance; per evaluation: one pass for min / max / mean of a,
//                           one pass per root iteration (sum p, sum p (1 - p)), one pass for the four sums at the root, one
//                           for dz.  Where a_i lives between the passes is picked by n_k alone (internal.h: in LDS up to
//                           16384 columns, formed again from the logits in every pass beyond).  S noisy evaluations run in
//                           turn in the instance's workgroup; dz accumulates in d_dlogits (each word has one thread).
//   topm_loss_total_kernel  loss = sum_k w_k L_k in instance order (the order of weighted_loss_total_kernel)
//
// Every sum is ordered_sum.h's with all 1024 threads as the lanes: thread t adds terms t, t + 1024, ... from 0, then the
// butterfly, then the tree over the sixteen wavefronts: the order depends on n_k alone.  nu, the bracket and the iteration
// count come from those sums, so they are the same bits in every thread and every barrier is uniform.  No atomics.
#include <math.h>

#include "ordered_sum.h"

namespace mllp {

namespace {

constexpr int TL_T = TOPM_LOSS_T, TL_W = TL_T / 64;
constexpr int TL_TOTAL_T = 256;

__device__ __forceinline__ uint32_t tl_mix(uint32_t x) {
    x ^= x >> 16;
    x *= 0x7feb352du;
    x ^= x >> 15;
    x *= 0x846ca68bu;
    x ^= x >> 16;
    return x;
}

// the Gumbel perturbation of local column i in sample s; base = mix(seed ^ id_k * 0x9E3779B9)
__device__ __forceinline__ float tl_gumbel(uint32_t base, uint32_t i, uint32_t s) {
    const uint32_t h = tl_mix(tl_mix(base + i) + s * 0x85EBCA6Bu);
    const float t = ((float)(h >> 9) + 0.5f) * 0x1p-23f;        // exact, in (0, 1)
    return -logf(-logf(t));
}

// a_i of one evaluation from the logits: (z_i + sigma eps_i) / tau, or z_i / tau without noise
struct TlSrc {
    const float* z;      // the instance's first logit
    float tau, sigma;
    uint32_t base, sample;
    bool noisy;
    __device__ __forceinline__ float operator()(int i) const {
        const float zi = z[i];
        return __fdiv_rn(noisy ? __fadd_rn(zi, __fmul_rn(sigma, tl_gumbel(base, (uint32_t)i, sample))) : zi, tau);
    }
};

// the columns of a thread between the passes: column threadIdx.x + j * 1024 in LDS word threadIdx.x + j * 1024, which no
// other thread touches (no barrier, no bank conflict), or (LDS = false) nothing kept and a_i formed again in every pass
template <bool LDS>
struct TlCols {
    float* a;
    __device__ __forceinline__ void fill(int n, const TlSrc& src) {
        for (int i = threadIdx.x; i < n; i += TL_T) a[i] = src(i);
    }
    template <class F>
    __device__ __forceinline__ void each(int n, const TlSrc&, F f) const {
        for (int i = threadIdx.x; i < n; i += TL_T) f(i, a[i]);
    }
};
template <>
struct TlCols<false> {
    float* a;
    __device__ __forceinline__ void fill(int, const TlSrc&) {}
    template <class F>
    __device__ __forceinline__ void each(int n, const TlSrc& src, F f) const {
        for (int64_t i = threadIdx.x; i < n; i += TL_T) f((int)i, src((int)i));      // (64 bits: i + 1024 may pass 2^31)
    }
};

// p = sigma(u) and 1 - p = sigma(-u), both formed directly from e = exp(-|u|) <= 1 (weighted_loss.hip)
struct TlSig {
    float p, pm, e;
};
__device__ __forceinline__ TlSig tl_sigmoid(float u) {
    const float e = expf(-fabsf(u));
    const float big = __fdiv_rn(1.0f, 1.0f + e), small = __fdiv_rn(e, 1.0f + e);
    return u >= 0.0f ? TlSig{big, small, e} : TlSig{small, big, e};
}

// min and max over the workgroup, in every thread (exact, so any order)
__device__ __forceinline__ Sum2 tl_block_minmax(float lo, float hi, Sum2* part) {
    lo = group_min<64>(lo);
    hi = group_max<64>(hi);
    if ((threadIdx.x & 63) == 0) part[threadIdx.x >> 6] = {lo, hi};
    __syncthreads();
#pragma unroll
    for (int w = 0; w < TL_W; ++w) {
        lo = fminf(lo, part[w].a);
        hi = fmaxf(hi, part[w].b);
    }
    __syncthreads();
    return {lo, hi};
}

struct TlEval {
    float nu, Q, resid, L;
    int iters;
};

// One evaluation of the head on an instance with 0 < m < n.  Every thread returns the same TlEval.
//   y, pwm1: labels of the instance and pw_k - 1 (for L and dz);  prob: p written when given
//   dz: when given, dz_e = wt (g'_i - q_i G' / Q), wt = w_k / (tau n_k), written (sample 0), else added to what the word
//   holds; the last of S > 1 samples divides by S
template <bool LDS>
__device__ __forceinline__ TlEval tl_eval(int n, int m, const TlSrc& src, const float* __restrict__ y, float pwm1, float wt,
                                          float* dz, int sample, int n_samples, float* __restrict__ prob, Sum2* part,
                                          float* seg) {
    TlCols<LDS> cols{seg};
    cols.fill(n, src);
    const float nf = (float)n, mf = (float)m;
    // the bracket: F(c0 - max a) <= 0 <= F(c0 - min a) with c0 = logit(m / n); the start: c0 - mean a
    float amin = INFINITY, amax = -INFINITY, asum = 0.0f;
    cols.each(n, src, [&](int, float a) {
        amin = fminf(amin, a);
        amax = fmaxf(amax, a);
        asum = __fadd_rn(asum, a);
    });
    const Sum2 mm = tl_block_minmax(amin, amax, part);
    const float mean = __fdiv_rn(block_tree_sum<TL_W>(asum, &part[0].a), nf);
    const float c0 = logf(__fdiv_rn(mf, (float)(n - m)));
    float lo = c0 - mm.b, hi = c0 - mm.a;
    float nu = fminf(fmaxf(c0 - mean, lo), hi);
    TlEval r{};
    for (int it = 1; it <= TOPM_LOSS_MAX_ITER; ++it) {
        Sum2 acc{0.0f, 0.0f};
        cols.each(n, src, [&](int, float a) {
            const TlSig s = tl_sigmoid(a + nu);
            acc = ordered_add(acc, Sum2{s.p, s.p * s.pm});
        });
        const Sum2 t = block_tree_sum<TL_W>(acc, part);
        const float F = t.a - mf, Q = t.b;
        r.iters = it;
        if (F == 0.0f) break;
        if (F < 0.0f) lo = nu;
        else hi = nu;
        if (hi <= nextafterf(nextafterf(lo, INFINITY), INFINITY)) break;
        float next = nu - __fdiv_rn(F, Q);
        const bool newton = Q > 0.0f && next > lo && next < hi;       // (a NaN or an infinite step fails the comparisons)
        if (!newton) next = 0.5f * lo + 0.5f * hi;
        const bool done = newton && fabsf(next - nu) <= 0x1p-12f;     // (what Newton leaves is below step^2 / 2 = 2^-25)
        nu = next;
        if (done) break;
    }
    r.nu = nu;
    // the sums at the root: sum p, Q; sum l, G' = sum g'
    Sum2 pq{0.0f, 0.0f}, lg{0.0f, 0.0f};
    cols.each(n, src, [&](int i, float a) {
        const float u = a + nu, yi = y[i];
        const TlSig s = tl_sigmoid(u);
        const float c = 1.0f + pwm1 * yi, omy = 1.0f - yi;
        const float sp = fmaxf(-u, 0.0f) + log1pf(s.e);
        pq = ordered_add(pq, Sum2{s.p, s.p * s.pm});
        lg = ordered_add(lg, Sum2{omy * u + c * sp, omy - c * s.pm});
        if (prob) prob[i] = s.p;
    });
    pq = block_tree_sum<TL_W>(pq, part);
    lg = block_tree_sum<TL_W>(lg, part);
    r.Q = pq.b;
    r.resid = pq.a - mf;
    r.L = __fdiv_rn(lg.a, nf);
    if (dz) {
        const float ratio = pq.b > 0.0f ? __fdiv_rn(lg.b, pq.b) : 0.0f;      // (Q = 0: every q_i is 0)
        const bool add = sample > 0, mean_now = n_samples > 1 && sample == n_samples - 1;
        const float sf = (float)n_samples;
        cols.each(n, src, [&](int i, float a) {
            const float yi = y[i];
            const TlSig s = tl_sigmoid(a + nu);
            const float c = 1.0f + pwm1 * yi, omy = 1.0f - yi;
            float v = wt * ((omy - c * s.pm) - (s.p * s.pm) * ratio);
            if (add) v = __fadd_rn(dz[i], v);             // (the word is this thread's own in every sample)
            dz[i] = mean_now ? __fdiv_rn(v, sf) : v;
        });
    }
    return r;
}

struct TlArgs {
    const int *ptr_n, *ptr_m;
    int n_inst, serial;
    const float *z, *y, *inst_w, *pos_w;
    const int* inst_id;
    float tau, sigma;
    int n_samples;
    uint32_t seed;
    float *dz, *inst_loss, *loss, *prob, *info;
};

// L_k of instance k in every thread; dz, prob and info[k] written on the way
template <bool LDS>
__device__ __forceinline__ float tl_instance(const TlArgs& A, int k, int beg, int n, int m, Sum2* part, float* seg) {
    const float w = A.inst_w ? A.inst_w[k] : 1.0f, pw = A.pos_w ? A.pos_w[k] : 1.0f;
    const uint32_t id = A.inst_id ? (uint32_t)A.inst_id[k] : (uint32_t)k;
    TlSrc src{A.z + beg, A.tau, A.sigma, tl_mix(A.seed ^ (id * 0x9E3779B9u)), 0u, false};
    const float* y = A.y + beg;
    float* dz = A.dz ? A.dz + beg : nullptr;
    float* prob = A.prob ? A.prob + beg : nullptr;
    const float wt = __fdiv_rn(__fdiv_rn(w, A.tau), (float)n);
    // S = 0: one evaluation without noise, which writes everything.  S >= 1: S noisy ones for L and dz, then (when p or
    // info is wanted) a noise-free one that writes p alone
    const int S = A.n_samples, n_eval = S == 0 ? 1 : S + ((prob || A.info) ? 1 : 0);
    float acc = 0.0f;
    int iters = 0;
    TlEval e{};
    for (int s = 0; s < n_eval; ++s) {
        src.noisy = s < S;
        src.sample = (uint32_t)s;
        e = tl_eval<LDS>(n, m, src, y, pw - 1.0f, wt, (S == 0 || s < S) ? dz : nullptr, s, S, src.noisy ? nullptr : prob, part, seg);
        if (S == 0 || s < S) acc = __fadd_rn(acc, e.L);
        iters = max(iters, e.iters);
    }
    const float L = S > 0 ? __fdiv_rn(acc, (float)S) : acc;
    if (A.info && threadIdx.x == 0) {
        float* o = A.info + 4 * (int64_t)k;
        o[0] = e.nu;
        o[1] = e.Q;
        o[2] = e.resid;
        o[3] = (float)iters;
    }
    return L;
}

// serial == 0: workgroup k takes instance k.  serial != 0 (loss wanted without a place for the L_k): ONE workgroup takes
// the instances in turn and adds the loss as topm_loss_total_kernel does.
__global__ __launch_bounds__(TL_T) void topm_loss_kernel(const TlArgs A) {
    __shared__ Sum2 part[TL_W];
    __shared__ float seg[TOPM_LOSS_LDS_MAX];
    const int k0 = A.serial ? 0 : (int)blockIdx.x, k1 = A.serial ? A.n_inst : k0 + 1;
    float total = 0.0f;
    for (int k = k0; k < k1; ++k) {
        const int beg = A.ptr_n[k], n = A.ptr_n[k + 1] - beg, m = A.ptr_m[k + 1] - A.ptr_m[k];
        float L = 0.0f;
        if (m <= 0 || m >= n) {                               // no root: L = 0, dz = 0, p = 0 (m = 0) or 1
            const float p = m > 0 ? 1.0f : 0.0f;
            for (int64_t i = threadIdx.x; i < n; i += TL_T) {
                if (A.dz) A.dz[beg + i] = 0.0f;
                if (A.prob) A.prob[beg + i] = p;
            }
            if (A.info && threadIdx.x == 0) {
                float* o = A.info + 4 * (int64_t)k;
                o[0] = 0.0f;
                o[1] = 0.0f;
                o[2] = m > 0 ? (float)(n - m) : 0.0f;         // (sum p - m_k with these p)
                o[3] = -1.0f;
            }
        } else if (n <= TOPM_LOSS_LDS_MAX) {
            L = tl_instance<true>(A, k, beg, n, m, part, seg);
        } else {
            L = tl_instance<false>(A, k, beg, n, m, part, seg);
        }
        if (threadIdx.x == 0 && A.inst_loss) A.inst_loss[k] = L;
        total = __fadd_rn(total, __fmul_rn(A.inst_w ? A.inst_w[k] : 1.0f, L));
    }
    if (A.serial && threadIdx.x == 0) A.loss[0] = total;
}

__global__ __launch_bounds__(TL_TOTAL_T) void topm_loss_total_kernel(const float* __restrict__ inst_loss,
                                                                     const float* __restrict__ inst_w, int n_inst,
                                                                     float* __restrict__ loss) {
    __shared__ float prod[TL_TOTAL_T];
    float total = 0.0f;
    for (int base = 0; base < n_inst; base += TL_TOTAL_T) {
        const int k = base + (int)threadIdx.x;
        if (k < n_inst) prod[threadIdx.x] = __fmul_rn(inst_w ? inst_w[k] : 1.0f, inst_loss[k]);
        __syncthreads();
        if (threadIdx.x == 0) {
            const int m = min(TL_TOTAL_T, n_inst - base);
            for (int j = 0; j < m; ++j) total = __fadd_rn(total, prod[j]);
        }
        __syncthreads();
    }
    if (threadIdx.x == 0) loss[0] = total;
}

// the three library functions the head's error bound rests on, as this translation unit compiles them
__global__ __launch_bounds__(256) void topm_loss_math_kernel(int which, int64_t n, const float* __restrict__ x,
                                                             float* __restrict__ out) {
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const float v = x[i];
    out[i] = which == 0 ? expf(v) : which == 1 ? log1pf(v) : logf(v);
}

int topm_loss_check(float tau, float sigma, int64_t n_samples, const char* fn) {
    if (!(std::isfinite(tau) && tau > 0.0f)) return fail(MLLP_EINVAL, std::string(fn) + ": tau must be finite and > 0");
    if (!(std::isfinite(sigma) && sigma >= 0.0f)) return fail(MLLP_EINVAL, std::string(fn) + ": sigma must be finite and >= 0");
    if (n_samples < 0 || n_samples > (1 << 20)) return fail(MLLP_EINVAL, std::string(fn) + ": n_samples must be in [0, 2^20]");
    return MLLP_OK;
}

}  // namespace

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_topm_loss_limits(int64_t* limits) {
    REQUIRE(limits, "null argument");
    limits[0] = TOPM_LOSS_LDS_MAX;
    limits[1] = TOPM_LOSS_T;
    return MLLP_OK;
}

extern "C" int mllp_topm_loss(const mllp_graph_t* g, const float* d_logits, const float* d_labels, const float* d_inst_weight,
                              const float* d_pos_weight, const int32_t* d_inst_id, float tau, float sigma, int64_t n_samples,
                              uint32_t seed, float* d_dlogits, float* d_inst_loss, float* d_loss, float* d_prob, float* d_info,
                              void* stream) {
    REQUIRE(g && d_logits && d_labels, "null argument");
    REQUIRE(d_dlogits || d_inst_loss || d_loss || d_prob || d_info,
            "null outputs: at least one of dlogits, inst_loss, loss, prob, info");
    if (int rc = topm_loss_check(tau, sigma, n_samples, __func__)) return rc;
    hipStream_t s = (hipStream_t)stream;
    const int n_inst = (int)g->n_inst;
    const bool serial = d_loss && !d_inst_loss;
    TlArgs A{g->inst_ptr_n, g->inst_ptr_m, n_inst, serial ? 1 : 0, d_logits, d_labels, d_inst_weight, d_pos_weight, d_inst_id,
             tau, sigma, (int)n_samples, seed, d_dlogits, d_inst_loss, serial ? d_loss : nullptr, d_prob, d_info};
    if (serial) {
        hipLaunchKernelGGL(topm_loss_kernel, dim3(1), dim3(TL_T), 0, s, A);
        return check_launch("topm_loss (serial)");
    }
    if (n_inst > 0) {
        hipLaunchKernelGGL(topm_loss_kernel, dim3((unsigned)n_inst), dim3(TL_T), 0, s, A);
        if (int rc = check_launch("topm_loss")) return rc;
    }
    if (!d_loss) return MLLP_OK;
    hipLaunchKernelGGL(topm_loss_total_kernel, dim3(1), dim3(TL_TOTAL_T), 0, s, d_inst_loss, d_inst_weight, n_inst, d_loss);
    return check_launch("topm_loss total");
}

extern "C" int mllp_topm_loss_math(int which, int64_t n, const float* d_x, float* d_y, void* stream) {
    REQUIRE(d_x && d_y, "null argument");
    REQUIRE(which >= 0 && which <= 2, "which: 0 expf, 1 log1pf, 2 logf");
    REQUIRE(n >= 0 && n < (int64_t(1) << 31), "bad size");
    if (n == 0) return MLLP_OK;
    hipLaunchKernelGGL(topm_loss_math_kernel, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, (hipStream_t)stream, which, n,
                       d_x, d_y);
    return check_launch("topm_loss_math");
}

// mllp_gnn_forward, the head above, mllp_gnn_backward: the public calls themselves, so the workspace record is exactly what
// a caller of the two would leave (mllp_gnn_input_grads may follow)
extern "C" int mllp_gnn_loss_step_topm(const mllp_graph_t* g, const float* d_params, const float* d_x1, const float* d_x2,
                                       const float* d_labels, const float* d_inst_weight, const float* d_pos_weight,
                                       const int32_t* d_inst_id, float tau, float sigma, int64_t n_samples, uint32_t seed,
                                       void* d_ws, float* d_logits, float* d_loss, float* d_inst_loss, float* d_grads,
                                       float* d_dlogits, void* stream) {
    REQUIRE(g && d_params && d_x1 && d_x2 && d_labels && d_ws && d_logits && d_grads, "null argument");
    REQUIRE(((reinterpret_cast<uintptr_t>(d_ws) | reinterpret_cast<uintptr_t>(d_params) | reinterpret_cast<uintptr_t>(d_x1) |
              reinterpret_cast<uintptr_t>(d_x2)) & 15) == 0,
            "misaligned pointer: d_ws, d_params, d_x1 and d_x2 are accessed in 16-byte pieces");
    REQUIRE(d_dlogits, "null d_dlogits: the step needs [N] floats of scratch between its loss head and its backward");
    int rc;
    if ((rc = topm_loss_check(tau, sigma, n_samples, __func__))) return rc;
    if ((rc = mllp_gnn_forward(g, d_params, d_x1, d_x2, d_ws, d_logits, stream))) return rc;
    if ((rc = mllp_topm_loss(g, d_logits, d_labels, d_inst_weight, d_pos_weight, d_inst_id, tau, sigma, n_samples, seed, d_dlogits,
                             d_inst_loss, d_loss, nullptr, nullptr, stream)))
        return rc;
    return mllp_gnn_backward(g, d_params, d_x1, d_x2, d_ws, d_dlogits, d_grads, stream);
}
