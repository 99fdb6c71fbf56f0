// optim.hip -- mllp_optim_step: AdamW with global-norm gradient clipping and a warm-up + cosine learning-rate schedule on
// the flat parameter buffer, everything decided on the device (include/mllp_hip.h states the rule and the contracts).
// A translation unit of its own: the device code of node_kernels.hip (mllp_adam_step) and of the fused tail is not
// touched.  The element update restates node_bodies.h::adam_slice expression by expression -- with weight_decay 0,
// clip coefficient 1 and the constant rate it produces adam_slice's bits (tests/test_optim.py) -- as select.hip restates
// the metrics kernel's select.
//
// ORDER OF THE NORM'S SUM (the contract; it depends on n alone).  The elements are cut into slices of OPT_SLICE = 4096:
// slice s holds elements [4096 s, min(n, 4096 (s + 1))).  The partial P_s of a slice is ordered_sum.h's pattern over one
// workgroup of 1024 threads: thread t adds its terms t, t + 1024, t + 2048, t + 3072 of the slice in that order, from 0,
// each as __fmaf_rn(g, g, acc) with g = __fmul_rn(grad, grad_scale); the 64 lanes of a wavefront by the xor butterfly
// (group_sum<64>), the 16 wavefronts by the fixed binary tree (block_tree_sum<16>).  The total is the same pattern over
// the partials: thread t adds P_t, P_(t + 1024), ... in that order, from 0, by __fadd_rn, then butterfly and tree.
// ||g|| = sqrtf(total).  n <= 16384 (at most four slices): one workgroup computes the partials one after the other and
// keeps them in LDS.  Larger n: one workgroup per slice writes P_s to d_scratch[s]; EVERY workgroup of the update launch
// then adds the partials itself, so all of them hold the same bits and no finalize launch is needed.  No float atomics,
// one writer per word, no workgroup waits for another inside a launch.
#include <cmath>

#include "ordered_sum.h"

namespace mllp {

constexpr int OPT_THREADS = 1024;
constexpr int OPT_WAVES = OPT_THREADS / 64;
constexpr int OPT_SLICE = 4096;
constexpr int OPT_SINGLE_MAX = 4 * OPT_SLICE;       // up to here: one launch of one workgroup
constexpr float OPT_NORM_EPS = 1e-6f;               // torch.nn.utils.clip_grad_norm_'s

__host__ __device__ constexpr int64_t opt_slices(int64_t n) { return (n + OPT_SLICE - 1) / OPT_SLICE; }

// P_s of the slice that starts at g, in every thread
__device__ __forceinline__ float slice_sumsq(const float* __restrict__ g, int len, float gscale, float* part) {
    float a = 0.0f;
    for (int i = threadIdx.x; i < len; i += OPT_THREADS) {
        const float gi = __fmul_rn(g[i], gscale);
        a = __fmaf_rn(gi, gi, a);
    }
    return block_tree_sum<OPT_WAVES>(a, part);
}

// the total of the S partials, in every thread
__device__ __forceinline__ float partial_total(const float* partials, int S, float* part) {
    float a = 0.0f;
    for (int j = threadIdx.x; j < S; j += OPT_THREADS) a = __fadd_rn(a, partials[j]);
    return block_tree_sum<OPT_WAVES>(a, part);
}

// the rate of step t (= step + 1): linear warm-up over W steps, half a cosine down to r * lr_base at step T, constant after
__device__ __forceinline__ float lr_at(float lr_base, float t, float W, float T, float r) {
    if (W > 0.0f && t <= W) return lr_base * t / W;
    if (T > W) {
        const float x = fminf(1.0f, (t - W) / (T - W));
        return lr_base * (r + (1.0f - r) * (0.5f * (1.0f + cosf(3.14159274f * x))));
    }
    return lr_base;
}

// what a step's workgroups share.  `total` counts only with have_norm
struct OptStep {
    float t, lr, b1, b2, norm, c;
    bool skip;
};
__device__ __forceinline__ OptStep opt_step(const float* __restrict__ state, bool have_norm, float total, float max_norm) {
    OptStep o;
    o.t = state[0] + 1.0f;
    o.b1 = state[2];
    o.b2 = state[3];
    o.lr = lr_at(state[1], o.t, state[4], state[5], state[6]);
    o.norm = have_norm ? sqrtf(total) : 0.0f;
    o.skip = have_norm && !__builtin_isfinite(o.norm);
    o.c = max_norm > 0.0f ? fminf(1.0f, max_norm / (o.norm + OPT_NORM_EPS)) : 1.0f;
    return o;
}
__device__ __forceinline__ void write_info(float* __restrict__ info, const OptStep& o) {
    info[0] = o.norm;
    info[1] = o.skip ? 0.0f : o.c;
    info[2] = o.lr;
    info[3] = o.skip ? 1.0f : 0.0f;
}

// elements [0, n) of the given (offset) pointers: adam_slice with the gradient times c, the decoupled decay in front of
// it, and elements without a gradient left alone
__device__ __forceinline__ void optim_slice(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                            float* __restrict__ v, const OptStep& o, float eps, float gscale, float wd, int n) {
    const float b1 = o.b1, b2 = o.b2;
    const float bc1 = 1.0f - powf(b1, o.t), bc2 = 1.0f - powf(b2, o.t);
    const float step_size = o.lr / bc1, rs_bc2 = 1.0f / sqrtf(bc2);
    const float decay = o.lr * wd;
    for (int i = threadIdx.x; i < n; i += blockDim.x) {
        const float g0 = g[i] * gscale, m0 = m[i], v0 = v[i];
        if (g0 == 0.0f && m0 == 0.0f && v0 == 0.0f) continue;       // "grad is None": not decayed either
        const float gi = o.c == 1.0f ? g0 : o.c * g0;
        float pi = p[i];
        if (wd != 0.0f) pi = __fmaf_rn(-decay, pi, pi);
        const float mi = fmaf(b1, m0, (1.0f - b1) * gi);
        const float vi = fmaf(b2, v0, (1.0f - b2) * gi * gi);
        m[i] = mi;
        v[i] = vi;
        const float denom = sqrtf(vi) * rs_bc2 + eps;
        p[i] = pi - step_size * (mi / denom);
    }
}

// n <= OPT_SINGLE_MAX: norm, barrier, update, tick
__global__ __launch_bounds__(OPT_THREADS) void optim_single_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                    float* __restrict__ m, float* __restrict__ v,
                                                                    float* __restrict__ state, float eps, float gscale, float wd,
                                                                    float max_norm, float* __restrict__ info, int n, int need_norm) {
    __shared__ float part[OPT_WAVES];
    __shared__ float s_p[OPT_SINGLE_MAX / OPT_SLICE];
    float total = 0.0f;
    if (need_norm) {        // (uniform: a kernel argument)
        const int S = (int)opt_slices(n);
        for (int s = 0; s < S; ++s) {
            const float P = slice_sumsq(g + s * OPT_SLICE, min(OPT_SLICE, n - s * OPT_SLICE), gscale, part);
            if (threadIdx.x == 0) s_p[s] = P;
        }
        __syncthreads();
        total = partial_total(s_p, S, part);
    }
    const OptStep o = opt_step(state, need_norm != 0, total, max_norm);
    __syncthreads();        // every thread has read the state before thread 0 writes it
    if (threadIdx.x == 0 && info) write_info(info, o);
    if (o.skip) return;
    optim_slice(p, g, m, v, o, eps, gscale, wd, n);
    if (threadIdx.x == 0) state[0] = o.t;
}

// n > OPT_SINGLE_MAX, launch 1 (only when a norm is needed): P_s -> scratch[s]
__global__ __launch_bounds__(OPT_THREADS) void optim_partials_kernel(const float* __restrict__ g, float gscale,
                                                                      float* __restrict__ scratch, int n) {
    __shared__ float part[OPT_WAVES];
    const int o = blockIdx.x * OPT_SLICE;
    const float P = slice_sumsq(g + o, min(OPT_SLICE, n - o), gscale, part);
    if (threadIdx.x == 0) scratch[blockIdx.x] = P;
}

// launch 2: every workgroup adds the partials itself, then updates its slice.  The workgroups only READ the step counter;
// workgroup 0 writes the info words and, behind the partials, the word that tells the tick whether the step was skipped
__global__ __launch_bounds__(OPT_THREADS) void optim_wide_kernel(float* __restrict__ p, const float* __restrict__ g,
                                                                  float* __restrict__ m, float* __restrict__ v,
                                                                  const float* __restrict__ state, float eps, float gscale, float wd,
                                                                  float max_norm, float* scratch, float* __restrict__ info, int n,
                                                                  int need_norm) {
    __shared__ float part[OPT_WAVES];
    const int S = (int)gridDim.x;
    const float total = need_norm ? partial_total(scratch, S, part) : 0.0f;
    const OptStep st = opt_step(state, need_norm != 0, total, max_norm);
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        if (info) write_info(info, st);
        if (need_norm) scratch[S] = st.skip ? 1.0f : 0.0f;
    }
    if (st.skip) return;
    const int o = blockIdx.x * OPT_SLICE;
    optim_slice(p + o, g + o, m + o, v + o, st, eps, gscale, wd, min(OPT_SLICE, n - o));
}

// launch 3: one thread advances the step counter unless the step was skipped (stream order behind launch 2)
__global__ void optim_tick_kernel(float* __restrict__ state, const float* __restrict__ skipped) {
    if (!skipped || *skipped == 0.0f) state[0] += 1.0f;
}

static int launch_optim(float* p, const float* g, float* m, float* v, float* state, float eps, float gscale, float wd,
                        float max_norm, float* scratch, float* info, int64_t n, hipStream_t s) {
    const int need_norm = (max_norm > 0.0f || info) ? 1 : 0;
    if (n <= OPT_SINGLE_MAX) {
        hipLaunchKernelGGL(optim_single_kernel, dim3(1), dim3(OPT_THREADS), 0, s, p, g, m, v, state, eps, gscale, wd, max_norm,
                           info, (int)n, need_norm);
        return check_launch("optim_single");
    }
    const unsigned S = (unsigned)opt_slices(n);
    if (need_norm) {
        hipLaunchKernelGGL(optim_partials_kernel, dim3(S), dim3(OPT_THREADS), 0, s, g, gscale, scratch, (int)n);
        if (int rc = check_launch("optim_partials")) return rc;
    }
    hipLaunchKernelGGL(optim_wide_kernel, dim3(S), dim3(OPT_THREADS), 0, s, p, g, m, v, state, eps, gscale, wd, max_norm, scratch,
                       info, (int)n, need_norm);
    if (int rc = check_launch("optim_wide")) return rc;
    hipLaunchKernelGGL(optim_tick_kernel, dim3(1), dim3(1), 0, s, state, need_norm ? scratch + S : (const float*)nullptr);
    return check_launch("optim_tick");
}

}  // namespace mllp

using namespace mllp;

extern "C" int mllp_optim_scratch_floats(int64_t n, int64_t* out) {
    REQUIRE(out, "null argument");
    REQUIRE(n >= 0 && n < (int64_t)1 << 30, "bad parameter count");
    *out = n <= OPT_SINGLE_MAX ? 0 : opt_slices(n) + 1;
    return MLLP_OK;
}

extern "C" int mllp_optim_step(float* d_params, const float* d_grads, float* d_exp_avg, float* d_exp_avg_sq, float* d_state,
                               float eps, float grad_scale, float weight_decay, float max_norm, float* d_scratch, float* d_info,
                               int64_t n, void* stream) {
    REQUIRE(d_params && d_grads && d_exp_avg && d_exp_avg_sq && d_state, "null argument");
    REQUIRE(n >= 0 && n < (int64_t)1 << 30, "bad parameter count");
    REQUIRE(std::isfinite(eps) && std::isfinite(grad_scale) && std::isfinite(weight_decay) && std::isfinite(max_norm),
            "eps, grad_scale, weight_decay and max_norm must be finite");
    REQUIRE(weight_decay >= 0.0f, "weight_decay must not be negative");
    REQUIRE(max_norm >= 0.0f, "max_norm must not be negative (0 = no clipping)");
    REQUIRE(d_scratch || n <= OPT_SINGLE_MAX, "d_scratch: this n needs mllp_optim_scratch_floats(n) floats of scratch");
    return launch_optim(d_params, d_grads, d_exp_avg, d_exp_avg_sq, d_state, eps, grad_scale, weight_decay, max_norm, d_scratch,
                        d_info, n, (hipStream_t)stream);
}
