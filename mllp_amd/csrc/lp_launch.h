// lp_launch.h -- host only: what the LP solver entry points (basis.hip, simplex.hip, pdhg.hip) do around their kernels.
// Each of them runs one workgroup per instance from a kernel instantiated twice, once per address space of the instance's
// working set (LDS / the caller's scratch), and both launches cover the whole batch: a workgroup whose instance belongs to
// the other launch returns at once.  Here: the plan of such a call and the launch of one instantiation.
#pragma once

#include "internal.h"

namespace mllp {

// what a call needs, from the host copy of the instance offsets
struct LpPlan {
    int64_t words = 0;          // scratch, in 4-byte words
    int64_t lds_extent = 0;     // the largest extent (m, or pdhg_words(m, n)) that runs in LDS
    int64_t glb_extent = 0;     // ... in scratch
    bool any_lds = false, any_glb = false;      // which launches have an instance (a skipped one included)
};

// one instance, as a solver's classifier (m, n) -> LpInstance sees it
struct LpInstance {
    bool in_lds;        // which launch it belongs to
    bool runs;          // false: skipped (m > max_m) -- it counts for any_* alone
    int64_t words;      // its scratch
    int64_t extent;     // what sizes its launch's dynamic LDS
};

template <class Classify>
LpPlan lp_plan(const mllp_graph_t* g, Classify classify) {
    LpPlan p;
    const std::vector<int64_t>&pm = g->h_inst_ptr_m, &pn = g->h_inst_ptr_n;
    for (int64_t k = 0; k < g->n_inst && k + 1 < (int64_t)std::min(pm.size(), pn.size()); ++k) {
        const LpInstance i = classify(pm[k + 1] - pm[k], pn[k + 1] - pn[k]);
        (i.in_lds ? p.any_lds : p.any_glb) = true;
        if (!i.runs) continue;
        p.words += i.words;
        int64_t& extent = i.in_lds ? p.lds_extent : p.glb_extent;
        extent = std::max(extent, i.extent);
    }
    return p;
}

// dynamic LDS of a launch whose largest instance takes `words` (never 0 bytes)
constexpr size_t lp_lds_bytes(int64_t words) { return (size_t)std::max<int64_t>(words, 1) * sizeof(float); }

// One instantiation's launch over the n_inst > 0 instances of a batch.  `stem` is the entry point's name without mllp_,
// `where` " (LDS)" or " (scratch)": errors of HIP carry them.  attr_bytes > 0: the kernel may take that much dynamic LDS,
// more than the default limit -- set once per process and instantiation (the static below is this instantiation's own), and
// no stream operation.
template <auto Kernel, int NT, class Args>
int lp_launch(const std::string& stem, const char* where, int64_t n_inst, int64_t attr_bytes, size_t lds_bytes, hipStream_t s,
              const Args& args) {
    if (attr_bytes > 0) {
        static const hipError_t attr =
            hipFuncSetAttribute(reinterpret_cast<const void*>(Kernel), hipFuncAttributeMaxDynamicSharedMemorySize, (int)attr_bytes);
        if (attr != hipSuccess) return hip_fail(attr, (stem + ": hipFuncSetAttribute").c_str());
    }
    hipLaunchKernelGGL(Kernel, dim3((unsigned)n_inst), dim3(NT), lds_bytes, s, args);
    return check_launch((stem + where).c_str());
}

}  // namespace mllp
