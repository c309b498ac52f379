// ncx_scorer_util.h -- what the scorers (ncx_scorers.hip) and the contrastive path (ncx_contrastive.hip) share: planned launches on
// the generic GEMM engine with a split-K slab in the caller's workspace, and the fixed-order column sum.
#pragma once
#include <hip/hip_runtime.h>
#include "ncx_internal.h"

namespace ncx {

// Bytes of the split-K slab a launch of `a` with plan `pl` needs (0 when unsplit).
static size_t slab_need(GemmArgs a, const GemmPlan& pl) {
    bool any = false;
    for (int i = 0; i < (a.mode == MODE_GROUP ? a.nseg : 1); ++i) { if (a.split[i] == 0) a.split[i] = pl.split; any |= a.split[i] > 1; }
    if (!any) return 0;
    int bm, bn; cfg_tile(pl.cfg, bm, bn);
    return (size_t)gemm_layout(a, bm, bn, nullptr) * bm * bn * 4;
}
static int run_planned(GemmArgs& a, int form, const GemmPlan& pl, float* slab, size_t slab_bytes, hipStream_t s) {
    const size_t need = slab_need(a, pl);
    for (int i = 0; i < (a.mode == MODE_GROUP ? a.nseg : 1); ++i) if (a.split[i] == 0) a.split[i] = pl.split;
    if (need > slab_bytes) return NCX_E_WORKSPACE;
    a.slab = slab;
    if (form == FORM_NT) return run_gemm_nt(a, pl.cfg, s);
    if (form == FORM_TN) return run_gemm_tn(a, pl.cfg, s);
    return run_gemm_nn(a, pl.cfg, s);
}
static inline long long ksteps(long long k) { return (k + GEMM_BK - 1) / GEMM_BK; }

// out[c] = sum over rows r < R of in[r * ld + c]: one workgroup per column, each thread a fixed stride of rows, then a fixed
// LDS tree (deterministic).
static __global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ in, long long ld, int R, float* __restrict__ out) {
    const int c = blockIdx.x, t = threadIdx.x;
    __shared__ float red[256];
    float acc = 0.f;
    for (int r = t; r < R; r += 256) acc += in[(long long)r * ld + c];
    red[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) out[c] = red[0];
}

}  // namespace ncx
