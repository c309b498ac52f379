// ncx_adam.h -- the Adam update, shared by k_adam (ncx_loss_adam.hip) and by the launch of the answer-embedding gradient that applies it
// where the gradient is produced (ncx_main.h: the tile epilogue for answer_embedding, passenger workgroups for the rest of the flat buffer).
//
// torch.optim.Adam (counterexamples.py:275-276): m = lerp(m, g, 1-b1); v = b2 v + (1-b2) g^2; p -= (lr / bc1) * m / (sqrt(v) / sqrt(bc2) + eps).
// Every caller must return the same bits, so the roundings are spelled out: contraction is off inside adam_update and each fused operation
// is an explicit fma.  They are the ones hipcc chose for k_adam when the expression stood in the kernel (read from its gfx950 code):
//     d  = fma(g, gscale, -m)               (NOT gj - m with the rounded gj)
//     m' = fma(1 - b1, d, m)
//     gj = g * gscale;  u = gj * ((1 - b2) * gj)
//     v' = fma(b2, v, u)                    (VFMA; the one exception is below)
//     p' = fma(-step_size, m' / fma(inv_bc2_sqrt, sqrt(v'), eps), p)
// The exception: the ragged end of the buffer (n % 4 elements) was a scalar loop that hipcc unrolled by two; the pairs kept the fma above,
// the odd last element came out as v' = b2 * v + u with two roundings.  adam_tail keeps that, element for element.
#pragma once
#include "ncx_gemm.h"
#include <math.h>

namespace ncx {

struct AdamScalars { float step_size, b1, b2, eps, inv_bc2_sqrt, gscale; };

// the host-side scalars of step `step` (1-based): bias corrections in double, rounded once
static inline AdamScalars adam_scalars(float lr, float beta1, float beta2, float eps, int step, float grad_scale) {
    const double bc1 = 1.0 - pow((double)beta1, (double)step);
    const double bc2 = 1.0 - pow((double)beta2, (double)step);
    AdamScalars s;
    s.step_size = (float)((double)lr / bc1);
    s.inv_bc2_sqrt = (float)(1.0 / sqrt(bc2));
    s.b1 = beta1; s.b2 = beta2; s.eps = eps; s.gscale = grad_scale;
    return s;
}

template <bool VFMA = true>
__device__ __forceinline__ void adam_update(float& p, const float g, float& m, float& v, const float step_size, const float b1, const float b2,
                                            const float eps, const float inv_bc2_sqrt, const float gscale) {
#pragma clang fp contract(off)
    const float gj = g * gscale;
    const float d = __builtin_fmaf(g, gscale, -m);
    m = __builtin_fmaf(1.f - b1, d, m);
    const float u = gj * ((1.f - b2) * gj);
    if (VFMA) v = __builtin_fmaf(b2, v, u);
    else v = b2 * v + u;
    const float den = __builtin_fmaf(inv_bc2_sqrt, sqrtf(v), eps);
    p = __builtin_fmaf(-step_size, m / den, p);
}

// elements [i, i + 4) of 16-byte aligned buffers
__device__ __forceinline__ void adam_quad(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          const size_t i, const AdamScalars& s) {
    f32x4 pv = *(f32x4*)(p + i), mv = *(f32x4*)(m + i), vv = *(f32x4*)(v + i);
    const f32x4 gv = *(const f32x4*)(g + i);
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        float pj = pv[j], mj = mv[j], vj = vv[j];
        adam_update(pj, gv[j], mj, vj, s.step_size, s.b1, s.b2, s.eps, s.inv_bc2_sqrt, s.gscale);
        pv[j] = pj; mv[j] = mj; vv[j] = vj;
    }
    *(f32x4*)(p + i) = pv; *(f32x4*)(m + i) = mv; *(f32x4*)(v + i) = vv;
}

// the ragged end [i, n), n - i < 4: one thread
__device__ __forceinline__ void adam_tail(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m, float* __restrict__ v,
                                          const size_t i, const size_t n, const AdamScalars& s) {
    const size_t paired = i + ((n - i) & ~(size_t)1);
    for (size_t j = i; j < n; ++j) {
        float pj = p[j], mj = m[j], vj = v[j];
        if (j < paired) adam_update<true>(pj, g[j], mj, vj, s.step_size, s.b1, s.b2, s.eps, s.inv_bc2_sqrt, s.gscale);
        else adam_update<false>(pj, g[j], mj, vj, s.step_size, s.b1, s.b2, s.eps, s.inv_bc2_sqrt, s.gscale);
        m[j] = mj; v[j] = vj; p[j] = pj;
    }
}

// What the launch of the answer-embedding gradient needs to apply Adam itself (MainArgs::adam, ncx_main.h).  The tile epilogue updates
// p / m / v at the element whose gradient it has just stored (the same [A][da] layout and leading dimension as the output); workgroups
// [pass_at, pass_at + n_pass) of the grid are passengers: no tile, a contiguous slice of the other tn elements (tp, tg, tm, tv: 16-byte
// aligned, every gradient there final before the launch).
struct AdamFuse {
    float* p; float* m; float* v;
    float* tp; const float* tg; float* tm; float* tv;
    unsigned long long tn;
    int n_pass, pass_at;
    AdamScalars s;
};

// passenger w of a.n_pass: quads [w * per, (w + 1) * per) of the tail, per = ceil(quads / n_pass); the ragged last quad goes through adam_tail
__device__ __forceinline__ void adam_passenger(const AdamFuse& a, const int w, const int tid, const int nthreads) {
    const size_t n = a.tn, quads = (n + 3) / 4, per = (quads + a.n_pass - 1) / a.n_pass;
    const size_t q0 = (size_t)w * per, q1 = q0 + per < quads ? q0 + per : quads;
    for (size_t q = q0 + tid; q < q1; q += nthreads) {
        const size_t i = q * 4;
        if (i + 3 < n) adam_quad(a.tp, a.tg, a.tm, a.tv, i, a.s);
        else adam_tail(a.tp, a.tg, a.tm, a.tv, i, n, a.s);
    }
}

// k_adam over a whole buffer (ncx_loss_adam.hip); n >= 1, 16-byte aligned pointers
__attribute__((visibility("hidden"))) int adam_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                                                      const AdamScalars& s, hipStream_t stream);

}  // namespace ncx
