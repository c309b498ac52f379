// ncx_train.hip -- the element-wise kernels that more than one VQA trainer launches, behind the launchers of ncx_train.h: the library is
// built without relocatable device code, so each kernel has this one home.  What they compute, bit for bit, is what the trainers' own
// copies computed.
#include "ncx_train.h"

namespace ncx {
// vd[b] = drop_v(feats[clamp(img_idx[b])]), qd[b] = drop_q(q_emb[b]): V elements per thread, rows of (dv + dq) / V groups.
template <int V>
__global__ __launch_bounds__(256) void k_train_drop_vq(const float* __restrict__ feats, const int* __restrict__ img_idx, const float* __restrict__ q,
                                                       int B, int dv, int dq, int n_img, TrainDrop k, const float* __restrict__ masks,
                                                       float* __restrict__ vd, float* __restrict__ qd) {
    const int gv = dv / V, W = gv + dq / V;
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (long long)B * W) return;
    const int b = (int)(i / W), c = (int)(i - (long long)b * W);
    if (c < gv) {
        const int row = clamp_img(img_idx[b], n_img);
        const long long e = (long long)b * dv + c * V;
        TrainVec<V> x = train_ld<V>(feats + (long long)row * dv + c * V);
        const float sc = 1.f / (1.f - k.p[VQ_LAYER_V - 1]);
#pragma unroll
        for (int j = 0; j < V; ++j) x.v[j] = train_keep(k, VQ_LAYER_V, masks, e + j) ? x.v[j] * sc : 0.f;
        train_st<V>(vd + e, x);
    } else {
        const long long e = (long long)b * dq + (c - gv) * V;
        TrainVec<V> x = train_ld<V>(q + e);
        const float sc = 1.f / (1.f - k.p[VQ_LAYER_Q - 1]);
        const float* mq = masks ? masks + (long long)B * dv : nullptr;
#pragma unroll
        for (int j = 0; j < V; ++j) x.v[j] = train_keep(k, VQ_LAYER_Q, mq, e + j) ? x.v[j] * sc : 0.f;
        train_st<V>(qd + e, x);
    }
}
// 16-byte lanes: row widths that are multiples of 4 keep every group inside one row and every row 16-byte aligned
hipError_t train_drop_vq(const ncx_vqa_train_dims& d, const float* feats, const int* img_idx, const float* q, const TrainDrop& k,
                                const float* masks, float* vd, float* qd, hipStream_t s) {
    if (d.dv % 4 == 0 && d.dq % 4 == 0 && al16(feats) && al16(q))
        hipLaunchKernelGGL(k_train_drop_vq<4>, dim3(grid256((long long)d.B * ((d.dv + d.dq) / 4))), dim3(256), 0, s, feats, img_idx, q, d.B, d.dv,
                           d.dq, d.n_img, k, masks, vd, qd);
    else
        hipLaunchKernelGGL(k_train_drop_vq<1>, dim3(grid256((long long)d.B * (d.dv + d.dq))), dim3(256), 0, s, feats, img_idx, q, d.B, d.dv, d.dq,
                           d.n_img, k, masks, vd, qd);
    return hipGetLastError();
}

// out[i] = drop_layer(in[i]), i < n (in == out allowed)
__global__ __launch_bounds__(256) void k_train_drop_flat(const float* in, float* out, long long n, TrainDrop k, int layer, const float* __restrict__ mask) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    out[i] = train_keep(k, layer, mask, i) ? in[i] * train_scale(k, layer) : 0.f;
}
hipError_t train_drop_flat(const float* in, float* out, long long n, const TrainDrop& k, int layer, const float* mask, hipStream_t s) {
    hipLaunchKernelGGL(k_train_drop_flat, dim3(grid256(n)), dim3(256), 0, s, in, out, n, k, layer, mask);
    return hipGetLastError();
}

// The backward of t = act_c(x_v * x_q):  dz = dt (1 - t^2);  dpv = dz x_q (1 - x_v^2);  dpq = dz x_v (1 - x_q^2): a tanh factor only
// where that activation is tanh (t is read only then).  n elements, V per thread.
template <int V>
__global__ __launch_bounds__(256) void k_train_dfuse(const float* __restrict__ dt, const float* __restrict__ t, const float* __restrict__ xv,
                                                     const float* __restrict__ xq, long long n, int act_v, int act_q, int act_c,
                                                     float* __restrict__ dpv, float* __restrict__ dpq) {
    const long long i = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (i >= n) return;
    const TrainVec<V> g = train_ld<V>(dt + i), a = train_ld<V>(xv + i), b = train_ld<V>(xq + i);
    TrainVec<V> tt{};
    if (act_c == 2) tt = train_ld<V>(t + i);
    TrainVec<V> pv, pq;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float dz = act_c == 2 ? g.v[j] * (1.f - tt.v[j] * tt.v[j]) : g.v[j];
        const float gv = dz * b.v[j], gq = dz * a.v[j];
        pv.v[j] = act_v == 2 ? gv * (1.f - a.v[j] * a.v[j]) : gv;
        pq.v[j] = act_q == 2 ? gq * (1.f - b.v[j] * b.v[j]) : gq;
    }
    train_st<V>(dpv + i, pv);
    train_st<V>(dpq + i, pq);
}
// every operand is a 256-byte aligned workspace region
hipError_t train_dfuse(const float* dt, const float* t, const float* xv, const float* xq, long long n, int act_v, int act_q, int act_c,
                              float* dpv, float* dpq, hipStream_t s) {
    if (n % 4 == 0) hipLaunchKernelGGL(k_train_dfuse<4>, dim3(grid256(n / 4)), dim3(256), 0, s, dt, t, xv, xq, n, act_v, act_q, act_c, dpv, dpq);
    else hipLaunchKernelGGL(k_train_dfuse<1>, dim3(grid256(n)), dim3(256), 0, s, dt, t, xv, xq, n, act_v, act_q, act_c, dpv, dpq);
    return hipGetLastError();
}

// d *= 1 - y^2 in place over up to two tensors, for the ones whose activation is tanh (n1 == 0: one tensor)
__global__ __launch_bounds__(256) void k_train_dact(float* __restrict__ d0, const float* __restrict__ y0, long long n0, int act0,
                                                    float* __restrict__ d1, const float* __restrict__ y1, long long n1, int act1) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n0) {
        if (act0 == 2) { const float x = y0[i]; d0[i] *= 1.f - x * x; }
    } else if (i < n0 + n1) {
        const long long e = i - n0;
        if (act1 == 2) { const float x = y1[e]; d1[e] *= 1.f - x * x; }
    }
}
hipError_t train_dact(float* d0, const float* y0, long long n0, int act0, float* d1, const float* y1, long long n1, int act1, hipStream_t s) {
    hipLaunchKernelGGL(k_train_dact, dim3(grid256(n0 + n1)), dim3(256), 0, s, d0, y0, n0, act0, d1, y1, n1, act1);
    return hipGetLastError();
}
}  // namespace ncx
