// ncx_contrastive.hip -- the contrastive training path of the reference's second script: ContrastiveModel (vqa/models/cx.py:
// 428-487), ContrastiveLoss (contrastive.py:293-309) and the distance-ranked evaluation (contrastive.py:259-290).
//
// Per image j of example b (P = knn_size + 1 images, slot 0 the original; H = 300, cx.py:437):
//   h[b, j] = relu(W . cat(v_j, z_j) + bias)                              (cx.py:470-472; W = linear.weight [300, dv + dz], v | z)
// The concat is never built and the feature rows are never copied out dense:
//   k_ct_prep      clamps the P feature-table rows of every example (sets *bad_id_flag when it had to) and lays z_orig / z_knns
//                  out as one [B P, dz] operand (row b P + j: z_orig[b] for j = 0, else z_knns[b, j - 1])
//   h [B P, 300]   = relu([v (gathered) | z] . W^T + bias)                one NT chain of 2 segments, bias + ReLU epilogue
// Evaluation:
//   k_ct_dist      dist[b, k] = || h[b, 0] - h[b, k + 1] + 1e-6 ||        (cx.py:478-487, F.pairwise_distance), one wave per pair
// Training (P = 3: original, counterexample, one other neighbour; contrastive.py:213-219):
//   k_ct_loss      one wave per example: both distances, max(margin - d_comp, 0)^2 and d_other^2 (each times `scale`), and
//                  dpre [B, 3, 300], the gradient with respect to the PRE-activation (ReLU mask applied, the two contributions
//                  to slot 0 summed, `scale` folded in)
//   k_colsum       loss_comp, loss_other and the two mean distances: fixed-order sums over b of the per-example values
//   dW             dpre^T . [v (gathered again) | z]                      one TN group of 2 problems over the B P rows
//   k_colsum       d linear.bias = sum over rows of dpre
// answer_embedding.weight (cx.py:440-441) is never read by the model and has no gradient: it does not appear here.
// Nothing uses atomics; every result is bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ncx_internal.h"

namespace ncx {

constexpr int CT_H = 300;          // dim_h (cx.py:437)
constexpr int CT_MAX_K = 64;       // ncx_loss_rank's bound (the evaluation ranks the distances with it)
constexpr float CT_EPS = 1e-6f;    // F.pairwise_distance's eps, inside the norm

struct CtLayout { size_t idx, zall, h, dpre, per, slab, slab_bytes, total; };

static bool ct_dims_ok(const ncx_contrastive_dims* d) {
    if (d->B < 1 || d->P < 2 || d->P - 1 > CT_MAX_K || d->dv < 4 || d->dz < 4 || d->n_img < 1) return false;
    const long long M = (long long)d->B * d->P;
    return M * CT_H < (1ll << 31) && M * d->dv < (1ll << 31) && M * d->dz < (1ll << 31) && (long long)d->n_img * d->dv < (1ll << 31);
}

struct CtPtrs {
    const float *feats, *zall, *W, *b, *dpre;
    const int* idx;
    float *h, *gW;
};
static GemmArgs ct_gemm_h(const ncx_contrastive_dims& d, const CtPtrs& p, GemmPlan* pl) {
    const int M = d.B * d.P, din = d.dv + d.dz;
    GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 2; a.M = M;
    a.a[0] = x_gather(p.feats, d.dv, p.idx, M, d.dv); a.b[0] = x_plain(p.W, din, CT_H, d.dv);        a.klen[0] = d.dv;
    a.a[1] = x_plain(p.zall, d.dz, M, d.dz);          a.b[1] = x_plain(p.W + d.dv, din, CT_H, d.dz); a.klen[1] = d.dz;
    a.out[0] = p.h; a.ldo[0] = CT_H; a.n_cols[0] = CT_H;
    a.epi.bias = p.b; a.epi.relu = 1;
    *pl = plan_gemm(FORM_NT, M, CT_H, ksteps(d.dv) + ksteps(d.dz), true);
    return a;
}
static GemmArgs ct_gemm_dw(const ncx_contrastive_dims& d, const CtPtrs& p, GemmPlan* pl) {
    const int M = d.B * d.P, din = d.dv + d.dz;
    GemmArgs a{}; a.mode = MODE_GROUP; a.nseg = 2; a.M = CT_H;
    a.a[0] = x_plain(p.dpre, CT_H, M, CT_H); a.b[0] = x_gather(p.feats, d.dv, p.idx, M, d.dv); a.klen[0] = M;
    a.out[0] = p.gW; a.ldo[0] = din; a.n_cols[0] = d.dv;
    a.a[1] = x_plain(p.dpre, CT_H, M, CT_H); a.b[1] = x_plain(p.zall, d.dz, M, d.dz);          a.klen[1] = M;
    a.out[1] = p.gW ? p.gW + d.dv : nullptr; a.ldo[1] = din; a.n_cols[1] = d.dz;
    *pl = plan_gemm(FORM_TN, CT_H, d.dv + d.dz, ksteps(M), false);
    return a;
}

static CtLayout ct_layout(const ncx_contrastive_dims& d) {
    CtLayout w{}; WsCarver cv;
    const size_t M = (size_t)d.B * d.P;
    w.idx = cv.take(M * 4); w.zall = cv.take(M * d.dz * 4); w.h = cv.take(M * CT_H * 4); w.dpre = cv.take(M * CT_H * 4);
    w.per = cv.take((size_t)d.B * 16);
    CtPtrs p{}; GemmPlan pl; size_t sb, t;
    GemmArgs a = ct_gemm_h(d, p, &pl); sb = gemm_slab_bytes(a, pl);
    a = ct_gemm_dw(d, p, &pl);         t = gemm_slab_bytes(a, pl); sb = t > sb ? t : sb;
    w.slab = cv.take(sb); w.slab_bytes = sb;
    w.total = cv.off;
    return w;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// One thread per element of zall [B P, dz]; the thread of a row's column 0 also clamps that row's feature-table id.
__global__ __launch_bounds__(256) void k_ct_prep(const int* __restrict__ img_idx, const float* __restrict__ z_orig,
                                                 const float* __restrict__ z_knns, int B, int P, int dz, int n_img,
                                                 int* __restrict__ idx, float* __restrict__ zall, int* __restrict__ bad) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (long long)B * P * dz) return;
    const int r = (int)(i / dz), c = (int)(i % dz);
    const int b = r / P, j = r % P;
    zall[i] = j == 0 ? z_orig[(long long)b * dz + c] : z_knns[((long long)b * (P - 1) + j - 1) * dz + c];
    if (c == 0) {
        int v = img_idx[r];
        if (v < 0 || v >= n_img) { *bad = 1; v = v < 0 ? 0 : n_img - 1; }
        idx[r] = v;
    }
}

// dist[b, k] = || h[b, 0] - h[b, k + 1] + eps ||: one wave per (b, k), 75 float4 per row, fixed butterfly.
__global__ __launch_bounds__(256) void k_ct_dist(const float* __restrict__ h, int B, int P, float* __restrict__ dist) {
    const long long w = blockIdx.x * 4ll + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (w >= (long long)B * (P - 1)) return;
    const int b = (int)(w / (P - 1)), k = (int)(w % (P - 1));
    const float4* h0 = (const float4*)(h + (long long)b * P * CT_H);
    const float4* hk = (const float4*)(h + ((long long)b * P + k + 1) * CT_H);
    float ss = 0.f;
    for (int q = lane; q < CT_H / 4; q += 64) {
        const float4 x = h0[q], y = hk[q];
        const float e0 = x.x - y.x + CT_EPS, e1 = x.y - y.y + CT_EPS, e2 = x.z - y.z + CT_EPS, e3 = x.w - y.w + CT_EPS;
        ss = fmaf(e0, e0, ss); ss = fmaf(e1, e1, ss); ss = fmaf(e2, e2, ss); ss = fmaf(e3, e3, ss);
    }
    for (int o = 32; o > 0; o >>= 1) ss += __shfl_xor(ss, o);
    if (lane == 0) dist[w] = sqrtf(ss);
}

// One wave per example (P = 3).  per[b] = {scale max(margin - d1, 0)^2, scale d2^2, scale d1, scale d2}; dist[b] = {d1, d2};
// dpre[b, j, c] = d (loss_comp + loss_other) / d pre-activation.  With e1 = h0 - h1 + eps, e2 = h0 - h2 + eps:
//   d loss_comp / d h0 = -2 max(margin - d1, 0) e1 / d1,  d loss_other / d h0 = 2 e2  (d (d2^2) = 2 d2 . e2 / d2), and the
//   negatives for h1 / h2; a unit whose activation is 0 passes nothing (ReLU).
__global__ __launch_bounds__(256) void k_ct_loss(const float* __restrict__ h, int B, float margin, float scale,
                                                 float* __restrict__ per, float* __restrict__ dist, float* __restrict__ dpre) {
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (b >= B) return;
    const float4* h0 = (const float4*)(h + (long long)b * 3 * CT_H);
    const float4* h1 = h0 + CT_H / 4;
    const float4* h2 = h1 + CT_H / 4;
    constexpr int NQ = (CT_H / 4 + 63) / 64;          // float4 per lane and row: 2 (75 per row)
    float a0[NQ][4], e1[NQ][4], e2[NQ][4], m1[NQ][4], m2[NQ][4];
    float ss1 = 0.f, ss2 = 0.f;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = lane + 64 * i;
        if (q < CT_H / 4) {
            const float4 x = h0[q], y = h1[q], z = h2[q];
            const float xs[4] = {x.x, x.y, x.z, x.w}, ys[4] = {y.x, y.y, y.z, y.w}, zs[4] = {z.x, z.y, z.z, z.w};
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                a0[i][j] = xs[j]; m1[i][j] = ys[j]; m2[i][j] = zs[j];
                e1[i][j] = xs[j] - ys[j] + CT_EPS; e2[i][j] = xs[j] - zs[j] + CT_EPS;
                ss1 = fmaf(e1[i][j], e1[i][j], ss1); ss2 = fmaf(e2[i][j], e2[i][j], ss2);
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) { ss1 += __shfl_xor(ss1, o); ss2 += __shfl_xor(ss2, o); }
    const float d1 = sqrtf(ss1), d2 = sqrtf(ss2);
    const float hinge = margin - d1 > 0.f ? margin - d1 : 0.f;
    if (lane == 0) {
        float4 p; p.x = scale * hinge * hinge; p.y = scale * d2 * d2; p.z = scale * d1; p.w = scale * d2;
        *(float4*)(per + (long long)b * 4) = p;
        if (dist) { dist[(long long)b * 2] = d1; dist[(long long)b * 2 + 1] = d2; }
    }
    const float g1 = hinge > 0.f ? -2.f * hinge / d1 * scale : 0.f;      // coefficient of e1 in d loss / d h0
    const float g2 = 2.f * scale;                                        // coefficient of e2
    float4* o0 = (float4*)(dpre + (long long)b * 3 * CT_H);
    float4* o1 = o0 + CT_H / 4;
    float4* o2 = o1 + CT_H / 4;
#pragma unroll
    for (int i = 0; i < NQ; ++i) {
        const int q = lane + 64 * i;
        if (q < CT_H / 4) {
            float r0[4], r1[4], r2[4];
#pragma unroll
            for (int j = 0; j < 4; ++j) {
                const float c1 = g1 * e1[i][j], c2 = g2 * e2[i][j];
                r0[j] = a0[i][j] > 0.f ? c1 + c2 : 0.f;
                r1[j] = m1[i][j] > 0.f ? -c1 : 0.f;
                r2[j] = m2[i][j] > 0.f ? -c2 : 0.f;
            }
            o0[q] = make_float4(r0[0], r0[1], r0[2], r0[3]);
            o1[q] = make_float4(r1[0], r1[1], r1[2], r1[3]);
            o2[q] = make_float4(r2[0], r2[1], r2[2], r2[3]);
        }
    }
}

// dpre = dh where h > 0, else 0 (the ReLU of cx.py:472), for a gradient that comes from outside (the drop-in module's autograd).
__global__ __launch_bounds__(256) void k_ct_mask(const float* __restrict__ dh, const float* __restrict__ h, long long n4,
                                                 float* __restrict__ dpre) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n4) return;
    const float4 g = ((const float4*)dh)[i], a = ((const float4*)h)[i];
    ((float4*)dpre)[i] = make_float4(a.x > 0.f ? g.x : 0.f, a.y > 0.f ? g.y : 0.f, a.z > 0.f ? g.z : 0.f, a.w > 0.f ? g.w : 0.f);
}

}  // namespace ncx

using namespace ncx;

extern "C" size_t ncx_contrastive_workspace_bytes(const ncx_contrastive_dims* d) {
    if (!d || !ct_dims_ok(d)) return 0;
    return ct_layout(*d).total;
}

extern "C" int ncx_contrastive_forward(const ncx_contrastive_dims* dp, const ncx_inputs* in, const float* w, const float* b, void* ws,
                                       size_t ws_bytes, float* h_out, int32_t* bad_id_flag, void* stream_) {
    if (!dp || !in || !w || !b || !ws || !bad_id_flag) return NCX_E_NULL;
    if (!in->feats || !in->img_idx || !in->z_orig || !in->z_knns) return NCX_E_NULL;
    if (!ct_dims_ok(dp)) return NCX_E_DIMS;
    const ncx_contrastive_dims& d = *dp;
    const CtLayout l = ct_layout(d);
    if (!ws_ok(ws, ws_bytes, l.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    const long long M = (long long)d.B * d.P, n = M * d.dz;
    CtPtrs q{};
    q.feats = in->feats; q.W = w; q.b = b; q.idx = (int*)(base + l.idx); q.zall = (float*)(base + l.zall); q.h = (float*)(base + l.h);
    hipLaunchKernelGGL(k_ct_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in->img_idx, in->z_orig, in->z_knns, d.B, d.P, d.dz,
                       d.n_img, (int*)q.idx, (float*)q.zall, (int*)bad_id_flag);
    NCX_HIP_TRY(hipGetLastError());
    GemmPlan pl;
    GemmArgs a = ct_gemm_h(d, q, &pl);
    int rc = run_gemm_planned(a, FORM_NT, pl, (float*)(base + l.slab), l.slab_bytes, nullptr, s); if (rc) return rc;
    if (h_out) NCX_HIP_TRY(hipMemcpyAsync(h_out, q.h, (size_t)M * CT_H * 4, hipMemcpyDeviceToDevice, s));
    return NCX_OK;
}

extern "C" int ncx_contrastive_distances(const ncx_contrastive_dims* dp, const float* h, void* ws, size_t ws_bytes, float* dist, void* stream_) {
    if (!dp || !dist || (!h && !ws)) return NCX_E_NULL;
    if (!ct_dims_ok(dp)) return NCX_E_DIMS;
    if (!h) {
        const CtLayout l = ct_layout(*dp);
        if (!ws_ok(ws, ws_bytes, l.total)) return NCX_E_WORKSPACE;
        h = (const float*)((char*)ws + l.h);
    } else if ((uintptr_t)h & 15) return NCX_E_DIMS;
    const long long n = (long long)dp->B * (dp->P - 1);
    hipLaunchKernelGGL(k_ct_dist, dim3((unsigned)((n + 3) / 4)), dim3(256), 0, (hipStream_t)stream_, h, dp->B, dp->P, dist);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

extern "C" int ncx_contrastive_loss(const ncx_contrastive_dims* dp, void* ws, size_t ws_bytes, float margin, float scale, float* losses4,
                                    float* dist, void* stream_) {
    if (!dp || !ws || !losses4) return NCX_E_NULL;
    if (!ct_dims_ok(dp) || dp->P != 3) return NCX_E_DIMS;
    const CtLayout l = ct_layout(*dp);
    if (!ws_ok(ws, ws_bytes, l.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    float* per = (float*)(base + l.per);
    hipLaunchKernelGGL(k_ct_loss, dim3((unsigned)((dp->B + 3) / 4)), dim3(256), 0, s, (const float*)(base + l.h), dp->B, margin, scale, per, dist,
                       (float*)(base + l.dpre));
    NCX_HIP_TRY(hipGetLastError());
    NCX_HIP_TRY(colsum_rows((const float*)per, 4ll, dp->B, 4, losses4, s));
    return NCX_OK;
}

extern "C" int ncx_contrastive_backward(const ncx_contrastive_dims* dp, const ncx_inputs* in, void* ws, size_t ws_bytes, const float* dh,
                                        float* gw, float* gb, void* stream_) {
    if (!dp || !in || !ws || !gw || !gb) return NCX_E_NULL;
    if (!in->feats) return NCX_E_NULL;
    if (!ct_dims_ok(dp)) return NCX_E_DIMS;
    const ncx_contrastive_dims& d = *dp;
    const CtLayout l = ct_layout(d);
    if (!ws_ok(ws, ws_bytes, l.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    const long long M = (long long)d.B * d.P;
    float* dpre = (float*)(base + l.dpre);
    if (dh) {
        if ((uintptr_t)dh & 15) return NCX_E_DIMS;
        const long long n4 = M * CT_H / 4;
        hipLaunchKernelGGL(k_ct_mask, dim3((unsigned)((n4 + 255) / 256)), dim3(256), 0, s, dh, (const float*)(base + l.h), n4, dpre);
        NCX_HIP_TRY(hipGetLastError());
    }
    CtPtrs q{};
    q.feats = in->feats; q.idx = (int*)(base + l.idx); q.zall = (float*)(base + l.zall); q.dpre = dpre; q.gW = gw;
    GemmPlan pl;
    GemmArgs a = ct_gemm_dw(d, q, &pl);
    int rc = run_gemm_planned(a, FORM_TN, pl, (float*)(base + l.slab), l.slab_bytes, nullptr, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows((const float*)dpre, (long long)CT_H, (int)M, CT_H, gb, s));
    return NCX_OK;
}
