// ncx_mlb_train.hip -- the trainable MLBNoAtt VQA model below the question encoder: training-mode forward and backward (reference
// MLBFusion.forward vqa/models/fusion.py:31-50, AbstractNoAtt._classif vqa/models/noatt.py:24-29; the step itself vqa/lib/engine.py:6-56).
// One image per question: row b reads feats[img_idx[b]].  The loss is ncx_ce_loss, the optimiser ncx_adam_step (ncx_vqa_train.hip,
// ncx_loss_adam.hip): the sibling of the MutanNoAtt trainer, with the same dims struct, dropout modes and workspace rules.
//
// Forward (5 launches + split fix-ups):
//   k_mt_drop   vd [B, dv] = drop_v(feats[img_idx]), qd [B, dq] = drop_q(q_emb)                 (F.dropout, fusion.py:34, 42)
//   NT x 2      x_v = act_v(vd Wv^T + bv), x_q = act_q(qd Wq^T + bq), both [B, dh] and kept     (fusion.py:35-47)
//   k_mt_fuse   z = x_q * x_v;  t = act_c(z) (stored only when act_c is tanh);  tc = drop_c(t)  (fusion.py:49, noatt.py:25-27)
//   NT          logits = tc Wc^T + bc                                                           (noatt.py:28)
// Backward, given dlogits (ncx_ce_loss) (5 launches, 6 with dq_emb, + split fix-ups):
//   TN          dWc = dlogits^T tc
//   NN          dt = (dlogits Wc) * mask_c: the dropout epilogue of the engine regenerates (or reads) the forward's mask
//   k_mt_dfuse  dz = dt (1 - t^2);  dpv = dz x_q (1 - x_v^2);  dpq = dz x_v (1 - x_q^2)  (each tanh factor only where that activation is tanh)
//   TN group    dWv = dpv^T vd | dWq = dpq^T qd (one launch)
//   k_mt_colsum dbc = sum_b dlogits, dbv = sum_b dpv, dbq = sum_b dpq (one launch for the three)
//   NN          dq_emb = (dpq Wq) * mask_q, on request (dropout epilogue again)
// The three element-wise kernels move 16 bytes per lane where widths and pointers allow it, one element otherwise.  No transcendental
// sits on a GEMM's load side: tanh runs in the NT epilogues and once in k_mt_fuse, the backward multiplies by stored values.
// Dropout: mode 1 is the counter-based generator of ncx_common.h with layer ids 1 (v), 2 (q), 3 (the classifier's input) and element
// index r * width + c; nothing is stored but the dropped tensors themselves.  Mode 2 reads explicit keep masks [B dv | B dq | B dh].
// No atomics, every reduction in a fixed order: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ncx_internal.h"

namespace ncx {

enum MtGemm : int { MT_XV = 0, MT_XQ, MT_LOGITS, MT_DWC, MT_DT, MT_DWVQ, MT_DQ, MT_COUNT };
constexpr unsigned MT_LAYER_V = 1, MT_LAYER_Q = 2, MT_LAYER_C = 3;

struct MtLayout { size_t vd, qd, xv, xq, t, tc, dt, dpv, dpq, slab, slab_bytes, total; };
struct MtPtrs {
    const float *vd, *qd, *xv, *xq, *t, *tc, *dt, *dpv, *dpq, *dlogits, *masks;
    float *logits, *dq;
    ncx_mlb_grads g;
};

static int mt_check(const ncx_vqa_train_dims* d, const ncx_mlb_params* m) {
    if (!d || !m) return NCX_E_NULL;
    if (d->B < 1 || d->dv < 4 || d->dq < 4 || d->dz < 4 || d->A < 4 || d->n_img < 1) return NCX_E_DIMS;
    if (m->dh != d->dz) return NCX_E_DIMS;
    if (d->dropout_mode < 0 || d->dropout_mode > 2) return NCX_E_DIMS;
    const float ps[3] = {d->p_v, d->p_q, d->p_c};
    for (int i = 0; i < 3; ++i) if (!(ps[i] >= 0.f && ps[i] < 1.f)) return NCX_E_DIMS;
    const long long lim = 1ll << 31, B = d->B;
    long long w = d->dv; if (d->dq > w) w = d->dq; if (d->dz > w) w = d->dz; if (d->A > w) w = d->A;
    if (B * w >= lim || (long long)d->n_img * d->dv >= lim || (long long)d->A * d->dz >= lim ||
        (long long)d->dz * (d->dv > d->dq ? d->dv : d->dq) >= lim) return NCX_E_DIMS;
    const int acts[3] = {m->act_v, m->act_q, m->act_c};
    for (int i = 0; i < 3; ++i) if (acts[i] != 0 && acts[i] != 2) return NCX_E_FLAGS;
    return NCX_OK;
}

static void mt_dropout(EpiArgs& e, const ncx_vqa_train_dims& d, float p, unsigned layer, const float* mask, long long ld) {
    if (d.dropout_mode == 0 || (d.dropout_mode == 1 && p <= 0.f)) return;
    e.dropout = d.dropout_mode; e.drop_p = p; e.drop_scale = 1.f / (1.f - p);
    e.seed_lo = (unsigned)(d.seed & 0xFFFFFFFFull); e.seed_hi = (unsigned)(d.seed >> 32); e.layer = layer;
    e.keep_mask = mask; e.ld_mask = ld;
}

// The products of the step on the generic engine (pointers may be NULL when only sizing the slab).
static GemmArgs mt_gemm(const ncx_vqa_train_dims& d, const ncx_mlb_params& m, const MtPtrs& p, int which, int* form, GemmPlan* pl) {
    const int B = d.B, dh = d.dz;
    GemmArgs a{};
    auto nt = [&](const float* X, int K, const float* W, int N, float* out, int act) {        // out [B, N] = act(X [B, K] . W [N, K]^T + bias)
        a.mode = MODE_CHAIN; a.nseg = 1; a.M = B;
        a.a[0] = x_plain(X, K, B, K); a.b[0] = x_plain(W, K, N, K); a.klen[0] = K;
        a.out[0] = out; a.ldo[0] = N; a.n_cols[0] = N; a.epi.relu = act;
        *form = FORM_NT; *pl = plan_gemm(FORM_NT, B, N, ksteps(K), true);
    };
    auto tn = [&](int i, const float* D, int Mo, const float* X, int N, float* out) {          // out [Mo, N] = D [B, Mo]^T . X [B, N]
        a.mode = MODE_GROUP; a.nseg = i + 1; a.M = Mo;
        a.a[i] = x_plain(D, Mo, B, Mo); a.b[i] = x_plain(X, N, B, N); a.klen[i] = B;
        a.out[i] = out; a.ldo[i] = N; a.n_cols[i] = N;
        *form = FORM_TN;
    };
    auto nn = [&](const float* D, int K, const float* W, int N, float* out) {                  // out [B, N] = D [B, K] . W [K, N], unsplit:
        a.mode = MODE_CHAIN; a.nseg = 1; a.M = B;                                              // the dropout epilogue does not split
        a.a[0] = x_plain(D, K, B, K); a.b[0] = x_plain(W, N, K, N); a.klen[0] = K;
        a.out[0] = out; a.ldo[0] = N; a.n_cols[0] = N;
        *form = FORM_NN; *pl = plan_gemm(FORM_NN, B, N, ksteps(K), false);
        a.split[0] = 1; pl->split = 1;
    };
    const float* mk = p.masks;
    switch (which) {
    case MT_XV: nt(p.vd, d.dv, m.wv, dh, (float*)p.xv, m.act_v); break;
    case MT_XQ: nt(p.qd, d.dq, m.wq, dh, (float*)p.xq, m.act_q); break;
    case MT_LOGITS: nt(p.tc, dh, m.wc, d.A, p.logits, 0); break;
    case MT_DWC: tn(0, p.dlogits, d.A, p.tc, dh, p.g.wc); *pl = plan_gemm(FORM_TN, d.A, dh, ksteps(B), false); break;
    case MT_DT:
        nn(p.dlogits, d.A, m.wc, dh, (float*)p.dt);
        mt_dropout(a.epi, d, d.p_c, MT_LAYER_C, mk ? mk + (long long)B * (d.dv + d.dq) : nullptr, dh);
        break;
    case MT_DWVQ:
        tn(0, p.dpv, dh, p.vd, d.dv, p.g.wv); tn(1, p.dpq, dh, p.qd, d.dq, p.g.wq);
        *pl = plan_gemm(FORM_TN, dh, (long long)d.dv + d.dq, ksteps(B), false);
        break;
    default:
        nn(p.dpq, dh, m.wq, d.dq, p.dq);
        mt_dropout(a.epi, d, d.p_q, MT_LAYER_Q, mk ? mk + (long long)B * d.dv : nullptr, d.dq);
        break;
    }
    return a;
}

static MtLayout mt_layout(const ncx_vqa_train_dims& d, const ncx_mlb_params& m) {
    MtLayout w{}; size_t o = 0;
    const size_t B = d.B, dh = d.dz;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    w.vd = take(B * d.dv * 4); w.qd = take(B * d.dq * 4);
    w.xv = take(B * dh * 4); w.xq = take(B * dh * 4);
    w.t = take(m.act_c == 2 ? B * dh * 4 : 0); w.tc = take(B * dh * 4);
    w.dt = take(B * dh * 4); w.dpv = take(B * dh * 4); w.dpq = take(B * dh * 4);
    MtPtrs p{}; size_t sb = 0;
    for (int i = 0; i < MT_COUNT; ++i) {
        int form; GemmPlan pl;
        GemmArgs a = mt_gemm(d, m, p, i, &form, &pl);
        const size_t t = gemm_slab_bytes(a, pl);
        sb = t > sb ? t : sb;
    }
    w.slab = take(sb); w.slab_bytes = sb; w.total = o;
    return w;
}

static MtPtrs mt_ptrs(char* base, const MtLayout& w, const ncx_mlb_params& m) {
    MtPtrs p{};
    p.vd = (float*)(base + w.vd); p.qd = (float*)(base + w.qd); p.xv = (float*)(base + w.xv); p.xq = (float*)(base + w.xq);
    p.t = m.act_c == 2 ? (float*)(base + w.t) : nullptr; p.tc = (float*)(base + w.tc);
    p.dt = (float*)(base + w.dt); p.dpv = (float*)(base + w.dpv); p.dpq = (float*)(base + w.dpq);
    return p;
}

static int mt_run(const ncx_vqa_train_dims& d, const ncx_mlb_params& m, const MtPtrs& p, int which, const float* bias, char* base,
                  const MtLayout& w, hipStream_t s) {
    int form; GemmPlan pl;
    GemmArgs a = mt_gemm(d, m, p, which, &form, &pl);
    return run_gemm_planned(a, form, pl, (float*)(base + w.slab), w.slab_bytes, bias, s);
}

struct MtDrop { int mode; float p_v, p_q, p_c; unsigned lo, hi; };
__device__ __forceinline__ bool mt_keep(const MtDrop& k, unsigned layer, float p, const float* mask, long long i) {
    if (k.mode == 1) return p > 0.f ? dropout_keep(k.lo, k.hi, layer, (unsigned long long)i, p) : true;
    if (k.mode == 2) return mask[i] != 0.f;
    return true;
}

// V consecutive floats: one 16-byte access when V == 4 (the caller has checked widths and alignment), one element when V == 1
template <int V> struct MtVec { float v[V]; };
template <int V> __device__ __forceinline__ MtVec<V> mt_ld(const float* p) {
    MtVec<V> r;
    if constexpr (V == 4) { const f32x4 t = *(const f32x4*)p; r.v[0] = t[0]; r.v[1] = t[1]; r.v[2] = t[2]; r.v[3] = t[3]; }
    else r.v[0] = p[0];
    return r;
}
template <int V> __device__ __forceinline__ void mt_st(float* p, const MtVec<V>& x) {
    if constexpr (V == 4) { f32x4 t; t[0] = x.v[0]; t[1] = x.v[1]; t[2] = x.v[2]; t[3] = x.v[3]; *(f32x4*)p = t; }
    else p[0] = x.v[0];
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// vd[b] = drop_v(feats[clamp(img_idx[b])]), qd[b] = drop_q(q_emb[b]): V elements per thread, rows of (dv + dq) / V groups.
template <int V>
__global__ __launch_bounds__(256) void k_mt_drop(const float* __restrict__ feats, const int* __restrict__ img_idx, const float* __restrict__ q,
                                                 int B, int dv, int dq, int n_img, MtDrop k, const float* __restrict__ masks,
                                                 float* __restrict__ vd, float* __restrict__ qd) {
    const int gv = dv / V, W = gv + dq / V;
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (long long)B * W) return;
    const int b = (int)(i / W), c = (int)(i - (long long)b * W);
    if (c < gv) {
        int row = img_idx[b];
        row = row < 0 ? 0 : row >= n_img ? n_img - 1 : row;
        const long long e = (long long)b * dv + c * V;
        MtVec<V> x = mt_ld<V>(feats + (long long)row * dv + c * V);
        const float sc = 1.f / (1.f - k.p_v);
#pragma unroll
        for (int j = 0; j < V; ++j) x.v[j] = mt_keep(k, MT_LAYER_V, k.p_v, masks, e + j) ? x.v[j] * sc : 0.f;
        mt_st<V>(vd + e, x);
    } else {
        const long long e = (long long)b * dq + (c - gv) * V;
        MtVec<V> x = mt_ld<V>(q + e);
        const float sc = 1.f / (1.f - k.p_q);
        const float* mq = masks ? masks + (long long)B * dv : nullptr;
#pragma unroll
        for (int j = 0; j < V; ++j) x.v[j] = mt_keep(k, MT_LAYER_Q, k.p_q, mq, e + j) ? x.v[j] * sc : 0.f;
        mt_st<V>(qd + e, x);
    }
}

// z = x_q * x_v;  t = tanh(z) when act_c == 2 (else t is z and is not stored);  tc = drop_c(t).  n = B dh elements, V per thread.
template <int V>
__global__ __launch_bounds__(256) void k_mt_fuse(const float* __restrict__ xv, const float* __restrict__ xq, long long n, int act_c, MtDrop k,
                                                 const float* __restrict__ mask_c, float* __restrict__ z, float* __restrict__ t, float* __restrict__ tc) {
    const long long i = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (i >= n) return;
    const MtVec<V> a = mt_ld<V>(xv + i), b = mt_ld<V>(xq + i);
    MtVec<V> zz, tt, cc;
    const float sc = 1.f / (1.f - k.p_c);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        zz.v[j] = b.v[j] * a.v[j];
        tt.v[j] = act_c == 2 ? tanhf(zz.v[j]) : zz.v[j];
        cc.v[j] = mt_keep(k, MT_LAYER_C, k.p_c, mask_c, i + j) ? tt.v[j] * sc : 0.f;
    }
    mt_st<V>(z + i, zz);
    if (act_c == 2) mt_st<V>(t + i, tt);
    mt_st<V>(tc + i, cc);
}

// dz = dt (1 - t^2);  dpv = dz x_q (1 - x_v^2);  dpq = dz x_v (1 - x_q^2): a tanh factor only where that activation is tanh
template <int V>
__global__ __launch_bounds__(256) void k_mt_dfuse(const float* __restrict__ dt, const float* __restrict__ t, const float* __restrict__ xv,
                                                  const float* __restrict__ xq, long long n, int act_v, int act_q, int act_c,
                                                  float* __restrict__ dpv, float* __restrict__ dpq) {
    const long long i = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (i >= n) return;
    const MtVec<V> g = mt_ld<V>(dt + i), a = mt_ld<V>(xv + i), b = mt_ld<V>(xq + i);
    MtVec<V> tt{};
    if (act_c == 2) tt = mt_ld<V>(t + i);
    MtVec<V> pv, pq;
#pragma unroll
    for (int j = 0; j < V; ++j) {
        const float dz = act_c == 2 ? g.v[j] * (1.f - tt.v[j] * tt.v[j]) : g.v[j];
        const float gv = dz * b.v[j], gq = dz * a.v[j];
        pv.v[j] = act_v == 2 ? gv * (1.f - a.v[j] * a.v[j]) : gv;
        pq.v[j] = act_q == 2 ? gq * (1.f - b.v[j] * b.v[j]) : gq;
    }
    mt_st<V>(dpv + i, pv);
    mt_st<V>(dpq + i, pq);
}

// out[c] = sum over rows r < B of in[r * cols + c], for up to three tensors in one launch.  A workgroup owns 32 columns of one tensor:
// wave w reads rows 2 w, 2 w + 1, then + 8, ... as two 128-byte row segments per load (coalesced, unlike one workgroup per column);
// thread (g, c) sums rows g, g + 8, ... in ascending order, the 8 partial sums are added in ascending g.  Fixed order, no atomics.
struct MtSum { const float* in; float* out; int cols; int blk0; };
struct MtSums { MtSum s[3]; int n; };
__global__ __launch_bounds__(256) void k_mt_colsum(MtSums js, int B) {
    __shared__ float red[8][32];
    int j = 0;
    for (int i = 1; i < js.n; ++i) if ((int)blockIdx.x >= js.s[i].blk0) j = i;
    const MtSum s = js.s[j];
    const int g = threadIdx.x >> 5, l = threadIdx.x & 31, c = ((int)blockIdx.x - s.blk0) * 32 + l;
    float acc = 0.f;
    if (c < s.cols)
        for (int r = g; r < B; r += 8) acc += s.in[(long long)r * s.cols + c];
    red[g][l] = acc;
    __syncthreads();
    if (g == 0 && c < s.cols) {
        float v = red[0][l];
#pragma unroll
        for (int i = 1; i < 8; ++i) v += red[i][l];
        s.out[c] = v;
    }
}

}  // namespace ncx

using namespace ncx;

static inline unsigned mt_grid(long long n) { return (unsigned)((n + 255) / 256); }
static inline bool mt_al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static MtDrop mt_drop_args(const ncx_vqa_train_dims& d) {
    MtDrop k{};
    k.mode = d.dropout_mode;
    if (k.mode) { k.p_v = d.p_v; k.p_q = d.p_q; k.p_c = d.p_c; }
    k.lo = (unsigned)(d.seed & 0xFFFFFFFFull); k.hi = (unsigned)(d.seed >> 32);
    return k;
}

extern "C" size_t ncx_mlb_train_workspace_bytes(const ncx_vqa_train_dims* d, const ncx_mlb_params* m) {
    if (mt_check(d, m) != NCX_OK) return 0;
    return mt_layout(*d, *m).total;
}

extern "C" int ncx_mlb_train_ws_region(const ncx_vqa_train_dims* d, const ncx_mlb_params* m, int32_t which, size_t* offset, size_t* bytes) {
    if (!offset || !bytes) return NCX_E_NULL;
    const int rc = mt_check(d, m);
    if (rc != NCX_OK) return rc;
    const MtLayout w = mt_layout(*d, *m);
    const size_t B = d->B;
    if (which == NCX_VT_WS_VD) { *offset = w.vd; *bytes = B * d->dv * 4; }
    else if (which == NCX_VT_WS_QD) { *offset = w.qd; *bytes = B * d->dq * 4; }
    else if (which == NCX_VT_WS_ZC) { *offset = w.tc; *bytes = B * d->dz * 4; }
    else return NCX_E_FLAGS;
    return NCX_OK;
}

static bool mt_params_null(const ncx_mlb_params* m) { return !m->wv || !m->bv || !m->wq || !m->bq || !m->wc || !m->bc; }

extern "C" int ncx_mlb_train_forward(const ncx_vqa_train_dims* dp, const float* feats, const int32_t* img_idx, const float* q_emb,
                                     const ncx_mlb_params* mp, const float* masks, void* ws, size_t ws_bytes, float* logits, float* z,
                                     void* stream_) {
    if (!dp || !mp || !feats || !img_idx || !q_emb || !ws || !logits || !z || mt_params_null(mp)) return NCX_E_NULL;
    int rc = mt_check(dp, mp);
    if (rc != NCX_OK) return rc;
    const ncx_vqa_train_dims& d = *dp; const ncx_mlb_params& m = *mp;
    if (d.dropout_mode == 2 && !masks) return NCX_E_NULL;
    const MtLayout w = mt_layout(d, m);
    if (ws_bytes < w.total || ((uintptr_t)ws & 255)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    MtPtrs p = mt_ptrs(base, w, m);
    p.logits = logits; p.masks = d.dropout_mode == 2 ? masks : nullptr;
    const MtDrop k = mt_drop_args(d);
    const long long n = (long long)d.B * d.dz;
    const float* mask_c = p.masks ? p.masks + (long long)d.B * (d.dv + d.dq) : nullptr;
    // 16-byte lanes: row widths that are multiples of 4 keep every group inside one row and every row 16-byte aligned
    if (d.dv % 4 == 0 && d.dq % 4 == 0 && mt_al16(feats) && mt_al16(q_emb))
        hipLaunchKernelGGL(k_mt_drop<4>, dim3(mt_grid((long long)d.B * ((d.dv + d.dq) / 4))), dim3(256), 0, s, feats, img_idx, q_emb, d.B, d.dv, d.dq,
                           d.n_img, k, p.masks, (float*)p.vd, (float*)p.qd);
    else
        hipLaunchKernelGGL(k_mt_drop<1>, dim3(mt_grid((long long)d.B * (d.dv + d.dq))), dim3(256), 0, s, feats, img_idx, q_emb, d.B, d.dv, d.dq,
                           d.n_img, k, p.masks, (float*)p.vd, (float*)p.qd);
    NCX_HIP_TRY(hipGetLastError());
    rc = mt_run(d, m, p, MT_XV, m.bv, base, w, s); if (rc) return rc;
    rc = mt_run(d, m, p, MT_XQ, m.bq, base, w, s); if (rc) return rc;
    if (n % 4 == 0 && mt_al16(z))
        hipLaunchKernelGGL(k_mt_fuse<4>, dim3(mt_grid(n / 4)), dim3(256), 0, s, p.xv, p.xq, n, m.act_c, k, mask_c, z, (float*)p.t, (float*)p.tc);
    else
        hipLaunchKernelGGL(k_mt_fuse<1>, dim3(mt_grid(n)), dim3(256), 0, s, p.xv, p.xq, n, m.act_c, k, mask_c, z, (float*)p.t, (float*)p.tc);
    NCX_HIP_TRY(hipGetLastError());
    return mt_run(d, m, p, MT_LOGITS, m.bc, base, w, s);
}

extern "C" int ncx_mlb_train_backward(const ncx_vqa_train_dims* dp, const ncx_mlb_params* mp, const float* masks, void* ws, size_t ws_bytes,
                                      const float* dlogits, const ncx_mlb_grads* g, float* dq_emb, void* stream_) {
    if (!dp || !mp || !ws || !dlogits || !g || mt_params_null(mp)) return NCX_E_NULL;
    if (!g->wv || !g->bv || !g->wq || !g->bq || !g->wc || !g->bc) return NCX_E_NULL;
    int rc = mt_check(dp, mp);
    if (rc != NCX_OK) return rc;
    const ncx_vqa_train_dims& d = *dp; const ncx_mlb_params& m = *mp;
    if ((d.dropout_mode == 2 && !masks) || (d.want_dq && !dq_emb)) return NCX_E_NULL;
    const MtLayout w = mt_layout(d, m);
    if (ws_bytes < w.total || ((uintptr_t)ws & 255)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    MtPtrs p = mt_ptrs(base, w, m);
    p.dlogits = dlogits; p.masks = d.dropout_mode == 2 ? masks : nullptr; p.g = *g; p.dq = dq_emb;
    const long long n = (long long)d.B * d.dz;
    rc = mt_run(d, m, p, MT_DWC, nullptr, base, w, s); if (rc) return rc;
    rc = mt_run(d, m, p, MT_DT, nullptr, base, w, s); if (rc) return rc;
    if (n % 4 == 0)                                      // every operand is a 256-byte aligned workspace region
        hipLaunchKernelGGL(k_mt_dfuse<4>, dim3(mt_grid(n / 4)), dim3(256), 0, s, p.dt, p.t, p.xv, p.xq, n, m.act_v, m.act_q, m.act_c, (float*)p.dpv,
                           (float*)p.dpq);
    else
        hipLaunchKernelGGL(k_mt_dfuse<1>, dim3(mt_grid(n)), dim3(256), 0, s, p.dt, p.t, p.xv, p.xq, n, m.act_v, m.act_q, m.act_c, (float*)p.dpv,
                           (float*)p.dpq);
    NCX_HIP_TRY(hipGetLastError());
    rc = mt_run(d, m, p, MT_DWVQ, nullptr, base, w, s); if (rc) return rc;
    MtSums js{};
    js.n = 3;
    js.s[0] = MtSum{dlogits, g->bc, d.A, 0};
    js.s[1] = MtSum{p.dpv, g->bv, d.dz, (d.A + 31) / 32};
    js.s[2] = MtSum{p.dpq, g->bq, d.dz, js.s[1].blk0 + (d.dz + 31) / 32};
    hipLaunchKernelGGL(k_mt_colsum, dim3(js.s[2].blk0 + (d.dz + 31) / 32), dim3(256), 0, s, js, d.B);
    NCX_HIP_TRY(hipGetLastError());
    if (d.want_dq) { rc = mt_run(d, m, p, MT_DQ, nullptr, base, w, s); if (rc) return rc; }
    return NCX_OK;
}
