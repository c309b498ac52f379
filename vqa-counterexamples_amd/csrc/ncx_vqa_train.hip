// ncx_vqa_train.hip -- the trainable MutanNoAtt VQA model below the question encoder: training-mode forward, cross-entropy head and
// backward (reference vqa/lib/engine.py:6-56, train.py:136-145; MutanFusion.forward vqa/models/fusion.py:78-121, AbstractNoAtt._classif
// vqa/models/noatt.py:24-29).  One image per question: row b reads feats[img_idx[b]].
//
// Forward (7 launches + split fix-ups):
//   k_vt_drop   vd [B, dv] = drop_v(feats[img_idx]), qd [B, dq] = drop_q(q_emb)                (F.dropout, fusion.py:82, 88)
//   NT x 2      x_v = act_v(vd Wv^T + bv), x_q = act_q(qd Wq^T + bq)                            (fusion.py:83-93)
//   NT x 2      Hv = x_v Whv^T + bhv, Hq = x_q Whq^T + bhq, both [B, R dz] and kept            (fusion.py:96-107, all R at once)
//   k_vt_fuse   z = sum_r Hv_r * Hq_r;  z_c = drop_c(z)                                         (fusion.py:108-115, noatt.py:27)
//   NT          logits = z_c Wc^T + bc                                                          (noatt.py:28)
// Backward, given dlogits (ncx_ce_loss) (15 launches, 16 with dq_emb, + split fix-ups):
//   TN, colsum  dWc = dlogits^T z_c, dbc
//   NN          dz = (dlogits Wc) * mask_c: the dropout epilogue of the engine regenerates (or reads) the forward's mask
//   k_vt_dh     dHv_r = dz * Hq_r, dHq_r = dz * Hv_r
//   TN group    dWhv = dHv^T x_v | dWhq = dHq^T x_q (one launch);  colsum x 2: dbhv, dbhq
//   NN x 2      dx_v = dHv Whv, dx_q = dHq Whq;  k_vt_dact: dpre = dx (1 - x^2) where the activation is tanh
//   TN x 2      dWv = dpre_v^T vd, dWq = dpre_q^T qd;  colsum x 2: dbv, dbq
//   NN          dq_emb = (dpre_q Wq) * mask_q, on request (dropout epilogue again)
// Dropout: mode 1 is the counter-based generator of ncx_common.h with layer ids 1 (v), 2 (q), 3 (z) and element index r * width + c;
// nothing is stored but the dropped tensors themselves.  Mode 2 reads explicit keep masks [B dv | B dq | B dz].
// No atomics, every reduction in a fixed order: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ncx_internal.h"

namespace ncx {

enum VtGemm : int { VT_XV = 0, VT_XQ, VT_HV, VT_HQ, VT_LOGITS, VT_DWC, VT_DZ, VT_DWH, VT_DXV, VT_DXQ, VT_DWV, VT_DWQ, VT_DQ, VT_COUNT };
constexpr unsigned VT_LAYER_V = 1, VT_LAYER_Q = 2, VT_LAYER_C = 3;

struct VtLayout { size_t idx, vd, qd, xv, xq, hv, hq, zc, dzc, dhv, dhq, dxv, dxq, slab, slab_bytes, total; };
struct VtPtrs {
    const float *vd, *qd, *xv, *xq, *hv, *hq, *zc, *dzc, *dhv, *dhq, *dxv, *dxq, *dlogits, *masks;
    float *logits, *dq;
    ncx_mutan_grads g;
};

static int vt_check(const ncx_vqa_train_dims* d, const ncx_mutan_params* m) {
    if (!d || !m) return NCX_E_NULL;
    if (d->B < 1 || d->dv < 4 || d->dq < 4 || d->dz < 4 || d->A < 4 || d->n_img < 1) return NCX_E_DIMS;
    if (m->dhv < 4 || m->dhq < 4 || m->R < 1 || m->R > NCX_MAX_SEG) return NCX_E_DIMS;
    if (d->dropout_mode < 0 || d->dropout_mode > 2) return NCX_E_DIMS;
    const float ps[3] = {d->p_v, d->p_q, d->p_c};
    for (int i = 0; i < 3; ++i) if (!(ps[i] >= 0.f && ps[i] < 1.f)) return NCX_E_DIMS;
    const long long lim = 1ll << 31, B = d->B, RZ = (long long)m->R * d->dz;
    long long w = d->dv; if (d->dq > w) w = d->dq; if (RZ > w) w = RZ; if (d->A > w) w = d->A;
    long long h = m->dhv > m->dhq ? m->dhv : m->dhq;
    if (B * w >= lim || (long long)d->n_img * d->dv >= lim || (long long)d->A * d->dz >= lim || RZ * h >= lim ||
        h * (d->dv > d->dq ? d->dv : d->dq) >= lim) return NCX_E_DIMS;
    if ((m->act_v != 0 && m->act_v != 2) || (m->act_q != 0 && m->act_q != 2)) return NCX_E_FLAGS;
    return NCX_OK;
}

static void vt_dropout(EpiArgs& e, const ncx_vqa_train_dims& d, float p, unsigned layer, const float* mask, long long ld) {
    if (d.dropout_mode == 0 || (d.dropout_mode == 1 && p <= 0.f)) return;
    e.dropout = d.dropout_mode; e.drop_p = p; e.drop_scale = 1.f / (1.f - p);
    e.seed_lo = (unsigned)(d.seed & 0xFFFFFFFFull); e.seed_hi = (unsigned)(d.seed >> 32); e.layer = layer;
    e.keep_mask = mask; e.ld_mask = ld;
}

// The products of the step on the generic engine (pointers may be NULL when only sizing the slab).
static GemmArgs vt_gemm(const ncx_vqa_train_dims& d, const ncx_mutan_params& m, const VtPtrs& p, int which, int* form, GemmPlan* pl) {
    const int B = d.B, RZ = m.R * d.dz;
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
    auto nn = [&](const float* D, int K, const float* W, int N, float* out) {                  // out [B, N] = D [B, K] . W [K, N]
        a.mode = MODE_CHAIN; a.nseg = 1; a.M = B;
        a.a[0] = x_plain(D, K, B, K); a.b[0] = x_plain(W, N, K, N); a.klen[0] = K;
        a.out[0] = out; a.ldo[0] = N; a.n_cols[0] = N;
        *form = FORM_NN; *pl = plan_gemm(FORM_NN, B, N, ksteps(K), false);
    };
    auto unsplit = [&]() { a.split[0] = 1; pl->split = 1; };                                   // the dropout epilogue does not split
    const float* mk = p.masks;
    switch (which) {
    case VT_XV: nt(p.vd, d.dv, m.wv, m.dhv, (float*)p.xv, m.act_v); break;
    case VT_XQ: nt(p.qd, d.dq, m.wq, m.dhq, (float*)p.xq, m.act_q); break;
    case VT_HV: nt(p.xv, m.dhv, m.whv, RZ, (float*)p.hv, 0); break;
    case VT_HQ: nt(p.xq, m.dhq, m.whq, RZ, (float*)p.hq, 0); break;
    case VT_LOGITS: nt(p.zc, d.dz, m.wc, d.A, p.logits, 0); break;
    case VT_DWC: tn(0, p.dlogits, d.A, p.zc, d.dz, p.g.wc); *pl = plan_gemm(FORM_TN, d.A, d.dz, ksteps(B), false); break;
    case VT_DZ:
        nn(p.dlogits, d.A, m.wc, d.dz, (float*)p.dzc); unsplit();
        vt_dropout(a.epi, d, d.p_c, VT_LAYER_C, mk ? mk + (long long)B * (d.dv + d.dq) : nullptr, d.dz);
        break;
    case VT_DWH:
        tn(0, p.dhv, RZ, p.xv, m.dhv, p.g.whv); tn(1, p.dhq, RZ, p.xq, m.dhq, p.g.whq);
        *pl = plan_gemm(FORM_TN, RZ, m.dhv + m.dhq, ksteps(B), false);
        break;
    case VT_DXV: nn(p.dhv, RZ, m.whv, m.dhv, (float*)p.dxv); break;
    case VT_DXQ: nn(p.dhq, RZ, m.whq, m.dhq, (float*)p.dxq); break;
    case VT_DWV: tn(0, p.dxv, m.dhv, p.vd, d.dv, p.g.wv); *pl = plan_gemm(FORM_TN, m.dhv, d.dv, ksteps(B), false); break;
    case VT_DWQ: tn(0, p.dxq, m.dhq, p.qd, d.dq, p.g.wq); *pl = plan_gemm(FORM_TN, m.dhq, d.dq, ksteps(B), false); break;
    default:
        nn(p.dxq, m.dhq, m.wq, d.dq, p.dq); unsplit();
        vt_dropout(a.epi, d, d.p_q, VT_LAYER_Q, mk ? mk + (long long)B * d.dv : nullptr, d.dq);
        break;
    }
    return a;
}

static VtLayout vt_layout(const ncx_vqa_train_dims& d, const ncx_mutan_params& m) {
    VtLayout w{}; size_t o = 0;
    const size_t B = d.B, RZ = (size_t)m.R * d.dz;
    auto take = [&](size_t bytes) { const size_t r = o; o = align_up(o + bytes, 256); return r; };
    w.idx = take(B * 4); w.vd = take(B * d.dv * 4); w.qd = take(B * d.dq * 4);
    w.xv = take(B * m.dhv * 4); w.xq = take(B * m.dhq * 4); w.hv = take(B * RZ * 4); w.hq = take(B * RZ * 4);
    w.zc = take(B * d.dz * 4); w.dzc = take(B * d.dz * 4); w.dhv = take(B * RZ * 4); w.dhq = take(B * RZ * 4);
    w.dxv = take(B * m.dhv * 4); w.dxq = take(B * m.dhq * 4);
    VtPtrs p{}; size_t sb = 0;
    for (int i = 0; i < VT_COUNT; ++i) {
        int form; GemmPlan pl;
        GemmArgs a = vt_gemm(d, m, p, i, &form, &pl);
        const size_t t = gemm_slab_bytes(a, pl);
        sb = t > sb ? t : sb;
    }
    w.slab = take(sb); w.slab_bytes = sb; w.total = o;
    return w;
}

static VtPtrs vt_ptrs(char* base, const VtLayout& w) {
    VtPtrs p{};
    p.vd = (float*)(base + w.vd); p.qd = (float*)(base + w.qd); p.xv = (float*)(base + w.xv); p.xq = (float*)(base + w.xq);
    p.hv = (float*)(base + w.hv); p.hq = (float*)(base + w.hq); p.zc = (float*)(base + w.zc); p.dzc = (float*)(base + w.dzc);
    p.dhv = (float*)(base + w.dhv); p.dhq = (float*)(base + w.dhq); p.dxv = (float*)(base + w.dxv); p.dxq = (float*)(base + w.dxq);
    return p;
}

static int vt_run(const ncx_vqa_train_dims& d, const ncx_mutan_params& m, const VtPtrs& p, int which, const float* bias, char* base,
                  const VtLayout& w, hipStream_t s) {
    int form; GemmPlan pl;
    GemmArgs a = vt_gemm(d, m, p, which, &form, &pl);
    return run_gemm_planned(a, form, pl, (float*)(base + w.slab), w.slab_bytes, bias, s);
}

struct VtDrop { int mode; float p_v, p_q, p_c; unsigned lo, hi; };
__device__ __forceinline__ bool vt_keep(const VtDrop& k, unsigned layer, float p, const float* mask, long long i) {
    if (k.mode == 1) return dropout_keep(k.lo, k.hi, layer, (unsigned long long)i, p);
    if (k.mode == 2) return mask[i] != 0.f;
    return true;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// vd[b] = drop_v(feats[clamp(img_idx[b])]), qd[b] = drop_q(q_emb[b]): one element per thread, rows of dv + dq elements.
__global__ __launch_bounds__(256) void k_vt_drop(const float* __restrict__ feats, const int* __restrict__ img_idx, const float* __restrict__ q,
                                                 int B, int dv, int dq, int n_img, VtDrop k, const float* __restrict__ masks,
                                                 int* __restrict__ idx_c, float* __restrict__ vd, float* __restrict__ qd) {
    const long long i = blockIdx.x * 256ll + threadIdx.x, W = (long long)dv + dq;
    if (i >= (long long)B * W) return;
    const int b = (int)(i / W), c = (int)(i - (long long)b * W);
    if (c < dv) {
        int row = img_idx[b];
        row = row < 0 ? 0 : row >= n_img ? n_img - 1 : row;
        if (c == 0) idx_c[b] = row;
        const long long e = (long long)b * dv + c;
        const bool keep = k.p_v > 0.f || k.mode == 2 ? vt_keep(k, VT_LAYER_V, k.p_v, masks, e) : true;
        vd[e] = keep ? feats[(long long)row * dv + c] * (1.f / (1.f - k.p_v)) : 0.f;
    } else {
        const long long e = (long long)b * dq + (c - dv);
        const bool keep = k.p_q > 0.f || k.mode == 2 ? vt_keep(k, VT_LAYER_Q, k.p_q, masks ? masks + (long long)B * dv : nullptr, e) : true;
        qd[e] = keep ? q[e] * (1.f / (1.f - k.p_q)) : 0.f;
    }
}

// z[b][j] = sum_r Hv[b][r dz + j] Hq[b][r dz + j] (r ascending); zc = drop_c(z)
__global__ __launch_bounds__(256) void k_vt_fuse(const float* __restrict__ hv, const float* __restrict__ hq, int B, int dz, int R, VtDrop k,
                                                 const float* __restrict__ mask_c, float* __restrict__ z, float* __restrict__ zc) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (long long)B * dz) return;
    const int b = (int)(i / dz), j = (int)(i - (long long)b * dz);
    const long long row = (long long)b * R * dz + j;
    float acc = 0.f;
    for (int r = 0; r < R; ++r) acc = fmaf(hv[row + (long long)r * dz], hq[row + (long long)r * dz], acc);
    z[i] = acc;
    const bool keep = k.p_c > 0.f || k.mode == 2 ? vt_keep(k, VT_LAYER_C, k.p_c, mask_c, i) : true;
    zc[i] = keep ? acc * (1.f / (1.f - k.p_c)) : 0.f;
}

// dHv = dz (broadcast over r) * Hq, dHq = dz * Hv
__global__ __launch_bounds__(256) void k_vt_dh(const float* __restrict__ dzc, const float* __restrict__ hv, const float* __restrict__ hq, int B, int dz,
                                               int R, float* __restrict__ dhv, float* __restrict__ dhq) {
    const long long i = blockIdx.x * 256ll + threadIdx.x, RZ = (long long)R * dz;
    if (i >= (long long)B * RZ) return;
    const int b = (int)(i / RZ), j = (int)((i - (long long)b * RZ) % dz);
    const float g = dzc[(long long)b * dz + j];
    dhv[i] = g * hq[i];
    dhq[i] = g * hv[i];
}

// dpre = dx (1 - x^2) in place, for the sides whose activation is tanh
__global__ __launch_bounds__(256) void k_vt_dact(float* __restrict__ dxv, const float* __restrict__ xv, long long nv, int act_v,
                                                 float* __restrict__ dxq, const float* __restrict__ xq, long long nq, int act_q) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < nv) {
        if (act_v == 2) { const float x = xv[i]; dxv[i] *= 1.f - x * x; }
    } else if (i < nv + nq) {
        const long long e = i - nv;
        if (act_q == 2) { const float x = xq[e]; dxq[e] *= 1.f - x * x; }
    }
}

// Mean cross-entropy over A answers: one workgroup per example.  rows[b] = CE_b scale, rows[B + b] (as int) = hit bits (1: top-1, 2: top-5).
__device__ __forceinline__ float vt_block_max(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float vt_block_sum(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_ce_rows(const float* __restrict__ logits, const int* __restrict__ target, int B, int A, float scale,
                                                 float* __restrict__ dlogits, float* __restrict__ rows, int* __restrict__ bad) {
    __shared__ float red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* x = logits + (long long)b * A;
    const int tg = target[b];
    const bool ok = tg >= 0 && tg < A;
    if (!ok) {                                           // never used as an address: the row contributes nothing
        if (t == 0) { *bad = 1; rows[b] = 0.f; ((int*)rows)[B + b] = 0; }
        if (dlogits) for (int c = t; c < A; c += 256) dlogits[(long long)b * A + c] = 0.f;
        return;
    }
    const float xt = x[tg];
    float mx = -INFINITY; int ahead = 0;
    for (int c = t; c < A; c += 256) {
        const float v = x[c];
        mx = fmaxf(mx, v);
        ahead += (v > xt || (v == xt && c < tg)) ? 1 : 0;
    }
    mx = vt_block_max(mx, red);
    float se = 0.f;
    for (int c = t; c < A; c += 256) se += __expf(x[c] - mx);
    se = vt_block_sum(se, red);
    const int rank = (int)vt_block_sum((float)ahead, red);
    if (dlogits) {
        const float inv = 1.f / se;
        for (int c = t; c < A; c += 256) dlogits[(long long)b * A + c] = (__expf(x[c] - mx) * inv - (c == tg ? 1.f : 0.f)) * scale;
    }
    if (t == 0) {
        rows[b] = (logf(se) - (xt - mx)) * scale;              // (xt - mx first: the row's offset never meets the small log term)
        ((int*)rows)[B + b] = (rank < 1 ? 1 : 0) | (rank < 5 ? 2 : 0);
    }
}
// loss = sum_b rows[b]; the hit counts: single workgroup, fixed order
__global__ __launch_bounds__(256) void k_ce_finish(const float* __restrict__ rows, int B, float* __restrict__ loss, int* __restrict__ h1,
                                                   int* __restrict__ h5) {
    __shared__ float red[4];
    float acc = 0.f, c1 = 0.f, c5 = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) {
        acc += rows[i];
        const int bits = ((const int*)rows)[B + i];
        c1 += (float)(bits & 1); c5 += (float)((bits >> 1) & 1);
    }
    acc = vt_block_sum(acc, red); c1 = vt_block_sum(c1, red); c5 = vt_block_sum(c5, red);
    if (threadIdx.x == 0) {
        if (loss) loss[0] = acc;
        if (h1) h1[0] = (int)c1;
        if (h5) h5[0] = (int)c5;
    }
}

}  // namespace ncx

using namespace ncx;

static inline unsigned vt_grid(long long n) { return (unsigned)((n + 255) / 256); }
static VtDrop vt_drop_args(const ncx_vqa_train_dims& d) {
    VtDrop k{};
    k.mode = d.dropout_mode;
    if (k.mode) { k.p_v = d.p_v; k.p_q = d.p_q; k.p_c = d.p_c; }
    k.lo = (unsigned)(d.seed & 0xFFFFFFFFull); k.hi = (unsigned)(d.seed >> 32);
    return k;
}

extern "C" size_t ncx_vqa_train_workspace_bytes(const ncx_vqa_train_dims* d, const ncx_mutan_params* m) {
    if (vt_check(d, m) != NCX_OK) return 0;
    return vt_layout(*d, *m).total;
}

extern "C" int ncx_vqa_train_ws_region(const ncx_vqa_train_dims* d, const ncx_mutan_params* m, int32_t which, size_t* offset, size_t* bytes) {
    if (!offset || !bytes) return NCX_E_NULL;
    const int rc = vt_check(d, m);
    if (rc != NCX_OK) return rc;
    const VtLayout w = vt_layout(*d, *m);
    const size_t B = d->B;
    if (which == NCX_VT_WS_VD) { *offset = w.vd; *bytes = B * d->dv * 4; }
    else if (which == NCX_VT_WS_QD) { *offset = w.qd; *bytes = B * d->dq * 4; }
    else if (which == NCX_VT_WS_ZC) { *offset = w.zc; *bytes = B * d->dz * 4; }
    else return NCX_E_FLAGS;
    return NCX_OK;
}

static bool vt_params_null(const ncx_mutan_params* m) {
    return !m->wv || !m->bv || !m->wq || !m->bq || !m->whv || !m->bhv || !m->whq || !m->bhq || !m->wc || !m->bc;
}

extern "C" int ncx_vqa_train_forward(const ncx_vqa_train_dims* dp, const float* feats, const int32_t* img_idx, const float* q_emb,
                                     const ncx_mutan_params* mp, const float* masks, void* ws, size_t ws_bytes, float* logits, float* z,
                                     void* stream_) {
    if (!dp || !mp || !feats || !img_idx || !q_emb || !ws || !logits || !z || vt_params_null(mp)) return NCX_E_NULL;
    int rc = vt_check(dp, mp);
    if (rc != NCX_OK) return rc;
    const ncx_vqa_train_dims& d = *dp; const ncx_mutan_params& m = *mp;
    if (d.dropout_mode == 2 && !masks) return NCX_E_NULL;
    const VtLayout w = vt_layout(d, m);
    if (ws_bytes < w.total || ((uintptr_t)ws & 255)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    VtPtrs p = vt_ptrs(base, w);
    p.logits = logits; p.masks = d.dropout_mode == 2 ? masks : nullptr;
    const VtDrop k = vt_drop_args(d);
    hipLaunchKernelGGL(k_vt_drop, dim3(vt_grid((long long)d.B * (d.dv + d.dq))), dim3(256), 0, s, feats, img_idx, q_emb, d.B, d.dv, d.dq, d.n_img,
                       k, p.masks, (int*)(base + w.idx), (float*)p.vd, (float*)p.qd);
    NCX_HIP_TRY(hipGetLastError());
    rc = vt_run(d, m, p, VT_XV, m.bv, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_XQ, m.bq, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_HV, m.bhv, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_HQ, m.bhq, base, w, s); if (rc) return rc;
    hipLaunchKernelGGL(k_vt_fuse, dim3(vt_grid((long long)d.B * d.dz)), dim3(256), 0, s, p.hv, p.hq, d.B, d.dz, m.R, k,
                       p.masks ? p.masks + (long long)d.B * (d.dv + d.dq) : nullptr, z, (float*)p.zc);
    NCX_HIP_TRY(hipGetLastError());
    return vt_run(d, m, p, VT_LOGITS, m.bc, base, w, s);
}

extern "C" int ncx_vqa_train_backward(const ncx_vqa_train_dims* dp, const ncx_mutan_params* mp, const float* masks, void* ws, size_t ws_bytes,
                                      const float* dlogits, const ncx_mutan_grads* g, float* dq_emb, void* stream_) {
    if (!dp || !mp || !ws || !dlogits || !g || vt_params_null(mp)) return NCX_E_NULL;
    if (!g->wv || !g->bv || !g->wq || !g->bq || !g->whv || !g->bhv || !g->whq || !g->bhq || !g->wc || !g->bc) return NCX_E_NULL;
    int rc = vt_check(dp, mp);
    if (rc != NCX_OK) return rc;
    const ncx_vqa_train_dims& d = *dp; const ncx_mutan_params& m = *mp;
    if ((d.dropout_mode == 2 && !masks) || (d.want_dq && !dq_emb)) return NCX_E_NULL;
    const VtLayout w = vt_layout(d, m);
    if (ws_bytes < w.total || ((uintptr_t)ws & 255)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    VtPtrs p = vt_ptrs(base, w);
    p.dlogits = dlogits; p.masks = d.dropout_mode == 2 ? masks : nullptr; p.g = *g; p.dq = dq_emb;
    const int RZ = m.R * d.dz;
    rc = vt_run(d, m, p, VT_DWC, nullptr, base, w, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows(dlogits, (long long)d.A, d.B, d.A, g->bc, s));
    rc = vt_run(d, m, p, VT_DZ, nullptr, base, w, s); if (rc) return rc;
    hipLaunchKernelGGL(k_vt_dh, dim3(vt_grid((long long)d.B * RZ)), dim3(256), 0, s, p.dzc, p.hv, p.hq, d.B, d.dz, m.R, (float*)p.dhv, (float*)p.dhq);
    NCX_HIP_TRY(hipGetLastError());
    rc = vt_run(d, m, p, VT_DWH, nullptr, base, w, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows(p.dhv, (long long)RZ, d.B, RZ, g->bhv, s));
    NCX_HIP_TRY(colsum_rows(p.dhq, (long long)RZ, d.B, RZ, g->bhq, s));
    rc = vt_run(d, m, p, VT_DXV, nullptr, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_DXQ, nullptr, base, w, s); if (rc) return rc;
    if (m.act_v == 2 || m.act_q == 2) {
        const long long nv = (long long)d.B * m.dhv, nq = (long long)d.B * m.dhq;
        hipLaunchKernelGGL(k_vt_dact, dim3(vt_grid(nv + nq)), dim3(256), 0, s, (float*)p.dxv, p.xv, nv, m.act_v, (float*)p.dxq, p.xq, nq, m.act_q);
        NCX_HIP_TRY(hipGetLastError());
    }
    rc = vt_run(d, m, p, VT_DWV, nullptr, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_DWQ, nullptr, base, w, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows(p.dxv, (long long)m.dhv, d.B, m.dhv, g->bv, s));
    NCX_HIP_TRY(colsum_rows(p.dxq, (long long)m.dhq, d.B, m.dhq, g->bq, s));
    if (d.want_dq) { rc = vt_run(d, m, p, VT_DQ, nullptr, base, w, s); if (rc) return rc; }
    return NCX_OK;
}

extern "C" int ncx_ce_loss(const float* logits, const int32_t* target, int32_t B, int32_t A, float scale, float* loss, float* dlogits,
                           int32_t* hits_top1, int32_t* hits_top5, int32_t* bad_flag, float* rows, void* stream_) {
    if (!logits || !target || !bad_flag || !rows) return NCX_E_NULL;
    if (B < 1 || A < 1 || (long long)B * A >= (1ll << 31)) return NCX_E_DIMS;
    hipStream_t s = (hipStream_t)stream_;
    if (scale <= 0.f) scale = 1.f / (float)B;
    hipLaunchKernelGGL(k_ce_rows, dim3(B), dim3(256), 0, s, logits, target, B, A, scale, dlogits, rows, bad_flag);
    NCX_HIP_TRY(hipGetLastError());
    if (loss || hits_top1 || hits_top5) {
        hipLaunchKernelGGL(k_ce_finish, dim3(1), dim3(256), 0, s, (const float*)rows, B, loss, hits_top1, hits_top5);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}
