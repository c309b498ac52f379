// ncx_mlb_train.hip -- the trainable MLBNoAtt VQA model below the question encoder: training-mode forward and backward (reference
// MLBFusion.forward vqa/models/fusion.py:31-50, AbstractNoAtt._classif vqa/models/noatt.py:24-29; the step itself vqa/lib/engine.py:6-56).
// One image per question: row b reads feats[img_idx[b]].  The loss is ncx_ce_loss, the optimiser ncx_adam_step (both
// ncx_loss_adam.hip): the sibling of the MutanNoAtt trainer, with the same dims struct, dropout modes and workspace rules.
//
// Forward (5 launches + split fix-ups):
//   drop_vq     vd [B, dv] = drop_v(feats[img_idx]), qd [B, dq] = drop_q(q_emb)                 (F.dropout, fusion.py:34, 42)
//   NT x 2      x_v = act_v(vd Wv^T + bv), x_q = act_q(qd Wq^T + bq), both [B, dh] and kept     (fusion.py:35-47)
//   k_mt_fuse   z = x_q * x_v;  t = act_c(z) (stored only when act_c is tanh);  tc = drop_c(t)  (fusion.py:49, noatt.py:25-27)
//   NT          logits = tc Wc^T + bc                                                           (noatt.py:28)
// Backward, given dlogits (ncx_ce_loss) (5 launches, 6 with dq_emb, + split fix-ups):
//   TN          dWc = dlogits^T tc
//   NN          dt = (dlogits Wc) * mask_c: the dropout epilogue of the engine regenerates (or reads) the forward's mask
//   dfuse       dz = dt (1 - t^2);  dpv = dz x_q (1 - x_v^2);  dpq = dz x_v (1 - x_q^2)  (each tanh factor only where that activation is tanh)
//   TN group    dWv = dpv^T vd | dWq = dpq^T qd (one launch)
//   k_mt_colsum dbc = sum_b dlogits, dbv = sum_b dpv, dbq = sum_b dpq (one launch for the three)
//   NN          dq_emb = (dpq Wq) * mask_q, on request (dropout epilogue again)
// drop_vq and dfuse are the shared kernels of ncx_train.hip (k_train_drop_vq, k_train_dfuse); the dropout front end, the GEMM request
// builders, the runner and the entry points' checks are ncx_train.h's.  What is here is the model: the products, the workspace, the
// launch order, k_mt_fuse and the bias sums.  The three element-wise kernels move 16 bytes per lane where widths and pointers allow
// it, one element otherwise.  No transcendental sits on a GEMM's load side: tanh runs in the NT epilogues and once in
// k_mt_fuse, the backward multiplies by stored values.
// Dropout: mode 1 is the counter-based generator of ncx_common.h with layer ids 1 (v), 2 (q), 3 (the classifier's input) and element
// index r * width + c; nothing is stored but the dropped tensors themselves.  Mode 2 reads explicit keep masks [B dv | B dq | B dh].
// No atomics, every reduction in a fixed order: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ncx_train.h"

namespace ncx {

enum MtGemm : int { MT_XV = 0, MT_XQ, MT_LOGITS, MT_DWC, MT_DT, MT_DWVQ, MT_DQ, MT_COUNT };

struct MtLayout { size_t vd, qd, xv, xq, t, tc, dt, dpv, dpq, slab, slab_bytes, total; };
struct MtPtrs {
    const float *vd, *qd, *xv, *xq, *t, *tc, *dt, *dpv, *dpq, *dlogits, *masks;
    float *logits, *dq;
    ncx_mlb_grads g;
};

static int mt_check(const ncx_vqa_train_dims* d, const ncx_mlb_params* m) {
    if (!d || !m) return NCX_E_NULL;
    const int rc = vq_check_dims(d);
    if (rc != NCX_OK) return rc;
    if (m->dh != d->dz) return NCX_E_DIMS;
    if ((long long)d->dz * (d->dv > d->dq ? d->dv : d->dq) >= (1ll << 31)) return NCX_E_DIMS;
    const int acts[3] = {m->act_v, m->act_q, m->act_c};
    for (int i = 0; i < 3; ++i) if (acts[i] != 0 && acts[i] != 2) return NCX_E_FLAGS;
    return NCX_OK;
}

// The products of the step on the generic engine (pointers may be NULL when only sizing the slab).
static GemmReq mt_gemm(const ncx_vqa_train_dims& d, const ncx_mlb_params& m, const MtPtrs& p, int which) {
    const int B = d.B, dh = d.dz;
    GemmReq r{};
    auto tn = [&](int i, const float* D, int Mo, const float* X, int N, float* out) { gemm_tn_piece(r.a, i, D, Mo, Mo, X, N, N, out, B); };
    const float* mk = p.masks;
    switch (which) {
    case MT_XV: req_nt(r, B, dh, d.dv, p.vd, m.wv, (float*)p.xv, m.act_v, m.bv); break;
    case MT_XQ: req_nt(r, B, dh, d.dq, p.qd, m.wq, (float*)p.xq, m.act_q, m.bq); break;
    case MT_LOGITS: req_nt(r, B, d.A, dh, p.tc, m.wc, p.logits, 0, m.bc); break;
    case MT_DWC: tn(0, p.dlogits, d.A, p.tc, dh, p.g.wc); req_tn(r, d.A, dh, B); break;
    case MT_DT:
        req_nn_unsplit(r, B, p.dlogits, d.A, d.A, m.wc, dh, (float*)p.dt, dh);
        epi_dropout(r.a.epi, d.dropout_mode, d.seed, d.p_c, VQ_LAYER_C, ptr_off(mk, (long long)B * (d.dv + d.dq)), dh);
        break;
    case MT_DWVQ:
        tn(0, p.dpv, dh, p.vd, d.dv, p.g.wv); tn(1, p.dpq, dh, p.qd, d.dq, p.g.wq);
        req_tn(r, dh, (long long)d.dv + d.dq, B);
        break;
    default:
        req_nn_unsplit(r, B, p.dpq, dh, dh, m.wq, d.dq, p.dq, d.dq);
        epi_dropout(r.a.epi, d.dropout_mode, d.seed, d.p_q, VQ_LAYER_Q, ptr_off(mk, (long long)B * d.dv), d.dq);
        break;
    }
    return r;
}

static MtLayout mt_layout(const ncx_vqa_train_dims& d, const ncx_mlb_params& m) {
    MtLayout w{}; WsCarver cv;
    const size_t B = d.B, dh = d.dz;
    w.vd = cv.take(B * d.dv * 4); w.qd = cv.take(B * d.dq * 4);
    w.xv = cv.take(B * dh * 4); w.xq = cv.take(B * dh * 4);
    w.t = cv.take(m.act_c == 2 ? B * dh * 4 : 0); w.tc = cv.take(B * dh * 4);
    w.dt = cv.take(B * dh * 4); w.dpv = cv.take(B * dh * 4); w.dpq = cv.take(B * dh * 4);
    const MtPtrs p{};
    w.slab_bytes = max_slab_bytes<MT_COUNT>([&](int which) { return mt_gemm(d, m, p, which); });
    w.slab = cv.take(w.slab_bytes); w.total = cv.off;
    return w;
}

static MtPtrs mt_ptrs(char* base, const MtLayout& w, const ncx_mlb_params& m) {
    MtPtrs p{};
    p.vd = (float*)(base + w.vd); p.qd = (float*)(base + w.qd); p.xv = (float*)(base + w.xv); p.xq = (float*)(base + w.xq);
    p.t = m.act_c == 2 ? (float*)(base + w.t) : nullptr; p.tc = (float*)(base + w.tc);
    p.dt = (float*)(base + w.dt); p.dpv = (float*)(base + w.dpv); p.dpq = (float*)(base + w.dpq);
    return p;
}

static int mt_run(const ncx_vqa_train_dims& d, const ncx_mlb_params& m, const MtPtrs& p, int which, char* base, const MtLayout& w, hipStream_t s) {
    return run_request(mt_gemm(d, m, p, which), base, w.slab, w.slab_bytes, s);
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// z = x_q * x_v;  t = tanh(z) when act_c == 2 (else t is z and is not stored);  tc = drop_c(t).  n = B dh elements, V per thread.
template <int V>
__global__ __launch_bounds__(256) void k_mt_fuse(const float* __restrict__ xv, const float* __restrict__ xq, long long n, int act_c, TrainDrop k,
                                                 const float* __restrict__ mask_c, float* __restrict__ z, float* __restrict__ t, float* __restrict__ tc) {
    const long long i = (blockIdx.x * 256ll + threadIdx.x) * V;
    if (i >= n) return;
    const TrainVec<V> a = train_ld<V>(xv + i), b = train_ld<V>(xq + i);
    TrainVec<V> zz, tt, cc;
    const float sc = 1.f / (1.f - k.p[VQ_LAYER_C - 1]);
#pragma unroll
    for (int j = 0; j < V; ++j) {
        zz.v[j] = b.v[j] * a.v[j];
        tt.v[j] = act_c == 2 ? tanhf(zz.v[j]) : zz.v[j];
        cc.v[j] = train_keep(k, VQ_LAYER_C, mask_c, i + j) ? tt.v[j] * sc : 0.f;
    }
    train_st<V>(z + i, zz);
    if (act_c == 2) train_st<V>(t + i, tt);
    train_st<V>(tc + i, cc);
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

extern "C" size_t ncx_mlb_train_workspace_bytes(const ncx_vqa_train_dims* d, const ncx_mlb_params* m) {
    if (mt_check(d, m) != NCX_OK) return 0;
    return mt_layout(*d, *m).total;
}

extern "C" int ncx_mlb_train_ws_region(const ncx_vqa_train_dims* d, const ncx_mlb_params* m, int32_t which, size_t* offset, size_t* bytes) {
    if (!offset || !bytes) return NCX_E_NULL;
    const int rc = mt_check(d, m);
    if (rc != NCX_OK) return rc;
    const MtLayout w = mt_layout(*d, *m);
    return vq_ws_region(*d, which, w.vd, w.qd, w.tc, offset, bytes);
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
    if (!ws_ok(ws, ws_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    MtPtrs p = mt_ptrs(base, w, m);
    p.logits = logits; p.masks = d.dropout_mode == 2 ? masks : nullptr;
    const TrainDrop k = train_drop(d.dropout_mode, d.seed, {d.p_v, d.p_q, d.p_c});
    const long long n = (long long)d.B * d.dz;
    const float* mask_c = p.masks ? p.masks + (long long)d.B * (d.dv + d.dq) : nullptr;
    NCX_HIP_TRY(train_drop_vq(d, feats, img_idx, q_emb, k, p.masks, (float*)p.vd, (float*)p.qd, s));
    rc = mt_run(d, m, p, MT_XV, base, w, s); if (rc) return rc;
    rc = mt_run(d, m, p, MT_XQ, base, w, s); if (rc) return rc;
    if (n % 4 == 0 && al16(z))
        hipLaunchKernelGGL(k_mt_fuse<4>, dim3(grid256(n / 4)), dim3(256), 0, s, p.xv, p.xq, n, m.act_c, k, mask_c, z, (float*)p.t, (float*)p.tc);
    else
        hipLaunchKernelGGL(k_mt_fuse<1>, dim3(grid256(n)), dim3(256), 0, s, p.xv, p.xq, n, m.act_c, k, mask_c, z, (float*)p.t, (float*)p.tc);
    NCX_HIP_TRY(hipGetLastError());
    return mt_run(d, m, p, MT_LOGITS, base, w, s);
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
    if (!ws_ok(ws, ws_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    MtPtrs p = mt_ptrs(base, w, m);
    p.dlogits = dlogits; p.masks = d.dropout_mode == 2 ? masks : nullptr; p.g = *g; p.dq = dq_emb;
    const long long n = (long long)d.B * d.dz;
    rc = mt_run(d, m, p, MT_DWC, base, w, s); if (rc) return rc;
    rc = mt_run(d, m, p, MT_DT, base, w, s); if (rc) return rc;
    NCX_HIP_TRY(train_dfuse(p.dt, p.t, p.xv, p.xq, n, m.act_v, m.act_q, m.act_c, (float*)p.dpv, (float*)p.dpq, s));
    rc = mt_run(d, m, p, MT_DWVQ, base, w, s); if (rc) return rc;
    MtSums js{};
    js.n = 3;
    js.s[0] = MtSum{dlogits, g->bc, d.A, 0};
    js.s[1] = MtSum{p.dpv, g->bv, d.dz, (d.A + 31) / 32};
    js.s[2] = MtSum{p.dpq, g->bq, d.dz, js.s[1].blk0 + (d.dz + 31) / 32};
    hipLaunchKernelGGL(k_mt_colsum, dim3(js.s[2].blk0 + (d.dz + 31) / 32), dim3(256), 0, s, js, d.B);
    NCX_HIP_TRY(hipGetLastError());
    if (d.want_dq) { rc = mt_run(d, m, p, MT_DQ, base, w, s); if (rc) return rc; }
    return NCX_OK;
}
