// ncx_vqa_train.hip -- the trainable MutanNoAtt VQA model below the question encoder: training-mode forward and backward (the loss is
// ncx_ce_loss, ncx_loss_adam.hip; reference vqa/lib/engine.py:6-56, train.py:136-145; MutanFusion.forward vqa/models/fusion.py:78-121, AbstractNoAtt._classif
// vqa/models/noatt.py:24-29).  One image per question: row b reads feats[img_idx[b]].
//
// Forward (7 launches + split fix-ups):
//   drop_vq     vd [B, dv] = drop_v(feats[img_idx]), qd [B, dq] = drop_q(q_emb)                (F.dropout, fusion.py:82, 88)
//   NT x 2      x_v = act_v(vd Wv^T + bv), x_q = act_q(qd Wq^T + bq)                            (fusion.py:83-93)
//   NT x 2      Hv = x_v Whv^T + bhv, Hq = x_q Whq^T + bhq, both [B, R dz] and kept            (fusion.py:96-107, all R at once)
//   k_vt_fuse   z = sum_r Hv_r * Hq_r;  z_c = drop_c(z)                                         (fusion.py:108-115, noatt.py:27)
//   NT          logits = z_c Wc^T + bc                                                          (noatt.py:28)
// Backward, given dlogits (ncx_ce_loss) (15 launches, 16 with dq_emb, + split fix-ups):
//   TN, colsum  dWc = dlogits^T z_c, dbc
//   NN          dz = (dlogits Wc) * mask_c: the dropout epilogue of the engine regenerates (or reads) the forward's mask
//   k_vt_dh     dHv_r = dz * Hq_r, dHq_r = dz * Hv_r
//   TN group    dWhv = dHv^T x_v | dWhq = dHq^T x_q (one launch);  colsum x 2: dbhv, dbhq
//   NN x 2      dx_v = dHv Whv, dx_q = dHq Whq;  dact: dpre = dx (1 - x^2) where the activation is tanh
//   TN x 2      dWv = dpre_v^T vd, dWq = dpre_q^T qd;  colsum x 2: dbv, dbq
//   NN          dq_emb = (dpre_q Wq) * mask_q, on request (dropout epilogue again)
// drop_vq and dact are the shared kernels of ncx_train.hip (k_train_drop_vq, k_train_dact); the dropout front end, the GEMM request
// builders, the runner and the entry points' checks are ncx_train.h's, where the dropout contract is stated: mode 1 is the counter-based
// generator with layer ids 1 (v), 2 (q), 3 (z) and element index r * width + c, nothing is stored but the dropped tensors themselves;
// mode 2 reads explicit keep masks [B dv | B dq | B dz].  What is here is the model: the products, the workspace, the launch order.
// No atomics, every reduction in a fixed order: bit-identical from run to run.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ncx_train.h"

namespace ncx {

enum VtGemm : int { VT_XV = 0, VT_XQ, VT_HV, VT_HQ, VT_LOGITS, VT_DWC, VT_DZ, VT_DWH, VT_DXV, VT_DXQ, VT_DWV, VT_DWQ, VT_DQ, VT_COUNT };

struct VtLayout { size_t vd, qd, xv, xq, hv, hq, zc, dzc, dhv, dhq, dxv, dxq, slab, slab_bytes, total; };
struct VtPtrs {
    const float *vd, *qd, *xv, *xq, *hv, *hq, *zc, *dzc, *dhv, *dhq, *dxv, *dxq, *dlogits, *masks;
    float *logits, *dq;
    ncx_mutan_grads g;
};

static int vt_check(const ncx_vqa_train_dims* d, const ncx_mutan_params* m) {
    if (!d || !m) return NCX_E_NULL;
    const int rc = vq_check_dims(d);
    if (rc != NCX_OK) return rc;
    if (m->dhv < 4 || m->dhq < 4 || m->R < 1 || m->R > NCX_MAX_SEG) return NCX_E_DIMS;
    const long long lim = 1ll << 31, RZ = (long long)m->R * d->dz, h = m->dhv > m->dhq ? m->dhv : m->dhq;
    if (d->B * RZ >= lim || RZ * h >= lim || h * (d->dv > d->dq ? d->dv : d->dq) >= lim) return NCX_E_DIMS;
    if ((m->act_v != 0 && m->act_v != 2) || (m->act_q != 0 && m->act_q != 2)) return NCX_E_FLAGS;
    return NCX_OK;
}

// The products of the step on the generic engine (pointers may be NULL when only sizing the slab).
static GemmReq vt_gemm(const ncx_vqa_train_dims& d, const ncx_mutan_params& m, const VtPtrs& p, int which) {
    const int B = d.B, RZ = m.R * d.dz;
    GemmReq r{};
    auto tn = [&](int i, const float* D, int Mo, const float* X, int N, float* out) { gemm_tn_piece(r.a, i, D, Mo, Mo, X, N, N, out, B); };
    const float* mk = p.masks;
    switch (which) {
    case VT_XV: req_nt(r, B, m.dhv, d.dv, p.vd, m.wv, (float*)p.xv, m.act_v, m.bv); break;
    case VT_XQ: req_nt(r, B, m.dhq, d.dq, p.qd, m.wq, (float*)p.xq, m.act_q, m.bq); break;
    case VT_HV: req_nt(r, B, RZ, m.dhv, p.xv, m.whv, (float*)p.hv, 0, m.bhv); break;
    case VT_HQ: req_nt(r, B, RZ, m.dhq, p.xq, m.whq, (float*)p.hq, 0, m.bhq); break;
    case VT_LOGITS: req_nt(r, B, d.A, d.dz, p.zc, m.wc, p.logits, 0, m.bc); break;
    case VT_DWC: tn(0, p.dlogits, d.A, p.zc, d.dz, p.g.wc); req_tn(r, d.A, d.dz, B); break;
    case VT_DZ:
        req_nn_unsplit(r, B, p.dlogits, d.A, d.A, m.wc, d.dz, (float*)p.dzc, d.dz);
        epi_dropout(r.a.epi, d.dropout_mode, d.seed, d.p_c, VQ_LAYER_C, ptr_off(mk, (long long)B * (d.dv + d.dq)), d.dz);
        break;
    case VT_DWH:
        tn(0, p.dhv, RZ, p.xv, m.dhv, p.g.whv); tn(1, p.dhq, RZ, p.xq, m.dhq, p.g.whq);
        req_tn(r, RZ, m.dhv + m.dhq, B);
        break;
    case VT_DXV: req_nn(r, B, p.dhv, RZ, RZ, m.whv, m.dhv, (float*)p.dxv, m.dhv); break;      // no epilogue: these two may split
    case VT_DXQ: req_nn(r, B, p.dhq, RZ, RZ, m.whq, m.dhq, (float*)p.dxq, m.dhq); break;
    case VT_DWV: tn(0, p.dxv, m.dhv, p.vd, d.dv, p.g.wv); req_tn(r, m.dhv, d.dv, B); break;
    case VT_DWQ: tn(0, p.dxq, m.dhq, p.qd, d.dq, p.g.wq); req_tn(r, m.dhq, d.dq, B); break;
    default:
        req_nn_unsplit(r, B, p.dxq, m.dhq, m.dhq, m.wq, d.dq, p.dq, d.dq);
        epi_dropout(r.a.epi, d.dropout_mode, d.seed, d.p_q, VQ_LAYER_Q, ptr_off(mk, (long long)B * d.dv), d.dq);
        break;
    }
    return r;
}

static VtLayout vt_layout(const ncx_vqa_train_dims& d, const ncx_mutan_params& m) {
    VtLayout w{}; WsCarver cv;
    const size_t B = d.B, RZ = (size_t)m.R * d.dz;
    w.vd = cv.take(B * d.dv * 4); w.qd = cv.take(B * d.dq * 4);
    w.xv = cv.take(B * m.dhv * 4); w.xq = cv.take(B * m.dhq * 4); w.hv = cv.take(B * RZ * 4); w.hq = cv.take(B * RZ * 4);
    w.zc = cv.take(B * d.dz * 4); w.dzc = cv.take(B * d.dz * 4); w.dhv = cv.take(B * RZ * 4); w.dhq = cv.take(B * RZ * 4);
    w.dxv = cv.take(B * m.dhv * 4); w.dxq = cv.take(B * m.dhq * 4);
    const VtPtrs p{};
    w.slab_bytes = max_slab_bytes<VT_COUNT>([&](int which) { return vt_gemm(d, m, p, which); });
    w.slab = cv.take(w.slab_bytes); w.total = cv.off;
    return w;
}

static VtPtrs vt_ptrs(char* base, const VtLayout& w) {
    VtPtrs p{};
    p.vd = (float*)(base + w.vd); p.qd = (float*)(base + w.qd); p.xv = (float*)(base + w.xv); p.xq = (float*)(base + w.xq);
    p.hv = (float*)(base + w.hv); p.hq = (float*)(base + w.hq); p.zc = (float*)(base + w.zc); p.dzc = (float*)(base + w.dzc);
    p.dhv = (float*)(base + w.dhv); p.dhq = (float*)(base + w.dhq); p.dxv = (float*)(base + w.dxv); p.dxq = (float*)(base + w.dxq);
    return p;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// z[b][j] = sum_r Hv[b][r dz + j] Hq[b][r dz + j] (r ascending); zc = drop_c(z)
__global__ __launch_bounds__(256) void k_vt_fuse(const float* __restrict__ hv, const float* __restrict__ hq, int B, int dz, int R, TrainDrop k,
                                                 const float* __restrict__ mask_c, float* __restrict__ z, float* __restrict__ zc) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (long long)B * dz) return;
    const int b = (int)(i / dz), j = (int)(i - (long long)b * dz);
    const long long row = (long long)b * R * dz + j;
    float acc = 0.f;
    for (int r = 0; r < R; ++r) acc = fmaf(hv[row + (long long)r * dz], hq[row + (long long)r * dz], acc);
    z[i] = acc;
    zc[i] = train_keep(k, VQ_LAYER_C, mask_c, i) ? acc * (1.f / (1.f - k.p[VQ_LAYER_C - 1])) : 0.f;
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

}  // namespace ncx

using namespace ncx;

static int vt_run(const ncx_vqa_train_dims& d, const ncx_mutan_params& m, const VtPtrs& p, int which, char* base, const VtLayout& w, hipStream_t s) {
    return run_request(vt_gemm(d, m, p, which), base, w.slab, w.slab_bytes, s);
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
    return vq_ws_region(*d, which, w.vd, w.qd, w.zc, offset, bytes);
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
    if (!ws_ok(ws, ws_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    VtPtrs p = vt_ptrs(base, w);
    p.logits = logits; p.masks = d.dropout_mode == 2 ? masks : nullptr;
    const TrainDrop k = train_drop(d.dropout_mode, d.seed, {d.p_v, d.p_q, d.p_c});
    NCX_HIP_TRY(train_drop_vq(d, feats, img_idx, q_emb, k, p.masks, (float*)p.vd, (float*)p.qd, s));
    rc = vt_run(d, m, p, VT_XV, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_XQ, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_HV, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_HQ, base, w, s); if (rc) return rc;
    hipLaunchKernelGGL(k_vt_fuse, dim3(grid256((long long)d.B * d.dz)), dim3(256), 0, s, p.hv, p.hq, d.B, d.dz, m.R, k,
                       p.masks ? p.masks + (long long)d.B * (d.dv + d.dq) : nullptr, z, (float*)p.zc);
    NCX_HIP_TRY(hipGetLastError());
    return vt_run(d, m, p, VT_LOGITS, base, w, s);
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
    if (!ws_ok(ws, ws_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    VtPtrs p = vt_ptrs(base, w);
    p.dlogits = dlogits; p.masks = d.dropout_mode == 2 ? masks : nullptr; p.g = *g; p.dq = dq_emb;
    const int RZ = m.R * d.dz;
    rc = vt_run(d, m, p, VT_DWC, base, w, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows(dlogits, (long long)d.A, d.B, d.A, g->bc, s));
    rc = vt_run(d, m, p, VT_DZ, base, w, s); if (rc) return rc;
    hipLaunchKernelGGL(k_vt_dh, dim3(grid256((long long)d.B * RZ)), dim3(256), 0, s, p.dzc, p.hv, p.hq, d.B, d.dz, m.R, (float*)p.dhv, (float*)p.dhq);
    NCX_HIP_TRY(hipGetLastError());
    rc = vt_run(d, m, p, VT_DWH, base, w, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows(p.dhv, (long long)RZ, d.B, RZ, g->bhv, s));
    NCX_HIP_TRY(colsum_rows(p.dhq, (long long)RZ, d.B, RZ, g->bhq, s));
    rc = vt_run(d, m, p, VT_DXV, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_DXQ, base, w, s); if (rc) return rc;
    if (m.act_v == 2 || m.act_q == 2) {
        const long long nv = (long long)d.B * m.dhv, nq = (long long)d.B * m.dhq;
        NCX_HIP_TRY(train_dact((float*)p.dxv, p.xv, nv, m.act_v, (float*)p.dxq, p.xq, nq, m.act_q, s));
    }
    rc = vt_run(d, m, p, VT_DWV, base, w, s); if (rc) return rc;
    rc = vt_run(d, m, p, VT_DWQ, base, w, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows(p.dxv, (long long)m.dhv, d.B, m.dhv, g->bv, s));
    NCX_HIP_TRY(colsum_rows(p.dxq, (long long)m.dhq, d.B, m.dhq, g->bq, s));
    if (d.want_dq) { rc = vt_run(d, m, p, VT_DQ, base, w, s); if (rc) return rc; }
    return NCX_OK;
}
