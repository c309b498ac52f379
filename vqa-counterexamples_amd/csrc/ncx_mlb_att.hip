// ncx_mlb_att.hip -- the MLB attention model (MLBAtt in eval mode) below the question encoder: ncx_mlb_att_workspace_bytes,
// ncx_mlb_att_forward, ncx_mlb_att_forward_flags (flags = NCX_F_X6: step b on k_att_logits_x6, ncx_mlb_att.h; same slab, same
// workspace), ncx_mlb_att_logits_form.
//
// Reference: AbstractAtt._attention / _fusion_glimpses / _classif and MLBAtt (vqa/models/att.py:39-192); every dropout the identity.
//   a. x_q = act(q . Wq_att^T + b)                                       generic engine
//   b. k_att_logits: the 1 x 1 convolution conv_v_att over the image's NCHW map as an MFMA product whose A operand is the map
//      itself in "row-is-k" form (ncx_gemm.h: the reduction index c runs along rows of pitch P, the position p is contiguous), with
//      the whole attention head in the epilogue: bias, act_v, * x_q[b], act_mm, then the contraction with conv_att.weight over the
//      tile's 64 hidden columns.  x_att [B, P, dh_att] never exists in memory; what leaves the kernel is the partial position
//      logits of one dh_att tile, slab[b][h-tile][g][p].
//   c. k_att_pool: sums the slab over the h-tiles in a fixed order (no float atomics: two calls are bit-identical), adds
//      conv_att.bias, max-subtracted softmax over the P positions of each glimpse -> att; then every row c of the map is read once
//      and dotted with all G maps -> v_att [B, G, dv].
//   d. the G glimpse Linears as one grouped launch of the generic engine writing column slices of x_v; x_qf on the generic engine;
//      k_att_fuse: t = act_c(act_v(x_v + bg) * x_qf)   (the engine's epilogue has one bias vector per launch, the G Linears have G)
//   e. logits = t . Wc^T + bc                                            generic engine
// Tiling of the positions: per image (a tile never spans two images, so x_q is one row per tile).  Two tile shapes: 208 = 13 x 16
// positions when that pads P less than 64-row tiles do (P = 196: 208 rows, 5.8 % of the MFMAs wasted, against 23 % for 4 x 64 or
// 2 x 128 and 12.5 % for 7 x 32), else 64.  The 208-row tile puts its four waves side by side along the hidden columns, 13 blocks
// each (2 x 2 waves would give 7 + 6 blocks and wait for the 7); its loader tile is 224 wide, the last 16 columns are not multiplied.
// P < 4 (no 16-byte window fits a row of the map) takes k_att_logits_small, a plain per-position kernel.
#include "ncx_mlb_att.h"

namespace {
struct AttLayout {
    size_t xq, aslab, v_att, xv, xqf, slab, slab_bytes, total;
    int HT, PT, TM;          // TM: positions per tile of k_att_logits (208 or 64); 0: k_att_logits_small
    GemmPlan plan[4];        // 0 x_q, 1 glimpse Linears (grouped), 2 x_qf, 3 classifier
};

AttLayout att_layout(const ncx_mlb_att_dims& d) {
    AttLayout w{};
    WsCarver cv;
    const int GF = d.G * d.dh_f;
    if (d.P >= 4) {
        w.TM = cdiv(d.P, 208) * 208 < cdiv(d.P, 64) * 64 ? 208 : 64;
        w.HT = (int)cdiv(d.dh_att, ATT_BN); w.PT = (int)cdiv(d.P, w.TM);
    } else {
        w.TM = 0; w.HT = 1; w.PT = 1;
    }
    w.xq = cv.take((size_t)d.B * d.dh_att * 4);
    w.aslab = cv.take((size_t)d.B * w.HT * d.G * d.P * 4);
    w.v_att = cv.take((size_t)d.B * d.G * d.dv * 4);
    w.xv = cv.take((size_t)d.B * GF * 4);
    w.xqf = cv.take((size_t)d.B * GF * 4);
    w.plan[0] = plan_gemm(FORM_NT, d.B, d.dh_att, ksteps(d.dq), true);
    w.plan[1] = plan_gemm(FORM_NT, d.B, d.dh_f, ksteps(d.dv), true);
    w.plan[2] = plan_gemm(FORM_NT, d.B, GF, ksteps(d.dq), true);
    w.plan[3] = plan_gemm(FORM_NT, d.B, d.A, ksteps(GF), true);
    const GemmArgs probe[4] = {gemm_nt(d.B, d.dh_att, d.dq, nullptr, nullptr, nullptr, 0), glimpse_gemm(d, nullptr, nullptr, nullptr),
                               gemm_nt(d.B, GF, d.dq, nullptr, nullptr, nullptr, 0), gemm_nt(d.B, d.A, GF, nullptr, nullptr, nullptr, 0)};
    for (int i = 0; i < 4; ++i) {
        const size_t e = gemm_slab_bytes(probe[i], w.plan[i]);
        if (e > w.slab_bytes) w.slab_bytes = e;
    }
    w.slab = cv.take(w.slab_bytes);
    w.total = cv.off;
    return w;
}
}  // namespace

extern "C" {
size_t ncx_mlb_att_workspace_bytes(const ncx_mlb_att_dims* d, const ncx_mlb_att_params* m) {
    if (check_att(d, m) != NCX_OK) return 0;
    return att_layout(*d).total;
}

int ncx_mlb_att_logits_form(const ncx_mlb_att_dims* d, uint32_t flags) {
    if (!att_flags_ok(flags)) return NCX_E_DIMS;
    const int rc = check_att_dims(d);
    if (rc != NCX_OK) return rc;
    return att_logits_form(d->P, flags);
}

int ncx_mlb_att_forward(const ncx_mlb_att_dims* dp, const float* feats, const int32_t* img_idx, const float* q_emb,
                        const ncx_mlb_att_params* mp, void* workspace, size_t workspace_bytes,
                        float* logits, float* att, void* stream_) {
    return ncx_mlb_att_forward_flags(dp, feats, img_idx, q_emb, mp, 0, workspace, workspace_bytes, logits, att, stream_);
}

int ncx_mlb_att_forward_flags(const ncx_mlb_att_dims* dp, const float* feats, const int32_t* img_idx, const float* q_emb,
                              const ncx_mlb_att_params* mp, uint32_t flags, void* workspace, size_t workspace_bytes,
                              float* logits, float* att, void* stream_) {
    if (!att_flags_ok(flags)) return NCX_E_DIMS;
    int rc = check_att(dp, mp);
    if (rc != NCX_OK) return rc;
    if (!feats || !img_idx || !q_emb || !workspace || !logits || !att) return NCX_E_NULL;
    const ncx_mlb_att_dims& d = *dp; const ncx_mlb_att_params& m = *mp;
    const AttLayout w = att_layout(d);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float* xq = (float*)(ws + w.xq); float* aslab = (float*)(ws + w.aslab); float* v_att = (float*)(ws + w.v_att);
    float* xv = (float*)(ws + w.xv); float* xqf = (float*)(ws + w.xqf); float* slab = (float*)(ws + w.slab);
    const int GF = d.G * d.dh_f;
    {   // a. x_q = act(q . Wq_att^T + b)                                               att.py:58-63
        GemmArgs a = gemm_nt(d.B, d.dh_att, d.dq, q_emb, m.wq_att, xq, m.act_q_att);
        rc = run_gemm_planned(a, FORM_NT, w.plan[0], slab, w.slab_bytes, m.bq_att, s); if (rc) return rc;
    }
    {   // b. partial position logits of every dh_att tile                              att.py:46-57,71-90
        AttArgs a{};
        a.feats = feats; a.img_idx = img_idx; a.wv = m.wv_att; a.bv = m.bv_att; a.xq = xq; a.wa = m.wa; a.slab = aslab;
        a.P = d.P; a.dv = d.dv; a.dh = d.dh_att; a.G = d.G; a.n_img = d.n_img; a.HT = w.HT; a.PT = w.PT;
        a.act_v = m.act_v_att; a.act_mm = m.act_mm;
        const AttTrain tr{};
        rc = run_att_logits<false>(a, tr, d.B, flags, s);
        if (rc) return rc;
    }
    {   // c. softmax over the positions, attention-weighted pooling                    att.py:91-116
        PoolArgs a{};
        a.feats = feats; a.img_idx = img_idx; a.slab = aslab; a.ba = m.ba; a.att = att; a.v_att = v_att;
        a.P = d.P; a.dv = d.dv; a.G = d.G; a.n_img = d.n_img; a.HT = w.HT;
        long long chunks = cdiv(1024, d.B);                       // enough workgroups for every CU several times over
        if (chunks > cdiv(d.dv, 16)) chunks = cdiv(d.dv, 16);
        if (chunks < 1) chunks = 1;
        a.rows_per_chunk = (int)(cdiv(cdiv(d.dv, chunks), 8) * 8);
        chunks = cdiv(d.dv, a.rows_per_chunk);
        hipLaunchKernelGGL(k_att_pool, dim3((unsigned)chunks, (unsigned)d.B), dim3(256), (size_t)(d.G * d.P + 4) * 4, s, a);
        NCX_HIP_TRY(hipGetLastError());
    }
    {   // d. the glimpse Linears (pre-activation, column slices of x_v), x_qf, the second fusion      att.py:120-143,145-148
        GemmArgs a = glimpse_gemm(d, v_att, m.wg, xv);
        rc = run_gemm_planned(a, FORM_NT, w.plan[1], slab, w.slab_bytes, nullptr, s); if (rc) return rc;
        GemmArgs q = gemm_nt(d.B, GF, d.dq, q_emb, m.wqf, xqf, m.act_q);
        rc = run_gemm_planned(q, FORM_NT, w.plan[2], slab, w.slab_bytes, m.bqf, s); if (rc) return rc;
        const long long total = (long long)d.B * GF;
        hipLaunchKernelGGL(k_att_fuse, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, xv, m.bg, xqf, GF, total, m.act_v, m.act_c);
        NCX_HIP_TRY(hipGetLastError());
    }
    {   // e. logits = t . Wc^T + bc                                                     att.py:149-153
        GemmArgs a = gemm_nt(d.B, d.A, GF, xv, m.wc, logits, 0);
        rc = run_gemm_planned(a, FORM_NT, w.plan[3], slab, w.slab_bytes, m.bc, s); if (rc) return rc;
    }
    return NCX_OK;
}
}  // extern "C"
