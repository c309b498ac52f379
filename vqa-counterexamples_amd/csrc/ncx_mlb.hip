// ncx_mlb.hip -- the frozen MLB producer (MLBNoAtt in eval mode): ncx_mlb_workspace_bytes, ncx_mlb_forward.
//
// Reference: MLBFusion.forward (vqa/models/fusion.py:31-50), AbstractNoAtt._classif (vqa/models/noatt.py:24-29), called from
// CXModelBase.vqa_forward (vqa/models/cx.py:64-104) on the original + K candidate images of every question:
//   x_q[b]    = act_q(q[b] . Wq^T + bq)                      once per question (the reference duplicates q K + 1 times first)
//   x_v[b, r] = act_v(feats[img_idx[b, r]] . Wv^T + bv)
//   z[b, r]   = x_q[b] * x_v[b, r]                           -> z_orig / z_knns (before the classifier's activation)
//   a[b, r]   = act_c(z[b, r]) . Wc^T + bc                   -> a_knns, a_orig
// Plan: x_q on the generic engine (B rows); x_v on the fused forward kernel (ncx_main.h) as one row-gathered segment whose EPI_MLB
// epilogue multiplies by x_q[r / (K + 1)], row-splits z and stores t = tanh(z) beside it, so x_v never exists in memory and the
// classifier reads a plain operand (an activation on its load side would put a transcendental under every fp32 MFMA k-step:
// DESIGN 4f); the classifier on the fused forward kernel over the B K neighbour rows, the B original rows only on request.
// Widths the fused kernel does not take (dv not a multiple of 32, dh or A not a multiple of 4) run on the generic engine: x_v with
// its activation goes to the workspace and k_mlb_mul finishes it.
#include "ncx_train.h"

using namespace ncx;

// z = x_v * x_q[question], row-split; t = tanh(z) when t_knns is set (the generic-engine route's twin of the EPI_MLB epilogue)
__global__ __launch_bounds__(256) void k_mlb_mul(const float* __restrict__ xv, const float* __restrict__ xq, int dh, int g, long long total,
                                                 float* __restrict__ z_orig, float* __restrict__ z_knns, float* __restrict__ t_orig, float* __restrict__ t_knns) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const long long r = i / dh;
    const int n = (int)(i - r * dh);
    const long long b = r / g;
    const int jr = (int)(r - b * g);
    const float z = xv[i] * xq[b * dh + n];
    const long long o = (jr == 0 ? b : b * (g - 1) + jr - 1) * dh + n;
    (jr == 0 ? z_orig : z_knns)[o] = z;
    if (t_knns) (jr == 0 ? t_orig : t_knns)[o] = tanhf(z);
}

extern "C" {
struct MlbLayout { size_t xq, t_knns, t_orig, xv, wcp, slab, slab_bytes, total; bool main_v, main_c; };

static int check_mlb(const ncx_dims* d, const ncx_mlb_params* m) {
    if (!d || !m) return NCX_E_NULL;
    if (d->B < 1 || d->K < 1 || d->dv < 4 || d->dq < 4 || d->dz < 4 || d->A < 4 || d->n_img < 1) return NCX_E_DIMS;
    if (m->dh != d->dz) return NCX_E_DIMS;
    if ((long long)d->B * (d->K + 1) * (long long)(d->dz > d->A ? d->dz : d->A) >= (1ll << 31)) return NCX_E_DIMS;
    auto act_ok = [](int a) { return a == 0 || a == 2; };
    if (!act_ok(m->act_v) || !act_ok(m->act_q) || !act_ok(m->act_c)) return NCX_E_FLAGS;
    if (!m->wv || !m->bv || !m->wq || !m->bq || !m->wc || !m->bc) return NCX_E_NULL;
    return NCX_OK;
}

static MlbLayout mlb_layout(const ncx_dims& d, const ncx_mlb_params& m, GemmPlan* plans /*[3]*/) {
    MlbLayout w{};
    WsCarver cv;
    const long long Mv = (long long)d.B * (d.K + 1), Mk = (long long)d.B * d.K;
    // the fused forward kernel reads with 32-bit byte offsets and whole 32-column k-steps on the weight side (ncx_main.h)
    const ProducerMainRoutes pr = producer_main_routes(d, d.dz);
    w.main_v = pr.v; w.main_c = pr.c;
    w.xq = cv.take((size_t)d.B * d.dz * 4);
    w.t_knns = cv.take(m.act_c ? (size_t)Mk * d.dz * 4 : 0);
    w.t_orig = cv.take(m.act_c ? (size_t)d.B * d.dz * 4 : 0);
    w.xv = cv.take(w.main_v ? 0 : (size_t)Mv * d.dz * 4);
    w.wcp = cv.take(w.main_c && d.dz % 32 ? (size_t)d.A * pad_to(d.dz, 32) * 4 : 0);
    // 0: xq = act_q(q Wq^T)   1: xv = act_v(gather(v) Wv^T) (generic route)   2: a_knns = t Wc^T (generic route)
    const long long shp[3][3] = {{d.B, d.dz, ksteps(d.dq)}, {Mv, d.dz, ksteps(d.dv)}, {Mk, d.A, ksteps(d.dz)}};
    long long slab = 0;
    for (int i = 0; i < 3; ++i) {
        plans[i] = plan_gemm(FORM_NT, shp[i][0], shp[i][1], shp[i][2], true);
        int bm, bn; cfg_tile(plans[i].cfg, bm, bn);
        const long long e = plans[i].split > 1 ? (long long)WgMap{(int)cdiv(shp[i][0], bm), (int)cdiv(shp[i][1], bn), plans[i].split}.count() * bm * bn : 0;
        if (e > slab) slab = e;
    }
    w.slab_bytes = (size_t)slab * 4;
    w.slab = cv.take(w.slab_bytes);
    w.total = cv.off;
    return w;
}

size_t ncx_mlb_workspace_bytes(const ncx_dims* d, const ncx_mlb_params* m) {
    if (check_mlb(d, m) != NCX_OK) return 0;
    GemmPlan plans[3];
    return mlb_layout(*d, *m, plans).total;
}

int ncx_mlb_route(const ncx_dims* d, const ncx_mlb_params* m, int32_t* out4) {
    if (!out4) return NCX_E_NULL;
    const int rc = check_mlb(d, m);
    if (rc != NCX_OK) return rc;
    GemmPlan plans[3];
    const MlbLayout w = mlb_layout(*d, *m, plans);
    out4[0] = w.main_v;
    out4[1] = w.main_v ? main_mlb_form((long long)d->B * (d->K + 1), d->dz) : -1;
    out4[2] = w.main_c ? (d->dz % 32 ? 2 : 1) : 0;
    out4[3] = m->act_c != 0;
    return NCX_OK;
}

int ncx_mlb_ws_region(const ncx_dims* d, const ncx_mlb_params* m, int32_t which, size_t* offset, size_t* bytes) {
    if (!offset || !bytes) return NCX_E_NULL;
    const int rc = check_mlb(d, m);
    if (rc != NCX_OK) return rc;
    GemmPlan plans[3];
    const MlbLayout w = mlb_layout(*d, *m, plans);
    const size_t B = d->B, row = (size_t)d->dz * 4;
    if (which == NCX_MLB_WS_XQ) { *offset = w.xq; *bytes = B * row; }
    else if (which == NCX_MLB_WS_T_KNNS && m->act_c) { *offset = w.t_knns; *bytes = B * d->K * row; }
    else if (which == NCX_MLB_WS_T_ORIG && m->act_c) { *offset = w.t_orig; *bytes = B * row; }
    else if (which == NCX_MLB_WS_XV && !w.main_v) { *offset = w.xv; *bytes = B * (d->K + 1) * row; }
    else return NCX_E_FLAGS;         // (an unknown id, or a tensor this route never stores)
    return NCX_OK;
}

int ncx_mlb_forward(const ncx_dims* dp, const float* feats, const int32_t* img_idx, const float* q_emb,
                    const ncx_mlb_params* mp, void* workspace, size_t workspace_bytes,
                    float* z_orig, float* z_knns, float* a_knns, float* a_orig, void* stream_) {
    int rc = check_mlb(dp, mp);
    if (rc != NCX_OK) return rc;
    if (!feats || !img_idx || !q_emb || !workspace || !z_orig || !z_knns || !a_knns) return NCX_E_NULL;
    const ncx_dims& d = *dp; const ncx_mlb_params& m = *mp;
    GemmPlan plans[3];
    const MlbLayout w = mlb_layout(d, m, plans);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float* xq = (float*)(ws + w.xq); float* slab = (float*)(ws + w.slab);
    float* t_knns = m.act_c ? (float*)(ws + w.t_knns) : nullptr; float* t_orig = m.act_c ? (float*)(ws + w.t_orig) : nullptr;
    const int Mv = d.B * (d.K + 1), Mk = d.B * d.K, dh = d.dz;
    {   // x_q = act_q(q . Wq^T + bq), once per question                                fusion.py:41-47
        GemmArgs a = gemm_nt(d.B, dh, d.dq, q_emb, m.wq, xq, m.act_q);
        rc = run_gemm_planned(a, FORM_NT, plans[0], slab, w.slab_bytes, m.bq, s); if (rc) return rc;
    }
    if (w.main_v) {
        // z = act_v(gather(feats, img_idx) . Wv^T + bv) * x_q[question] -> z_orig / z_knns, t = tanh(z) -> workspace: ONE launch of the
        // fused forward kernel with the EPI_MLB epilogue                                fusion.py:33-39,49 (+ the host gather, cx.py:83-92)
        MainArgs a{}; a.M = Mv; a.N = dh; a.nseg = 1;
        a.seg[0].kind = MK_GATHER; a.seg[0].a = feats; a.seg[0].lda = d.dv; a.seg[0].idx = img_idx; a.seg[0].klen = d.dv;
        a.seg[0].b = m.wv; a.seg[0].ldb = d.dv;
        a.out = z_knns; a.ldo = dh; a.epi.bias = m.bv; a.epi.relu = m.act_v; a.split = 1;
        a.epi.fold_mul = xq; a.epi.ld_fold = dh; a.epi.rowsplit_g = d.K + 1; a.epi.out0 = z_orig; a.epi.ldo0 = dh;
        a.t_out = t_knns; a.t_out0 = t_orig;
        rc = main_forward_mlb(a, s); if (rc) return rc;
    } else {
        float* xv = (float*)(ws + w.xv);
        GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = Mv;
        a.a[0] = x_gather(feats, d.dv, img_idx, Mv, d.dv); a.b[0] = x_plain(m.wv, d.dv, dh, d.dv); a.klen[0] = d.dv;
        a.out[0] = xv; a.ldo[0] = dh; a.n_cols[0] = dh; a.epi.relu = m.act_v;
        rc = run_gemm_planned(a, FORM_NT, plans[1], slab, w.slab_bytes, m.bv, s); if (rc) return rc;
        const long long total = (long long)Mv * dh;
        hipLaunchKernelGGL(k_mlb_mul, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, xv, xq, dh, d.K + 1, total, z_orig, z_knns, t_orig, t_knns);
        NCX_HIP_TRY(hipGetLastError());
    }
    // the classifier's operand: t = tanh(z) from the workspace, or z itself without classif.activation      noatt.py:25-26
    const float* ck = m.act_c ? t_knns : z_knns; const float* co = m.act_c ? t_orig : z_orig;
    if (w.main_c) {
        // a_knns = t_knns . Wc^T + bc on the fused forward kernel (weight rows zero-padded to whole k-steps)   noatt.py:24-29
        const float* wc = m.wc; long long ldw = dh;
        if (dh % 32) {
            float* wcp = (float*)(ws + w.wcp);
            const int ldd = pad_to(dh, 32);
            NCX_HIP_TRY(pad_rows(m.wc, (long long)dh, dh, wcp, ldd, d.A, s));
            wc = wcp; ldw = ldd;
        }
        MainArgs a{}; a.M = Mk; a.N = d.A; a.nseg = 1;
        a.seg[0].kind = MK_PLAIN; a.seg[0].a = ck; a.seg[0].lda = dh; a.seg[0].klen = dh; a.seg[0].b = wc; a.seg[0].ldb = ldw;
        a.out = a_knns; a.ldo = d.A; a.epi.bias = m.bc; a.split = 1;
        rc = main_forward(a, s); if (rc) return rc;
    } else {
        GemmArgs a = gemm_nt(Mk, d.A, dh, ck, m.wc, a_knns, 0);
        rc = run_gemm_planned(a, FORM_NT, plans[2], slab, w.slab_bytes, m.bc, s); if (rc) return rc;
    }
    if (a_orig) {   // the B original rows, only on request (NeuralModel never reads a_orig)
        GemmArgs a = gemm_nt(d.B, d.A, dh, co, m.wc, a_orig, 0);
        a.split[0] = 1;
        GemmPlan pl; pl.cfg = CFG_64x64; pl.split = 1;
        rc = run_gemm_planned(a, FORM_NT, pl, slab, w.slab_bytes, m.bc, s); if (rc) return rc;
    }
    return NCX_OK;
}
}  // extern "C"
