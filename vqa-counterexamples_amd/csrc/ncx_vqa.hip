// ncx_vqa.hip -- the fused MUTAN producer: ncx_vqa_workspace_bytes, ncx_vqa_forward.
#include "ncx_train.h"
#include <stdio.h>

using namespace ncx;
extern "C" {
struct VqaLayout { size_t xq, hq, xv, wcp, slab, slab_bytes, total; };
// What ncx_vqa_forward launches for a shape; ncx_vqa_route reports it from here.
struct VqaRoute {
    bool main_v;     // x_v on the fused forward kernel (one gathered segment), else the generic engine's gather
    bool fold;       // the fusion on k_mutan_fold (one product per question), else the generic engine's FOLD chain of R pairs
    bool main_c;     // a_knns on the fused forward kernel, else the generic engine
    bool pad_c;      // ... against a copy of the classifier weights with rows zero-padded to whole 32-column k-steps
};
// dst[r][0 .. cols) = src[r][0 .. cols), dst[r][cols .. ldd) = 0: the classifier weights with their rows zero-padded to whole 32-column
// k-steps for the fused forward kernel (ncx_main.h reads the weight side of a segment up to the next multiple of 32 columns)
__global__ __launch_bounds__(256) void k_pad_rows(const float* __restrict__ src, long long lds_, int cols, float* __restrict__ dst, int ldd, int rows) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)rows * ldd) return;
    const int r = (int)(i / ldd), c = (int)(i - (long long)r * ldd);
    dst[i] = c < cols ? src[(long long)r * lds_ + c] : 0.f;
}
}  // extern "C"
namespace ncx {
hipError_t pad_rows(const float* src, long long ld_src, int cols, float* dst, int ldd, int rows, hipStream_t s) {
    hipLaunchKernelGGL(k_pad_rows, dim3((unsigned)cdiv((long long)rows * ldd, 256)), dim3(256), 0, s, src, ld_src, cols, dst, ldd, rows);
    return hipGetLastError();
}
}  // namespace ncx
extern "C" {
static VqaRoute vqa_route(const ncx_dims& d, const ncx_mutan_params& m) {
    const ProducerMainRoutes p = producer_main_routes(d, m.dhv);
    VqaRoute r;
    r.main_v = p.v; r.fold = mutan_fold_supported(d, m); r.main_c = p.c; r.pad_c = p.c && d.dz % 32 != 0;
    return r;
}
static VqaLayout vqa_layout(const ncx_dims& d, const ncx_mutan_params& m, GemmPlan* plans /*[5]*/) {
    VqaLayout w{};
    WsCarver cv;
    const long long Mv = (long long)d.B * (d.K + 1), RZ = (long long)m.R * d.dz;
    w.xq = cv.take((size_t)d.B * m.dhq * 4);
    w.hq = cv.take((size_t)d.B * RZ * 4);
    w.xv = cv.take((size_t)Mv * m.dhv * 4);
    w.wcp = cv.take(d.dz % 32 ? (size_t)d.A * pad_to(d.dz, 32) * 4 : 0);
    // 0: xq = act(q Wq^T)  1: hq = xq Whq^T  2: xv = act(gather(v) Wv^T)  3: z (fold, never split)  4: a = z Wc^T
    const long long shp[5][3] = {{d.B, m.dhq, ksteps(d.dq)}, {d.B, RZ, ksteps(m.dhq)}, {Mv, m.dhv, ksteps(d.dv)}, {Mv, d.dz, 0}, {(long long)d.B * d.K, d.A, ksteps(d.dz)}};
    long long slab = 0;
    for (int i = 0; i < 5; ++i) {
        plans[i] = plan_gemm(FORM_NT, shp[i][0], shp[i][1], shp[i][2], true);
        {   // experiment hook
            char name[32]; snprintf(name, sizeof name, "NCX_VQA_CFG_%d", i);
            const char* c = hook_env(name);
            if (c && cfg_supported(FORM_NT, atoi(c))) { plans[i].cfg = atoi(c); plans[i].split = 1; }
        }
        if (i == 3) { plans[i].cfg = CFG_64x64; plans[i].split = 1; }
        int bm, bn; cfg_tile(plans[i].cfg, bm, bn);
        const long long e = plans[i].split > 1 ? (long long)WgMap{(int)cdiv(shp[i][0], bm), (int)cdiv(shp[i][1], bn), plans[i].split}.count() * bm * bn : 0;
        if (e > slab) slab = e;
    }
    w.slab_bytes = (size_t)slab * 4;
    w.slab = cv.take(w.slab_bytes);
    w.total = cv.off;
    return w;
}
static int check_mutan(const ncx_dims* d, const ncx_mutan_params* m) {
    if (!d || !m) return NCX_E_NULL;
    if (d->B < 1 || d->K < 1 || d->dv < 4 || d->dq < 4 || d->dz < 4 || d->A < 4 || d->n_img < 1) return NCX_E_DIMS;
    if (m->dhv < 4 || m->dhq < 4 || m->R < 1 || m->R > NCX_MAX_SEG) return NCX_E_DIMS;
    if ((long long)d->B * (d->K + 1) * (long long)(d->dz > d->A ? d->dz : d->A) >= (1ll << 31)) return NCX_E_DIMS;      // (row and element counts are ints)
    if ((m->act_v != 0 && m->act_v != 2) || (m->act_q != 0 && m->act_q != 2)) return NCX_E_FLAGS;
    if (!m->wv || !m->bv || !m->wq || !m->bq || !m->whv || !m->bhv || !m->whq || !m->bhq || !m->wc || !m->bc) return NCX_E_NULL;
    return NCX_OK;
}

size_t ncx_vqa_workspace_bytes(const ncx_dims* d, const ncx_mutan_params* m) {
    if (check_mutan(d, m) != NCX_OK) return 0;
    GemmPlan plans[5];
    return vqa_layout(*d, *m, plans).total;
}

int ncx_vqa_route(const ncx_dims* d, const ncx_mutan_params* m, int32_t* out4) {
    if (!out4) return NCX_E_NULL;
    const int rc = check_mutan(d, m);
    if (rc != NCX_OK) return rc;
    const VqaRoute r = vqa_route(*d, *m);
    out4[0] = r.main_v; out4[1] = r.fold; out4[2] = r.main_c ? (r.pad_c ? 2 : 1) : 0;
    out4[3] = r.main_v ? main_chain_form((long long)d->B * (d->K + 1), m->dhv, ksteps(d->dv), 1, true, true) : -1;
    return NCX_OK;
}

int ncx_vqa_ws_region(const ncx_dims* d, const ncx_mutan_params* m, int32_t which, size_t* offset, size_t* bytes) {
    if (!offset || !bytes) return NCX_E_NULL;
    const int rc = check_mutan(d, m);
    if (rc != NCX_OK) return rc;
    GemmPlan plans[5];
    const VqaLayout w = vqa_layout(*d, *m, plans);
    const size_t B = d->B;
    if (which == NCX_VQA_WS_XQ) { *offset = w.xq; *bytes = B * m->dhq * 4; }
    else if (which == NCX_VQA_WS_HQ) { *offset = w.hq; *bytes = B * m->R * d->dz * 4; }
    else if (which == NCX_VQA_WS_XV) { *offset = w.xv; *bytes = B * (d->K + 1) * m->dhv * 4; }
    else return NCX_E_FLAGS;
    return NCX_OK;
}

int ncx_vqa_forward(const ncx_dims* dp, const float* feats, const int32_t* img_idx, const float* q_emb,
                    const ncx_mutan_params* mp, void* workspace, size_t workspace_bytes,
                    float* z_orig, float* z_knns, float* a_knns, float* a_orig, void* stream_) {
    int rc = check_mutan(dp, mp);
    if (rc != NCX_OK) return rc;
    if (!feats || !img_idx || !q_emb || !workspace || !z_orig || !z_knns || !a_knns) return NCX_E_NULL;
    const ncx_dims& d = *dp; const ncx_mutan_params& m = *mp;
    GemmPlan plans[5];
    const VqaLayout w = vqa_layout(d, m, plans);
    const VqaRoute route = vqa_route(d, m);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float* xq = (float*)(ws + w.xq); float* hq = (float*)(ws + w.hq); float* xv = (float*)(ws + w.xv);
    float* slab = (float*)(ws + w.slab);
    const int Mv = d.B * (d.K + 1), RZ = m.R * d.dz;
    {   // x_q = act_q(q . Wq^T + bq)                                            fusion.py:88-93
        GemmArgs a = gemm_nt(d.B, m.dhq, d.dq, q_emb, m.wq, xq, m.act_q);
        rc = run_gemm_planned(a, FORM_NT, plans[0], slab, w.slab_bytes, m.bq, s); if (rc) return rc;
    }
    {   // hq[b][r*dz + j] = x_q . Whq_r^T + bhq_r   (all R at once)               fusion.py:103-107
        GemmArgs a = gemm_nt(d.B, RZ, m.dhq, xq, m.whq, hq, 0);
        rc = run_gemm_planned(a, FORM_NT, plans[1], slab, w.slab_bytes, m.bhq, s); if (rc) return rc;
    }
    if (route.main_v) {
        // x_v on the fused forward kernel (ncx_main.h): one gathered segment, bias + activation in the epilogue (round 3: 249 -> see DESIGN 5b)
        MainArgs a{}; a.M = Mv; a.N = m.dhv; a.nseg = 1;
        a.seg[0].kind = MK_GATHER; a.seg[0].a = feats; a.seg[0].lda = d.dv; a.seg[0].idx = img_idx; a.seg[0].klen = d.dv;
        a.seg[0].b = m.wv; a.seg[0].ldb = d.dv;
        a.out = xv; a.ldo = m.dhv; a.epi.bias = m.bv; a.epi.relu = m.act_v; a.split = 1;
        rc = main_forward(a, s); if (rc) return rc;
    } else
    {   // x_v = act_v(gather(feats, img_idx) . Wv^T + bv) for the B*(K+1) images      fusion.py:82-87 (+ the host gather)
        GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = Mv;
        a.a[0] = x_gather(feats, d.dv, img_idx, Mv, d.dv); a.b[0] = x_plain(m.wv, d.dv, m.dhv, d.dv); a.klen[0] = d.dv;
        a.out[0] = xv; a.ldo[0] = m.dhv; a.n_cols[0] = m.dhv; a.epi.relu = m.act_v;
        rc = run_gemm_planned(a, FORM_NT, plans[2], slab, w.slab_bytes, m.bv, s); if (rc) return rc;
    }
    if (route.fold) {
        // z = sum_r (x_v . Whv_r^T + bhv_r) * hq_r[question] as ONE product per question against Weff_q = sum_r diag(hq_r[q]) Whv_r,
        // built on the vector ALU on the way into LDS (ncx_mutan.hip): 4.2 + 0.7 GF instead of 33.2 at configs[2]        fusion.py:96-115
        rc = mutan_fold(d, m, xv, hq, z_orig, z_knns, s); if (rc) return rc;
    } else
    {   // z = sum_r (x_v . Whv_r^T + bhv_r) * hq_r[question]  -> z_orig / z_knns     fusion.py:96-115
        GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = m.R; a.M = Mv;
        for (int r = 0; r < m.R; ++r) {
            a.a[r] = x_plain(xv, m.dhv, Mv, m.dhv);
            a.b[r] = x_plain(m.whv + (long long)r * d.dz * m.dhv, m.dhv, d.dz, m.dhv);
            a.klen[r] = m.dhv;
        }
        a.out[0] = z_knns; a.ldo[0] = d.dz; a.n_cols[0] = d.dz; a.split[0] = 1;
        a.epi.fold_mul = hq; a.epi.ld_fold = RZ; a.epi.fold_div = d.K + 1; a.epi.fold_bias = m.bhv;
        a.epi.rowsplit_g = d.K + 1; a.epi.out0 = z_orig; a.epi.ldo0 = d.dz;
        rc = run_gemm_nt_fold(a, s); if (rc) return rc;
    }
    if (route.main_c) {      // (the kernel's epilogue wants whole 16-byte pieces per output row)
        // a_knns = z_knns . Wc^T + bc on the fused forward kernel (round 4): 11-12 k-steps per workgroup -> 64 x 64 tiles at three
        // workgroups per CU (the plan the answer-embedding gradient takes); generic engine: 241 us at configs[2]          noatt.py:24-29
        const float* wc = m.wc; long long ldw = d.dz;
        if (route.pad_c) {
            float* wcp = (float*)(ws + w.wcp);
            const int ldd = pad_to(d.dz, 32);
            NCX_HIP_TRY(pad_rows(m.wc, (long long)d.dz, d.dz, wcp, ldd, d.A, s));
            wc = wcp; ldw = ldd;
        }
        MainArgs a{}; a.M = d.B * d.K; a.N = d.A; a.nseg = 1;
        a.seg[0].kind = MK_PLAIN; a.seg[0].a = z_knns; a.seg[0].lda = d.dz; a.seg[0].klen = d.dz; a.seg[0].b = wc; a.seg[0].ldb = ldw;
        a.out = a_knns; a.ldo = d.A; a.epi.bias = m.bc; a.split = 1;
        rc = main_forward(a, s); if (rc) return rc;
    } else
    {   // a_knns = z_knns . Wc^T + bc                                               noatt.py:24-29 (dropout off in eval)
        GemmArgs a = gemm_nt(d.B * d.K, d.A, d.dz, z_knns, m.wc, a_knns, 0);
        rc = run_gemm_planned(a, FORM_NT, plans[4], slab, w.slab_bytes, m.bc, s); if (rc) return rc;
    }
    if (a_orig) {
        GemmArgs a = gemm_nt(d.B, d.A, d.dz, z_orig, m.wc, a_orig, 0);
        a.split[0] = 1;
        GemmPlan pl; pl.cfg = CFG_64x64; pl.split = 1;
        rc = run_gemm_planned(a, FORM_NT, pl, slab, w.slab_bytes, m.bc, s); if (rc) return rc;
    }
    return NCX_OK;
}
}  // extern "C"
