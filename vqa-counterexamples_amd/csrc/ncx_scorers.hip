// ncx_scorers.hip -- the two trainable scorers besides NeuralModel: LinearContext (reference vqa/models/cx.py:139-156) and
// PairwiseLinearModel (cx.py:379-425), forward and backward.  Loss / Recall (ncx_loss_rank) and Adam (ncx_adam_step) are the
// library's own, unchanged.
//
// PairwiseLinearModel, per candidate k of question b (H = dim_h = 300, da = dim_a = 300):
//   x = cat(v_orig, v_other_k, q_emb, z_orig, z_other_k, E[aid])      (cx.py:416; Din = 2 dv + dq + 2 dz + 300)
//   h = relu(W x + b);  s = relu(w_out . h + b_out)                   (cx.py:417-418)
// The concat is never built.  W splits by column blocks into a per-question part and a per-candidate part:
//   P [B, H]       = [v_orig | q | z_orig | E[aid]] . W_q^T + b        one NT chain of 4 segments (v_orig, E[aid] gathered)
//   h [B K, H]     = relu([v_other | z_other] . W_c^T + P[r / K])      one NT chain of 2 segments, rowadd + ReLU epilogue
//   s [B K]        = relu(h . w_out + b_out)                           k_pl_score, one wave per row
// Backward, given dscores (ncx_loss_rank, a separate launch):
//   k_pl_head      one workgroup per triplet: g = dscores [s > 0], dpre = g w_out [h > 0], dP[b] = sum_k dpre,
//                  per-triplet partials of d out.weight (sum_k g h) and d out.bias (sum_k g)
//   k_colsum       d linear.bias = sum_b dP, d out.weight, d out.bias: fixed-order tree sums over b
//   dW_c           dpre^T . [v_other | z_other]                        one TN group of 2 problems over B K rows
//   dW_q           dP^T . [v_orig | q | z_orig | E[aid]]               one TN group of 4 problems over B rows
//   dA [B, 300]    dP . W[:, a-cols]                                   NN
//   k_pl_demb      d answer_embedding[a] = sum over b with aid_b == a of dA[b], b ascending (owner computes: one
//                  workgroup per row of E, every row written, zero where no id points; no atomics)
// LinearContext: scores = z_flat [B, K dz] . W^T + b (NT, split-K over the 8640-long reduction), dW = dscores^T . z_flat (TN,
// reduction over B), db = sum_b dscores (k_colsum).
// Ids: k_pl_prep clamps every feature-table row and answer id into range before any gather reads them and sets *bad_id_flag
// when it had to (the reference raises IndexError there); the clamped ids are what the kernels use.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ncx_internal.h"

namespace ncx {

constexpr int PL_H = 300;     // dim_h (cx.py:391)
constexpr int PL_DA = 300;     // dim_a (cx.py:392)
constexpr int SC_MAX_K = 64;   // ncx_loss_rank's bound

struct PlLayout {
    size_t idx_o, aid, idx_k, P, h, s, dpre, dP, pw, pg, dA, slab, slab_bytes, total;
};
struct PlCols { int v_orig, v_other, q, z_orig, z_other, a, din; };
static inline PlCols pl_cols(const ncx_scorer_dims& d) {
    PlCols c; int o = 0;
    c.v_orig = o; o += d.dv; c.v_other = o; o += d.dv; c.q = o; o += d.dq; c.z_orig = o; o += d.dz; c.z_other = o; o += d.dz;
    c.a = o; o += PL_DA; c.din = o;
    return c;
}

static bool scorer_dims_ok(const ncx_scorer_dims* d, bool pairlin) {
    if (d->B < 1 || d->K < 1 || d->K > SC_MAX_K || d->dz < 1) return false;
    if ((long long)d->K * d->dz < 4 || (long long)d->B * d->K * d->dz >= (1ll << 31)) return false;
    if (!pairlin) return true;
    if (d->dv < 4 || d->dq < 4 || d->dz < 4 || d->A < 1 || d->n_img < 1) return false;
    const long long M = (long long)d->B * d->K;
    return M * PL_H < (1ll << 31) && M * d->dv < (1ll << 31) && (long long)d->n_img * d->dv < (1ll << 31) &&
           (long long)d->A * PL_DA < (1ll << 31);
}

// ---- PairwiseLinearModel: the GEMMs (pointers may be NULL when only sizing the slab) -------------------------------------
struct PlPtrs {
    const float *feats, *q, *z_o, *z_k, *E, *W, *b;
    const int *idx_o, *idx_k, *aid;
    float *P, *h, *dpre, *dP, *dA, *gW;
};
static GemmArgs pl_gemm_p(const ncx_scorer_dims& d, const PlPtrs& p, GemmPlan* pl) {
    const PlCols c = pl_cols(d);
    GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 4; a.M = d.B;
    a.a[0] = x_gather(p.feats, d.dv, p.idx_o, d.B, d.dv); a.b[0] = x_plain(p.W + c.v_orig, c.din, PL_H, d.dv); a.klen[0] = d.dv;
    a.a[1] = x_plain(p.q, d.dq, d.B, d.dq);               a.b[1] = x_plain(p.W + c.q, c.din, PL_H, d.dq);      a.klen[1] = d.dq;
    a.a[2] = x_plain(p.z_o, d.dz, d.B, d.dz);             a.b[2] = x_plain(p.W + c.z_orig, c.din, PL_H, d.dz); a.klen[2] = d.dz;
    a.a[3] = x_gather(p.E, PL_DA, p.aid, d.B, PL_DA);     a.b[3] = x_plain(p.W + c.a, c.din, PL_H, PL_DA);     a.klen[3] = PL_DA;
    a.out[0] = p.P; a.ldo[0] = PL_H; a.n_cols[0] = PL_H;
    a.epi.bias = p.b;
    *pl = plan_gemm(FORM_NT, d.B, PL_H, ksteps(d.dv) + ksteps(d.dq) + ksteps(d.dz) + ksteps(PL_DA), false);
    return a;
}
static GemmArgs pl_gemm_h(const ncx_scorer_dims& d, const PlPtrs& p, GemmPlan* pl) {
    const PlCols c = pl_cols(d);
    const int M = d.B * d.K;
    GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 2; a.M = M;
    a.a[0] = x_gather(p.feats, d.dv, p.idx_k, M, d.dv); a.b[0] = x_plain(p.W + c.v_other, c.din, PL_H, d.dv); a.klen[0] = d.dv;
    a.a[1] = x_plain(p.z_k, d.dz, M, d.dz);            a.b[1] = x_plain(p.W + c.z_other, c.din, PL_H, d.dz); a.klen[1] = d.dz;
    a.out[0] = p.h; a.ldo[0] = PL_H; a.n_cols[0] = PL_H; a.split[0] = 1;        // the rowadd epilogue does not split
    a.epi.rowadd = p.P; a.epi.ld_rowadd = PL_H; a.epi.rowdiv = d.K; a.epi.relu = 1;
    *pl = plan_gemm(FORM_NT, M, PL_H, ksteps(d.dv) + ksteps(d.dz), true);
    pl->split = 1;
    return a;
}
static GemmArgs pl_gemm_dwc(const ncx_scorer_dims& d, const PlPtrs& p, GemmPlan* pl) {
    const PlCols c = pl_cols(d);
    const int M = d.B * d.K;
    GemmArgs a{}; a.mode = MODE_GROUP; a.nseg = 2; a.M = PL_H;
    a.a[0] = x_plain(p.dpre, PL_H, M, PL_H); a.b[0] = x_gather(p.feats, d.dv, p.idx_k, M, d.dv); a.klen[0] = M;
    a.out[0] = p.gW ? p.gW + c.v_other : nullptr; a.ldo[0] = c.din; a.n_cols[0] = d.dv;
    a.a[1] = x_plain(p.dpre, PL_H, M, PL_H); a.b[1] = x_plain(p.z_k, d.dz, M, d.dz);           a.klen[1] = M;
    a.out[1] = p.gW ? p.gW + c.z_other : nullptr; a.ldo[1] = c.din; a.n_cols[1] = d.dz;
    *pl = plan_gemm(FORM_TN, PL_H, d.dv + d.dz, ksteps(M), false);
    return a;
}
static GemmArgs pl_gemm_dwq(const ncx_scorer_dims& d, const PlPtrs& p, GemmPlan* pl) {
    const PlCols c = pl_cols(d);
    GemmArgs a{}; a.mode = MODE_GROUP; a.nseg = 4; a.M = PL_H;
    const XDesc xs[4] = {x_gather(p.feats, d.dv, p.idx_o, d.B, d.dv), x_plain(p.q, d.dq, d.B, d.dq), x_plain(p.z_o, d.dz, d.B, d.dz),
                         x_gather(p.E, PL_DA, p.aid, d.B, PL_DA)};
    const int off[4] = {c.v_orig, c.q, c.z_orig, c.a};
    for (int i = 0; i < 4; ++i) {
        a.a[i] = x_plain(p.dP, PL_H, d.B, PL_H); a.b[i] = xs[i]; a.klen[i] = d.B;
        a.out[i] = p.gW ? p.gW + off[i] : nullptr; a.ldo[i] = c.din; a.n_cols[i] = xs[i].cols;
    }
    *pl = plan_gemm(FORM_TN, PL_H, d.dv + d.dq + d.dz + PL_DA, ksteps(d.B), false);
    return a;
}
static GemmArgs pl_gemm_da(const ncx_scorer_dims& d, const PlPtrs& p, GemmPlan* pl) {
    const PlCols c = pl_cols(d);
    GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = d.B;
    a.a[0] = x_plain(p.dP, PL_H, d.B, PL_H); a.b[0] = x_plain(p.W + c.a, c.din, PL_H, PL_DA); a.klen[0] = PL_H;
    a.out[0] = p.dA; a.ldo[0] = PL_DA; a.n_cols[0] = PL_DA;
    *pl = plan_gemm(FORM_NN, d.B, PL_DA, ksteps(PL_H), false);
    return a;
}

static PlLayout pl_layout(const ncx_scorer_dims& d) {
    PlLayout w{}; WsCarver cv;
    const size_t B = d.B, M = (size_t)d.B * d.K;
    w.idx_o = cv.take(B * 4); w.aid = cv.take(B * 4); w.idx_k = cv.take(M * 4);
    w.P = cv.take(B * PL_H * 4); w.h = cv.take(M * PL_H * 4); w.s = cv.take(M * 4); w.dpre = cv.take(M * PL_H * 4);
    w.dP = cv.take(B * PL_H * 4); w.pw = cv.take(B * PL_H * 4); w.pg = cv.take(B * 4); w.dA = cv.take(B * PL_DA * 4);
    PlPtrs p{}; GemmPlan pl; size_t sb = 0, t;
    GemmArgs a = pl_gemm_p(d, p, &pl);   t = gemm_slab_bytes(a, pl); sb = t > sb ? t : sb;
    a = pl_gemm_dwc(d, p, &pl);          t = gemm_slab_bytes(a, pl); sb = t > sb ? t : sb;
    a = pl_gemm_dwq(d, p, &pl);          t = gemm_slab_bytes(a, pl); sb = t > sb ? t : sb;
    a = pl_gemm_da(d, p, &pl);           t = gemm_slab_bytes(a, pl); sb = t > sb ? t : sb;
    w.slab = cv.take(sb); w.slab_bytes = sb;
    w.total = cv.off;
    return w;
}

// ---- kernels ----------------------------------------------------------------------------------------------------------------
// Clamped feature-table rows of the original images [B] and of the candidates [B K], clamped answer ids [B].
__global__ __launch_bounds__(256) void k_pl_prep(const int* __restrict__ img_idx, const int* __restrict__ aids, int B, int K, int n_img,
                                                 int A, int* __restrict__ idx_o, int* __restrict__ idx_k, int* __restrict__ aid_c,
                                                 int* __restrict__ bad) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    const long long n = (long long)B * (K + 1);
    if (i < n) {
        const int b = (int)(i / (K + 1)), j = (int)(i % (K + 1));
        int v = img_idx[i];
        if (v < 0 || v >= n_img) { *bad = 1; v = v < 0 ? 0 : n_img - 1; }
        if (j == 0) idx_o[b] = v; else idx_k[(long long)b * K + j - 1] = v;
    }
    if (i < B) {
        int a = aids[i];
        if (a < 0 || a >= A) { *bad = 1; a = a < 0 ? 0 : A - 1; }
        aid_c[i] = a;
    }
}

// s[r] = relu(h[r] . w_out + b_out): one wave per row, lane-strided dot product, fixed butterfly.
__global__ __launch_bounds__(256) void k_pl_score(const float* __restrict__ h, const float* __restrict__ w_out, const float* __restrict__ b_out,
                                                  int M, float* __restrict__ s_ws, float* __restrict__ scores) {
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (r >= M) return;
    const float* hr = h + (long long)r * PL_H;
    float acc = 0.f;
    for (int c = lane; c < PL_H; c += 64) acc = fmaf(hr[c], w_out[c], acc);
    for (int o = 32; o > 0; o >>= 1) acc += __shfl_xor(acc, o);
    if (lane == 0) {
        const float v = acc + b_out[0];
        const float sv = v > 0.f ? v : 0.f;
        s_ws[r] = sv; scores[r] = sv;
    }
}

// One workgroup per triplet b; thread t owns columns t, t + 256 of H.
__global__ __launch_bounds__(256) void k_pl_head(const float* __restrict__ dscores, const float* __restrict__ s_ws, const float* __restrict__ h,
                                                 const float* __restrict__ w_out, int K, float* __restrict__ dpre, float* __restrict__ dP,
                                                 float* __restrict__ pw, float* __restrict__ pg) {
    const int b = blockIdx.x, t = threadIdx.x;
    __shared__ float g_s[SC_MAX_K];
    if (t < K) {
        const long long r = (long long)b * K + t;
        g_s[t] = s_ws[r] > 0.f ? dscores[r] : 0.f;                  // d relu(score) (cx.py:418)
    }
    __syncthreads();
    if (t == 0) {
        float sg = 0.f;
        for (int k = 0; k < K; ++k) sg += g_s[k];
        pg[b] = sg;
    }
    for (int c = t; c < PL_H; c += 256) {
        const float wc = w_out[c];
        float adp = 0.f, aw = 0.f;
        for (int k = 0; k < K; ++k) {
            const long long r = (long long)b * K + k;
            const float hv = h[r * PL_H + c], g = g_s[k];
            const float dp = hv > 0.f ? g * wc : 0.f;               // d relu(linear(x)) (cx.py:417)
            dpre[r * PL_H + c] = dp;
            adp += dp;
            aw = fmaf(g, hv, aw);
        }
        dP[(long long)b * PL_H + c] = adp;
        pw[(long long)b * PL_H + c] = aw;
    }
}

// out[c] = sum over rows r < R of in[r * ld + c]: one workgroup per column, each thread a fixed stride of rows, then a fixed
// LDS tree (deterministic).  colsum_rows (ncx_internal.h) is its launcher: the contrastive path sums with it too.
static __global__ __launch_bounds__(256) void k_colsum(const float* __restrict__ in, long long ld, int R, float* __restrict__ out) {
    const int c = blockIdx.x, t = threadIdx.x;
    __shared__ float red[256];
    float acc = 0.f;
    for (int r = t; r < R; r += 256) acc += in[(long long)r * ld + c];
    red[t] = acc;
    __syncthreads();
    for (int o = 128; o > 0; o >>= 1) {
        if (t < o) red[t] += red[t + o];
        __syncthreads();
    }
    if (t == 0) out[c] = red[0];
}
hipError_t colsum_rows(const float* in, long long ld, int R, int cols, float* out, hipStream_t s) {
    hipLaunchKernelGGL(k_colsum, dim3(cols), dim3(256), 0, s, in, ld, R, out);
    return hipGetLastError();
}

// d answer_embedding: row a = sum of dA[b] over the b with aid_c[b] == a, b ascending; every row written.
constexpr int DEMB_CHUNK = 1024;
__global__ __launch_bounds__(256) void k_pl_demb(const float* __restrict__ dA, const int* __restrict__ aid_c, int B, float* __restrict__ gE) {
    const int a = blockIdx.x, t = threadIdx.x;
    __shared__ int ids[DEMB_CHUNK];
    float acc0 = 0.f, acc1 = 0.f;
    const int c0 = t, c1 = t + 256;
    for (int b0 = 0; b0 < B; b0 += DEMB_CHUNK) {
        const int n = B - b0 < DEMB_CHUNK ? B - b0 : DEMB_CHUNK;
        __syncthreads();
        for (int i = t; i < n; i += 256) ids[i] = aid_c[b0 + i];
        __syncthreads();
        for (int i = 0; i < n; ++i) {
            if (ids[i] == a) {
                const float* row = dA + (long long)(b0 + i) * PL_DA;
                acc0 += row[c0];
                if (c1 < PL_DA) acc1 += row[c1];
            }
        }
    }
    gE[(long long)a * PL_DA + c0] = acc0;
    if (c1 < PL_DA) gE[(long long)a * PL_DA + c1] = acc1;
}

// [B, K] -> [B, 4] zero padded (the engine's operand windows are 4 floats wide)
__global__ __launch_bounds__(256) void k_pad4(const float* __restrict__ in, int B, int K, float* __restrict__ out) {
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= B * 4) return;
    const int b = i / 4, k = i % 4;
    out[i] = k < K ? in[(long long)b * K + k] : 0.f;
}

// ---- LinearContext ----------------------------------------------------------------------------------------------------------
static GemmArgs lc_gemm_fwd(const ncx_scorer_dims& d, const float* z, const float* W, const float* b, float* scores, GemmPlan* pl) {
    const int kd = d.K * d.dz;
    GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = d.B;
    a.a[0] = x_plain(z, kd, d.B, kd); a.b[0] = x_plain(W, kd, d.K, kd); a.klen[0] = kd;
    a.out[0] = scores; a.ldo[0] = d.K; a.n_cols[0] = d.K; a.epi.bias = b;
    *pl = plan_gemm(FORM_NT, d.B, d.K, ksteps(kd), false);
    return a;
}
static GemmArgs lc_gemm_dw(const ncx_scorer_dims& d, const float* z, const float* ds, long long ld_ds, float* gW, GemmPlan* pl) {
    const int kd = d.K * d.dz;
    GemmArgs a{}; a.mode = MODE_GROUP; a.nseg = 1; a.M = d.K;
    a.a[0] = x_plain(ds, ld_ds, d.B, (int)ld_ds); a.b[0] = x_plain(z, kd, d.B, kd); a.klen[0] = d.B;
    a.out[0] = gW; a.ldo[0] = kd; a.n_cols[0] = kd;
    *pl = plan_gemm(FORM_TN, d.K, kd, ksteps(d.B), false);
    return a;
}
struct LcLayout { size_t pad, slab, slab_bytes, total; };
static LcLayout lc_layout(const ncx_scorer_dims& d) {
    LcLayout w{}; WsCarver cv;
    w.pad = cv.take(d.K < 4 ? (size_t)d.B * 16 : 0);
    GemmPlan pl; size_t sb, t;
    GemmArgs a = lc_gemm_fwd(d, nullptr, nullptr, nullptr, nullptr, &pl); sb = gemm_slab_bytes(a, pl);
    a = lc_gemm_dw(d, nullptr, nullptr, d.K < 4 ? 4 : d.K, nullptr, &pl); t = gemm_slab_bytes(a, pl); sb = t > sb ? t : sb;
    w.slab = cv.take(sb); w.slab_bytes = sb; w.total = cv.off > 256 ? cv.off : 256;      // (0 is the "unsupported dims" answer)
    return w;
}

}  // namespace ncx

using namespace ncx;

extern "C" size_t ncx_pairlin_workspace_bytes(const ncx_scorer_dims* d) {
    if (!d || !scorer_dims_ok(d, true)) return 0;
    return pl_layout(*d).total;
}

extern "C" int ncx_pairlin_forward(const ncx_scorer_dims* dp, const ncx_inputs* in, const ncx_pairlin_params* p, void* ws, size_t ws_bytes,
                                   float* scores, int32_t* bad_id_flag, void* stream_) {
    if (!dp || !in || !p || !ws || !scores || !bad_id_flag) return NCX_E_NULL;
    if (!in->feats || !in->img_idx || !in->q_emb || !in->z_orig || !in->z_knns || !in->answer_aids) return NCX_E_NULL;
    if (!p->answer_embedding || !p->w || !p->b || !p->w_out || !p->b_out) return NCX_E_NULL;
    if (!scorer_dims_ok(dp, true)) return NCX_E_DIMS;
    const ncx_scorer_dims& d = *dp;
    const PlLayout w = pl_layout(d);
    if (!ws_ok(ws, ws_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    const int M = d.B * d.K;
    PlPtrs q{};
    q.feats = in->feats; q.q = in->q_emb; q.z_o = in->z_orig; q.z_k = in->z_knns; q.E = p->answer_embedding; q.W = p->w; q.b = p->b;
    q.idx_o = (int*)(base + w.idx_o); q.idx_k = (int*)(base + w.idx_k); q.aid = (int*)(base + w.aid);
    q.P = (float*)(base + w.P); q.h = (float*)(base + w.h);
    const long long n = (long long)d.B * (d.K + 1);
    hipLaunchKernelGGL(k_pl_prep, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, in->img_idx, in->answer_aids, d.B, d.K, d.n_img, d.A,
                       (int*)q.idx_o, (int*)q.idx_k, (int*)q.aid, (int*)bad_id_flag);
    NCX_HIP_TRY(hipGetLastError());
    GemmPlan pl;
    GemmArgs a = pl_gemm_p(d, q, &pl);
    int rc = run_gemm_planned(a, FORM_NT, pl, (float*)(base + w.slab), w.slab_bytes, nullptr, s); if (rc) return rc;
    a = pl_gemm_h(d, q, &pl);
    rc = run_gemm_planned(a, FORM_NT, pl, (float*)(base + w.slab), w.slab_bytes, nullptr, s); if (rc) return rc;
    hipLaunchKernelGGL(k_pl_score, dim3((unsigned)((M + 3) / 4)), dim3(256), 0, s, (const float*)q.h, p->w_out, p->b_out, M,
                       (float*)(base + w.s), scores);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

extern "C" int ncx_pairlin_backward(const ncx_scorer_dims* dp, const ncx_inputs* in, const ncx_pairlin_params* p, void* ws, size_t ws_bytes,
                                    const float* dscores, const ncx_pairlin_grads* g, void* stream_) {
    if (!dp || !in || !p || !ws || !dscores || !g) return NCX_E_NULL;
    if (!in->feats || !in->q_emb || !in->z_orig || !in->z_knns) return NCX_E_NULL;
    if (!p->answer_embedding || !p->w || !p->w_out) return NCX_E_NULL;
    if (!g->answer_embedding || !g->w || !g->b || !g->w_out || !g->b_out) return NCX_E_NULL;
    if (!scorer_dims_ok(dp, true)) return NCX_E_DIMS;
    const ncx_scorer_dims& d = *dp;
    const PlLayout w = pl_layout(d);
    if (!ws_ok(ws, ws_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* base = (char*)ws;
    PlPtrs q{};
    q.feats = in->feats; q.q = in->q_emb; q.z_o = in->z_orig; q.z_k = in->z_knns; q.E = p->answer_embedding; q.W = p->w;
    q.idx_o = (int*)(base + w.idx_o); q.idx_k = (int*)(base + w.idx_k); q.aid = (int*)(base + w.aid);
    q.h = (float*)(base + w.h); q.dpre = (float*)(base + w.dpre); q.dP = (float*)(base + w.dP); q.dA = (float*)(base + w.dA); q.gW = g->w;
    float* pw = (float*)(base + w.pw);
    float* pg = (float*)(base + w.pg);
    hipLaunchKernelGGL(k_pl_head, dim3(d.B), dim3(256), 0, s, dscores, (const float*)(base + w.s), (const float*)q.h, p->w_out, d.K,
                       q.dpre, q.dP, pw, pg);
    NCX_HIP_TRY(hipGetLastError());
    NCX_HIP_TRY(colsum_rows((const float*)q.dP, (long long)PL_H, d.B, PL_H, g->b, s));
    NCX_HIP_TRY(colsum_rows((const float*)pw, (long long)PL_H, d.B, PL_H, g->w_out, s));
    NCX_HIP_TRY(colsum_rows((const float*)pg, 1ll, d.B, 1, g->b_out, s));
    GemmPlan pl;
    GemmArgs a = pl_gemm_dwc(d, q, &pl);
    int rc = run_gemm_planned(a, FORM_TN, pl, (float*)(base + w.slab), w.slab_bytes, nullptr, s); if (rc) return rc;
    a = pl_gemm_dwq(d, q, &pl);
    rc = run_gemm_planned(a, FORM_TN, pl, (float*)(base + w.slab), w.slab_bytes, nullptr, s); if (rc) return rc;
    a = pl_gemm_da(d, q, &pl);
    rc = run_gemm_planned(a, FORM_NN, pl, (float*)(base + w.slab), w.slab_bytes, nullptr, s); if (rc) return rc;
    hipLaunchKernelGGL(k_pl_demb, dim3(d.A), dim3(256), 0, s, (const float*)q.dA, q.aid, d.B, g->answer_embedding);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

extern "C" size_t ncx_linctx_workspace_bytes(const ncx_scorer_dims* d) {
    if (!d || !scorer_dims_ok(d, false)) return 0;
    return lc_layout(*d).total;
}

extern "C" int ncx_linctx_forward(const ncx_scorer_dims* dp, const float* z_knns, const float* w, const float* b, void* ws, size_t ws_bytes,
                                  float* scores, void* stream_) {
    if (!dp || !z_knns || !w || !b || !ws || !scores) return NCX_E_NULL;
    if (!scorer_dims_ok(dp, false)) return NCX_E_DIMS;
    const LcLayout l = lc_layout(*dp);
    if (!ws_ok(ws, ws_bytes, l.total)) return NCX_E_WORKSPACE;
    GemmPlan pl;
    GemmArgs a = lc_gemm_fwd(*dp, z_knns, w, b, scores, &pl);
    return run_gemm_planned(a, FORM_NT, pl, (float*)((char*)ws + l.slab), l.slab_bytes, nullptr, (hipStream_t)stream_);
}

extern "C" int ncx_linctx_backward(const ncx_scorer_dims* dp, const float* z_knns, const float* dscores, void* ws, size_t ws_bytes,
                                   float* gw, float* gb, void* stream_) {
    if (!dp || !z_knns || !dscores || !ws || !gw || !gb) return NCX_E_NULL;
    if (!scorer_dims_ok(dp, false)) return NCX_E_DIMS;
    const ncx_scorer_dims& d = *dp;
    const LcLayout l = lc_layout(d);
    if (!ws_ok(ws, ws_bytes, l.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    const float* ds = dscores;
    long long ld = d.K;
    if (d.K < 4) {
        float* pad = (float*)((char*)ws + l.pad);
        hipLaunchKernelGGL(k_pad4, dim3((unsigned)((d.B * 4 + 255) / 256)), dim3(256), 0, s, dscores, d.B, d.K, pad);
        NCX_HIP_TRY(hipGetLastError());
        ds = pad; ld = 4;
    }
    GemmPlan pl;
    GemmArgs a = lc_gemm_dw(d, z_knns, ds, ld, gw, &pl);
    int rc = run_gemm_planned(a, FORM_TN, pl, (float*)((char*)ws + l.slab), l.slab_bytes, nullptr, s); if (rc) return rc;
    NCX_HIP_TRY(colsum_rows(dscores, (long long)d.K, d.B, d.K, gb, s));
    return NCX_OK;
}
