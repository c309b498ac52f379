// ncx_train.h -- what the three VQA trainers below the question encoder share (MutanNoAtt ncx_vqa_train.hip, MLBNoAtt ncx_mlb_train.hip,
// MLBAtt ncx_mlb_att_train.hip + ncx_mlb_att.h): the dropout front end, the GEMM request builders and their runner, the entry points'
// argument checks, and the element-wise kernels that compute the same values in more than one trainer.  The model -- which product is
// which, the workspace regions, the launch order -- stays in each trainer.
//
// The dropout contract of all three:
//   layer ids      Mutan and MLB: 1 v, 2 q, 3 the classifier's input.  MLBAtt: 1 the map fed to conv_v_att, 2 q fed to linear_q_att,
//                  3 x_att, 4 v_att, 5 q fed to linear_q_fusion, 6 t.  TrainDrop::p[layer - 1] is that layer's p.
//   element index  the linear index in the dropped tensor (row * width + column); the GEMM epilogues take the tensor's width as ld_mask.
//   mode 2 masks   the keep masks (0 / 1 floats) concatenated in layer order: Mutan [B dv | B dq | B dz], MLB [B dv | B dq | B dh],
//                  MLBAtt [B dv P | B dq | B P dh_att | B G dv | B dq | B G dh_f].  A kernel is handed its own layer's mask.
//   scale          a kept element is multiplied by 1.f / (1.f - p), computed in fp32 in exactly that form; mode 0 holds p = 0.
// Mode 1 with p == 0 keeps every element without asking the generator; mode 2 always reads its mask.
#pragma once
#include <initializer_list>
#include "ncx_internal.h"

namespace ncx {

// ---- dropout ---------------------------------------------------------------------------------------------------------------------
struct TrainDrop { int mode; float p[6]; unsigned lo, hi; };
constexpr int VQ_LAYER_V = 1, VQ_LAYER_Q = 2, VQ_LAYER_C = 3;      // the layers of the two no-attention trainers
__device__ __forceinline__ bool train_keep(const TrainDrop& k, int layer, const float* mask, long long i) {
    if (k.mode == 1) return k.p[layer - 1] > 0.f ? dropout_keep(k.lo, k.hi, (unsigned)layer, (unsigned long long)i, k.p[layer - 1]) : true;
    if (k.mode == 2) return mask[i] != 0.f;
    return true;
}
__device__ __forceinline__ float train_scale(const TrainDrop& k, int layer) { return k.mode ? 1.f / (1.f - k.p[layer - 1]) : 1.f; }

static inline TrainDrop train_drop(int mode, uint64_t seed, std::initializer_list<float> p) {
    TrainDrop k{};
    k.mode = mode;
    int i = 0;
    if (mode) for (float v : p) k.p[i++] = v;
    k.lo = (unsigned)(seed & 0xFFFFFFFFull); k.hi = (unsigned)(seed >> 32);
    return k;
}
// a layer does anything at all: explicit masks, or the generator with p > 0
static inline bool drop_on(int mode, float p) { return mode == 2 || (mode == 1 && p > 0.f); }
// the same dropout in the epilogue of a GEMM on the generic engine (the backward regenerates, or reads, the forward's mask)
static inline void epi_dropout(EpiArgs& e, int mode, uint64_t seed, float p, unsigned layer, const float* mask, long long ld_mask) {
    if (!drop_on(mode, p)) return;
    e.dropout = mode; e.drop_p = p; e.drop_scale = 1.f / (1.f - p);
    e.seed_lo = (unsigned)(seed & 0xFFFFFFFFull); e.seed_hi = (unsigned)(seed >> 32); e.layer = layer;
    e.keep_mask = mask; e.ld_mask = ld_mask;
}

// ---- GEMM requests on the generic engine --------------------------------------------------------------------------------------------
// out [M, N] = act(X [M, K] . W [N, K]^T + bias); the bias goes in through run_gemm_planned
static inline GemmArgs gemm_nt(int M, int N, int K, const float* X, const float* W, float* out, int act) {
    GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = M;
    a.a[0] = x_plain(X, K, M, K); a.b[0] = x_plain(W, K, N, K); a.klen[0] = K;
    a.out[0] = out; a.ldo[0] = N; a.n_cols[0] = N; a.epi.relu = act;
    return a;
}
// a request: the arguments, the operand form, the plan and the bias of one launch (pointers may be NULL when only sizing the slab)
struct GemmReq { GemmArgs a; int form; GemmPlan pl; const float* bias; };
static inline void req_nt(GemmReq& r, int M, int N, int K, const float* X, const float* W, float* out, int act, const float* bias) {
    r.a = gemm_nt(M, N, K, X, W, out, act);
    r.form = FORM_NT; r.pl = plan_gemm(FORM_NT, M, N, ksteps(K), true); r.bias = bias;
}
// problem i of a TN group: out [Mo, N] = D [B, Mo]^T . X [B, N]; the caller plans the whole group
static inline void gemm_tn_piece(GemmArgs& a, int i, const float* D, long long ldd, int Mo, const float* X, long long ldx, int N, float* out, int B) {
    a.mode = MODE_GROUP; a.nseg = i + 1; a.M = Mo;
    a.a[i] = x_plain(D, ldd, B, Mo); a.b[i] = x_plain(X, ldx, B, N); a.klen[i] = B;
    a.out[i] = out; a.ldo[i] = N; a.n_cols[i] = N;
}
static inline void req_tn(GemmReq& r, long long M, long long N, int B) { r.form = FORM_TN; r.pl = plan_gemm(FORM_TN, M, N, ksteps(B), false); }
// out [B, N] = D [B, K] . W [K, N]
static inline void req_nn(GemmReq& r, int B, const float* D, long long ldd, int K, const float* W, int N, float* out, long long ldo) {
    GemmArgs& a = r.a;
    a.mode = MODE_CHAIN; a.nseg = 1; a.M = B;
    a.a[0] = x_plain(D, ldd, B, K); a.b[0] = x_plain(W, N, K, N); a.klen[0] = K;
    a.out[0] = out; a.ldo[0] = ldo; a.n_cols[0] = N;
    r.form = FORM_NN; r.pl = plan_gemm(FORM_NN, B, N, ksteps(K), false);
}
// ... never split over k: the dropout epilogue does not split
static inline void req_nn_unsplit(GemmReq& r, int B, const float* D, long long ldd, int K, const float* W, int N, float* out, long long ldo) {
    req_nn(r, B, D, ldd, K, W, N, out, ldo);
    r.a.split[0] = 1; r.pl.split = 1;
}
// the split-K slab a trainer needs: the largest over its COUNT requests
template <int COUNT, class Build> static inline size_t max_slab_bytes(Build&& build) {
    size_t sb = 0;
    for (int which = 0; which < COUNT; ++which) {
        const GemmReq r = build(which);
        const size_t t = gemm_slab_bytes(r.a, r.pl);
        sb = t > sb ? t : sb;
    }
    return sb;
}
static inline int run_request(GemmReq r, char* ws, size_t slab, size_t slab_bytes, hipStream_t s) {
    return run_gemm_planned(r.a, r.form, r.pl, (float*)(ws + slab), slab_bytes, r.bias, s);
}

// ---- argument checks ------------------------------------------------------------------------------------------------------------------
static inline bool probs_ok(std::initializer_list<float> ps) {
    for (float p : ps) if (!(p >= 0.f && p < 1.f)) return false;
    return true;
}
// what ncx_vqa_train_dims must satisfy for either no-attention trainer; each adds the limits of its own hidden widths
static inline int vq_check_dims(const ncx_vqa_train_dims* d) {
    if (d->B < 1 || d->dv < 4 || d->dq < 4 || d->dz < 4 || d->A < 4 || d->n_img < 1) return NCX_E_DIMS;
    if (d->dropout_mode < 0 || d->dropout_mode > 2 || !probs_ok({d->p_v, d->p_q, d->p_c})) return NCX_E_DIMS;
    const long long lim = 1ll << 31;
    long long w = d->dv; if (d->dq > w) w = d->dq; if (d->dz > w) w = d->dz; if (d->A > w) w = d->A;
    if (d->B * w >= lim || (long long)d->n_img * d->dv >= lim || (long long)d->A * d->dz >= lim) return NCX_E_DIMS;
    return NCX_OK;
}
// the regions ncx_vqa_train_ws_region and ncx_mlb_train_ws_region expose: the three dropped tensors
static inline int vq_ws_region(const ncx_vqa_train_dims& d, int32_t which, size_t vd, size_t qd, size_t zc, size_t* offset, size_t* bytes) {
    const size_t B = d.B;
    if (which == NCX_VT_WS_VD) { *offset = vd; *bytes = B * d.dv * 4; }
    else if (which == NCX_VT_WS_QD) { *offset = qd; *bytes = B * d.dq * 4; }
    else if (which == NCX_VT_WS_ZC) { *offset = zc; *bytes = B * d.dz * 4; }
    else return NCX_E_FLAGS;
    return NCX_OK;
}

// ---- launch helpers ---------------------------------------------------------------------------------------------------------------------
static inline unsigned grid256(long long n) { return (unsigned)((n + 255) / 256); }
static inline bool al16(const void* p) { return ((uintptr_t)p & 15) == 0; }
static inline const float* ptr_off(const float* p, long long n) { return p ? p + n : nullptr; }
static inline float* ptr_off(float* p, long long n) { return p ? p + n : nullptr; }
__device__ __forceinline__ int clamp_img(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }

// V consecutive floats: one 16-byte access when V == 4 (the caller has checked widths and alignment), one element when V == 1
template <int V> struct TrainVec { float v[V]; };
template <int V> __device__ __forceinline__ TrainVec<V> train_ld(const float* p) {
    TrainVec<V> r;
    if constexpr (V == 4) { const f32x4 t = *(const f32x4*)p; r.v[0] = t[0]; r.v[1] = t[1]; r.v[2] = t[2]; r.v[3] = t[3]; }
    else r.v[0] = p[0];
    return r;
}
template <int V> __device__ __forceinline__ void train_st(float* p, const TrainVec<V>& x) {
    if constexpr (V == 4) { f32x4 t; t[0] = x.v[0]; t[1] = x.v[1]; t[2] = x.v[2]; t[3] = x.v[3]; *(f32x4*)p = t; }
    else p[0] = x.v[0];
}

// ---- the element-wise kernels more than one trainer launches (ncx_train.hip) --------------------------------------------------------
#define NCX_HIDDEN __attribute__((visibility("hidden")))
// vd [B, dv] = drop_v(feats[clamp(img_idx)]), qd [B, dq] = drop_q(q): Mutan and MLB.  One launch; 16 bytes per lane where both widths are
// multiples of 4 and both sources 16-byte aligned, one element otherwise.  masks: [B dv | B dq | ...] or NULL.
NCX_HIDDEN hipError_t train_drop_vq(const ncx_vqa_train_dims& d, const float* feats, const int* img_idx, const float* q, const TrainDrop& k,
                                    const float* masks, float* vd, float* qd, hipStream_t s);
// out[i] = drop_layer(in[i]), i < n (in == out allowed): MLBAtt's q and v_att tensors and dv_att
NCX_HIDDEN hipError_t train_drop_flat(const float* in, float* out, long long n, const TrainDrop& k, int layer, const float* mask, hipStream_t s);
// The backward of t = act_c(x_v * x_q): dz = dt (1 - t^2); dpv = dz x_q (1 - x_v^2); dpq = dz x_v (1 - x_q^2), a tanh factor only where
// that activation is tanh (t is read only then): MLB and MLBAtt.  Every operand is a 256-byte aligned workspace region; 16 bytes per
// lane when n is a multiple of 4.
NCX_HIDDEN hipError_t train_dfuse(const float* dt, const float* t, const float* xv, const float* xq, long long n, int act_v, int act_q, int act_c,
                                  float* dpv, float* dpq, hipStream_t s);
// d *= 1 - y^2 in place over up to two tensors in one launch, for the ones whose activation is tanh (n1 == 0: one tensor): Mutan, MLBAtt
NCX_HIDDEN hipError_t train_dact(float* d0, const float* y0, long long n0, int act0, float* d1, const float* y1, long long n1, int act1, hipStream_t s);
#undef NCX_HIDDEN

}  // namespace ncx
