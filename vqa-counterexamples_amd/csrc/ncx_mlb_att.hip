// ncx_mlb_att.hip -- the MLB attention model (MLBAtt in eval mode) below the question encoder: ncx_mlb_att_workspace_bytes,
// ncx_mlb_att_forward.
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
#include "ncx_internal.h"
#include "ncx_wave.h"

using namespace ncx;

namespace {
constexpr int ATT_BN = 64;            // hidden columns per tile of k_att_logits
constexpr int ATT_XP = ATT_BN + 1;    // pitch of the x_att tile in LDS (threads of the contraction walk p: odd pitch, no conflicts)
constexpr int ATT_MAX_G = 8;
constexpr int ATT_MAX_GP = 12288;     // G * P floats of k_att_pool's LDS copy of the maps

struct AttArgs {
    const float* feats; const int* img_idx;
    const float* wv; const float* bv; const float* xq; const float* wa;
    float* slab;
    int P, dv, dh, G, n_img, HT, PT, act_v, act_mm;
};

// TM: positions per tile, 208 or 64
template <int TM> struct AttCfg {
    static constexpr int LOAD_M = (TM + 31) / 32 * 32;        // the loader's tile extent: whole 32-column chunks
    typedef OpLoader<false, LOAD_M> ALoad;                     // the map: [32 channels][LOAD_M positions]
    typedef OpLoader<true, ATT_BN> BLoad;                      // conv_v_att.weight: [64 hidden][32 channels]
    static constexpr int A_ELEMS = ALoad::ELEMS, B_ELEMS = BLoad::ELEMS;
    static constexpr int TILE_FLOATS = 2 * (A_ELEMS + B_ELEMS);
    static constexpr int EPI_FLOATS = TM * ATT_XP + ATT_MAX_G * ATT_BN;
    static constexpr int LDS_BYTES = (TILE_FLOATS > EPI_FLOATS ? TILE_FLOATS : EPI_FLOATS) * 4;
    static constexpr int WAVES_M = TM == 64 ? 2 : 1, WAVES_N = 4 / WAVES_M;
    static constexpr int WM = TM / 16 / WAVES_M, WN = ATT_BN / 16 / WAVES_N;      // 16 x 16 blocks per wave
    static_assert(TM % (16 * WAVES_M) == 0 && ATT_BN % (16 * WAVES_N) == 0, "wave tiles");
};

__device__ __forceinline__ float att_act(float v, int act) { return act == 2 ? tanhf(v) : v; }
__device__ __forceinline__ int clamp_img(int i, int n) { return i < 0 ? 0 : i >= n ? n - 1 : i; }

// One workgroup: TM positions of one image x 64 hidden columns, reduction over the dv channels.
template <int TM>
__global__ __launch_bounds__(256, 2) void k_att_logits(const AttArgs a) {
    typedef AttCfg<TM> Cfg;
    constexpr int PA = Cfg::ALoad::PITCH, PB = Cfg::BLoad::PITCH, WM = Cfg::WM, WN = Cfg::WN, BK = GEMM_BK;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    float* const lds_a = smem;
    float* const lds_b = smem + 2 * Cfg::A_ELEMS;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int wm0 = (wave / Cfg::WAVES_N) * (WM * 16), wn0 = (wave % Cfg::WAVES_N) * (WN * 16);
    int id = blockIdx.x;
    const int pt = id % a.PT; id /= a.PT;
    const int ht = id % a.HT;
    const int b = id / a.HT;
    const int p0 = pt * TM, h0 = ht * ATT_BN;
    const int img = clamp_img(a.img_idx[b], a.n_img);

    XDesc da{}; da.base = a.feats + (long long)img * a.dv * a.P;      // 64-bit image base; 32-bit offsets inside the image
    da.ld = a.P; da.kind = X_PLAIN; da.rows = a.dv; da.cols = a.P; da.idx_stride = 1;
    XDesc db{}; db.base = a.wv; db.ld = a.dv; db.kind = X_PLAIN; db.rows = a.dh; db.cols = a.dv; db.idx_stride = 1;

    typename Cfg::ALoad la;
    typename Cfg::BLoad lb;
    la.setup(da, p0, tid);
    lb.setup(db, h0, tid);

    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int dv = a.dv;
    // whole 32-channel steps take the loader's straight-line path (position windows clamped and repaired, hidden rows beyond dh_att
    // zeroed); the ragged last step takes its bounds-checked path
    auto issue = [&](int k) __attribute__((always_inline)) {
        if (k + BK <= dv) { la.template issue_fast<X_PLAIN, true>(da, k, tid); lb.template issue_fast<X_PLAIN, true>(db, k, tid); }
        else { la.issue(da, k, tid); lb.issue(db, k, tid); }
    };
    auto store = [&](int k, int buf) __attribute__((always_inline)) {
        float* pa = lds_a + buf * Cfg::A_ELEMS; float* pb = lds_b + buf * Cfg::B_ELEMS;
        if (k + BK <= dv) { la.template store_fast<X_PLAIN, true>(pa, tid); lb.template store_fast<X_PLAIN, true>(pb, tid); }
        else { la.store(pa, k, tid); lb.store(pb, k, tid); }
    };
    issue(0);
    store(0, 0);
    __syncthreads();
    int buf = 0;
    for (int k = 0; k < dv; k += BK) {
        const bool has_next = k + BK < dv;
        if (has_next) issue(k + BK);             // in flight under the first three sub-steps
        const float* pa = lds_a + buf * Cfg::A_ELEMS;
        const float* pb = lds_b + buf * Cfg::B_ELEMS;
#pragma unroll
        for (int t = 0; t < BK / 8; ++t) {
            // the next tile goes to the other buffer before the last sub-step: its ds_writes drain under that sub-step's MFMAs
            // (measured against storing after the last sub-step: 1.71 -> 1.65 ms per batch of 128)
            if (t == BK / 8 - 1 && has_next) store(k + BK, buf ^ 1);
            const int kk = t * 8 + 2 * lk;       // MFMA (t, e) takes k = 8 t + 2 lk + e from lane group lk, for both operands
            f32x2 af[WM], bf[WN];
#pragma unroll
            for (int i = 0; i < WM; ++i) af[i] = f32x2{pa[kk * PA + wm0 + i * 16 + li], pa[(kk + 1) * PA + wm0 + i * 16 + li]};
#pragma unroll
            for (int j = 0; j < WN; ++j) bf[j] = *(const f32x2*)(pb + (wn0 + j * 16 + li) * PB + kk);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < WM; ++i)
#pragma unroll
                    for (int j = 0; j < WN; ++j)
                        acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(af[i][e], bf[j][e], acc[i][j], 0, 0, 0);
        }
        __syncthreads();
        buf ^= 1;
    }

    // ---- epilogue: x_att tile -> LDS, then the contraction with conv_att.weight over this tile's hidden columns -------------------
    float* const xs = smem;                         // [TM][ATT_XP]  (the operand tiles are dead: the loop ended on a barrier)
    float* const was = smem + TM * ATT_XP;          // [G][64]
#pragma unroll
    for (int j = 0; j < WN; ++j) {
        const int hl = wn0 + j * 16 + li, h = h0 + hl, hc = min(h, a.dh - 1);
        const float bias = a.bv[hc], xq = a.xq[(long long)b * a.dh + hc];
#pragma unroll
        for (int i = 0; i < WM; ++i)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int pl = wm0 + i * 16 + lk * 4 + q;
                float v = att_act(acc[i][j][q] + bias, a.act_v) * xq;
                v = att_act(v, a.act_mm);
                xs[pl * ATT_XP + hl] = h < a.dh ? v : 0.f;
            }
    }
    for (int i = tid; i < a.G * ATT_BN; i += 256) {
        const int g = i / ATT_BN, hl = i - g * ATT_BN;
        was[i] = h0 + hl < a.dh ? a.wa[(long long)g * a.dh + h0 + hl] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < a.G * TM; i += 256) {
        const int g = i / TM, pl = i - g * TM, p = p0 + pl;
        if (p >= a.P) continue;
        float s = 0.f;
#pragma unroll 16
        for (int hl = 0; hl < ATT_BN; ++hl) s = __builtin_fmaf(xs[pl * ATT_XP + hl], was[g * ATT_BN + hl], s);
        a.slab[(((long long)b * a.HT + ht) * a.G + g) * a.P + p] = s;
    }
}

// P < 4: one workgroup per (question, position); thread t takes the hidden units t, t + 256, ...; fixed-order block sum.  HT == 1.
__global__ __launch_bounds__(256) void k_att_logits_small(const AttArgs a) {
    __shared__ float red[ATT_MAX_G][256];
    const int tid = threadIdx.x;
    const int p = blockIdx.x % a.P, b = blockIdx.x / a.P;
    const int img = clamp_img(a.img_idx[b], a.n_img);
    const float* v = a.feats + (long long)img * a.dv * a.P + p;
    float t[ATT_MAX_G];
#pragma unroll
    for (int g = 0; g < ATT_MAX_G; ++g) t[g] = 0.f;
    for (int h = tid; h < a.dh; h += 256) {
        const float* w = a.wv + (long long)h * a.dv;
        float s = 0.f;
        for (int c = 0; c < a.dv; ++c) s = __builtin_fmaf(v[c * a.P], w[c], s);
        float x = att_act(s + a.bv[h], a.act_v) * a.xq[(long long)b * a.dh + h];
        x = att_act(x, a.act_mm);
#pragma unroll
        for (int g = 0; g < ATT_MAX_G; ++g)
            if (g < a.G) t[g] = __builtin_fmaf(a.wa[(long long)g * a.dh + h], x, t[g]);
    }
#pragma unroll
    for (int g = 0; g < ATT_MAX_G; ++g) red[g][tid] = t[g];
    __syncthreads();
    if (tid < a.G) {
        float s = 0.f;
        for (int i = 0; i < 256; ++i) s += red[tid][i];
        a.slab[((long long)b * a.G + tid) * a.P + p] = s;
    }
}

struct PoolArgs {
    const float* feats; const int* img_idx; const float* slab; const float* ba;
    float* att; float* v_att;
    int P, dv, G, n_img, HT, rows_per_chunk;
};

// grid (channel chunks, B).  Every workgroup rebuilds the image's G maps in LDS (HT x G x P slab reads: small beside its share of
// the map); chunk 0 writes them to `att`.  Then wave w takes the rows c0 + w, c0 + w + 4, ... of its chunk: 16-byte loads along p,
// one dot per glimpse, wave reductions.
__global__ __launch_bounds__(256) void k_att_pool(const PoolArgs a) {
    extern __shared__ __attribute__((aligned(16))) float att_s[];     // [G][P] + 4 zeros
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int b = blockIdx.y, P = a.P, G = a.G;
    for (int g = wave; g < G; g += 4) {
        float mx = -INFINITY;
        for (int p = lane; p < P; p += 64) {
            float s = a.ba[g];
            for (int ht = 0; ht < a.HT; ++ht) s += a.slab[(((long long)b * a.HT + ht) * G + g) * P + p];     // fixed order
            att_s[g * P + p] = s;
            mx = fmaxf(mx, s);
        }
        mx = wave_max(mx);
        float sum = 0.f;
        for (int p = lane; p < P; p += 64) {
            const float e = expf(att_s[g * P + p] - mx);
            att_s[g * P + p] = e;
            sum += e;
        }
        sum = wave_sum(sum);
        for (int p = lane; p < P; p += 64) {
            const float w = att_s[g * P + p] / sum;
            att_s[g * P + p] = w;
            if (blockIdx.x == 0) a.att[((long long)b * G + g) * P + p] = w;
        }
    }
    if (tid < 4) att_s[G * P + tid] = 0.f;
    __syncthreads();

    const int img = clamp_img(a.img_idx[b], a.n_img);
    const float* map = a.feats + (long long)img * a.dv * P;
    const int c0 = blockIdx.x * a.rows_per_chunk, c1 = min(c0 + a.rows_per_chunk, a.dv);
    for (int cb = c0 + wave * 2; cb < c1; cb += 8) {          // two rows per wave and trip: two loads in flight
        float s[2][ATT_MAX_G];
#pragma unroll
        for (int r = 0; r < 2; ++r)
#pragma unroll
            for (int g = 0; g < ATT_MAX_G; ++g) s[r][g] = 0.f;
        const int cr1 = min(cb + 1, c1 - 1);
        for (int p4 = lane * 4; p4 < P; p4 += 256) {
            const f32x4 v0 = load4(map + cb * P, p4, P);
            const f32x4 v1 = load4(map + cr1 * P, p4, P);
#pragma unroll
            for (int g = 0; g < ATT_MAX_G; ++g) {
                if (g < G) {
                    const float* ap = att_s + g * P + p4;       // rows of the LDS copy are not 16-byte aligned when P % 4 != 0
                    const f32x4 w = {ap[0], ap[1], ap[2], ap[3]};
                    s[0][g] += dot4(v0, w);
                    s[1][g] += dot4(v1, w);
                }
            }
        }
#pragma unroll
        for (int g = 0; g < ATT_MAX_G; ++g) {
            if (g < G) {
                const float r0 = wave_sum(s[0][g]), r1 = wave_sum(s[1][g]);
                if (lane == 0) {
                    a.v_att[((long long)b * G + g) * a.dv + cb] = r0;
                    if (cb + 1 < c1) a.v_att[((long long)b * G + g) * a.dv + cb + 1] = r1;
                }
            }
        }
    }
}

// t = act_c(act_v(x_v + bg) * x_qf), in place over x_v [B, G dh_f]
__global__ __launch_bounds__(256) void k_att_fuse(float* __restrict__ xv, const float* __restrict__ bg, const float* __restrict__ xqf, int n,
                                                  long long total, int act_v, int act_c) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % n);
    xv[i] = att_act(att_act(xv[i] + bg[c], act_v) * xqf[i], act_c);
}

struct AttLayout {
    size_t xq, aslab, v_att, xv, xqf, slab, slab_bytes, total;
    int HT, PT, TM;          // TM: positions per tile of k_att_logits (208 or 64); 0: k_att_logits_small
    GemmPlan plan[4];        // 0 x_q, 1 glimpse Linears (grouped), 2 x_qf, 3 classifier
};

int check_att(const ncx_mlb_att_dims* d, const ncx_mlb_att_params* m) {
    if (!d || !m) return NCX_E_NULL;
    if (d->B < 1 || d->P < 1 || d->n_img < 1 || d->G < 1 || d->G > ATT_MAX_G) return NCX_E_DIMS;
    if (d->dv < 4 || d->dq < 4 || d->dh_att < 4 || d->dh_f < 4 || d->A < 4) return NCX_E_DIMS;
    const long long lim = 1ll << 31, B = d->B, GF = (long long)d->G * d->dh_f;
    if ((long long)d->G * d->P > ATT_MAX_GP) return NCX_E_DIMS;
    if ((long long)d->dv * d->P * 4 >= lim) return NCX_E_DIMS;                       // 32-bit offsets inside one image
    if (GF >= lim / 4 || B * GF >= lim || B * d->G * (long long)d->dv >= lim || B * d->A >= lim || B * d->dh_att >= lim) return NCX_E_DIMS;
    if (B * cdiv(d->dh_att, ATT_BN) * cdiv(d->P, 64) >= lim || B * d->P >= lim) return NCX_E_DIMS;      // grids
    auto act_ok = [](int a) { return a == 0 || a == 2; };
    if (!act_ok(m->act_v_att) || !act_ok(m->act_q_att) || !act_ok(m->act_mm) || !act_ok(m->act_v) || !act_ok(m->act_q) || !act_ok(m->act_c))
        return NCX_E_FLAGS;
    if (!m->wv_att || !m->bv_att || !m->wq_att || !m->bq_att || !m->wa || !m->ba || !m->wg || !m->bg || !m->wqf || !m->bqf || !m->wc || !m->bc)
        return NCX_E_NULL;
    return NCX_OK;
}

// the grouped launch of the G glimpse Linears: problem g reads v_att[:, g] and writes the column slice g of x_v
GemmArgs glimpse_gemm(const ncx_mlb_att_dims& d, const float* v_att, const float* wg, float* xv) {
    GemmArgs a{}; a.mode = MODE_GROUP; a.nseg = d.G; a.M = d.B;
    for (int g = 0; g < d.G; ++g) {
        a.a[g] = x_plain(v_att ? v_att + (long long)g * d.dv : nullptr, (long long)d.G * d.dv, d.B, d.dv);
        a.b[g] = x_plain(wg ? wg + (long long)g * d.dh_f * d.dv : nullptr, d.dv, d.dh_f, d.dv);
        a.klen[g] = d.dv;
        a.out[g] = xv ? xv + (long long)g * d.dh_f : nullptr; a.ldo[g] = (long long)d.G * d.dh_f; a.n_cols[g] = d.dh_f;
    }
    return a;
}
GemmArgs linear_gemm(int M, int N, int K, const float* x, const float* w, float* out, int act) {
    GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = M;
    a.a[0] = x_plain(x, K, M, K); a.b[0] = x_plain(w, K, N, K); a.klen[0] = K;
    a.out[0] = out; a.ldo[0] = N; a.n_cols[0] = N; a.epi.relu = act;
    return a;
}

AttLayout att_layout(const ncx_mlb_att_dims& d) {
    AttLayout w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const int GF = d.G * d.dh_f;
    if (d.P >= 4) {
        w.TM = cdiv(d.P, 208) * 208 < cdiv(d.P, 64) * 64 ? 208 : 64;
        w.HT = (int)cdiv(d.dh_att, ATT_BN); w.PT = (int)cdiv(d.P, w.TM);
    } else {
        w.TM = 0; w.HT = 1; w.PT = 1;
    }
    w.xq = take((size_t)d.B * d.dh_att * 4);
    w.aslab = take((size_t)d.B * w.HT * d.G * d.P * 4);
    w.v_att = take((size_t)d.B * d.G * d.dv * 4);
    w.xv = take((size_t)d.B * GF * 4);
    w.xqf = take((size_t)d.B * GF * 4);
    w.plan[0] = plan_gemm(FORM_NT, d.B, d.dh_att, ksteps(d.dq), true);
    w.plan[1] = plan_gemm(FORM_NT, d.B, d.dh_f, ksteps(d.dv), true);
    w.plan[2] = plan_gemm(FORM_NT, d.B, GF, ksteps(d.dq), true);
    w.plan[3] = plan_gemm(FORM_NT, d.B, d.A, ksteps(GF), true);
    const GemmArgs probe[4] = {linear_gemm(d.B, d.dh_att, d.dq, nullptr, nullptr, nullptr, 0), glimpse_gemm(d, nullptr, nullptr, nullptr),
                               linear_gemm(d.B, GF, d.dq, nullptr, nullptr, nullptr, 0), linear_gemm(d.B, d.A, GF, nullptr, nullptr, nullptr, 0)};
    for (int i = 0; i < 4; ++i) {
        const size_t e = gemm_slab_bytes(probe[i], w.plan[i]);
        if (e > w.slab_bytes) w.slab_bytes = e;
    }
    w.slab = take(w.slab_bytes);
    w.total = off;
    return w;
}

template <int TM>
int launch_att_logits(const AttArgs& a, int B, hipStream_t s) {
    static DevMask attr_set{0};
    NCX_HIP_TRY(set_max_lds_once(attr_set, (const void*)k_att_logits<TM>, AttCfg<TM>::LDS_BYTES));
    hipLaunchKernelGGL((k_att_logits<TM>), dim3((unsigned)((long long)B * a.HT * a.PT)), dim3(256), AttCfg<TM>::LDS_BYTES, s, a);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
}  // namespace

extern "C" {
size_t ncx_mlb_att_workspace_bytes(const ncx_mlb_att_dims* d, const ncx_mlb_att_params* m) {
    if (check_att(d, m) != NCX_OK) return 0;
    return att_layout(*d).total;
}

int ncx_mlb_att_forward(const ncx_mlb_att_dims* dp, const float* feats, const int32_t* img_idx, const float* q_emb,
                        const ncx_mlb_att_params* mp, void* workspace, size_t workspace_bytes,
                        float* logits, float* att, void* stream_) {
    int rc = check_att(dp, mp);
    if (rc != NCX_OK) return rc;
    if (!feats || !img_idx || !q_emb || !workspace || !logits || !att) return NCX_E_NULL;
    const ncx_mlb_att_dims& d = *dp; const ncx_mlb_att_params& m = *mp;
    const AttLayout w = att_layout(d);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    float* xq = (float*)(ws + w.xq); float* aslab = (float*)(ws + w.aslab); float* v_att = (float*)(ws + w.v_att);
    float* xv = (float*)(ws + w.xv); float* xqf = (float*)(ws + w.xqf); float* slab = (float*)(ws + w.slab);
    const int GF = d.G * d.dh_f;
    {   // a. x_q = act(q . Wq_att^T + b)                                               att.py:58-63
        GemmArgs a = linear_gemm(d.B, d.dh_att, d.dq, q_emb, m.wq_att, xq, m.act_q_att);
        rc = run_gemm_planned(a, FORM_NT, w.plan[0], slab, w.slab_bytes, m.bq_att, s); if (rc) return rc;
    }
    {   // b. partial position logits of every dh_att tile                              att.py:46-57,71-90
        AttArgs a{};
        a.feats = feats; a.img_idx = img_idx; a.wv = m.wv_att; a.bv = m.bv_att; a.xq = xq; a.wa = m.wa; a.slab = aslab;
        a.P = d.P; a.dv = d.dv; a.dh = d.dh_att; a.G = d.G; a.n_img = d.n_img; a.HT = w.HT; a.PT = w.PT;
        a.act_v = m.act_v_att; a.act_mm = m.act_mm;
        if (w.TM == 208) rc = launch_att_logits<208>(a, d.B, s);
        else if (w.TM == 64) rc = launch_att_logits<64>(a, d.B, s);
        else {
            hipLaunchKernelGGL(k_att_logits_small, dim3((unsigned)((long long)d.B * d.P)), dim3(256), 0, s, a);
            rc = (int)hipGetLastError();
        }
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
        GemmArgs q = linear_gemm(d.B, GF, d.dq, q_emb, m.wqf, xqf, m.act_q);
        rc = run_gemm_planned(q, FORM_NT, w.plan[2], slab, w.slab_bytes, m.bqf, s); if (rc) return rc;
        const long long total = (long long)d.B * GF;
        hipLaunchKernelGGL(k_att_fuse, dim3((unsigned)cdiv(total, 256)), dim3(256), 0, s, xv, m.bg, xqf, GF, total, m.act_v, m.act_c);
        NCX_HIP_TRY(hipGetLastError());
    }
    {   // e. logits = t . Wc^T + bc                                                     att.py:149-153
        GemmArgs a = linear_gemm(d.B, d.A, GF, xv, m.wc, logits, 0);
        rc = run_gemm_planned(a, FORM_NT, w.plan[3], slab, w.slab_bytes, m.bc, s); if (rc) return rc;
    }
    return NCX_OK;
}
}  // extern "C"
