// ncx_mlb_att.h -- the kernels and host helpers that the eval-mode forward (ncx_mlb_att.hip) and the training step
// (ncx_mlb_att_train.hip) of the MLB attention model share.  Included by those two translation units only.
#pragma once
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

// The six dropouts of the training step (ncx_mlb_att_train.hip): layer ids 1 .. 6 of the counter-based generator, p[layer - 1].
struct AttDrop { int mode; float p[6]; unsigned lo, hi; };
__device__ __forceinline__ bool att_keep(const AttDrop& k, int layer, const float* mask, long long i) {
    if (k.mode == 1) return k.p[layer - 1] > 0.f ? dropout_keep(k.lo, k.hi, (unsigned)layer, (unsigned long long)i, k.p[layer - 1]) : true;
    if (k.mode == 2) return mask[i] != 0.f;
    return true;
}
__device__ __forceinline__ float att_scale(const AttDrop& k, int layer) { return k.mode ? 1.f / (1.f - k.p[layer - 1]) : 1.f; }
// What the training form of the logits kernels adds: the stash of Xv = act_v_att(conv_v_att(.)) [B, P, dh_att], layer 3's dropout on
// x_att before the contraction, and the map read from the dropped copy Vd [B, dv, P] with the identity index (identity != 0).
struct AttTrain { float* xv_stash; const float* mask3; AttDrop drop; int identity; };

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
template <int TM, bool TRAIN>
__global__ __launch_bounds__(256, 2) void k_att_logits(const AttArgs a, const AttTrain tr) {
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
    int img;
    if constexpr (TRAIN) img = tr.identity ? b : clamp_img(a.img_idx[b], a.n_img);
    else img = clamp_img(a.img_idx[b], a.n_img);

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
                float v = att_act(acc[i][j][q] + bias, a.act_v);
                if constexpr (!TRAIN) v = att_act(v * xq, a.act_mm);          // training: the tile holds Xv first (below)
                xs[pl * ATT_XP + hl] = h < a.dh ? v : 0.f;
            }
    }
    if constexpr (TRAIN) {
        // the Xv tile goes to the stash from LDS, 64 consecutive hidden units per wave store; the same thread then turns its
        // element into drop_mm(act_mm(Xv * x_q)) in place (thread t owns column t & 63 of rows t >> 6, + 4, ...)
        __syncthreads();
        const int hl = tid & 63, h = h0 + hl;
        if (h < a.dh) {
            const float xq = a.xq[(long long)b * a.dh + h], sc = att_scale(tr.drop, 3);
            float* const st = tr.xv_stash + (long long)b * a.P * a.dh;
            for (int pl = tid >> 6; pl < TM && p0 + pl < a.P; pl += 4) {
                const int e = (p0 + pl) * a.dh + h;
                const float xv = xs[pl * ATT_XP + hl];
                st[e] = xv;
                const float v = att_act(xv * xq, a.act_mm);
                xs[pl * ATT_XP + hl] = att_keep(tr.drop, 3, tr.mask3, (long long)b * a.P * a.dh + e) ? v * sc : 0.f;      // index over [B, P, dh_att]
            }
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
template <bool TRAIN>
__global__ __launch_bounds__(256) void k_att_logits_small(const AttArgs a, const AttTrain tr) {
    __shared__ float red[ATT_MAX_G][256];
    const int tid = threadIdx.x;
    const int p = blockIdx.x % a.P, b = blockIdx.x / a.P;
    int img;
    if constexpr (TRAIN) img = tr.identity ? b : clamp_img(a.img_idx[b], a.n_img);
    else img = clamp_img(a.img_idx[b], a.n_img);
    const float* v = a.feats + (long long)img * a.dv * a.P + p;
    float t[ATT_MAX_G];
#pragma unroll
    for (int g = 0; g < ATT_MAX_G; ++g) t[g] = 0.f;
    for (int h = tid; h < a.dh; h += 256) {
        const float* w = a.wv + (long long)h * a.dv;
        float s = 0.f;
        for (int c = 0; c < a.dv; ++c) s = __builtin_fmaf(v[c * a.P], w[c], s);
        float x = att_act(s + a.bv[h], a.act_v);
        const long long e = ((long long)b * a.P + p) * a.dh + h;
        if constexpr (TRAIN) tr.xv_stash[e] = x;
        x = att_act(x * a.xq[(long long)b * a.dh + h], a.act_mm);
        if constexpr (TRAIN) x = att_keep(tr.drop, 3, tr.mask3, e) ? x * att_scale(tr.drop, 3) : 0.f;
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

template <int TM, bool TRAIN>
int launch_att_logits(const AttArgs& a, const AttTrain& tr, int B, hipStream_t s) {
    static DevMask attr_set{0};
    NCX_HIP_TRY(set_max_lds_once(attr_set, (const void*)k_att_logits<TM, TRAIN>, AttCfg<TM>::LDS_BYTES));
    hipLaunchKernelGGL((k_att_logits<TM, TRAIN>), dim3((unsigned)((long long)B * a.HT * a.PT)), dim3(256), AttCfg<TM>::LDS_BYTES, s, a, tr);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
}  // namespace
