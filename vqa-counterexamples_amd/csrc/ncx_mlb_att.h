// ncx_mlb_att.h -- the kernels and host helpers that the eval-mode forward (ncx_mlb_att.hip) and the training step
// (ncx_mlb_att_train.hip) of the MLB attention model share.  Included by those two translation units only.
#pragma once
#include "ncx_train.h"
#include "ncx_wave.h"
#include "ncx_x6.h"

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

// What the training form of the logits kernels adds: the stash of Xv = act_v_att(conv_v_att(.)) [B, P, dh_att], layer 3's dropout on
// x_att before the contraction, and the map read from the dropped copy Vd [B, dv, P] with the identity index (identity != 0).
struct AttTrain { float* xv_stash; const float* mask3; TrainDrop drop; int identity; };

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

// The epilogue the logits kernels share: the x_att tile -> LDS, then the contraction with conv_att.weight over the tile's hidden
// columns in groups of 64; group c of the tile goes to slab slot ht0 + c.  BN: hidden columns per workgroup; T: threads; GUARD: the
// waves' block rows run past TM (the X6 form's 224-row wave grid over a 208-row tile).  The operand tiles in `smem` are dead: the
// main loop ended on a barrier.
template <int TM, int BN, int T, bool TRAIN, bool GUARD, int WM, int WN>
__device__ __forceinline__ void att_epilogue(float* const smem, const f32x4 (&acc)[WM][WN], const AttArgs& a, const AttTrain& tr, const int b,
                                             const int p0, const int h0, const int ht0, const int wm0, const int wn0, const int tid) {
    constexpr int XP = BN + 1, NG = BN / ATT_BN;    // odd pitch: threads of the contraction walk p, no conflicts
    const int lane = tid & 63, li = lane & 15, lk = lane >> 4;
    float* const xs = smem;                         // [TM][XP]
    float* const was = smem + TM * XP;              // [G][BN]
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
                if (!GUARD || pl < TM) xs[pl * XP + hl] = h < a.dh ? v : 0.f;
            }
    }
    if constexpr (TRAIN) {
        // the Xv tile goes to the stash from LDS, BN consecutive hidden units per store row; the same thread then turns its
        // element into drop_mm(act_mm(Xv * x_q)) in place (thread t owns column t % BN of rows t / BN, + T / BN, ...)
        __syncthreads();
        const int hl = tid % BN, h = h0 + hl;
        if (h < a.dh) {
            const float xq = a.xq[(long long)b * a.dh + h], sc = train_scale(tr.drop, 3);
            float* const st = tr.xv_stash + (long long)b * a.P * a.dh;
            for (int pl = tid / BN; pl < TM && p0 + pl < a.P; pl += T / BN) {
                const int e = (p0 + pl) * a.dh + h;
                const float xv = xs[pl * XP + hl];
                st[e] = xv;
                const float v = att_act(xv * xq, a.act_mm);
                xs[pl * XP + hl] = train_keep(tr.drop, 3, tr.mask3, (long long)b * a.P * a.dh + e) ? v * sc : 0.f;      // index over [B, P, dh_att]
            }
        }
    }
    for (int i = tid; i < a.G * BN; i += T) {
        const int g = i / BN, hl = i - g * BN;
        was[i] = h0 + hl < a.dh ? a.wa[(long long)g * a.dh + h0 + hl] : 0.f;
    }
    __syncthreads();
    for (int i = tid; i < a.G * NG * TM; i += T) {
        const int gc = i / TM, pl = i - gc * TM, g = gc / NG, c = gc - g * NG, p = p0 + pl;
        if (p >= a.P || ht0 + c >= a.HT) continue;
        float s = 0.f;
#pragma unroll 16
        for (int hl = 0; hl < ATT_BN; ++hl) s = __builtin_fmaf(xs[pl * XP + c * ATT_BN + hl], was[g * BN + c * ATT_BN + hl], s);
        a.slab[(((long long)b * a.HT + ht0 + c) * a.G + g) * a.P + p] = s;
    }
}

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

    att_epilogue<TM, ATT_BN, 256, TRAIN, false>(smem, acc, a, tr, b, p0, h0, ht, wm0, wn0, tid);
}

// ---- the same product on the bf16 matrix path with fp32-grade operands (NCX_F_X6; not the default) ----------------------------------
// As k_dw_tn8_x6 and the X6 form of k_main_fwd: the operands are cut into three bf16 planes when the tile is stored to LDS and six plane
// products per 16 x 16 x 32 block run with fp32 accumulation -- the cut, the order of the products, what is dropped and what is outside
// the contract (a non-finite map or weight value): ncx_x6.h.
// One workgroup: 8 waves, TM positions of one image x 128 hidden columns (two slab slots), one 32-channel step = one MFMA depth.
// The waves form a 2 x 4 grid: 7 (TM = 208: a 224-row grid, the last 16 rows are loader padding and are dropped) or 2 block rows x 2
// column blocks each, so a map fragment is read by 4 waves and serves 12 MFMAs.  LDS, double-buffered: three planes of the map tile in
// the global layout [32 channels][positions] (fragments through ds_read_b64_tr_b16; the row pitch, positions * 2 + 32 bytes, puts 8
// consecutive channel rows on distinct 32-byte bank groups) and three planes of the weight tile [128 hidden][32 channels] at 80 bytes
// per row (plain 16-byte reads).  A transposed read hands lane group lk the channels 4 lk .. 4 lk + 3 and 16 + 4 lk .. 16 + 4 lk + 3,
// so the weight rows are stored in that order: channel quad q < 4 at byte 16 q, quad q >= 4 at byte 16 (q - 4) + 8.
// Loop: one barrier per step; the global loads run a whole step ahead of their cut in a second register set (measured against one
// set, B = 128, G = 4: 1.199 -> 1.086 ms per forward); the schedule inside a step is the compiler's.  Compiler report (gfx950): 208-row
// form 199 VGPRs, 153 600 bytes of LDS, 2 waves per SIMD; 64-row form 111 VGPRs, 92 160 bytes, 4 waves per SIMD by registers; by LDS
// both run one workgroup per CU, i.e. 2 resident waves per SIMD; no scratch, for both values of TRAIN.  The epilogue, the slab layout and the order k_att_pool sums it in are those of the fp32 kernel.
constexpr int ATT6_BN = 128, ATT6_T = 512, ATT6_PB = 80;

template <int TM> struct AttCfg6 {
    static constexpr int LOAD_M = (TM + 31) / 32 * 32;
    static constexpr int PA = LOAD_M * 2 + 32;                                 // bytes per channel row of one map plane: 480 / 160
    static constexpr int A_PL = GEMM_BK * PA, PL = A_PL + ATT6_BN * ATT6_PB, BUF = 3 * PL;      // one plane (map rows | weight rows), one buffer
    static constexpr int QR = LOAD_M / 4, QA = QR * GEMM_BK;                   // 16-byte items per channel row, per map tile
    static constexpr int NA = (QA + ATT6_T - 1) / ATT6_T, NB = ATT6_BN * 8 / ATT6_T;      // items per thread: 4 (the last one half used) / 1; 2
    static constexpr int EPI_BYTES = (TM * (ATT6_BN + 1) + ATT_MAX_G * ATT6_BN) * 4;
    static constexpr int LDS_BYTES = 2 * BUF > EPI_BYTES ? 2 * BUF : EPI_BYTES;
    static constexpr int WM = LOAD_M / 32, WN = 2;                             // 16 x 16 blocks per wave
    static_assert(PA % 64 == 32 && (PA / 32) % 2 == 1, "map pitch: an odd number of 32-byte bank groups");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

template <int TM, bool TRAIN>
__global__ __launch_bounds__(ATT6_T, 1) void k_att_logits_x6(const AttArgs a, const AttTrain tr) {
    typedef AttCfg6<TM> Cfg;
    constexpr int T = ATT6_T, PA = Cfg::PA, PB = ATT6_PB, PL = Cfg::PL, A_PL = Cfg::A_PL, BUF = Cfg::BUF, WM = Cfg::WM, WN = Cfg::WN;
    constexpr int NA = Cfg::NA, NB = Cfg::NB, QR = Cfg::QR, QA = Cfg::QA, BK = GEMM_BK;
    extern __shared__ __attribute__((aligned(16))) float smem[];
    unsigned char* const lds = (unsigned char*)smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int wm0 = (wave >> 2) * (WM * 16), wn0 = (wave & 3) * (WN * 16);
    const int HT6 = (a.HT + 1) / 2;
    int id = blockIdx.x;
    const int pt = id % a.PT; id /= a.PT;
    const int ht6 = id % HT6;
    const int b = id / HT6;
    const int p0 = pt * TM, h0 = ht6 * ATT6_BN;
    int img;
    if constexpr (TRAIN) img = tr.identity ? b : clamp_img(a.img_idx[b], a.n_img);
    else img = clamp_img(a.img_idx[b], a.n_img);
    const float* const map = a.feats + (long long)img * a.dv * a.P;      // 64-bit image base; 32-bit offsets inside the image
    const int P = a.P, dv = a.dv;

    // ---- loader: map item e = tid + T i -> channel row e / QR, positions p0 + 4 (e % QR) ..; weight item i -> hidden row (tid >> 3) + 64 i,
    // channel quad tid & 7.  16-byte windows slid left to stay inside the row and repaired at store time (load_window / fix_window).
    int arow[NA], acol[NA], adst[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int e = min(tid + T * i, QA - 1);            // (items beyond the tile re-load its last one; never stored)
        arow[i] = e / QR; acol[i] = p0 + 4 * (e % QR);
        adst[i] = arow[i] * PA + (e % QR) * 8;
    }
    const int bq = tid & 7;
    const float* brp[NB];
    bool bok[NB];
    int bdst[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int r = (tid >> 3) + 64 * i, h = h0 + r;
        bok[i] = h < a.dh;
        brp[i] = a.wv + (long long)min(h, a.dh - 1) * dv;
        bdst[i] = A_PL + r * PB + (bq < 4 ? 16 * bq : 16 * (bq - 4) + 8);
    }
    f32x4 va[2][NA], vb[2][NB];                            // two register sets: the loads run a whole step ahead of their store
    auto issue = [&](auto set_c, int k) __attribute__((always_inline)) {
        constexpr int S = decltype(set_c)::value;
#ifdef NCX_ATT6_ABLATE_LOADS     // timing experiment only: keep the registers of the first tile
        if (k) return;
#endif
        if (k + BK <= dv) {                                // whole 32-channel steps: straight-line
#pragma unroll
            for (int i = 0; i < NA; ++i) va[S][i] = load_window(map + (k + arow[i]) * P, acol[i], P);
#pragma unroll
            for (int i = 0; i < NB; ++i) vb[S][i] = *(const f32x4u*)(brp[i] + k + 4 * bq);
        } else {                                           // the ragged last step: channel rows clamped, channel windows slid
#pragma unroll
            for (int i = 0; i < NA; ++i) va[S][i] = load_window(map + min(k + arow[i], dv - 1) * P, acol[i], P);
#pragma unroll
            for (int i = 0; i < NB; ++i) vb[S][i] = load_window(brp[i], k + 4 * bq, dv);
        }
    };
    // part s < NA: map item s; part NA + i: weight item i.  Positions beyond P, channels beyond dv and hidden rows beyond dh_att are zero.
    auto store = [&](auto set_c, int k, int buf, int s0, int s1) __attribute__((always_inline)) {
        constexpr int S = decltype(set_c)::value;
#ifdef NCX_ATT6_ABLATE_STORES    // timing experiment only: no cut, no ds_write after the first tile
        if (k) return;
#endif
        unsigned char* const base = lds + buf * BUF;
        const bool ragged = k + BK > dv;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (i < s0 || i >= s1) continue;
            if (NA * T != QA && tid + T * i >= QA) continue;
            f32x4 v = fix_window(va[S][i], acol[i], P);
            if (ragged && k + arow[i] >= dv) v = zero;
            x6_split_store(v, base + adst[i], PL);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (NA + i < s0 || NA + i >= s1) continue;
            f32x4 v = vb[S][i];
            if (ragged) v = fix_window(v, k + 4 * bq, dv);
            if (!bok[i]) v = zero;
            x6_split_store(v, base + bdst[i], PL);
        }
    };

    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    const int tq = li >> 2, tp = li & 3;
    const int fragA = (4 * lk + tq) * PA + (wm0 + 4 * tp) * 2, fragB = A_PL + (wn0 + li) * PB + 16 * lk;
    constexpr int NP = NA + NB;                        // parts of the next tile's store, spread over the block rows of this step
    typedef std::integral_constant<int, 0> S0; typedef std::integral_constant<int, 1> S1;
    // tile t (channels 32 t ..) lives in register set t & 1 and LDS buffer t & 1.  Step t: the loads of tile t + 2 are issued into the
    // set tile t left (stored during step t - 1), tile t is multiplied, and tile t + 1, loaded a whole step ago, is cut and stored
    // to the other buffer part by part under the MFMAs of the later block rows.  One barrier per step.
    auto step = [&](auto par_c, int k) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_c)::value;
        typedef std::integral_constant<int, PAR ^ 1> SN;
        const bool has_next = k + BK < dv;
        if (k + 2 * BK < dv) issue(par_c, k + 2 * BK);
        const unsigned char* const base = lds + PAR * BUF;
        x6_bf16x8 bf[WN][3];
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int p = 0; p < 3; ++p) bf[j][p] = *(const x6_bf16x8*)(base + p * PL + fragB + j * 16 * PB);
#pragma unroll
        for (int i = 0; i < WM; ++i) {
            x6_bf16x8 af[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) af[p] = x6_frag_tr(base + p * PL + fragA + i * 32, PA);
            // the 12 MFMAs of block row i: the two column blocks alternate (a dependent MFMA is two issues away); small terms first
#ifdef NCX_ATT6_ABLATE_MFMA      // timing experiment only: one product of the six (every fragment read stays live)
#pragma unroll
            for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0], bf[j][0], acc[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < WN; ++j) asm volatile("" :: "v"(af[1]), "v"(af[2]), "v"(bf[j][1]), "v"(bf[j][2]));
#else
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[X6_A[c]], bf[j][X6_B[c]], acc[i][j], 0, 0, 0);
#endif
            if (has_next) store(SN{}, k + BK, PAR ^ 1, i * NP / WM, (i + 1) * NP / WM);
        }
        __syncthreads();
    };
    issue(S0{}, 0);
    if (BK < dv) issue(S1{}, BK);
    store(S0{}, 0, 0, 0, NP);
    __syncthreads();
    for (int k = 0; k < dv; k += 2 * BK) {
        step(S0{}, k);
        if (k + BK < dv) step(S1{}, k + BK);
    }
    att_epilogue<TM, ATT6_BN, T, TRAIN, (WM * 32 > TM)>(smem, acc, a, tr, b, p0, h0, 2 * ht6, wm0, wn0, tid);
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
        if constexpr (TRAIN) x = train_keep(tr.drop, 3, tr.mask3, e) ? x * train_scale(tr.drop, 3) : 0.f;
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

// the part of check_att that reads the dims alone (ncx_mlb_att_logits_form has no params)
int check_att_dims(const ncx_mlb_att_dims* d) {
    if (!d) return NCX_E_NULL;
    if (d->B < 1 || d->P < 1 || d->n_img < 1 || d->G < 1 || d->G > ATT_MAX_G) return NCX_E_DIMS;
    if (d->dv < 4 || d->dq < 4 || d->dh_att < 4 || d->dh_f < 4 || d->A < 4) return NCX_E_DIMS;
    const long long lim = 1ll << 31, B = d->B, GF = (long long)d->G * d->dh_f;
    if ((long long)d->G * d->P > ATT_MAX_GP) return NCX_E_DIMS;
    if ((long long)d->dv * d->P * 4 >= lim) return NCX_E_DIMS;                       // 32-bit offsets inside one image
    if (GF >= lim / 4 || B * GF >= lim || B * d->G * (long long)d->dv >= lim || B * d->A >= lim || B * d->dh_att >= lim) return NCX_E_DIMS;
    if (B * cdiv(d->dh_att, ATT_BN) * cdiv(d->P, 64) >= lim || B * d->P >= lim) return NCX_E_DIMS;      // grids
    return NCX_OK;
}
int check_att(const ncx_mlb_att_dims* d, const ncx_mlb_att_params* m) {
    if (!d || !m) return NCX_E_NULL;
    const int rc = check_att_dims(d);
    if (rc != NCX_OK) return rc;
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

template <int TM, bool TRAIN>
int launch_att_logits(const AttArgs& a, const AttTrain& tr, int B, hipStream_t s) {
    static DevMask attr_set{0};
    NCX_HIP_TRY(set_max_lds_once(attr_set, (const void*)k_att_logits<TM, TRAIN>, AttCfg<TM>::LDS_BYTES));
    hipLaunchKernelGGL((k_att_logits<TM, TRAIN>), dim3((unsigned)((long long)B * a.HT * a.PT)), dim3(256), AttCfg<TM>::LDS_BYTES, s, a, tr);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
template <int TM, bool TRAIN>
int launch_att_logits_x6(const AttArgs& a, const AttTrain& tr, int B, hipStream_t s) {
    static DevMask attr_set{0};
    NCX_HIP_TRY(set_max_lds_once(attr_set, (const void*)k_att_logits_x6<TM, TRAIN>, AttCfg6<TM>::LDS_BYTES));
    hipLaunchKernelGGL((k_att_logits_x6<TM, TRAIN>), dim3((unsigned)((long long)B * ((a.HT + 1) / 2) * a.PT)), dim3(ATT6_T), AttCfg6<TM>::LDS_BYTES, s, a, tr);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

// positions per tile of the logits stage: 208 when that pads P less than 64-row tiles do, else 64; 0: k_att_logits_small (P < 4)
inline int att_tile_rows(int P) { return P < 4 ? 0 : cdiv(P, 208) * 208 < cdiv(P, 64) * 64 ? 208 : 64; }
// the flags of the ..._flags entry points: 0 or NCX_F_X6
inline bool att_flags_ok(uint32_t flags) { return flags == 0 || flags == NCX_F_X6; }
// which kernel the logits stage takes (ncx_mlb_att_logits_form): 0 small, 1 / 2 fp32 64- / 208-row, 3 / 4 X6 64- / 208-row
inline int att_logits_form(int P, uint32_t flags) {
    const int tm = att_tile_rows(P);
    return tm == 0 ? 0 : (tm == 208 ? 2 : 1) + ((flags & NCX_F_X6) ? 2 : 0);
}
// the logits stage of both forwards
template <bool TRAIN>
int run_att_logits(const AttArgs& a, const AttTrain& tr, int B, uint32_t flags, hipStream_t s) {
    switch (att_logits_form(a.P, flags)) {
    case 4: return launch_att_logits_x6<208, TRAIN>(a, tr, B, s);
    case 3: return launch_att_logits_x6<64, TRAIN>(a, tr, B, s);
    case 2: return launch_att_logits<208, TRAIN>(a, tr, B, s);
    case 1: return launch_att_logits<64, TRAIN>(a, tr, B, s);
    default:
        hipLaunchKernelGGL(k_att_logits_small<TRAIN>, dim3((unsigned)((long long)B * a.P)), dim3(256), 0, s, a, tr);
        return (int)hipGetLastError();
    }
}
}  // namespace
