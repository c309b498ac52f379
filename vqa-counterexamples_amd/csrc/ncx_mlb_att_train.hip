// ncx_mlb_att_train.hip -- the trainable MLB attention model (MLBAtt in training mode) below the question encoder:
// ncx_mlb_att_train_workspace_bytes, _forward[_flags], _backward[_flags], _ws_region, ncx_mlb_att_dwv_form.  Reference: vqa/models/att.py:39-163 with F.dropout active;
// the kernels of the eval-mode forward are shared through ncx_mlb_att.h; the dropout front end (TrainDrop), the GEMM request builders, the
// runner and the element-wise kernels drop_flat, dfuse and dact (k_train_* of ncx_train.hip) are the ones all three VQA trainers use
// (ncx_train.h).  DESIGN 5r, 5y.
//
// Dropout layers (generator layer id, element index = linear index in the tensor): 1 the map fed to conv_v_att [B, dv, P] (the pooled
// map is not dropped), 2 q fed to linear_q_att [B, dq], 3 x_att [B, P, dh_att], 4 v_att [B, G, dv], 5 q fed to linear_q_fusion
// [B, dq], 6 t [B, G dh_f].  Mode 2 reads the six keep masks concatenated in that order.
//
// Forward:
//   k_at_dropmap        Vd = drop1(feats[img_idx]) [B, dv, P]  (only when layer 1 is on; else the table is read in place)
//   drop_flat x 2       q2 = drop2(q), q5 = drop5(q)           (only when on)
//   NT                  x_q = act(q2 Wq_att^T + b)
//   k_att_logits<TRAIN> the eval kernel + the Xv stash [B, P, dh_att] written from the LDS tile + drop3 before the contraction
//   k_att_pool          softmax, pooling of the UNDROPPED map -> att, v_att
//   drop_flat           v4 = drop4(v_att)                       (only when on)
//   NT group, NT        the glimpse Linears (pre-activation), x_qf
//   k_att_fuse_train    x_v = act_v(. + bg) in place; t = act_c(x_v x_qf); tc = drop6(t)
//   NT                  logits = tc Wc^T + bc
// Backward from dlogits:
//   TN, NN + drop6      dWc = dlogits^T tc;  dt = (dlogits Wc) m6
//   dfuse               dz = dt (1 - t^2); dpv = dz x_qf (1 - x_v^2); dpqf = dz x_v (1 - x_qf^2)
//   TN group, TN        dWg[g] = dpv[:, g]^T v4[:, g];  dWqf = dpqf^T q5
//   NN x G              dv_att[:, g] = dpv[:, g] Wg[g];  drop_flat applies m4 (its index runs over [B, G, dv])
//   k_at_datt           partial[b][chunk][g][p] = sum over the chunk's channels of dv_att[b, g, c] V[b, c, p]   (undropped map)
//   k_at_ds             datt = sum of the chunks in order; ds = att (datt - sum_p att datt); per-question partial of dba
//   k_at_head           a workgroup owns (b, 64 hidden units) and walks p over the stash: recomputes a = act_mm(Xv x_q) and m3, da =
//                       (sum_g ds Wa) m3, du = da (1 - a^2); accumulates dxq[b, h] and per-question partials of dWa and dbv_att; overwrites
//                       the stash with dXv = du x_q (1 - Xv^2)
//   k_att_dwv           dWv_att[h, c] = sum_{b, p} dXv[b, p, h] Vd[b, c, p]: fp32 MFMA, A = the stash (row-is-k), B = the map (col-is-k),
//                       the two loaders of k_att_logits swapped; the reduction is split over S groups of images into a slab
//                       (NCX_F_X6 on the backward: k_att_dwv_x6, the same product and slab on the bf16 matrix path with three-plane
//                       operands; a non-finite map or dXv value is outside that contract)
//   k_at_sumrows        fixed-order sums over b / S: dWv_att, dWa, dbv_att, dba, and the bias gradients of the tail
//   dact, TN            dpq = dxq (1 - x_q^2);  dWq_att = dpq^T q2
//   NN + drop2, NN + drop5, k_at_add      dq_emb, on request
// No atomics; every reduction in a fixed order; tanh only in epilogues and element-wise kernels.
#include "ncx_mlb_att.h"

namespace {
enum AtGemm : int { AT_XQ = 0, AT_GLIMPSE, AT_XQF, AT_LOGITS, AT_DWC, AT_DT, AT_DWG, AT_DWQF, AT_DVATT, AT_DWQ, AT_DQ1, AT_DQ2, AT_COUNT };
constexpr int DATT_ROWS = 64;         // channels per chunk of k_at_datt
constexpr int DWV_TH = 64, DWV_TC = 128;   // k_att_dwv: 64 hidden x 128 channel tiles
constexpr int DWV_MAX_S = 8;

// ---- element-wise kernels ----------------------------------------------------------------------------------------------------
// Vd[b, c, p] = drop1(feats[clamp(img_idx[b]), c, p]); per = dv P elements per image
__global__ __launch_bounds__(256) void k_at_dropmap(const float* __restrict__ feats, const int* __restrict__ img_idx, int n_img, long long per,
                                                    long long total, TrainDrop k, const float* __restrict__ mask, float* __restrict__ vd) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= total) return;
    const long long b = i / per, r = i - b * per;
    const int img = clamp_img(img_idx[b], n_img);
    const float v = feats[(long long)img * per + r];
    vd[i] = train_keep(k, 1, mask, i) ? v * train_scale(k, 1) : 0.f;
}
// x_v = act_v(xv + bg) (in place), t = act_c(x_v x_qf), tc = drop6(t); n = G dh_f columns
__global__ __launch_bounds__(256) void k_att_fuse_train(float* __restrict__ xv, const float* __restrict__ bg, const float* __restrict__ xqf, int n,
                                                        long long total, int act_v, int act_c, TrainDrop k, const float* __restrict__ mask6,
                                                        float* __restrict__ t, float* __restrict__ tc) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= total) return;
    const int c = (int)(i % n);
    const float x = att_act(xv[i] + bg[c], act_v);
    const float tt = att_act(x * xqf[i], act_c);
    xv[i] = x; t[i] = tt;
    tc[i] = train_keep(k, 6, mask6, i) ? tt * train_scale(k, 6) : 0.f;
}
__global__ __launch_bounds__(256) void k_at_add(float* __restrict__ d, const float* __restrict__ x, long long n) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i < n) d[i] += x[i];
}
// out[i] = sum over r < R of in[r n + i], r ascending
__global__ __launch_bounds__(256) void k_at_sumrows(const float* __restrict__ in, long long n, int R, float* __restrict__ out) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= n) return;
    float s = 0.f;
    for (int r = 0; r < R; ++r) s += in[(long long)r * n + i];
    out[i] = s;
}

// ---- d att: the mirror of k_att_pool ---------------------------------------------------------------------------------------------
struct DattArgs {
    const float* feats; const int* img_idx; const float* dvatt; float* partial;
    int P, dv, G, n_img, chunks;
};
// grid (chunks, B): thread t takes the positions t, t + 256, ...; the chunk's dv_att rows sit in LDS
__global__ __launch_bounds__(256) void k_at_datt(const DattArgs a) {
    __shared__ float dvs[ATT_MAX_G][DATT_ROWS];
    const int tid = threadIdx.x, b = blockIdx.y, ch = blockIdx.x;
    const int c0 = ch * DATT_ROWS, nc = min(DATT_ROWS, a.dv - c0);
    for (int i = tid; i < a.G * DATT_ROWS; i += 256) {
        const int g = i / DATT_ROWS, c = i - g * DATT_ROWS;
        dvs[g][c] = c < nc ? a.dvatt[((long long)b * a.G + g) * a.dv + c0 + c] : 0.f;
    }
    __syncthreads();
    const int img = clamp_img(a.img_idx[b], a.n_img);
    const float* map = a.feats + (long long)img * a.dv * a.P + (long long)c0 * a.P;
    for (int p = tid; p < a.P; p += 256) {
        float acc[ATT_MAX_G];
#pragma unroll
        for (int g = 0; g < ATT_MAX_G; ++g) acc[g] = 0.f;
        for (int c = 0; c < nc; ++c) {
            const float v = map[c * a.P + p];
#pragma unroll
            for (int g = 0; g < ATT_MAX_G; ++g) acc[g] = __builtin_fmaf(dvs[g][c], v, acc[g]);
        }
#pragma unroll
        for (int g = 0; g < ATT_MAX_G; ++g)
            if (g < a.G) a.partial[(((long long)b * a.chunks + ch) * a.G + g) * a.P + p] = acc[g];
    }
}
// grid (G, B).  ds = att (datt - sum_p att datt); dba_p[b, g] = sum_p ds.  Both sums are exact zeros in mathematics and rounding noise
// in fp32 (the softmax is shift-invariant), so the two block sums run in double and in a fixed order.
__global__ __launch_bounds__(256) void k_at_ds(const float* __restrict__ partial, const float* __restrict__ att, int P, int G, int chunks,
                                               float* __restrict__ ds, float* __restrict__ dba_p) {
    __shared__ double red[256], red1[256];
    __shared__ double tot;
    const int tid = threadIdx.x, g = blockIdx.x, b = blockIdx.y;
    const long long row = ((long long)b * G + g) * P;
    double part = 0.0, mass = 0.0;
    for (int p = tid; p < P; p += 256) {
        float s = 0.f;
        for (int ch = 0; ch < chunks; ++ch) s += partial[(((long long)b * chunks + ch) * G + g) * P + p];
        ds[row + p] = s;
        part += (double)att[row + p] * (double)s;
        mass += (double)att[row + p];
    }
    red[tid] = part; red1[tid] = mass;
    __syncthreads();
    // the fp32 map sums to 1 only within rounding: dividing by its own mass keeps sum_p ds = 0 to the last bit of the double sums
    if (tid == 0) { double t = 0.0, m = 0.0; for (int i = 0; i < 256; ++i) { t += red[i]; m += red1[i]; } tot = t / m; }
    __syncthreads();
    const double dot = tot;
    part = 0.0;
    for (int p = tid; p < P; p += 256) {
        const double v = (double)att[row + p] * ((double)ds[row + p] - dot);
        ds[row + p] = (float)v;
        part += v;
    }
    __syncthreads();
    red[tid] = part;
    __syncthreads();
    if (tid == 0) { double t = 0.0; for (int i = 0; i < 256; ++i) t += red[i]; dba_p[(long long)b * G + g] = (float)t; }
}

// ---- the element-wise part of the attention head's backward, over the stash ---------------------------------------------------------
struct HeadArgs {
    float* stash; const float* xq; const float* ds; const float* wa; const float* mask3;
    float* dxq; float* dwa_p; float* dbv_p;
    TrainDrop drop;
    int P, dh, G, act_v, act_mm;
};
// grid (h tiles of 64, B); thread (pq = t >> 6, hl = t & 63) walks p = pq, pq + 4, ...; the four partial sums are added in pq order
__global__ __launch_bounds__(256) void k_at_head(const HeadArgs a) {
    extern __shared__ __attribute__((aligned(16))) float hs[];
    const int G = a.G, P = a.P, RW = G + 2;
    float* const ds_s = hs;                     // [G][P]
    float* const wa_s = hs + G * P;             // [G][64]
    float* const red = wa_s + G * 64;           // [4][64][G + 2]
    const int tid = threadIdx.x, hl = tid & 63, pq = tid >> 6, b = blockIdx.y, h = blockIdx.x * 64 + hl;
    const bool hv = h < a.dh;
    for (int i = tid; i < G * P; i += 256) ds_s[i] = a.ds[(long long)b * G * P + i];
    for (int i = tid; i < G * 64; i += 256) {
        const int g = i >> 6, hh = blockIdx.x * 64 + (i & 63);
        wa_s[i] = hh < a.dh ? a.wa[(long long)g * a.dh + hh] : 0.f;
    }
    __syncthreads();
    float dxq = 0.f, dbv = 0.f, dwa[ATT_MAX_G];
#pragma unroll
    for (int g = 0; g < ATT_MAX_G; ++g) dwa[g] = 0.f;
    if (hv) {
        const long long base = (long long)b * P * a.dh;
        float* const st = a.stash + base;
        const float xq = a.xq[(long long)b * a.dh + h], sc = train_scale(a.drop, 3);
        for (int p = pq; p < P; p += 4) {
            const int e = p * a.dh + h;
            const float x = st[e];
            const float av = att_act(x * xq, a.act_mm);
            const float m = train_keep(a.drop, 3, a.mask3, base + e) ? sc : 0.f;       // index over [B, P, dh_att]
            const float ad = av * m;
            float s = 0.f;
#pragma unroll
            for (int g = 0; g < ATT_MAX_G; ++g)
                if (g < G) {
                    const float d = ds_s[g * P + p];
                    s = __builtin_fmaf(d, wa_s[g * 64 + hl], s);
                    dwa[g] = __builtin_fmaf(d, ad, dwa[g]);
                }
            const float da = s * m;
            const float du = a.act_mm == 2 ? da * (1.f - av * av) : da;
            dxq = __builtin_fmaf(du, x, dxq);
            float dx = du * xq;
            if (a.act_v == 2) dx *= 1.f - x * x;
            dbv += dx;
            st[e] = dx;
        }
    }
    float* const r = red + (pq * 64 + hl) * RW;
    r[0] = dxq; r[1] = dbv;
#pragma unroll
    for (int g = 0; g < ATT_MAX_G; ++g)
        if (g < G) r[2 + g] = dwa[g];
    __syncthreads();
    if (pq == 0 && hv) {
        for (int j = 0; j < RW; ++j) {
            float v = red[hl * RW + j];
            for (int q = 1; q < 4; ++q) v += red[(q * 64 + hl) * RW + j];
            if (j == 0) a.dxq[(long long)b * a.dh + h] = v;
            else if (j == 1) a.dbv_p[(long long)b * a.dh + h] = v;
            else a.dwa_p[((long long)b * G + (j - 2)) * a.dh + h] = v;
        }
    }
}

// ---- d conv_v_att.weight ----------------------------------------------------------------------------------------------------------
struct DwvArgs {
    const float* dxv; const float* map; const int* img_idx; float* slab;
    int P, dv, dh, B, n_img, ipg, HT, CT, identity;
};
// One workgroup: 64 hidden units x 128 channels (2 x 2 waves of 32 x 64: 8 fragment reads feed 16 MFMAs), reduction over the positions of the images [z ipg, (z + 1) ipg) as ONE pipeline of
// 32-deep steps (the loaders are re-pointed at the next image while the last step of the previous one is multiplied).  A ragged last
// step of an image (P = 196: 4 positions) multiplies only the 8-deep sub-steps it occupies.
__global__ __launch_bounds__(256, 2) void k_att_dwv(const DwvArgs a) {
    typedef OpLoader<false, DWV_TH> ALoad;                 // dXv: [32 positions][64 hidden]
    typedef OpLoader<true, DWV_TC> BLoad;                  // the map: [128 channels][32 positions]
    constexpr int PA = ALoad::PITCH, PB = BLoad::PITCH, BK = GEMM_BK, WM = 2, WN = 4;
    __shared__ __attribute__((aligned(16))) float lds_a[2 * ALoad::ELEMS];
    __shared__ __attribute__((aligned(16))) float lds_b[2 * BLoad::ELEMS];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int wm0 = (wave >> 1) * 32, wn0 = (wave & 1) * 64;
    int id = blockIdx.x;
    const int ct = id % a.CT; id /= a.CT;
    const int ht = id % a.HT;
    const int z = id / a.HT;
    const int h0 = ht * DWV_TH, c0 = ct * DWV_TC, P = a.P;
    const int b0 = z * a.ipg, b1 = min(a.B, b0 + a.ipg);
    const int nsteps = (b1 - b0) * ((P + BK - 1) / BK);

    XDesc da{}; da.ld = a.dh; da.kind = X_PLAIN; da.rows = P; da.cols = a.dh; da.idx_stride = 1;
    XDesc db{}; db.ld = P; db.kind = X_PLAIN; db.rows = a.dv; db.cols = P; db.idx_stride = 1;
    ALoad la;
    BLoad lb;
    auto prep = [&](int b) __attribute__((always_inline)) {
        const int img = a.identity ? b : clamp_img(a.img_idx[b], a.n_img);
        da.base = a.dxv + (long long)b * P * a.dh;               // 64-bit bases; 32-bit offsets inside a row-block
        db.base = a.map + (long long)img * a.dv * P;
        la.setup(da, h0, tid);
        lb.setup(db, c0, tid);
    };
    auto issue = [&](int k) __attribute__((always_inline)) {
        if (k + BK <= P) { la.template issue_fast<X_PLAIN, true>(da, k, tid); lb.template issue_fast<X_PLAIN, true>(db, k, tid); }
        else { la.issue(da, k, tid); lb.issue(db, k, tid); }
    };
    auto store = [&](int k, int buf) __attribute__((always_inline)) {
        float* pa = lds_a + buf * ALoad::ELEMS; float* pb = lds_b + buf * BLoad::ELEMS;
        if (k + BK <= P) { la.template store_fast<X_PLAIN, true>(pa, tid); lb.template store_fast<X_PLAIN, true>(pb, tid); }
        else { la.store(pa, k, tid); lb.store(pb, k, tid); }
    };
    f32x4 acc[WM][WN];
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j) acc[i][j] = f32x4{0.f, 0.f, 0.f, 0.f};

    prep(b0);
    issue(0);
    store(0, 0);
    __syncthreads();
    int buf = 0, k = 0, b = b0;
    for (int stp = 0; stp < nsteps; ++stp) {
        int kn = k + BK, bn = b;
        if (kn >= P) { kn = 0; bn = b + 1; }
        const bool has_next = stp + 1 < nsteps;
        if (has_next) {
            if (kn == 0) prep(bn);
            issue(kn);
        }
        const int nsub = (min(BK, P - k) + 7) / 8;              // sub-steps that hold positions of this image
        const float* pa = lds_a + buf * ALoad::ELEMS;
        const float* pb = lds_b + buf * BLoad::ELEMS;
#pragma unroll
        for (int t = 0; t < BK / 8; ++t) {
            if (t < nsub) {
                if (t == nsub - 1 && has_next) store(kn, buf ^ 1);      // drains under the last sub-step's MFMAs
                const int kk = t * 8 + 2 * lk;
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
        }
        __syncthreads();
        buf ^= 1; k = kn; b = bn;
    }
    float* const out = a.slab + (long long)z * a.dh * a.dv;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int h = h0 + wm0 + i * 16 + lk * 4 + q, c = c0 + wn0 + j * 16 + li;
                if (h < a.dh && c < a.dv) out[(long long)h * a.dv + c] = acc[i][j][q];
            }
}
// ---- the same product on the bf16 matrix path with fp32-grade operands (NCX_F_X6; not the default) ----------------------------------
// The cut, the six products and their order are those of ncx_x6.h, and the LDS image is that of k_att_logits_x6 (ncx_mlb_att.h) with
// the roles renamed: the operand whose k runs along rows is dXv [P positions][dh_att] (there the map [dv channels][P]) and goes to LDS in the
// global layout, three planes of [32 positions][DWV6_TH hidden] at a pitch of DWV6_TH * 2 + 32 bytes (8 consecutive position rows on
// 8 distinct 32-byte bank groups), read through ds_read_b64_tr_b16; the operand whose k is contiguous is the map [dv][P] (there the
// weight [dh_att][dv]), three planes of [128 channels][32 positions] at 80 bytes per row, read with plain 16-byte loads.  A transposed
// read hands lane group lk the positions 4 lk .. 4 lk + 3 and 16 + 4 lk .. 16 + 4 lk + 3, so a map row is stored in that order:
// position quad q < 4 at byte 16 q, quad q >= 4 at byte 16 (q - 4) + 8.  Neither fragment is permuted in registers.
// One workgroup: 8 waves in a 2 x 4 grid, DWV6_TH = 160 hidden x 128 channels (5 block rows x 2 column blocks of 16 x 16 per wave),
// all images of group z as ONE pipeline of 32-deep steps like k_att_dwv: tile t lives in register set t & 1 and LDS buffer t & 1;
// step t issues the loads of tile t + 2 (re-pointed at the next image when tile t + 1 was an image's last), multiplies tile t, and
// cuts and stores tile t + 1 part by part under the MFMAs of the later block rows.  One barrier per step.  The ragged last step of
// an image is a full 32-deep step whose rows beyond P are stored as exact zeros (clamped loads, zeroed by select at store time):
// 7 x 32 = 224 against P = 196 is 12.5 % more MFMA work, accepted because the kernel is bound by its loader path, not by the matrix
// cores, and a 16-deep MFMA needs a second fragment layout.  160 hidden units: at dh_att = 1200, dv = 2048 the slab's S = 4 groups
// give 8 x 16 x 4 = 512 workgroups, two whole rounds at one workgroup per CU, and 1280 / 1200 is the smallest padding of any tile
// that fits LDS.  The slab, S, ipg and the order k_at_sumrows adds the groups in are those of k_att_dwv.
constexpr int DWV6_TH = 160, DWV6_TC = 128, DWV6_T = 512, DWV6_PB = 80;
struct DwvCfg6 {
    static constexpr int PA = DWV6_TH * 2 + 32;                                // bytes per position row of one dXv plane
    static constexpr int A_PL = GEMM_BK * PA, PL = A_PL + DWV6_TC * DWV6_PB, BUF = 3 * PL;     // one plane (dXv rows | map rows), one buffer
    static constexpr int QR = DWV6_TH / 4, QA = QR * GEMM_BK;                  // 16-byte items per position row, per dXv tile
    static constexpr int NA = (QA + DWV6_T - 1) / DWV6_T, NB = DWV6_TC * 8 / DWV6_T;      // items per thread: 3 (the last one half used); 2
    static constexpr int LDS_BYTES = 2 * BUF;
    static constexpr int WM = DWV6_TH / 32, WN = 2;                            // 16 x 16 blocks per wave
    static_assert(PA % 64 == 32, "dXv pitch: an odd number of 32-byte bank groups");
    static_assert(DWV6_TH % 32 == 0 && GEMM_BK == 32, "wave grid");
    static_assert(LDS_BYTES <= 160 * 1024, "LDS");
};

__global__ __launch_bounds__(DWV6_T, 1) void k_att_dwv_x6(const DwvArgs a) {
    typedef DwvCfg6 Cfg;
    constexpr int T = DWV6_T, PA = Cfg::PA, PB = DWV6_PB, PL = Cfg::PL, A_PL = Cfg::A_PL, BUF = Cfg::BUF, WM = Cfg::WM, WN = Cfg::WN;
    constexpr int NA = Cfg::NA, NB = Cfg::NB, QR = Cfg::QR, QA = Cfg::QA, BK = GEMM_BK;
    extern __shared__ __attribute__((aligned(16))) float dwv6_smem[];
    unsigned char* const lds = (unsigned char*)dwv6_smem;

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6, li = lane & 15, lk = lane >> 4;
    const int wm0 = (wave >> 2) * (WM * 16), wn0 = (wave & 3) * (WN * 16);
    int id = blockIdx.x;
    const int ct = id % a.CT; id /= a.CT;
    const int ht = id % a.HT;
    const int z = id / a.HT;
    const int h0 = ht * DWV6_TH, c0 = ct * DWV6_TC, P = a.P, dh = a.dh, dv = a.dv;
    const int b0 = z * a.ipg, b1 = min(a.B, b0 + a.ipg);
    const int nsteps = (b1 - b0) * ((P + BK - 1) / BK);

    // ---- loader: dXv item e = tid + T i -> position row e / QR, hidden units h0 + 4 (e % QR) ..; map item i -> channel row
    // (tid >> 3) + 64 i, position quad tid & 7.  16-byte windows slid left to stay inside the row and repaired at store time.
    int arow[NA], acol[NA], adst[NA];
#pragma unroll
    for (int i = 0; i < NA; ++i) {
        const int e = min(tid + T * i, QA - 1);            // (items beyond the tile re-load its last one; never stored)
        arow[i] = e / QR; acol[i] = h0 + 4 * (e % QR);
        adst[i] = arow[i] * PA + (e % QR) * 8;
    }
    const int bq = tid & 7;
    int boff[NB], bdst[NB];
    bool bok[NB];
#pragma unroll
    for (int i = 0; i < NB; ++i) {
        const int r = (tid >> 3) + 64 * i, c = c0 + r;
        bok[i] = c < dv;
        boff[i] = min(c, dv - 1) * P;                      // 32-bit offsets inside one image
        bdst[i] = A_PL + r * PB + (bq < 4 ? 16 * bq : 16 * (bq - 4) + 8);
    }
    f32x4 va[2][NA], vb[2][NB];                            // two register sets: the loads run a whole step ahead of their store
    auto issue = [&](auto set_c, int b, int k) __attribute__((always_inline)) {
        constexpr int S = decltype(set_c)::value;
        const int img = a.identity ? b : clamp_img(a.img_idx[b], a.n_img);
        const float* const xb = a.dxv + (long long)b * P * dh;               // 64-bit bases; 32-bit offsets inside a row-block
        const float* const mb = a.map + (long long)img * dv * P;
        if (k + BK <= P) {                                 // whole 32-position steps: straight-line
#pragma unroll
            for (int i = 0; i < NA; ++i) va[S][i] = load_window(xb + (k + arow[i]) * dh, acol[i], dh);
#pragma unroll
            for (int i = 0; i < NB; ++i) vb[S][i] = *(const f32x4u*)(mb + boff[i] + k + 4 * bq);
        } else {                                           // the ragged last step of an image: position rows clamped, position windows slid
#pragma unroll
            for (int i = 0; i < NA; ++i) va[S][i] = load_window(xb + min(k + arow[i], P - 1) * dh, acol[i], dh);
#pragma unroll
            for (int i = 0; i < NB; ++i) vb[S][i] = load_window(mb + boff[i], k + 4 * bq, P);
        }
    };
    // part s < NA: dXv item s; part NA + i: map item i.  Positions beyond P, hidden units beyond dh_att and channels beyond dv are zero.
    auto store = [&](auto set_c, int k, int buf, int s0, int s1) __attribute__((always_inline)) {
        constexpr int S = decltype(set_c)::value;
        unsigned char* const base = lds + buf * BUF;
        const bool ragged = k + BK > P;
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int i = 0; i < NA; ++i) {
            if (i < s0 || i >= s1) continue;
            if (NA * T != QA && tid + T * i >= QA) continue;
            f32x4 v = fix_window(va[S][i], acol[i], dh);
            if (ragged && k + arow[i] >= P) v = zero;
            x6_split_store(v, base + adst[i], PL);
        }
#pragma unroll
        for (int i = 0; i < NB; ++i) {
            if (NA + i < s0 || NA + i >= s1) continue;
            f32x4 v = vb[S][i];
            if (ragged) v = fix_window(v, k + 4 * bq, P);
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
    int k1 = 0;                                        // first position of tile t + 1
    int b2 = b0, k2 = 0;                               // image and first position of tile t + 2
    auto advance = [&](int& b, int& k) __attribute__((always_inline)) { k += BK; if (k >= P) { k = 0; ++b; } };
    auto step = [&](auto par_c, int t) __attribute__((always_inline)) {
        constexpr int PAR = decltype(par_c)::value;
        typedef std::integral_constant<int, PAR ^ 1> SN;
        const bool has_next = t + 1 < nsteps;
        if (t + 2 < nsteps) { issue(par_c, b2, k2); advance(b2, k2); }
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
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int j = 0; j < WN; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[X6_A[c]], bf[j][X6_B[c]], acc[i][j], 0, 0, 0);
            if (has_next) store(SN{}, k1, PAR ^ 1, i * NP / WM, (i + 1) * NP / WM);
        }
        __syncthreads();
        k1 += BK; if (k1 >= P) k1 = 0;
    };
    issue(S0{}, b2, k2); advance(b2, k2);
    if (nsteps > 1) { issue(S1{}, b2, k2); advance(b2, k2); }
    store(S0{}, 0, 0, 0, NP);
    __syncthreads();
    k1 = BK < P ? BK : 0;
    for (int t = 0; t < nsteps; t += 2) {
        step(S0{}, t);
        if (t + 1 < nsteps) step(S1{}, t + 1);
    }
    float* const out = a.slab + (long long)z * dh * dv;
#pragma unroll
    for (int i = 0; i < WM; ++i)
#pragma unroll
        for (int j = 0; j < WN; ++j)
#pragma unroll
            for (int q = 0; q < 4; ++q) {
                const int h = h0 + wm0 + i * 16 + lk * 4 + q, c = c0 + wn0 + j * 16 + li;
                if (h < dh && c < dv) out[(long long)h * dv + c] = acc[i][j][q];
            }
}
// P < 4 (no 16-byte window fits a row of the map): one thread per (h, c), b then p ascending
__global__ __launch_bounds__(256) void k_att_dwv_small(const DwvArgs a, float* __restrict__ out) {
    const long long i = blockIdx.x * 256ll + threadIdx.x;
    if (i >= (long long)a.dh * a.dv) return;
    const int h = (int)(i / a.dv), c = (int)(i - (long long)h * a.dv);
    float s = 0.f;
    for (int b = 0; b < a.B; ++b) {
        const int img = a.identity ? b : clamp_img(a.img_idx[b], a.n_img);
        const float* x = a.dxv + (long long)b * a.P * a.dh + h;
        const float* v = a.map + ((long long)img * a.dv + c) * a.P;
        for (int p = 0; p < a.P; ++p) s = __builtin_fmaf(x[p * a.dh], v[p], s);
    }
    out[i] = s;
}

// ---- host -------------------------------------------------------------------------------------------------------------------------
struct AtLayout {
    size_t vd, q2, q5, xq, stash, aslab, v_att, v4, xv, xqf, t, tc, dt, dpv, dpqf, dvatt, dattp, ds, dba_p, dxq, dwa_p, dbv_p, dwv, dq2,
           slab, slab_bytes, total;
    size_t vd_bytes, dwv_bytes;
    int HT, PT, TM, chunks, S, ipg;
    long long m_off[6];          // element offsets of the six keep masks
};
struct AtPtrs {
    const float *q2, *q5, *v4, *tc, *dlogits, *dpv, *dpqf, *dxq, *masks;
    float *xq, *xv, *xqf, *logits, *dt, *dvatt, *dq, *dq2;
    ncx_mlb_att_grads g;
};
// the step's six p, in layer order
inline float at_p(const ncx_mlb_att_train& t, int layer) {
    const float p[6] = {t.p_att_v, t.p_att_q, t.p_att_mm, t.p_v, t.p_q, t.p_c};
    return p[layer - 1];
}
inline bool at_on(const ncx_mlb_att_train& t, int layer) { return drop_on(t.dropout_mode, at_p(t, layer)); }
inline TrainDrop at_drop(const ncx_mlb_att_train& t) {
    return train_drop(t.dropout_mode, t.seed, {t.p_att_v, t.p_att_q, t.p_att_mm, t.p_v, t.p_q, t.p_c});
}

// the limits the training step adds to check_att_dims (d has passed it)
int at_check_dims(const ncx_mlb_att_dims* d) {
    const long long lim = 1ll << 31, B = d->B;
    if ((long long)d->P * d->dh_att * 4 >= lim) return NCX_E_DIMS;                    // 32-bit offsets inside one question's stash block
    if ((long long)d->dh_att * d->dv >= lim / 4 || (long long)d->G * d->dh_att >= lim) return NCX_E_DIMS;
    if (B * d->dv * (long long)d->P / 256 >= lim - 1 || B * d->P * (long long)d->dh_att / 256 >= lim - 1) return NCX_E_DIMS;     // grids
    if (B * d->dq >= lim || (long long)d->G * d->dh_f * (long long)(d->dq > d->dv ? d->dq : d->dv) >= lim || (long long)d->A * d->G * d->dh_f >= lim ||
        (long long)d->dh_att * d->dq >= lim) return NCX_E_DIMS;
    if (cdiv(d->dh_att, DWV_TH) * cdiv(d->dv, DWV_TC) * DWV_MAX_S >= lim || d->B > 65535 || cdiv(d->dv, DATT_ROWS) > 65535) return NCX_E_DIMS;
    return NCX_OK;
}
int at_check(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const ncx_mlb_att_params* m, bool need_ptrs) {
    if (!d || !t || !m) return NCX_E_NULL;
    if (need_ptrs) { const int rc = check_att(d, m); if (rc != NCX_OK) return rc; }
    else {
        ncx_mlb_att_params probe = *m;          // sizing reads dims and activation codes only
        const float one = 0.f;
        probe.wv_att = probe.bv_att = probe.wq_att = probe.bq_att = probe.wa = probe.ba = probe.wg = probe.bg = probe.wqf = probe.bqf = probe.wc =
            probe.bc = &one;
        const int rc = check_att(d, &probe); if (rc != NCX_OK) return rc;
    }
    if (t->dropout_mode < 0 || t->dropout_mode > 2) return NCX_E_DIMS;
    if (!probs_ok({t->p_att_v, t->p_att_q, t->p_att_mm, t->p_v, t->p_q, t->p_c})) return NCX_E_DIMS;
    return at_check_dims(d);
}

// The products of the step on the generic engine (pointers may be NULL when only sizing the slab).  AT_DVATT: problem `gi` of G.
GemmReq at_gemm(const ncx_mlb_att_dims& d, const ncx_mlb_att_train& t, const ncx_mlb_att_params& m, const AtLayout& w, const AtPtrs& p, int which,
                int gi) {
    const int B = d.B, GF = d.G * d.dh_f;
    GemmReq r{};
    GemmArgs& a = r.a;
    auto drop = [&](int layer, long long ld) {
        epi_dropout(a.epi, t.dropout_mode, t.seed, at_p(t, layer), (unsigned)layer, ptr_off(p.masks, w.m_off[layer - 1]), ld);
    };
    switch (which) {
    case AT_XQ: req_nt(r, B, d.dh_att, d.dq, p.q2, m.wq_att, p.xq, m.act_q_att, m.bq_att); break;
    case AT_GLIMPSE:
        a = glimpse_gemm(d, p.v4, m.wg, p.xv);
        r.form = FORM_NT; r.pl = plan_gemm(FORM_NT, B, d.dh_f, ksteps(d.dv), true);
        break;
    case AT_XQF: req_nt(r, B, GF, d.dq, p.q5, m.wqf, p.xqf, m.act_q, m.bqf); break;
    case AT_LOGITS: req_nt(r, B, d.A, GF, p.tc, m.wc, p.logits, 0, m.bc); break;
    case AT_DWC: gemm_tn_piece(a, 0, p.dlogits, d.A, d.A, p.tc, GF, GF, p.g.wc, B); req_tn(r, d.A, GF, B); break;
    case AT_DT: req_nn_unsplit(r, B, p.dlogits, d.A, d.A, m.wc, GF, p.dt, GF); drop(6, GF); break;
    case AT_DWG:
        for (int g = 0; g < d.G; ++g)
            gemm_tn_piece(a, g, ptr_off(p.dpv, (long long)g * d.dh_f), GF, d.dh_f, ptr_off(p.v4, (long long)g * d.dv), (long long)d.G * d.dv, d.dv,
                          ptr_off(p.g.wg, (long long)g * d.dh_f * d.dv), B);
        req_tn(r, d.dh_f, (long long)d.G * d.dv, B);
        break;
    case AT_DWQF: gemm_tn_piece(a, 0, p.dpqf, GF, GF, p.q5, d.dq, d.dq, p.g.wqf, B); req_tn(r, GF, d.dq, B); break;
    case AT_DVATT:
        req_nn_unsplit(r, B, ptr_off(p.dpv, (long long)gi * d.dh_f), GF, d.dh_f, ptr_off(m.wg, (long long)gi * d.dh_f * d.dv), d.dv,
                       ptr_off(p.dvatt, (long long)gi * d.dv), (long long)d.G * d.dv);
        break;
    case AT_DWQ: gemm_tn_piece(a, 0, p.dxq, d.dh_att, d.dh_att, p.q2, d.dq, d.dq, p.g.wq_att, B); req_tn(r, d.dh_att, d.dq, B); break;
    case AT_DQ1: req_nn_unsplit(r, B, p.dxq, d.dh_att, d.dh_att, m.wq_att, d.dq, p.dq, d.dq); drop(2, d.dq); break;
    default: req_nn_unsplit(r, B, p.dpqf, GF, GF, m.wqf, d.dq, p.dq2, d.dq); drop(5, d.dq); break;
    }
    return r;
}

AtLayout at_layout(const ncx_mlb_att_dims& d, const ncx_mlb_att_train& t, const ncx_mlb_att_params& m) {
    AtLayout w{};
    WsCarver cv;
    const size_t B = d.B, P = d.P, GF = (size_t)d.G * d.dh_f, G = d.G;
    if (d.P >= 4) {
        w.TM = cdiv(d.P, 208) * 208 < cdiv(d.P, 64) * 64 ? 208 : 64;
        w.HT = (int)cdiv(d.dh_att, ATT_BN); w.PT = (int)cdiv(d.P, w.TM);
    } else {
        w.TM = 0; w.HT = 1; w.PT = 1;
    }
    w.chunks = (int)cdiv(d.dv, DATT_ROWS);
    // groups of images of the dWv_att reduction: enough workgroups for every CU four times over, at most DWV_MAX_S partial copies
    const long long tiles = cdiv(d.dh_att, DWV_TH) * cdiv(d.dv, DWV_TC);
    long long S = cdiv(4ll * 256, tiles);
    if (S > DWV_MAX_S) S = DWV_MAX_S;
    if (S > d.B) S = d.B;
    w.ipg = (int)cdiv(d.B, S);
    w.S = (int)cdiv(d.B, w.ipg);
    long long mo = 0;
    const long long msz[6] = {(long long)(B * d.dv * P), (long long)(B * d.dq), (long long)(B * P * d.dh_att), (long long)(B * G * d.dv),
                              (long long)(B * d.dq), (long long)(B * GF)};
    for (int i = 0; i < 6; ++i) { w.m_off[i] = mo; mo += msz[i]; }
    w.vd_bytes = at_on(t, 1) ? B * d.dv * P * 4 : 0;
    w.vd = cv.take(w.vd_bytes);
    w.q2 = cv.take(at_on(t, 2) ? B * d.dq * 4 : 0);
    w.q5 = cv.take(at_on(t, 5) ? B * d.dq * 4 : 0);
    w.xq = cv.take(B * d.dh_att * 4);
    w.stash = cv.take(B * P * d.dh_att * 4);
    w.aslab = cv.take(B * w.HT * G * P * 4);
    w.v_att = cv.take(B * G * d.dv * 4);
    w.v4 = cv.take(at_on(t, 4) ? B * G * d.dv * 4 : 0);
    w.xv = cv.take(B * GF * 4); w.xqf = cv.take(B * GF * 4); w.t = cv.take(B * GF * 4); w.tc = cv.take(B * GF * 4);
    w.dt = cv.take(B * GF * 4); w.dpv = cv.take(B * GF * 4); w.dpqf = cv.take(B * GF * 4);
    w.dvatt = cv.take(B * G * d.dv * 4);
    w.dattp = cv.take(B * w.chunks * G * P * 4);
    w.ds = cv.take(B * G * P * 4);
    w.dba_p = cv.take(B * G * 4);
    w.dxq = cv.take(B * d.dh_att * 4);
    w.dwa_p = cv.take(B * G * d.dh_att * 4);
    w.dbv_p = cv.take(B * d.dh_att * 4);
    w.dwv_bytes = d.P >= 4 ? (size_t)w.S * d.dh_att * d.dv * 4 : 0;
    w.dwv = cv.take(w.dwv_bytes);
    w.dq2 = cv.take(B * d.dq * 4);
    const AtPtrs p{};
    w.slab_bytes = max_slab_bytes<AT_COUNT>([&](int which) { return at_gemm(d, t, m, w, p, which, 0); });
    w.slab = cv.take(w.slab_bytes);
    w.total = cv.off;
    return w;
}

int at_run(const ncx_mlb_att_dims& d, const ncx_mlb_att_train& t, const ncx_mlb_att_params& m, const AtLayout& w, const AtPtrs& p, int which, int gi,
           char* ws, hipStream_t s) {
    return run_request(at_gemm(d, t, m, w, p, which, gi), ws, w.slab, w.slab_bytes, s);
}

// which kernel d conv_v_att.weight takes (ncx_mlb_att_dwv_form): 0 k_att_dwv_small, 1 fp32 k_att_dwv, 2 k_att_dwv_x6
inline int at_dwv_form(int P, uint32_t flags) { return P < 4 ? 0 : (flags & NCX_F_X6) ? 2 : 1; }

bool at_grads_null(const ncx_mlb_att_grads* g) {
    return !g->wv_att || !g->bv_att || !g->wq_att || !g->bq_att || !g->wa || !g->ba || !g->wg || !g->bg || !g->wqf || !g->bqf || !g->wc || !g->bc;
}
}  // namespace

extern "C" {
size_t ncx_mlb_att_train_workspace_bytes(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const ncx_mlb_att_params* m) {
    if (at_check(d, t, m, false) != NCX_OK) return 0;
    return at_layout(*d, *t, *m).total;
}

int ncx_mlb_att_train_ws_region(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const ncx_mlb_att_params* m, int32_t which,
                                size_t* offset, size_t* bytes) {
    if (!offset || !bytes) return NCX_E_NULL;
    const int rc = at_check(d, t, m, false);
    if (rc != NCX_OK) return rc;
    const AtLayout w = at_layout(*d, *t, *m);
    const size_t B = d->B;
    if (which == NCX_AT_WS_XV) { *offset = w.stash; *bytes = B * d->P * d->dh_att * 4; }
    else if (which == NCX_AT_WS_VATT) { *offset = w.v_att; *bytes = B * d->G * d->dv * 4; }
    else if (which == NCX_AT_WS_T) { *offset = w.t; *bytes = B * d->G * d->dh_f * 4; }
    else if (which == NCX_AT_WS_VD) { *offset = w.vd; *bytes = w.vd_bytes; }
    else if (which == NCX_AT_WS_DWV) { *offset = w.dwv; *bytes = w.dwv_bytes; }
    else return NCX_E_FLAGS;
    return NCX_OK;
}

int ncx_mlb_att_train_forward(const ncx_mlb_att_dims* dp, const ncx_mlb_att_train* tp, const float* feats, const int32_t* img_idx,
                              const float* q_emb, const ncx_mlb_att_params* mp, const float* masks, void* workspace,
                              size_t workspace_bytes, float* logits, float* att, void* stream_) {
    return ncx_mlb_att_train_forward_flags(dp, tp, feats, img_idx, q_emb, mp, masks, 0, workspace, workspace_bytes, logits, att, stream_);
}

int ncx_mlb_att_train_forward_flags(const ncx_mlb_att_dims* dp, const ncx_mlb_att_train* tp, const float* feats, const int32_t* img_idx,
                                    const float* q_emb, const ncx_mlb_att_params* mp, const float* masks, uint32_t flags, void* workspace,
                                    size_t workspace_bytes, float* logits, float* att, void* stream_) {
    if (!att_flags_ok(flags)) return NCX_E_DIMS;
    int rc = at_check(dp, tp, mp, true);
    if (rc != NCX_OK) return rc;
    if (!feats || !img_idx || !q_emb || !workspace || !logits || !att) return NCX_E_NULL;
    const ncx_mlb_att_dims& d = *dp; const ncx_mlb_att_train& t = *tp; const ncx_mlb_att_params& m = *mp;
    if (t.dropout_mode == 2 && !masks) return NCX_E_NULL;
    const AtLayout w = at_layout(d, t, m);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    auto F = [&](size_t o) { return (float*)(ws + o); };
    const TrainDrop k = at_drop(t);
    const float* mk = t.dropout_mode == 2 ? masks : nullptr;
    const int GF = d.G * d.dh_f;
    const long long nq = (long long)d.B * d.dq, nmap = (long long)d.B * d.dv * d.P, nva = (long long)d.B * d.G * d.dv;
    AtPtrs p{};
    p.masks = mk; p.q2 = q_emb; p.q5 = q_emb; p.v4 = F(w.v_att);
    p.xq = F(w.xq); p.xv = F(w.xv); p.xqf = F(w.xqf); p.tc = F(w.tc); p.logits = logits;
    if (at_on(t, 1)) {
        hipLaunchKernelGGL(k_at_dropmap, dim3(grid256(nmap)), dim3(256), 0, s, feats, img_idx, d.n_img, (long long)d.dv * d.P, nmap, k,
                           ptr_off(mk, w.m_off[0]), F(w.vd));
        NCX_HIP_TRY(hipGetLastError());
    }
    if (at_on(t, 2)) {
        NCX_HIP_TRY(train_drop_flat(q_emb, F(w.q2), nq, k, 2, ptr_off(mk, w.m_off[1]), s));
        p.q2 = F(w.q2);
    }
    if (at_on(t, 5)) {
        NCX_HIP_TRY(train_drop_flat(q_emb, F(w.q5), nq, k, 5, ptr_off(mk, w.m_off[4]), s));
        p.q5 = F(w.q5);
    }
    rc = at_run(d, t, m, w, p, AT_XQ, 0, ws, s); if (rc) return rc;
    {
        AttArgs a{};
        a.feats = at_on(t, 1) ? F(w.vd) : feats; a.img_idx = img_idx; a.wv = m.wv_att; a.bv = m.bv_att; a.xq = p.xq; a.wa = m.wa;
        a.slab = F(w.aslab);
        a.P = d.P; a.dv = d.dv; a.dh = d.dh_att; a.G = d.G; a.n_img = d.n_img; a.HT = w.HT; a.PT = w.PT;
        a.act_v = m.act_v_att; a.act_mm = m.act_mm;
        AttTrain tr{};
        tr.xv_stash = F(w.stash); tr.mask3 = ptr_off(mk, w.m_off[2]); tr.drop = k; tr.identity = at_on(t, 1) ? 1 : 0;
        rc = run_att_logits<true>(a, tr, d.B, flags, s);
        if (rc) return rc;
    }
    {
        PoolArgs a{};
        a.feats = feats; a.img_idx = img_idx; a.slab = F(w.aslab); a.ba = m.ba; a.att = att; a.v_att = F(w.v_att);
        a.P = d.P; a.dv = d.dv; a.G = d.G; a.n_img = d.n_img; a.HT = w.HT;
        long long chunks = cdiv(1024, d.B);
        if (chunks > cdiv(d.dv, 16)) chunks = cdiv(d.dv, 16);
        if (chunks < 1) chunks = 1;
        a.rows_per_chunk = (int)(cdiv(cdiv(d.dv, chunks), 8) * 8);
        chunks = cdiv(d.dv, a.rows_per_chunk);
        hipLaunchKernelGGL(k_att_pool, dim3((unsigned)chunks, (unsigned)d.B), dim3(256), (size_t)(d.G * d.P + 4) * 4, s, a);
        NCX_HIP_TRY(hipGetLastError());
    }
    if (at_on(t, 4)) {
        NCX_HIP_TRY(train_drop_flat(F(w.v_att), F(w.v4), nva, k, 4, ptr_off(mk, w.m_off[3]), s));
        p.v4 = F(w.v4);
    }
    rc = at_run(d, t, m, w, p, AT_GLIMPSE, 0, ws, s); if (rc) return rc;
    rc = at_run(d, t, m, w, p, AT_XQF, 0, ws, s); if (rc) return rc;
    const long long total = (long long)d.B * GF;
    hipLaunchKernelGGL(k_att_fuse_train, dim3(grid256(total)), dim3(256), 0, s, p.xv, m.bg, (const float*)p.xqf, GF, total, m.act_v, m.act_c, k,
                       ptr_off(mk, w.m_off[5]), F(w.t), F(w.tc));
    NCX_HIP_TRY(hipGetLastError());
    return at_run(d, t, m, w, p, AT_LOGITS, 0, ws, s);
}

int ncx_mlb_att_train_backward(const ncx_mlb_att_dims* dp, const ncx_mlb_att_train* tp, const float* feats, const int32_t* img_idx,
                               const float* q_emb, const ncx_mlb_att_params* mp, const float* masks, void* workspace,
                               size_t workspace_bytes, const float* att, const float* dlogits, const ncx_mlb_att_grads* g,
                               float* dq_emb, void* stream_) {
    return ncx_mlb_att_train_backward_flags(dp, tp, feats, img_idx, q_emb, mp, masks, 0, workspace, workspace_bytes, att, dlogits, g, dq_emb,
                                            stream_);
}

int ncx_mlb_att_dwv_form(const ncx_mlb_att_dims* d, uint32_t flags) {
    if (!att_flags_ok(flags)) return NCX_E_DIMS;
    int rc = check_att_dims(d);
    if (rc == NCX_OK) rc = at_check_dims(d);
    return rc != NCX_OK ? rc : at_dwv_form(d->P, flags);
}

int ncx_mlb_att_train_backward_flags(const ncx_mlb_att_dims* dp, const ncx_mlb_att_train* tp, const float* feats, const int32_t* img_idx,
                                     const float* q_emb, const ncx_mlb_att_params* mp, const float* masks, uint32_t flags, void* workspace,
                                     size_t workspace_bytes, const float* att, const float* dlogits, const ncx_mlb_att_grads* g,
                                     float* dq_emb, void* stream_) {
    if (!att_flags_ok(flags)) return NCX_E_DIMS;
    int rc = at_check(dp, tp, mp, true);
    if (rc != NCX_OK) return rc;
    if (!feats || !img_idx || !q_emb || !workspace || !att || !dlogits || !g || at_grads_null(g)) return NCX_E_NULL;
    const ncx_mlb_att_dims& d = *dp; const ncx_mlb_att_train& t = *tp; const ncx_mlb_att_params& m = *mp;
    if ((t.dropout_mode == 2 && !masks) || (t.want_dq && !dq_emb)) return NCX_E_NULL;
    const AtLayout w = at_layout(d, t, m);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    auto F = [&](size_t o) { return (float*)(ws + o); };
    const TrainDrop k = at_drop(t);
    const float* mk = t.dropout_mode == 2 ? masks : nullptr;
    const int GF = d.G * d.dh_f, B = d.B;
    const long long total = (long long)B * GF, nva = (long long)B * d.G * d.dv, nxq = (long long)B * d.dh_att, nq = (long long)B * d.dq;
    AtPtrs p{};
    p.masks = mk; p.g = *g; p.dlogits = dlogits;
    p.q2 = at_on(t, 2) ? F(w.q2) : q_emb; p.q5 = at_on(t, 5) ? F(w.q5) : q_emb; p.v4 = at_on(t, 4) ? F(w.v4) : F(w.v_att);
    p.tc = F(w.tc); p.dt = F(w.dt); p.dpv = F(w.dpv); p.dpqf = F(w.dpqf); p.dvatt = F(w.dvatt); p.dxq = F(w.dxq);
    p.dq = dq_emb; p.dq2 = F(w.dq2);
    auto sumrows = [&](const float* in, long long n, int R, float* out) {
        hipLaunchKernelGGL(k_at_sumrows, dim3(grid256(n)), dim3(256), 0, s, in, n, R, out);
        return (int)hipGetLastError();
    };
    // the classifier and the glimpse fusion
    rc = at_run(d, t, m, w, p, AT_DWC, 0, ws, s); if (rc) return rc;
    rc = at_run(d, t, m, w, p, AT_DT, 0, ws, s); if (rc) return rc;
    NCX_HIP_TRY(train_dfuse(F(w.dt), F(w.t), F(w.xv), F(w.xqf), total, m.act_v, m.act_q, m.act_c, F(w.dpv), F(w.dpqf), s));
    rc = at_run(d, t, m, w, p, AT_DWG, 0, ws, s); if (rc) return rc;
    rc = at_run(d, t, m, w, p, AT_DWQF, 0, ws, s); if (rc) return rc;
    rc = sumrows(dlogits, d.A, B, g->bc); if (rc) return rc;
    rc = sumrows(p.dpv, GF, B, g->bg); if (rc) return rc;
    rc = sumrows(p.dpqf, GF, B, g->bqf); if (rc) return rc;
    for (int gi = 0; gi < d.G; ++gi) { rc = at_run(d, t, m, w, p, AT_DVATT, gi, ws, s); if (rc) return rc; }
    if (at_on(t, 4)) {
        NCX_HIP_TRY(train_drop_flat(p.dvatt, p.dvatt, nva, k, 4, ptr_off(mk, w.m_off[3]), s));
    }
    {   // the pooling and the softmax over positions
        DattArgs a{};
        a.feats = feats; a.img_idx = img_idx; a.dvatt = p.dvatt; a.partial = F(w.dattp);
        a.P = d.P; a.dv = d.dv; a.G = d.G; a.n_img = d.n_img; a.chunks = w.chunks;
        hipLaunchKernelGGL(k_at_datt, dim3((unsigned)w.chunks, (unsigned)B), dim3(256), 0, s, a);
        NCX_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_at_ds, dim3((unsigned)d.G, (unsigned)B), dim3(256), 0, s, (const float*)F(w.dattp), att, d.P, d.G, w.chunks, F(w.ds),
                           F(w.dba_p));
        NCX_HIP_TRY(hipGetLastError());
        rc = sumrows(F(w.dba_p), d.G, B, g->ba); if (rc) return rc;
    }
    {   // the attention head, element-wise over the stash
        HeadArgs a{};
        a.stash = F(w.stash); a.xq = F(w.xq); a.ds = F(w.ds); a.wa = m.wa; a.mask3 = ptr_off(mk, w.m_off[2]);
        a.dxq = F(w.dxq); a.dwa_p = F(w.dwa_p); a.dbv_p = F(w.dbv_p); a.drop = k;
        a.P = d.P; a.dh = d.dh_att; a.G = d.G; a.act_v = m.act_v_att; a.act_mm = m.act_mm;
        const size_t lds = ((size_t)d.G * d.P + (size_t)d.G * 64 + 4 * 64 * (size_t)(d.G + 2)) * 4;
        hipLaunchKernelGGL(k_at_head, dim3((unsigned)cdiv(d.dh_att, 64), (unsigned)B), dim3(256), lds, s, a);
        NCX_HIP_TRY(hipGetLastError());
        rc = sumrows(F(w.dwa_p), (long long)d.G * d.dh_att, B, g->wa); if (rc) return rc;
        rc = sumrows(F(w.dbv_p), d.dh_att, B, g->bv_att); if (rc) return rc;
    }
    {   // d conv_v_att.weight
        DwvArgs a{};
        a.dxv = F(w.stash); a.map = at_on(t, 1) ? F(w.vd) : feats; a.img_idx = img_idx; a.slab = F(w.dwv);
        a.P = d.P; a.dv = d.dv; a.dh = d.dh_att; a.B = B; a.n_img = d.n_img; a.ipg = w.ipg;
        a.HT = (int)cdiv(d.dh_att, DWV_TH); a.CT = (int)cdiv(d.dv, DWV_TC); a.identity = at_on(t, 1) ? 1 : 0;
        if (at_dwv_form(d.P, flags) == 2) {             // the same slab, groups and sum; fewer, larger tiles
            static DevMask attr_set{0};
            a.HT = (int)cdiv(d.dh_att, DWV6_TH); a.CT = (int)cdiv(d.dv, DWV6_TC);
            NCX_HIP_TRY(set_max_lds_once(attr_set, (const void*)k_att_dwv_x6, DwvCfg6::LDS_BYTES));
            hipLaunchKernelGGL(k_att_dwv_x6, dim3((unsigned)((long long)w.S * a.HT * a.CT)), dim3(DWV6_T), DwvCfg6::LDS_BYTES, s, a);
            NCX_HIP_TRY(hipGetLastError());
            rc = sumrows(F(w.dwv), (long long)d.dh_att * d.dv, w.S, g->wv_att); if (rc) return rc;
        } else if (d.P >= 4) {
            hipLaunchKernelGGL(k_att_dwv, dim3((unsigned)((long long)w.S * a.HT * a.CT)), dim3(256), 0, s, a);
            NCX_HIP_TRY(hipGetLastError());
            rc = sumrows(F(w.dwv), (long long)d.dh_att * d.dv, w.S, g->wv_att); if (rc) return rc;
        } else {
            hipLaunchKernelGGL(k_att_dwv_small, dim3(grid256((long long)d.dh_att * d.dv)), dim3(256), 0, s, a, g->wv_att);
            NCX_HIP_TRY(hipGetLastError());
        }
    }
    // the question side
    if (m.act_q_att == 2) {
        NCX_HIP_TRY(train_dact(F(w.dxq), F(w.xq), nxq, 2, nullptr, nullptr, 0, 0, s));
    }
    rc = at_run(d, t, m, w, p, AT_DWQ, 0, ws, s); if (rc) return rc;
    rc = sumrows(p.dxq, d.dh_att, B, g->bq_att); if (rc) return rc;
    if (t.want_dq) {
        rc = at_run(d, t, m, w, p, AT_DQ1, 0, ws, s); if (rc) return rc;
        rc = at_run(d, t, m, w, p, AT_DQ2, 0, ws, s); if (rc) return rc;
        hipLaunchKernelGGL(k_at_add, dim3(grid256(nq)), dim3(256), 0, s, dq_emb, (const float*)p.dq2, nq);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}
}  // extern "C"
