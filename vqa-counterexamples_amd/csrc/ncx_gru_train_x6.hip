// ncx_gru_train_x6.hip -- the bf16 x 6 (NCX_F_X6) form of the question encoder's backward through time: its four matrix products on
// v_mfma_f32_16x16x32_bf16.  k_gru_dw_x6 is the weight-gradient walk of k_rnn_dw<GATHER, false> (ncx_rnn.hip), k_gru_bgemm_x6 the reverse
// sweep and dX of k_gru_bgemm (ncx_gru_train.hip); gru_dw_x6, gru_sweep_x6 and gru_dx_x6 launch them.  Not the default:
// ncx_gru_train_backward_flags takes them when its `flags` say so (ncx_gru_bwd_form names the products).
//
// The walk is k_rnn_dw's line for line: out[g units + u][c] = sum over (t >= xshift, row < n_t[t]) of dG_t[row][col(g unitsp + u)] X(t, row)[c],
// n_t read on the device, rows in k-steps of 32, a step's k-range ends at n_t rounded up to the k-step, the gate-gradient rows beyond n_t
// are zeroed on the load side BEFORE the cut (the workspace may hold anything there, and the cut of a NaN is NaN), X rows beyond n_t are
// read from the clamped row n_t - 1 (a valid stash row or a row of E), gathered rows go through the tok table (-1 is never an address), one
// workgroup walks the whole contraction in order (no slabs, no reduction launch, no atomics), and with no k-step at all the tile is
// exactly 0.  What differs is the product, as in k_dw_tn8_x6 (ncx_dwtn.hip): the operands are cut into three bf16 planes when their tile
// is stored to LDS and EIGHT plane products per 16 x 16 x 32 block run with fp32 accumulation, a1 x1 on one accumulator and the seven
// small ones on a second, added when the tile leaves (six products on one accumulator were 2.2 - 2.5 x the fp32 error there) -- the cut,
// the order of the products, what is dropped and what is outside the contract: ncx_x6.h.
// One workgroup: 8 waves in a 4 x 2 grid, 256 gate rows x 64 feature columns, a wave 64 x 32 = 4 x 2 MFMA blocks.  LDS, double buffered:
// three planes of [32 k-rows][256 | 64] bf16 in the global row-is-k layout, row pitches 544 / 160 bytes (= 32 mod 256: the eight k-rows
// that one 32-lane half of a ds_read_b64_tr_b16 touches fall on disjoint banks); fragments come from the transposing read, so lane group
// lk holds k = 4 lk .. + 3 and 16 + 4 lk .. + 3 of BOTH operands.  135 168 bytes: one workgroup per CU, two waves per SIMD.
// Register-staged, one barrier per k-step: the loads of step s + 1 fly over the MFMAs of step s and are cut and stored to the other buffer
// after them; a thread loads four quads of the gate-gradient tile and one of the X tile per k-step.
#include "ncx_gru.h"

using namespace ncx;

namespace {
constexpr int W6_BM = 256, W6_BN = 64, W6_T = 512;
constexpr int W6_GM = 4;                                           // gate-row tiles that are neighbours in the work order
constexpr int W6_PA = 2 * W6_BM + 32, W6_PB = 2 * W6_BN + 32;      // bytes per k-row of one plane
constexpr int W6_APL = GEMM_BK * W6_PA;                            // the gate-gradient rows of one plane; the X rows follow
constexpr int W6_PL = GEMM_BK * (W6_PA + W6_PB), W6_BUF = 3 * W6_PL, W6_LDS = 2 * W6_BUF;
static_assert(GEMM_BK == 32, "one k-step is one MFMA depth");
static_assert(W6_LDS <= 160 * 1024, "LDS");
static_assert(W6_T * 4 == GEMM_BK * W6_BM / 4 && W6_T == GEMM_BK * W6_BN / 4, "the loader: 4 quads of the gate-gradient tile, 1 of the X tile per thread");
}  // namespace

template <bool GATHER>
__global__ __launch_bounds__(W6_T, 1) void k_gru_dw_x6(const RnnDwArgs a) {
    extern __shared__ __attribute__((aligned(16))) unsigned char w6_smem[];
    // Consecutive work items run on the same XCD at the same time (rnn_work_item), and they are ordered so that 32 of them (an XCD's
    // CUs) form W6_GM gate-row tiles x 8 column tiles: per
    // k-step that L2 then fetches 4 gate-gradient tiles and 8 X tiles (192 KB) for its 32 workgroups instead of 32 of each (1 280 KB).
    // The operands are far larger than an L2 (dG 511 MB at B = 512, T = 26), so what is not shared there comes from beyond it.
    const int tiles_n = (a.cols + W6_BN - 1) / W6_BN, total = a.tiles_m * tiles_n;
    const int w = rnn_work_item(blockIdx.x, total);
    if (w >= total) return;                      // (uniform: before any barrier)
    const int grp = w / (W6_GM * tiles_n), rest = w - grp * (W6_GM * tiles_n), gm = min(W6_GM, a.tiles_m - grp * W6_GM);
    const int tn = rest / gm, m0 = (grp * W6_GM + (rest - tn * gm)) * W6_BM, n0 = tn * W6_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wm0 = 64 * (wave >> 1), wn0 = 32 * (wave & 1);

    // loader: thread owns column quad aq of the k-rows arow + 8 i of the gate-gradient tile, and column quad bq of k-row brow of the X tile
    const int arow = tid >> 6, aq = tid & 63, brow = tid >> 4, bq = tid & 15;
    const int am = min(m0 + 4 * aq, a.kp - 4);                                    // columns beyond kp: clamped here, never stored
    const int acol = am + (am >= a.skip_from ? a.skip_by : 0);
    const int bcol = n0 + 4 * bq;
    const bool b_full = n0 + W6_BN <= a.cols;

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 va[4], vb;
    bool a_ok[4] = {false, false, false, false};
    auto issue = [&](int t, int r0, int nr) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            const int krow = r0 + arow + 8 * i;
            a_ok[i] = krow < nr;                                                  // rows n_t .. the end of the k-step: zeroed in store()
            va[i] = *(const f32x4*)(a.dG + ((size_t)t * a.B + min(krow, nr - 1)) * a.ld + acol);
        }
        const int rc = min(r0 + brow, nr - 1);
        const float* bp = GATHER ? a.X + (size_t)max(a.tok[(size_t)t * a.B + rc], 0) * a.cols  // an id out of range is -1 here: never an address
                                 : a.X + ((size_t)(t - a.xshift) * a.B + rc) * a.cols;
        if (b_full) vb = *(const f32x4u*)(bp + bcol);
        else vb = load4(bp, bcol, a.cols);
    };
    auto store = [&](int buf) __attribute__((always_inline)) {
        unsigned char* const base = w6_smem + buf * W6_BUF;
#pragma unroll
        for (int i = 0; i < 4; ++i) x6_split_store(a_ok[i] ? va[i] : zero, base + (arow + 8 * i) * W6_PA + 8 * aq, W6_PL);
        x6_split_store(vb, base + W6_APL + brow * W6_PB + 8 * bq, W6_PL);
    };

    f32x4 acc[4][2], acl[4][2];                  // a1 x1 | the seven small plane products
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int j = 0; j < 2; ++j) { acc[i][j] = zero; acl[i][j] = zero; }

    // fragments through x6_frag_tr (ncx_x6.h): lane 4 tq + tp of a 16-lane group points at k-row 4 lk + tq, columns 4 tp .. + 3
    const int tq = li >> 2, tp = li & 3;
    const int fragA = (4 * lk + tq) * W6_PA + 2 * (wm0 + 4 * tp), fragB = W6_APL + (4 * lk + tq) * W6_PB + 2 * (wn0 + 4 * tp);
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const unsigned char* const base = w6_smem + buf * W6_BUF;
        x6_bf16x8 bf[3][2];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int j = 0; j < 2; ++j) bf[p][j] = x6_frag_tr(base + p * W6_PL + fragB + 32 * j, W6_PB);
#pragma unroll
        for (int i = 0; i < 4; ++i) {
            x6_bf16x8 af[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) af[p] = x6_frag_tr(base + p * W6_PL + fragA + 32 * i, W6_PA);
            // small terms first; the two column blocks alternate (a dependent MFMA is two issues away)
#pragma unroll
            for (int c = 0; c < 7; ++c)
#pragma unroll
                for (int j = 0; j < 2; ++j) acl[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[X6S_A[c]], bf[X6S_B[c]][j], acl[i][j], 0, 0, 0);
#pragma unroll
            for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[0], bf[0][j], acc[i][j], 0, 0, 0);
        }
    };

    // the walk: steps xshift .. while n_t[t] > 0 (n_t never rises), rows in k-steps of 32
    int t = a.xshift, r0 = 0, nr = t < a.T ? a.n_t[t] : 0;
    if (nr > 0) {                                // (uniform)
        issue(t, r0, nr); store(0);
        __syncthreads();
        int buf = 0;
        for (;;) {
            r0 += GEMM_BK;
            if (r0 >= nr) { ++t; r0 = 0; nr = t < a.T ? a.n_t[t] : 0; }
            const bool more = nr > 0;
            if (more) issue(t, r0, nr);
            compute(buf);
            if (more) store(buf ^ 1);
            __syncthreads();
            buf ^= 1;
            if (!more) break;
        }
    }

    // epilogue: C layout col = lane & 15 (feature column), row = 4 (lane >> 4) + reg (gate row); with no k-step at all the tile is exactly 0
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = m0 + wm0 + 16 * i + 4 * lk + q, g = m / a.unitsp, uu = m - g * a.unitsp;
            if (m >= a.kp || uu >= a.units) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = n0 + wn0 + 16 * j + li;
                if (c < a.cols) a.out[((size_t)g * a.units + uu) * a.cols + c] = acc[i][j][q] + acl[i][j][q];
            }
        }
}

// ---- the reverse sweep and dX: k_gru_bgemm<DX> (ncx_gru_train.hip) on the bf16 matrix path ------------------------------------------------
// The NT product acc = dG_t[m0 .. + BM][K = 3 dqp] . wT[n0 .. + 64]^T of rnn_nt_tile, both operands col-is-k, cut from fp32 on the way to LDS
// (the transposed pack is read as ncx_gru_pack_t left it); everything around it is k_gru_bgemm's: n_t read on the device, workgroups beyond
// it exit before their first barrier, rows beyond n_t clamped to row n_t - 1 and never stored, the sweep's k-steps from s_hn on one block
// further (da_hn after da_n), and the epilogue line for line.  The LDS row tile is RnnX6Tile<WR, 64> (ncx_rnn.h), as in k_gru_step_x6.
// The waves form a WR x 2 grid, 32 rows x 32 columns each (2 x 2 MFMA blocks, eight plane products per block on two accumulators as in
// the walk).  Work items are dealt to the XCDs in contiguous runs, row tiles of a column
// tile next to each other: an XCD's L2 fetches its share of the weight rows once per launch.
namespace {
constexpr int B6_BN = 64;
template <int WR> using B6 = RnnX6Tile<WR, B6_BN>;
}  // namespace

template <bool DX, int WR>
__global__ __launch_bounds__(128 * WR, 1) void k_gru_bgemm_x6(const GruBgArgs a, int tiles_n) {
    typedef B6<WR> Tile;
    constexpr int BM = Tile::BM, NB = Tile::NB;
    extern __shared__ __attribute__((aligned(16))) unsigned char b6_smem[];
    const int t = DX ? (int)blockIdx.y : a.t;
    const int total = a.tiles_m * tiles_n;
    const int w = rnn_work_item(blockIdx.x, total);
    if (w >= total) return;
    const int tn = w / a.tiles_m, m0 = (w - tn * a.tiles_m) * BM, n0 = tn * B6_BN;       // row tiles of a column tile share its weight rows
    const int nprod = t < a.T ? a.n_t[t] : 0;
    const int nout = DX ? nprod : a.n_t[t - 1];
    if (m0 >= nout) return;                    // (uniform: before any barrier)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wu = wave & 1;   // wave tile: rows 32 wr .. + 32, columns 32 wu .. + 32
    const int kp = 3 * a.dqp, dg_ld = 4 * a.dqp;
    const int ns = m0 < nprod ? kp / GEMM_BK : 0;
    const bool live = m0 + 32 * wr < nprod;    // (wave-uniform)

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][2] = {{zero, zero}, {zero, zero}}, acl[2][2] = {{zero, zero}, {zero, zero}};     // a1 w1 | the seven small plane products
    if (ns > 0) {
        const Tile tile(b6_smem);
        // loader: the gate-gradient rows behind the A tile's rows, the column tile's rows of the transposed pack
        const float* aptr[2]; const float* bptr[NB];
#pragma unroll
        for (int i = 0; i < 2; ++i) aptr[i] = a.dG + ((size_t)t * a.B + rnn_clamp_row(m0 + tile.arow(i), nprod)) * dg_ld + tile.c4;
#pragma unroll
        for (int i = 0; i < NB; ++i) bptr[i] = a.wT + (size_t)(n0 + tile.wrow(i)) * kp + tile.c4;
        const int s_hn = 2 * a.dqp / GEMM_BK, skip = DX ? 0 : a.dqp;
        f32x4 va[2], vb[NB];
        auto issue = [&](int s) __attribute__((always_inline)) {
            const int ka = s * GEMM_BK + (s >= s_hn ? skip : 0);                 // (uniform)
#pragma unroll
            for (int i = 0; i < 2; ++i) va[i] = *(const f32x4*)(aptr[i] + ka);
            tile.load_w(bptr, s, vb);
        };
        const int fragA = tile.frag_at(32 * wr + li), fragB = tile.frag_at(BM + 32 * wu + li);
        auto compute = [&](int buf, int) __attribute__((always_inline)) {
            x6_bf16x8 af[2][3], bf[2][3];
            tile.read_a(buf, fragA, af);
            tile.read_a(buf, fragB, bf);
            // small terms first; inside one product the four blocks alternate (a dependent MFMA is four issues away)
#pragma unroll
            for (int c = 0; c < 7; ++c)
#pragma unroll
                for (int i = 0; i < 2; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acl[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][X6S_A[c]], bf[j][X6S_B[c]], acl[i][j], 0, 0, 0);
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][0], bf[j][0], acc[i][j], 0, 0, 0);
        };
        tile.run(ns, live, va, vb, issue, [](int) {}, compute);
    }

    // epilogue (k_gru_bgemm's): C layout col = lane & 15, row = 4 (lane >> 4) + reg
    const int u = t - 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + 32 * wr + 16 * i + 4 * lk + e, col = n0 + 32 * wu + 16 * jj + li;
                const float prod = acc[i][jj][e] + acl[i][jj][e];
                if (row >= nout) continue;
                if (DX) {
                    if (col < a.de) a.dX[((size_t)t * a.B + row) * a.de + col] = prod;
                    continue;
                }
                if (col >= a.dqp) continue;
                float* dgo = a.dG + ((size_t)u * a.B + row) * dg_ld + col;
                if (col >= a.dq) {                                               // pad columns: zero, they are k positions of later products
                    dgo[0] = 0.f; dgo[a.dqp] = 0.f; dgo[2 * a.dqp] = 0.f; dgo[3 * a.dqp] = 0.f;
                    continue;
                }
                float dh = 0.f;
                if (row < nprod) dh = prod + a.gates[((size_t)t * a.B + row) * dg_ld + a.dqp + col] * a.dh_in[(size_t)row * a.dq + col];
                if (a.lens[row] == t) dh += a.dq_out[(size_t)a.perm[row] * a.dq + col];
                const float* g = a.gates + ((size_t)u * a.B + row) * dg_ld + col;
                const float r = g[0], z = g[a.dqp], n = g[2 * a.dqp], hn = g[3 * a.dqp];
                const float hp = u > 0 ? a.hstash[((size_t)(u - 1) * a.B + row) * a.dq + col] : 0.f;
                const float dn = dh * (1.f - z), dz = dh * (hp - n);
                const float da_n = dn * (1.f - n * n), da_z = dz * z * (1.f - z);
                a.dh_out[(size_t)row * a.dq + col] = dh;
                dgo[0] = da_n * hn * r * (1.f - r); dgo[a.dqp] = da_z; dgo[2 * a.dqp] = da_n; dgo[3 * a.dqp] = da_n * r;
            }
}

namespace ncx {
template <bool DX, int WR>
static hipError_t gru_bgemm_x6_launch(const GruBgArgs& args, int cols, int steps, hipStream_t s) {
    static DevMask attr{0};
    const hipError_t e = set_max_lds_once(attr, (const void*)k_gru_bgemm_x6<DX, WR>, B6<WR>::LDS);
    if (e != hipSuccess) return e;
    GruBgArgs a = args;
    a.tiles_m = (int)cdiv(a.B, B6<WR>::BM);
    const int tiles_n = (int)cdiv(cols, B6_BN);
    hipLaunchKernelGGL((k_gru_bgemm_x6<DX, WR>), dim3((unsigned)(8 * cdiv((long long)a.tiles_m * tiles_n, 8)), (unsigned)steps), dim3(B6<WR>::T),
                       B6<WR>::LDS, s, a, tiles_n);
    return hipGetLastError();
}

hipError_t gru_sweep_x6(const GruBgArgs& a, hipStream_t s) { return gru_bgemm_x6_launch<false, GRU_B6_WR>(a, a.dq, 1, s); }
hipError_t gru_dx_x6(const GruBgArgs& a, hipStream_t s) { return gru_bgemm_x6_launch<true, GRU_B6_WR>(a, a.de, a.T, s); }
}  // namespace ncx

namespace ncx {
hipError_t gru_dw_x6(const RnnDwArgs& args, bool gather, hipStream_t s) {
    static DevMask attr_g{0}, attr_s{0};
    RnnDwArgs a = args;
    a.tiles_m = (int)cdiv(a.kp, W6_BM);
    const dim3 grid((unsigned)(8 * cdiv(a.tiles_m * cdiv(a.cols, W6_BN), 8)));
    if (gather) {
        const hipError_t e = set_max_lds_once(attr_g, (const void*)k_gru_dw_x6<true>, W6_LDS);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_gru_dw_x6<true>, grid, dim3(W6_T), W6_LDS, s, a);
    } else {
        const hipError_t e = set_max_lds_once(attr_s, (const void*)k_gru_dw_x6<false>, W6_LDS);
        if (e != hipSuccess) return e;
        hipLaunchKernelGGL(k_gru_dw_x6<false>, grid, dim3(W6_T), W6_LDS, s, a);
    }
    return hipGetLastError();
}
}  // namespace ncx
