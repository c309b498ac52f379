// ncx_lstm_train.hip -- training the two-layer LSTM question encoder (TwoLSTM below its dropout): the forward that keeps what the backward
// needs, and backward through time.  ncx_lstm2_train_workspace_bytes, ncx_lstm2_packed_t_bytes, ncx_lstm2_pack_t, ncx_lstm2_train_forward,
// ncx_lstm2_train_backward.
//
// Reference: vqa/models/seq2vec.py -- process_lengths + select_last (11-25), TwoLSTM (48-76); what is replaced is torch autograd through
// tanh(nn.Embedding) + two nn.LSTMs + the last-step selection.  With len_b, perm, n_t of ncx_lstm.hip, per layer l, for t from len_b - 1 down to 0:
//   dh^l_t = [t == len_b - 1] dq_out[b, l H : (l + 1) H] + da^l_{t+1} . W_hh^l  (+ da^1_t . W_ih^1 when l == 0)
//   dc_t   = dc_{t+1} f_{t+1} + dh_t o_t (1 - tanh(c_t)^2)
//   da_o = dh_t tanh(c_t) o (1 - o);  da_i = dc_t g i (1 - i);  da_g = dc_t i (1 - g^2);  da_f = dc_t c_{t-1} f (1 - f)   (c_{-1} = 0)
//   dW_ih^l = sum da^l_t^T x^l_t;  dW_hh^l = sum_{t >= 1} da^l_t^T h^l_{t-1};  db_ih^l = db_hh^l = sum da^l_t
//   dX_t = da^0_t . W_ih^0;  dE[w] = (sum over the valid pairs with id w of dX_t) (1 - tanh(E[w])^2);  dE[0] = 0
// Stash (workspace, per layer, [T][B] in the plan's sorted row order): h_t [H]; c_t [H]; gates i | f | g | o [4][Hp]; gate gradients
// da_i | da_f | da_g | da_o [4][Hp] (Hp = H up to a whole 32-deep k-step, pad columns written as zeros: they are k positions of the
// later products); dcf [B][H] = dc_t f_t, what step t - 1 takes from step t.
// Plan (forward T + 2 launches; backward T + 9, T + 7 without dE; nothing read back, no atomics, no inter-workgroup wait):
//   k_lstm_bgemm<false>  the reverse wavefront, launch u = T - 1 .. -1, all issued: layer 1 at step u and layer 0 at step u + 1 as two ranges of
//                        workgroup ids; both read only what launch u + 1 wrote.  Layer 1: da^1_{u+1}[0:n_{u+1}) . W_hh^1 (K = 4 Hp); layer 0 at
//                        t = u + 1: [da^0_{t+1}[0:n_{t+1}) | da^1_t[0:n_t)] . [W_hh^0 ; W_ih^1] (K = 8 Hp) on v_mfma_f32_16x16x4_f32.  The rows
//                        [n_{t+1}, n_t) of the first segment are zeroed on the load side.  Epilogue: + the injected half of dq_out[perm[row]]
//                        where len_row - 1 == t, the cell arithmetic from the stash (one tanhf: tanh(c_t) is not kept), dcf and the four
//                        gate-gradient blocks of step t.
//   k_lstm_bgemm<true>   dX_t = da^0_t . W_ih^0 for every step in one launch (grid.y = t) after the sweep; skipped when dE is NULL.
//   k_lstm_dw<GATHER>    the four weight gradients as TN products whose contraction walks (t, row < n_t[t]) with n_t read from memory; one
//                        workgroup per 128 x 64 output tile, the whole walk in order.  GATHER: x = tanh(E[tok]) on the load side.
//   k_lstm_dbias         column sums of da^l -> db_ih^l and db_hh^l.
//   k_lstm_tok, k_lstm_de  the word id of every valid pair (or -1); one workgroup per row of E sums the dX rows of its id in (t, row) order.
#include "ncx_lstm.h"

using namespace ncx;

namespace {
constexpr int LB_BM = 64, LB_BN = 64, LB_P = GEMM_BK + 4;           // sweep / dX tile; LDS pitch as in k_gru_bgemm
constexpr int LW_BM = 128, LW_BN = 64;                                // weight-gradient tile: gate rows x feature columns
constexpr int LW_PA = pitch_rowk(LW_BM), LW_PB = pitch_rowk(LW_BN);   // row-is-k pitches (ncx_gemm.h)

// packed_t = P0 [rows_h][8 Hp] | P1 [rows_h][4 Hp] | PX [rows_x][4 Hp]
struct LstmPackT { int Hp, rows_h, rows_x; size_t off1, offx, floats; };
__host__ __device__ inline LstmPackT lstm_pack_t(int emb, int H) {
    LstmPackT p;
    p.Hp = pad_to(H, GEMM_BK); p.rows_h = pad_to(H, LB_BN); p.rows_x = pad_to(emb, LB_BN);
    p.off1 = (size_t)p.rows_h * 8 * p.Hp; p.offx = p.off1 + (size_t)p.rows_h * 4 * p.Hp;
    p.floats = p.offx + (size_t)p.rows_x * 4 * p.Hp;
    return p;
}
}  // namespace

// P0[j][g Hp + u] = W_hh^0[g H + u][j], P0[j][4 Hp + g Hp + u] = W_ih^1[g H + u][j];  P1[j][g Hp + u] = W_hh^1[g H + u][j];
// PX[c][g Hp + u] = W_ih^0[g H + u][c]; zero where u >= H or the row does not exist (rows up to a multiple of 64).  A 32 x 32 tile per
// workgroup through LDS: both sides coalesced.  grid.x covers 8 Hp / 32 column tiles; P1 and PX use the first half of them.
__global__ __launch_bounds__(256) void k_lstm_pack_t(const float* __restrict__ w_ih0, const float* __restrict__ w_hh0, const float* __restrict__ w_ih1,
                                                     const float* __restrict__ w_hh1, int emb, int H, float* __restrict__ packed_t) {
    __shared__ float tile[32][33];
    const LstmPackT p = lstm_pack_t(emb, H);
    const int c0 = blockIdx.x * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    int row0 = blockIdx.y * 32;                          // (rows_h, rows_x are multiples of 32: a tile never straddles two matrices)
    const int which = row0 < p.rows_h ? 0 : row0 < 2 * p.rows_h ? 1 : 2;
    row0 -= which * p.rows_h;
    const int kp = which == 0 ? 8 * p.Hp : 4 * p.Hp;
    if (c0 >= kp) return;                                // (uniform: before the barrier)
    const bool second = c0 >= 4 * p.Hp;                  // P0's W_ih^1 half
    const float* src = which == 0 ? (second ? w_ih1 : w_hh0) : which == 1 ? w_hh1 : w_ih0;
    const int ld = which == 2 ? emb : H, sc = row0 + tx;
    float* dst = packed_t + (which == 0 ? 0 : which == 1 ? p.off1 : p.offx);
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int c = c0 - (second ? 4 * p.Hp : 0) + ty + 8 * rr, g = c / p.Hp, u = c - g * p.Hp;
        tile[ty + 8 * rr][tx] = (u < H && sc < ld) ? src[((size_t)g * H + u) * ld + sc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) dst[(size_t)(row0 + ty + 8 * rr) * kp + c0 + tx] = tile[tx][ty + 8 * rr];
}

struct LbArgs {
    const float* g0; const float* g1;          // activated gates [T][B][4 Hp]
    const float* c0; const float* c1;          // c_t [T][B][H]
    float* dg0; float* dg1;                    // gate gradients [T][B][4 Hp]
    float* dcf0; float* dcf1;                  // dc_t f_t [B][H]
    const float* w0; const float* w1; const float* wx;      // P0, P1, PX
    const int* perm; const int* lens; const int* n_t; const float* dq_out;
    float* dX;
    int B, T, H, Hp, emb, tiles_m, grid1;
};

// DX = false: launch u of the reverse wavefront; workgroups [0, grid1) run layer `layer_base`, [grid1, 2 grid1) layer 0.
// DX = true: dX_t, t = blockIdx.y.
template <bool DX>
__global__ __launch_bounds__(256) void k_lstm_bgemm(const LbArgs a, int u, int layer_base) {
    __shared__ __attribute__((aligned(16))) float lds[2][(LB_BM + LB_BN) * LB_P];
    const int second = !DX && (int)blockIdx.x >= a.grid1;
    const int layer = DX ? 0 : second ? 0 : layer_base, bid = (int)blockIdx.x - second * a.grid1;
    const int t = DX ? (int)blockIdx.y : layer ? u : u + 1;
    const int tn = bid / a.tiles_m, m0 = (bid - tn * a.tiles_m) * LB_BM, n0 = tn * LB_BN;      // row tiles of a column tile share its weight rows
    const int nout = a.n_t[t];
    const int nnext = (!DX && t + 1 < a.T) ? a.n_t[t + 1] : 0;
    if (m0 >= nout) return;                    // (uniform: before any barrier)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wu = wave & 1;   // wave tile: rows 32 wr .. + 32, columns 32 wu .. + 32
    const int c4 = 4 * (tid & 7), lr = tid >> 3;
    const int H = a.H, Hp = a.Hp, dg_ld = 4 * Hp, nk = dg_ld / GEMM_BK;
    // the k-steps of the weight rows: [0, ka) belong to the first segment (da^l_{t+1}, rows below n_{t+1}), [ka, ..) to the second
    // (layer 0: da^1_t; dX: da^0_t; rows below n_t)
    const int ka = DX ? 0 : nk;
    const int wld = (DX || layer) ? dg_ld : 2 * dg_ld;
    const bool has_a = m0 < nnext;
    const int s0 = DX ? 0 : has_a ? 0 : nk;
    const int s1 = DX ? nk : layer ? (has_a ? nk : 0) : 2 * nk;
    float* const dgl = layer ? a.dg1 : a.dg0;

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][2] = {{zero, zero}, {zero, zero}};
    if (s0 < s1) {
        // loader: thread owns column quad c4 of tile rows lr + 32 i (2 of the A tile, 2 of the weight tile); every load is an aligned 16 bytes
        const float* pa1[2]; const float* pa2[2]; const float* bptr[2];
        bool ok1[2];
        const float* seg2 = DX ? a.dg0 : a.dg1;
        const float* wT = DX ? a.wx : layer ? a.w1 : a.w0;
        const int t1 = min(t + 1, a.T - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = m0 + lr + 32 * i;
            ok1[i] = r < nnext;                                                   // rows [n_{t+1}, n_t): zeroed in store()
            pa1[i] = dgl + ((size_t)t1 * a.B + max(min(r, nnext - 1), 0)) * dg_ld + c4;
            pa2[i] = seg2 + ((size_t)t * a.B + min(r, nout - 1)) * dg_ld + c4;   // rows beyond n_t: clamped here, never stored
            bptr[i] = wT + (size_t)(n0 + lr + 32 * i) * wld + c4;               // (weight rows are padded to whole tiles)
        }
        f32x4 va[2], vb[2];
        bool first = false;
        auto issue = [&](int s) __attribute__((always_inline)) {
            first = s < ka;
#pragma unroll
            for (int i = 0; i < 2; ++i) va[i] = *(const f32x4*)(first ? pa1[i] + s * GEMM_BK : pa2[i] + (s - ka) * GEMM_BK);
#pragma unroll
            for (int i = 0; i < 2; ++i) vb[i] = *(const f32x4*)(bptr[i] + s * GEMM_BK);
        };
        auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(lr + 32 * i) * LB_P + c4]) = (first && !ok1[i]) ? zero : va[i];
#pragma unroll
            for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(LB_BM + lr + 32 * i) * LB_P + c4]) = vb[i];
        };
        // MFMA (tt, e) takes k = 8 tt + 2 lk + e from lane group lk for both operands (ncx_gemm.h)
        auto compute = [&](int buf) __attribute__((always_inline)) {
            const float* pa = &lds[buf][(32 * wr + li) * LB_P + 2 * lk];
            const float* pb = &lds[buf][(LB_BM + 32 * wu + li) * LB_P + 2 * lk];
#pragma unroll
            for (int tt = 0; tt < GEMM_BK / 8; ++tt) {
                const f32x2 a0 = *(const f32x2*)(pa + 8 * tt), a1 = *(const f32x2*)(pa + 16 * LB_P + 8 * tt);
                const f32x2 b0 = *(const f32x2*)(pb + 8 * tt), b1 = *(const f32x2*)(pb + 16 * LB_P + 8 * tt);
#pragma unroll
                for (int e = 0; e < 2; ++e) {
                    acc[0][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b0[e], acc[0][0], 0, 0, 0);
                    acc[1][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b0[e], acc[1][0], 0, 0, 0);
                    acc[0][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b1[e], acc[0][1], 0, 0, 0);
                    acc[1][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b1[e], acc[1][1], 0, 0, 0);
                }
            }
        };
        // register-staged double-buffered LDS, one barrier per k-step: the loads of step s + 1 fly over the MFMAs of step s
        issue(s0); store(0);
        __syncthreads();
        int buf = 0;
        for (int s = s0; s < s1; ++s) {
            const bool more = s + 1 < s1;
            if (more) issue(s + 1);
            compute(buf);
            if (more) store(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
    }

    // epilogue: C layout col = lane & 15, row = 4 (lane >> 4) + reg
    const float* gl = layer ? a.g1 : a.g0;
    const float* cl = layer ? a.c1 : a.c0;
    float* dcf = layer ? a.dcf1 : a.dcf0;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + 32 * wr + 16 * i + 4 * lk + e, col = n0 + 32 * wu + 16 * jj + li;
                if (row >= nout) continue;
                if (DX) {
                    if (col < a.emb) a.dX[((size_t)t * a.B + row) * a.emb + col] = acc[i][jj][e];
                    continue;
                }
                if (col >= Hp) continue;
                float* dgo = dgl + ((size_t)t * a.B + row) * dg_ld + col;
                if (col >= H) {                                                  // pad columns: zero, they are k positions of later products
                    dgo[0] = 0.f; dgo[Hp] = 0.f; dgo[2 * Hp] = 0.f; dgo[3 * Hp] = 0.f;
                    continue;
                }
                float dh = acc[i][jj][e];
                if (a.lens[row] - 1 == t) dh += a.dq_out[(size_t)a.perm[row] * (2 * (size_t)H) + (size_t)layer * H + col];
                const float* g = gl + ((size_t)t * a.B + row) * dg_ld + col;
                const float gi = g[0], gf = g[Hp], gg = g[2 * Hp], go = g[3 * Hp];
                const size_t at = (size_t)row * H + col;
                const float tc = tanhf(cl[(size_t)t * a.B * H + at]);
                const float cp = t > 0 ? cl[(size_t)(t - 1) * a.B * H + at] : 0.f;
                float dc = dh * go * (1.f - tc * tc);
                if (row < nnext) dc += dcf[at];                                  // dc_{t+1} f_{t+1}, written by this thread's counterpart of step t + 1
                dcf[at] = dc * gf;
                dgo[0] = dc * gg * gi * (1.f - gi); dgo[Hp] = dc * cp * gf * (1.f - gf); dgo[2 * Hp] = dc * gi * (1.f - gg * gg);
                dgo[3 * Hp] = dh * tc * go * (1.f - go);
            }
}

struct LwArgs {
    const float* dG; const float* X;           // X: a [T][B][cols] stash, row (t - xshift, row); GATHER: E, row tok[t][row]
    const int* tok; const int* n_t; float* out;
    int B, T, H, Hp, cols, tiles_m, xshift;     // cols: width of X's rows = columns of out; the walk starts at t = xshift
};

// out[g H + u][c] = sum over t >= xshift, row < n_t[t] of dG_t[row][g Hp + u] * X(t, row)[c]
template <bool GATHER>
__global__ __launch_bounds__(256) void k_lstm_dw(const LwArgs a) {
    __shared__ __attribute__((aligned(16))) float la[2][GEMM_BK * LW_PA];
    __shared__ __attribute__((aligned(16))) float lb[2][GEMM_BK * LW_PB];
    const int tn = (int)blockIdx.x / a.tiles_m, m0 = ((int)blockIdx.x - tn * a.tiles_m) * LW_BM, n0 = tn * LW_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wm0 = (wave >> 1) * (LW_BM / 2), wn0 = (wave & 1) * (LW_BN / 2);
    const int kr = tid >> 3, cq = 4 * (tid & 7);
    const int kp = 4 * a.Hp;                   // (a multiple of 128: the gate-row tiles are whole)

    // loader: thread owns k-row kr of the step, column quads cq + 32 i (4 of the gate-gradient tile, 2 of the X tile)
    int acol[4], bcol[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) acol[i] = min(m0 + cq + 32 * i, kp - 4);
#pragma unroll
    for (int i = 0; i < 2; ++i) bcol[i] = n0 + cq + 32 * i;
    const bool b_full = n0 + LW_BN <= a.cols;

    f32x4 va[4], vb[2];
    bool a_ok = false;
    auto issue = [&](int t, int r0, int nr) __attribute__((always_inline)) {
        const int krow = r0 + kr, rc = min(krow, nr - 1);
        a_ok = krow < nr;                                                         // rows n_t .. the end of the k-step: zeroed in store()
        const float* ap = a.dG + ((size_t)t * a.B + rc) * kp;
        const float* bp = GATHER ? a.X + (size_t)max(a.tok[(size_t)t * a.B + rc], 0) * a.cols  // an id out of range is -1 here: never an address
                                 : a.X + ((size_t)(t - a.xshift) * a.B + rc) * a.cols;
#pragma unroll
        for (int i = 0; i < 4; ++i) va[i] = *(const f32x4*)(ap + acol[i]);
        if (b_full) {
#pragma unroll
            for (int i = 0; i < 2; ++i) vb[i] = *(const f32x4u*)(bp + bcol[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) vb[i] = load4(bp, bcol[i], a.cols);
        }
    };
    auto store = [&](int buf) __attribute__((always_inline)) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if (GATHER) {                          // x = tanh(E[wid]); tanh(0) = 0 keeps the zero fill
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) vb[i][e] = tanhf(vb[i][e]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) *(f32x4*)(&la[buf][kr * LW_PA + cq + 32 * i]) = a_ok ? va[i] : zero;
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(&lb[buf][kr * LW_PB + cq + 32 * i]) = vb[i];
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc[i][0] = zero; acc[i][1] = zero; }
    // interleaved block mapping (ncx_gemm.h): MFMA block i of a wave owns tile rows wm0 + 4 r + i, block j tile columns wn0 + 2 c + j, so one
    // ds_read_b128 / ds_read_b64 per k-row feeds all of a lane's blocks
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const float* pa = &la[buf][wm0 + 4 * li];
        const float* pb = &lb[buf][wn0 + 2 * li];
#pragma unroll
        for (int tt = 0; tt < GEMM_BK / 8; ++tt) {
            const int kk = 8 * tt + 2 * lk;
            f32x4 av[2]; f32x2 bv[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) { av[e] = *(const f32x4*)(pa + (kk + e) * LW_PA); bv[e] = *(const f32x2*)(pb + (kk + e) * LW_PB); }
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e][i], bv[e][j], acc[i][j], 0, 0, 0);
        }
    };

    // the walk: steps xshift .. while n_t[t] > 0 (n_t never rises), rows in k-steps of 32; same double-buffered pipeline as above
    int t = a.xshift, r0 = 0, nr = t < a.T ? a.n_t[t] : 0;
    if (nr > 0) {
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

    // epilogue: acc[i][j][q] is tile row wm0 + 4 (4 lk + q) + i, tile column wn0 + 2 li + j; with no k-step at all the tile is exactly 0
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = m0 + wm0 + 4 * (4 * lk + q) + i, g = m / a.Hp, uu = m - g * a.Hp;
            if (m >= kp || uu >= a.H) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = n0 + wn0 + 2 * li + j;
                if (c < a.cols) a.out[((size_t)g * a.H + uu) * a.cols + c] = acc[i][j][q];
            }
        }
}

// db_ih^l = db_hh^l = column sums of da^l over every valid pair.  grid = 2 layers x (4 Hp / 32); a workgroup owns 32 columns; thread (g, c)
// sums rows g, g + 8, ... of every step in ascending order, the 8 partial sums are added in ascending g (k_mt_colsum's scheme).
__global__ __launch_bounds__(256) void k_lstm_dbias(const float* __restrict__ dg0, const float* __restrict__ dg1, const int* __restrict__ n_t, int B, int T,
                                                    int H, int Hp, float* __restrict__ db_ih0, float* __restrict__ db_hh0, float* __restrict__ db_ih1,
                                                    float* __restrict__ db_hh1) {
    __shared__ float part[8][32];
    const int per = 4 * Hp / 32, layer = (int)blockIdx.x >= per;
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5, col = ((int)blockIdx.x - layer * per) * 32 + c;
    const float* dG = layer ? dg1 : dg0;
    const size_t ld = 4 * (size_t)Hp;
    float sum = 0.f;
    for (int t = 0; t < T; ++t) {
        const int nr = n_t[t];
        if (nr == 0) break;
        const float* p = dG + (size_t)t * B * ld + col;
#pragma unroll 4
        for (int row = g; row < nr; row += 8) sum += p[(size_t)row * ld];
    }
    part[g][c] = sum;
    __syncthreads();
    if (g != 0) return;
    float s = part[0][c];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += part[k][c];
    const int blk = col / Hp, u = col - blk * Hp;
    if (u >= H) return;
    (layer ? db_ih1 : db_ih0)[blk * H + u] = s;
    (layer ? db_hh1 : db_hh0)[blk * H + u] = s;
}

// tok[t][row] = the word id of the valid pair (t, row < n_t[t]) when it is inside [0, V1), else -1
__global__ __launch_bounds__(256) void k_lstm_tok(const int* __restrict__ wids, int B, int T, int V1, const int* __restrict__ perm,
                                                  const int* __restrict__ n_t, int* __restrict__ tok) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= B * T) return;
    const int t = p / B, row = p - t * B;
    int v = -1;
    if (row < n_t[t]) {
        const int w = wids[(size_t)perm[row] * T + t];
        if (w >= 0 && w < V1) v = w;
    }
    tok[p] = v;
}

// dE[v] = (sum of dX over the valid pairs whose word id is v, in (t, row) order) (1 - tanh(E[v])^2); dE[0] = 0 (padding_idx: torch's
// embedding backward skips it, whatever read E[0] in the forward).  One workgroup per row of E: it scans tok 256 positions at a time (one
// ballot per wave) and adds the rows it finds.
__global__ __launch_bounds__(256) void k_lstm_de(const int* __restrict__ tok, const float* __restrict__ dX, const float* __restrict__ E, int npos, int de,
                                                 float* __restrict__ dE) {
    __shared__ unsigned long long found[4];
    const int v = blockIdx.x, tid = threadIdx.x;
    for (int c0 = 0; c0 < de; c0 += 1024) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (v != 0) {
            for (int p0 = 0; p0 < npos; p0 += 256) {
                const bool hit = p0 + tid < npos && tok[p0 + tid] == v;
                const unsigned long long m = __ballot(hit);
                if ((tid & 63) == 0) found[tid >> 6] = m;
                __syncthreads();
                for (int w = 0; w < 4; ++w) {
                    unsigned long long mm = found[w];
                    while (mm) {
                        const int b = __ffsll((long long)mm) - 1;
                        mm &= mm - 1;
                        const float* src = dX + (size_t)(p0 + 64 * w + b) * de;
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const int c = c0 + tid + 256 * k; if (c < de) acc[k] += src[c]; }
                    }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + tid + 256 * k;
            if (c >= de) continue;
            float out = 0.f;
            if (v != 0) { const float th = tanhf(E[(size_t)v * de + c]); out = acc[k] * (1.f - th * th); }
            dE[(size_t)v * de + c] = out;
        }
    }
}

extern "C" {
struct Lstm2TrainLayout { size_t perm, lens, lens_tmp, n_t, tok, h[2], c[2], gates[2], dg[2], dcf[2], dx, total; };

static Lstm2TrainLayout lstm2_train_layout(int B, int T, int emb, int H) {
    Lstm2TrainLayout w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t pairs = (size_t)B * T, Hp = pad_to(H, GEMM_BK);
    w.perm = take((size_t)B * 4); w.lens = take((size_t)B * 4); w.lens_tmp = take((size_t)B * 4); w.n_t = take(LSTM_MAX_T * 4);
    w.tok = take(pairs * 4);
    for (int l = 0; l < 2; ++l) {
        w.h[l] = take(pairs * H * 4); w.c[l] = take(pairs * H * 4);
        w.gates[l] = take(pairs * 4 * Hp * 4); w.dg[l] = take(pairs * 4 * Hp * 4);
        w.dcf[l] = take((size_t)B * H * 4);
    }
    w.dx = take(pairs * emb * 4);
    w.total = off;
    return w;
}

static bool lstm2_train_dims_ok(long long B, long long T, long long emb, long long H) {
    if (!lstm2_dims_ok(B, T, emb, H)) return false;
    if (H >= (1 << 19) || emb >= (1 << 19)) return false;                                      // the pack launch's grid.y
    const long long Hp = pad_to((int)H, GEMM_BK), wide = H > emb ? H : emb;
    if (8 * Hp >= (1ll << 30)) return false;                                                   // k extents and column offsets are ints
    if (2 * cdiv(B, LB_BM) * cdiv(wide, LB_BN) >= (1ll << 28)) return false;                   // sweep (two layers) / dX grids
    return cdiv(4 * Hp, LW_BM) * cdiv(wide, LW_BN) < (1ll << 28);                              // weight-gradient grids
}

size_t ncx_lstm2_packed_t_bytes(int32_t emb, int32_t H) {
    if (!lstm2_train_dims_ok(1, 1, emb, H)) return 0;
    return lstm_pack_t(emb, H).floats * 4;
}

size_t ncx_lstm2_train_workspace_bytes(int32_t B, int32_t T, int32_t emb, int32_t H) {
    if (!lstm2_train_dims_ok(B, T, emb, H)) return 0;
    return lstm2_train_layout(B, T, emb, H).total;
}

int ncx_lstm2_pack_t(const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1, int32_t emb, int32_t H, float* packed_t,
                     void* stream) {
    if (!w_ih0 || !w_hh0 || !w_ih1 || !w_hh1 || !packed_t || ((uintptr_t)packed_t & 15) || !lstm2_train_dims_ok(1, 1, emb, H)) return -1;
    const LstmPackT p = lstm_pack_t(emb, H);
    hipLaunchKernelGGL(k_lstm_pack_t, dim3((unsigned)(8 * p.Hp / 32), (unsigned)((2 * p.rows_h + p.rows_x) / 32)), dim3(256), 0, (hipStream_t)stream,
                       w_ih0, w_hh0, w_ih1, w_hh1, emb, H, packed_t);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

int ncx_lstm2_train_forward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                            void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    if (!wids || !E || !packed || !workspace || !q_out || !bad_id_flag) return -1;
    if (!lstm2_train_dims_ok(B, T, emb, H) || V1 < 1 || ((uintptr_t)packed & 15)) return -1;
    const Lstm2TrainLayout w = lstm2_train_layout(B, T, emb, H);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return -1;
    char* ws = (char*)workspace;
    const Lstm2Plan plan{(int*)(ws + w.perm), (int*)(ws + w.lens), (int*)(ws + w.lens_tmp), (int*)(ws + w.n_t)};
    const LstmKeep<true> keep{(float*)(ws + w.h[0]), (float*)(ws + w.h[1]), (float*)(ws + w.c[0]), (float*)(ws + w.c[1]),
                              (float*)(ws + w.gates[0]), (float*)(ws + w.gates[1]), B, pad_to(H, GEMM_BK)};
    return lstm2_forward_keep(wids, B, T, E, V1, emb, H, packed, plan, keep, q_out, bad_id_flag, (hipStream_t)stream);
}

int ncx_lstm2_train_backward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed_t,
                             void* workspace, size_t workspace_bytes, const float* dq_out, float* dW_ih0, float* dW_hh0, float* db_ih0,
                             float* db_hh0, float* dW_ih1, float* dW_hh1, float* db_ih1, float* db_hh1, float* dE, void* stream) {
    if (!wids || !E || !packed_t || !workspace || !dq_out || !dW_ih0 || !dW_hh0 || !db_ih0 || !db_hh0 || !dW_ih1 || !dW_hh1 || !db_ih1 || !db_hh1)
        return -1;
    if (!lstm2_train_dims_ok(B, T, emb, H) || V1 < 1 || ((uintptr_t)packed_t & 15)) return -1;
    const Lstm2TrainLayout w = lstm2_train_layout(B, T, emb, H);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return -1;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const LstmPackT pk = lstm_pack_t(emb, H);
    const int* n_t = (const int*)(ws + w.n_t);
    int* tok = (int*)(ws + w.tok);
    const float* hst[2] = {(const float*)(ws + w.h[0]), (const float*)(ws + w.h[1])};

    LbArgs a{};
    a.g0 = (const float*)(ws + w.gates[0]); a.g1 = (const float*)(ws + w.gates[1]);
    a.c0 = (const float*)(ws + w.c[0]); a.c1 = (const float*)(ws + w.c[1]);
    a.dg0 = (float*)(ws + w.dg[0]); a.dg1 = (float*)(ws + w.dg[1]); a.dcf0 = (float*)(ws + w.dcf[0]); a.dcf1 = (float*)(ws + w.dcf[1]);
    a.w0 = packed_t; a.w1 = packed_t + pk.off1; a.wx = packed_t + pk.offx;
    a.perm = (const int*)(ws + w.perm); a.lens = (const int*)(ws + w.lens); a.n_t = n_t; a.dq_out = dq_out; a.dX = (float*)(ws + w.dx);
    a.B = B; a.T = T; a.H = H; a.Hp = pk.Hp; a.emb = emb; a.tiles_m = (int)cdiv(B, LB_BM); a.grid1 = a.tiles_m * (int)cdiv(H, LB_BN);
    for (int u = T - 1; u >= -1; --u) {        // every launch is issued: how many rows it has is known on the device only
        const int layers = (u >= 0) + (u + 1 < T);
        hipLaunchKernelGGL(k_lstm_bgemm<false>, dim3((unsigned)(layers * a.grid1)), dim3(256), 0, s, a, u, u >= 0 ? 1 : 0);
        NCX_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_lstm_tok, dim3((unsigned)cdiv((long long)B * T, 256)), dim3(256), 0, s, wids, B, T, V1, a.perm, n_t, tok);
    NCX_HIP_TRY(hipGetLastError());
    if (dE) {
        hipLaunchKernelGGL(k_lstm_bgemm<true>, dim3((unsigned)(a.tiles_m * cdiv(emb, LB_BN)), (unsigned)T), dim3(256), 0, s, a, 0, 0);
        NCX_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_lstm_de, dim3((unsigned)V1), dim3(256), 0, s, tok, a.dX, E, B * T, emb, dE);
        NCX_HIP_TRY(hipGetLastError());
    }
    LwArgs d{};
    d.tok = tok; d.n_t = n_t; d.B = B; d.T = T; d.H = H; d.Hp = pk.Hp; d.tiles_m = (int)cdiv(4 * pk.Hp, LW_BM);
    const unsigned grid_h = (unsigned)(d.tiles_m * cdiv(H, LW_BN));
    d.dG = a.dg0; d.X = hst[0]; d.out = dW_hh0; d.cols = H; d.xshift = 1;
    hipLaunchKernelGGL(k_lstm_dw<false>, dim3(grid_h), dim3(256), 0, s, d);
    NCX_HIP_TRY(hipGetLastError());
    d.dG = a.dg1; d.X = hst[0]; d.out = dW_ih1; d.xshift = 0;
    hipLaunchKernelGGL(k_lstm_dw<false>, dim3(grid_h), dim3(256), 0, s, d);
    NCX_HIP_TRY(hipGetLastError());
    d.X = hst[1]; d.out = dW_hh1; d.xshift = 1;
    hipLaunchKernelGGL(k_lstm_dw<false>, dim3(grid_h), dim3(256), 0, s, d);
    NCX_HIP_TRY(hipGetLastError());
    d.dG = a.dg0; d.X = E; d.out = dW_ih0; d.cols = emb; d.xshift = 0;
    hipLaunchKernelGGL(k_lstm_dw<true>, dim3((unsigned)(d.tiles_m * cdiv(emb, LW_BN))), dim3(256), 0, s, d);
    NCX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_lstm_dbias, dim3((unsigned)(2 * 4 * pk.Hp / 32)), dim3(256), 0, s, a.dg0, a.dg1, n_t, B, T, H, pk.Hp, db_ih0, db_hh0,
                       db_ih1, db_hh1);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
}  // extern "C"
