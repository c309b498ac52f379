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
//                        Both share their 64 x 64 tile loop with the GRU's sweep (rnn_nt_tile, ncx_rnn.h).
//   k_rnn_dw             (ncx_rnn.hip) the four weight gradients as TN products whose contraction walks (t, row < n_t[t]); three over stash
//                        rows, dW_ih^0 over the gathered rows x = tanh(E[tok]), taken on the load side.
//   k_lstm_dbias         column sums of da^l (rnn_colsum) -> db_ih^l and db_hh^l.
//   k_rnn_tok, k_rnn_de  (ncx_rnn.hip) the word id of every valid pair (or -1); one workgroup per row of E sums the dX rows of its id in
//                        (t, row) order, times 1 - tanh(E)^2.
#include "ncx_lstm.h"

using namespace ncx;

namespace {
constexpr int LB_BM = RNN_NT_BM, LB_BN = RNN_NT_BN;                   // sweep / dX tile (rnn_nt_tile, ncx_rnn.h)

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

// rnn_nt_tile's A rows: the k-steps [0, ka) are the first segment, whose rows [n_{t+1}, n_t) count as zeros, the rest the second
struct LstmBgSrc {
    const float* pa1[2]; const float* pa2[2]; bool ok1[2]; int ka;
    __device__ __forceinline__ const float* ptr(int s, int i) const { return s < ka ? pa1[i] + s * GEMM_BK : pa2[i] + (s - ka) * GEMM_BK; }
    __device__ __forceinline__ bool zero(int s, int i) const { return s < ka && !ok1[i]; }
};

// DX = false: launch u of the reverse wavefront; workgroups [0, grid1) run layer `layer_base`, [grid1, 2 grid1) layer 0.
// DX = true: dX_t, t = blockIdx.y.
template <bool DX>
__global__ __launch_bounds__(256) void k_lstm_bgemm(const LbArgs a, int u, int layer_base) {
    __shared__ __attribute__((aligned(16))) float lds[2][RNN_NT_LDS];
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
        LstmBgSrc src;
        const float* seg2 = DX ? a.dg0 : a.dg1;
        const float* wT = DX ? a.wx : layer ? a.w1 : a.w0;
        const int t1 = min(t + 1, a.T - 1);
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int r = m0 + lr + 32 * i;
            src.ok1[i] = r < nnext;
            src.pa1[i] = dgl + ((size_t)t1 * a.B + rnn_clamp_row(r, nnext)) * dg_ld + c4;
            src.pa2[i] = seg2 + ((size_t)t * a.B + rnn_clamp_row(r, nout)) * dg_ld + c4;
        }
        src.ka = ka;
        rnn_nt_tile(lds, src, wT + (size_t)(n0 + lr) * wld + c4, wld, s0, s1, acc);
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

// db_ih^l = db_hh^l = column sums of da^l over every valid pair (rnn_colsum, ncx_rnn.h).  grid = 2 layers x (4 Hp / 32); a workgroup owns 32 columns.
__global__ __launch_bounds__(256) void k_lstm_dbias(const float* __restrict__ dg0, const float* __restrict__ dg1, const int* __restrict__ n_t, int B, int T,
                                                    int H, int Hp, float* __restrict__ db_ih0, float* __restrict__ db_hh0, float* __restrict__ db_ih1,
                                                    float* __restrict__ db_hh1) {
    const int per = 4 * Hp / 32, layer = (int)blockIdx.x >= per;
    const int col = ((int)blockIdx.x - layer * per) * 32 + (threadIdx.x & 31);
    float s;
    if (!rnn_colsum(layer ? dg1 : dg0, 4 * (size_t)Hp, n_t, B, T, col, s)) return;
    const int blk = col / Hp, u = col - blk * Hp;
    if (u >= H) return;
    (layer ? db_ih1 : db_ih0)[blk * H + u] = s;
    (layer ? db_hh1 : db_hh0)[blk * H + u] = s;
}

extern "C" {
struct Lstm2TrainLayout { RnnPlanOff plan; size_t tok, h[2], c[2], gates[2], dg[2], dcf[2], dx, total; };

static Lstm2TrainLayout lstm2_train_layout(int B, int T, int emb, int H) {
    Lstm2TrainLayout w{};
    WsCarver c;
    const size_t pairs = (size_t)B * T, Hp = pad_to(H, GEMM_BK);
    w.plan = take_plan(c, B);
    w.tok = c.take(pairs * 4);
    for (int l = 0; l < 2; ++l) {
        w.h[l] = c.take(pairs * H * 4); w.c[l] = c.take(pairs * H * 4);
        w.gates[l] = c.take(pairs * 4 * Hp * 4); w.dg[l] = c.take(pairs * 4 * Hp * 4);
        w.dcf[l] = c.take((size_t)B * H * 4);
    }
    w.dx = c.take(pairs * emb * 4);
    w.total = c.off;
    return w;
}

static bool lstm2_train_dims_ok(long long B, long long T, long long emb, long long H) {
    if (!lstm2_dims_ok(B, T, emb, H)) return false;
    if (H >= (1 << 19) || emb >= (1 << 19)) return false;                                      // the pack launch's grid.y
    const long long Hp = pad_to((int)H, GEMM_BK), wide = H > emb ? H : emb;
    if (8 * Hp >= (1ll << 30)) return false;                                                   // k extents and column offsets are ints
    if (2 * cdiv(B, LB_BM) * cdiv(wide, LB_BN) >= (1ll << 28)) return false;                   // sweep (two layers) / dX grids
    return cdiv(4 * Hp, RNN_DW_BM) * cdiv(wide, RNN_DW_BN) < (1ll << 28);                              // weight-gradient grids
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
    if (!lstm2_train_dims_ok(1, 1, emb, H) || !rnn_ptrs_ok({w_ih0, w_hh0, w_ih1, w_hh1}, packed_t)) return -1;
    const LstmPackT p = lstm_pack_t(emb, H);
    hipLaunchKernelGGL(k_lstm_pack_t, dim3((unsigned)(8 * p.Hp / 32), (unsigned)((2 * p.rows_h + p.rows_x) / 32)), dim3(256), 0, (hipStream_t)stream,
                       w_ih0, w_hh0, w_ih1, w_hh1, emb, H, packed_t);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

int ncx_lstm2_train_forward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                            void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    return ncx_lstm2_train_forward_flags(wids, B, T, E, V1, emb, H, packed, 0, workspace, workspace_bytes, q_out, bad_id_flag, stream);
}

int ncx_lstm2_train_forward_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                                  uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    if (!lstm2_flags_ok(flags) || !lstm2_train_dims_ok(B, T, emb, H) || V1 < 1) return -1;
    const Lstm2TrainLayout w = lstm2_train_layout(B, T, emb, H);
    if (!rnn_args_ok({wids, E, q_out, bad_id_flag}, packed, workspace, workspace_bytes, w.total)) return -1;
    char* ws = (char*)workspace;
    const LstmKeep<true> keep{(float*)(ws + w.h[0]), (float*)(ws + w.h[1]), (float*)(ws + w.c[0]), (float*)(ws + w.c[1]),
                              (float*)(ws + w.gates[0]), (float*)(ws + w.gates[1]), B, pad_to(H, GEMM_BK)};
    return lstm2_forward_keep(wids, B, T, E, V1, emb, H, packed, w.plan.at(ws), keep, q_out, bad_id_flag, flags, (hipStream_t)stream);
}

int ncx_lstm2_train_backward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed_t,
                             void* workspace, size_t workspace_bytes, const float* dq_out, float* dW_ih0, float* dW_hh0, float* db_ih0,
                             float* db_hh0, float* dW_ih1, float* dW_hh1, float* db_ih1, float* db_hh1, float* dE, void* stream) {
    if (!lstm2_train_dims_ok(B, T, emb, H) || V1 < 1) return -1;
    const Lstm2TrainLayout w = lstm2_train_layout(B, T, emb, H);
    if (!rnn_args_ok({wids, E, dq_out, dW_ih0, dW_hh0, db_ih0, db_hh0, dW_ih1, dW_hh1, db_ih1, db_hh1}, packed_t, workspace, workspace_bytes, w.total))
        return -1;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const LstmPackT pk = lstm_pack_t(emb, H);
    const RnnPlan plan = w.plan.at(ws);
    const int* n_t = plan.n_t;
    int* tok = (int*)(ws + w.tok);
    const float* hst[2] = {(const float*)(ws + w.h[0]), (const float*)(ws + w.h[1])};

    LbArgs a{};
    a.g0 = (const float*)(ws + w.gates[0]); a.g1 = (const float*)(ws + w.gates[1]);
    a.c0 = (const float*)(ws + w.c[0]); a.c1 = (const float*)(ws + w.c[1]);
    a.dg0 = (float*)(ws + w.dg[0]); a.dg1 = (float*)(ws + w.dg[1]); a.dcf0 = (float*)(ws + w.dcf[0]); a.dcf1 = (float*)(ws + w.dcf[1]);
    a.w0 = packed_t; a.w1 = packed_t + pk.off1; a.wx = packed_t + pk.offx;
    a.perm = plan.perm; a.lens = plan.lens; a.n_t = n_t; a.dq_out = dq_out; a.dX = (float*)(ws + w.dx);
    a.B = B; a.T = T; a.H = H; a.Hp = pk.Hp; a.emb = emb; a.tiles_m = (int)cdiv(B, LB_BM); a.grid1 = a.tiles_m * (int)cdiv(H, LB_BN);
    for (int u = T - 1; u >= -1; --u) {        // every launch is issued: how many rows it has is known on the device only
        const int layers = (u >= 0) + (u + 1 < T);
        hipLaunchKernelGGL(k_lstm_bgemm<false>, dim3((unsigned)(layers * a.grid1)), dim3(256), 0, s, a, u, u >= 0 ? 1 : 0);
        NCX_HIP_TRY(hipGetLastError());
    }
    NCX_HIP_TRY(rnn_tok(wids, B, T, V1, a.perm, n_t, tok, s));
    if (dE) {
        hipLaunchKernelGGL(k_lstm_bgemm<true>, dim3((unsigned)(a.tiles_m * cdiv(emb, LB_BN)), (unsigned)T), dim3(256), 0, s, a, 0, 0);
        NCX_HIP_TRY(hipGetLastError());
        NCX_HIP_TRY(rnn_embed_grad(tok, a.dX, E, B, T, V1, emb, dE, s));
    }
    RnnDwArgs d{};
    d.tok = tok; d.n_t = n_t; d.B = B; d.T = T; d.ld = d.kp = 4 * pk.Hp; d.units = H; d.unitsp = pk.Hp;      // (kp is a multiple of 128: whole gate-row tiles)
    d.dG = a.dg0; d.X = hst[0]; d.out = dW_hh0; d.cols = H; d.xshift = 1;
    NCX_HIP_TRY(rnn_dw(d, false, false, s));
    d.dG = a.dg1; d.X = hst[0]; d.out = dW_ih1; d.xshift = 0;
    NCX_HIP_TRY(rnn_dw(d, false, false, s));
    d.X = hst[1]; d.out = dW_hh1; d.xshift = 1;
    NCX_HIP_TRY(rnn_dw(d, false, false, s));
    d.dG = a.dg0; d.X = E; d.out = dW_ih0; d.cols = emb; d.xshift = 0;
    NCX_HIP_TRY(rnn_dw(d, true, true, s));                                     // x = tanh(E[tok])
    hipLaunchKernelGGL(k_lstm_dbias, dim3((unsigned)(2 * 4 * pk.Hp / 32)), dim3(256), 0, s, a.dg0, a.dg1, n_t, B, T, H, pk.Hp, db_ih0, db_hh0,
                       db_ih1, db_hh1);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
}  // extern "C"
