// ncx_gru_train.hip -- training the question encoder (GRUEncoder: embedding -> one-layer GRU -> last valid step): the forward that keeps
// what the backward needs, and backward through time.  ncx_gru_train_workspace_bytes, ncx_gru_packed_t_bytes, ncx_gru_pack_t,
// ncx_gru_train_forward, ncx_gru_train_backward, their ..._flags forms and ncx_gru_bwd_form.
//
// Reference: vqa/models/seq2vec.py -- process_lengths + select_last (11-25) and factory (79-97); what is replaced is torch autograd
// through nn.Embedding + nn.GRU + the last-step selection.  With len_b, perm, n_t of ncx_gru.hip, for t from len_b - 1 down to 0:
//   dh_t = [t == len_b - 1] dq_out[b] + (what step t + 1 sends back)
//   dn = dh (1 - z);  dz = dh (h_{t-1} - n);  h_{-1} = 0
//   da_n = dn (1 - n^2);  da_z = dz z (1 - z);  da_r = da_n hn r (1 - r);  da_hn = da_n r          (hn = W_hn h_{t-1} + b_hn)
//   dh_{t-1} = dh z + [da_r | da_z | da_hn] . W_hh
//   dGx_t = [da_r | da_z | da_n] -> dW_ih, db_ih, dX_t = dGx_t . W_ih;   dGh_t = [da_r | da_z | da_hn] -> dW_hh (t >= 1), db_hh
// Stash (workspace, [T][B] in the plan's sorted row order): h_t [dq]; gates r | z | n | hn [4][dqp]; gate gradients
// da_r | da_z | da_n | da_hn [4][dqp] (dqp = dim_q up to a whole 32-deep k-step, pad columns zero): dGx is the first three blocks, dGh
// blocks 0, 1, 3.
// Plan (forward T + 1 launches; backward T + 6, T + 3 without dE; nothing read back, no atomics, no inter-workgroup wait):
//   k_gru_bgemm<false>  the reverse sweep, one launch per t = T .. 1, all issued: dh_{t-1} for the rows [0, n_{t-1}) -- the product
//                       dGh_t[0:n_t) . W_hh (M = n_t, N = dim_q, K = 3 dqp; launch T runs none) on v_mfma_f32_16x16x4_f32, then in the
//                       epilogue + z_t dh_t + the injected dq_out[perm[row]] where len_row == t, the gate arithmetic of step t - 1 from
//                       the stash (no transcendentals), dh_{t-1} (two alternating buffers) and the four gate-gradient blocks of t - 1.
//   k_gru_bgemm<true>   dX_t = dGx_t . W_ih for every step in one launch (grid.y = t) after the sweep; skipped when dE is NULL.
//                       Both share their 64 x 64 tile loop with the LSTM's sweep (rnn_nt_tile, ncx_rnn.h).
//   k_rnn_dw            (ncx_rnn.hip) dW_hh = sum_{t >= 1} dGh_t^T h_{t-1} (stash rows, the walk skips the da_n block),
//                       dW_ih = sum_t dGx_t^T E[wid] (gathered rows): TN products whose contraction walks (t, row < n_t[t]).
//   NCX_F_X6            (ncx_gru_train_backward_flags; ncx_gru_train_x6.hip) the four products above on the bf16 matrix path with three-plane
//                       operands: k_gru_bgemm_x6<false> / <true> for the sweep and dX, k_gru_dw_x6 for the two walks.  The launches, what
//                       they read and write and everything else in this plan stay as they are.
//   k_gru_dbias         column sums of the four blocks over the same ranges (rnn_colsum) -> db_ih, db_hh.
//   k_rnn_tok, k_rnn_de (ncx_rnn.hip) the word id of every valid pair (or -1); one workgroup per row of E sums the dX rows of its id.
#include "ncx_gru.h"

using namespace ncx;

namespace {
constexpr int BG_BM = RNN_NT_BM, BG_BN = RNN_NT_BN;                 // sweep / dX tile (rnn_nt_tile, ncx_rnn.h)

struct GruPackT { int dqp, kp, rows_h, rows_x; size_t floats; };
__host__ __device__ inline GruPackT gru_pack_t(int dim_emb, int dim_q) {
    GruPackT p;
    p.dqp = pad_to(dim_q, GEMM_BK); p.kp = 3 * p.dqp; p.rows_h = pad_to(dim_q, BG_BN); p.rows_x = pad_to(dim_emb, BG_BN);
    p.floats = (size_t)(p.rows_h + p.rows_x) * p.kp;
    return p;
}
}  // namespace

// packed_t = WhhT [rows_h][kp] | WihT [rows_x][kp]: WhhT[j][g dqp + u] = W_hh[g dim_q + u][j], WihT[c][g dqp + u] = W_ih[g dim_q + u][c],
// zero where u >= dim_q or the row does not exist (rows up to a multiple of 64).  A 32 x 32 tile per workgroup through LDS: both sides coalesced.
__global__ __launch_bounds__(256) void k_gru_pack_t(const float* __restrict__ w_ih, const float* __restrict__ w_hh, int dim_emb, int dim_q,
                                                    float* __restrict__ packed_t) {
    __shared__ float tile[32][33];
    const GruPackT p = gru_pack_t(dim_emb, dim_q);
    const int c0 = blockIdx.x * 32, row0 = blockIdx.y * 32, tx = threadIdx.x & 31, ty = threadIdx.x >> 5;
    const bool hh = row0 < p.rows_h;                     // (rows_h is a multiple of 32: a tile never straddles the two matrices)
    const float* src = hh ? w_hh : w_ih;
    const int ld = hh ? dim_q : dim_emb, sc = (hh ? row0 : row0 - p.rows_h) + tx;
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) {
        const int c = c0 + ty + 8 * rr, g = c / p.dqp, u = c - g * p.dqp;
        tile[ty + 8 * rr][tx] = (u < dim_q && sc < ld) ? src[((size_t)g * dim_q + u) * ld + sc] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int rr = 0; rr < 4; ++rr) packed_t[(size_t)(row0 + ty + 8 * rr) * p.kp + c0 + tx] = tile[tx][ty + 8 * rr];
}

typedef GruBgArgs BgArgs;      // (ncx_gru.h: shared with the X6 form of this kernel)

// rnn_nt_tile's A rows: dG_t's rows, the k-steps in order; the sweep's k-steps from s_hn on sit one block further (da_hn, after da_n)
// (the column offset is one int, uniform over the workgroup, before it meets the row pointer: the loop then keeps it in scalar registers)
struct GruBgSrc {
    const float* aptr[2]; int s_hn, skip;
    __device__ __forceinline__ const float* ptr(int s, int i) const { return aptr[i] + (s * GEMM_BK + (s >= s_hn ? skip : 0)); }
    __device__ __forceinline__ bool zero(int, int) const { return false; }   // (rows beyond n_t are clamped and never stored)
};

// DX = false: launch t of the reverse sweep (finishes step u = t - 1).  DX = true: dX_t, t = blockIdx.y.
template <bool DX>
__global__ __launch_bounds__(256) void k_gru_bgemm(const BgArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][RNN_NT_LDS];
    const int t = DX ? (int)blockIdx.y : a.t;
    const int tn = (int)blockIdx.x / a.tiles_m, m0 = ((int)blockIdx.x - tn * a.tiles_m) * BG_BM, n0 = tn * BG_BN;   // row tiles of a column tile share its weight rows
    const int nprod = t < a.T ? a.n_t[t] : 0;
    const int nout = DX ? nprod : a.n_t[t - 1];
    if (m0 >= nout) return;                    // (uniform: before any barrier)

    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wu = wave & 1;   // wave tile: rows 32 wr .. + 32, columns 32 wu .. + 32
    const int c4 = 4 * (tid & 7), lr = tid >> 3;
    const int kp = 3 * a.dqp, dg_ld = 4 * a.dqp;
    const int ns = m0 < nprod ? kp / GEMM_BK : 0;

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][2] = {{zero, zero}, {zero, zero}};
    if (ns > 0) {
        GruBgSrc src;
#pragma unroll
        for (int i = 0; i < 2; ++i) src.aptr[i] = a.dG + ((size_t)t * a.B + rnn_clamp_row(m0 + lr + 32 * i, nprod)) * dg_ld + c4;
        src.s_hn = 2 * a.dqp / GEMM_BK; src.skip = DX ? 0 : a.dqp;
        rnn_nt_tile(lds, src, a.wT + (size_t)(n0 + lr) * kp + c4, kp, 0, ns, acc);
    }

    // epilogue: C layout col = lane & 15, row = 4 (lane >> 4) + reg
    const int u = t - 1;
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int jj = 0; jj < 2; ++jj)
#pragma unroll
            for (int e = 0; e < 4; ++e) {
                const int row = m0 + 32 * wr + 16 * i + 4 * lk + e, col = n0 + 32 * wu + 16 * jj + li;
                if (row >= nout) continue;
                if (DX) {
                    if (col < a.de) a.dX[((size_t)t * a.B + row) * a.de + col] = acc[i][jj][e];
                    continue;
                }
                if (col >= a.dqp) continue;
                float* dgo = a.dG + ((size_t)u * a.B + row) * dg_ld + col;
                if (col >= a.dq) {                                               // pad columns: zero, they are k positions of later products
                    dgo[0] = 0.f; dgo[a.dqp] = 0.f; dgo[2 * a.dqp] = 0.f; dgo[3 * a.dqp] = 0.f;
                    continue;
                }
                float dh = 0.f;
                if (row < nprod) dh = acc[i][jj][e] + a.gates[((size_t)t * a.B + row) * dg_ld + a.dqp + col] * a.dh_in[(size_t)row * a.dq + col];
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

// db_ih = column sums of da_r | da_z | da_n, db_hh of da_r | da_z | da_hn over every valid pair (rnn_colsum, ncx_rnn.h).  A workgroup owns 32 columns.
__global__ __launch_bounds__(256) void k_gru_dbias(const float* __restrict__ dG, const int* __restrict__ n_t, int B, int T, int dq, int dqp,
                                                   float* __restrict__ db_ih, float* __restrict__ db_hh) {
    const int col = blockIdx.x * 32 + (threadIdx.x & 31);
    float s;
    if (!rnn_colsum(dG, 4 * (size_t)dqp, n_t, B, T, col, s)) return;
    const int blk = col / dqp, u = col - blk * dqp;
    if (u >= dq) return;
    if (blk < 2) { db_ih[blk * dq + u] = s; db_hh[blk * dq + u] = s; }
    else if (blk == 2) db_ih[2 * dq + u] = s;
    else db_hh[2 * dq + u] = s;
}

extern "C" {
struct GruTrainLayout { RnnPlanOff plan; size_t tok, h, gates, dg, dh0, dh1, dx, total; };

static GruTrainLayout gru_train_layout(int B, int T, int dim_emb, int dim_q) {
    GruTrainLayout w{};
    WsCarver c;
    const size_t pairs = (size_t)B * T, dqp = pad_to(dim_q, GEMM_BK);
    w.plan = take_plan(c, B);
    w.tok = c.take(pairs * 4);
    w.h = c.take(pairs * dim_q * 4); w.gates = c.take(pairs * 4 * dqp * 4); w.dg = c.take(pairs * 4 * dqp * 4);
    w.dh0 = c.take((size_t)B * dim_q * 4); w.dh1 = c.take((size_t)B * dim_q * 4);
    w.dx = c.take(pairs * dim_emb * 4);
    w.total = c.off;
    return w;
}

static bool gru_train_dims_ok(long long B, long long T, long long dim_emb, long long dim_q) {
    if (!rnn_dims_ok(B, T, dim_emb, dim_q)) return false;
    if (dim_q >= (1 << 19) || dim_emb >= (1 << 19)) return false;                              // the pack launch's grid.y
    const long long dqp = pad_to((int)dim_q, GEMM_BK);
    if (3 * dqp >= (1ll << 30)) return false;                                                  // k extents and column offsets are ints
    if (cdiv(B, BG_BM) * cdiv(dim_q > dim_emb ? dim_q : dim_emb, BG_BN) >= (1ll << 28)) return false;   // sweep / dX grids
    return cdiv(3 * dqp, RNN_DW_BM) * cdiv(dim_q > dim_emb ? dim_q : dim_emb, RNN_DW_BN) < (1ll << 28);        // weight-gradient grids
}

size_t ncx_gru_packed_t_bytes(int32_t dim_emb, int32_t dim_q) {
    if (!gru_train_dims_ok(1, 1, dim_emb, dim_q)) return 0;
    return gru_pack_t(dim_emb, dim_q).floats * 4;
}

size_t ncx_gru_train_workspace_bytes(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q) {
    if (!gru_train_dims_ok(B, T, dim_emb, dim_q)) return 0;
    return gru_train_layout(B, T, dim_emb, dim_q).total;
}

int ncx_gru_pack_t(const float* w_ih, const float* w_hh, int32_t dim_emb, int32_t dim_q, float* packed_t, void* stream) {
    if (!gru_train_dims_ok(1, 1, dim_emb, dim_q) || !rnn_ptrs_ok({w_ih, w_hh}, packed_t)) return -1;
    const GruPackT p = gru_pack_t(dim_emb, dim_q);
    hipLaunchKernelGGL(k_gru_pack_t, dim3((unsigned)(p.kp / 32), (unsigned)((p.rows_h + p.rows_x) / 32)), dim3(256), 0, (hipStream_t)stream,
                       w_ih, w_hh, dim_emb, dim_q, packed_t);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

int ncx_gru_train_forward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                          const float* packed, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    return ncx_gru_train_forward_flags(wids, B, T, E, V1, dim_emb, dim_q, packed, 0, workspace, workspace_bytes, q_out, bad_id_flag, stream);
}

int ncx_gru_train_forward_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                                const float* packed, uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag,
                                void* stream) {
    if (!gru_flags_ok(flags) || !gru_train_dims_ok(B, T, dim_emb, dim_q) || V1 < 1) return -1;
    const GruTrainLayout w = gru_train_layout(B, T, dim_emb, dim_q);
    if (!rnn_args_ok({wids, E, q_out, bad_id_flag}, packed, workspace, workspace_bytes, w.total)) return -1;
    char* ws = (char*)workspace;
    return gru_forward_keep(wids, B, T, E, V1, dim_emb, dim_q, packed, w.plan.at(ws), (float*)(ws + w.h), (float*)(ws + w.gates), q_out, bad_id_flag,
                            flags, (hipStream_t)stream);
}

int ncx_gru_train_backward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                           const float* packed_t, void* workspace, size_t workspace_bytes, const float* dq_out,
                           float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, float* dE, void* stream) {
    return ncx_gru_train_backward_flags(wids, B, T, E, V1, dim_emb, dim_q, packed_t, 0, workspace, workspace_bytes, dq_out, dW_ih, dW_hh, db_ih, db_hh,
                                        dE, stream);
}

int ncx_gru_bwd_form(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q, uint32_t flags) {
    if (!gru_flags_ok(flags) || !gru_train_dims_ok(B, T, dim_emb, dim_q)) return -1;
    return (flags & NCX_F_X6) ? GRU_BWD_X6 : 0;
}

int ncx_gru_train_backward_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                                 const float* packed_t, uint32_t flags, void* workspace, size_t workspace_bytes, const float* dq_out,
                                 float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, float* dE, void* stream) {
    if (!gru_flags_ok(flags) || !gru_train_dims_ok(B, T, dim_emb, dim_q) || V1 < 1) return -1;
    const int form = (flags & NCX_F_X6) ? GRU_BWD_X6 : 0;
    const GruTrainLayout w = gru_train_layout(B, T, dim_emb, dim_q);
    if (!rnn_args_ok({wids, E, dq_out, dW_ih, dW_hh, db_ih, db_hh}, packed_t, workspace, workspace_bytes, w.total)) return -1;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const GruPackT pk = gru_pack_t(dim_emb, dim_q);
    const RnnPlan plan = w.plan.at(ws);
    const int* n_t = plan.n_t;
    int* tok = (int*)(ws + w.tok);
    float* dh[2] = {(float*)(ws + w.dh0), (float*)(ws + w.dh1)};

    BgArgs a{};
    a.gates = (const float*)(ws + w.gates); a.hstash = (const float*)(ws + w.h); a.wT = packed_t;
    a.perm = plan.perm; a.lens = plan.lens; a.n_t = n_t; a.dq_out = dq_out;
    a.dG = (float*)(ws + w.dg); a.dX = (float*)(ws + w.dx);
    a.B = B; a.T = T; a.dq = dim_q; a.dqp = pk.dqp; a.de = dim_emb; a.tiles_m = (int)cdiv(B, BG_BM);
    const unsigned grid_h = (unsigned)(a.tiles_m * cdiv(dim_q, BG_BN));
    for (int t = T; t >= 1; --t) {             // every launch is issued: how many rows it has is known on the device only
        a.t = t; a.dh_in = dh[t & 1]; a.dh_out = dh[(t + 1) & 1];
        if (form & GRU_BWD_SWEEP) {
            NCX_HIP_TRY(gru_sweep_x6(a, s));
            continue;
        }
        hipLaunchKernelGGL(k_gru_bgemm<false>, dim3(grid_h), dim3(256), 0, s, a);
        NCX_HIP_TRY(hipGetLastError());
    }
    NCX_HIP_TRY(rnn_tok(wids, B, T, V1, a.perm, n_t, tok, s));
    if (dE) {
        a.wT = packed_t + (size_t)pk.rows_h * pk.kp; a.t = 0;
        if (form & GRU_BWD_DX) {
            NCX_HIP_TRY(gru_dx_x6(a, s));
        } else {
            hipLaunchKernelGGL(k_gru_bgemm<true>, dim3((unsigned)(a.tiles_m * cdiv(dim_emb, BG_BN)), (unsigned)T), dim3(256), 0, s, a);
            NCX_HIP_TRY(hipGetLastError());
        }
        NCX_HIP_TRY(rnn_embed_grad(tok, a.dX, nullptr, B, T, V1, dim_emb, dE, s));
    }
    RnnDwArgs d{};
    d.dG = a.dG; d.tok = tok; d.n_t = n_t; d.B = B; d.T = T; d.ld = 4 * pk.dqp; d.kp = pk.kp; d.units = dim_q; d.unitsp = pk.dqp;
    d.X = a.hstash; d.out = dW_hh; d.cols = dim_q; d.xshift = 1; d.skip_from = 2 * pk.dqp; d.skip_by = pk.dqp;     // blocks r z hn
    NCX_HIP_TRY((form & GRU_BWD_DWHH) ? gru_dw_x6(d, false, s) : rnn_dw(d, false, false, s));
    d.X = E; d.out = dW_ih; d.cols = dim_emb; d.xshift = 0; d.skip_from = 0; d.skip_by = 0;                         // blocks r z n
    NCX_HIP_TRY((form & GRU_BWD_DWIH) ? gru_dw_x6(d, true, s) : rnn_dw(d, true, false, s));
    hipLaunchKernelGGL(k_gru_dbias, dim3((unsigned)(4 * pk.dqp / 32)), dim3(256), 0, s, a.dG, n_t, B, T, dim_q, pk.dqp, db_ih, db_hh);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
}  // extern "C"
