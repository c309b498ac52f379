// ncx_gru_train.hip -- training the question encoder (GRUEncoder: embedding -> one-layer GRU -> last valid step): the forward that keeps
// what the backward needs, and backward through time.  ncx_gru_train_workspace_bytes, ncx_gru_packed_t_bytes, ncx_gru_pack_t,
// ncx_gru_train_forward, ncx_gru_train_backward.
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
//   k_gru_dw<IH>        dW_hh = sum_{t >= 1} dGh_t^T h_{t-1},  dW_ih = sum_t dGx_t^T E[wid]: TN products whose contraction walks
//                       (t, row < n_t[t]) with n_t read from memory; a step's k-range ends at n_t rounded up to the k-step (the rows
//                       beyond are zeroed on the load side).  128 x 64 output tiles, one workgroup per tile, the whole walk in order.
//   k_gru_dbias         column sums of the four blocks over the same ranges -> db_ih, db_hh.
//   k_gru_tok, k_gru_de the word id of every valid pair (or -1); one workgroup per row of E sums the dX rows of its id in (t, row) order.
#include "ncx_gru.h"

using namespace ncx;

namespace {
constexpr int BG_BM = 64, BG_BN = 64, BG_P = GEMM_BK + 4;         // sweep / dX tile; LDS pitch as in k_gru_step
constexpr int DW_BM = 128, DW_BN = 64;                              // weight-gradient tile: gate rows x feature columns
constexpr int DW_PA = pitch_rowk(DW_BM), DW_PB = pitch_rowk(DW_BN); // row-is-k pitches (ncx_gemm.h): ds_read_b128 / ds_read_b64

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

struct BgArgs {
    const float* gates; const float* hstash; const float* wT;      // wT: WhhT (sweep) or WihT (dX), [rows][kp]
    const int* perm; const int* lens; const int* n_t; const float* dq_out;
    const float* dh_in; float* dh_out;                               // dh_t (read), dh_{t-1} (written)
    float* dG; float* dX;
    int B, T, t, dq, dqp, de, tiles_m;
};

// DX = false: launch t of the reverse sweep (finishes step u = t - 1).  DX = true: dX_t, t = blockIdx.y.
template <bool DX>
__global__ __launch_bounds__(256) void k_gru_bgemm(const BgArgs a) {
    __shared__ __attribute__((aligned(16))) float lds[2][(BG_BM + BG_BN) * BG_P];
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
    const int s_hn = 2 * a.dqp / GEMM_BK;      // sweep: from this k-step on the A columns are the da_hn block (one block further)

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[2][2] = {{zero, zero}, {zero, zero}};
    if (ns > 0) {
        // loader: thread owns column quad c4 of tile rows lr + 32 i (2 of the A tile, 2 of the weight tile); every load is an aligned 16 bytes
        const float* aptr[2]; const float* bptr[2];
#pragma unroll
        for (int i = 0; i < 2; ++i) {
            const int row = min(m0 + lr + 32 * i, nprod - 1);                    // rows beyond n_t: clamped here, never stored
            aptr[i] = a.dG + ((size_t)t * a.B + row) * dg_ld + c4;
            bptr[i] = a.wT + (size_t)(n0 + lr + 32 * i) * kp + c4;              // (weight rows are padded to whole tiles)
        }
        f32x4 va[2], vb[2];
        auto issue = [&](int s) __attribute__((always_inline)) {
            const int ka = s * GEMM_BK + (!DX && s >= s_hn ? a.dqp : 0);
#pragma unroll
            for (int i = 0; i < 2; ++i) va[i] = *(const f32x4*)(aptr[i] + ka);
#pragma unroll
            for (int i = 0; i < 2; ++i) vb[i] = *(const f32x4*)(bptr[i] + s * GEMM_BK);
        };
        auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
            for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(lr + 32 * i) * BG_P + c4]) = va[i];
#pragma unroll
            for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(BG_BM + lr + 32 * i) * BG_P + c4]) = vb[i];
        };
        // MFMA (tt, e) takes k = 8 tt + 2 lk + e from lane group lk for both operands (ncx_gemm.h)
        auto compute = [&](int buf) __attribute__((always_inline)) {
            const float* pa = &lds[buf][(32 * wr + li) * BG_P + 2 * lk];
            const float* pb = &lds[buf][(BG_BM + 32 * wu + li) * BG_P + 2 * lk];
#pragma unroll
            for (int tt = 0; tt < GEMM_BK / 8; ++tt) {
                const f32x2 a0 = *(const f32x2*)(pa + 8 * tt), a1 = *(const f32x2*)(pa + 16 * BG_P + 8 * tt);
                const f32x2 b0 = *(const f32x2*)(pb + 8 * tt), b1 = *(const f32x2*)(pb + 16 * BG_P + 8 * tt);
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
        issue(0); store(0);
        __syncthreads();
        int buf = 0;
        for (int s = 0; s < ns; ++s) {
            const bool more = s + 1 < ns;
            if (more) issue(s + 1);
            compute(buf);
            if (more) store(buf ^ 1);
            __syncthreads();
            buf ^= 1;
        }
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

struct DwArgs {
    const float* dG; const float* X;           // X: hstash (dW_hh: row (t - 1, row)) or E (dW_ih: row tok[t][row])
    const int* tok; const int* n_t; float* out;
    int B, T, dq, dqp, cols, tiles_m;           // cols: width of X's rows = columns of out
};

// out[g dq + u][c] = sum over t >= t0, row < n_t[t] of dG_t[row][block(g)][u] * X(t, row)[c]; IH: blocks r z n, t0 = 0; else r z hn, t0 = 1
template <bool IH>
__global__ __launch_bounds__(256) void k_gru_dw(const DwArgs a) {
    __shared__ __attribute__((aligned(16))) float la[2][GEMM_BK * DW_PA];
    __shared__ __attribute__((aligned(16))) float lb[2][GEMM_BK * DW_PB];
    const int tn = (int)blockIdx.x / a.tiles_m, m0 = ((int)blockIdx.x - tn * a.tiles_m) * DW_BM, n0 = tn * DW_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wm0 = (wave >> 1) * (DW_BM / 2), wn0 = (wave & 1) * (DW_BN / 2);
    const int kr = tid >> 3, cq = 4 * (tid & 7);
    const int kp = 3 * a.dqp, dg_ld = 4 * a.dqp;

    // loader: thread owns k-row kr of the step, column quads cq + 32 i (4 of the gate-gradient tile, 2 of the X tile)
    int acol[4], bcol[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = min(m0 + cq + 32 * i, kp - 4);                             // columns beyond 3 dqp: clamped here, never stored
        acol[i] = m + (!IH && m >= 2 * a.dqp ? a.dqp : 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) bcol[i] = n0 + cq + 32 * i;
    const bool b_full = n0 + DW_BN <= a.cols;

    f32x4 va[4], vb[2];
    bool a_ok = false;
    auto issue = [&](int t, int r0, int nr) __attribute__((always_inline)) {
        const int krow = r0 + kr, rc = min(krow, nr - 1);
        a_ok = krow < nr;                                                         // rows n_t .. the end of the k-step: zeroed in store()
        const float* ap = a.dG + ((size_t)t * a.B + rc) * dg_ld;
        const float* bp = IH ? a.X + (size_t)max(a.tok[(size_t)t * a.B + rc], 0) * a.cols      // an id out of range is -1 here: never an address
                             : a.X + ((size_t)(t - 1) * a.B + rc) * a.cols;
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
#pragma unroll
        for (int i = 0; i < 4; ++i) *(f32x4*)(&la[buf][kr * DW_PA + cq + 32 * i]) = a_ok ? va[i] : zero;
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(&lb[buf][kr * DW_PB + cq + 32 * i]) = vb[i];
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
            for (int e = 0; e < 2; ++e) { av[e] = *(const f32x4*)(pa + (kk + e) * DW_PA); bv[e] = *(const f32x2*)(pb + (kk + e) * DW_PB); }
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e][i], bv[e][j], acc[i][j], 0, 0, 0);
        }
    };

    // the walk: steps t0 .. while n_t[t] > 0 (n_t never rises), rows in k-steps of 32; same double-buffered pipeline as above
    int t = IH ? 0 : 1, r0 = 0, nr = t < a.T ? a.n_t[t] : 0;
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
            const int m = m0 + wm0 + 4 * (4 * lk + q) + i, g = m / a.dqp, uu = m - g * a.dqp;
            if (m >= kp || uu >= a.dq) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = n0 + wn0 + 2 * li + j;
                if (c < a.cols) a.out[((size_t)g * a.dq + uu) * a.cols + c] = acc[i][j][q];
            }
        }
}

// db_ih = column sums of da_r | da_z | da_n, db_hh of da_r | da_z | da_hn over every valid pair.  A workgroup owns 32 columns; thread
// (g, c) sums rows g, g + 8, ... of every step in ascending order, the 8 partial sums are added in ascending g (k_mt_colsum's scheme).
__global__ __launch_bounds__(256) void k_gru_dbias(const float* __restrict__ dG, const int* __restrict__ n_t, int B, int T, int dq, int dqp,
                                                   float* __restrict__ db_ih, float* __restrict__ db_hh) {
    __shared__ float part[8][32];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5, col = blockIdx.x * 32 + c;
    float sum = 0.f;
    for (int t = 0; t < T; ++t) {
        const int nr = n_t[t];
        if (nr == 0) break;
        const float* p = dG + (size_t)t * B * (4 * (size_t)dqp) + col;
#pragma unroll 4
        for (int row = g; row < nr; row += 8) sum += p[(size_t)row * (4 * (size_t)dqp)];
    }
    part[g][c] = sum;
    __syncthreads();
    if (g != 0) return;
    float s = part[0][c];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += part[k][c];
    const int blk = col / dqp, u = col - blk * dqp;
    if (u >= dq) return;
    if (blk < 2) { db_ih[blk * dq + u] = s; db_hh[blk * dq + u] = s; }
    else if (blk == 2) db_ih[2 * dq + u] = s;
    else db_hh[2 * dq + u] = s;
}

// tok[t][row] = the word id of the valid pair (t, row < n_t[t]) when it is inside [0, V1), else -1
__global__ __launch_bounds__(256) void k_gru_tok(const int* __restrict__ wids, int B, int T, int V1, const int* __restrict__ perm,
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

// dE[v] = sum of dX over the valid pairs whose word id is v, in (t, row) order; dE[0] = 0 (padding_idx: torch's embedding backward skips
// it).  One workgroup per row of E: it scans tok 256 positions at a time (one ballot per wave) and adds the rows it finds.
__global__ __launch_bounds__(256) void k_gru_de(const int* __restrict__ tok, const float* __restrict__ dX, int npos, int de, float* __restrict__ dE) {
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
        for (int k = 0; k < 4; ++k) { const int c = c0 + tid + 256 * k; if (c < de) dE[(size_t)v * de + c] = acc[k]; }
    }
}

extern "C" {
struct GruTrainLayout { size_t perm, lens, lens_tmp, n_t, tok, h, gates, dg, dh0, dh1, dx, total; };

static GruTrainLayout gru_train_layout(int B, int T, int dim_emb, int dim_q) {
    GruTrainLayout w{};
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off = align_up(off + bytes, 256); return o; };
    const size_t pairs = (size_t)B * T, dqp = pad_to(dim_q, GEMM_BK);
    w.perm = take((size_t)B * 4); w.lens = take((size_t)B * 4); w.lens_tmp = take((size_t)B * 4); w.n_t = take(GRU_MAX_T * 4);
    w.tok = take(pairs * 4);
    w.h = take(pairs * dim_q * 4); w.gates = take(pairs * 4 * dqp * 4); w.dg = take(pairs * 4 * dqp * 4);
    w.dh0 = take((size_t)B * dim_q * 4); w.dh1 = take((size_t)B * dim_q * 4);
    w.dx = take(pairs * dim_emb * 4);
    w.total = off;
    return w;
}

static bool gru_train_dims_ok(long long B, long long T, long long dim_emb, long long dim_q) {
    if (!gru_dims_ok(B, T, dim_emb, dim_q)) return false;
    if (dim_q >= (1 << 19) || dim_emb >= (1 << 19)) return false;                              // the pack launch's grid.y
    const long long dqp = pad_to((int)dim_q, GEMM_BK);
    if (3 * dqp >= (1ll << 30)) return false;                                                  // k extents and column offsets are ints
    if (cdiv(B, BG_BM) * cdiv(dim_q > dim_emb ? dim_q : dim_emb, BG_BN) >= (1ll << 28)) return false;   // sweep / dX grids
    return cdiv(3 * dqp, DW_BM) * cdiv(dim_q > dim_emb ? dim_q : dim_emb, DW_BN) < (1ll << 28);        // weight-gradient grids
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
    if (!w_ih || !w_hh || !packed_t || ((uintptr_t)packed_t & 15) || !gru_train_dims_ok(1, 1, dim_emb, dim_q)) return -1;
    const GruPackT p = gru_pack_t(dim_emb, dim_q);
    hipLaunchKernelGGL(k_gru_pack_t, dim3((unsigned)(p.kp / 32), (unsigned)((p.rows_h + p.rows_x) / 32)), dim3(256), 0, (hipStream_t)stream,
                       w_ih, w_hh, dim_emb, dim_q, packed_t);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

int ncx_gru_train_forward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                          const float* packed, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    if (!wids || !E || !packed || !workspace || !q_out || !bad_id_flag) return -1;
    if (!gru_train_dims_ok(B, T, dim_emb, dim_q) || V1 < 1 || ((uintptr_t)packed & 15)) return -1;
    const GruTrainLayout w = gru_train_layout(B, T, dim_emb, dim_q);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return -1;
    char* ws = (char*)workspace;
    const GruPlan plan{(int*)(ws + w.perm), (int*)(ws + w.lens), (int*)(ws + w.lens_tmp), (int*)(ws + w.n_t)};
    return gru_forward_keep(wids, B, T, E, V1, dim_emb, dim_q, packed, plan, (float*)(ws + w.h), (float*)(ws + w.gates), q_out, bad_id_flag,
                            (hipStream_t)stream);
}

int ncx_gru_train_backward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                           const float* packed_t, void* workspace, size_t workspace_bytes, const float* dq_out,
                           float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, float* dE, void* stream) {
    if (!wids || !E || !packed_t || !workspace || !dq_out || !dW_ih || !dW_hh || !db_ih || !db_hh) return -1;
    if (!gru_train_dims_ok(B, T, dim_emb, dim_q) || V1 < 1 || ((uintptr_t)packed_t & 15)) return -1;
    const GruTrainLayout w = gru_train_layout(B, T, dim_emb, dim_q);
    if (workspace_bytes < w.total || ((uintptr_t)workspace & 255)) return -1;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const GruPackT pk = gru_pack_t(dim_emb, dim_q);
    const int* n_t = (const int*)(ws + w.n_t);
    int* tok = (int*)(ws + w.tok);
    float* dh[2] = {(float*)(ws + w.dh0), (float*)(ws + w.dh1)};

    BgArgs a{};
    a.gates = (const float*)(ws + w.gates); a.hstash = (const float*)(ws + w.h); a.wT = packed_t;
    a.perm = (const int*)(ws + w.perm); a.lens = (const int*)(ws + w.lens); a.n_t = n_t; a.dq_out = dq_out;
    a.dG = (float*)(ws + w.dg); a.dX = (float*)(ws + w.dx);
    a.B = B; a.T = T; a.dq = dim_q; a.dqp = pk.dqp; a.de = dim_emb; a.tiles_m = (int)cdiv(B, BG_BM);
    const unsigned grid_h = (unsigned)(a.tiles_m * cdiv(dim_q, BG_BN));
    for (int t = T; t >= 1; --t) {             // every launch is issued: how many rows it has is known on the device only
        a.t = t; a.dh_in = dh[t & 1]; a.dh_out = dh[(t + 1) & 1];
        hipLaunchKernelGGL(k_gru_bgemm<false>, dim3(grid_h), dim3(256), 0, s, a);
        NCX_HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_gru_tok, dim3((unsigned)cdiv((long long)B * T, 256)), dim3(256), 0, s, wids, B, T, V1, a.perm, n_t, tok);
    NCX_HIP_TRY(hipGetLastError());
    if (dE) {
        a.wT = packed_t + (size_t)pk.rows_h * pk.kp; a.t = 0;
        hipLaunchKernelGGL(k_gru_bgemm<true>, dim3((unsigned)(a.tiles_m * cdiv(dim_emb, BG_BN)), (unsigned)T), dim3(256), 0, s, a);
        NCX_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_gru_de, dim3((unsigned)V1), dim3(256), 0, s, tok, a.dX, B * T, dim_emb, dE);
        NCX_HIP_TRY(hipGetLastError());
    }
    DwArgs d{};
    d.dG = a.dG; d.tok = tok; d.n_t = n_t; d.B = B; d.T = T; d.dq = dim_q; d.dqp = pk.dqp; d.tiles_m = (int)cdiv(pk.kp, DW_BM);
    d.X = a.hstash; d.out = dW_hh; d.cols = dim_q;
    hipLaunchKernelGGL(k_gru_dw<false>, dim3((unsigned)(d.tiles_m * cdiv(dim_q, DW_BN))), dim3(256), 0, s, d);
    NCX_HIP_TRY(hipGetLastError());
    d.X = E; d.out = dW_ih; d.cols = dim_emb;
    hipLaunchKernelGGL(k_gru_dw<true>, dim3((unsigned)(d.tiles_m * cdiv(dim_emb, DW_BN))), dim3(256), 0, s, d);
    NCX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_gru_dbias, dim3((unsigned)(4 * pk.dqp / 32)), dim3(256), 0, s, a.dG, n_t, B, T, dim_q, pk.dqp, db_ih, db_hh);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
}  // extern "C"
