// ncx_lstm.hip -- the two-layer LSTM question encoder (TwoLSTM in eval mode: tanh(embedding) -> LSTM -> LSTM -> both layers' hidden
// state at the last valid step, side by side): ncx_lstm2_packed_bytes, ncx_lstm2_pack, ncx_lstm2_workspace_bytes, ncx_lstm2_encode[_flags],
// ncx_lstm2_step_form.  The training forward (ncx_lstm_train.hip) is the same step kernel with KEEP = true.  The step kernel here is the
// fp32 one; under NCX_F_X6 the entries launch its bf16 x 6 form instead (ncx_lstm_x6.hip).
//
// Reference: vqa/models/seq2vec.py -- process_lengths + select_last (11-25), TwoLSTM (48-76), factory's `2-lstm` branch (86-89).
// Semantics, gate order i, f, g, o as torch.nn.LSTM, the recurrence over TIME (batch_first; DESIGN 5n on why not as written):
//   len_b = #{t : wids[b, t] != 0}, and T when that is 0 (select_last's index -1);  x_t = tanh(E[wids[b, t]])  (row 0 is read like any row)
//   layer l:  [i f g o] = W_ih x + b_ih + W_hh h + b_hh;  c' = s(f) c + s(i) tanh(g);  h' = s(o) tanh(c');  h_0 = c_0 = 0;  layer 1's x is layer 0's h'
//   q[b] = [h^0 | h^1] after step len_b - 1
// Plan (T + 2 launches, nothing read back, no inter-workgroup wait, no atomics):
//   k_rnn_plan   (ncx_rnn.hip, shared with the GRU encoder) one workgroup: the length rule above (an all-padding row has length T), the
//                rows sorted by length (descending) -> perm, n_t = #{b : len_b > t}.
//   k_lstm_step  launch s in [0, T]: layer 0 at step s (s < T) and layer 1 at step s - 1 (s >= 1) as two ranges of workgroup ids -- a
//                wavefront: both read only what launch s - 1 wrote.  A layer's step is the GEMM [x_t | h_{t-1}][0:n_t) . [W_ih | W_hh]^T on
//                v_mfma_f32_16x16x4_f32 (step 0 stops after the x columns: h_0 = 0).  A workgroup owns 64 rows x 32 hidden units with the
//                i, f, g, o weight rows of THOSE units side by side; one accumulator per gate (x and h share it); the epilogue does the cell
//                arithmetic from registers, updates c in place, writes h_t (double buffered) and q[perm[row]] when t == len_row - 1.
//                Layer 0 gathers E[wid] on the load side and takes tanh on the way from registers to LDS.
#include "ncx_lstm.h"

using namespace ncx;

namespace {
// LDS rows are one 32-deep k-step with no padding; the 16-byte quad q of tile row r sits at quad q ^ ((r >> 1) & 7).  A 32-lane half
// of a ds_read_b64 fragment read (16 rows, one logical quad, two 8-byte halves) then covers all 64 banks once, as the padded pitch
// of 36 (ncx_gru.hip) does, and the two buffers take 48 KB instead of 54: three workgroups fit a CU's LDS, not two.
constexpr int LSTM_P = GEMM_BK;
constexpr int LSTM_TILE_ROWS = RNN_BM + 4 * RNN_BU;

// packed = layer 0 | layer 1;  layer l = W [nj][4 gates][32 units][kp_l] | bias [nj][4][32 units] (b_ih + b_hh)
struct LstmPacked { int kx[2], kp[2], nj; size_t w_floats[2], off[2], floats; };
__host__ __device__ inline LstmPacked lstm_packed(int emb, int H) {
    LstmPacked p;
    p.nj = (H + RNN_BU - 1) / RNN_BU;
    size_t off = 0;
    for (int l = 0; l < 2; ++l) {
        p.kx[l] = pad_to(l ? H : emb, GEMM_BK); p.kp[l] = p.kx[l] + pad_to(H, GEMM_BK);
        p.w_floats[l] = (size_t)p.nj * 4 * RNN_BU * p.kp[l];
        p.off[l] = off; off += p.w_floats[l] + (size_t)p.nj * 4 * RNN_BU;
    }
    p.floats = off;
    return p;
}

struct LstmW { const float* w_ih; const float* w_hh; const float* b_ih; const float* b_hh; };
}  // namespace

// row (j, g, u) of layer l = W_ih^l[g H + 32 j + u, :] zero-padded to whole k-steps, then W_hh^l[g H + 32 j + u, :] likewise; units beyond H
// are zero rows
__global__ __launch_bounds__(256) void k_lstm_pack(LstmW w0, LstmW w1, int emb, int H, float* __restrict__ packed) {
    const LstmPacked p = lstm_packed(emb, H);
    size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.floats) return;
    const int l = i >= p.off[1];
    const LstmW w = l ? w1 : w0;
    const int in = l ? H : emb, kx = p.kx[l], kp = p.kp[l];
    const size_t o = i - p.off[l];
    float v = 0.f;
    if (o < p.w_floats[l]) {
        const size_t row = o / kp;
        const int c = (int)(o - row * kp);
        const int u = (int)(row % RNN_BU), g = (int)(row / RNN_BU % 4), unit = (int)(row / (4 * RNN_BU)) * RNN_BU + u;
        if (unit < H) {
            if (c < kx) { if (c < in) v = w.w_ih[((size_t)g * H + unit) * in + c]; }
            else if (c - kx < H) v = w.w_hh[((size_t)g * H + unit) * H + (c - kx)];
        }
    } else {
        const size_t b = o - p.w_floats[l];
        const int u = (int)(b % RNN_BU), g = (int)(b / RNN_BU % 4), unit = (int)(b / (4 * RNN_BU)) * RNN_BU + u;
        if (unit < H) v = w.b_ih[(size_t)g * H + unit] + w.b_hh[(size_t)g * H + unit];
    }
    packed[i] = v;
}

// grid = (layers of this launch) x grid1; workgroups [0, grid1) run layer `layer_base`, [grid1, 2 grid1) layer 1
// KEEP (the training forward, ncx_lstm_train.hip): the same step; h_{t-1} / c_{t-1} are read from and h_t / c_t written to the [T][B]
// stash instead of the alternating buffers, and the epilogue also leaves the four activated gates of every valid (row, t) pair there.
template <bool KEEP>
__global__ __launch_bounds__(256) void k_lstm_step(LstmStep a, int s, int layer_base, LstmKeep<KEEP> keep) {
    __shared__ __attribute__((aligned(16))) float lds[2][LSTM_TILE_ROWS * LSTM_P];
    const int second = (int)blockIdx.x >= a.grid1;
    const int layer = layer_base + second, bid = (int)blockIdx.x - second * a.grid1;
    const int t = s - layer;
    // workgroup ids are dealt round-robin over the 8 XCDs (grid1 is a multiple of 8): the row tiles of one unit tile, which share its
    // weight rows, go to the same XCD's L2
    const int w = rnn_work_item(bid, a.total);
    if (w >= a.total) return;
    const int nt = a.n_t[t];
    const int j = w / a.tiles_m, m0 = (w - j * a.tiles_m) * RNN_BM;
    if (m0 >= nt) return;                      // (uniform: before any barrier)

    const int H = a.H, in = layer ? H : a.emb;
    // (the two layers' entries of lstm_packed by selects: a runtime index into that struct would cost a private copy of it)
    const int kx = pad_to(in, GEMM_BK), kp = kx + pad_to(H, GEMM_BK);
    const size_t blk = (size_t)((H + RNN_BU - 1) / RNN_BU) * 4 * RNN_BU;                // weight rows of a layer = floats of its bias block
    const size_t w_floats = blk * kp;
    const float* packed = a.packed + (layer ? blk * (pad_to(a.emb, GEMM_BK) + pad_to(H, GEMM_BK)) + blk : 0);
    // (selects, not indexing: a runtime index into the argument struct would cost a private copy of it)
    float* const hl0 = layer ? a.h[1][0] : a.h[0][0];
    float* const hl1 = layer ? a.h[1][1] : a.h[0][1];
    const float* h_prev = (t & 1) ? hl0 : hl1;
    float* h_next = (t & 1) ? hl1 : hl0;
    if constexpr (KEEP) {
        const size_t hs = (size_t)keep.B * a.H;
        float* const hst = layer ? keep.h1 : keep.h0;
        h_prev = hst + (size_t)(t > 0 ? t - 1 : 0) * hs; h_next = hst + (size_t)t * hs;
    }
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wu = wave & 1;   // wave tile: rows 32 wr .. + 32, units 16 wu .. + 16
    const int c4 = 4 * (tid & 7), lr = tid >> 3;
    const int sc4 = 4 * ((tid & 7) ^ ((lr >> 1) & 7));                       // where the loader's quad goes in its LDS rows (lr + 32 i)

    // loader: thread owns column quad c4 of tile rows lr + 32 i (2 of the A tile, 4 of the weight tile)
    const float* xptr[2]; const float* hptr[2]; const float* bptr[4];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = min(m0 + lr + 32 * i, nt - 1);                       // rows beyond n_t: clamped here, never stored
        if (layer == 0) {
            int wid = a.wids[(size_t)a.perm[row] * a.T + t];
            wid = min(max(wid, 0), a.V1 - 1);                                // an id out of range is never an address (k_rnn_plan flags it)
            xptr[i] = a.E + (size_t)wid * a.emb;
        } else {
            if constexpr (KEEP) xptr[i] = keep.h0 + ((size_t)t * keep.B + row) * H;
            else xptr[i] = ((t & 1) ? a.h[0][1] : a.h[0][0]) + (size_t)row * H;                  // layer 0's h_t, written by the previous launch
        }
        hptr[i] = h_prev + (size_t)row * H;
    }
#pragma unroll
    for (int i = 0; i < 4; ++i) bptr[i] = packed + ((size_t)j * 4 * RNN_BU + lr + 32 * i) * kp + c4;
    const int nx = kx / GEMM_BK, ns = nx + (t > 0 ? (kp - kx) / GEMM_BK : 0);

    f32x4 va[2], vb[4];
    auto issue = [&](int ks) __attribute__((always_inline)) {
        const bool ish = ks >= nx;
        const int k = (ish ? ks - nx : ks) * GEMM_BK + c4, cols = ish ? H : in;
        if (k - c4 + GEMM_BK <= cols) {
#pragma unroll
            for (int i = 0; i < 2; ++i) va[i] = *(const f32x4u*)((ish ? hptr[i] : xptr[i]) + k);
        } else {                               // the ragged last k-step of a segment: guarded, zero filled
#pragma unroll
            for (int i = 0; i < 2; ++i) va[i] = load4(ish ? hptr[i] : xptr[i], k, cols);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) vb[i] = *(const f32x4*)(bptr[i] + ks * GEMM_BK);
    };
    auto store = [&](int buf, int ks) __attribute__((always_inline)) {
        if (layer == 0 && ks < nx) {           // x = tanh(E[wid]); tanh(0) = 0 keeps the zero fill
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) va[i][e] = tanhf(va[i][e]);
        }
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(lr + 32 * i) * LSTM_P + sc4]) = va[i];
#pragma unroll
        for (int i = 0; i < 4; ++i) *(f32x4*)(&lds[buf][(RNN_BM + lr + 32 * i) * LSTM_P + sc4]) = vb[i];
    };

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4][2] = {{zero, zero}, {zero, zero}, {zero, zero}, {zero, zero}};     // [gate i f g o][row half]
    // MFMA (tt, e) takes k = 8 tt + 2 lk + e from lane group lk for both operands (ncx_gemm.h): logical quad 2 tt + (lk >> 1) of a
    // fragment row, whose swizzle key is (li >> 1) & 7 (every fragment starts at a multiple of 16 rows)
    int co[GEMM_BK / 8];
#pragma unroll
    for (int tt = 0; tt < GEMM_BK / 8; ++tt) co[tt] = 4 * ((2 * tt + (lk >> 1)) ^ ((li >> 1) & 7)) + ((2 * lk) & 3);
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const float* pa = &lds[buf][(32 * wr + li) * LSTM_P];
        const float* pb = &lds[buf][(RNN_BM + 16 * wu + li) * LSTM_P];
#pragma unroll
        for (int tt = 0; tt < GEMM_BK / 8; ++tt) {
            const f32x2 a0 = *(const f32x2*)(pa + co[tt]), a1 = *(const f32x2*)(pa + 16 * LSTM_P + co[tt]);
            f32x2 b[4];
#pragma unroll
            for (int g = 0; g < 4; ++g) b[g] = *(const f32x2*)(pb + g * RNN_BU * LSTM_P + co[tt]);
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int g = 0; g < 4; ++g) {
                    acc[g][0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], b[g][e], acc[g][0], 0, 0, 0);
                    acc[g][1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], b[g][e], acc[g][1], 0, 0, 0);
                }
        }
    };

    // register-staged double-buffered LDS, one barrier per k-step: the loads of step ks + 1 fly over the MFMAs of step ks
    issue(0); store(0, 0);
    __syncthreads();
    int buf = 0;
    for (int ks = 0; ks < ns; ++ks) {
        const bool more = ks + 1 < ns;
        if (more) issue(ks + 1);
        compute(buf);
        if (more) store(buf ^ 1, ks + 1);
        __syncthreads();
        buf ^= 1;
    }

    // epilogue: C layout col = lane & 15 (unit), row = 4 (lane >> 4) + reg
    const int ul = 16 * wu + li, unit = j * RNN_BU + ul;
    if (unit >= H) return;
    const LstmBias bias = lstm_bias(packed + w_floats + (size_t)j * 4 * RNN_BU + ul);
    float* cbuf = layer ? a.c[1] : a.c[0];
    const float* cprev = cbuf;
    if constexpr (KEEP) {
        const size_t hs = (size_t)keep.B * H;
        float* const cst = layer ? keep.c1 : keep.c0;
        cprev = cst + (size_t)(t > 0 ? t - 1 : 0) * hs; cbuf = cst + (size_t)t * hs;
    }
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = m0 + 32 * wr + 16 * i + 4 * lk + e;
            if (row >= nt) continue;
            lstm_cell_store<KEEP>(acc[0][i][e], acc[1][i][e], acc[2][i][e], acc[3][i][e], bias, t, layer, row, unit, H, cprev, cbuf, h_next, a.q, a.perm,
                                  a.lens, keep);
        }
}

namespace ncx {
bool lstm2_dims_ok(long long B, long long T, long long emb, long long H) {
    // rnn_dims_ok bounds B T, the widths and one layer's grid; the launch holds two layers
    return rnn_dims_ok(B, T, emb, H) && 2 * 8 * cdiv(cdiv(B, RNN_BM) * cdiv(H, RNN_BU), 8) < (1ll << 30);
}

static LstmStep lstm2_step_args(const int32_t* wids, int B, int T, const float* E, int V1, int emb, int H, const float* packed, const RnnPlan& p,
                                float* q_out) {
    LstmStep a{};
    a.wids = wids; a.E = E; a.packed = packed; a.perm = p.perm; a.lens = p.lens; a.n_t = p.n_t;
    a.q = q_out; a.T = T; a.V1 = V1; a.emb = emb; a.H = H;
    a.tiles_m = (int)cdiv(B, RNN_BM); a.total = a.tiles_m * (int)cdiv(H, RNN_BU); a.grid1 = (int)(8 * cdiv(a.total, 8));
    return a;
}

// the plan and the T + 1 wavefront launches; KEEP: into the stash
template <bool KEEP>
static int lstm2_run(const int32_t* wids, int B, int T, int V1, const RnnPlan& p, const LstmStep& a, const LstmKeep<KEEP>& keep, int32_t* bad_id_flag,
                     uint32_t flags, hipStream_t st) {
    NCX_HIP_TRY(rnn_plan(wids, B, T, V1, p, T, bad_id_flag, st));
    if (flags & NCX_F_X6) {
        if constexpr (KEEP) return lstm2_steps_x6(B, T, a, &keep, st);
        else return lstm2_steps_x6(B, T, a, nullptr, st);
    }
    for (int s = 0; s <= T; ++s) {             // every launch is issued: how many rows a step has is known on the device only
        const int layers = (s < T) + (s >= 1);
        hipLaunchKernelGGL(k_lstm_step<KEEP>, dim3((unsigned)(layers * a.grid1)), dim3(256), 0, st, a, s, s < T ? 0 : 1, keep);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}

int lstm2_forward_keep(const int32_t* wids, int B, int T, const float* E, int V1, int emb, int H, const float* packed, const RnnPlan& p,
                       const LstmKeep<true>& keep, float* q_out, int32_t* bad_id_flag, uint32_t flags, hipStream_t s) {
    return lstm2_run<true>(wids, B, T, V1, p, lstm2_step_args(wids, B, T, E, V1, emb, H, packed, p, q_out), keep, bad_id_flag, flags, s);
}
}  // namespace ncx

extern "C" {
struct Lstm2Layout { RnnPlanOff plan; size_t h[2][2], c[2], total; };

static Lstm2Layout lstm2_layout(int B, int H) {
    Lstm2Layout w{};
    WsCarver c;
    w.plan = take_plan(c, B);
    for (int l = 0; l < 2; ++l) {
        w.h[l][0] = c.take((size_t)B * H * 4); w.h[l][1] = c.take((size_t)B * H * 4); w.c[l] = c.take((size_t)B * H * 4);
    }
    w.total = c.off;
    return w;
}

size_t ncx_lstm2_packed_bytes(int32_t emb, int32_t H) {
    if (!lstm2_dims_ok(1, 1, emb, H)) return 0;
    return lstm_packed(emb, H).floats * 4;
}

size_t ncx_lstm2_workspace_bytes(int32_t B, int32_t T, int32_t emb, int32_t H) {
    if (!lstm2_dims_ok(B, T, emb, H)) return 0;
    return lstm2_layout(B, H).total;
}

int ncx_lstm2_pack(const float* w_ih0, const float* w_hh0, const float* b_ih0, const float* b_hh0, const float* w_ih1, const float* w_hh1,
                   const float* b_ih1, const float* b_hh1, int32_t emb, int32_t H, float* packed, void* stream) {
    if (!lstm2_dims_ok(1, 1, emb, H) || !rnn_ptrs_ok({w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1}, packed)) return -1;
    const size_t n = lstm_packed(emb, H).floats;
    if (cdiv((long long)n, 256) >= (1ll << 31)) return -1;
    hipLaunchKernelGGL(k_lstm_pack, dim3((unsigned)cdiv((long long)n, 256)), dim3(256), 0, (hipStream_t)stream, LstmW{w_ih0, w_hh0, b_ih0, b_hh0},
                       LstmW{w_ih1, w_hh1, b_ih1, b_hh1}, emb, H, packed);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

int ncx_lstm2_step_form(int32_t B, int32_t T, int32_t emb, int32_t H, uint32_t flags) {
    if (!lstm2_flags_ok(flags) || !lstm2_dims_ok(B, T, emb, H)) return -1;
    return (flags & NCX_F_X6) ? 1 : 0;
}

int ncx_lstm2_encode(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                     void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    return ncx_lstm2_encode_flags(wids, B, T, E, V1, emb, H, packed, 0, workspace, workspace_bytes, q_out, bad_id_flag, stream);
}

int ncx_lstm2_encode_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                           uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    if (!lstm2_flags_ok(flags) || !lstm2_dims_ok(B, T, emb, H) || V1 < 1) return -1;
    const Lstm2Layout w = lstm2_layout(B, H);
    if (!rnn_args_ok({wids, E, q_out, bad_id_flag}, packed, workspace, workspace_bytes, w.total)) return -1;
    char* ws = (char*)workspace;
    const RnnPlan p = w.plan.at(ws);
    LstmStep a = lstm2_step_args(wids, B, T, E, V1, emb, H, packed, p, q_out);
    for (int l = 0; l < 2; ++l) { a.h[l][0] = (float*)(ws + w.h[l][0]); a.h[l][1] = (float*)(ws + w.h[l][1]); a.c[l] = (float*)(ws + w.c[l]); }
    return lstm2_run<false>(wids, B, T, V1, p, a, LstmKeep<false>{}, bad_id_flag, flags, (hipStream_t)stream);
}
}  // extern "C"
