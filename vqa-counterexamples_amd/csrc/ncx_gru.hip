// ncx_gru.hip -- the frozen question encoder (GRUEncoder in eval mode: embedding -> one-layer GRU -> last valid step):
// ncx_gru_packed_bytes, ncx_gru_pack, ncx_gru_workspace_bytes, ncx_gru_encode[_flags], ncx_gru_step_form.  Forward only.  The step kernel here is
// the fp32 one; under NCX_F_X6 the entries launch its bf16 x 6 form instead (ncx_gru_x6.hip).
//
// Reference: vqa/models/seq2vec.py -- process_lengths + select_last (11-25: the length of a right-padded question and the hidden
// state of its last word) and factory (79-97: the GRU 620 -> 2400 encoder the VQA model is built with).  Semantics, gate order r, z, n
// as torch.nn.GRU:
//   len_b = max(1, #{t : wids[b, t] != 0});  x_t = E[wids[b, t]]  (row 0 is read like any other row)
//   r = s(W_ir x + b_ir + W_hr h + b_hr);  z = s(W_iz x + b_iz + W_hz h + b_hz);  n = tanh(W_in x + b_in + r (W_hn h + b_hn))
//   h' = (1 - z) n + z h,  h_0 = 0;  q[b] = h after step len_b - 1
// Plan (T + 1 launches, nothing read back, no inter-workgroup wait, no atomics):
//   k_rnn_plan  (ncx_rnn.hip, shared with the LSTM encoder; an all-padding row has length 1) one workgroup: id range check, len_b, a
//               stable counting sort of the rows by length (descending) -> perm, and n_t = #{b : len_b > t}: the active rows of step t
//               are the prefix [0, n_t) of the sorted order.
//   k_gru_step  once per time step t, always launched; it reads n_t from memory and workgroups beyond it exit.  One launch is the
//               GEMM  [x_t | h_{t-1}][0:n_t) . [W_ih | W_hh]^T  (K = dim_emb + dim_q; step 0 stops after the x columns: h_0 = 0) on
//               v_mfma_f32_16x16x4_f32, the rows of E gathered by word id on the load side, so the input projection is computed
//               for the valid (row, t) pairs only and Gx / Gh never exist in memory.  A workgroup owns 64 rows x 32 hidden units
//               with the r, z and n weight rows of THOSE units side by side (the packed layout), keeps W_in x and W_hn h in separate
//               accumulators, and its epilogue does the gate arithmetic from registers, writes h_t (double buffered) and
//               q[perm[row]] when t == len_row - 1.
#include "ncx_gru.h"

using namespace ncx;

namespace {
constexpr int GRU_P = GEMM_BK + 4;   // LDS pitch of a 32-deep k-step (conflict-free ds_read_b64 fragments, ncx_gemm.h)
constexpr int GRU_TILE_ROWS = RNN_BM + 3 * RNN_BU;
}  // namespace

// packed = W [nj][3 gates][32 units][kp] | bias [nj][6: ir iz in hr hz hn][32 units]; row (j, g, u) = W_i{g}[32 j + u, :] zero-padded to
// whole k-steps, then W_h{g}[32 j + u, :] zero-padded likewise; units beyond dim_q are zero rows
__global__ __launch_bounds__(256) void k_gru_pack(const float* __restrict__ w_ih, const float* __restrict__ w_hh, const float* __restrict__ b_ih,
                                                  const float* __restrict__ b_hh, int dim_emb, int dim_q, float* __restrict__ packed) {
    const GruPacked p = gru_packed(dim_emb, dim_q);
    const size_t i = (size_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.floats) return;
    float v = 0.f;
    if (i < p.w_floats) {
        const size_t row = i / p.kp;
        const int c = (int)(i - row * p.kp);
        const int u = (int)(row % RNN_BU), g = (int)(row / RNN_BU % 3), unit = (int)(row / (3 * RNN_BU)) * RNN_BU + u;
        if (unit < dim_q) {
            if (c < p.kx) { if (c < dim_emb) v = w_ih[((size_t)g * dim_q + unit) * dim_emb + c]; }
            else if (c - p.kx < dim_q) v = w_hh[((size_t)g * dim_q + unit) * dim_q + (c - p.kx)];
        }
    } else {
        const size_t b = i - p.w_floats;
        const int u = (int)(b % RNN_BU), g = (int)(b / RNN_BU % 6), unit = (int)(b / (6 * RNN_BU)) * RNN_BU + u;
        if (unit < dim_q) v = g < 3 ? b_ih[(size_t)g * dim_q + unit] : b_hh[(size_t)(g - 3) * dim_q + unit];
    }
    packed[i] = v;
}

// KEEP (the training forward, ncx_gru_train.hip): the same step; the epilogue also leaves r, z, n and hn = W_hn h + b_hn of every valid
// (row, t) pair in the stash, and the host hands it h_{t-1} / h_t of the [T][B] stash instead of the two alternating buffers.
template <bool KEEP>
__global__ __launch_bounds__(256) void k_gru_step(const int* __restrict__ wids, int T, int t, const float* __restrict__ E, int V1, int dim_emb, int dim_q,
                                                  const float* __restrict__ packed, const int* __restrict__ perm, const int* __restrict__ lens,
                                                  const int* __restrict__ n_t, const float* __restrict__ h_prev, float* __restrict__ h_next,
                                                  float* __restrict__ q, int tiles_m, int total, GruKeep<KEEP> keep) {
    __shared__ __attribute__((aligned(16))) float lds[2][GRU_TILE_ROWS * GRU_P];
    // workgroup ids are dealt round-robin over the 8 XCDs: consecutive work items (the row tiles of one unit tile, which share its
    // weight rows) go to the same XCD's L2
    const int w = rnn_work_item(blockIdx.x, total);
    if (w >= total) return;
    const int nt = n_t[t];
    const int j = w / tiles_m, m0 = (w - j * tiles_m) * RNN_BM;
    if (m0 >= nt) return;                      // (uniform: before any barrier)

    const GruPacked pk = gru_packed(dim_emb, dim_q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wu = wave & 1;   // wave tile: rows 32 wr .. + 32, units 16 wu .. + 16
    const int c4 = 4 * (tid & 7), lr = tid >> 3;

    // loader: thread owns column quad c4 of tile rows lr + 32 i (2 of the A tile, 3 of the weight tile)
    const float* xptr[2]; const float* hptr[2]; const float* bptr[3];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = min(m0 + lr + 32 * i, nt - 1);                       // rows beyond n_t: clamped here, never stored
        int wid = wids[(size_t)perm[row] * T + t];
        wid = min(max(wid, 0), V1 - 1);                                      // an id out of range is never an address (k_rnn_plan flags it)
        xptr[i] = E + (size_t)wid * dim_emb;
        hptr[i] = h_prev + (size_t)row * dim_q;
    }
#pragma unroll
    for (int i = 0; i < 3; ++i) bptr[i] = packed + ((size_t)j * 3 * RNN_BU + lr + 32 * i) * pk.kp + c4;
    const int nx = pk.kx / GEMM_BK, ns = nx + (t > 0 ? (pk.kp - pk.kx) / GEMM_BK : 0);

    f32x4 va[2], vb[3];
    auto issue = [&](int s) __attribute__((always_inline)) {
        const bool ish = s >= nx;
        const int k = (ish ? s - nx : s) * GEMM_BK + c4, cols = ish ? dim_q : dim_emb;
        if (k - c4 + GEMM_BK <= cols) {
#pragma unroll
            for (int i = 0; i < 2; ++i) va[i] = *(const f32x4u*)((ish ? hptr[i] : xptr[i]) + k);
        } else {                               // the ragged last k-step of a segment: guarded, zero filled
#pragma unroll
            for (int i = 0; i < 2; ++i) va[i] = load4(ish ? hptr[i] : xptr[i], k, cols);
        }
#pragma unroll
        for (int i = 0; i < 3; ++i) vb[i] = *(const f32x4*)(bptr[i] + s * GEMM_BK);
    };
    auto store = [&](int buf) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(lr + 32 * i) * GRU_P + c4]) = va[i];
#pragma unroll
        for (int i = 0; i < 3; ++i) *(f32x4*)(&lds[buf][(RNN_BM + lr + 32 * i) * GRU_P + c4]) = vb[i];
    };

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc_r[2] = {zero, zero}, acc_z[2] = {zero, zero}, acc_nx[2] = {zero, zero}, acc_nh[2] = {zero, zero};
    // MFMA (tt, e) takes k = 8 tt + 2 lk + e from lane group lk for both operands (ncx_gemm.h)
    auto compute = [&](int buf, bool ish) __attribute__((always_inline)) {
        const float* pa = &lds[buf][(32 * wr + li) * GRU_P + 2 * lk];
        const float* pb = &lds[buf][(RNN_BM + 16 * wu + li) * GRU_P + 2 * lk];
#pragma unroll
        for (int tt = 0; tt < GEMM_BK / 8; ++tt) {
            const f32x2 a0 = *(const f32x2*)(pa + 8 * tt), a1 = *(const f32x2*)(pa + 16 * GRU_P + 8 * tt);
            const f32x2 br = *(const f32x2*)(pb + 8 * tt), bz = *(const f32x2*)(pb + RNN_BU * GRU_P + 8 * tt),
                        bn = *(const f32x2*)(pb + 2 * RNN_BU * GRU_P + 8 * tt);
#pragma unroll
            for (int e = 0; e < 2; ++e) {
                acc_r[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], br[e], acc_r[0], 0, 0, 0);
                acc_r[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], br[e], acc_r[1], 0, 0, 0);
                acc_z[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], bz[e], acc_z[0], 0, 0, 0);
                acc_z[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], bz[e], acc_z[1], 0, 0, 0);
                if (ish) {
                    acc_nh[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], bn[e], acc_nh[0], 0, 0, 0);
                    acc_nh[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], bn[e], acc_nh[1], 0, 0, 0);
                } else {
                    acc_nx[0] = __builtin_amdgcn_mfma_f32_16x16x4f32(a0[e], bn[e], acc_nx[0], 0, 0, 0);
                    acc_nx[1] = __builtin_amdgcn_mfma_f32_16x16x4f32(a1[e], bn[e], acc_nx[1], 0, 0, 0);
                }
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
        if (s < nx) compute(buf, false); else compute(buf, true);
        if (more) store(buf ^ 1);
        __syncthreads();
        buf ^= 1;
    }

    // epilogue: C layout col = lane & 15 (unit), row = 4 (lane >> 4) + reg
    const int ul = 16 * wu + li, unit = j * RNN_BU + ul;
    if (unit >= dim_q) return;
    const GruBias bias = gru_bias(packed, pk, j, ul);
#pragma unroll
    for (int i = 0; i < 2; ++i)
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int row = m0 + 32 * wr + 16 * i + 4 * lk + e;
            if (row >= nt) continue;
            gru_gate_store<KEEP>(acc_r[i][e], acc_z[i][e], acc_nx[i][e], acc_nh[i][e], bias, t, row, unit, dim_q, h_prev, h_next, q, perm, lens, keep);
        }
}

namespace ncx {
// ncx_gru_encode_flags's plan and T step launches with the KEEP instantiation: h_t goes to hstash [T][B][dim_q], the gates to `gates`
int gru_forward_keep(const int32_t* wids, int B, int T, const float* E, int V1, int dim_emb, int dim_q, const float* packed, const RnnPlan& p,
                     float* hstash, float* gates, float* q_out, int32_t* bad_id_flag, uint32_t flags, hipStream_t s) {
    NCX_HIP_TRY(rnn_plan(wids, B, T, V1, p, 1, bad_id_flag, s));
    if (flags & NCX_F_X6) return gru_steps_x6(wids, B, T, E, V1, dim_emb, dim_q, packed, p, hstash, nullptr, gates, q_out, s);
    const int tiles_m = (int)cdiv(B, RNN_BM), total = tiles_m * (int)cdiv(dim_q, RNN_BU);
    const unsigned grid = (unsigned)(8 * cdiv(total, 8));
    const GruKeep<true> keep{gates, B, pad_to(dim_q, GEMM_BK)};
    const size_t hs = (size_t)B * dim_q;
    for (int t = 0; t < T; ++t) {
        hipLaunchKernelGGL(k_gru_step<true>, dim3(grid), dim3(256), 0, s, wids, T, t, E, V1, dim_emb, dim_q, packed, p.perm, p.lens, p.n_t,
                           t > 0 ? hstash + (t - 1) * hs : hstash, hstash + t * hs, q_out, tiles_m, total, keep);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}
}  // namespace ncx

extern "C" {
struct GruLayout { RnnPlanOff plan; size_t h0, h1, total; };

static GruLayout gru_layout(int B, int dim_q) {
    GruLayout w{};
    WsCarver c;
    w.plan = take_plan(c, B);
    w.h0 = c.take((size_t)B * dim_q * 4); w.h1 = c.take((size_t)B * dim_q * 4);
    w.total = c.off;
    return w;
}

size_t ncx_gru_packed_bytes(int32_t dim_emb, int32_t dim_q) {
    if (!rnn_dims_ok(1, 1, dim_emb, dim_q)) return 0;
    return gru_packed(dim_emb, dim_q).floats * 4;
}

size_t ncx_gru_workspace_bytes(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q) {
    if (!rnn_dims_ok(B, T, dim_emb, dim_q)) return 0;
    return gru_layout(B, dim_q).total;
}

int ncx_gru_pack(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t dim_emb, int32_t dim_q,
                 float* packed, void* stream) {
    if (!rnn_dims_ok(1, 1, dim_emb, dim_q) || !rnn_ptrs_ok({w_ih, w_hh, b_ih, b_hh}, packed)) return -1;
    const size_t n = gru_packed(dim_emb, dim_q).floats;
    hipLaunchKernelGGL(k_gru_pack, dim3((unsigned)cdiv((long long)n, 256)), dim3(256), 0, (hipStream_t)stream, w_ih, w_hh, b_ih, b_hh, dim_emb, dim_q, packed);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

int ncx_gru_step_form(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q, uint32_t flags) {
    if (!gru_flags_ok(flags) || !rnn_dims_ok(B, T, dim_emb, dim_q)) return -1;
    return (flags & NCX_F_X6) ? 1 : 0;
}

int ncx_gru_encode(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                   const float* packed, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream) {
    return ncx_gru_encode_flags(wids, B, T, E, V1, dim_emb, dim_q, packed, 0, workspace, workspace_bytes, q_out, bad_id_flag, stream);
}

int ncx_gru_encode_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                         const float* packed, uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag,
                         void* stream) {
    if (!gru_flags_ok(flags) || !rnn_dims_ok(B, T, dim_emb, dim_q) || V1 < 1) return -1;
    const GruLayout w = gru_layout(B, dim_q);
    if (!rnn_args_ok({wids, E, q_out, bad_id_flag}, packed, workspace, workspace_bytes, w.total)) return -1;
    hipStream_t s = (hipStream_t)stream;
    char* ws = (char*)workspace;
    const RnnPlan p = w.plan.at(ws);
    float* h[2] = {(float*)(ws + w.h0), (float*)(ws + w.h1)};
    NCX_HIP_TRY(rnn_plan(wids, B, T, V1, p, 1, bad_id_flag, s));
    if (flags & NCX_F_X6) return gru_steps_x6(wids, B, T, E, V1, dim_emb, dim_q, packed, p, h[0], h[1], nullptr, q_out, s);
    const int tiles_m = (int)cdiv(B, RNN_BM), total = tiles_m * (int)cdiv(dim_q, RNN_BU);
    const unsigned grid = (unsigned)(8 * cdiv(total, 8));
    for (int t = 0; t < T; ++t) {              // every step is launched: how many rows it has is known on the device only
        hipLaunchKernelGGL(k_gru_step<false>, dim3(grid), dim3(256), 0, s, wids, T, t, E, V1, dim_emb, dim_q, packed, p.perm, p.lens, p.n_t,
                           h[(t + 1) & 1], h[t & 1], q_out, tiles_m, total, GruKeep<false>{});
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}
}  // extern "C"
