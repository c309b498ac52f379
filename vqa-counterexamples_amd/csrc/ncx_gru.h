// ncx_gru.h -- what the question encoder's forward (ncx_gru.hip) shares with its bf16 x 6 step kernel (ncx_gru_x6.hip) and its training
// entries (ncx_gru_train.hip).
#pragma once
#include "ncx_rnn.h"

namespace ncx {

// Last argument of k_gru_step<KEEP>: nothing for ncx_gru_encode; for the training forward the gate stash
// [T][B][4: r z n hn][dqp] (sorted row order, dqp = dim_q rounded up to a whole k-step).
template <bool KEEP> struct GruKeep {};
template <> struct GruKeep<true> { float* gates; int B, dqp; };

// The packed layout of ncx_gru_pack: kx / kp the k extents of the x segment / of a whole weight row, nj the 32-unit blocks
struct GruPacked { int kx, kp, nj; size_t w_floats, floats; };
__host__ __device__ inline GruPacked gru_packed(int dim_emb, int dim_q) {
    GruPacked p;
    p.kx = pad_to(dim_emb, GEMM_BK); p.kp = p.kx + pad_to(dim_q, GEMM_BK); p.nj = (dim_q + RNN_BU - 1) / RNN_BU;
    p.w_floats = (size_t)p.nj * 3 * RNN_BU * p.kp;
    p.floats = p.w_floats + (size_t)p.nj * 6 * RNN_BU;
    return p;
}

#if defined(__HIPCC__)
// One (row, unit) element of a step's epilogue, shared by both forms of the step kernel: the gate arithmetic from the four accumulators
// (a_nx = W_in x and a_nh = W_hn h apart), h_t, q[perm[row]] at the row's last step and, with KEEP, the gate stash.
struct GruBias { float ir, iz, in, hr, hz, hn; };
__device__ __forceinline__ GruBias gru_bias(const float* __restrict__ packed, const GruPacked& pk, int j, int ul) {
    const float* bias = packed + pk.w_floats + (size_t)j * 6 * RNN_BU + ul;
    return {bias[0], bias[RNN_BU], bias[2 * RNN_BU], bias[3 * RNN_BU], bias[4 * RNN_BU], bias[5 * RNN_BU]};
}
template <bool KEEP>
__device__ __forceinline__ void gru_gate_store(float a_r, float a_z, float a_nx, float a_nh, const GruBias& b, int t, int row, int unit, int dim_q,
                                               const float* __restrict__ h_prev, float* __restrict__ h_next, float* __restrict__ q,
                                               const int* __restrict__ perm, const int* __restrict__ lens, const GruKeep<KEEP>& keep) {
    const float r = 1.f / (1.f + expf(-(a_r + b.ir + b.hr)));
    const float z = 1.f / (1.f + expf(-(a_z + b.iz + b.hz)));
    const float n = tanhf(a_nx + b.in + r * (a_nh + b.hn));
    const float hp = t > 0 ? h_prev[(size_t)row * dim_q + unit] : 0.f;
    const float hn = (1.f - z) * n + z * hp;
    h_next[(size_t)row * dim_q + unit] = hn;
    if (t == lens[row] - 1) q[(size_t)perm[row] * dim_q + unit] = hn;
    if constexpr (KEEP) {
        float* g = keep.gates + ((size_t)t * keep.B + row) * (4 * (size_t)keep.dqp) + unit;
        g[0] = r; g[keep.dqp] = z; g[2 * keep.dqp] = n; g[3 * keep.dqp] = a_nh + b.hn;
    }
}
#endif

// the flags of the ..._flags entry points: 0 or NCX_F_X6
inline bool gru_flags_ok(uint32_t flags) { return flags == 0 || flags == NCX_F_X6; }

// The T step launches of the bf16 x 6 form (ncx_gru_x6.hip) after rnn_plan.  gates == NULL: ncx_gru_encode's, step t writes h_t to ha (t even) or hb
// (t odd) and reads the other; otherwise the training forward's, ha is the h stash [T][B][dim_q] (hb unused) and `gates` the gate stash.
__attribute__((visibility("hidden"))) int gru_steps_x6(const int32_t* wids, int B, int T, const float* E, int V1, int dim_emb, int dim_q,
                                                       const float* packed, const RnnPlan& p, float* ha, float* hb, float* gates, float* q_out,
                                                       hipStream_t s);

// The arguments of the backward's sweep / dX kernel (k_gru_bgemm, ncx_gru_train.hip) and of its X6 form (k_gru_bgemm_x6, ncx_gru_train_x6.hip)
struct GruBgArgs {
    const float* gates; const float* hstash; const float* wT;      // wT: WhhT (sweep) or WihT (dX), [rows][kp]
    const int* perm; const int* lens; const int* n_t; const float* dq_out;
    const float* dh_in; float* dh_out;                               // dh_t (read), dh_{t-1} (written)
    float* dG; float* dX;
    int B, T, t, dq, dqp, de, tiles_m;
};

// The bf16 x 6 form of rnn_dw(a, gather, false, s) (ncx_gru_train_x6.hip): the same walk in 256 x 64 output tiles
__attribute__((visibility("hidden"))) hipError_t gru_dw_x6(const RnnDwArgs& a, bool gather, hipStream_t s);
// The bf16 x 6 forms of k_gru_bgemm's launches: launch a.t of the reverse sweep; dX of all a.T steps (a.wT = WihT)
constexpr int GRU_B6_WR = 4;                     // wave rows of their tile: 32 GRU_B6_WR rows x 64 columns (ablation: DESIGN 5w)
__attribute__((visibility("hidden"))) hipError_t gru_sweep_x6(const GruBgArgs& a, hipStream_t s);
__attribute__((visibility("hidden"))) hipError_t gru_dx_x6(const GruBgArgs& a, hipStream_t s);
// Which products of the backward take an X6 kernel under NCX_F_X6 (ncx_gru_bwd_form's bits)
constexpr int GRU_BWD_SWEEP = 1, GRU_BWD_DX = 2, GRU_BWD_DWHH = 4, GRU_BWD_DWIH = 8;
constexpr int GRU_BWD_X6 = GRU_BWD_SWEEP | GRU_BWD_DX | GRU_BWD_DWHH | GRU_BWD_DWIH;

__attribute__((visibility("hidden"))) int gru_forward_keep(const int32_t* wids, int B, int T, const float* E, int V1, int dim_emb, int dim_q,
                                                           const float* packed, const RnnPlan& p, float* hstash, float* gates, float* q_out,
                                                           int32_t* bad_id_flag, uint32_t flags, hipStream_t s);

}  // namespace ncx
