// ncx_lstm.h -- what the two-layer LSTM encoder's forward (ncx_lstm.hip) shares with its bf16 x 6 step kernel (ncx_lstm_x6.hip) and its
// training entries (ncx_lstm_train.hip).
#pragma once
#include "ncx_rnn.h"

namespace ncx {

// Last argument of k_lstm_step<KEEP>: nothing for ncx_lstm2_encode; for the training forward the stash of both layers, [T][B] in the
// plan's sorted row order: h_t [H], c_t [H] and the activated gates [4: i f g o][Hp] (Hp = H rounded up to a whole k-step).
template <bool KEEP> struct LstmKeep {};
template <> struct LstmKeep<true> { float* h0; float* h1; float* c0; float* c1; float* g0; float* g1; int B, Hp; };

// The argument block of a wavefront launch, either form of the step kernel.  tiles_m / total / grid1 belong to the form's row tile.
struct LstmStep {
    const int* wids; const float* E; const float* packed; const int* perm; const int* lens; const int* n_t;
    float* h[2][2];      // [layer][t & 1]: h_t of the rows [0, n_t), sorted row order, [B][H]
    float* c[2];         // [layer]: the cell state, [B][H], updated in place
    float* q;            // [B][2 H], input row order
    int T, V1, emb, H, tiles_m, total, grid1;
};

#if defined(__HIPCC__)
// One (row, unit) element of a step's epilogue, shared by both forms of the step kernel: the cell arithmetic from the four accumulators,
// c_t (in place, or to the stash: cprev / cnext are the caller's), h_t, q[perm[row], layer H + unit] at the row's last step and, with
// KEEP, the gate stash.
struct LstmBias { float i, f, g, o; };
__device__ __forceinline__ LstmBias lstm_bias(const float* __restrict__ bias) { return {bias[0], bias[RNN_BU], bias[2 * RNN_BU], bias[3 * RNN_BU]}; }
template <bool KEEP>
__device__ __forceinline__ void lstm_cell_store(float a_i, float a_f, float a_g, float a_o, const LstmBias& b, int t, int layer, int row, int unit, int H,
                                                const float* cprev, float* cnext, float* h_next, float* __restrict__ q,
                                                const int* __restrict__ perm, const int* __restrict__ lens, const LstmKeep<KEEP>& keep) {
    const size_t at = (size_t)row * H + unit;
    const float gi = 1.f / (1.f + expf(-(a_i + b.i)));
    const float gf = 1.f / (1.f + expf(-(a_f + b.f)));
    const float gg = tanhf(a_g + b.g);
    const float go = 1.f / (1.f + expf(-(a_o + b.o)));
    const float cp = t > 0 ? cprev[at] : 0.f;                            // step 0 never reads the workspace
    const float cn = gf * cp + gi * gg;
    const float hn = go * tanhf(cn);
    cnext[at] = cn;
    h_next[at] = hn;
    if (t == lens[row] - 1) q[(size_t)perm[row] * (2 * (size_t)H) + (size_t)layer * H + unit] = hn;
    if constexpr (KEEP) {
        float* g = (layer ? keep.g1 : keep.g0) + ((size_t)t * keep.B + row) * (4 * (size_t)keep.Hp) + unit;
        g[0] = gi; g[keep.Hp] = gf; g[2 * keep.Hp] = gg; g[3 * keep.Hp] = go;
    }
}
#endif

// the flags of the ..._flags entry points: 0 or NCX_F_X6
inline bool lstm2_flags_ok(uint32_t flags) { return flags == 0 || flags == NCX_F_X6; }

__attribute__((visibility("hidden"))) bool lstm2_dims_ok(long long B, long long T, long long emb, long long H);
// The T + 1 wavefront launches of the bf16 x 6 form (ncx_lstm_x6.hip) after rnn_plan.  `a` as lstm2_step_args left it (the tile fields are
// set here); keep == NULL: ncx_lstm2_encode_flags's, h and c in a.h / a.c; otherwise the training forward's, into the stash.
__attribute__((visibility("hidden"))) int lstm2_steps_x6(int B, int T, LstmStep a, const LstmKeep<true>* keep, hipStream_t s);
__attribute__((visibility("hidden"))) int lstm2_forward_keep(const int32_t* wids, int B, int T, const float* E, int V1, int emb, int H, const float* packed,
                                                             const RnnPlan& p, const LstmKeep<true>& keep, float* q_out, int32_t* bad_id_flag,
                                                             uint32_t flags, hipStream_t s);

}  // namespace ncx
