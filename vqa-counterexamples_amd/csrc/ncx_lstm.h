// ncx_lstm.h -- what the two-layer LSTM encoder's forward (ncx_lstm.hip) shares with its training entries (ncx_lstm_train.hip).
#pragma once
#include "ncx_rnn.h"

namespace ncx {

// Last argument of k_lstm_step<KEEP>: nothing for ncx_lstm2_encode; for the training forward the stash of both layers, [T][B] in the
// plan's sorted row order: h_t [H], c_t [H] and the activated gates [4: i f g o][Hp] (Hp = H rounded up to a whole k-step).
template <bool KEEP> struct LstmKeep {};
template <> struct LstmKeep<true> { float* h0; float* h1; float* c0; float* c1; float* g0; float* g1; int B, Hp; };

__attribute__((visibility("hidden"))) bool lstm2_dims_ok(long long B, long long T, long long emb, long long H);
__attribute__((visibility("hidden"))) int lstm2_forward_keep(const int32_t* wids, int B, int T, const float* E, int V1, int emb, int H, const float* packed,
                                                             const RnnPlan& p, const LstmKeep<true>& keep, float* q_out, int32_t* bad_id_flag,
                                                             hipStream_t s);

}  // namespace ncx
