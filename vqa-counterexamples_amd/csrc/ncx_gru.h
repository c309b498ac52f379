// ncx_gru.h -- what the question encoder's forward (ncx_gru.hip) shares with its training entries (ncx_gru_train.hip).
#pragma once
#include "ncx_rnn.h"

namespace ncx {

// Last argument of k_gru_step<KEEP>: nothing for ncx_gru_encode; for the training forward the gate stash
// [T][B][4: r z n hn][dqp] (sorted row order, dqp = dim_q rounded up to a whole k-step).
template <bool KEEP> struct GruKeep {};
template <> struct GruKeep<true> { float* gates; int B, dqp; };

__attribute__((visibility("hidden"))) int gru_forward_keep(const int32_t* wids, int B, int T, const float* E, int V1, int dim_emb, int dim_q,
                                                           const float* packed, const RnnPlan& p, float* hstash, float* gates, float* q_out,
                                                           int32_t* bad_id_flag, hipStream_t s);

}  // namespace ncx
