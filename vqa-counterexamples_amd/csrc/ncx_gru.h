// ncx_gru.h -- what the question encoder's forward (ncx_gru.hip) shares with its training entries (ncx_gru_train.hip).
#pragma once
#include "ncx_internal.h"

namespace ncx {

constexpr int GRU_BM = 64;        // rows (questions) per workgroup
constexpr int GRU_BU = 32;        // hidden units per workgroup (x 3 gates = 96 weight rows)
constexpr int GRU_MAX_T = 64;

// Last argument of k_gru_step<KEEP>: nothing for ncx_gru_encode; for the training forward the gate stash
// [T][B][4: r z n hn][dqp] (sorted row order, dqp = dim_q rounded up to a whole k-step).
template <bool KEEP> struct GruKeep {};
template <> struct GruKeep<true> { float* gates; int B, dqp; };

struct GruPlan { int* perm; int* lens; int* lens_tmp; int* n_t; };      // k_gru_plan's outputs ([B], [B], [B] scratch, [GRU_MAX_T])

__attribute__((visibility("hidden"))) bool gru_dims_ok(long long B, long long T, long long dim_emb, long long dim_q);
__attribute__((visibility("hidden"))) int gru_forward_keep(const int32_t* wids, int B, int T, const float* E, int V1, int dim_emb, int dim_q,
                                                           const float* packed, const GruPlan& p, float* hstash, float* gates, float* q_out,
                                                           int32_t* bad_id_flag, hipStream_t s);

}  // namespace ncx
