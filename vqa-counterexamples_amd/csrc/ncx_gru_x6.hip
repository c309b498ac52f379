// ncx_gru_x6.hip -- the bf16 x 6 (NCX_F_X6) form of the question encoder's step kernel: k_gru_step_x6 and its launches (gru_steps_x6).
// Not the default: ncx_gru_encode_flags / ncx_gru_train_forward_flags take it when their `flags` say so.
//
// Reference: vqa/models/seq2vec.py -- process_lengths + select_last (11-25) and factory (79-97), as ncx_gru.hip.  The step is k_gru_step's
// (ncx_gru.hip) line for line: one launch per time step, n_t read from memory, workgroups beyond it exit before their first barrier, rows
// of E gathered by (clamped) word id on the load side, rows beyond n_t clamped to row n_t - 1 and never stored, the ragged last k-step of
// the x and of the h segment zero filled, step 0 stops after the x columns, W_in x and W_hn h in separate accumulators, and the epilogue
// is the shared one (gru_gate_store, ncx_gru.h).  What differs is the product: the operands are cut into three bf16 planes when their tile
// is stored to LDS and six plane products per 16 x 16 x 32 block run with fp32 accumulation -- the cut, the order of the products, what
// is dropped and what is outside the contract: ncx_x6.h.
// One workgroup: 12 waves, 192 rows x the 96 weight rows (r, z, n) of one 32-unit block of the packed layout, read as ncx_gru_pack left
// them, on the LDS row tile RnnX6Tile<6, 96> (ncx_rnn.h: layout, loader, cut and store, fragment reads, the one-barrier loop in which a
// wave whose 32 rows all lie beyond n_t multiplies nothing); 138 240 bytes, one workgroup per CU.  The waves form a 6 x 2 grid, 32 rows x
// 16 units x 3 gates each (k_gru_step's wave tile): per 32-deep k-step a wave reads 6 row and 9 weight fragments of 16 bytes and issues
// 36 MFMAs; a thread loads two quads of the row tile and one of the weight tile.
// Measured (B = 512, T = 26, 620 -> 2400, ms per encode, every question 26 words / uniform 3..26 / VQA-like; the fp32 kernel 6.98 / 7.06 /
// 2.92): 128 rows with 8 waves 6.19 / 6.30 / 2.62 -- 4 row tiles x 75 unit blocks = 300 workgroups for 256 CUs, a second round of 44; 192
// rows with 12 waves 3.90 / 3.99 / 1.68 -- 225 workgroups, one round, and half as many loads again in flight per CU; with the idle
// waves' MFMAs skipped 3.89 / 3.76 / 1.53.  256 rows need 168 960 bytes of LDS: more than a CU has.  Compiler report (gfx950), both
// instantiations: 156 VGPRs, no AGPRs, 138 240 bytes of LDS (dynamic), no scratch, 3 waves per SIMD (one workgroup per CU).
#include "ncx_gru.h"

using namespace ncx;

namespace {
typedef RnnX6Tile<6, 3 * RNN_BU> G6;                     // a 6 x 2 wave grid: 192 rows | the 96 weight rows of a unit block; 138 240 bytes
}  // namespace

template <bool KEEP>
__global__ __launch_bounds__(G6::T, 1) void k_gru_step_x6(const int* __restrict__ wids, int T, int t, const float* __restrict__ E, int V1, int dim_emb,
                                                         int dim_q, const float* __restrict__ packed, const int* __restrict__ perm,
                                                         const int* __restrict__ lens, const int* __restrict__ n_t, const float* __restrict__ h_prev,
                                                         float* __restrict__ h_next, float* __restrict__ q, int tiles_m, int total, GruKeep<KEEP> keep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds6[];
    // consecutive work items (the row tiles of one unit block, which share its weight rows) go to the same XCD's L2
    const int w = rnn_work_item(blockIdx.x, total);
    if (w >= total) return;
    const int nt = n_t[t];
    const int j = w / tiles_m, m0 = (w - j * tiles_m) * G6::BM;
    if (m0 >= nt) return;                      // (uniform: before any barrier)

    const GruPacked pk = gru_packed(dim_emb, dim_q);
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wu = wave & 1;   // wave tile: rows 32 wr .. + 32, units 16 wu .. + 16
    const bool live = m0 + 32 * wr < nt;       // (wave-uniform)
    const G6 tile(lds6);

    // loader: the rows of E (by word id) and of h_prev behind the A tile's rows, the unit block's rows of the packed layout
    const float* xptr[2]; const float* hptr[2]; const float* bptr[G6::NB];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = min(m0 + tile.arow(i), nt - 1);                      // rows beyond n_t: clamped here, never stored
        int wid = wids[(size_t)perm[row] * T + t];
        wid = min(max(wid, 0), V1 - 1);                                      // an id out of range is never an address (k_rnn_plan flags it)
        xptr[i] = E + (size_t)wid * dim_emb;
        hptr[i] = h_prev + (size_t)row * dim_q;
    }
#pragma unroll
    for (int i = 0; i < G6::NB; ++i) bptr[i] = packed + ((size_t)j * 3 * RNN_BU + tile.wrow(i)) * pk.kp + tile.c4;
    const int nx = pk.kx / GEMM_BK, ns = nx + (t > 0 ? (pk.kp - pk.kx) / GEMM_BK : 0);

    f32x4 va[2], vb[G6::NB];
    auto issue = [&](int s) __attribute__((always_inline)) {
        rnn_xh_load(s, nx, tile.c4, xptr, dim_emb, hptr, dim_q, va);
        tile.load_w(bptr, s, vb);
    };

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc_r[2] = {zero, zero}, acc_z[2] = {zero, zero}, acc_nx[2] = {zero, zero}, acc_nh[2] = {zero, zero};
    const int fragA = tile.frag_at(32 * wr + li), fragB = tile.frag_at(G6::BM + 16 * wu + li);
    auto compute = [&](int buf, bool ish) __attribute__((always_inline)) {
        x6_bf16x8 af[2][3], bf[3][3];
        tile.read_a(buf, fragA, af);
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int g = 0; g < 3; ++g) bf[g][p] = tile.frag(buf, p, fragB + g * RNN_BU * G6::PB);
        // the six plane products, small terms first; inside one product the six accumulators alternate (a dependent MFMA is six issues away)
#pragma unroll
        for (int c = 0; c < 6; ++c) {
#pragma unroll
            for (int i = 0; i < 2; ++i) {
                acc_r[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][X6_A[c]], bf[0][X6_B[c]], acc_r[i], 0, 0, 0);
                acc_z[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][X6_A[c]], bf[1][X6_B[c]], acc_z[i], 0, 0, 0);
                if (ish) acc_nh[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][X6_A[c]], bf[2][X6_B[c]], acc_nh[i], 0, 0, 0);
                else acc_nx[i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][X6_A[c]], bf[2][X6_B[c]], acc_nx[i], 0, 0, 0);
            }
        }
    };
    tile.run(ns, live, va, vb, issue, [](int) {}, [&](int buf, int s) __attribute__((always_inline)) {
        if (s < nx) compute(buf, false); else compute(buf, true);
    });

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
template <bool KEEP>
static int gru_launch_x6(const int32_t* wids, int B, int T, const float* E, int V1, int dim_emb, int dim_q, const float* packed, const RnnPlan& p,
                         float* ha, float* hb, const GruKeep<KEEP>& keep, float* q_out, hipStream_t s) {
    static DevMask attr_set{0};
    NCX_HIP_TRY(set_max_lds_once(attr_set, (const void*)k_gru_step_x6<KEEP>, G6::LDS));
    const int tiles_m = (int)cdiv(B, G6::BM), total = tiles_m * (int)cdiv(dim_q, RNN_BU);
    const unsigned grid = (unsigned)(8 * cdiv(total, 8));
    const size_t hs = (size_t)B * dim_q;
    for (int t = 0; t < T; ++t) {              // every step is launched: how many rows it has is known on the device only
        const float* h_prev = KEEP ? (t > 0 ? ha + (t - 1) * hs : ha) : ((t & 1) ? ha : hb);
        float* h_next = KEEP ? ha + t * hs : ((t & 1) ? hb : ha);
        hipLaunchKernelGGL(k_gru_step_x6<KEEP>, dim3(grid), dim3(G6::T), G6::LDS, s, wids, T, t, E, V1, dim_emb, dim_q, packed, p.perm, p.lens, p.n_t,
                           h_prev, h_next, q_out, tiles_m, total, keep);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}

int gru_steps_x6(const int32_t* wids, int B, int T, const float* E, int V1, int dim_emb, int dim_q, const float* packed, const RnnPlan& p,
                 float* ha, float* hb, float* gates, float* q_out, hipStream_t s) {
    if (gates) return gru_launch_x6<true>(wids, B, T, E, V1, dim_emb, dim_q, packed, p, ha, hb, GruKeep<true>{gates, B, pad_to(dim_q, GEMM_BK)}, q_out, s);
    return gru_launch_x6<false>(wids, B, T, E, V1, dim_emb, dim_q, packed, p, ha, hb, GruKeep<false>{}, q_out, s);
}
}  // namespace ncx
