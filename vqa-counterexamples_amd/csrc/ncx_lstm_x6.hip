// ncx_lstm_x6.hip -- the bf16 x 6 (NCX_F_X6) form of the 2-lstm question encoder's step kernel: k_lstm_step_x6 and its wavefront launches
// (lstm2_steps_x6).  Not the default: ncx_lstm2_encode_flags / ncx_lstm2_train_forward_flags take it when their `flags` say so.
//
// Reference: vqa/models/seq2vec.py -- process_lengths + select_last (11-25), TwoLSTM (48-76), factory's `2-lstm` branch (86-89), as
// ncx_lstm.hip.  The step is k_lstm_step's (ncx_lstm.hip) line for line: one wavefront launch per s in [0, T], layer 0 at step s and layer
// 1 at step s - 1 as two ranges of workgroup ids (each a multiple of 8, dealt over the XCDs), n_t read from memory, workgroups beyond it
// exit before their first barrier, rows of E gathered by (clamped) word id on the load side, rows beyond n_t clamped to row n_t - 1 and
// never stored, the ragged last k-step of the x and of the h segment zero filled, step 0 of a layer stops after the x columns, one
// accumulator per gate, the layer's pointers picked by selects, and the epilogue is the shared one (lstm_cell_store, ncx_lstm.h).  What
// differs is the product, which is k_gru_step_x6's (ncx_gru_x6.hip): the operands are cut into three bf16 planes when their tile is stored
// to LDS (layer 0's tanh is taken before the cut, tanh(0) = 0 keeps the zero fill) and six plane products per 16 x 16 x 32 block run with
// fp32 accumulation -- the cut, the order of the products, what is dropped and what is outside the contract: ncx_x6.h.
// One workgroup: 12 waves, 192 rows x the 128 weight rows (i, f, g, o) of one 32-unit block of the packed layout, read as ncx_lstm2_pack
// left them, in the LDS row tile RnnX6Tile<6, 128> (ncx_rnn.h), whose geometry, cut-and-store, weight loads and x-then-h loads this
// kernel uses; the loader coordinates, the fragment reads and the one-barrier loop are written out here, because on the tile's shared
// loop this kernel measured 1.4 - 1.8 % slower; 153 600 bytes, one workgroup per CU.  The waves form a 6 x 2 grid,
// 32 rows x 16 units x 4 gates each (k_lstm_step's wave tile): per 32-deep k-step a wave reads 6 row and 12 weight fragments of 16 bytes
// and issues 48 MFMAs, one gate at a time so that only that gate's weight fragments are live beside the eight accumulators; a thread
// loads two quads of the row tile and up to two of the weight tile.
// Measured (B = 512, T = 26, 620 -> 1200, ms per encode, every question 26 words / uniform 3..26 / VQA-like; the fp32 kernel 6.54 / 6.33 /
// 2.64, torch 6.37 / 6.34 / 6.30 in the same run): 128 rows with 8 waves 5.64 / 5.13 / 2.00 -- 2 layers x 4 row tiles x 38 unit blocks = 304
// workgroups for 256 CUs, a second round of 48; 192 rows with 12 waves 3.84 / 3.59 / 1.53 -- 228 workgroups, one round.  Two gates at a
// time cost 5 % over one, all four at once 9 %.  Compiler report (gfx950), both instantiations: 120 VGPRs, no AGPRs,
// 153 600 bytes of LDS (dynamic), no scratch.
// NCX_LSTM_X6_WR (a build-time constant, 6) is the number of wave rows: 4 gives the 128-row tile on 8 waves (122 880 bytes) that DESIGN 5v
// measures beside this one.
#include "ncx_lstm.h"

using namespace ncx;

#ifndef NCX_LSTM_X6_WR
#define NCX_LSTM_X6_WR 6
#endif

namespace {
typedef RnnX6Tile<NCX_LSTM_X6_WR, 4 * RNN_BU> L6;        // 192 rows | the 128 weight rows of a unit block: 153 600 bytes
}  // namespace

// grid = (layers of this launch) x grid1; workgroups [0, grid1) run layer `layer_base`, [grid1, 2 grid1) layer 1.  KEEP as k_lstm_step.
template <bool KEEP>
__global__ __launch_bounds__(L6::T, 1) void k_lstm_step_x6(LstmStep a, int s, int layer_base, LstmKeep<KEEP> keep) {
    extern __shared__ __attribute__((aligned(16))) unsigned char lds6[];
    const int second = (int)blockIdx.x >= a.grid1;
    const int layer = layer_base + second, bid = (int)blockIdx.x - second * a.grid1;
    const int t = s - layer;
    // (grid1 is a multiple of 8) the row tiles of one unit block, which share its weight rows, go to the same XCD's L2
    const int w = rnn_work_item(bid, a.total);
    if (w >= a.total) return;
    const int nt = a.n_t[t];
    const int j = w / a.tiles_m, m0 = (w - j * a.tiles_m) * L6::BM;
    if (m0 >= nt) return;                      // (uniform: before any barrier)

    const int H = a.H, in = layer ? H : a.emb;
    // (the two layers' entries of the packed layout by selects: a runtime index into a struct would cost a private copy of it)
    const int kx = pad_to(in, GEMM_BK), kp = kx + pad_to(H, GEMM_BK);
    const size_t blk = (size_t)((H + RNN_BU - 1) / RNN_BU) * 4 * RNN_BU;                // weight rows of a layer = floats of its bias block
    const size_t w_floats = blk * kp;
    const float* packed = a.packed + (layer ? blk * (pad_to(a.emb, GEMM_BK) + pad_to(H, GEMM_BK)) + blk : 0);
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
    const L6 tile(lds6);
    const bool live = m0 + 32 * wr < nt;       // (wave-uniform) a wave whose 32 rows are all beyond n_t loads and stores, and multiplies nothing

    // loader: thread owns column quad c4 of tile rows lr + L6::LR i: 2 of the A tile, L6::NB of the weight tile (while inside its 128 rows;
    // c4, lr and bok are the tile's own values, restated: see the file header)
    const float* xptr[2]; const float* hptr[2]; const float* bptr[L6::NB];
    bool bok[L6::NB];
#pragma unroll
    for (int i = 0; i < 2; ++i) {
        const int row = min(m0 + lr + L6::LR * i, nt - 1);                    // rows beyond n_t: clamped here, never stored
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
    for (int i = 0; i < L6::NB; ++i) {
        bok[i] = lr + L6::LR * i < L6::WROWS;                                  // (uniform over a wave: 8 rows per wave and pass)
        bptr[i] = packed + ((size_t)j * L6::WROWS + (bok[i] ? lr + L6::LR * i : lr)) * kp + c4;
    }
    const int nx = kx / GEMM_BK, ns = nx + (t > 0 ? (kp - kx) / GEMM_BK : 0);

    f32x4 va[2], vb[L6::NB];
    auto issue = [&](int ks) __attribute__((always_inline)) {
        rnn_xh_load(ks, nx, c4, xptr, in, hptr, H, va);
        tile.load_w(bptr, ks, vb);
    };
    auto store = [&](int buf, int ks) __attribute__((always_inline)) {
        if (layer == 0 && ks < nx) {           // x = tanh(E[wid]), before the cut; tanh(0) = 0 keeps the zero fill
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) va[i][e] = tanhf(va[i][e]);
        }
        tile.store(buf, va, vb);
    };

    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4][2] = {{zero, zero}, {zero, zero}, {zero, zero}, {zero, zero}};     // [gate i f g o][row half]
    const int fragA = (32 * wr + li) * L6::PB + 16 * lk, fragB = (L6::BM + 16 * wu + li) * L6::PB + 16 * lk;
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const unsigned char* const base = lds6 + buf * L6::BUF;
        x6_bf16x8 af[2][3];
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i][p] = *(const x6_bf16x8*)(base + p * L6::PL + fragA + 16 * i * L6::PB);
        // the six plane products, small terms first, one gate at a time: only that gate's weight fragments are live, and its two
        // accumulators alternate
#pragma unroll
        for (int g = 0; g < 4; ++g) {
            x6_bf16x8 bf[3];
#pragma unroll
            for (int p = 0; p < 3; ++p) bf[p] = *(const x6_bf16x8*)(base + p * L6::PL + fragB + g * RNN_BU * L6::PB);
#pragma unroll
            for (int c = 0; c < 6; ++c)
#pragma unroll
                for (int i = 0; i < 2; ++i) acc[g][i] = __builtin_amdgcn_mfma_f32_16x16x32_bf16(af[i][X6_A[c]], bf[X6_B[c]], acc[g][i], 0, 0, 0);
        }
    };

    // register-staged double-buffered LDS, one barrier per k-step: the loads of step ks + 1 fly over the MFMAs of step ks
    issue(0); store(0, 0);
    __syncthreads();
    int buf = 0;
    for (int ks = 0; ks < ns; ++ks) {
        const bool more = ks + 1 < ns;
        if (more) issue(ks + 1);
        if (live) compute(buf);
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
template <bool KEEP>
static int lstm2_launch_x6(int B, int T, LstmStep a, const LstmKeep<KEEP>& keep, hipStream_t st) {
    static DevMask attr_set{0};
    NCX_HIP_TRY(set_max_lds_once(attr_set, (const void*)k_lstm_step_x6<KEEP>, L6::LDS));
    a.tiles_m = (int)cdiv(B, L6::BM); a.total = a.tiles_m * (int)cdiv(a.H, RNN_BU); a.grid1 = (int)(8 * cdiv(a.total, 8));
    for (int s = 0; s <= T; ++s) {             // every launch is issued: how many rows a step has is known on the device only
        const int layers = (s < T) + (s >= 1);
        hipLaunchKernelGGL(k_lstm_step_x6<KEEP>, dim3((unsigned)(layers * a.grid1)), dim3(L6::T), L6::LDS, st, a, s, s < T ? 0 : 1, keep);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}

int lstm2_steps_x6(int B, int T, LstmStep a, const LstmKeep<true>* keep, hipStream_t s) {
    if (keep) return lstm2_launch_x6<true>(B, T, a, *keep, s);
    return lstm2_launch_x6<false>(B, T, a, LstmKeep<false>{}, s);
}
}  // namespace ncx
