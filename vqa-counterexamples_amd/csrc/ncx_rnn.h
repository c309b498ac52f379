// ncx_rnn.h -- the recurrent core that the GRU encoder (ncx_gru*.hip) and the two-layer LSTM encoder (ncx_lstm*.hip) share: the length
// plan, the workspace carver and the entry points' argument check, the launchers of the shared kernels (ncx_rnn.hip), and the device code
// that is inlined into the encoders' own kernels (the 64 x 64 NT tile loop of the backward sweeps, the LDS row tile of the bf16 x 6
// kernels, the work-item numbering, the bias column sum).  The fp32 forward step kernels and the pack kernels are not here: their LDS
// layouts, accumulators and packed layouts differ.
#pragma once
#include <initializer_list>
#include "ncx_internal.h"
#include "ncx_x6.h"

namespace ncx {

constexpr int RNN_BM = 64;        // rows (questions) per workgroup of a step kernel
constexpr int RNN_BU = 32;        // hidden units per workgroup of a step kernel (x 3 or 4 gates of weight rows)
constexpr int RNN_MAX_T = 64;

// ---- host: plan, workspace, argument check ----

struct RnnPlan { int* perm; int* lens; int* lens_tmp; int* n_t; };      // k_rnn_plan's outputs ([B], [B], [B] scratch, [RNN_MAX_T])
struct RnnPlanOff {
    size_t perm, lens, lens_tmp, n_t;
    RnnPlan at(void* ws) const { char* b = (char*)ws; return {(int*)(b + perm), (int*)(b + lens), (int*)(b + lens_tmp), (int*)(b + n_t)}; }
};

// the plan's four regions, first in every encoder's workspace (WsCarver: ncx_internal.h)
static inline RnnPlanOff take_plan(WsCarver& c, int B) {
    return {c.take((size_t)B * 4), c.take((size_t)B * 4), c.take((size_t)B * 4), c.take(RNN_MAX_T * 4)};
}

// Sizes that every index, offset and the step launch's grid (rows / RNN_BM x units / RNN_BU workgroups) of either encoder can hold
__attribute__((visibility("hidden"))) bool rnn_dims_ok(long long B, long long T, long long emb, long long units);

// What every entry point asks of its pointers: none of `ptrs` is null, `packed` is there and 16-byte aligned
static inline bool rnn_ptrs_ok(std::initializer_list<const void*> ptrs, const void* packed) {
    for (const void* p : ptrs)
        if (!p) return false;
    return packed && !((uintptr_t)packed & 15);
}
// ... and of its workspace: there, 256-byte aligned and at least `total` bytes
static inline bool rnn_args_ok(std::initializer_list<const void*> ptrs, const void* packed, const void* workspace, size_t workspace_bytes,
                               size_t total) {
    return rnn_ptrs_ok(ptrs, packed) && workspace && !((uintptr_t)workspace & 255) && workspace_bytes >= total;
}

// ---- the kernels of ncx_rnn.hip ----

// One workgroup: id range check (-> *bad_id_flag = 1), len_b = #{t : wids[b, t] != 0} or empty_len when that is 0, a stable counting sort
// of the rows by length (descending) -> perm / lens, and n_t[t] = #{b : len_b > t}.
__attribute__((visibility("hidden"))) hipError_t rnn_plan(const int32_t* wids, int B, int T, int V1, const RnnPlan& p, int empty_len,
                                                          int32_t* bad_id_flag, hipStream_t s);
// tok[t][row] = the word id of the valid pair (t, row < n_t[t]) when it is inside [0, V1), else -1
__attribute__((visibility("hidden"))) hipError_t rnn_tok(const int32_t* wids, int B, int T, int V1, const int* perm, const int* n_t, int* tok,
                                                         hipStream_t s);
// dE[v] = sum of dX [B T][de] over the positions whose tok is v, in order; dE[0] = 0.  With tanh_of (the embedding matrix whose tanh
// was the encoder's input) the sum is multiplied by 1 - tanh(tanh_of[v])^2; NULL: tanh_of is never read.
__attribute__((visibility("hidden"))) hipError_t rnn_embed_grad(const int* tok, const float* dX, const float* tanh_of, int B, int T, int V1, int de,
                                                                float* dE, hipStream_t s);

// A weight gradient as a TN product whose contraction walks (t, row < n_t[t]) from t = xshift:
//   out[g units + u][c] = sum dG_t[row][col(g unitsp + u)] * X(t, row)[c],   g unitsp + u < kp, u < units, c < cols
// col(m) = m, + skip_by where m >= skip_from (the GRU's W_hh walk takes blocks r z hn of r z n hn; 0, 0 otherwise).
// X(t, row) = X[(t - xshift) B + row] (a [T][B][cols] stash); gather: X[tok[t][row]]; tanh_x (with gather): tanh of that row.
struct RnnDwArgs {
    const float* dG; const float* X; const int* tok; const int* n_t; float* out;
    int B, T, ld, kp, units, unitsp, skip_from, skip_by, cols, xshift;       // ld: floats of a dG row
    int tiles_m;                                                               // (rnn_dw sets it: gate-row tiles of the grid)
};
constexpr int RNN_DW_BM = 128, RNN_DW_BN = 64;                                 // the output tile: gate rows x feature columns
__attribute__((visibility("hidden"))) hipError_t rnn_dw(const RnnDwArgs& a, bool gather, bool tanh_x, hipStream_t s);

// ---- device code inlined into the encoders' kernels ----

// A row index at or beyond n is read from row n - 1 (row 0 when n is 0): such rows are never stored, or are zeroed on the way to LDS
__device__ __forceinline__ int rnn_clamp_row(int r, int n) { return max(min(r, n - 1), 0); }

// The 64 x 64 NT tile of the backward sweeps and the dX products: acc += A[m0 .. + 64][k-steps s0 .. s1) . W[n0 .. + 64]^T on
// v_mfma_f32_16x16x4_f32, both operands col-is-k at LDS pitch RNN_NT_P (conflict-free ds_read_b64 fragments, ncx_gemm.h).
//   src.ptr(s, i)   where the loader's quad of A row lr + 32 i sits at k-step s (an aligned, readable 16 bytes)
//   src.zero(s, i)  whether that row counts as zeros at k-step s (decided when the quad goes to LDS)
//   w               the loader's quad of weight row n0 + lr at k-step 0; weight rows are wld floats, padded to whole tiles
// acc[i][j][e] is tile row 32 wr + 16 i + 4 lk + e, tile column 32 wu + 16 j + li.
constexpr int RNN_NT_BM = 64, RNN_NT_BN = 64, RNN_NT_P = GEMM_BK + 4;
constexpr int RNN_NT_LDS = (RNN_NT_BM + RNN_NT_BN) * RNN_NT_P;               // floats of one buffer; the kernel owns float lds[2][RNN_NT_LDS]
template <class ASrc>
__device__ __forceinline__ void rnn_nt_tile(float (&lds)[2][RNN_NT_LDS], const ASrc& src, const float* w, int wld, int s0, int s1, f32x4 (&acc)[2][2]) {
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wr = wave >> 1, wu = wave & 1;   // wave tile: rows 32 wr .. + 32, columns 32 wu .. + 32
    const int c4 = 4 * (tid & 7), lr = tid >> 3;
    // loader: thread owns column quad c4 of tile rows lr + 32 i (2 of the A tile, 2 of the weight tile); every load is an aligned 16 bytes
    const float* bptr[2];
#pragma unroll
    for (int i = 0; i < 2; ++i) bptr[i] = w + (size_t)(32 * i) * wld;
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 va[2], vb[2];
    auto issue = [&](int s) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) va[i] = *(const f32x4*)src.ptr(s, i);
#pragma unroll
        for (int i = 0; i < 2; ++i) vb[i] = *(const f32x4*)(bptr[i] + s * GEMM_BK);
    };
    auto store = [&](int buf, int s) __attribute__((always_inline)) {
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(lr + 32 * i) * RNN_NT_P + c4]) = src.zero(s, i) ? zero : va[i];
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(&lds[buf][(RNN_NT_BM + lr + 32 * i) * RNN_NT_P + c4]) = vb[i];
    };
    // MFMA (tt, e) takes k = 8 tt + 2 lk + e from lane group lk for both operands (ncx_gemm.h)
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const float* pa = &lds[buf][(32 * wr + li) * RNN_NT_P + 2 * lk];
        const float* pb = &lds[buf][(RNN_NT_BM + 32 * wu + li) * RNN_NT_P + 2 * lk];
#pragma unroll
        for (int tt = 0; tt < GEMM_BK / 8; ++tt) {
            const f32x2 a0 = *(const f32x2*)(pa + 8 * tt), a1 = *(const f32x2*)(pa + 16 * RNN_NT_P + 8 * tt);
            const f32x2 b0 = *(const f32x2*)(pb + 8 * tt), b1 = *(const f32x2*)(pb + 16 * RNN_NT_P + 8 * tt);
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
    issue(s0); store(0, s0);
    __syncthreads();
    int buf = 0;
    for (int s = s0; s < s1; ++s) {
        const bool more = s + 1 < s1;
        if (more) issue(s + 1);
        compute(buf);
        if (more) store(buf ^ 1, s + 1);
        __syncthreads();
        buf ^= 1;
    }
}

// Workgroup ids are dealt round-robin over the 8 XCDs, so work item (id & 7) per + (id >> 3), per = ceil(total / 8): consecutive work
// items run on the same XCD at the same time and share its L2.  The grid is a multiple of 8; an item at or beyond `total` has no work.
template <class Id>                           // (blockIdx.x as it is, or an int)
__device__ __forceinline__ int rnn_work_item(Id id, int total) { return (int)(id & 7) * ((total + 7) >> 3) + (int)(id >> 3); }

// The LDS row tile of the bf16 x 6 recurrent kernels (k_gru_step_x6, k_lstm_step_x6, k_gru_bgemm_x6; the cut and the products: ncx_x6.h):
// acc += A[32 WR rows][k-steps 0 .. ns) . W[NW weight rows]^T, both operands col-is-k in fp32 and cut on the way to LDS.  The workgroup
// is a WR x 2 grid of waves, wave row wr owns tile rows 32 wr .. + 32.  LDS, double buffered: three planes of [BM rows | NW weight
// rows][32 k] bf16 at 80 bytes per row (32 bf16 + 16: plain, conflict-free 16-byte fragment reads; lane group lk holds k = 8 lk .. + 7
// of both operands).  Loader: thread owns column quad c4 of tile rows lr + LR i, 2 of the A tile and NB of the weight tile while inside
// its NW rows (bok[i]; uniform over a wave: 8 rows per wave and pass).  What is the kernel's: where the quads come from (issue), the
// MFMA schedule (compute) and the epilogue.  (k_lstm_step_x6 also keeps its fragment reads and its loop: DESIGN 5x has the timing.)
template <int WR, int NW>
struct RnnX6Tile {
    static constexpr int BM = 32 * WR, T = 128 * WR;         // rows per workgroup, threads
    static constexpr int LR = T / 8;                         // tile rows one pass of the loader covers (8 threads per row)
    static constexpr int NB = (NW + LR - 1) / LR;            // passes over the weight rows
    static constexpr int PB = 80;                            // bytes per LDS row of one plane
    static constexpr int WROWS = NW, ROWS = BM + NW;         // weight rows; tile rows: the A rows, then the weight rows
    static constexpr int PL = ROWS * PB, BUF = 3 * PL, LDS = 2 * BUF;        // one plane, one buffer (three planes), both buffers
    static_assert(GEMM_BK == 32, "one k-step is one MFMA depth");
    static_assert(BM == 2 * LR, "the loader takes the A tile in two passes");
    static_assert(LDS <= 160 * 1024, "LDS");

    unsigned char* const lds;
    const int c4, lr, lk;
    bool bok[NB];
    __device__ __forceinline__ explicit RnnX6Tile(unsigned char* lds_) : lds(lds_), c4(4 * (threadIdx.x & 7)), lr(threadIdx.x >> 3), lk((threadIdx.x & 63) >> 4) {
#pragma unroll
        for (int i = 0; i < NB; ++i) bok[i] = lr + LR * i < NW;
    }
    // the tile row of the loader's pass i over the A rows / the weight rows (a pass beyond them points at row lr and is never loaded)
    __device__ __forceinline__ int arow(int i) const { return lr + LR * i; }
    __device__ __forceinline__ int wrow(int i) const { return bok[i] ? lr + LR * i : lr; }
    // the weight quads of k-step s; w[i] points at this thread's quad of weight row wrow(i) at k-step 0
    __device__ __forceinline__ void load_w(const float* const (&w)[NB], int s, f32x4 (&vb)[NB]) const {
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (bok[i]) vb[i] = *(const f32x4*)(w[i] + s * GEMM_BK);
    }
    __device__ __forceinline__ void store(int buf, const f32x4 (&va)[2], const f32x4 (&vb)[NB]) const {
        unsigned char* const base = lds + buf * BUF + 2 * c4;
#pragma unroll
        for (int i = 0; i < 2; ++i) x6_split_store(va[i], base + (lr + LR * i) * PB, PL);
#pragma unroll
        for (int i = 0; i < NB; ++i)
            if (bok[i]) x6_split_store(vb[i], base + (BM + lr + LR * i) * PB, PL);
    }
    // byte offset of this lane's fragment of tile row `row` inside a plane; the fragment of plane p in buffer buf
    __device__ __forceinline__ int frag_at(int row) const { return row * PB + 16 * lk; }
    __device__ __forceinline__ x6_bf16x8 frag(int buf, int p, int at) const { return *(const x6_bf16x8*)(lds + buf * BUF + p * PL + at); }
    // the A fragments of the wave's two 16-row blocks (at = frag_at(32 wr + li)), every plane
    __device__ __forceinline__ void read_a(int buf, int at, x6_bf16x8 (&af)[2][3]) const {
#pragma unroll
        for (int p = 0; p < 3; ++p)
#pragma unroll
            for (int i = 0; i < 2; ++i) af[i][p] = frag(buf, p, at + 16 * i * PB);
    }
    // Register-staged, one barrier per k-step: issue(s + 1) loads into va / vb over the MFMAs of step s (compute(buf, s)), then
    // pre(s + 1) may transform the loaded quads before they are cut and stored to the other buffer.  A wave that is not `live` (its 32
    // rows all beyond n_t) takes part in the loads, the stores and the barriers and multiplies nothing.  ns >= 1.
    template <class Issue, class Pre, class Compute>
    __device__ __forceinline__ void run(int ns, bool live, f32x4 (&va)[2], f32x4 (&vb)[NB], const Issue& issue, const Pre& pre, const Compute& compute) const {
        issue(0); pre(0); store(0, va, vb);
        __syncthreads();
        int buf = 0;
        for (int s = 0; s < ns; ++s) {
            const bool more = s + 1 < ns;
            if (more) issue(s + 1);
            if (live) compute(buf, s);
            if (more) { pre(s + 1); store(buf ^ 1, va, vb); }
            __syncthreads();
            buf ^= 1;
        }
    }
};

// The A quads of k-step s of a step kernel's x-then-h walk: k-steps [0, nx) run over the xcols columns of the rows at x[i], the rest
// over the hcols columns of the rows at h[i]; the ragged last k-step of either segment is guarded and zero filled.  c4: the quad.
__device__ __forceinline__ void rnn_xh_load(int s, int nx, int c4, const float* const (&x)[2], int xcols, const float* const (&h)[2], int hcols,
                                            f32x4 (&va)[2]) {
    const bool ish = s >= nx;
    const int k = (ish ? s - nx : s) * GEMM_BK + c4, cols = ish ? hcols : xcols;
    if (k - c4 + GEMM_BK <= cols) {
#pragma unroll
        for (int i = 0; i < 2; ++i) va[i] = *(const f32x4u*)((ish ? h[i] : x[i]) + k);
    } else {
#pragma unroll
        for (int i = 0; i < 2; ++i) va[i] = load4(ish ? h[i] : x[i], k, cols);
    }
}

// The bias gradients' column sum: column `col` of dG [T][B][ld] over every valid pair (t, row < n_t[t]).  For a 256-thread workgroup that
// owns 32 columns: thread (g, c) = (tid >> 5, tid & 31) sums rows g, g + 8, ... of every step in ascending order, the 8 partial sums are
// added in ascending g (k_mt_colsum's scheme).  True for the threads g == 0, which hold the finished sum in `s`; where it goes is the
// caller's business.
__device__ __forceinline__ bool rnn_colsum(const float* __restrict__ dG, size_t ld, const int* __restrict__ n_t, int B, int T, int col, float& s) {
    __shared__ float part[8][32];
    const int c = threadIdx.x & 31, g = threadIdx.x >> 5;
    float sum = 0.f;
    for (int t = 0; t < T; ++t) {
        const int nr = n_t[t];
        if (nr == 0) break;
        const float* p = dG + (size_t)t * B * ld + col;
#pragma unroll 4
        for (int row = g; row < nr; row += 8) sum += p[(size_t)row * ld];
    }
    part[g][c] = sum;
    __syncthreads();
    if (g != 0) return false;
    s = part[0][c];
#pragma unroll
    for (int k = 1; k < 8; ++k) s += part[k][c];
    return true;
}

}  // namespace ncx
