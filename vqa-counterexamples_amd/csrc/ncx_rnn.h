// ncx_rnn.h -- the recurrent core that the GRU encoder (ncx_gru*.hip) and the two-layer LSTM encoder (ncx_lstm*.hip) share: the length
// plan, the workspace carver and the entry points' argument check, the launchers of the shared kernels (ncx_rnn.hip), and the device code
// that is inlined into the encoders' own kernels (the 64 x 64 NT tile loop of the backward sweeps, the bias column sum).  The forward step
// kernels and the pack kernels are not here: their LDS layouts, accumulators and packed layouts differ.
#pragma once
#include <initializer_list>
#include "ncx_internal.h"

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

// Byte offsets of a workspace's regions, each 256-byte aligned, in the order they are taken
struct WsCarver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
    RnnPlanOff take_plan(int B) { return {take((size_t)B * 4), take((size_t)B * 4), take((size_t)B * 4), take(RNN_MAX_T * 4)}; }
};

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

// The cut of the bf16 x 6 step kernels (ncx_gru_x6.hip, ncx_lstm_x6.hip): x -> three bf16 values by truncation, x = x1 + x2 + x3 exactly
// (x1 = x & 0xFFFF0000, x2 = (x - x1) & 0xFFFF0000, x3 = x - x1 - x2), as split_store of k_att_logits_x6.  Four values: one 8-byte store
// per plane, the planes `plane` bytes apart.
typedef __bf16 rnn_bf16x8 __attribute__((ext_vector_type(8)));
typedef unsigned int rnn_u32x2 __attribute__((ext_vector_type(2)));
__device__ __forceinline__ void rnn_split_store(f32x4 v, unsigned char* base, int plane) {
    unsigned p1[4], p2[4], p3[4];
#pragma unroll
    for (int j = 0; j < 4; ++j) {
        const float xj = v[j];               // (a scalar copy first: __builtin_bit_cast applied to the vector element itself reads element 0 -- hipcc 7.2)
        p1[j] = __builtin_bit_cast(unsigned, xj) & 0xFFFF0000u;
        const float r1 = xj - __builtin_bit_cast(float, p1[j]);
        p2[j] = __builtin_bit_cast(unsigned, r1) & 0xFFFF0000u;
        const float r2 = r1 - __builtin_bit_cast(float, p2[j]);
        p3[j] = __builtin_bit_cast(unsigned, r2);            // (at most 8 significant bits are left: the high half holds them all)
    }
    // v_perm_b32: the high halves of two dwords -> one dword (the even element in the low half)
    const rnn_u32x2 w1 = {__builtin_amdgcn_perm(p1[1], p1[0], 0x07060302u), __builtin_amdgcn_perm(p1[3], p1[2], 0x07060302u)};
    const rnn_u32x2 w2 = {__builtin_amdgcn_perm(p2[1], p2[0], 0x07060302u), __builtin_amdgcn_perm(p2[3], p2[2], 0x07060302u)};
    const rnn_u32x2 w3 = {__builtin_amdgcn_perm(p3[1], p3[0], 0x07060302u), __builtin_amdgcn_perm(p3[3], p3[2], 0x07060302u)};
    *(rnn_u32x2*)(base) = w1; *(rnn_u32x2*)(base + plane) = w2; *(rnn_u32x2*)(base + 2 * plane) = w3;
}

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
