// ncx_rnn.hip -- the kernels that the GRU encoder (ncx_gru*.hip) and the two-layer LSTM encoder (ncx_lstm*.hip) share, behind the
// launchers of ncx_rnn.h: nothing here knows a gate order or a cell.
//   k_rnn_plan   one workgroup: id range check, len_b, a stable counting sort of the rows by length (descending) -> perm, and
//                n_t = #{b : len_b > t}: the active rows of step t are the prefix [0, n_t) of the sorted order.  The length of an
//                all-padding row is the caller's (GRU 1: max(1, .); TwoLSTM T: select_last's index -1).
//   k_rnn_tok    the word id of every valid (t, row) pair, or -1.
//   k_rnn_de     the embedding gradient: one workgroup per row of E sums the dX rows of its id in (t, row) order.
//   k_rnn_dw     a weight gradient as a TN product whose contraction walks (t, row < n_t[t]) with n_t read from memory; a step's k-range
//                ends at n_t rounded up to the k-step (the rows beyond are zeroed on the load side).  128 x 64 output tiles, one workgroup
//                per tile, the whole walk in order.
#include "ncx_rnn.h"

using namespace ncx;

namespace {
constexpr int DW_PA = pitch_rowk(RNN_DW_BM), DW_PB = pitch_rowk(RNN_DW_BN);   // row-is-k pitches (ncx_gemm.h): ds_read_b128 / ds_read_b64
}  // namespace

// lens_tmp [B] is scratch; perm / lens [B] come out in sorted order (length descending, input order inside a length).
__global__ __launch_bounds__(256) void k_rnn_plan(const int* __restrict__ wids, int B, int T, int V1, int empty_len, int* __restrict__ perm,
                                                  int* __restrict__ lens, int* __restrict__ lens_tmp, int* __restrict__ n_t, int* __restrict__ bad) {
    __shared__ int cnt[RNN_MAX_T + 2], start[RNN_MAX_T + 2], sbad;
    const int tid = threadIdx.x;
    if (tid == 0) sbad = 0;
    __syncthreads();
    bool oob = false;
    for (int b = tid; b < B; b += 256) {
        int n = 0;
        for (int t = 0; t < T; ++t) {
            const int w = wids[(size_t)b * T + t];
            oob |= w < 0 || w >= V1;
            n += w != 0;
        }
        lens_tmp[b] = n > 0 ? n : empty_len;
    }
    if (oob) sbad = 1;
    __syncthreads();
    if (tid == 0 && sbad) *bad = 1;
    const int L = tid + 1;                     // thread L - 1 owns the rows of length L
    if (L <= T) {
        int c = 0;
        for (int b = 0; b < B; ++b) c += lens_tmp[b] == L;
        cnt[L] = c;
    }
    __syncthreads();
    if (tid == 0) {
        int run = 0;
        for (int l = T; l >= 1; --l) { start[l] = run; run += cnt[l]; n_t[l - 1] = run; }   // n_t[t] = #{len >= t + 1}
    }
    __syncthreads();
    if (L <= T) {
        int pos = start[L];
        for (int b = 0; b < B; ++b)
            if (lens_tmp[b] == L) { perm[pos] = b; lens[pos] = L; ++pos; }
    }
}

__global__ __launch_bounds__(256) void k_rnn_tok(const int* __restrict__ wids, int B, int T, int V1, const int* __restrict__ perm,
                                                 const int* __restrict__ n_t, int* __restrict__ tok) {
    const int p = blockIdx.x * 256 + threadIdx.x;
    if (p >= B * T) return;
    const int t = p / B, row = p - t * B;
    int v = -1;
    if (row < n_t[t]) {
        const int w = wids[(size_t)perm[row] * T + t];
        if (w >= 0 && w < V1) v = w;
    }
    tok[p] = v;
}

// dE[0] = 0 (padding_idx: torch's embedding backward skips it, whatever read E[0] in the forward).  The workgroup of row v scans tok 256
// positions at a time (one ballot per wave) and adds the rows it finds.  TANH: times 1 - tanh(E[v])^2; otherwise E is not read.
template <bool TANH>
__global__ __launch_bounds__(256) void k_rnn_de(const int* __restrict__ tok, const float* __restrict__ dX, const float* __restrict__ E, int npos, int de,
                                                float* __restrict__ dE) {
    __shared__ unsigned long long found[4];
    const int v = blockIdx.x, tid = threadIdx.x;
    for (int c0 = 0; c0 < de; c0 += 1024) {
        float acc[4] = {0.f, 0.f, 0.f, 0.f};
        if (v != 0) {
            for (int p0 = 0; p0 < npos; p0 += 256) {
                const bool hit = p0 + tid < npos && tok[p0 + tid] == v;
                const unsigned long long m = __ballot(hit);
                if ((tid & 63) == 0) found[tid >> 6] = m;
                __syncthreads();
                for (int w = 0; w < 4; ++w) {
                    unsigned long long mm = found[w];
                    while (mm) {
                        const int b = __ffsll((long long)mm) - 1;
                        mm &= mm - 1;
                        const float* src = dX + (size_t)(p0 + 64 * w + b) * de;
#pragma unroll
                        for (int k = 0; k < 4; ++k) { const int c = c0 + tid + 256 * k; if (c < de) acc[k] += src[c]; }
                    }
                }
                __syncthreads();
            }
        }
#pragma unroll
        for (int k = 0; k < 4; ++k) {
            const int c = c0 + tid + 256 * k;
            if (c >= de) continue;
            float out = acc[k];
            if constexpr (TANH) {
                out = 0.f;
                if (v != 0) { const float th = tanhf(E[(size_t)v * de + c]); out = acc[k] * (1.f - th * th); }
            }
            dE[(size_t)v * de + c] = out;
        }
    }
}

template <bool GATHER, bool TANH_X>
__global__ __launch_bounds__(256) void k_rnn_dw(const RnnDwArgs a) {
    __shared__ __attribute__((aligned(16))) float la[2][GEMM_BK * DW_PA];
    __shared__ __attribute__((aligned(16))) float lb[2][GEMM_BK * DW_PB];
    const int tn = (int)blockIdx.x / a.tiles_m, m0 = ((int)blockIdx.x - tn * a.tiles_m) * RNN_DW_BM, n0 = tn * RNN_DW_BN;
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const int li = lane & 15, lk = lane >> 4;
    const int wm0 = (wave >> 1) * (RNN_DW_BM / 2), wn0 = (wave & 1) * (RNN_DW_BN / 2);
    const int kr = tid >> 3, cq = 4 * (tid & 7);

    // loader: thread owns k-row kr of the step, column quads cq + 32 i (4 of the gate-gradient tile, 2 of the X tile)
    int acol[4], bcol[2];
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int m = min(m0 + cq + 32 * i, a.kp - 4);                           // columns beyond kp: clamped here, never stored
        acol[i] = m + (m >= a.skip_from ? a.skip_by : 0);
    }
#pragma unroll
    for (int i = 0; i < 2; ++i) bcol[i] = n0 + cq + 32 * i;
    const bool b_full = n0 + RNN_DW_BN <= a.cols;

    f32x4 va[4], vb[2];
    bool a_ok = false;
    auto issue = [&](int t, int r0, int nr) __attribute__((always_inline)) {
        const int krow = r0 + kr, rc = min(krow, nr - 1);
        a_ok = krow < nr;                                                         // rows n_t .. the end of the k-step: zeroed in store()
        const float* ap = a.dG + ((size_t)t * a.B + rc) * a.ld;
        const float* bp = GATHER ? a.X + (size_t)max(a.tok[(size_t)t * a.B + rc], 0) * a.cols  // an id out of range is -1 here: never an address
                                 : a.X + ((size_t)(t - a.xshift) * a.B + rc) * a.cols;
#pragma unroll
        for (int i = 0; i < 4; ++i) va[i] = *(const f32x4*)(ap + acol[i]);
        if (b_full) {
#pragma unroll
            for (int i = 0; i < 2; ++i) vb[i] = *(const f32x4u*)(bp + bcol[i]);
        } else {
#pragma unroll
            for (int i = 0; i < 2; ++i) vb[i] = load4(bp, bcol[i], a.cols);
        }
    };
    auto store = [&](int buf) __attribute__((always_inline)) {
        const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        if (TANH_X) {                          // x = tanh(E[wid]); tanh(0) = 0 keeps the zero fill
#pragma unroll
            for (int i = 0; i < 2; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) vb[i][e] = tanhf(vb[i][e]);
        }
#pragma unroll
        for (int i = 0; i < 4; ++i) *(f32x4*)(&la[buf][kr * DW_PA + cq + 32 * i]) = a_ok ? va[i] : zero;
#pragma unroll
        for (int i = 0; i < 2; ++i) *(f32x4*)(&lb[buf][kr * DW_PB + cq + 32 * i]) = vb[i];
    };
    const f32x4 zero = {0.f, 0.f, 0.f, 0.f};
    f32x4 acc[4][2];
#pragma unroll
    for (int i = 0; i < 4; ++i) { acc[i][0] = zero; acc[i][1] = zero; }
    // interleaved block mapping (ncx_gemm.h): MFMA block i of a wave owns tile rows wm0 + 4 r + i, block j tile columns wn0 + 2 c + j, so one
    // ds_read_b128 / ds_read_b64 per k-row feeds all of a lane's blocks
    auto compute = [&](int buf) __attribute__((always_inline)) {
        const float* pa = &la[buf][wm0 + 4 * li];
        const float* pb = &lb[buf][wn0 + 2 * li];
#pragma unroll
        for (int tt = 0; tt < GEMM_BK / 8; ++tt) {
            const int kk = 8 * tt + 2 * lk;
            f32x4 av[2]; f32x2 bv[2];
#pragma unroll
            for (int e = 0; e < 2; ++e) { av[e] = *(const f32x4*)(pa + (kk + e) * DW_PA); bv[e] = *(const f32x2*)(pb + (kk + e) * DW_PB); }
#pragma unroll
            for (int e = 0; e < 2; ++e)
#pragma unroll
                for (int i = 0; i < 4; ++i)
#pragma unroll
                    for (int j = 0; j < 2; ++j) acc[i][j] = __builtin_amdgcn_mfma_f32_16x16x4f32(av[e][i], bv[e][j], acc[i][j], 0, 0, 0);
        }
    };

    // the walk: steps xshift .. while n_t[t] > 0 (n_t never rises), rows in k-steps of 32; register-staged double-buffered LDS, one barrier
    // per k-step: the loads of the next step fly over the MFMAs of this one
    int t = a.xshift, r0 = 0, nr = t < a.T ? a.n_t[t] : 0;
    if (nr > 0) {
        issue(t, r0, nr); store(0);
        __syncthreads();
        int buf = 0;
        for (;;) {
            r0 += GEMM_BK;
            if (r0 >= nr) { ++t; r0 = 0; nr = t < a.T ? a.n_t[t] : 0; }
            const bool more = nr > 0;
            if (more) issue(t, r0, nr);
            compute(buf);
            if (more) store(buf ^ 1);
            __syncthreads();
            buf ^= 1;
            if (!more) break;
        }
    }

    // epilogue: acc[i][j][q] is tile row wm0 + 4 (4 lk + q) + i, tile column wn0 + 2 li + j; with no k-step at all the tile is exactly 0
#pragma unroll
    for (int i = 0; i < 4; ++i)
#pragma unroll
        for (int q = 0; q < 4; ++q) {
            const int m = m0 + wm0 + 4 * (4 * lk + q) + i, g = m / a.unitsp, uu = m - g * a.unitsp;
            if (m >= a.kp || uu >= a.units) continue;
#pragma unroll
            for (int j = 0; j < 2; ++j) {
                const int c = n0 + wn0 + 2 * li + j;
                if (c < a.cols) a.out[((size_t)g * a.units + uu) * a.cols + c] = acc[i][j][q];
            }
        }
}

namespace ncx {
bool rnn_dims_ok(long long B, long long T, long long emb, long long units) {
    if (B < 1 || T < 1 || T > RNN_MAX_T || emb < 1 || units < 1) return false;
    if (B * T >= (1ll << 31) || emb >= (1 << 24) || units >= (1 << 24)) return false;
    return cdiv(B, RNN_BM) * cdiv(units, RNN_BU) < (1ll << 28);        // the step launch's grid
}

hipError_t rnn_plan(const int32_t* wids, int B, int T, int V1, const RnnPlan& p, int empty_len, int32_t* bad_id_flag, hipStream_t s) {
    hipLaunchKernelGGL(k_rnn_plan, dim3(1), dim3(256), 0, s, wids, B, T, V1, empty_len, p.perm, p.lens, p.lens_tmp, p.n_t, (int*)bad_id_flag);
    return hipGetLastError();
}

hipError_t rnn_tok(const int32_t* wids, int B, int T, int V1, const int* perm, const int* n_t, int* tok, hipStream_t s) {
    hipLaunchKernelGGL(k_rnn_tok, dim3((unsigned)cdiv((long long)B * T, 256)), dim3(256), 0, s, wids, B, T, V1, perm, n_t, tok);
    return hipGetLastError();
}

hipError_t rnn_embed_grad(const int* tok, const float* dX, const float* tanh_of, int B, int T, int V1, int de, float* dE, hipStream_t s) {
    if (tanh_of) hipLaunchKernelGGL(k_rnn_de<true>, dim3((unsigned)V1), dim3(256), 0, s, tok, dX, tanh_of, B * T, de, dE);
    else hipLaunchKernelGGL(k_rnn_de<false>, dim3((unsigned)V1), dim3(256), 0, s, tok, dX, tanh_of, B * T, de, dE);
    return hipGetLastError();
}

hipError_t rnn_dw(const RnnDwArgs& args, bool gather, bool tanh_x, hipStream_t s) {
    RnnDwArgs a = args;
    a.tiles_m = (int)cdiv(a.kp, RNN_DW_BM);
    const dim3 grid((unsigned)(a.tiles_m * cdiv(a.cols, RNN_DW_BN)));
    if (!gather) hipLaunchKernelGGL((k_rnn_dw<false, false>), grid, dim3(256), 0, s, a);
    else if (!tanh_x) hipLaunchKernelGGL((k_rnn_dw<true, false>), grid, dim3(256), 0, s, a);
    else hipLaunchKernelGGL((k_rnn_dw<true, true>), grid, dim3(256), 0, s, a);
    return hipGetLastError();
}
}  // namespace ncx
