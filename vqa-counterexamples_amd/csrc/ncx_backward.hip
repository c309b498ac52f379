// ncx_backward.hip -- the backward entry points of the C ABI (ncx_train_tail, ncx_backward, ncx_backward_phase, ncx_ws_region)
// and their bandwidth-bound kernels.  The GEMMs run on ncx_gemm.h, ncx_dwkm.hip, ncx_dwtn.hip and ncx_main.h.
#include "ncx_driver.h"
#include "ncx_wave.h"
#include "ncx_dwred.h"
#include "ncx_bf16.h"

namespace ncx {
// dpre[r,n] = gs[r] * w_out[n] * (h[r,n] > 0 ? scale : 0)          (backward of out + dropout + relu)
__global__ __launch_bounds__(256) void k_dpre_last(const float* __restrict__ gs, const float* __restrict__ w_out,
                                                   const float* __restrict__ h, float* __restrict__ dpre,
                                                   long long total, int H, float scale) {
    long long i = ((long long)blockIdx.x * 256 + threadIdx.x) * 4;
    if (i >= total) return;
    const int r = (int)(i / H), n = (int)(i - (long long)r * H);
    if (n + 3 < H && i + 3 < total) {
        const f32x4 hv = *(const f32x4u*)(h + i);
        const f32x4 wv = *(const f32x4u*)(w_out + n);
        const float g = gs[r];
        f32x4 o;
#pragma unroll
        for (int j = 0; j < 4; ++j) o[j] = hv[j] > 0.f ? g * wv[j] * scale : 0.f;
        *(f32x4u*)(dpre + i) = o;
    } else {
        for (int j = 0; j < 4 && i + j < total; ++j) {
            const int rr = (int)((i + j) / H), nn = (int)((i + j) - (long long)rr * H);
            dpre[i + j] = h[i + j] > 0.f ? gs[rr] * w_out[nn] * scale : 0.f;
        }
    }
}

// partial[ch][n] = sum over rows of chunk ch of x[r][n] (* wgt[r]);  finish sums the chunks.
__global__ __launch_bounds__(256) void k_colsum_partial(const float* __restrict__ x, const float* __restrict__ wgt,
                                                        int M, int N, float* __restrict__ partial) {
    const int n = blockIdx.x * 256 + threadIdx.x;
    const int ch = blockIdx.y, nch = gridDim.y;
    if (n >= N) return;
    const int r0 = (int)((long long)M * ch / nch), r1 = (int)((long long)M * (ch + 1) / nch);
    float s0 = 0.f, s1 = 0.f, s2 = 0.f, s3 = 0.f;
    int r = r0;
    if (wgt) {
        for (; r + 3 < r1; r += 4) {
            s0 += x[(long long)r * N + n] * wgt[r];           s1 += x[(long long)(r + 1) * N + n] * wgt[r + 1];
            s2 += x[(long long)(r + 2) * N + n] * wgt[r + 2]; s3 += x[(long long)(r + 3) * N + n] * wgt[r + 3];
        }
        for (; r < r1; ++r) s0 += x[(long long)r * N + n] * wgt[r];
    } else {
        for (; r + 3 < r1; r += 4) {
            s0 += x[(long long)r * N + n];       s1 += x[(long long)(r + 1) * N + n];
            s2 += x[(long long)(r + 2) * N + n]; s3 += x[(long long)(r + 3) * N + n];
        }
        for (; r < r1; ++r) s0 += x[(long long)r * N + n];
    }
    partial[(long long)ch * N + n] = (s0 + s1) + (s2 + s3);
}
// out[n] = sum_ch partial[ch][n]: 32 threads per column (8 columns per block), fixed-order tree -> deterministic
__global__ __launch_bounds__(256) void k_colsum_finish(const float* __restrict__ partial, int nch, int N,
                                                       float* __restrict__ out) {
    __shared__ float red[32][9];
    const int c = threadIdx.x & 7, g = threadIdx.x >> 3;
    const int n = blockIdx.x * 8 + c;
    float s = 0.f;
    if (n < N) for (int ch = g; ch < nch; ch += 32) s += partial[(long long)ch * N + n];
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && n < N) {
        float t = 0.f;
        for (int i = 0; i < 32; ++i) t += red[i][c];
        out[n] = t;
    }
}
// out[0] = sum(x[0..n)); single block.
__global__ __launch_bounds__(256) void k_sum_vec(const float* __restrict__ x, int n, float* __restrict__ out) {
    __shared__ float sl[4];
    float acc = 0.f;
    for (int i = threadIdx.x; i < n; i += 256) acc += x[i];
    acc = wave_sum(acc);
    if ((threadIdx.x & 63) == 0) sl[threadIdx.x >> 6] = acc;
    __syncthreads();
    if (threadIdx.x == 0) out[0] = sl[0] + sl[1] + sl[2] + sl[3];
}

// Backward prelude in one pass over h_L.  One WAVE per run of triplets, lane = 4 consecutive columns (+ 256 per column pass):
//   dpre[r][n] = gs[r] * w_out[n] * (h[r][n] > 0 ? scale : 0)                    (out + dropout + relu backward)
//   partial_w[wave][n] = sum_r gs[r] h[r][n]    partial_b[wave] = sum_r gs[r]     (-> d out.weight, d out.bias)
//   L == 1 only: dsh[b][n] = sum_k dpre[b*K+k][n],  partial_b1[wave][n] = sum_b dsh[b][n]   (-> d linear_1.bias)
// The K rows of a triplet are fetched 8 at a time with unconditional 16-byte loads (the column-per-thread form walked them one
// dependent load at a time on 4 waves per CU: 18.7 us for 28 MB at configs[1]); no LDS, no barrier: a lane owns its columns.
__global__ __launch_bounds__(256) void k_bwd_prelude(const float* __restrict__ gs, const float* __restrict__ w_out,
                                                     const float* __restrict__ h, float* __restrict__ dpre,
                                                     float* __restrict__ dsh, int B, int K, int H, float scale,
                                                     float* __restrict__ partial_w, float* __restrict__ partial_b1,
                                                     float* __restrict__ partial_b, float* __restrict__ zero_buf, long long zero_n) {
    const int blk = blockIdx.x, nblk = gridDim.x;
    if (zero_buf) {          // dGgt = one-hot(aid)^T dSh is scattered into zeros later in the backward: cleared here (saves a memset launch)
        const long long z0 = zero_n * blk / nblk / 4 * 4, z1 = blk + 1 == nblk ? zero_n : zero_n * (blk + 1) / nblk / 4 * 4;
        for (long long i = z0 + 4 * threadIdx.x; i < z1; i += 1024) {
            if (i + 3 < z1) *(f32x4u*)(zero_buf + i) = f32x4{0.f, 0.f, 0.f, 0.f};
            else for (long long j = i; j < z1; ++j) zero_buf[j] = 0.f;
        }
    }
    const int lane = threadIdx.x & 63;
    const int wv = blk * 4 + (threadIdx.x >> 6), nwv = nblk * 4;
    const int b0 = (int)((long long)B * wv / nwv), b1 = (int)((long long)B * (wv + 1) / nwv);
    auto put4 = [&](float* p, int c, const f32x4& v) __attribute__((always_inline)) {
        if (c + 3 < H) *(f32x4u*)(p + c) = v;
        else { p[c] = v[0]; if (c + 1 < H) p[c + 1] = v[1]; if (c + 2 < H) p[c + 2] = v[2]; }
    };
    for (int c = lane * 4; c < H; c += 256) {
        const bool edge = c + 4 > H;
        const f32x4 w = fix_window(load_window(w_out, c, H), c, H);
        f32x4 aw = {0.f, 0.f, 0.f, 0.f}, ab1 = {0.f, 0.f, 0.f, 0.f};
        for (int b = b0; b < b1; ++b) {
            const long long r0 = (long long)b * K;
            f32x4 ds = {0.f, 0.f, 0.f, 0.f};
            for (int k0 = 0; k0 < K; k0 += 8) {
                f32x4 hv[8]; float g[8];
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    const long long r = r0 + min(k0 + j, K - 1);
                    hv[j] = load_window(h + r * H, c, H);
                    g[j] = k0 + j < K ? gs[r] : 0.f;
                }
#pragma unroll
                for (int j = 0; j < 8; ++j) {
                    if (k0 + j < K) {
                        const f32x4 v = edge ? fix_window(hv[j], c, H) : hv[j];
                        f32x4 dp;
#pragma unroll
                        for (int q = 0; q < 4; ++q) { dp[q] = v[q] > 0.f ? g[j] * w[q] * scale : 0.f; aw[q] = __builtin_fmaf(g[j], v[q], aw[q]); ds[q] += dp[q]; }
                        put4(dpre + (r0 + k0 + j) * H, c, dp);
                    }
                }
            }
            if (dsh) { put4(dsh + (long long)b * H, c, ds); ab1 += ds; }
        }
        put4(partial_w + (long long)wv * H, c, aw);
        if (dsh) put4(partial_b1 + (long long)wv * H, c, ab1);
    }
    float s = 0.f;
    for (long long r = (long long)b0 * K + lane; r < (long long)b1 * K; r += 64) s += gs[r];
    s = wave_sum(s);
    if (lane == 0) partial_b[wv] = s;
}
// out_w[n] = sum_blk partial_w[blk][n]; out_b1[n] likewise (nullable); out_b[0] = sum_blk partial_b[blk]
__global__ __launch_bounds__(256) void k_bwd_prelude_finish(const float* __restrict__ partial_w, const float* __restrict__ partial_b1,
                                                            const float* __restrict__ partial_b, int nblk, int H,
                                                            float* __restrict__ out_w, float* __restrict__ out_b1,
                                                            float* __restrict__ out_b, const float* __restrict__ loss_rows = nullptr,
                                                            const int* __restrict__ rank = nullptr, int B = 0,
                                                            float* __restrict__ loss = nullptr, int* __restrict__ hits = nullptr) {
    if (blockIdx.y == 2) {                                  // ncx_train_tail: k_loss_finish's sums ride in this launch (same order)
        if (blockIdx.x != 0) return;
        __shared__ float sl[4];
        __shared__ int s1[4], s5[4];
        float acc = 0.f; int h1 = 0, h5 = 0;
        for (int i = threadIdx.x; i < B; i += 256) {
            if (loss_rows) acc += loss_rows[i];
            if (rank) { const int rk = rank[i]; h1 += rk < 1; h5 += rk < 5; }
        }
        acc = wave_sum(acc);
        h1 = (int)wave_sum((float)h1); h5 = (int)wave_sum((float)h5);
        const int wq = threadIdx.x >> 6;
        if ((threadIdx.x & 63) == 0) { sl[wq] = acc; s1[wq] = h1; s5[wq] = h5; }
        __syncthreads();
        if (threadIdx.x == 0) {
            if (loss) loss[0] = sl[0] + sl[1] + sl[2] + sl[3];
            if (hits) { hits[0] = s1[0] + s1[1] + s1[2] + s1[3]; hits[1] = s5[0] + s5[1] + s5[2] + s5[3]; }
        }
        return;
    }
    __shared__ float red[32][9];
    const int c = threadIdx.x & 7, g = threadIdx.x >> 3;
    const int which = blockIdx.y;                                   // 0: out.weight, 1: linear_1.bias
    const float* part = which == 0 ? partial_w : partial_b1;
    float* out = which == 0 ? out_w : out_b1;
    if (!out) return;
    const int n = blockIdx.x * 8 + c;
    // the partial rows of this thread (ch = g, g + 32, ...) are requested 16 at a time before the first is added: a load per
    // iteration of the runtime-length loop was one dependent round trip per row (16 of them = the kernel's 7 us); same order of adds
    float s = 0.f;
    if (n < H) {
        for (int ch0 = g; ch0 < nblk; ch0 += 32 * 16) {
            float v[16];
#pragma unroll
            for (int i = 0; i < 16; ++i) { const int ch = ch0 + 32 * i; v[i] = part[(long long)min(ch, nblk - 1) * H + n]; }
#pragma unroll
            for (int i = 0; i < 16; ++i) s += ch0 + 32 * i < nblk ? v[i] : 0.f;
        }
    }
    red[g][c] = s;
    __syncthreads();
    if (g == 0 && n < H) {
        float t = 0.f;
        for (int i = 0; i < 32; ++i) t += red[i][c];
        out[n] = t;
    }
    if (which == 0 && blockIdx.x == 0) {              // d out.bias: fixed-order tree over the partials
        __shared__ float sb[4];
        float v = 0.f;
        for (int i = threadIdx.x; i < nblk; i += 256) v += partial_b[i];
        v = wave_sum(v);
        if ((threadIdx.x & 63) == 0) sb[threadIdx.x >> 6] = v;
        __syncthreads();
        if (threadIdx.x == 0) out_b[0] = (sb[0] + sb[1]) + (sb[2] + sb[3]);
    }
}

// Training-step fusion (ncx_train_tail): the out layer, the listwise loss / rank and the backward prelude in ONE pass over h_L.
// One wave per run of triplets, lane = 4 columns (H <= 256), the KB >= K rows of a triplet resident in registers:
//   scores[b,k] = h[(b,k),:] . w_out + b_out                       (k_scores)
//   loss_rows / dscores / rank of the triplet                      (k_loss_rank: lane k holds score k)
//   dpre, dSh, partial sums of d out.weight / d out.bias / d linear_1.bias   (k_bwd_prelude, same wave partition)
// Same per-lane arithmetic and the same wave reductions as the three kernels it replaces: scores, loss, ranks and every
// gradient except d out.bias (a sum of zeros-in-maths; other order) are bit-identical to the unfused path.
// FULL: H == 256 and K == KB exactly (every lane owns 4 in-range columns, every row slot a real row): the edge handling -- a branch per store, a repair per load -- is compiled
// out; the kernel is ONE wave's instruction stream per triplet and runs as long as that stream is (round 3: 5 100 -> see DESIGN 7)
template <int KB, bool FULL>
__global__ __launch_bounds__(64) void k_train_tail(const float* __restrict__ h, const float* __restrict__ w_out,
                                                    const float* __restrict__ b_out, const int* __restrict__ gt, int B, int K, int H,
                                                    float loss_scale, float gate_scale, float* __restrict__ scores,
                                                    float* __restrict__ loss_rows, float* __restrict__ dscores, int* __restrict__ rank,
                                                    float* __restrict__ dpre, float* __restrict__ dsh,
                                                    float* __restrict__ partial_w, float* __restrict__ partial_b1,
                                                    float* __restrict__ partial_b, float* __restrict__ zero_buf, long long zero_n, int zchunk) {
    if (FULL) { H = 256; K = KB; }                          // (compile-time extents: row addresses become base + constant, no clamps)
    const int blk = blockIdx.x, nblk = gridDim.x;
    if (zero_buf) {          // (as k_bwd_prelude: dGgt is scattered into zeros later in the backward; zchunk = ceil(zero_n / nblk) up to a
                             // multiple of 4, from the host: a 64-bit division here is ~300 scalar instructions of a 2 400-instruction kernel)
        const long long z0 = (long long)blk * zchunk, z1 = min(z0 + zchunk, zero_n);
        for (long long i = z0 + 4 * threadIdx.x; i < z1; i += 256) {
            if (i + 3 < z1) *(f32x4u*)(zero_buf + i) = f32x4{0.f, 0.f, 0.f, 0.f};
            else for (long long j = i; j < z1; ++j) zero_buf[j] = 0.f;
        }
    }
    const int lane = threadIdx.x;                           // one wave per block: 512 triplets spread over all CUs, not 128 of them
    const int wv = blk, nwv = nblk;
    const int b0 = (int)((unsigned)B * (unsigned)wv / (unsigned)nwv), b1 = (int)((unsigned)B * (unsigned)(wv + 1) / (unsigned)nwv);   // (B * nwv < 2^32: B <= 32768, nwv <= 4096)
    const int c = lane * 4;
    const bool live = FULL || c < H, edge = !FULL && c + 4 > H;
    auto put4 = [&](float* p, const f32x4& v) __attribute__((always_inline)) {
        if (FULL || c + 3 < H) *(f32x4u*)(p + c) = v;
        else if (live) { p[c] = v[0]; if (c + 1 < H) p[c + 1] = v[1]; if (c + 2 < H) p[c + 2] = v[2]; }
    };
    const f32x4 w = FULL ? *(const f32x4u*)(w_out + c) : fix_window(load_window(w_out, c, H), c, H);          // (lanes beyond H: all zeros)
    const float bias = b_out[0];
    f32x4 aw = {0.f, 0.f, 0.f, 0.f}, ab1 = {0.f, 0.f, 0.f, 0.f};
    float sb = 0.f;
    for (int b = b0; b < b1; ++b) {
        const long long r0 = (long long)b * K;
        f32x4 hv[KB];
#pragma unroll
        for (int k = 0; k < KB; ++k) hv[k] = FULL ? *(const f32x4u*)(h + (r0 + min(k, K - 1)) * H + c) : load_window(h + (r0 + min(k, K - 1)) * H, c, H);
        const int g = gt[b];
        if (edge) {
#pragma unroll
            for (int k = 0; k < KB; ++k) hv[k] = fix_window(hv[k], c, H);
        }
        float sc = 0.f;
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            const float t = wave_sum(0.f + dot4(hv[k], w));
            sc = lane == k ? t + bias : sc;
        }
        if (lane < K) scores[r0 + lane] = sc;
        // listwise softmax cross-entropy + rank (k_loss_rank)
        const float s = lane < K ? sc : -INFINITY;
        const float m = wave_max(s);
        const float e = lane < K ? __expf(s - m) : 0.f;
        const float sum = wave_sum(e);
        const float sg = __shfl(s, g, 64);
        const float dsc = lane < K ? (e / sum - (lane == g ? 1.f : 0.f)) * loss_scale : 0.f;
        if (dscores && lane < K) dscores[r0 + lane] = dsc;
        const bool ahead = lane < K && (s > sg || (s == sg && lane < g));
        const unsigned long long bal = __ballot(ahead);
        if (lane == 0) { loss_rows[b] = (logf(sum) - (sg - m)) * loss_scale; rank[b] = __popcll(bal); }
        sb += dsc;
        // backward of out + dropout + relu (k_bwd_prelude)
        f32x4 ds = {0.f, 0.f, 0.f, 0.f};
#pragma unroll
        for (int k = 0; k < KB; ++k) {
            if (k < K) {                                     // (uniform; a `break` would keep the loop rolled and hv[] in scratch)
                const float gk = __shfl(dsc, k, 64);
                f32x4 dp;
#pragma unroll
                for (int q = 0; q < 4; ++q) { dp[q] = hv[k][q] > 0.f ? gk * w[q] * gate_scale : 0.f; aw[q] = __builtin_fmaf(gk, hv[k][q], aw[q]); ds[q] += dp[q]; }
                put4(dpre + (r0 + k) * H, dp);
            }
        }
        if (dsh) { put4(dsh + (long long)b * H, ds); ab1 += ds; }
    }
    put4(partial_w + (long long)wv * H, aw);
    if (dsh) put4(partial_b1 + (long long)wv * H, ab1);
    sb = wave_sum(sb);
    if (lane == 0) partial_b[wv] = sb;
}

// dsh[b][n] = sum_k dpre[b*K + k][n]
__global__ __launch_bounds__(256) void k_rowgroup_sum(const float* __restrict__ dpre, int B, int K, int H,
                                                      float* __restrict__ dsh) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)B * H) return;
    const int b = (int)(i / H), n = (int)(i - (long long)b * H);
    const float* p = dpre + (long long)b * K * H + n;
    float s = 0.f;
    for (int k = 0; k < K; ++k) s += p[(long long)k * H];
    dsh[i] = s;
}

// dggt[n][a] = sum over {b : aid[b] == a} of dsh[b][n]   (dggt [H][A] pre-zeroed).  One block per triplet; the first
// occurrence of an answer id owns column a and adds its duplicates in batch order -> deterministic, no atomics on
// floats.  Backward of the a_emb_gt lookup (cx.py:280) in re-associated form:
//   dE += S^T (dSh . W1[:, a_emb_gt]) = (S^T dSh) . W1[:, a_emb_gt],  S = one-hot(aid)  -> a second pair of the dE GEMM.
__global__ __launch_bounds__(256) void k_scatter_dsh_by_answer(const float* __restrict__ dsh, const int* __restrict__ aid,
                                                               int B, int H, int A, float* __restrict__ dggt) {
    __shared__ unsigned bits[NCX_SCATTER_MAX_B / 32];
    const int b = blockIdx.x;
    const int id = aid[b];
    int earlier = 0;
    for (int j = threadIdx.x; j < b; j += 256) earlier |= aid[j] == id;
    if (__syncthreads_or(earlier)) return;                       // not the owner (uniform per block)
    const int nw = (B + 31) / 32;
    for (int w = threadIdx.x; w < nw; w += 256) bits[w] = 0u;
    __syncthreads();
    for (int j = b + threadIdx.x; j < B; j += 256)
        if (aid[j] == id) atomicOr(&bits[j >> 5], 1u << (j & 31));
    __syncthreads();
    for (int n = threadIdx.x; n < H; n += 256) {
        float s = 0.f;
        for (int w = b >> 5; w < nw; ++w) {
            unsigned m = bits[w];
            while (m) {
                const int j = (w << 5) + __ffs(m) - 1;
                m &= m - 1;
                s += dsh[(long long)j * H + n];
            }
        }
        dggt[(long long)n * A + id] = s;
    }
}

// fp32 path: the answer-embedding gradient runs on the fused forward kernel (ncx_main.h, NT form, 64 x 64 tiles at three
// workgroups per CU: 50 us against 80 us for the TN form of the generic engine -- tools/mb/mb_main.hip, "short chain"):
//   dE[a][j] = sum_n dGt^T[a][n] W1ak^T[j][n] + sum_n dGgt^T[a][n] W1agt^T[j][n]
// whose operands are rows with the reduction index contiguous.  ONE launch prepares them (roles by block range):
//   [0, B)            dGgt^T[id][n] = sum over {b : aid[b] == id} of dSh[b][n]   (owner-computes scatter as above, rows contiguous now;
//                     dGgt^T was cleared by k_bwd_prelude)
//   [B, B + T)        32 x 32 transposes through LDS: dGt [H][A] -> dGt^T [A][Hp4];  W1[:, a_other], W1[:, a_gt] -> [da][Hp32]
//                     (columns beyond H zero: the kernel's weight-side padding)
struct EmbPrepArgs {
    const float* dsh; const int* aid; float* dggtT;        // scatter
    const float* src[3]; float* dst[3]; long long lds_[3]; int cols[3], ldd[3], dcols[3], tile0[4];   // transposes: src [H][cols] -> dst [cols][ldd], dst cols < dcols written
    int B, H, A, Hp4;
    int* perm;                                             // presence permutation (nullable): block 0 builds it, every other role moves up one block
};
// perm (ea.perm != NULL): perm[0 .. A) = the answer ids that occur in aid[0 .. B) ascending, then the others ascending; perm[A] = how many occur.
// ONE block: a bitmap of the ids in LDS (atomicOr: the order of its updates cannot change it), a scan of the per-thread population counts,
// then every thread places the ids of its bitmap words.  Rebuilt on every call, read by the dE launch that follows on the stream.
// `fix` (valid: blocks beyond a.B + a.tile0[3]): the deferred split fix-up of the dW1[:, a_other] GEMM (64 x 64 tiles) rides along
__global__ __launch_bounds__(256) void k_emb_prep(const EmbPrepArgs a, const FixupArgs fix, const Tn8ReduceArgs red) {
    __shared__ unsigned bits[NCX_SCATTER_MAX_B / 32 > 32 * 33 ? NCX_SCATTER_MAX_B / 32 : 32 * 33];     // scatter: id bitmap; transposes: a [32][33] tile
    const int bx = (int)blockIdx.x - (a.perm ? 1 : 0);
    if (bx < 0) {
        __shared__ int scan[256];
        static_assert(NCX_PERM_MAX_A / 32 <= (int)(sizeof(bits) / sizeof(bits[0])), "one bit per answer");
        const int A = a.A, nw = (A + 31) / 32, per = (nw + 255) / 256, tid = threadIdx.x;
        for (int w = tid; w < nw; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int j = tid; j < a.B; j += 256) {
            const int id = a.aid[j];
            if ((unsigned)id < (unsigned)A) atomicOr(&bits[id >> 5], 1u << (id & 31));
        }
        __syncthreads();
        const int w0 = min(tid * per, nw), w1 = min(w0 + per, nw);      // this thread's bitmap words
        int cnt = 0;
        for (int w = w0; w < w1; ++w) cnt += __popc(bits[w]);
        scan[tid] = cnt;
        __syncthreads();
        for (int off = 1; off < 256; off <<= 1) {                        // inclusive scan over the 256 threads
            const int v = tid >= off ? scan[tid - off] : 0;
            __syncthreads();
            scan[tid] += v;
            __syncthreads();
        }
        const int n_present = scan[255];
        int pos = scan[tid] - cnt;                                       // present ids below 32 w0
        for (int w = w0; w < w1; ++w) {
            const unsigned m = bits[w];
            for (int bit = 0; bit < 32; ++bit) {
                const int id = 32 * w + bit;
                if (id >= A) break;
                if ((m >> bit) & 1u) a.perm[pos++] = id;
                else a.perm[n_present + (id - pos)] = id;                // id - pos: absent ids below id
            }
        }
        if (tid == 0) a.perm[A] = n_present;
        return;
    }
    if (bx >= a.B + a.tile0[3]) {
        const int id = bx - (a.B + a.tile0[3]);
        const int nfix = fix.valid ? fix.grid_x * 4 : 0;
        if (id < nfix) split_fixup_body<64, 64>(fix, id / 4, id % 4);
        else tn8_reduce_body(red, id - nfix);            // the partial tiles of the dW1[:, a_other] launch (ncx_dwtn.hip)
        return;
    }
    if (bx < a.B) {
        const int b = bx, B = a.B;
        const int id = a.aid[b];
        int earlier = 0;
        for (int j = threadIdx.x; j < b; j += 256) earlier |= a.aid[j] == id;
        if (__syncthreads_or(earlier)) return;                       // not the owner (uniform per block)
        const int nw = (B + 31) / 32;
        for (int w = threadIdx.x; w < nw; w += 256) bits[w] = 0u;
        __syncthreads();
        for (int j = b + threadIdx.x; j < B; j += 256)
            if (a.aid[j] == id) atomicOr(&bits[j >> 5], 1u << (j & 31));
        __syncthreads();
        for (int n = threadIdx.x; n < a.H; n += 256) {
            float s = 0.f;
            for (int w = b >> 5; w < nw; ++w) {
                unsigned m = bits[w];
                while (m) { const int j = (w << 5) + __ffs(m) - 1; m &= m - 1; s += a.dsh[(long long)j * a.H + n]; }
            }
            a.dggtT[(long long)id * a.Hp4 + n] = s;
        }
        return;
    }
    float* tile = (float*)bits;                                        // [32][33]
    int t = bx - a.B, e = 0;
    while (e < 2 && t >= a.tile0[e + 1]) ++e;
    t -= a.tile0[e];
    const int tiles_h = (a.dcols[e] + 31) / 32;                        // tiles along the source-row (h) direction
    const int th = t % tiles_h, tc = t / tiles_h;
    const int x = threadIdx.x & 31, y = threadIdx.x >> 5;              // 32 x 8 threads
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int h = th * 32 + y + 8 * i, c = tc * 32 + x;
        tile[(y + 8 * i) * 33 + x] = (h < a.H && c < a.cols[e]) ? a.src[e][(long long)h * a.lds_[e] + c] : 0.f;
    }
    __syncthreads();
#pragma unroll
    for (int i = 0; i < 4; ++i) {
        const int c = tc * 32 + y + 8 * i, h = th * 32 + x;
        if (c < a.cols[e] && h < a.dcols[e]) a.dst[e][(long long)c * a.ldd[e] + h] = tile[x * 33 + y + 8 * i];
    }
}

__global__ __launch_bounds__(256) void k_zero_cols(float* __restrict__ p, int rows, long long ld, int cols) {
    const long long i = (long long)blockIdx.x * 256 + threadIdx.x;
    if (i >= (long long)rows * cols) return;
    const int r = (int)(i / cols), c = (int)(i - (long long)r * cols);
    p[(long long)r * ld + c] = 0.f;
}
}  // namespace ncx

namespace ncx {
// ncx_backward_adam's dE launch applies Adam itself: the fp32 NT product (X6 leaves it fp32 too) on its 64 x 64 form, on the caller's stream.
// Experiment hook NCX_NO_FUSED_ADAM: the separate k_adam pass instead.
bool fused_adam_route(const ncx_dims& d, const StepRoutes& r) {
    if (!(d.flags & NCX_F_A_EMB) || (d.flags & NCX_F_BF16) || !r.emb_nt) return false;
    if (km_defers_to_side_stream(d, r) || hook_env("NCX_NO_FUSED_ADAM")) return false;
    return main_short_form(d.A, d.da, 2 * cdiv(pad_to(d.H, 4), GEMM_BK), 1);
}
}  // namespace ncx

using namespace ncx;
extern "C" {
int ncx_train_tail(const ncx_dims* dp, const ncx_params* p, void* workspace, size_t workspace_bytes, const int32_t* gt,
                   float* scores, float* loss_rows, float* loss, float* dscores, int32_t* rank, int32_t* hits,
                   const ncx_grads* g, void* stream_) {
    int rc = check_dims(dp);
    if (rc != NCX_OK) return rc;
    if (!p || !workspace || !gt || !scores || !loss_rows || !rank || !g) return NCX_E_NULL;
    if (!p->w_out || !p->b_out || !g->w_out || !g->b_out || !g->b1) return NCX_E_NULL;
    const ncx_dims& d = *dp;
    if (!(d.flags & NCX_F_FUSED_TAIL)) return NCX_E_FLAGS;
    if (d.K > 32 || d.H > 256) return NCX_E_DIMS;            // the K rows of a triplet live in registers, one lane per 4 columns
    const StepRoutes r = routes(d);
    const WsLayout w = ws_layout(d, r);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const int H = d.H;
    const bool aemb = d.flags & NCX_F_A_EMB;
    const bool emb_nt = r.emb_nt;
    const int Hp4 = pad_to(H, 4);
    float* dagtT = (float*)(ws + w.dgtT) + (size_t)d.A * Hp4;
    float* dagt = (float*)(ws + w.dagt);
    float* partial = (float*)(ws + w.partial);
    float* part_w = partial;
    float* part_b1 = partial + (size_t)NCX_PRELUDE_WAVES * H;
    float* part_b = partial + (size_t)NCX_PRELUDE_WAVES * H * 2;
    const float dscale = (d.training && d.drop_p > 0.f) ? 1.f / (1.f - d.drop_p) : 1.f;
    const float scale = d.loss_scale > 0.f ? d.loss_scale : 1.f / (float)d.B;
    const int nblk = (int)cdiv(d.B < NCX_PRELUDE_WAVES ? d.B : NCX_PRELUDE_WAVES, 4);
    const bool fuse_l1 = d.L == 1;
    const float* hL = (const float*)(ws + w.h[d.L - 1]);
    float* dpre = (float*)(ws + w.dpre[0]);
    float* dsh = fuse_l1 ? (float*)(ws + w.dsh) : (float*)nullptr;
    float* zb = emb_nt ? dagtT : aemb ? dagt : (float*)nullptr;
    const long long zn = emb_nt ? (long long)d.A * Hp4 : (long long)H * d.A;
#define NCX_TAIL_LAUNCH(KB, FULL) hipLaunchKernelGGL((k_train_tail<KB, FULL>), dim3(nblk * 4), dim3(64), 0, s, hL, p->w_out, p->b_out, gt, d.B, d.K, H, scale, dscale, \
                                               scores, loss_rows, dscores, rank, dpre, dsh, part_w, part_b1, part_b, zb, zn, zchunk)
    const int zchunk = (int)((cdiv(zn, (long long)nblk * 4) + 3) / 4 * 4);
    if (H == 256 && d.K == 24) NCX_TAIL_LAUNCH(24, true);          // (the configuration of every options/cx/*.yaml with dim_h 256)
    else if (d.K <= 8) NCX_TAIL_LAUNCH(8, false); else if (d.K <= 16) NCX_TAIL_LAUNCH(16, false); else if (d.K <= 24) NCX_TAIL_LAUNCH(24, false); else NCX_TAIL_LAUNCH(32, false);
#undef NCX_TAIL_LAUNCH
    NCX_HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_bwd_prelude_finish, dim3((unsigned)cdiv(H, 8), 3), dim3(256), 0, s, (const float*)part_w, (const float*)part_b1,
                       (const float*)part_b, nblk * 4, H, g->w_out, fuse_l1 ? g->b1 : (float*)nullptr, g->b_out,
                       (const float*)loss_rows, (const int*)rank, d.B, loss, hits);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

// phase 0: everything.  phase 1: out / hidden layers / b1 and the answer_embedding gradient (complete when it
// returns);  phase 2: linear_1.weight.  1 then 2 == 0 bit for bit (same kernels, the dGt problem launched alone).
// phase 3: everything except the answer_embedding GEMM (leaves dGt | dGgt in the workspace, ncx_ws_region);
// phase 5: phase 1 without the answer_embedding GEMM (leaves dGt | dGgt like phase 3): 5, 2, 4 == 0 bit for bit, and the
// region can be on the wire while phase 2 (the bulk of the backward) runs.
// phase 4: answer_embedding gradient from dGt | dGgt.  3 then 4 == 0 bit for bit; under data parallelism the
// 2 x [H, A] block is summed over ranks between the two, so the [A, da] embedding gradient never crosses the wire.
// adam (phase 0 only, nullable): the optimiser's buffers for the dE launch that applies Adam itself (fused_adam_route); *adam_done tells the
// caller whether that launch ran -- it does not when the dE product takes another route after all.
static int backward_impl(const ncx_dims* dp, const ncx_inputs* in, const ncx_params* p, void* workspace,
                         size_t workspace_bytes, const float* dscores, const ncx_grads* g, void* stream_, int phase,
                         const AdamFuse* adam = nullptr, bool* adam_done = nullptr) {
    int rc = check_dims(dp);
    if (rc != NCX_OK) return rc;
    if (!in || !p || !workspace || !g || (!dscores && !(dp->flags & NCX_F_FUSED_TAIL))) return NCX_E_NULL;
    const ncx_dims& d = *dp;
    const bool aemb = d.flags & NCX_F_A_EMB;
    if (!g->answer_embedding || !g->w1 || !g->b1 || !g->w_out || !g->b_out) return NCX_E_NULL;
    if (d.L >= 2 && (!g->w2 || !g->b2)) return NCX_E_NULL;
    if (d.L >= 3 && (!g->w3 || !g->b3)) return NCX_E_NULL;
    const StepRoutes r = routes(d);
    const WsLayout w = ws_layout(d, r);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const int M = d.B * d.K, H = d.H;
    const SegOffsets o = seg_offsets(d);
    const long long din = o.din;
    const int* idx_k = (const int*)(ws + w.idx_k); const int* idx_o = (const int*)(ws + w.idx_o);
    const int* idx_ob = (const int*)(ws + w.idx_ob);
    const float* mx = (const float*)(ws + w.mx); const float* inv = (const float*)(ws + w.inv);
    const float* misc = (const float*)(ws + w.misc);
    float* dsh = (float*)(ws + w.dsh); float* dgt = (float*)(ws + w.dgt); float* dagt = (float*)(ws + w.dagt);
    const bool emb_nt = r.emb_nt;   // answer-embedding gradient in NT form on the fused forward kernel
    const int Hp4 = pad_to(H, 4), Hp32 = pad_to(H, 32);
    float* dgtT = (float*)(ws + w.dgtT); float* dagtT = dgtT + (size_t)d.A * Hp4;
    float* w1akT = (float*)(ws + w.w1aT); float* w1agtT = w1akT + (size_t)d.da * Hp32;
    float* partial = (float*)(ws + w.partial); float* slab = (float*)(ws + w.slab);
    GemmUse u[U_COUNT];
    list_uses(d, r, u);
    const float dscale = (d.training && d.drop_p > 0.f) ? 1.f / (1.f - d.drop_p) : 1.f;

    auto colsum = [&](const float* x, const float* wgt, int rows, int cols, float* out) -> int {
        const int ch = rows < NCX_COLSUM_CHUNKS * 8 ? (int)cdiv(rows, 8) : NCX_COLSUM_CHUNKS;
        hipLaunchKernelGGL(k_colsum_partial, dim3((unsigned)cdiv(cols, 256), ch), dim3(256), 0, s, x, wgt, rows, cols, partial);
        hipLaunchKernelGGL(k_colsum_finish, dim3((unsigned)cdiv(cols, 8)), dim3(256), 0, s, (const float*)partial, ch, cols, out);
        return (int)hipGetLastError();
    };

    // ---- out layer + last hidden layer's activation ------------------------------------------------
    const float* hL = (const float*)(ws + w.h[d.L - 1]);
    float* dpre = (float*)(ws + w.dpre[0]);
    const bool only_de = phase == 4;                    // phase 4: just the dE GEMM
    const bool skip_de = phase == 3 || phase == 5;
    const bool do1 = phase != 2 && !only_de, do2 = phase != 1 && phase != 5 && !only_de;
    // The dE product skips the dGgt^T segment of the row tiles without an answer of THIS batch where the call that scatters dSh also runs the
    // product (the one-call backward and phase 1).  Phases 3 | 4 and 5 | 2 | 4 keep the full form: between them a data-parallel job sums
    // the dGt^T | dGgt^T block over ranks, so it carries other batches' answers.
    const bool de_skip = r.de_skip && (phase == 0 || phase == 1);
    int* const de_perm = (int*)(ws + w.de_perm);
    if (!do1) {                                       // phase 2: dpre_1 lives where phase 1 left it
        dpre = (float*)(ws + w.dpre[(d.L - 1) & 1]);
    } else if (d.flags & NCX_F_FUSED_TAIL) {
        // ncx_train_tail has produced dpre_L, dSh and the out-layer / linear_1.bias gradients
    } else {
        // one pass: dpre_L, d out.weight / d out.bias partials, and for L == 1 also dSh + d linear_1.bias partials
        const int nblk = (int)cdiv(d.B < NCX_PRELUDE_WAVES ? d.B : NCX_PRELUDE_WAVES, 4);      // one wave per run of triplets
        float* part_w = partial;
        float* part_b1 = partial + (size_t)NCX_PRELUDE_WAVES * H;
        float* part_b = partial + (size_t)NCX_PRELUDE_WAVES * H * 2;
        const bool fuse_l1 = d.L == 1;
        hipLaunchKernelGGL(k_bwd_prelude, dim3(nblk), dim3(256), 0, s, dscores, p->w_out, hL, dpre, fuse_l1 ? dsh : (float*)nullptr,
                           d.B, d.K, H, dscale, part_w, part_b1, part_b,
                           emb_nt ? dagtT : aemb ? dagt : (float*)nullptr, emb_nt ? (long long)d.A * Hp4 : (long long)H * d.A);
        NCX_HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_bwd_prelude_finish, dim3((unsigned)cdiv(H, 8), fuse_l1 ? 2 : 1), dim3(256), 0, s, (const float*)part_w,
                           (const float*)part_b1, (const float*)part_b, nblk * 4, H, g->w_out, fuse_l1 ? g->b1 : (float*)nullptr, g->b_out);
        NCX_HIP_TRY(hipGetLastError());
    }
    // ---- hidden layers L..2 ---------------------------------------------------------------------------
    int cur = 0;
    for (int l = d.L; l >= 2 && do1; --l) {
        const float* wl = l == 2 ? p->w2 : p->w3;
        float* gw = l == 2 ? g->w2 : g->w3;
        float* gb = l == 2 ? g->b2 : g->b3;
        const float* hprev = (const float*)(ws + w.h[l - 2]);
        rc = colsum(dpre, nullptr, M, H, gb); if (rc) return rc;
        {   // dW_l[n][k] = sum_r dpre[r][n] h_{l-1}[r][k]
            GemmArgs a{}; a.mode = MODE_GROUP; a.nseg = 1; a.M = H;
            a.a[0] = x_plain(dpre, H, M, H); a.b[0] = x_plain(hprev, H, M, H); a.klen[0] = M;
            a.out[0] = gw; a.ldo[0] = H; a.n_cols[0] = H;
            rc = run_gemm(U_DWL, a, FORM_TN, u[U_DWL].plan, slab, w.slab_bytes, nullptr, s); if (rc) return rc;
        }
        {   // dpre_{l-1} = (dpre_l . W_l) * gate(h_{l-1})
            float* dnext = (float*)(ws + w.dpre[cur ^ 1]);
            GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = M;
            a.a[0] = x_plain(dpre, H, M, H); a.b[0] = x_plain(wl, H, H, H); a.klen[0] = H;
            a.out[0] = dnext; a.ldo[0] = H; a.n_cols[0] = H;
            a.epi.gate = hprev; a.epi.ld_gate = H; a.epi.gate_scale = dscale;
            rc = run_gemm(U_DXL, a, FORM_NN, u[U_DXL].plan, slab, w.slab_bytes, nullptr, s); if (rc) return rc;
            dpre = dnext; cur ^= 1;
        }
    }
    // ---- layer 1 ---------------------------------------------------------------------------------------
    if (do1 && d.L >= 2) {                              // (L == 1: already produced by k_bwd_prelude)
        hipLaunchKernelGGL(k_rowgroup_sum, dim3((unsigned)cdiv((long long)d.B * H, 256)), dim3(256), 0, s, (const float*)dpre, d.B, d.K, H, dsh);
        NCX_HIP_TRY(hipGetLastError());
        rc = colsum(dsh, nullptr, d.B, H, g->b1); if (rc) return rc;
    }
    bool km_deferred = false, km_reduced = false;
    auto run_km = [&](bool finish = true) -> int {
        return profiled(U_DW1C, s, [&] { return dw_km(d, dpre, in->feats, idx_k, idx_o, (float*)(ws + w.km_slab), g->w1 + o.v_other, g->w1 + o.v_mult, din, s, finish); });
    };
    {   // dW1 = [dpre^T . candidate segments (+ dGt) | dSh^T . shared segments]: ONE grouped launch, per-problem
        // reduction extent (M rows of dpre vs B rows of dSh) and k-split
        GemmArgs a{}; a.mode = MODE_GROUP; a.M = H;
        int n = 0;
        auto add_c = [&](const XDesc& x, float* out, long long ldo) {
            a.a[n] = x_plain(dpre, H, M, H); a.b[n] = x; a.klen[n] = M; a.out[n] = out; a.ldo[n] = ldo; a.n_cols[n] = x.cols;
            a.split[n] = dw1c_seg_split(x.cols, u[U_DW1C].plan.split, u[U_DW1C].ksteps); ++n; };
        auto add_s = [&](const XDesc& x, float* out) {
            a.a[n] = x_plain(dsh, H, d.B, H); a.b[n] = x; a.klen[n] = d.B; a.out[n] = out; a.ldo[n] = din; a.n_cols[n] = x.cols;
            a.split[n] = u[U_DW1S].plan.split; ++n; };
        // the dGt problem is what the answer_embedding gradient waits for: phase 1 launches it alone
        const bool bf16 = d.flags & NCX_F_BF16;
        const bool want_dgt = aemb && do1 && !bf16, want_rest = do2;
        if (bf16 && do1) {   // all candidate columns + dGt: dpre^T . Xc on the bf16 MFMA path (complete in phases 0, 1, 3)
            rc = profiled(U_DW1C, s, [&] { return bf16_dw1c(d, dpre, (u16*)(ws + w.dpre_bf), (const u16*)(ws + w.xc), (float*)(ws + w.bf_slab), g->w1, dgt, s); }); if (rc) return rc;
        }
        const bool km = r.km;
        const bool tn8 = r.tn8;               // dGt + every column block that is not the per-triplet fold's: ONE balanced launch (ncx_dwtn.hip)
        // With the side stream the per-triplet fold kernel (a full round of long workgroups) is launched AFTER the grouped
        // launch, next to the answer-embedding chain (dW1ak, dE: short latency-bound workgroups) that waits for dGt.
        km_deferred = want_rest && do1 && do2 && km_defers_to_side_stream(d, r);
        // the sums over its k-chunk partials ride in one launch with the split fix-up of the grouped GEMM below
        const bool km_merge = want_rest && km && !km_deferred && !hook_env("NCX_NO_MERGE_FIX");
        if (want_rest && km && !km_deferred) {      // v_other and v_mult columns in one MFMA pass (per-triplet fold)
            rc = run_km(!km_merge); if (rc) return rc;
        }
        if (want_rest && !bf16 && !km) {
            add_c(x_gather(in->feats, d.dv, idx_k, M, d.dv), g->w1 + o.v_other, din);
            if (d.flags & NCX_F_V_MULT) add_c(x_gather_mul(in->feats, d.dv, idx_k, idx_o, M, d.dv), g->w1 + o.v_mult, din);
        }
        if (tn8 && (want_dgt || want_rest)) {
            // The problem list is the same in every phase (the chunking of the dGt part and of the rest do not depend on each other,
            // and the slab slots are numbered over the whole list): phases 5 | 2 launch its two parts separately, bit-identically.
            Tn8Prob tp[TN8_MAX_PROB]; int np = 0, n_al = 0;
            auto prob = [&](const float* A_, int rows, const float* X, long long ldx, const float* lse, int gsel, int N, float* out, long long ldo, int n_valid) {
                tp[np] = Tn8Prob{};
                Tn8Prob& q = tp[np++]; q.A = A_; q.rows = rows; q.X = X; q.ldx = ldx; q.lse = lse; q.gsel = gsel; q.N = N; q.out = out; q.ldo = ldo; q.n_valid = n_valid; };
            if (aemb) {
                prob(dpre, M, in->a_knns, d.A, mx, 0, d.A, dgt, d.A, d.A); n_al = 1;
                if (emb_nt) {       // the reduction also writes dGt^T (what the dE product and the DP exchange read) and a private copy with
                    // zero rows up to a multiple of 32 (the A operand of the dW1[:, a_other] = dGt . E launch below)
                    tp[0].outT = dgtT; tp[0].outT2 = (float*)(ws + w.dgtT2); tp[0].ldT = Hp4; tp[0].padT2 = pad_to(d.A, 32) - d.A;
                }
            }
            else prob(dpre, M, in->a_knns, d.da, nullptr, 0, d.da, g->w1 + o.a_other, din, d.da);
            prob(dpre, M, in->z_knns, d.dz, nullptr, 0, d.dz, g->w1 + o.z_other, din, d.dz);
            prob(dpre, M, misc, w.ldm, nullptr, 0, w.ldm, g->w1 + o.v_dist, din, d.K + 1);
            prob(dsh, d.B, in->feats, d.dv, nullptr, 1, d.dv, g->w1 + o.v_orig, din, d.dv);
            prob(dsh, d.B, in->q_emb, d.dq, nullptr, 0, d.dq, g->w1 + o.q_emb, din, d.dq);
            prob(dsh, d.B, in->z_orig, d.dz, nullptr, 0, d.dz, g->w1 + o.z_orig, din, d.dz);
            if (aemb) prob(dsh, d.B, p->answer_embedding, d.da, nullptr, 2, d.da, g->w1 + o.a_gt, din, d.da);
            else      prob(dsh, d.B, in->a_emb_gt, d.da, nullptr, 0, d.da, g->w1 + o.a_gt, din, d.da);
            // ... and ONE launch sums its partial tiles and the fold kernel's k-chunks (when that kernel ran just above)
            const bool with_km = want_rest && km && !km_deferred && km_merge;
            Tn8ReduceArgs red{};
            rc = prof_open(U_DW1C, s); if (rc) return rc;
            rc = dw_tn8_products(d, tp, np, n_al, want_dgt, want_rest, idx_ob, aemb ? in->answer_aids : nullptr, slab, w.slab_bytes, &red, s); if (rc) return rc;
            bool kvec = true;
            KmReduceArgs kr{};
            if (with_km) { kr = dw_km_reduce_args(d, (const float*)(ws + w.km_slab), g->w1 + o.v_other, g->w1 + o.v_mult, din, &kvec); km_reduced = true; }
            rc = dw_reduce_km_tn8(with_km ? &kr : nullptr, kvec, &red, s); if (rc) return rc;
            rc = prof_close(U_DW1C, s); if (rc) return rc;
        }
        if (want_rest && !bf16 && !tn8) {
            if (!aemb) add_c(x_plain(in->a_knns, d.da, M, d.da), g->w1 + o.a_other, din);
        }
        if (want_dgt && !tn8) add_c(x_softmax(in->a_knns, d.A, mx, inv, M, d.A), dgt, d.A);
        if (want_rest && !bf16 && !tn8) {      // the narrow problems last among the candidate ones (shorter k-chunks: see dw1c_seg_split)
            add_c(x_plain(in->z_knns, d.dz, M, d.dz), g->w1 + o.z_other, din);
            add_c(x_plain(misc, w.ldm, M, d.K + 1), g->w1 + o.v_dist, din);
        }
        if (want_rest && bf16 && r.tn8_shared) {      // bf16 variant: the fp32 shared segments' weight gradient on the balanced TN kernel
            Tn8Prob tp[4]; int np = 0;
            auto prob = [&](const float* X, long long ldx, int gsel, int N, float* out) {
                tp[np] = Tn8Prob{};
                Tn8Prob& q = tp[np++]; q.A = dsh; q.rows = d.B; q.X = X; q.ldx = ldx; q.gsel = gsel; q.N = N; q.out = out; q.ldo = din; q.n_valid = N; };
            prob(in->feats, d.dv, 1, d.dv, g->w1 + o.v_orig);
            prob(in->q_emb, d.dq, 0, d.dq, g->w1 + o.q_emb);
            prob(in->z_orig, d.dz, 0, d.dz, g->w1 + o.z_orig);
            if (aemb) prob(p->answer_embedding, d.da, 2, d.da, g->w1 + o.a_gt);
            else      prob(in->a_emb_gt, d.da, 0, d.da, g->w1 + o.a_gt);
            rc = dw_tn8(d, tp, np, 0, false, true, idx_ob, aemb ? in->answer_aids : nullptr, slab, w.slab_bytes, s); if (rc) return rc;
        } else
        if (want_rest && !tn8) {
            add_s(x_gather(in->feats, d.dv, idx_ob, d.B, d.dv), g->w1 + o.v_orig);
            add_s(x_plain(in->q_emb, d.dq, d.B, d.dq), g->w1 + o.q_emb);
            add_s(x_plain(in->z_orig, d.dz, d.B, d.dz), g->w1 + o.z_orig);
            add_s(aemb ? x_gather(p->answer_embedding, d.da, in->answer_aids, d.B, d.da) : x_plain(in->a_emb_gt, d.da, d.B, d.da),
                  g->w1 + o.a_gt);
        }
        a.nseg = n;
        FixupArgs fix_tn{};
        if (km_merge) a.defer_fix = &fix_tn;
        if (n > 0) { rc = run_gemm(U_DW1C, a, FORM_TN, u[U_DW1C].plan, slab, w.slab_bytes, nullptr, s); if (rc) return rc; }
        if (km_merge && !km_reduced) {
            rc = profiled(U_DW1C, s, [&] { return dw_km_finish(d, (const float*)(ws + w.km_slab), g->w1 + o.v_other, g->w1 + o.v_mult, din, &fix_tn, u[U_DW1C].plan.cfg, s); }); if (rc) return rc;
        }
        if (!(d.flags & NCX_F_V_MULT) && do2) {
            hipLaunchKernelGGL(k_zero_cols, dim3((unsigned)cdiv((long long)H * d.dv, 256)), dim3(256), 0, s, g->w1 + o.v_mult, H, din, d.dv);
            NCX_HIP_TRY(hipGetLastError());
        }
    }
    if (aemb) {
        // The consumers of dGt (dW1[:, a_other] = dGt . E, then dE) form a chain of short launches: with the side stream they
        // run there (own slab) while the caller's stream runs the per-triplet fold kernel
        SideStream* ss = km_deferred ? side_stream() : nullptr;
        hipStream_t se = ss ? ss->s : s;
        FixupArgs fix_ak{};
        Tn8ReduceArgs red_ak{};
        const bool tn8_ak = r.dw1ak_on_tn8(ss != nullptr);
        if (ss) { rc = side_fork(ss, s); if (rc) return rc; }
        const bool bf16e = d.flags & NCX_F_BF16;
        const Bf16Emb bm = bf16e ? bf16_emb_layout(d, ws + w.bf_emb) : Bf16Emb{};
        if (do2 && bf16e) {
            rc = profiled(U_DW1AK, se, [&] { return bf16_dw1ak(d, bm, dgt, g->w1, se); }); if (rc) return rc;
        } else if (do2 && tn8_ak) {   // dW1[:, a_other][n][j] = sum_a dGt^T[a][n] E[a][j]: a row-reduction over the A answers on the 8-wave TN kernel
            // (round 4; NN form on the generic engine: 39 us + fix-up for 2.46 GF).  Its A operand is the PRIVATE copy of dGt^T: under data
            // parallelism the other copy is being summed over ranks in place while this runs.
            Tn8Prob q{};
            q.A = (const float*)(ws + w.dgtT2); q.rows = pad_to(d.A, 32); q.rows_valid = d.A; q.X = p->answer_embedding; q.ldx = d.da; q.N = d.da;
            q.out = g->w1 + o.a_other; q.ldo = din; q.n_valid = d.da;
            rc = prof_open(U_DW1AK, se); if (rc) return rc;
            rc = dw_tn8_products(d, &q, 1, 0, false, true, nullptr, nullptr, slab, w.slab_bytes, &red_ak, se); if (rc) return rc;
            if (!(do1 && emb_nt)) { rc = dw_reduce_km_tn8(nullptr, true, &red_ak, se); if (rc) return rc; red_ak.n_tiles_total = 0; }   // (else: rides in k_emb_prep's launch)
            rc = prof_close(U_DW1AK, se); if (rc) return rc;
        } else if (do2) {   // dW1[:, a_other][n][j] = sum_a dGt[n][a] E[a][j]
            GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = H;
            a.a[0] = x_plain(dgt, d.A, H, d.A); a.b[0] = x_plain(p->answer_embedding, d.da, d.A, d.da); a.klen[0] = d.A;
            a.out[0] = g->w1 + o.a_other; a.ldo[0] = din; a.n_cols[0] = d.da;
            if (do1 && emb_nt && u[U_DW1AK].plan.cfg == CFG_64x64 && !hook_env("NCX_NO_MERGE_FIX")) a.defer_fix = &fix_ak;
            rc = run_gemm(U_DW1AK, a, FORM_NN, u[U_DW1AK].plan, ss ? (float*)(ws + w.slab2) : slab,
                          ss ? w.slab2_bytes : w.slab_bytes, nullptr, se); if (rc) return rc;
        }
        if (do1 && emb_nt) {   // dGgt^T, dGt^T and the transposed weight slices for the NT embedding gradient
            EmbPrepArgs ea{};
            ea.dsh = dsh; ea.aid = in->answer_aids; ea.dggtT = dagtT; ea.B = d.B; ea.H = H; ea.A = d.A; ea.Hp4 = Hp4;
            const float* srcs[3] = {dgt, p->w1 + o.a_other, p->w1 + o.a_gt};
            float* dsts[3] = {dgtT, w1akT, w1agtT};
            const long long ldss[3] = {d.A, din, din};
            const int colss[3] = {tn8_ak ? 0 : d.A, d.da, d.da}, ldds[3] = {Hp4, Hp32, Hp32};      // (tn8: dGt^T came out of the reduction)
            int tiles = 0;
            for (int e = 0; e < 3; ++e) {
                ea.src[e] = srcs[e]; ea.dst[e] = dsts[e]; ea.lds_[e] = ldss[e]; ea.cols[e] = colss[e]; ea.ldd[e] = ldds[e]; ea.dcols[e] = ldds[e];
                ea.tile0[e] = tiles; tiles += ((ldds[e] + 31) / 32) * ((colss[e] + 31) / 32);
            }
            ea.tile0[3] = tiles;
            ea.perm = de_skip ? de_perm : (int*)nullptr;
            // (the dW1[:, a_other] GEMM above left its split fix-up to this launch)
            hipLaunchKernelGGL(k_emb_prep, dim3((de_skip ? 1 : 0) + d.B + tiles + (fix_ak.valid ? fix_ak.grid_x * 4 : 0) + red_ak.n_tiles_total * 8), dim3(256), 0, se, ea, fix_ak, red_ak);
            fix_ak.valid = 0; red_ak.n_tiles_total = 0;
            NCX_HIP_TRY(hipGetLastError());
        } else if (do1) {   // dGgt = one-hot(aid)^T dSh   (dGgt was cleared by k_bwd_prelude)
            hipLaunchKernelGGL(k_scatter_dsh_by_answer, dim3(d.B), dim3(256), 0, se, (const float*)dsh, in->answer_aids, d.B, H, d.A, dagt);
            NCX_HIP_TRY(hipGetLastError());
        }
        if (fix_ak.valid) { rc = run_fixup2(fix_ak, FixupArgs{}, CFG_64x64, se); if (rc) return rc; }      // (not picked up above)
        if (((do1 && !skip_de) || only_de) && bf16e) {
            rc = profiled(U_DE, se, [&] { return bf16_de(d, bm, dgt, g->answer_embedding, se); }); if (rc) return rc;
        } else if (((do1 && !skip_de) || only_de) && emb_nt) {   // dE = dGt^T . (W1ak^T)^T + dGgt^T . (W1agt^T)^T on the fused forward kernel
            MainArgs a{}; a.M = d.A; a.N = d.da; a.nseg = 2;
            a.seg[0].kind = MK_PLAIN; a.seg[0].a = dgtT;  a.seg[0].lda = Hp4; a.seg[0].klen = Hp4; a.seg[0].b = w1akT;  a.seg[0].ldb = Hp32;
            a.seg[1].kind = MK_PLAIN; a.seg[1].a = dagtT; a.seg[1].lda = Hp4; a.seg[1].klen = Hp4; a.seg[1].b = w1agtT; a.seg[1].ldb = Hp32;
            a.out = g->answer_embedding; a.ldo = d.da;
            a.split = 1;
            if (de_skip) {      // rows in the order of de_perm: dGgt^T has a non-zero row only for an answer of the batch, and those come first
                a.seg[0].kind = MK_GATHER; a.seg[0].idx = de_perm;
                a.seg[1].kind = MK_GATHER; a.seg[1].idx = de_perm;
            }
            // Nothing below reads a weight, and with no side stream every other gradient is final on this stream: g->w1 (the fold kernel, the TN
            // launch and their reduction; the a_other block's reduction or fix-up in k_emb_prep's launch or just above), the biases, the hidden
            // and out layers.  The product reads the workspace copies k_emb_prep made (W1ak^T, W1agt^T), never p->w1 or p->answer_embedding.
            if (adam && phase == 0 && !ss) {
                a.adam = *adam;
                rc = profiled(U_DE, se, [&] { return main_forward_adam(a, de_skip, se); }); if (rc) return rc;
                if (adam_done) *adam_done = true;
            } else {
            rc = profiled(U_DE, se, [&] { return de_skip ? main_forward_rowmap(a, se) : main_forward(a, se); }); if (rc) return rc;
            }
        } else if ((do1 && !skip_de) || only_de) {   // dE[a][j] = sum_n dGt[n][a] W1ak[n][j] + sum_n dGgt[n][a] W1agt[n][j]
            GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 2; a.M = d.A;
            a.a[0] = x_plain(dgt, d.A, H, d.A);  a.b[0] = x_plain(p->w1 + o.a_other, din, H, d.da); a.klen[0] = H;
            a.a[1] = x_plain(dagt, d.A, H, d.A); a.b[1] = x_plain(p->w1 + o.a_gt, din, H, d.da);    a.klen[1] = H;
            a.out[0] = g->answer_embedding; a.ldo[0] = d.da; a.n_cols[0] = d.da;
            rc = run_gemm(U_DE, a, FORM_TN, u[U_DE].plan, ss ? (float*)(ws + w.slab2) : slab, ss ? w.slab2_bytes : w.slab_bytes, nullptr, se); if (rc) return rc;
        }
        if (km_deferred) { rc = run_km(); if (rc) return rc; }
        if (ss) { rc = side_join(ss, s); if (rc) return rc; }
    } else if (do1) {
        NCX_HIP_TRY(hipMemsetAsync(g->answer_embedding, 0, (size_t)d.A * d.da * 4, s));
    }
    return NCX_OK;
}

int ncx_backward(const ncx_dims* dp, const ncx_inputs* in, const ncx_params* p, void* workspace,
                 size_t workspace_bytes, const float* dscores, const ncx_grads* g, void* stream_) {
    return backward_impl(dp, in, p, workspace, workspace_bytes, dscores, g, stream_, 0);
}

int ncx_backward_adam(const ncx_dims* dp, const ncx_inputs* in, const ncx_params* p, void* workspace, size_t workspace_bytes,
                      const float* dscores, const ncx_grads* g, const ncx_adam_state* opt, void* stream_) {
    int rc = check_dims(dp);
    if (rc != NCX_OK) return rc;
    if (!in || !p || !g || !opt || !opt->param || !opt->grad || !opt->exp_avg || !opt->exp_avg_sq) return NCX_E_NULL;
    if (!p->answer_embedding || !g->answer_embedding) return NCX_E_NULL;
    const ncx_dims& d = *dp;
    const size_t n = opt->n, n_emb = opt->n_emb, emb = (size_t)d.A * d.da;
    if (opt->step < 1 || n == 0 || n_emb > n || n_emb < emb) return NCX_E_DIMS;
    if (((uintptr_t)opt->param | (uintptr_t)opt->grad | (uintptr_t)opt->exp_avg | (uintptr_t)opt->exp_avg_sq) & 15) return NCX_E_WORKSPACE;
    // answer_embedding leads both flat buffers; every other tensor of the model lies behind it, inside them
    if (p->answer_embedding != opt->param || g->answer_embedding != opt->grad) return NCX_E_DIMS;
    const SegOffsets o = seg_offsets(d);
    const size_t H = (size_t)d.H;
    auto inside = [&](const float* x, const float* base, size_t count) { return !x || (x >= base + n_emb && x + count <= base + n); };
    const float* const pf[8] = {p->w1, p->b1, p->w2, p->b2, p->w3, p->b3, p->w_out, p->b_out};
    const float* const gf[8] = {g->w1, g->b1, g->w2, g->b2, g->w3, g->b3, g->w_out, g->b_out};
    const size_t cnt[8] = {H * (size_t)o.din, H, H * H, H, H * H, H, H, 1};
    for (int i = 0; i < 8; ++i) {
        const bool used = i < 2 || i >= 6 || (d.L >= 2 && i < 4) || d.L >= 3;
        if (!used) continue;
        if (!inside(pf[i], opt->param, cnt[i]) || !inside(gf[i], opt->grad, cnt[i])) return NCX_E_DIMS;
    }
    const AdamScalars sc = adam_scalars(opt->lr, opt->beta1, opt->beta2, opt->eps, opt->step, opt->grad_scale);
    AdamFuse af{};
    // (the tile epilogue covers exactly the A x da elements, the passengers the rest: the embedding slice has no padding behind it)
    const bool want = fused_adam_route(d, routes(d)) && n_emb == emb && emb % 4 == 0;
    if (want) {
        af.p = opt->param; af.m = opt->exp_avg; af.v = opt->exp_avg_sq;
        af.tp = opt->param + n_emb; af.tg = opt->grad + n_emb; af.tm = opt->exp_avg + n_emb; af.tv = opt->exp_avg_sq + n_emb;
        af.tn = n - n_emb; af.s = sc;
    }
    bool done = false;
    rc = backward_impl(dp, in, p, workspace, workspace_bytes, dscores, g, stream_, 0, want ? &af : nullptr, &done);
    if (rc != NCX_OK || done) return rc;
    return adam_launch(opt->param, opt->grad, opt->exp_avg, opt->exp_avg_sq, n, sc, (hipStream_t)stream_);
}

int ncx_backward_phase(const ncx_dims* dp, const ncx_inputs* in, const ncx_params* p, void* workspace,
                       size_t workspace_bytes, const float* dscores, const ncx_grads* g, int32_t phase, void* stream_) {
    if (phase < 0 || phase > 5) return NCX_E_FLAGS;
    return backward_impl(dp, in, p, workspace, workspace_bytes, dscores, g, stream_, phase);
}

int ncx_ws_region(const ncx_dims* dp, int32_t which, size_t* offset, size_t* bytes) {
    if (check_dims(dp) != NCX_OK) return NCX_E_DIMS;
    if (!offset || !bytes) return NCX_E_NULL;
    if (which != NCX_WS_DGT && which != NCX_WS_H1 && which != NCX_WS_DPRE1 && which != NCX_WS_DE_PERM && which != NCX_WS_H2 && which != NCX_WS_H3 &&
        which != NCX_WS_DPRE2 && which != NCX_WS_XC && which != NCX_WS_WC && which != NCX_WS_GT) return NCX_E_FLAGS;
    const StepRoutes r = routes(*dp);
    const WsLayout w = ws_layout(*dp, r);
    if (which == NCX_WS_XC || which == NCX_WS_WC) {      // (size 0 without NCX_F_BF16: the fp32 path packs no operands)
        const bool bf16 = dp->flags & NCX_F_BF16;
        *offset = which == NCX_WS_XC ? w.xc : w.wc;
        *bytes = !bf16 ? 0 : which == NCX_WS_XC ? bf16_xc_bytes(*dp) : bf16_wc_bytes(*dp);
        return NCX_OK;
    }
    if (which == NCX_WS_GT) {      // [H][ldgt] (ws_layout: A under NCX_F_BF16, else pad_to(A, 32))
        *offset = w.gt; *bytes = (size_t)dp->H * w.ldgt * 4;
        return NCX_OK;
    }
    if (which == NCX_WS_DE_PERM) {      // (size 0: the shape or the variant keeps the full form of the product)
        *offset = w.de_perm; *bytes = r.de_skip ? ((size_t)dp->A + 1) * 4 : 0;
        return NCX_OK;
    }
    if (which == NCX_WS_H2 || which == NCX_WS_H3) {      // (size 0: the model has no such layer)
        const int l = which == NCX_WS_H2 ? 2 : 3;
        *offset = w.h[l - 1]; *bytes = dp->L >= l ? (size_t)dp->B * dp->K * dp->H * 4 : 0;
        return NCX_OK;
    }
    if (which == NCX_WS_DPRE2) {      // (L == 2: dpre_2 stays in the first ping-pong buffer, dpre_1 goes to the second)
        *offset = w.dpre[0]; *bytes = dp->L == 2 ? (size_t)dp->B * dp->K * dp->H * 4 : 0;
        return NCX_OK;
    }
    if (which == NCX_WS_H1 || which == NCX_WS_DPRE1) {
        *offset = which == NCX_WS_H1 ? w.h[0] : w.dpre[(dp->L - 1) & 1];
        *bytes = (size_t)dp->B * dp->K * dp->H * 4;
        return NCX_OK;
    }
    // the block a DP job sums between phases 5 / 3 and 4 is the one backward_impl fills: the same predicate decides its form
    if (!r.emb_nt) { *offset = w.dgt; *bytes = (dp->flags & NCX_F_A_EMB) ? (size_t)2 * dp->H * dp->A * 4 : 0; }               // dGt | dGgt, [H][A] x 2
    else { *offset = w.dgtT; *bytes = (size_t)2 * dp->A * pad_to(dp->H, 4) * 4; }                                                     // dGt^T | dGgt^T, [A][pad4(H)] x 2
    return NCX_OK;
}
}  // extern "C"
