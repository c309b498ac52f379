// ncx_loss_adam.hip -- the losses and the optimiser every model shares: the scorers' listwise loss / rank (ncx_loss_rank), the VQA
// trainers' cross-entropy over the answers (ncx_ce_loss) and the Adam update (ncx_adam_step).
#include "ncx_wave.h"
#include "ncx_adam.h"

namespace ncx {
// Listwise softmax cross-entropy over the K candidates of a triplet + rank of the ground truth.
// One wave per triplet, lane k holds score k (K <= 64).
__global__ __launch_bounds__(256) void k_loss_rank(const float* __restrict__ scores, const int* __restrict__ gt,
                                                   int B, int K, float scale, float* __restrict__ loss_rows,
                                                   float* __restrict__ dscores, int* __restrict__ rank) {
    const int lane = threadIdx.x & 63;
    const int b = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (b >= B) return;
    const float s = lane < K ? scores[(long long)b * K + lane] : -INFINITY;
    const int g = gt[b];
    const float m = wave_max(s);
    const float e = lane < K ? __expf(s - m) : 0.f;
    const float sum = wave_sum(e);
    const float sg = __shfl(s, g, 64);
    if (dscores && lane < K) dscores[(long long)b * K + lane] = (e / sum - (lane == g ? 1.f : 0.f)) * scale;
    const bool ahead = lane < K && (s > sg || (s == sg && lane < g));
    const unsigned long long bal = __ballot(ahead);
    if (lane == 0) {
        if (loss_rows) loss_rows[b] = (logf(sum) - (sg - m)) * scale;      // (sg - m first: log(sum) + m would round at the magnitude of the scores, not of the loss)
        if (rank) rank[b] = __popcll(bal);
    }
}

// loss = sum(loss_rows); hits = {#rank<1, #rank<5}.  Single block: deterministic.
__global__ __launch_bounds__(256) void k_loss_finish(const float* __restrict__ loss_rows, const int* __restrict__ rank,
                                                     int B, float* __restrict__ loss, int* __restrict__ hits) {
    __shared__ float sl[4];
    __shared__ int s1[4], s5[4];
    float acc = 0.f; int h1 = 0, h5 = 0;
    for (int i = threadIdx.x; i < B; i += 256) {
        if (loss_rows) acc += loss_rows[i];
        if (rank) { const int rk = rank[i]; h1 += rk < 1; h5 += rk < 5; }
    }
    acc = wave_sum(acc);
    h1 = (int)wave_sum((float)h1); h5 = (int)wave_sum((float)h5);
    const int w = threadIdx.x >> 6;
    if ((threadIdx.x & 63) == 0) { sl[w] = acc; s1[w] = h1; s5[w] = h5; }
    __syncthreads();
    if (threadIdx.x == 0) {
        if (loss) loss[0] = sl[0] + sl[1] + sl[2] + sl[3];
        if (hits) { hits[0] = s1[0] + s1[1] + s1[2] + s1[3]; hits[1] = s5[0] + s5[1] + s5[2] + s5[3]; }
    }
}

// Mean cross-entropy over A answers (the loss of the three VQA trainers): one workgroup per example.  rows[b] = CE_b scale,
// rows[B + b] (as int) = hit bits (1: top-1, 2: top-5).
__device__ __forceinline__ float ce_block_max(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return fmaxf(fmaxf(red[0], red[1]), fmaxf(red[2], red[3]));
}
__device__ __forceinline__ float ce_block_sum(float v, float* red) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    __syncthreads();
    if ((threadIdx.x & 63) == 0) red[threadIdx.x >> 6] = v;
    __syncthreads();
    return (red[0] + red[1]) + (red[2] + red[3]);
}
__global__ __launch_bounds__(256) void k_ce_rows(const float* __restrict__ logits, const int* __restrict__ target, int B, int A, float scale,
                                                 float* __restrict__ dlogits, float* __restrict__ rows, int* __restrict__ bad) {
    __shared__ float red[4];
    const int b = blockIdx.x, t = threadIdx.x;
    const float* x = logits + (long long)b * A;
    const int tg = target[b];
    const bool ok = tg >= 0 && tg < A;
    if (!ok) {                                           // never used as an address: the row contributes nothing
        if (t == 0) { *bad = 1; rows[b] = 0.f; ((int*)rows)[B + b] = 0; }
        if (dlogits) for (int c = t; c < A; c += 256) dlogits[(long long)b * A + c] = 0.f;
        return;
    }
    const float xt = x[tg];
    float mx = -INFINITY; int ahead = 0;
    for (int c = t; c < A; c += 256) {
        const float v = x[c];
        mx = fmaxf(mx, v);
        ahead += (v > xt || (v == xt && c < tg)) ? 1 : 0;
    }
    mx = ce_block_max(mx, red);
    float se = 0.f;
    for (int c = t; c < A; c += 256) se += __expf(x[c] - mx);
    se = ce_block_sum(se, red);
    const int rank = (int)ce_block_sum((float)ahead, red);
    if (dlogits) {
        const float inv = 1.f / se;
        for (int c = t; c < A; c += 256) dlogits[(long long)b * A + c] = (__expf(x[c] - mx) * inv - (c == tg ? 1.f : 0.f)) * scale;
    }
    if (t == 0) {
        rows[b] = (logf(se) - (xt - mx)) * scale;              // (xt - mx first: the row's offset never meets the small log term)
        ((int*)rows)[B + b] = (rank < 1 ? 1 : 0) | (rank < 5 ? 2 : 0);
    }
}
// loss = sum_b rows[b]; the hit counts: single workgroup, fixed order
__global__ __launch_bounds__(256) void k_ce_finish(const float* __restrict__ rows, int B, float* __restrict__ loss, int* __restrict__ h1,
                                                   int* __restrict__ h5) {
    __shared__ float red[4];
    float acc = 0.f, c1 = 0.f, c5 = 0.f;
    for (int i = threadIdx.x; i < B; i += 256) {
        acc += rows[i];
        const int bits = ((const int*)rows)[B + i];
        c1 += (float)(bits & 1); c5 += (float)((bits >> 1) & 1);
    }
    acc = ce_block_sum(acc, red); c1 = ce_block_sum(c1, red); c5 = ce_block_sum(c5, red);
    if (threadIdx.x == 0) {
        if (loss) loss[0] = acc;
        if (h1) h1[0] = (int)c1;
        if (h5) h5[0] = (int)c5;
    }
}

// torch.optim.Adam on a flat buffer: the update itself is adam_update (ncx_adam.h), shared with the launch that applies it where the
// answer-embedding gradient is produced.
__global__ __launch_bounds__(256) void k_adam(float* __restrict__ p, const float* __restrict__ g, float* __restrict__ m,
                                              float* __restrict__ v, size_t n, const AdamScalars s) {
    size_t i = ((size_t)blockIdx.x * 256 + threadIdx.x) * 4;
    const size_t stride = (size_t)gridDim.x * 256 * 4;
    for (; i < n; i += stride) {
        if (i + 3 < n) adam_quad(p, g, m, v, i, s);
        else adam_tail(p, g, m, v, i, n, s);
    }
}

int adam_launch(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, const AdamScalars& s, hipStream_t stream) {
    size_t blocks = (n + 1023) / 1024;
    if (blocks > 4096) blocks = 4096;
    hipLaunchKernelGGL(k_adam, dim3((unsigned)blocks), dim3(256), 0, stream, param, grad, exp_avg, exp_avg_sq, n, s);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
}  // namespace ncx

using namespace ncx;
extern "C" {
int ncx_loss_rank(const float* scores, const int32_t* gt, int32_t B, int32_t K, float scale, float* loss_rows,
                  float* loss, float* dscores, int32_t* rank, int32_t* hits, void* stream_) {
    if (!scores || !gt) return NCX_E_NULL;
    if (B < 1 || K < 1 || K > 64) return NCX_E_DIMS;
    if ((loss && !loss_rows) || (hits && !rank)) return NCX_E_NULL;
    hipStream_t s = (hipStream_t)stream_;
    if (scale <= 0.f) scale = 1.f / (float)B;
    hipLaunchKernelGGL(k_loss_rank, dim3((unsigned)cdiv(B, 4)), dim3(256), 0, s, scores, gt, B, K, scale, loss_rows, dscores, rank);
    NCX_HIP_TRY(hipGetLastError());
    if (loss || hits) {
        hipLaunchKernelGGL(k_loss_finish, dim3(1), dim3(256), 0, s, (const float*)loss_rows, (const int*)rank, B, loss, hits);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}

int ncx_ce_loss(const float* logits, const int32_t* target, int32_t B, int32_t A, float scale, float* loss, float* dlogits,
                int32_t* hits_top1, int32_t* hits_top5, int32_t* bad_flag, float* rows, void* stream_) {
    if (!logits || !target || !bad_flag || !rows) return NCX_E_NULL;
    if (B < 1 || A < 1 || (long long)B * A >= (1ll << 31)) return NCX_E_DIMS;
    hipStream_t s = (hipStream_t)stream_;
    if (scale <= 0.f) scale = 1.f / (float)B;
    hipLaunchKernelGGL(k_ce_rows, dim3(B), dim3(256), 0, s, logits, target, B, A, scale, dlogits, rows, bad_flag);
    NCX_HIP_TRY(hipGetLastError());
    if (loss || hits_top1 || hits_top5) {
        hipLaunchKernelGGL(k_ce_finish, dim3(1), dim3(256), 0, s, (const float*)rows, B, loss, hits_top1, hits_top5);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}

int ncx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n, float lr,
                  float beta1, float beta2, float eps, int32_t step, float grad_scale, void* stream_) {
    if (!param || !grad || !exp_avg || !exp_avg_sq) return NCX_E_NULL;
    if (step < 1 || n == 0) return NCX_E_DIMS;
    if (((uintptr_t)param | (uintptr_t)grad | (uintptr_t)exp_avg | (uintptr_t)exp_avg_sq) & 15) return NCX_E_WORKSPACE;
    return adam_launch(param, grad, exp_avg, exp_avg_sq, n, adam_scalars(lr, beta1, beta2, eps, step, grad_scale), (hipStream_t)stream_);
}
}  // extern "C"
