// ncx_similarity.hip -- the similarity scorer (reference vqa/models/cx.py:490-518, SimilarityModel): no parameters.
//
// Reference (a Python loop over the K candidates, three torch ops each, cx.py:511-516):
//   scores[b, k] = cos(v_orig[b], v_knn[b, k]) + cos(z_orig[b], z_knn[b, k]) + CE(a_knns[b, k, :], aid[b])
//   cos(x, y)    = x . y / (max(|x|, 1e-8) max(|y|, 1e-8))          (F.cosine_similarity: an all-zero row gives 0)
//   CE(a, aid)   = logsumexp(a) - a[aid]                             (F.cross_entropy, no reduction)
//
// k_similarity<LDS> (one launch per batch): one 512-thread workgroup per question.  The K + 1 feature row ids and the answer
// id are checked first (workgroup-uniform verdict; nothing is read at a bad id).  v_orig (gathered by id from the table) and
// z_orig are staged in LDS once; every wave takes their two norms from there (same order in every wave: same bits).  Wave w
// then walks the candidates k = w, w + 8, ...: it streams the candidate's feature row (gathered by id, never copied out),
// its z row and its logit row, each once, with 16-byte loads where base and row length allow (dword loads otherwise):
// dot product and squared norm in one pass against the LDS copy, and the logsumexp as a running (max, sum) pair per lane
// that the lanes merge at the end, so the logits are read once whatever A is.  Lane sums are fixed-order, the cross-lane
// reductions xor butterflies: no atomics, bit-identical from run to run.  LDS = false (dv + dz beyond the 32 KiB staging
// area) reads the originals from global memory (cache-resident after the first candidate) with the same arithmetic.
#include <float.h>
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ncx_internal.h"

namespace ncx {

constexpr int SIM_THREADS = 512;
constexpr int SIM_WAVES = SIM_THREADS / 64;
constexpr int SIM_MAX_K = 64;
constexpr int SIM_MAX_A = 4096;
constexpr int SIM_LDS_FLOATS = 8192;        // staging area of v_orig | z_orig (each padded to a multiple of 4 floats): 32 KiB
constexpr int SIM_U = 8;                    // float4 loads in flight per lane and batch (dv = 2048: the whole row)
constexpr float SIM_EPS = 1e-8f;            // F.cosine_similarity's eps

typedef float sim_f32x4 __attribute__((ext_vector_type(4)));

static inline int sim_pad4(int n) { return (n + 3) / 4 * 4; }

__device__ __forceinline__ float sim_wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float sim_wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}
__device__ __forceinline__ float sim_hsum(sim_f32x4 v) { return (v[0] + v[1]) + (v[2] + v[3]); }

// |x|^2 over n columns (every lane returns it).  al: x is 16-byte aligned and n % 4 == 0.
__device__ __forceinline__ float sim_sumsq(const float* x, int n, bool al, int lane) {
    float s;
    if (al) {
        const sim_f32x4* x4 = reinterpret_cast<const sim_f32x4*>(x);
        sim_f32x4 a = {0.f, 0.f, 0.f, 0.f};
        for (int q = lane; q < (n >> 2); q += 64) { const sim_f32x4 v = x4[q]; a += v * v; }
        s = sim_hsum(a);
    } else {
        s = 0.f;
        for (int c = lane; c < n; c += 64) s = fmaf(x[c], x[c], s);
    }
    return sim_wave_sum(s);
}

// row . org and |row|^2 over n columns in one pass (every lane returns both).  al: both 16-byte aligned and n % 4 == 0.
__device__ __forceinline__ void sim_dot(const float* __restrict__ row, const float* org, int n, bool al, int lane, float& dot, float& nn) {
    float d, s;
    if (al) {
        const sim_f32x4* r4 = reinterpret_cast<const sim_f32x4*>(row);
        const sim_f32x4* o4 = reinterpret_cast<const sim_f32x4*>(org);
        const int nq = n >> 2;
        const sim_f32x4 zero = {0.f, 0.f, 0.f, 0.f};
        sim_f32x4 ad = zero, an = zero;
        // wave-uniform trip count, lanes past the row's end predicated off: every batch issues its loads together
        for (int q0 = lane; q0 - lane < nq; q0 += 64 * SIM_U) {
            sim_f32x4 r[SIM_U];
#pragma unroll
            for (int i = 0; i < SIM_U; ++i) r[i] = q0 + 64 * i < nq ? __builtin_nontemporal_load(r4 + q0 + 64 * i) : zero;
#pragma unroll
            for (int i = 0; i < SIM_U; ++i) {
                const sim_f32x4 o = q0 + 64 * i < nq ? o4[q0 + 64 * i] : zero;
                ad += r[i] * o; an += r[i] * r[i];
            }
        }
        d = sim_hsum(ad); s = sim_hsum(an);
    } else {
        d = 0.f; s = 0.f;
#pragma unroll 4
        for (int c = lane; c < n; c += 64) { const float r = row[c]; d = fmaf(r, org[c], d); s = fmaf(r, r, s); }
    }
    dot = sim_wave_sum(d); nn = sim_wave_sum(s);
}

__device__ __forceinline__ float sim_cos(float dot, float nn_a, float nn_b) {
    return dot / (fmaxf(sqrtf(nn_a), SIM_EPS) * fmaxf(sqrtf(nn_b), SIM_EPS));
}

// logsumexp(row[0 .. A)) - row[aid] (every lane returns it).  Each lane keeps a running max m (never below -FLT_MAX, so that
// -inf logits give exp = 0 and not inf - inf) and the sum of exp(x - m); the lanes' pairs are merged at the wave's max.
__device__ __forceinline__ float sim_xent(const float* __restrict__ row, int A, bool al, int aid, int lane) {
    constexpr float L2E = 1.4426950408889634f;
    float m = -FLT_MAX, s = 0.f;
    if (al) {
        const sim_f32x4* r4 = reinterpret_cast<const sim_f32x4*>(row);
        const int nq = A >> 2;
        const sim_f32x4 low = {-INFINITY, -INFINITY, -INFINITY, -INFINITY};   // (exp = 0, the max untouched)
        for (int q0 = lane; q0 - lane < nq; q0 += 64 * SIM_U) {              // (wave-uniform trip count, as in sim_dot)
            sim_f32x4 r[SIM_U];
#pragma unroll
            for (int i = 0; i < SIM_U; ++i) r[i] = q0 + 64 * i < nq ? __builtin_nontemporal_load(r4 + q0 + 64 * i) : low;
            float mn = m;
#pragma unroll
            for (int i = 0; i < SIM_U; ++i) mn = fmaxf(fmaxf(fmaxf(mn, r[i][0]), fmaxf(r[i][1], r[i][2])), r[i][3]);
            s *= __builtin_amdgcn_exp2f((m - mn) * L2E);
#pragma unroll
            for (int i = 0; i < SIM_U; ++i)
#pragma unroll
                for (int e = 0; e < 4; ++e) s += __builtin_amdgcn_exp2f((r[i][e] - mn) * L2E);
            m = mn;
        }
    } else {
        for (int c = lane; c < A; c += 64) {
            const float x = row[c];
            const float mn = fmaxf(m, x);
            s = fmaf(s, __builtin_amdgcn_exp2f((m - mn) * L2E), __builtin_amdgcn_exp2f((x - mn) * L2E));
            m = mn;
        }
    }
    const float M = sim_wave_max(m);
    s *= __builtin_amdgcn_exp2f((m - M) * L2E);          // (a lane without columns: s = 0)
    const float S = sim_wave_sum(s);
    return (M + logf(S)) - row[aid];
}

template <bool LDS>
__global__ __launch_bounds__(SIM_THREADS) void k_similarity(const float* __restrict__ feats, const int* __restrict__ img_idx, int n_img, int dv,
                                                            const float* __restrict__ z_orig, const float* __restrict__ z_knns, int dz,
                                                            const float* __restrict__ a_knns, const int* __restrict__ aids, int A, int K,
                                                            int alv, int alz, int ala, float* __restrict__ scores,
                                                            float* __restrict__ parts, int* __restrict__ bad) {
    __shared__ sim_f32x4 s_org[LDS ? SIM_LDS_FLOATS / 4 : 1];
    __shared__ int s_ids[SIM_MAX_K + 1];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    const int aid = aids[b];
    int is_bad = tid == 0 && (aid < 0 || aid >= A);
    if (tid <= K) {
        const int id = img_idx[b * (K + 1) + tid];
        s_ids[tid] = id;
        is_bad |= id < 0 || id >= n_img;
    }
    if (__syncthreads_or(is_bad)) {            // workgroup-uniform: nothing is read at a bad id, the row is NaN, the flag is set
        if (tid == 0) *bad = 1;
        for (int k = tid; k < K; k += SIM_THREADS) {
            scores[b * K + k] = NAN;
            if (parts) { parts[(b * K + k) * 3] = NAN; parts[(b * K + k) * 3 + 1] = NAN; parts[(b * K + k) * 3 + 2] = NAN; }
        }
        return;
    }
    const float* vo = feats + (long long)s_ids[0] * dv;
    const float* zo = z_orig + b * dz;
    if (LDS) {
        float* sv = reinterpret_cast<float*>(s_org);
        float* sz = sv + (dv + 3) / 4 * 4;
        if (alv) for (int q = tid; q < (dv >> 2); q += SIM_THREADS) s_org[q] = reinterpret_cast<const sim_f32x4*>(vo)[q];
        else     for (int c = tid; c < dv; c += SIM_THREADS) sv[c] = vo[c];
        for (int c = tid; c < dz; c += SIM_THREADS) sz[c] = zo[c];
        __syncthreads();
        vo = sv; zo = sz;
    }
    const float nn_vo = sim_sumsq(vo, dv, alv, lane), nn_zo = sim_sumsq(zo, dz, alz, lane);
    for (int k = wave; k < K; k += SIM_WAVES) {
        const long long bk = b * K + k;
        float dvk, nn_vk, dzk, nn_zk;
        sim_dot(feats + (long long)s_ids[k + 1] * dv, vo, dv, alv, lane, dvk, nn_vk);
        sim_dot(z_knns + bk * dz, zo, dz, alz, lane, dzk, nn_zk);
        const float xe = sim_xent(a_knns + bk * A, A, ala, aid, lane);
        if (lane == 0) {
            const float cv = sim_cos(dvk, nn_vo, nn_vk), cz = sim_cos(dzk, nn_zo, nn_zk);
            scores[bk] = (cv + cz) + xe;                 // cx.py:516
            if (parts) { parts[bk * 3] = cv; parts[bk * 3 + 1] = cz; parts[bk * 3 + 2] = xe; }
        }
    }
}

}  // namespace ncx

using namespace ncx;

extern "C" int ncx_similarity_scores(const float* feats, const int32_t* img_idx, int32_t n_img, int32_t dv, const float* z_orig,
                                     const float* z_knns, int32_t dz, const float* a_knns, const int32_t* aid, int32_t A, int32_t B,
                                     int32_t K, float* scores, float* parts, int32_t* bad_id_flag, void* stream_) {
    if (!feats || !img_idx || !z_orig || !z_knns || !a_knns || !aid || !scores || !bad_id_flag) return NCX_E_NULL;
    if (B < 1 || K < 1 || K > SIM_MAX_K || A < 1 || A > SIM_MAX_A || dv < 1 || dz < 1 || n_img < 1) return NCX_E_DIMS;
    hipStream_t s = (hipStream_t)stream_;
    const auto al16 = [](const void* p) { return ((uintptr_t)p & 15) == 0; };
    const int alv = dv % 4 == 0 && al16(feats), alz = dz % 4 == 0 && al16(z_orig) && al16(z_knns), ala = A % 4 == 0 && al16(a_knns);
    int* bad = (int*)bad_id_flag;
    if ((long long)sim_pad4(dv) + sim_pad4(dz) <= SIM_LDS_FLOATS)
        hipLaunchKernelGGL((k_similarity<true>), dim3(B), dim3(SIM_THREADS), 0, s, feats, (const int*)img_idx, n_img, dv, z_orig, z_knns, dz,
                           a_knns, (const int*)aid, A, K, alv, alz, ala, scores, parts, bad);
    else
        hipLaunchKernelGGL((k_similarity<false>), dim3(B), dim3(SIM_THREADS), 0, s, feats, (const int*)img_idx, n_img, dv, z_orig, z_knns, dz,
                           a_knns, (const int*)aid, A, K, alv, alz, ala, scores, parts, bad);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
