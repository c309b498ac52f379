// ncx_semantic.hip -- the semantic baseline scorer (reference vqa/models/cx.py:159-210, SemanticBaseline; README row
// "Semantic Baseline").
//
// Reference (per question b with answer id aid, per candidate k; a Python double loop over numpy rows):
//   p   = softmax(a_knns[b, k, :])                       (cx.py:177-180, 193)
//   ws  = emb_pairs[aid, :] . p - p[aid]                 (cx.py:194-197; emb_pairs = cosine_similarity(emb), cx.py:174-175)
//   s_k = lam * ws - (1 - lam) * log(p[aid] + 1e-8)      (cx.py:199-204)
//   scores[b, :] = softmax_k(s)                          (cx.py:206-207)
//
//   1. k_cos_rownorm    (once per embedding)  E^ = E / ||E||_2 per row; a zero row stays zero (sklearn's normalize rule),
//                       written with a leading dimension padded to a multiple of 4 (zero columns)
//   2. E^ . E^^T        the library's fp32-MFMA NT engine (run_gemm_nt, as ncx_knn.hip does): the cosine Gram [A, A], in
//                       column chunks of E^ (<= 320 wide) whose partial products are summed in fp64 (k_gram_acc): one fp32
//                       accumulation over all 2400 columns drifts by up to ~2e-6 on the near-1 entries (the diagonal,
//                       duplicated rows); per chunk the partial sums stay small and so does their rounding
//   3. k_semantic<NV>   (hot path, one launch per batch)  one workgroup per question: its 8 waves stream candidate rows
//                       (16-byte buffer loads, the row held in VGPRs: NV float4 per lane), wave max, then sum e and
//                       sum e * G[aid, :] in one pass with exp2 on pre-scaled inputs; the Gram row of aid sits in LDS; the
//                       K scores meet in LDS and wave 0 takes their softmax.
// The reference's softmax does not subtract the max (NaN for a logit above ~88.7 in fp32); both softmaxes here do: equal
// wherever the reference is finite, finite elsewhere.  p[aid] + 1e-8 and its log are fp32, as in the reference.
#include <hip/hip_runtime.h>
#include <math.h>
#include <stdint.h>
#include "ncx_internal.h"

namespace ncx {

constexpr int SEM_THREADS = 512;
constexpr int SEM_WAVES = SEM_THREADS / 64;
constexpr int SEM_MAX_K = 64;
constexpr int SEM_MAX_A = 4096;             // 16 float4 per lane: the row stays in registers
constexpr int GRAM_MAX_A = 8192;
constexpr long long GRAM_MAX_ELEMS = 1ll << 28;   // rows x padded width of E^ (1 GiB)
constexpr int GRAM_CHUNK = 320;                   // columns of E^ per partial product (a multiple of the engine's 32-deep k-step)

typedef float sem_f32x4 __attribute__((ext_vector_type(4)));
typedef unsigned int sem_u32x4 __attribute__((ext_vector_type(4)));

static inline int gram_ld(int da) { return da < 4 ? 4 : (da + 3) / 4 * 4; }

// One wave per row: fp64 sum of squares, each element divided by the fp64 norm (correctly rounded E^); pad columns zero.
__global__ __launch_bounds__(256) void k_cos_rownorm(const float* __restrict__ emb, int A, int da, int ldp, float* __restrict__ out) {
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= A) return;
    const float* p = emb + (long long)row * da;
    double s = 0.0;
    for (int c = lane; c < da; c += 64) { const double v = p[c]; s = fma(v, v, s); }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    const double nrm = sqrt(s);
    float* q = out + (long long)row * ldp;
    for (int c = lane; c < ldp; c += 64) q[c] = (c < da && s > 0.0) ? (float)((double)p[c] / nrm) : 0.f;
}

// acc += part (fp64); the last chunk writes the rounded sum to out (which may be `part` itself: same element, same thread).
__global__ __launch_bounds__(256) void k_gram_acc(const float* part, double* __restrict__ acc, float* out, long long n, int first, int last) {
    for (long long i = blockIdx.x * 256ll + threadIdx.x; i < n; i += (long long)gridDim.x * 256) {
        const double v = (first ? 0.0 : acc[i]) + (double)part[i];
        if (last) out[i] = (float)v;
        else acc[i] = v;
    }
}

__device__ __forceinline__ float wave_max(float v) {
    for (int o = 32; o > 0; o >>= 1) v = fmaxf(v, __shfl_xor(v, o));
    return v;
}
__device__ __forceinline__ float wave_sum(float v) {
    for (int o = 32; o > 0; o >>= 1) v += __shfl_xor(v, o);
    return v;
}

// Row k of the question's [K, A] block: lane l holds columns 4 (l + 64 i) .. + 3, i < NV.  The buffer resource spans exactly
// the question's block, so the window past its last row reads zeros and never leaves it; columns >= A are masked by the
// caller.  AL: A % 4 == 0 (16-byte aligned rows, one b128 load per float4); else four dword loads.
template <int NV, bool AL>
__device__ __forceinline__ void sem_load_row(__amdgpu_buffer_rsrc_t rs, int k, int A, int lane, sem_f32x4* v) {
    const unsigned base = (unsigned)k * (unsigned)A * 4u;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const unsigned off = base + (unsigned)(lane + 64 * i) * 16u;
        if (AL) {
            v[i] = __builtin_bit_cast(sem_f32x4, (sem_u32x4)__builtin_amdgcn_raw_buffer_load_b128(rs, off, 0, 0));
        } else {
#pragma unroll
            for (int e = 0; e < 4; ++e)
                v[i][e] = __builtin_bit_cast(float, (unsigned)__builtin_amdgcn_raw_buffer_load_b32(rs, off + 4u * e, 0, 0));
        }
    }
}

// s_k of one candidate row (every lane returns it).
template <int NV>
__device__ __forceinline__ float sem_row_score(sem_f32x4* v, const float* g_row, int A, int aid, int lane, float lam) {
    constexpr float L2E = 1.4426950408889634f;
    float m = -INFINITY;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const int c = 4 * (lane + 64 * i) + e;
            v[i][e] = c < A ? v[i][e] : -INFINITY;
            m = fmaxf(m, v[i][e]);
        }
    }
    m = wave_max(m);
    const float mL = m * L2E;
    float se = 0.f, sg = 0.f, ea = 0.f;
#pragma unroll
    for (int i = 0; i < NV; ++i) {
        const sem_f32x4 g = *reinterpret_cast<const sem_f32x4*>(g_row + 4 * (lane + 64 * i));
#pragma unroll
        for (int e = 0; e < 4; ++e) {
            const float t = __builtin_amdgcn_exp2f(fmaf(v[i][e], L2E, -mL));      // exp(x - max); 0 for masked columns
            se += t;
            sg = fmaf(t, g[e], sg);
            ea = (4 * (lane + 64 * i) + e == aid) ? t : ea;
        }
    }
    se = wave_sum(se); sg = wave_sum(sg); ea = wave_sum(ea);      // (ea: one lane holds it, the others 0: exact)
    const float p = ea / se;
    const float ws = sg / se - p;                                  // emb_pairs[aid,:] . p - p[aid]   (cx.py:194-197)
    const float logp = logf(p + 1e-8f);                            // cx.py:199-202 (fp32)
    return lam * ws - (1.f - lam) * logp;                          // cx.py:204
}

template <int NV, bool AL>
__global__ __launch_bounds__(SEM_THREADS) void k_semantic(const float* __restrict__ a_knns, const int* __restrict__ aids, int K, int A,
                                                          const float* __restrict__ gram, float lam, float* __restrict__ scores,
                                                          float* __restrict__ raw, int* __restrict__ bad) {
    __shared__ __attribute__((aligned(16))) float g_row[256 * NV];
    __shared__ float s_k[SEM_MAX_K];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long b = blockIdx.x;
    const int aid = aids[b];
    if (aid < 0 || aid >= A) {                 // workgroup-uniform: nothing is read at this id, the row is NaN, the flag is set
        if (tid == 0) *bad = 1;
        for (int k = tid; k < K; k += SEM_THREADS) {
            scores[b * K + k] = NAN;
            if (raw) raw[b * K + k] = NAN;
        }
        return;
    }
    const __amdgpu_buffer_rsrc_t rs = __builtin_amdgcn_make_buffer_rsrc(const_cast<float*>(a_knns + b * K * (long long)A), 0,
                                                                        (int)((unsigned)K * (unsigned)A * 4u), 0x00020000);
    sem_f32x4 r0[NV], r1[NV];
    if (wave < K) sem_load_row<NV, AL>(rs, wave, A, lane, r0);     // (in flight while the Gram row is staged)
    const float* grow = gram + (long long)aid * A;
    for (int c = tid; c < 256 * NV; c += SEM_THREADS) g_row[c] = c < A ? grow[c] : 0.f;
    __syncthreads();
    // rows wave, wave + 8, ...: two in flight per wave (ping-pong register sets)
    for (int k = wave; k < K; k += 2 * SEM_WAVES) {
        const int k1 = k + SEM_WAVES, k2 = k + 2 * SEM_WAVES;
        if (k1 < K) sem_load_row<NV, AL>(rs, k1, A, lane, r1);
        const float s0 = sem_row_score<NV>(r0, g_row, A, aid, lane, lam);
        if (lane == 0) s_k[k] = s0;
        if (k2 < K) sem_load_row<NV, AL>(rs, k2, A, lane, r0);
        if (k1 < K) {
            const float s1 = sem_row_score<NV>(r1, g_row, A, aid, lane, lam);
            if (lane == 0) s_k[k1] = s1;
        }
    }
    __syncthreads();
    if (wave == 0) {                           // softmax over the K scores (cx.py:206), K <= 64: one lane each
        const float s = lane < K ? s_k[lane] : -INFINITY;
        const float mx = wave_max(s);
        const float e = lane < K ? expf(s - mx) : 0.f;
        const float tot = wave_sum(e);
        if (lane < K) {
            scores[b * K + lane] = e / tot;
            if (raw) raw[b * K + lane] = s;
        }
    }
}

template <int NV>
static void launch_semantic(bool al, int B, const float* a_knns, const int* aids, int K, int A, const float* gram, float lam,
                            float* scores, float* raw, int* bad, hipStream_t s) {
    if (al) hipLaunchKernelGGL((k_semantic<NV, true>), dim3(B), dim3(SEM_THREADS), 0, s, a_knns, aids, K, A, gram, lam, scores, raw, bad);
    else    hipLaunchKernelGGL((k_semantic<NV, false>), dim3(B), dim3(SEM_THREADS), 0, s, a_knns, aids, K, A, gram, lam, scores, raw, bad);
}

}  // namespace ncx

using namespace ncx;

extern "C" size_t ncx_cosine_gram_workspace_bytes(int32_t A, int32_t da) {
    if (A < 1 || da < 1 || A > GRAM_MAX_A || (long long)A * gram_ld(da) > GRAM_MAX_ELEMS) return 0;
    return align_up((size_t)A * (size_t)gram_ld(da) * 4, 256) + (size_t)A * (size_t)A * 8;
}

extern "C" int ncx_cosine_gram(const float* emb, int32_t A, int32_t da, void* ws, size_t ws_bytes, float* gram, void* stream_) {
    if (!emb || !ws || !gram) return NCX_E_NULL;
    if (A < 1 || da < 1 || A > GRAM_MAX_A || (long long)A * gram_ld(da) > GRAM_MAX_ELEMS) return NCX_E_DIMS;
    if (ws_bytes < ncx_cosine_gram_workspace_bytes(A, da) || ((uintptr_t)ws & 255)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    const int ldp = gram_ld(da);
    float* en = (float*)ws;
    hipLaunchKernelGGL(k_cos_rownorm, dim3((A + 3) / 4), dim3(256), 0, s, emb, A, da, ldp, en);
    NCX_HIP_TRY(hipGetLastError());
    double* acc = (double*)((char*)ws + align_up((size_t)A * (size_t)ldp * 4, 256));
    const long long n = (long long)A * A;
    const int grid = (int)((n + 255) / 256 < 4096 ? (n + 255) / 256 : 4096);
    for (int c0 = 0; c0 < ldp; c0 += GRAM_CHUNK) {
        const int w = ldp - c0 < GRAM_CHUNK ? ldp - c0 : GRAM_CHUNK;          // a multiple of 4 (ldp is)
        GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = A;
        a.a[0] = x_plain(en + c0, ldp, A, w); a.b[0] = x_plain(en + c0, ldp, A, w); a.klen[0] = w;
        a.out[0] = gram; a.ldo[0] = A; a.n_cols[0] = A; a.split[0] = 1;
        GemmPlan pl = plan_gemm(FORM_NT, A, A, ksteps(w), true);
        pl.split = 1;
        const int rc = run_gemm_nt(a, pl.cfg, s);
        if (rc) return rc;
        const bool first = c0 == 0, last = c0 + GRAM_CHUNK >= ldp;
        if (first && last) break;                                                // one chunk: the product is the Gram
        hipLaunchKernelGGL(k_gram_acc, dim3(grid), dim3(256), 0, s, (const float*)gram, acc, gram, n, (int)first, (int)last);
        NCX_HIP_TRY(hipGetLastError());
    }
    return NCX_OK;
}

extern "C" int ncx_semantic_scores(const float* a_knns, const int32_t* aid, int32_t B, int32_t K, int32_t A, const float* gram,
                                   float lam, float* scores, float* raw, int32_t* bad_id_flag, void* stream_) {
    if (!a_knns || !aid || !gram || !scores || !bad_id_flag) return NCX_E_NULL;
    if (B < 1 || K < 1 || K > SEM_MAX_K || A < 1 || A > SEM_MAX_A) return NCX_E_DIMS;
    hipStream_t s = (hipStream_t)stream_;
    const bool al = A % 4 == 0;
    int* bad = (int*)bad_id_flag;
    if (A <= 256)       launch_semantic<1>(al, B, a_knns, aid, K, A, gram, lam, scores, raw, bad, s);
    else if (A <= 512)  launch_semantic<2>(al, B, a_knns, aid, K, A, gram, lam, scores, raw, bad, s);
    else if (A <= 1024) launch_semantic<4>(al, B, a_knns, aid, K, A, gram, lam, scores, raw, bad, s);
    else if (A <= 2048) launch_semantic<8>(al, B, a_knns, aid, K, A, gram, lam, scores, raw, bad, s);
    else                launch_semantic<16>(al, B, a_knns, aid, K, A, gram, lam, scores, raw, bad, s);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
