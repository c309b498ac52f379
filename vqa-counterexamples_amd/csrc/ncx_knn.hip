// ncx_knn.hip -- brute-force k nearest neighbours of image-feature rows.
//
// Replaces the reference's knn.py:41-58 (sklearn NearestNeighbors(n_neighbors=25).fit(features).kneighbors(batch),
// brute force, euclidean): the step that builds the 24-candidate lists the CX data set is made of.
//
//   1. halfneg[j] = -|x_j|^2 / 2                                         (k_knn_halfnorm, once per table)
//   2. V[i][j]    = q_i . x_j - |x_j|^2 / 2   for a block of queries      (the NT GEMM engine, bias = halfneg)
//                   |q_i - x_j|^2 = |q_i|^2 - 2 V[i][j]: per query, the k nearest rows are the k LARGEST V
//   3. per query row: linear-histogram select of the k+8 largest V by (V, index) (3 coalesced passes over the row; more
//      only when a bin must be refined), then the candidates' distances are recomputed exactly as sum (q - x)^2 (no
//      cancellation), sorted by (distance, index) and the first k are written.   (k_knn_select, one workgroup per query)
// Precision contract (DESIGN f4): a returned row's exact d2 exceeds the true k-th d2 by at most
//   tau = 4 (dv + 2) 2^-24 max_j (sum_t |q_t x_jt| + |x_j|^2 / 2); input must be finite.
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "ncx_internal.h"

namespace ncx {

constexpr int KNN_BINS = 1024;
constexpr int KNN_CAP = 1024;        // candidate buffer (elements at or above the threshold bin)
constexpr int KNN_MAXK = 128;        // k + margin
constexpr int KNN_LEVELS = 3;

__global__ __launch_bounds__(256) void k_knn_halfnorm(const float* __restrict__ x, int n, int dv, float* __restrict__ halfneg,
                                                      int* __restrict__ status) {
    if (blockIdx.x == 0 && threadIdx.x < 2) status[threadIdx.x] = 0;
    const int row = blockIdx.x * 4 + (threadIdx.x >> 6), lane = threadIdx.x & 63;
    if (row >= n) return;
    const float* p = x + (long long)row * dv;
    float s = 0.f;
    for (int c = lane; c < dv; c += 64) { const float v = p[c]; s = fmaf(v, v, s); }
    for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
    if (lane == 0) halfneg[row] = -0.5f * s;
}

// Status word of a table's workspace (see ncx_knn_status_offset in neuralcx.h): cleared by k_knn_halfnorm, set by k_knn_select.
// Each word is only ever stored as 1 (plain stores from any workgroup: no atomics, no ordering needed).
constexpr int KNN_ST_EXHAUSTED = 0;  // word 0: distinct products still overflow the candidate buffer after the last level
constexpr int KNN_ST_NONFINITE = 1;  // word 1: a product row is not finite (the input was not, or its products overflow fp32)

// bin of v in a histogram of [lo, lo + KNN_BINS / scale): monotone in v, clamped at both ends
__device__ inline int knn_bin(float v, float lo, float scale) {
    const float f = (v - lo) * scale;
    int b = (int)f;
    return b < 0 ? 0 : b > KNN_BINS - 1 ? KNN_BINS - 1 : b;
}
// +1 above, 0 inside, -1 below the chosen bin of the last level.  That level's members are the values inside [lo, hi]; knn_bin
// is monotone, so everything above hi is above the bin and everything below lo is below it.
__device__ inline int knn_classify(float v, float lo, float hi, float scale, int chosen) {
    if (v > hi) return 1;
    if (v < lo) return -1;
    const int b = knn_bin(v, lo, scale);
    return b > chosen ? 1 : b < chosen ? -1 : 0;
}

__global__ __launch_bounds__(256) void k_knn_select(const float* __restrict__ V, long long ldv, const float* __restrict__ table,
                                                    const float* __restrict__ queries, int n, int dv, int k, int kc,
                                                    long long* __restrict__ out_idx, float* __restrict__ out_dist,
                                                    int* __restrict__ status) {
    __shared__ int hist[KNN_BINS];
    __shared__ float cand_v[KNN_CAP];
    __shared__ int cand_j[KNN_CAP];
    __shared__ float red_a[4], red_b[4], red_c[4];
    __shared__ int s_count, s_count_in, s_done, s_above_total, s_chosen;
    __shared__ int s_wcnt[2][4];
    __shared__ float top_v[KNN_MAXK];
    __shared__ int top_j[KNN_MAXK];
    __shared__ double top_d[KNN_MAXK];
    const int tid = threadIdx.x, lane = tid & 63, wave = tid >> 6;
    const long long q = blockIdx.x;
    const float* row = V + q * ldv;

    // pass 1: range of the row
    float mx = -INFINITY, mn = INFINITY, nf = 0.f;                 // nf: v - v is 0 for a finite v, NaN otherwise
    for (int j = tid; j < n; j += 256) { const float v = row[j]; mx = fmaxf(mx, v); mn = fminf(mn, v); nf += v - v; }
    for (int o = 32; o > 0; o >>= 1) { mx = fmaxf(mx, __shfl_xor(mx, o)); mn = fminf(mn, __shfl_xor(mn, o)); nf += __shfl_xor(nf, o); }
    if (lane == 0) { red_a[wave] = mx; red_b[wave] = mn; red_c[wave] = nf; }
    if (tid == 0) { s_done = 0; s_above_total = 0; s_chosen = 0; }
    if (tid < KNN_MAXK) { top_v[tid] = 0.f; top_j[tid] = 0; }       // a non-finite row may leave ranks unfilled: never an address
    __syncthreads();
    mx = fmaxf(fmaxf(red_a[0], red_a[1]), fmaxf(red_a[2], red_a[3]));
    mn = fminf(fminf(red_b[0], red_b[1]), fminf(red_b[2], red_b[3]));
    if (tid == 0 && (red_c[0] + red_c[1]) + (red_c[2] + red_c[3]) != 0.f) status[KNN_ST_NONFINITE] = 1;

    // refinement levels: histogram of the members (values inside [lo, hi]), pick the bin holding the kc-th largest.  A bin whose
    // members do not fit the buffer's tie region is refined over the smallest and largest of ITS MEMBERS (a reduction over the
    // row, run only then): each level narrows the real value range, wherever the row's minimum lies.
    float lo = mn, hi = mx, scale = 0.f;
    bool fits = true;
    for (int level = 0; level < KNN_LEVELS; ++level) {
        for (int b = tid; b < KNN_BINS; b += 256) hist[b] = 0;
        const float range = hi - lo;
        // a refined range can be a few denormal steps wide: keep the scale finite, so that (lo - lo) * scale is 0, never 0 * inf
        scale = range > 0.f ? fminf((float)KNN_BINS / range, 3.402823466e38f) : 0.f;
        __syncthreads();
        for (int j = tid; j < n; j += 256) {
            const float v = row[j];
            if (v >= lo && v <= hi) atomicAdd(&hist[knn_bin(v, lo, scale)], 1);
        }
        __syncthreads();
        if (wave == 0) {
            // suffix counts from the top bin: lane L owns bins [16 L, 16 L + 16)
            int local = 0;
            for (int b = 0; b < 16; ++b) local += hist[lane * 16 + b];
            int above = 0;                                      // elements in bins owned by higher lanes
            for (int o = 1; o < 64; ++o) { const int other = __shfl(local, (lane + o) & 63); if (lane + o < 64) above += other; }
            const int need = kc - s_above_total;                // still to be found inside this level's range
            // the owning lane: above < need <= above + local
            if (above < need && need <= above + local) {
                int acc = above, chosen = lane * 16;
                for (int b = 15; b >= 0; --b) {
                    const int h = hist[lane * 16 + b];
                    if (acc + h >= need) { chosen = lane * 16 + b; break; }
                    acc += h;
                }
                s_chosen = chosen;
                // stop when the chosen bin's members fit the buffer's tie region (elements above it number < kc)
                if (hist[chosen] <= KNN_CAP - kc) s_done = 1;
                else s_above_total += acc;                      // read by the next level, if the bin is refined
            }
        }
        __syncthreads();
        if (s_done) break;
        // the chosen bin's members do not fit: their smallest and largest value
        const int chosen = s_chosen;
        float bmx = -INFINITY, bmn = INFINITY;
        for (int j = tid; j < n; j += 256) {
            const float v = row[j];
            if (v >= lo && v <= hi && knn_bin(v, lo, scale) == chosen) { bmx = fmaxf(bmx, v); bmn = fminf(bmn, v); }
        }
        for (int o = 32; o > 0; o >>= 1) { bmx = fmaxf(bmx, __shfl_xor(bmx, o)); bmn = fminf(bmn, __shfl_xor(bmn, o)); }
        if (lane == 0) { red_a[wave] = bmx; red_b[wave] = bmn; }
        __syncthreads();
        bmx = fmaxf(fmaxf(red_a[0], red_a[1]), fmaxf(red_a[2], red_a[3]));
        bmn = fminf(fminf(red_b[0], red_b[1]), fminf(red_b[2], red_b[3]));
        __syncthreads();                                        // red_a / red_b are written again by the next level
        // one value (exact ties: the lowest row indices are kept below), or no level left for distinct ones: never a guess
        if (!(bmn < bmx) || level == KNN_LEVELS - 1) {
            if (bmn < bmx && tid == 0) status[KNN_ST_EXHAUSTED] = 1;
            fits = false;
            break;
        }
        lo = bmn; hi = bmx;
    }

    // pass 3: collect everything above the chosen bin (from the front of the buffer) and inside it (from the back, so that
    // the in-bin elements never displace the ones above).  When the in-bin members fit, their slots come in arrival order: the
    // set is complete and the rank sort below orders it.  When they do not (ties), the first KNN_CAP - kc of them BY ROW INDEX
    // are kept: a block scan over each stride of 256 rows, j ascending.
    if (tid == 0) { s_count = 0; s_count_in = 0; }
    __syncthreads();
    {
        const int chosen = s_chosen;
        if (fits) {
            for (int j = tid; j < n; j += 256) {
                const float v = row[j];
                const int cls = knn_classify(v, lo, hi, scale, chosen);
                if (cls > 0) {
                    const int slot = atomicAdd(&s_count, 1);
                    if (slot < KNN_CAP) { cand_v[slot] = v; cand_j[slot] = j; }
                } else if (cls == 0) {
                    const int slot = KNN_CAP - 1 - atomicAdd(&s_count_in, 1);
                    if (slot >= kc) { cand_v[slot] = v; cand_j[slot] = j; }      // above-elements number < kc <= slot
                }
            }
        } else {
            int base = 0;                                                        // in-bin members before this stride (uniform)
            for (int j0 = 0, it = 0; j0 < n && base < KNN_CAP - kc; j0 += 256, ++it) {
                const int j = j0 + tid;
                const float v = j < n ? row[j] : 0.f;
                const int cls = j < n ? knn_classify(v, lo, hi, scale, chosen) : -1;
                const unsigned long long in = __ballot(cls == 0);
                if (lane == 0) s_wcnt[it & 1][wave] = __popcll(in);
                __syncthreads();                                                 // two buffers: one barrier per stride
                int before = base + __popcll(in & ((1ull << lane) - 1ull));
                for (int w = 0; w < 4; ++w) { const int c = s_wcnt[it & 1][w]; if (w < wave) before += c; base += c; }
                if (cls == 0) {
                    const int slot = KNN_CAP - 1 - before;
                    if (slot >= kc) { cand_v[slot] = v; cand_j[slot] = j; }
                }
            }
            if (tid == 0) s_count_in = base;
            for (int j = tid; j < n; j += 256) {                                 // the elements above: fewer than kc, any order
                const float v = row[j];
                if (knn_classify(v, lo, hi, scale, chosen) > 0) {
                    const int slot = atomicAdd(&s_count, 1);
                    if (slot < KNN_CAP) { cand_v[slot] = v; cand_j[slot] = j; }
                }
            }
        }
    }
    __syncthreads();
    const int na = s_count;                                                   // < kc by construction
    const int nb = s_count_in < KNN_CAP - kc ? s_count_in : KNN_CAP - kc;
    const int nc = na + nb;
    const int kk = kc < nc ? kc : nc;
    auto phys = [&](int e) { return e < na ? e : KNN_CAP - 1 - (e - na); };
    // rank sort by (V descending, index ascending); the first kc go on
    for (int e = tid; e < nc; e += 256) {
        const float v = cand_v[phys(e)]; const int j = cand_j[phys(e)];
        int rank = 0;
        for (int f = 0; f < nc; ++f) {
            const float vf = cand_v[phys(f)];
            rank += (vf > v) || (vf == v && cand_j[phys(f)] < j);
        }
        if (rank < kk) { top_v[rank] = v; top_j[rank] = j; }
    }
    __syncthreads();
    // exact distances of the candidates in fp64 (fp32 inputs: the differences are exact, the ordering is the true one;
    // an fp32 sum swaps neighbours closer than ~1e-6 relative): one wave per candidate
    const float* qrow = queries + q * dv;
    for (int c = wave; c < kk; c += 4) {
        const float* xr = table + (long long)top_j[c] * dv;
        double s = 0.0;
        for (int t = lane; t < dv; t += 64) { const double df = (double)qrow[t] - (double)xr[t]; s = fma(df, df, s); }
        for (int o = 32; o > 0; o >>= 1) s += __shfl_xor(s, o);
        if (lane == 0) top_d[c] = s;
    }
    __syncthreads();
    if (tid < kk) {
        const double dd = top_d[tid]; const int j = top_j[tid];
        int rank = 0;
        for (int f = 0; f < kk; ++f) rank += (top_d[f] < dd) || (top_d[f] == dd && top_j[f] < j);
        if (rank < k) { out_idx[q * k + rank] = j; out_dist[q * k + rank] = (float)sqrt(dd); }
    }
    // fewer than k rows in the table: pad (callers validate k <= n, so this is unreachable in practice)
    for (int r = kk + tid; r < k; r += 256) { out_idx[q * k + r] = -1; out_dist[q * k + r] = INFINITY; }
}

}  // namespace ncx

using namespace ncx;

// workspace: halfneg [n] | status words (256 B) | V [block_rows, n]
extern "C" size_t ncx_knn_status_offset(int32_t n) { return n < 1 ? 0 : align_up((size_t)n * 4, 256); }

extern "C" size_t ncx_knn_workspace_bytes(int32_t n, int32_t block_rows) {
    if (n < 1 || block_rows < 1) return 0;
    return align_up((size_t)n * 4, 256) + 256 + (size_t)block_rows * (size_t)n * 4;
}

extern "C" int ncx_knn(const float* table, int32_t n, const float* queries, int32_t nq, int32_t dv, int32_t k,
                       int32_t norms_ready, void* workspace, size_t workspace_bytes, int64_t* out_idx, float* out_dist,
                       void* stream_) {
    if (!table || !queries || !workspace || !out_idx || !out_dist) return NCX_E_NULL;
    if (n < 1 || nq < 1 || dv < 4 || k < 1 || k > n || k + 8 > KNN_MAXK) return NCX_E_DIMS;
    if (workspace_bytes < ncx_knn_workspace_bytes(n, nq) || ((uintptr_t)workspace & 255)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    float* halfneg = (float*)workspace;
    int* status = (int*)((char*)workspace + ncx_knn_status_offset(n));
    float* V = (float*)((char*)status + 256);
    if (!norms_ready) {
        hipLaunchKernelGGL(k_knn_halfnorm, dim3((n + 3) / 4), dim3(256), 0, s, table, n, dv, halfneg, status);
        NCX_HIP_TRY(hipGetLastError());
    }
    {
        GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = nq;
        a.a[0] = x_plain(queries, dv, nq, dv); a.b[0] = x_plain(table, dv, n, dv); a.klen[0] = dv;
        a.out[0] = V; a.ldo[0] = n; a.n_cols[0] = n; a.split[0] = 1;
        a.epi.bias = halfneg;
        GemmPlan pl = plan_gemm(FORM_NT, nq, n, ksteps(dv), true);
        pl.split = 1;
        const int rc = run_gemm_nt(a, pl.cfg, s);
        if (rc) return rc;
    }
    const int kc = k + 8 < n ? k + 8 : n;
    hipLaunchKernelGGL(k_knn_select, dim3(nq), dim3(256), 0, s, (const float*)V, (long long)n, table, queries, n, dv, k, kc,
                       (long long*)out_idx, out_dist, status);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}
