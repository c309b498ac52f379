// ncx_forward.hip -- the forward entry points of the C ABI (include/neuralcx.h) and their bandwidth-bound kernels around
// the segmented MFMA GEMM engine (ncx_gemm.h) and the fused forward kernel (ncx_main.h).  gfx950 only.
//
// Forward of one batch (B triplets x K candidates, M = B*K rows), replacing vqa/models/cx.py:279-331:
//   k_prep           per row (b,k): feature-table row ids, ||v_o - v_k + 1e-6||_2 (cx.py:300), rank one-hot
//                    (cx.py:304-305) and the softmax statistics of a_knns[b,k,:] (cx.py:281)          [HBM]
//   Gt   = W1[:, a_emb_other] . E^T      [H, A]   re-association of K3: softmax(a).E.W^T = softmax(a).(E.W^T) [MFMA]
//   Sh   = b1 + [v_o | q | z_o | E[aid]] . W1[:, shared cols]^T      [B, H]  once per triplet        [MFMA]
//   h1   = drop(relu(Sh[b] + [v_k | v_o*v_k | dist,rank | z_k | softmax(a_k)] . [W1 slices | Gt]^T)) [MFMA]
//   h2, h3 (L >= 2), scores = h_L . w_out + b_out                                                     [MFMA/HBM]
// The backward mirrors it (ncx_backward.hip).  Nothing here allocates or synchronises.
#include "ncx_driver.h"
#include "ncx_wave.h"
#include "ncx_bf16.h"

namespace ncx {
// One wave per logical row r = b*K + k.  4 rows per 256-thread block.
__device__ __forceinline__ u16 f32_to_bf16(float x) { return __builtin_bit_cast(u16, (__bf16)x); }     // round to nearest even
// 4 consecutive bf16 at an 8-byte aligned position (one store); `valid` < 4 keeps the tail of a segment untouched
__device__ __forceinline__ void store_bf16x4(u16* p, const float (&v)[4], int valid) {
    typedef unsigned short u16x4 __attribute__((ext_vector_type(4)));
    if (valid >= 4) { *(u16x4*)p = u16x4{f32_to_bf16(v[0]), f32_to_bf16(v[1]), f32_to_bf16(v[2]), f32_to_bf16(v[3])}; }
    else { for (int j = 0; j < valid; ++j) p[j] = f32_to_bf16(v[j]); }
}

constexpr int PACK_N = WPAD_N + 1 + PAIR_WPAD_N;      // the padded weight copies of linear_1 / the hidden layers, Gt's pad columns, those of the Gt + Sh pair launch
struct PackArgs { const float* src[PACK_N]; float* dst[PACK_N]; long long lds[PACK_N]; int cols[PACK_N], ldd[PACK_N], zero_from[PACK_N], first[PACK_N + 1]; int n; int nprep; };   // first[e]: entry e's first pack block (its rows follow; first[n]: all of them); nprep: row blocks (4 candidate rows each) in front of the pack blocks
// dst[e][h][0 .. cols) = src[e][h][0 .. cols);  dst[e][h][zero_from .. ldd) = 0.   One block per row h of entry e, which
// ride at the end of k_prep's grid (a launch of their own cost 5 us for 0.5 MB of copies).
__device__ __forceinline__ void pack_rows_block(const PackArgs& a, int idx) {
    int e = 0;
    while (e + 1 < a.n && idx >= a.first[e + 1]) ++e;
    const int h = idx - a.first[e];
    float* drow = a.dst[e] + (long long)h * a.ldd[e];
    if (a.src[e]) {
        const float* srow = a.src[e] + (long long)h * a.lds[e];
        for (int c = threadIdx.x; c < a.cols[e]; c += 256) drow[c] = srow[c];
    }
    for (int c = a.zero_from[e] + threadIdx.x; c < a.ldd[e]; c += 256) drow[c] = 0.f;
}

// One wave per candidate row.  Rows of up to 2048 floats (the real widths: 2048-d features, 2000 answers) are read from
// memory ONCE into registers (8 x float4 per lane) and every pass -- distance, max, sum, bf16 pack -- runs on the
// registers; wider rows (RESIDENT = false) re-read them from memory per pass.  Same per-lane element order and the same
// wave reductions either way, so the results do not depend on the path.
template <bool RESIDENT>
__global__ __launch_bounds__(256) void k_prep(ncx_dims d, ncx_inputs in, int* __restrict__ idx_k,
                                              int* __restrict__ idx_o, int* __restrict__ idx_ob,
                                              float* __restrict__ mx, float* __restrict__ inv,
                                              float* __restrict__ misc, u16* __restrict__ xc, Bf16Cols cc, const PackArgs pk) {
    constexpr int NR = RESIDENT ? 8 : 1;
    const int lane = threadIdx.x & 63;
    const int M = d.B * d.K;
    const int nprep = pk.nprep;                // (M + 3) / 4, or 0 in a pack-only launch (ncx_forward_phase: the weights-only half)
    if ((int)blockIdx.x >= nprep) { pack_rows_block(pk, (int)blockIdx.x - nprep); return; }     // the weight-pack blocks
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const int b = r / d.K, k = r - b * d.K;
    // RESIDENT: every row load is an UNCONDITIONAL 16-byte window (slid left at the row end, repaired below); the guarded form
    // put each load in its own basic block behind an s_waitcnt vmcnt(0): 24 serialised round trips per row, 2 TB/s.
    // The answer-logit row needs no index, so its loads go first; the two feature rows follow their indices.
    const bool aemb_ = d.flags & NCX_F_A_EMB;
    f32x4 ra[NR];
    if (RESIDENT && aemb_) {
        const float* arow = in.a_knns + (long long)r * d.A;
#pragma unroll
        for (int i = 0; i < NR; ++i) ra[i] = load_window(arow, lane * 4 + 256 * i, d.A);
    }
    const int io = in.img_idx[(long long)b * (d.K + 1)];
    const int ik = in.img_idx[(long long)b * (d.K + 1) + 1 + k];
    if (lane == 0) { idx_o[r] = io; idx_k[r] = ik; if (k == 0) idx_ob[b] = io; }
    const float* vo = in.feats + (long long)io * d.dv;
    const float* vk = in.feats + (long long)ik * d.dv;
    u16* xr = xc ? xc + (long long)r * cc.kc : nullptr;
    const bool own_dist = (d.flags & NCX_F_V_DIST) && !(d.flags & NCX_F_PRIV_DIST_IN_MAIN);
    const bool need_v = own_dist || xc;

    f32x4 ro[NR], rk[NR];
    if (RESIDENT && need_v) {
#pragma unroll
        for (int i = 0; i < NR; ++i) { ro[i] = load_window(vo, lane * 4 + 256 * i, d.dv); rk[i] = load_window(vk, lane * 4 + 256 * i, d.dv); }
        if (d.dv % 256 != 0) {                     // (uniform: whole 256-column passes need no repair)
#pragma unroll
            for (int i = 0; i < NR; ++i) { ro[i] = fix_window(ro[i], lane * 4 + 256 * i, d.dv); rk[i] = fix_window(rk[i], lane * 4 + 256 * i, d.dv); }
        }
    }
    auto v_at = [&](int i, int c, f32x4& a, f32x4& e) __attribute__((always_inline)) {
        if (RESIDENT) { a = ro[i]; e = rk[i]; } else { a = load4(vo, c, d.dv); e = load4(vk, c, d.dv); }
    };
    float dist = 0.f;
    if (own_dist) {
        float s = 0.f;
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int c = lane * 4 + 256 * i;
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < d.dv) { const float t = ro[i][j] - rk[i][j] + 1e-6f; s += t * t; }
            }
        } else {
            for (int c = lane * 4; c < d.dv; c += 256) {
                f32x4 a, e; v_at(0, c, a, e);
#pragma unroll
                for (int j = 0; j < 4; ++j)
                    if (c + j < d.dv) { const float t = a[j] - e[j] + 1e-6f; s += t * t; }
            }
        }
        dist = sqrtf(wave_sum(s));
    }
    const int mw = pad_to(d.K + 1, 4);                        // (zero padded to whole 16-byte windows: ncx_main.h)
    float* mrow = misc + (long long)r * mw;
    if (lane == 0) mrow[0] = dist;
    for (int j = lane; j < mw - 1; j += 64)
        mrow[1 + j] = j >= d.K ? 0.f : (d.flags & NCX_F_V_RANK) ? (j == k ? 1.f : 0.f) : in.v_rank[((long long)r) * d.K + j];
    if (xc) {               // NCX_F_BF16: [ v_k | v_o * v_k | dist, rank | z_k | softmax (below) ], zero in the gaps
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < NR; ++i) {
                const int c = lane * 4 + 256 * i;
                if (c < cc.c_vm) {                                     // (segments are padded to multiples of 8 columns)
                    float pk[4], pm[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) { pk[j] = rk[i][j]; pm[j] = ro[i][j] * rk[i][j]; }   // load4: zero beyond dv
                    store_bf16x4(xr + cc.c_vk + c, pk, 4);
                    store_bf16x4(xr + cc.c_vm + c, pm, 4);
                }
            }
        } else {
            for (int c = lane * 4; c < cc.c_vm; c += 256) {
                f32x4 a, e; v_at(0, c, a, e);
                float pk[4], pm[4];
#pragma unroll
                for (int j = 0; j < 4; ++j) { pk[j] = e[j]; pm[j] = a[j] * e[j]; }
                store_bf16x4(xr + cc.c_vk + c, pk, 4);
                store_bf16x4(xr + cc.c_vm + c, pm, 4);
            }
        }
        for (int j = lane; j < cc.c_z - cc.c_misc; j += 64)
            xr[cc.c_misc + j] = f32_to_bf16(j == 0 ? dist : (j <= d.K && j - 1 == k ? 1.f : 0.f));
        const float* zk = in.z_knns + (long long)r * d.dz;
        for (int c = lane * 4; c < cc.c_p - cc.c_z; c += 256) {
            float pz[4];
            const f32x4 z4 = load4(zk, c, d.dz);
#pragma unroll
            for (int j = 0; j < 4; ++j) pz[j] = z4[j];
            store_bf16x4(xr + cc.c_z + c, pz, 4);
        }
        for (int c = cc.raw + lane; c < cc.kc; c += 64) xr[c] = 0;
    }

    if (d.flags & NCX_F_A_EMB) {
        const float* a = in.a_knns + (long long)r * d.A;
        if (RESIDENT && d.A % 256 != 0) {
#pragma unroll
            for (int i = 0; i < NR; ++i) ra[i] = fix_window(ra[i], lane * 4 + 256 * i, d.A);
        }
        float m = -INFINITY;
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) if (lane * 4 + 256 * i + j < d.A) m = fmaxf(m, ra[i][j]);
        } else {
            for (int c = lane * 4; c < d.A; c += 256) {
                const f32x4 v = load4(a, c, d.A);
#pragma unroll
                for (int j = 0; j < 4; ++j) if (c + j < d.A) m = fmaxf(m, v[j]);
            }
        }
        m = wave_max(m);
        float s = 0.f;
        if (RESIDENT) {
#pragma unroll
            for (int i = 0; i < NR; ++i)
#pragma unroll
                for (int j = 0; j < 4; ++j) if (lane * 4 + 256 * i + j < d.A) s += __expf(ra[i][j] - m);
        } else {
            for (int c = lane * 4; c < d.A; c += 256) {
                const f32x4 v = load4(a, c, d.A);
#pragma unroll
                for (int j = 0; j < 4; ++j) if (c + j < d.A) s += __expf(v[j] - m);
            }
        }
        s = wave_sum(s);
        // base-2 log-sum-exp: softmax(a)[c] = exp2(a[c]*log2e - lse2)
        const float lse2 = m * 1.44269504088896341f + __log2f(s);
        if (lane == 0) { mx[r] = lse2; inv[r] = 0.f; }
        if (xc) {           // NCX_F_BF16: the softmax row itself, rounded to bf16, is the last segment of the packed row
            u16* xp = xr + cc.c_p;
            if (RESIDENT) {
#pragma unroll
                for (int i = 0; i < NR; ++i) {
                    const int c = lane * 4 + 256 * i;
                    if (c < d.A) {
                        float e[4];
#pragma unroll
                        for (int j = 0; j < 4; ++j) e[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(ra[i][j], 1.44269504088896341f, -lse2));
                        store_bf16x4(xp + c, e, d.A - c);
                    }
                }
            } else {
                for (int c = lane * 4; c < d.A; c += 256) {
                    const f32x4 v = load4(a, c, d.A);
                    float e[4];
#pragma unroll
                    for (int j = 0; j < 4; ++j) e[j] = __builtin_amdgcn_exp2f(__builtin_fmaf(v[j], 1.44269504088896341f, -lse2));
                    store_bf16x4(xp + c, e, d.A - c);
                }
            }
        }
    }
}

// scores[r] = h[r,:] . w + b     (cx.py:327); one wave per row.
__global__ __launch_bounds__(256) void k_scores(const float* __restrict__ h, const float* __restrict__ w,
                                                const float* __restrict__ bias, float* __restrict__ scores,
                                                int M, int H) {
    const int lane = threadIdx.x & 63;
    const int r = blockIdx.x * 4 + (threadIdx.x >> 6);
    if (r >= M) return;
    const float* row = h + (long long)r * H;
    float s = 0.f;
    for (int c = lane * 4; c < H; c += 256) {
        const f32x4 a = load4(row, c, H), e = load4(w, c, H);
        s += dot4(a, e);
    }
    s = wave_sum(s);
    if (lane == 0) scores[r] = s + bias[0];
}

// The route of linear_1 on the fused forward kernel (ncx_plan.h): forward_impl launches by it, NCX_QUERY_FWD_ROUTE reports it.
FwdRoute forward_route(const ncx_dims& d, const StepRoutes& r) {
    const long long M = (long long)d.B * d.K, H = d.H, din = seg_offsets(d).din;
    const long long main_T = r.cand_ksteps;
    FwdRoute f{};
    // K = 24, whole 32-column tiles, no k-split: the two v segments as one pass with the per-triplet fold (ncx_main.h, MK_VFOLD)
    // (K = 48: on 96-row tiles only -- two triplets per tile -- so only where those fill the chip)
    f.vfold = main_fwd_dims_ok(d) && (d.flags & NCX_F_V_MULT) && (d.K == 24 || (d.K == 48 && (main_fold_rows(M, H) >= 96 || hook_env("NCX_FOLD4") || hook_env("NCX_FOLD8")))) && d.dv % 32 == 0 && d.dv >= 64 &&
              main_split(M, H, main_T) == 1 && !hook_env("NCX_NO_VFOLD") &&
              (long long)d.n_img * d.dv * 4 < (1ll << 32) - 65536 && (long long)H * din * 4 < (1ll << 32) - 65536;      // (the fold's buffer loads: 32-bit byte offsets)
    // The pairwise distance rides in the fused forward kernel when that kernel sees whole v rows (no k-split, no slid windows).
    // Measured at configs[1]: inside the plain chain the distance costs the kernel 12 us and saves k_prep 30; inside the fold's
    // 48 x 64 tiles (a quarter of the MFMA work per vector instruction) it costs 31 us: there k_prep keeps computing it.
    // Round 4, measured again for the one-triplet-per-wave fold forms (96 / 192-row tiles, K = 24: a wave's loader holds v_o beside every v_k quad it loads,
    // the distance is ~14 vector operations per loaded quad and k_prep stops reading the feature rows): the fold loop goes from 5 085 to 5 790 cycles per k-step
    // (5 740 with the arithmetic spread over the sub-steps) -- vector instructions are not free under fp32 MFMAs, each costs the matrix pipe ~8-15 cycles --
    // so the kernel loses the 17 us k_prep gains (0.2938 against 0.2771 ms; step 0.8443 / 0.8483 against 0.8489).  Kept behind the hook NCX_DIST_IN_FOLD.
    f.dist_in_fold = f.vfold && d.K == 24 && main_fold_rows_eff(M, H, d.K) >= 96 && !(d.flags & NCX_F_X6) && hook_env("NCX_DIST_IN_FOLD");
    f.dist_in_main = main_fwd_dims_ok(d) && (d.flags & NCX_F_V_DIST) && (d.flags & NCX_F_V_MULT) && d.dv % 32 == 0 &&
                     main_split(M, H, main_T) == 1 && (!f.vfold || f.dist_in_fold) && !(hook_env("NCX_NO_DIST_IN_MAIN"));
    return f;
}
}  // namespace ncx

using namespace ncx;
extern "C" {
const char* ncx_version(void) { return "neuralcx-hip gfx950 fp32-mfma r4 (" __DATE__ ")"; }

int64_t ncx_input_size(const ncx_dims* d) { return d ? (int64_t)seg_offsets(*d).din : 0; }

size_t ncx_workspace_bytes(const ncx_dims* d) {
    if (check_dims(d) != NCX_OK) return 0;
    return ws_layout(*d).total;
}

// phase 0: everything.  phase 1 (NCX_FWD_PRELUDE): the part that is a function of the DATA only -- k_prep's row pass (table row
// ids, pairwise distance, rank one-hot, softmax statistics of the answer logits; the bf16 variant's row pack) -- so a
// data-parallel job can run it for step n + 1 while step n's last gradient bucket is still on the wire and its weights are
// not final.  phase 2 (NCX_FWD_REST): everything that reads the weights (the padded weight copies, Gt, Sh, the Linear layers,
// the scores).  1 then 2 == 0 bit for bit: the same kernels on the same operands, k_prep's launch cut between its row blocks
// and its weight-pack blocks.
static int forward_impl(const ncx_dims* dp, const ncx_inputs* in, const ncx_params* p, void* workspace,
                        size_t workspace_bytes, float* scores, void* stream_, int phase) {
    int rc = check_dims(dp);
    if (rc != NCX_OK) return rc;
    const bool do_pre = phase != 2, do_rest = phase != 1;
    if (!in || !p || !workspace || (do_rest && !scores && !(dp->flags & NCX_F_FUSED_TAIL))) return NCX_E_NULL;
    const ncx_dims& d = *dp;
    const bool aemb = d.flags & NCX_F_A_EMB;
    if (!in->feats || !in->img_idx || !in->q_emb || !in->z_orig || !in->z_knns || !in->a_knns) return NCX_E_NULL;
    if (aemb && (!in->answer_aids || !p->answer_embedding)) return NCX_E_NULL;
    if (!aemb && !in->a_emb_gt) return NCX_E_FLAGS;
    if (!(d.flags & NCX_F_V_RANK) && !in->v_rank) return NCX_E_FLAGS;
    if (!p->w1 || !p->b1 || !p->w_out || !p->b_out) return NCX_E_NULL;
    if (d.L >= 2 && (!p->w2 || !p->b2)) return NCX_E_NULL;
    if (d.L >= 3 && (!p->w3 || !p->b3)) return NCX_E_NULL;
    const StepRoutes r = routes(d);
    const WsLayout w = ws_layout(d, r);
    if (!ws_ok(workspace, workspace_bytes, w.total)) return NCX_E_WORKSPACE;
    hipStream_t s = (hipStream_t)stream_;
    char* ws = (char*)workspace;
    const int M = d.B * d.K, H = d.H;
    const SegOffsets o = seg_offsets(d);
    const long long din = o.din;
    int* idx_k = (int*)(ws + w.idx_k); int* idx_o = (int*)(ws + w.idx_o); int* idx_ob = (int*)(ws + w.idx_ob);
    float* mx = (float*)(ws + w.mx); float* inv = (float*)(ws + w.inv); float* misc = (float*)(ws + w.misc);
    float* gt = (float*)(ws + w.gt); float* sh = (float*)(ws + w.sh); float* slab = (float*)(ws + w.slab);
    GemmUse u[U_COUNT];
    list_uses(d, r, u);

    // k_prep (HBM-bound) on the caller's stream  ||  Gt, Sh (small MFMA GEMMs; Sh only needs idx_ob, which k_prep
    // produces, so it gathers through img_idx directly) on the side stream
    SideStream* ss = side_stream();
    if (ss && ss->mode == 3) ss = nullptr;
    hipStream_t s2 = ss ? ss->s : s;
    float* slab_side = ss ? (float*)(ws + w.slab2) : slab;
    const size_t slab_side_bytes = ss ? w.slab2_bytes : w.slab_bytes;
    if (ss) { rc = side_fork(ss, s); if (rc) return rc; }
    const bool bf16 = d.flags & NCX_F_BF16;
    u16* xc = bf16 ? (u16*)(ws + w.xc) : nullptr;
    // zero-padded copies of the weight slices the fused forward kernel reads past their width (+ the pad columns of Gt):
    // functions of the weights only, like Gt -- evaluation passes reuse them (NCX_F_REUSE_GT)
    struct { const float* ptr[WPAD_N]; int width[WPAD_N]; } wp{};
    // Gt and Sh as one launch of the fused forward kernel's 64 x 64 form (StepRoutes::gtsh_pair); its weight sides are padded like linear_1's
    const bool pair = r.gtsh_pair(d, ss != nullptr);
    struct { const float* ptr[PAIR_WPAD_N]; int width[PAIR_WPAD_N]; } pw{};
    PackArgs pk{};
    auto pack = [&](const float* src, long long lds, int cols, float* dst, int ldd, int zero_from, int rows) {
        const int e = pk.n++;
        pk.src[e] = src; pk.lds[e] = lds; pk.cols[e] = cols; pk.dst[e] = dst; pk.ldd[e] = ldd; pk.zero_from[e] = zero_from; pk.first[e + 1] = pk.first[e] + rows;
    };
    {
        const float* srcs[WPAD_N] = {p->w1 + o.v_other, p->w1 + o.v_mult, p->w1 + o.v_dist, p->w1 + o.z_other, p->w1 + o.a_other, p->w2, p->w3};
        float* cur = (float*)(ws + w.wpad);
        for (int i = 0; i < WPAD_N; ++i) {
            wp.width[i] = wpad_width(d, i); wp.ptr[i] = cur;
            if (!wp.width[i]) continue;
            pack(srcs[i], (i == 5 || i == 6) ? H : din, wpad_cols(d, i), cur, wp.width[i], wpad_cols(d, i), H);
            cur += (size_t)H * wp.width[i];
        }
        if (aemb && w.ldgt > d.A) pack(nullptr, 0, 0, gt, w.ldgt, d.A, H);
        if (pair) {
            const float* psrc[PAIR_WPAD_N] = {p->w1 + o.v_orig, p->w1 + o.q_emb, p->w1 + o.z_orig, p->w1 + o.a_gt, p->answer_embedding};
            const int pcols[PAIR_WPAD_N] = {d.dv, d.dq, d.dz, d.da, d.da};
            float* pcur = (float*)(ws + w.pwpad);
            for (int i = 0; i < PAIR_WPAD_N; ++i) {
                const int rows = i == 4 ? d.A : H;
                pw.width[i] = pair_wpad_width(d, r, i); pw.ptr[i] = pcur;
                if (!pw.width[i]) continue;
                pack(psrc[i], i == 4 ? d.da : din, pcols[i], pcur, pw.width[i], pcols[i], rows);
                pcur += (size_t)rows * pw.width[i];
            }
        }
        if (d.flags & NCX_F_REUSE_GT) pk.n = 0;
    }
    // the per-triplet fold of the two v segments, and the pairwise distance inside the fused forward kernel (forward_route, above)
    const FwdRoute fr = forward_route(d, r);
    const bool vfold = fr.vfold, dist_in_main = fr.dist_in_main;
    ncx_dims dprep = d;
    if (dist_in_main) dprep.flags |= NCX_F_PRIV_DIST_IN_MAIN;
    if (!do_rest) pk.n = 0;                                   // prelude: no weight is read
    pk.nprep = do_pre ? (int)cdiv(M, 4) : 0;                  // rest: the pack blocks alone
    const unsigned prep_grid = (unsigned)(pk.nprep + (long long)pk.first[pk.n]);
    if (prep_grid > 0) {
        if (d.dv <= 2048 && d.A <= 2048)
            hipLaunchKernelGGL(k_prep<true>, dim3(prep_grid), dim3(256), 0, s, dprep, *in, idx_k, idx_o, idx_ob, mx, inv, misc, xc, bf16_cols(d), pk);
        else
            hipLaunchKernelGGL(k_prep<false>, dim3(prep_grid), dim3(256), 0, s, dprep, *in, idx_k, idx_o, idx_ob, mx, inv, misc, xc, bf16_cols(d), pk);
        NCX_HIP_TRY(hipGetLastError());
    }
    if (!do_rest) {
        if (ss) { rc = side_join(ss, s); if (rc) return rc; }
        return NCX_OK;
    }

    // Gt and Sh are two back-to-back split GEMMs on 64 x 64 tiles: their fix-ups (6 us each, mostly launch and ramp) run as one
    FixupArgs fix_gt{}, fix_sh{};
    const bool merge_fix = !ss && !bf16 && aemb && !(d.flags & NCX_F_REUSE_GT) && u[U_GT].plan.cfg == u[U_SH].plan.cfg &&
                           !hook_env("NCX_NO_MERGE_FIX");
    // Gt[H, A] = W1[:, a_other] . E^T   (weights only: evaluation passes reuse it, NCX_F_REUSE_GT)
    if (pair) {
        // ... and Sh in ONE launch of 64 x 64 tiles split by the joint plan, one fix-up behind it: the two products are independent, and on launches
        // of their own each pays the chip's ramp and drain for k-chunks too short to amortise it
        auto seg = [&](MainArgs& a, int i, int kind, const float* x, long long lda, int klen, const int* idx, int slot, const float* wgt, long long ldb) {
            MainSeg& g = a.seg[i]; g.kind = kind; g.a = x; g.lda = lda; g.idx = idx; g.klen = klen;
            if (slot >= 0 && pw.width[slot]) { g.b = pw.ptr[slot]; g.ldb = pw.width[slot]; } else { g.b = wgt; g.ldb = ldb; } };
        float* const pslab = (float*)(ws + w.slab2);
        const size_t gt_elems = (size_t)r.pair_s_gt * H * d.A, sh_elems = (size_t)r.pair_s_sh * d.B * H;
        if ((gt_elems + sh_elems) * 4 > w.slab2_bytes) return NCX_E_WORKSPACE;
        MainArgs ag{}; ag.M = H; ag.N = d.A; ag.nseg = 4;          // Gt rides in the plain slot of the one kind sequence; its other segments are empty
        seg(ag, 0, MK_GATHER, nullptr, 0, 0, nullptr, -1, nullptr, 0);
        seg(ag, 1, MK_PLAIN, p->w1 + o.a_other, din, d.da, nullptr, 4, p->answer_embedding, d.da);
        seg(ag, 2, MK_PLAIN, nullptr, 0, 0, nullptr, -1, nullptr, 0);
        seg(ag, 3, MK_GATHER, nullptr, 0, 0, nullptr, -1, nullptr, 0);
        ag.out = gt; ag.ldo = w.ldgt; ag.split = r.pair_s_gt; ag.slab = pslab;
        MainArgs as{}; as.M = d.B; as.N = H; as.nseg = 4;
        seg(as, 0, MK_GATHER, in->feats, d.dv, d.dv, idx_ob, 0, p->w1 + o.v_orig, din);
        seg(as, 1, MK_PLAIN, in->q_emb, d.dq, d.dq, nullptr, 1, p->w1 + o.q_emb, din);
        seg(as, 2, MK_PLAIN, in->z_orig, d.dz, d.dz, nullptr, 2, p->w1 + o.z_orig, din);
        seg(as, 3, MK_GATHER, p->answer_embedding, d.da, d.da, in->answer_aids, 3, p->w1 + o.a_gt, din);
        as.out = sh; as.ldo = H; as.split = r.pair_s_sh; as.slab = pslab + gt_elems; as.epi.bias = p->b1;
        // (the chunks are the generic engine's, so Gt and Sh are the bits of the two launches below; the joint plan only shares them among fewer workgroups)
        rc = profiled(U_SH, s, [&] { return main_forward_pair(ag, as, r.pair_s_gt / r.pair_w_gt, r.pair_s_sh / r.pair_w_sh, s); }); if (rc) return rc;
    } else
    if (aemb && bf16 && !(d.flags & NCX_F_REUSE_GT)) {       // bf16 copies of E / W1[:, a_*] (also the backward's operands)
        const Bf16Emb m = bf16_emb_layout(d, ws + w.bf_emb);
        rc = bf16_pack_embedding(d, p->answer_embedding, p->w1, m, s2); if (rc) return rc;
        rc = profiled(U_GT, s2, [&] { return bf16_gt(d, m, gt, s2); }); if (rc) return rc;
    } else if (aemb && !(d.flags & NCX_F_REUSE_GT)) {
        GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = H;
        a.a[0] = x_plain(p->w1 + o.a_other, din, H, d.da);
        a.b[0] = x_plain(p->answer_embedding, d.da, d.A, d.da);
        a.klen[0] = d.da; a.out[0] = gt; a.ldo[0] = w.ldgt; a.n_cols[0] = d.A;
        if (merge_fix) a.defer_fix = &fix_gt;                  // (its partial tiles wait in the side slab for the merged fix-up below)
        rc = run_gemm(U_GT, a, FORM_NT, u[U_GT].plan, merge_fix ? (float*)(ws + w.slab2) : slab_side,
                      merge_fix ? w.slab2_bytes : slab_side_bytes, nullptr, s2);
        if (rc) return rc;
    }
    // Sh[B, H] = b1 + shared segments
    if (!pair) {
        GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 4; a.M = d.B;
        a.a[0] = ss ? x_gather_strided(in->feats, d.dv, in->img_idx, d.K + 1, d.B, d.dv)      // (idx_ob is written by k_prep, concurrently)
                    : x_gather(in->feats, d.dv, idx_ob, d.B, d.dv);
        a.b[0] = x_plain(p->w1 + o.v_orig, din, H, d.dv); a.klen[0] = d.dv;
        a.a[1] = x_plain(in->q_emb, d.dq, d.B, d.dq);            a.b[1] = x_plain(p->w1 + o.q_emb, din, H, d.dq);  a.klen[1] = d.dq;
        a.a[2] = x_plain(in->z_orig, d.dz, d.B, d.dz);           a.b[2] = x_plain(p->w1 + o.z_orig, din, H, d.dz); a.klen[2] = d.dz;
        a.a[3] = aemb ? x_gather(p->answer_embedding, d.da, in->answer_aids, d.B, d.da)
                      : x_plain(in->a_emb_gt, d.da, d.B, d.da);
        a.b[3] = x_plain(p->w1 + o.a_gt, din, H, d.da); a.klen[3] = d.da;
        a.out[0] = sh; a.ldo[0] = H; a.n_cols[0] = H;
        if (merge_fix) a.defer_fix = &fix_sh;
        rc = run_gemm(U_SH, a, FORM_NT, u[U_SH].plan, slab_side, slab_side_bytes, p->b1, s2);
        if (rc) return rc;
        if (merge_fix) { rc = run_fixup2(fix_gt, fix_sh, u[U_SH].plan.cfg, s); if (rc) return rc; }   // Gt's and Sh's reductions: one launch
        if (ss) { rc = side_join(ss, s); if (rc) return rc; }
    }
    // h1 = drop(relu(Sh[b] + candidate segments))
    if (bf16) {     // plain bf16 product of the packed rows with the packed weights (Wc repacked every step: weights move)
        rc = bf16_pack_wc(d, p->w1, gt, (u16*)(ws + w.wc), s); if (rc) return rc;
        EpiArgs e{};
        e.rowadd = sh; e.ld_rowadd = H; e.rowdiv = d.K;
        set_dropout(e, d, *in, 1, M);
        rc = profiled(U_MAIN, s, [&] { return bf16_main_forward(d, xc, (const u16*)(ws + w.wc), e, (float*)(ws + w.h[0]), s); }); if (rc) return rc;
    } else if (main_fwd_dims_ok(d)) {        // the fused forward kernel (ncx_main.h): weights zero-padded to 32 columns
        MainArgs a{}; a.M = M; a.N = H; a.x6 = (d.flags & NCX_F_X6) && !hook_env("NCX_NO_X6") && !hook_env("NCX_NO_MAIN_X6");
        int n = 0;
        auto seg = [&](int kind, const float* x, long long lda, int klen, const int* i1, const int* i2, const float* lse, int slot, const float* wgt, long long ldb) {
            MainSeg& g = a.seg[n++]; g.kind = kind; g.a = x; g.lda = lda; g.idx = i1; g.idx2 = i2; g.lse = lse; g.klen = klen;
            if (slot >= 0 && wp.width[slot]) { g.b = wp.ptr[slot]; g.ldb = wp.width[slot]; } else { g.b = wgt; g.ldb = ldb; } };
        if (vfold) {
            seg(MK_VFOLD, in->feats, d.dv, d.dv, idx_k, idx_o, nullptr, -1, p->w1 + o.v_other, din);
            a.seg[0].b2 = p->w1 + o.v_mult;
        } else {
            seg(MK_GATHER, in->feats, d.dv, d.dv, idx_k, nullptr, nullptr, 0, p->w1 + o.v_other, din);
            if (d.flags & NCX_F_V_MULT) seg(MK_GATHER_MUL, in->feats, d.dv, d.dv, idx_k, idx_o, nullptr, 1, p->w1 + o.v_mult, din);
        }
        seg(MK_PLAIN, misc, w.ldm, w.ldm, nullptr, nullptr, nullptr, 2, p->w1 + o.v_dist, din);       // (ldm - K - 1 zero columns on both sides)
        seg(MK_PLAIN, in->z_knns, d.dz, d.dz, nullptr, nullptr, nullptr, 3, p->w1 + o.z_other, din);
        if (aemb) seg(MK_SOFTMAX, in->a_knns, d.A, d.A, nullptr, nullptr, mx, -1, gt, w.ldgt);
        else      seg(MK_PLAIN, in->a_knns, d.da, d.da, nullptr, nullptr, nullptr, 4, p->w1 + o.a_other, din);
        a.nseg = n;
        a.out = (float*)(ws + w.h[0]); a.ldo = H;
        a.epi.rowadd = sh; a.epi.ld_rowadd = H; a.epi.rowdiv = d.K;
        set_dropout(a.epi, d, *in, 1, M);
        if (dist_in_main) { a.dist_out = misc; a.ld_dist = w.ldm; }
        {
            long long T = 0; for (int i = 0; i < n; ++i) T += ksteps(a.seg[i].klen);
            a.split = main_split(M, H, T); a.slab = (float*)(ws + w.mslab);
            if (a.split > 1 && (size_t)a.split * M * H * 4 > w.mslab_bytes) return NCX_E_WORKSPACE;
        }
        if (a.split <= 1) a.stamps = stamps_for_current_device((long long)(((M + 47) / 48 + 7) / 8 * 8) * ((H + 63) / 64) * 16);   // (bound: the smallest tile = the most workgroups; null unless armed on THIS device)
        rc = profiled(U_MAIN, s, [&] { return main_forward(a, s); }); if (rc) return rc;
    } else {                                  // widths that are not multiples of 4: the generic segmented engine
        GemmArgs a{}; a.mode = MODE_CHAIN; a.M = M;
        int n = 0;
        a.a[n] = x_gather(in->feats, d.dv, idx_k, M, d.dv); a.b[n] = x_plain(p->w1 + o.v_other, din, H, d.dv); a.klen[n] = d.dv; ++n;
        if (d.flags & NCX_F_V_MULT) {
            a.a[n] = x_gather_mul(in->feats, d.dv, idx_k, idx_o, M, d.dv); a.b[n] = x_plain(p->w1 + o.v_mult, din, H, d.dv); a.klen[n] = d.dv; ++n;
        }
        a.a[n] = x_plain(misc, w.ldm, M, d.K + 1); a.b[n] = x_plain(p->w1 + o.v_dist, din, H, d.K + 1); a.klen[n] = d.K + 1; ++n;
        a.a[n] = x_plain(in->z_knns, d.dz, M, d.dz); a.b[n] = x_plain(p->w1 + o.z_other, din, H, d.dz); a.klen[n] = d.dz; ++n;
        if (aemb) { a.a[n] = x_softmax(in->a_knns, d.A, mx, inv, M, d.A); a.b[n] = x_plain(gt, w.ldgt, H, d.A); a.klen[n] = d.A; ++n; }
        else      { a.a[n] = x_plain(in->a_knns, d.da, M, d.da); a.b[n] = x_plain(p->w1 + o.a_other, din, H, d.da); a.klen[n] = d.da; ++n; }
        a.nseg = n;
        a.out[0] = (float*)(ws + w.h[0]); a.ldo[0] = H; a.n_cols[0] = H;
        a.epi.rowadd = sh; a.epi.ld_rowadd = H; a.epi.rowdiv = d.K;
        set_dropout(a.epi, d, *in, 1, M);
        rc = run_gemm(U_MAIN, a, FORM_NT, u[U_MAIN].plan, slab, w.slab_bytes, nullptr, s);
        if (rc) return rc;
    }
    for (int l = 2; l <= d.L; ++l) {
        const float* wl = l == 2 ? p->w2 : p->w3;
        const float* bl = l == 2 ? p->b2 : p->b3;
        if (hidden_fwd_dims_ok(d) && !bf16) {
            MainArgs a{}; a.M = M; a.N = H; a.nseg = 1;
            MainSeg& g = a.seg[0]; g.kind = MK_PLAIN; g.a = (const float*)(ws + w.h[l - 2]); g.lda = H; g.klen = H;
            const int slot = 3 + l;                                       // 5: linear_2, 6: linear_3
            if (wp.width[slot]) { g.b = wp.ptr[slot]; g.ldb = wp.width[slot]; } else { g.b = wl; g.ldb = H; }
            a.out = (float*)(ws + w.h[l - 1]); a.ldo = H;
            a.epi.bias = bl;
            set_dropout(a.epi, d, *in, l, M);
            a.split = main_split(M, H, ksteps(H)); a.slab = (float*)(ws + w.mslab);
            if (a.split > 1 && (size_t)a.split * M * H * 4 > w.mslab_bytes) return NCX_E_WORKSPACE;
            rc = profiled(U_FWD_L, s, [&] { return main_forward(a, s); }); if (rc) return rc;
        } else {
            GemmArgs a{}; a.mode = MODE_CHAIN; a.nseg = 1; a.M = M;
            a.a[0] = x_plain((const float*)(ws + w.h[l - 2]), H, M, H); a.b[0] = x_plain(wl, H, H, H); a.klen[0] = H;
            a.out[0] = (float*)(ws + w.h[l - 1]); a.ldo[0] = H; a.n_cols[0] = H;
            a.epi.bias = bl;
            set_dropout(a.epi, d, *in, l, M);
            rc = run_gemm(U_FWD_L, a, FORM_NT, u[U_FWD_L].plan, slab, w.slab_bytes, nullptr, s);
            if (rc) return rc;
        }
    }
    if (d.flags & NCX_F_FUSED_TAIL) return NCX_OK;       // the out layer runs in ncx_train_tail
    hipLaunchKernelGGL(k_scores, dim3((unsigned)cdiv(M, 4)), dim3(256), 0, s, (const float*)(ws + w.h[d.L - 1]),
                       p->w_out, p->b_out, scores, M, H);
    NCX_HIP_TRY(hipGetLastError());
    return NCX_OK;
}

int ncx_forward(const ncx_dims* dp, const ncx_inputs* in, const ncx_params* p, void* workspace,
                size_t workspace_bytes, float* scores, void* stream_) {
    return forward_impl(dp, in, p, workspace, workspace_bytes, scores, stream_, 0);
}

int ncx_forward_phase(const ncx_dims* dp, const ncx_inputs* in, const ncx_params* p, void* workspace,
                      size_t workspace_bytes, float* scores, int32_t phase, void* stream_) {
    if (phase < 0 || phase > 2) return NCX_E_FLAGS;
    return forward_impl(dp, in, p, workspace, workspace_bytes, scores, stream_, phase);
}
}  // extern "C"
