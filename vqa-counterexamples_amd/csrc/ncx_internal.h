// ncx_internal.h -- declarations shared by the translation units of libneuralcx_hip.so.
#pragma once
#include "ncx_common.h"
#include "ncx_gemm.h"
#include "ncx_adam.h"

namespace ncx {

enum TileCfg : int { CFG_64x64 = 0, CFG_128x128 = 1, CFG_96x128 = 2, CFG_96x64 = 3, CFG_128x64 = 4 };
enum GemmForm : int { FORM_NT = 0, FORM_TN = 1, FORM_NN = 2 };
// The tile configs run_gemm_nt / _tn / _nn (ncx_gemm_inst.hip) instantiate for a form.  Any other value falls through their `default:` to
// 64x64 while default_splits and run_fixup2 size by cfg_tile(cfg): whoever takes a cfg from outside the planner asks here first.
static inline bool cfg_supported(int form, int cfg) {
    switch (form) {
    case FORM_NT: return cfg == CFG_64x64 || cfg == CFG_128x128 || cfg == CFG_96x128 || cfg == CFG_96x64;
    case FORM_TN: return cfg == CFG_64x64 || cfg == CFG_128x128 || cfg == CFG_128x64;
    case FORM_NN: return cfg == CFG_64x64 || cfg == CFG_128x128;
    default:      return false;
    }
}

int run_gemm_nt(GemmArgs& a, int cfg, hipStream_t s);
int run_fixup2(const FixupArgs& a, const FixupArgs& b, int cfg, hipStream_t s);
int run_gemm_nt_fold(GemmArgs& a, hipStream_t s);
int run_gemm_tn(GemmArgs& a, int cfg, hipStream_t s);
int run_gemm_nn(GemmArgs& a, int cfg, hipStream_t s);
int occupancy_nt(int cfg);
int occupancy_tn(int cfg);
int occupancy_nn(int cfg);

// Column offsets of the reference's concat (vqa/models/cx.py:309-320) == layout of linear_1.weight.
struct SegOffsets {
    int v_orig, v_other, v_mult, v_dist, v_rank, q_emb, z_orig, z_other, a_gt, a_other, din;
};
static inline SegOffsets seg_offsets(const ncx_dims& d) {
    SegOffsets o; int c = 0;
    o.v_orig = c;  c += d.dv;
    o.v_other = c; c += d.dv;
    o.v_mult = c;  c += d.dv;
    o.v_dist = c;  c += 1;
    o.v_rank = c;  c += d.K;
    o.q_emb = c;   c += d.dq;
    o.z_orig = c;  c += d.dz;
    o.z_other = c; c += d.dz;
    o.a_gt = c;    c += d.da;
    o.a_other = c; c += d.da;
    o.din = c;
    return o;
}

// Split-K plan of one GEMM: tile config + number of K splits (slabs reduced by k_slab_reduce).
struct GemmPlan { int cfg; int split; };   // split: aligned k-chunks per output tile (1 = none)
GemmPlan plan_gemm(int form, long long M, long long N, long long ksteps, bool allow_96);
int num_cus();
static inline long long cdiv(long long a, long long b) { return (a + b - 1) / b; }
static inline long long ksteps(long long k) { return cdiv(k, GEMM_BK); }      // 32-deep reduction steps of a k extent
// The GEMM driver (ncx_driver.hip) of every launch on the generic engine.  Problems whose a.split[i] is 0 take pl.split (callers
// may preset per-problem splits); a split launch puts its partial tiles in `slab` (NCX_E_WORKSPACE when slab_bytes is short).
// reduce_bias (nullable): applied by the epilogue or by the fix-up kernel.  Hook NCX_NO_FAST, or no_fast (ncx_diag_gemm only): the diagnostic tile path.
// Preconditions (callers keep them; ncx_diag_gemm, ncx_diag.hip, checks them): cfg_supported(form, pl.cfg); every operand has cols >= 4
// (16-byte windows); klen[i] == the operands' reduction extents; a split problem applies bias and activation only (the fix-up drops
// rowadd, dropout, gate and rowsplit_g).
__attribute__((visibility("hidden"))) size_t gemm_slab_bytes(GemmArgs a, const GemmPlan& pl);      // 0 when unsplit
__attribute__((visibility("hidden"))) int run_gemm_planned(GemmArgs& a, int form, const GemmPlan& pl, float* slab, size_t slab_bytes,
                                                           const float* reduce_bias, hipStream_t s, bool no_fast = false);
// ncx_scorers.hip: out[c] = sum over rows r < R of in[r * ld + c], c < cols, in a fixed order (k_colsum)
__attribute__((visibility("hidden"))) hipError_t colsum_rows(const float* in, long long ld, int R, int cols, float* out, hipStream_t s);

// Byte offsets of a workspace's regions, each 256-byte aligned, in the order they are taken (off: the bytes taken so far)
struct WsCarver {
    size_t off = 0;
    size_t take(size_t bytes) { const size_t o = off; off = align_up(off + bytes, 256); return o; }
};
// what every entry point asks of the workspace it is handed: 256-byte aligned and at least `total` bytes (else NCX_E_WORKSPACE)
static inline bool ws_ok(const void* ws, size_t bytes, size_t total) { return bytes >= total && !((uintptr_t)ws & 255); }

// Workspace partition (byte offsets from a 256-byte aligned base).  Saved-for-backward part first.
struct WsLayout {
    size_t idx_k, idx_o, idx_ob;        // int32 [M], [M], [B]: feature-table rows per logical row
    size_t mx, inv;                     // [M] softmax stats of a_knns rows
    size_t misc;                        // [M][K+1]: v_dist column + v_rank block (cx.py:299-307)
    size_t gt;                          // Gt[H][A] = W1[:, a_other] . E^T  (re-associated K3)
    size_t sh;                          // Sh[B][H]: per-triplet shared part of linear_1 (+ bias)
    size_t h[3];                        // post-dropout activations of layers 1..L, [M][H]
    size_t dpre[2];                     // [M][H] ping-pong of pre-activation gradients
    size_t dsh;                         // [B][H]
    size_t dgt;                         // [H][A]
    size_t dagt;                        // dGgt [H][A]  (bf16 variant only; the fp32 path keeps it transposed, below)
    size_t dgtT;                        // fp32 path: dGt^T [A][Hp4] then dGgt^T [A][Hp4] (contiguous: the all-reduce bucket under DP); Hp4 = H up to a multiple of 4
    size_t dgtT2;                       // private copy of dGt^T with zero rows up to a multiple of 32 (A operand of the dW1[:, a_other] launch, ncx_dwtn.hip)
    size_t de_perm;                     // fp32 path: int32 [A + 1]: the batch's present answer ids ascending, then the absent ones ascending; [A] = how many are present (k_emb_prep)
    size_t w1aT;                        // fp32 path: W1[:, a_other]^T then W1[:, a_gt]^T, [da][Hp32] each (zero padded)
    size_t partial;                     // column-sum partials [NCX_COLSUM_CHUNKS][H] x 2 + scalars
    size_t slab;                        // split-K slabs (max over all uses)
    size_t slab_bytes;
    size_t slab2, slab2_bytes;          // slab of the GEMMs that run on the internal side stream
    size_t xc, wc, dpre_bf, bf_slab;    // NCX_F_BF16: packed bf16 candidate rows / weights / dpre, k-chunk slabs of dWc
    size_t bf_emb;                      // NCX_F_BF16: bf16 images of E, E^T, [W1ak; W1agt], [dGt; dGgt]
    size_t km_slab;                     // k-chunk slabs of the fused v_other / v_mult weight gradient (ncx_dwkm.hip)
    size_t mslab, mslab_bytes;          // [split][M][N] partial sums of the fused forward kernel's split problems (max over its uses)
    size_t wpad;                        // zero-padded copies of the weight slices whose width is not a multiple of 32 (ncx_main.h)
    size_t pwpad;                       // ... of the Gt + Sh pair launch's weight sides (W1[:, v_orig | q_emb | z_orig | a_gt], answer_embedding): ncx_plan.h
    int ldm;                            // leading dimension of misc: K + 1 rounded up to a multiple of 4 (zero padded)
    int ldgt;                           // leading dimension of Gt: A rounded up to a multiple of 32 (zero padded); bf16 variant: A
    size_t total;
};
constexpr int NCX_COLSUM_CHUNKS = 256;
constexpr int NCX_PRELUDE_WAVES = 1024;       // waves of k_bwd_prelude = rows of its partial sums (>= NCX_COLSUM_CHUNKS: same buffer)

// ncx_main.hip: the fused forward kernel of the Linear layers (segments of never-materialised operands chained into one
// accumulator; Sh / bias / ReLU / Dropout in the epilogue)
enum MainKind : int { MK_PLAIN = 0, MK_GATHER = 1, MK_GATHER_MUL = 2, MK_SOFTMAX = 3,
                      // the v_other and v_orig * v_other segments as ONE pass over the v_k rows against per-triplet effective
                      // weights W_k + diag(v_o[b]) W_m (the forward twin of the weight gradient's per-triplet fold); first
                      // segment only, K == 24, 48 x 64 tiles
                      MK_VFOLD = 4 };
constexpr int MAIN_MAX_SEG = 5;
struct MainSeg {
    const float* a;      // operand rows: x(r, c) = a[row(r) * lda + c], row(r) = r or idx[r]
    const int*   idx;    // MK_GATHER / MK_GATHER_MUL: table row of logical row r
    const int*   idx2;   // MK_GATHER_MUL: x(r, c) = a[idx[r]][c] * a[idx2[r]][c]        (v_other * v_orig, cx.py:296)
    const float* lse;    // MK_SOFTMAX: x(r, c) = exp2(a[r][c] * log2(e) - lse[r])        (softmax(a_knns), cx.py:281)
    const float* b;      // weight slice: w(n, c) = b[n * ldb + c]
    const float* b2;     // MK_VFOLD: the second weight slice (linear_1.weight[:, v_mult]), same ldb
    long long lda, ldb;
    int kind, klen;      // klen: reduction extent (columns of the segment), >= 4
};
struct MainArgs {
    MainSeg seg[MAIN_MAX_SEG]; int nseg, M, N, split; float* out; long long ldo; EpiArgs epi;
    float* slab;                     // split > 1: [split][M][N] partial sums
    // dist_out != NULL (sequence G, X, P, ...; split == 1; v rows a multiple of 32 wide): the pairwise distance
    // ||v_o - v_k + 1e-6|| (cx.py:300) is accumulated while the v_o * v_k segment streams both rows, patched into column 0 of
    // the following (dist | rank) segment's first tile and stored to dist_out[r * ld_dist] for the backward pass -- k_prep then
    // does not have to read the 200 MB of feature rows a second time
    float* dist_out; long long ld_dist;
    unsigned long long* stamps;      // diagnostics (tools/mb/mb_main.hip): 16 words per workgroup of s_memtime / s_memrealtime stamps; NULL in the library
    int x6;                          // NCX_F_X6: the plain / softmax segments of the 192 x 64 fold form on the bf16 matrix path with three-plane operands
    float* t_out; float* t_out0;     // main_forward_mlb only (nullable): t = tanh(z) of the rows that go to out / epi.out0, leading dimension N
    AdamFuse adam;                   // main_forward_adam only: the optimiser's buffers (last: the other forms' arguments keep their offsets)
};
int main_forward(MainArgs& a, hipStream_t s);
// The chain over permuted rows (EPI_ROWMAP of ncx_main.h): two MK_GATHER segments sharing one table idx[0 .. M]; tile row r reads operand rows
// idx[r] and writes output row idx[r]; row tiles from idx[M] on stop after the first segment.  Same tile form per shape as main_forward.
int main_forward_rowmap(MainArgs& a, hipStream_t s);
// a chain of T k-steps over an M x N output takes the 64 x 64 form with three workgroups per CU
bool main_short_form(long long M, long long N, long long T, int split);
// the tile form main_forward / main_forward_rowmap launch a chain without the fold on, hooks applied (codes of NCX_QUERY_FWD_ROUTE)
int main_chain_form(long long M, long long N, long long T, int split, bool single_gather, bool wide_ok);
// The answer-embedding gradient (two segments, plain or -- rowmap -- over permuted rows) on that form with Adam applied by the same launch
// (a.adam; WithAdam of ncx_main.h).  NCX_E_FLAGS when the shape does not take the 64 x 64 form: callers ask main_short_form first.
int main_forward_adam(MainArgs& a, bool rowmap, hipStream_t s);
int main_adam_passengers();          // passenger workgroups of that launch
// Gt and Sh, the two short products in front of linear_1, as ONE launch of that 64 x 64 form plus one fix-up (the PAIR form of k_main_fwd, ncx_main.h).
// Both argument sets are {G, P, P, G} chains with split and slab set: Sh fills all four segments, Gt the plain segment 1 with the others at
// zero length.  Raw partial tiles go to each set's slab[z][M][N]; the fix-up sums them z ascending and applies each set's epilogue (bias only).
// reps: consecutive chunks one workgroup runs (a divisor of the set's split): the chunks, and with them the bits of the sums, stay those of
// `split` workgroups per tile -- the generic engine's for the same split -- while split / reps workgroups per tile share the round.
int main_forward_pair(const MainArgs& gt, const MainArgs& sh, int reps_gt, int reps_sh, hipStream_t s);
// The MLB producer's x_v product (ncx_mlb.hip): one MK_GATHER segment with the EPI_MLB epilogue of ncx_main.h
int main_forward_mlb(MainArgs& a, hipStream_t s);
int main_mlb_form(long long M, long long N);       // ... its tile form, as a code of NCX_QUERY_FWD_ROUTE: 2 (96 x 128) or 0 (48 x 128)
// k-split of a problem for the fused forward kernel (48 x 128 tiles): 1 when its tiles already give every CU a workgroup,
// else as many k-chunks as keep all workgroups resident at once (two per CU), at least 8 k-steps each.  T: k-steps of the whole chain.
int main_split(long long M, long long N, long long T);
int main_fold_rows_eff(long long M, long long N, int rowdiv);   // ... the form main_forward takes (hooks, K = 48 rule)
int main_fold_rows(long long M, long long N);      // tile rows of the per-triplet fold: 192 (one 8-wave workgroup per CU), 96 (four triplets per workgroup) or 48

// ncx_dwkm.hip: d linear_1.weight[:, v_other] and [:, v_mult] in one MFMA pass with a per-triplet fold
constexpr int DW_KM_SPLIT = 8;
bool dw_km_supported(const ncx_dims& d);
// which kernel dw_km launches for the shape (the codes of NCX_QUERY_DW1_ROUTE, include/neuralcx.h)
enum DwKmForm : int { KM_FORM_NONE = 0, KM_FORM_8 = 1, KM_FORM_X6 = 2, KM_FORM_GENERIC = 3, KM_FORM_GROUPED = 4 };
int dw_km_form(const ncx_dims& d);
size_t dw_km_slab_bytes(const ncx_dims& d);
int dw_km(const ncx_dims& d, const float* dpre, const float* feats, const int* idx_k, const int* idx_o, float* slab,
          float* g_vother, float* g_vmult, long long din, hipStream_t s, bool finish = true);
int dw_km_finish(const ncx_dims& d, const float* slab, float* g_vother, float* g_vmult, long long din, const FixupArgs* fix, int fix_cfg,
                 hipStream_t s);
// ncx_dwtn.hip: every other row-reduction product of linear_1's weight gradient (dGt, z_other, dist | rank, the per-triplet shared
// segments) as one balanced launch of 8-wave workgroups on 256 x 64 tiles
constexpr int TN8_MAX_PROB = 8;
constexpr int TN8_MAX_SEG = 16;             // pieces per workgroup (the LDS table of k_dw_tn8 / k_dw_tn8_x6; host-checked)
struct Tn8Prob {             // out[h][n] = sum_r A[r][h] * x(r, n)
    const float* A;          // [rows][H]: dpre (rows = B K) or dSh (rows = B)
    const float* X; long long ldx;   // operand rows, x(r, n) = X[row(r) * ldx + n]
    const float* lse;        // non-NULL: x = exp2(X log2e - lse[r])   (softmax(a_knns), cx.py:281)
    int gsel;                // row(r): 0 = r; 1 = idx_ob[r] (feature-table row of triplet r's original image); 2 = answer_aids[r]   (rows == B)
    int rows, N;             // rows % 32 == 0; N % 4 == 0 (columns the operand rows hold)
    float* out; long long ldo; int n_valid;      // columns written: n < n_valid <= N
    int rows_valid;          // 0: = rows.  Else operand rows >= rows_valid do not exist (their index is clamped) and A's rows there are ZERO
    float* outT; float* outT2; long long ldT; int padT2;   // optional transposed copies out^T[n][h] (ld ldT); outT2 also gets padT2 zero rows after n_valid
};
bool dw_tn8_supported(const ncx_dims& d);          // the fp32 launch (dGt + rest, then dW1[:, a_other]): shapes and plans fit
bool dw_tn8_shapes_ok(const ncx_dims& d);          // ... the shape rules alone, ignoring the bf16 flag and the plans
bool dw_tn8_shared_ok(const ncx_dims& d);          // the per-triplet shared segments take the kernel (bf16 variant: on their own launch)
// The problem lists backward_impl hands to the kernel, shapes only (rows, N): TN8_LIST_MAIN the fp32 launch (dGt aligned + 6 rest problems,
// or 7 rest problems under the a_emb lesion), TN8_LIST_SHARED the bf16 variant's 4 shared segments, TN8_LIST_AK dW1[:, a_other].
enum Tn8List : int { TN8_LIST_MAIN = 0, TN8_LIST_SHARED = 1, TN8_LIST_AK = 2 };
// pieces per workgroup of that list's plan (the kernel's LDS table holds TN8_MAX_SEG) and its grid; 0 when dw_tn8_shapes_ok fails
int dw_tn8_pieces(const ncx_dims& d, int list, int* grid);
bool dw_tn8_x6(const ncx_dims& d);
size_t dw_tn8_slab_bytes(const ncx_dims& d);
// problems [0, n_al) (n_al <= 1): tile-aligned row chunks, one per workgroup; [n_al, np): laid end to end and cut into equal ranges.
// do_al / do_rest: which part this call launches (the chunking of each part does not depend on the other: phased backward)
int dw_tn8(const ncx_dims& d, const Tn8Prob* probs, int np, int n_al, bool do_al, bool do_rest, const int* idx_ob, const int* aid,
           float* slab, size_t slab_bytes, hipStream_t s);
// ncx_mutan.hip: the rank-R fusion of the MUTAN producer as ONE product per question against an effective weight tile built on the fly
bool mutan_fold_supported(const ncx_dims& d, const ncx_mutan_params& m);
int mutan_fold(const ncx_dims& d, const ncx_mutan_params& m, const float* xv, const float* hq, float* z_orig, float* z_knns, hipStream_t s);
// ncx_vqa.hip: dst[r][0 .. cols) = src[r][0 .. cols), dst[r][cols .. ldd) = 0 (weight rows zero-padded to whole 32-column k-steps for ncx_main.h)
__attribute__((visibility("hidden"))) hipError_t pad_rows(const float* src, long long ld_src, int cols, float* dst, int ldd, int rows, hipStream_t s);
WsLayout ws_layout(const ncx_dims& d);
__host__ __device__ static inline int pad_to(int x, int m) { return (x + m - 1) / m * m; }
// The fused forward kernel (ncx_main.h) takes operands whose widths are multiples of 4 (16-byte windows, no straddling);
// other shapes (only the ragged test shapes: every real width is a multiple of 8) run on the generic engine.
// ... and whose extents are below 4 GiB (its loads are buffer loads with 32-bit byte offsets: the feature table, the candidate logits, the activations).
static inline bool main_fwd_extents_ok(const ncx_dims& d) {
    const long long lim = (1ll << 32) - 65536, M = (long long)d.B * d.K, wa = d.A > d.da ? d.A : d.da;
    return (long long)d.n_img * d.dv * 4 < lim && M * wa * 4 < lim && M * (long long)d.H * 4 < lim && M * (long long)d.dz * 4 < lim && (long long)d.A * wa * 4 < lim &&
           (long long)d.H * (2ll * d.dv + d.dq + 2ll * d.dz + 2ll * d.da + d.K + 2) * 4 < lim;
}
static inline bool main_fwd_dims_ok(const ncx_dims& d) {
    return d.dv % 4 == 0 && d.dz % 4 == 0 && ((d.flags & NCX_F_A_EMB) ? d.A : d.da) % 4 == 0 && !(d.flags & NCX_F_BF16) && main_fwd_extents_ok(d);
}
static inline bool hidden_fwd_dims_ok(const ncx_dims& d) { return d.H % 4 == 0 && main_fwd_extents_ok(d); }
// The two products the frozen VQA producers (ncx_vqa.hip, ncx_mlb.hip) put on the fused forward kernel, by the width rules above and by
// what that kernel addresses with 32-bit byte offsets (ncx_main.h, setup / issue: operand row x lda x 4 + the column window, weight row x
// ldb x 4 + the k-step's offset; bias, x_q and every store take 64-bit addresses):
//   v: x_v = feats[img_idx] . Wv^T   operand: the feature table [n_img][dv] (whole 32-column rows, at least two k-steps), weights [n_xv][dv]
//   c: a = z_knns . Wc^T             operand: [B K][dz], weights [A][dz rounded up to 32] (whole 16-byte pieces on both sides)
// Anything else runs on the generic engine, whose loaders take 64-bit addresses (OpLoader, ncx_gemm.h).  n_xv: rows of Wv.
struct ProducerMainRoutes { bool v, c; };
static inline ProducerMainRoutes producer_main_routes(const ncx_dims& d, int n_xv) {
    const long long lim = (1ll << 32) - 65536, Mk = (long long)d.B * d.K;
    const bool on = !hook_env("NCX_VQA_NO_MAIN");
    ProducerMainRoutes r;
    r.v = on && d.dv % 32 == 0 && d.dv >= 64 && (long long)d.n_img * d.dv * 4 < lim && (long long)n_xv * d.dv * 4 < lim;
    r.c = on && d.dz % 4 == 0 && d.A % 4 == 0 && Mk * d.dz * 4 < lim && (long long)d.A * pad_to(d.dz, 32) * 4 < lim;
    return r;
}
// private flag bit (never set by callers: check_dims rejects it): the pairwise distance is computed inside the fused forward
// kernel, k_prep leaves the feature rows alone
constexpr uint32_t NCX_F_PRIV_DIST_IN_MAIN = 1u << 30;


}  // namespace ncx
