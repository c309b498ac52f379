/*
 * neuralcx.h -- C ABI of libneuralcx_hip.so: the NeuralCX hot path on MI355X (gfx950).
 *
 * Drop-in boundary for gabegrand/VQA-Counterexamples.  Every entry point names the reference
 * code it replaces (paths relative to the reference root).  The reference is pure Python on
 * PyTorch, so "what its FFI would bind" is the body of vqa.models.cx.NeuralModel.forward and the
 * loss / optimiser calls of the training loop in counterexamples.py; the ctypes binding a
 * maintainer adds is shown in INTEGRATION.md and shipped in
 * vqa-counterexamples_amd/neuralcx/_lib.py.
 *
 * Conventions
 *   - plain C: raw DEVICE pointers + sizes + a HIP stream (hipStream_t passed as void*); no
 *     torch types, no exceptions, no allocation inside, no global state on the product path (the
 *     only process-level state is the OPT-IN diagnostics at the end of this file -- ncx_profile_begin /
 *     _end and ncx_profile_stamps, the latter keyed by device -- and the lazily created per-device
 *     side stream, off unless NCX_SIDE_STREAM is set).  The caller owns every
 *     buffer (PyTorch's caching allocator in the shipped binding) and must keep them alive until
 *     the enqueued work has completed.
 *   - all floating point data is fp32, contiguous row-major; indices are int32.
 *   - weights use torch's nn.Linear layout [out, in]; linear_1.weight keeps the reference's
 *     concat column order (vqa/models/cx.py:309-320) so checkpoints are interchangeable.
 *   - return value: NCX_OK (0), a negative NCX_E_* for invalid arguments (nothing was enqueued),
 *     or a positive hipError_t passed through.
 *   - everything is enqueued on `stream`; nothing synchronises the host.
 *   - results are deterministic run to run (no floating point atomics anywhere).
 */
#ifndef NEURALCX_H
#define NEURALCX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define NCX_OK            0
#define NCX_E_NULL       -1   /* required pointer is NULL */
#define NCX_E_DIMS       -2   /* a dimension is out of the supported range */
#define NCX_E_WORKSPACE  -3   /* workspace too small / misaligned */
#define NCX_E_FLAGS      -4   /* inconsistent flags / lesion inputs */
#define NCX_E_UNSUPPORTED -5  /* the RCCL library could not be loaded (ncx_comm_* / ncx_allreduce only) */
#define NCX_E_COMM       -6   /* RCCL reported an error */

/* model_spec switches of the reference (vqa/models/cx.py:265-307), 1 = feature present */
#define NCX_F_V_MULT   (1u << 0)   /* v_orig * v_other segment (cx.py:295-298), else zeros          */
#define NCX_F_V_DIST   (1u << 1)   /* pairwise_distance column (cx.py:299-302), else zero           */
#define NCX_F_V_RANK   (1u << 2)   /* one-hot candidate rank (cx.py:303-305), else inputs->v_rank   */
#define NCX_F_A_EMB    (1u << 3)   /* answer embeddings (cx.py:279-282), else noise blocks          */
#define NCX_F_ALL      (NCX_F_V_MULT | NCX_F_V_DIST | NCX_F_V_RANK | NCX_F_A_EMB)
/* BASELINE configs[4] ("bf16 weights"; net-new, the reference is fp32 only): the two dominant GEMMs -- candidate
 * segments of linear_1 forward, and their weight gradient -- and the three answer-embedding products (Gt forward,
 * d linear_1.weight[:, a_emb_other] and d answer_embedding backward) take bf16 operands (round-to-nearest-even
 * copies of the fp32 master weights, inputs and gradients) with fp32 accumulation on the bf16 MFMA path; everything
 * else, including Adam on the fp32 master weights, is unchanged.  Needs NCX_F_ALL (no lesions). */
#define NCX_F_BF16     (1u << 4)
/* Evaluation loops (eval_model, counterexamples.py:450-490): Gt = W1[:, a_emb_other] . E^T depends on the weights only.
 * With this bit ncx_forward trusts the Gt left in the workspace by an earlier ncx_forward on the SAME workspace and
 * weights and skips that GEMM.  The caller owns the invariant (the engine sets it from the second batch of an
 * evaluation pass on). */
#define NCX_F_REUSE_GT (1u << 5)
/* Training steps (counterexamples.py:330-339: forward, criterion, backward back to back): with this bit the out layer
 * (cx.py:327), the loss / Recall pass and the head of the backward run as ONE pass over the last hidden activations in
 * ncx_train_tail -- ncx_forward then leaves `scores` alone (it may be NULL) and ncx_backward[_phase] expects ncx_train_tail to
 * have run on the same workspace (its `dscores` may be NULL).  K <= 32 and H <= 256 only (ncx_train_tail says NCX_E_DIMS
 * otherwise: clear the bit and use the three calls). */
#define NCX_F_FUSED_TAIL (1u << 6)
/* "bf16 x 6": fp32-grade arithmetic on the bf16 matrix path.  NOT the default -- the headline path is fp32 MFMA, and this bit is never set unless the
 * caller sets it.  With it, the three big products of the training step take their fp32 operands as THREE bf16 planes each (x = x1 + x2 + x3
 * EXACTLY: x1 = x & 0xFFFF0000, x2 = (x - x1) & 0xFFFF0000, x3 = x - x1 - x2, cut when a tile is stored to LDS) and run the six plane products
 * that matter (a1 x1 + a1 x2 + a2 x1 + a1 x3 + a2 x2 + a3 x1) on v_mfma_f32_16x16x32_bf16 with fp32 accumulation; products of bf16 values are
 * exact in fp32, so what is dropped is 2^-24 relative: the rounding error of ONE fp32 operation (unlike the two-plane "bf16 x 3" form, whose
 * 2^-16 error fails the suite's ReLU-kink conditioning: DESIGN 5d).  Covered:
 *   - linear_1 forward on the 192-row form at K = 24 (per-triplet fold: the effective weight is formed in fp32, b = fma(v_o, W_m, W_k), then cut),
 *   - d linear_1.weight[:, v_other | v_orig*v_other] (the per-triplet fold pass, H % 256 == 0 and dv % 64 == 0),
 *   - dGt and every other column block of d linear_1.weight (the balanced TN launch, B <= 2048),
 *   - the conv_v_att product of the MLB attention model (ncx_mlb_att_forward_flags, ncx_mlb_att_train_forward_flags: P >= 4, any dv, dh_att, G).
 *   - d conv_v_att.weight of the MLB attention model's training step (ncx_mlb_att_train_backward_flags: P >= 4, any dv, dh_att, G, B).
 *   - the GRU question encoder's step product [x_t | h_{t-1}] . [W_ih | W_hh]^T (ncx_gru_encode_flags, ncx_gru_train_forward_flags: every legal
 *     shape, no fall-back; these two take the bit from their own `flags` argument only).
 *   - the 2-lstm question encoder's step product [x_t | h_{t-1}] . [W_ih | W_hh]^T of both layers (ncx_lstm2_encode_flags,
 *     ncx_lstm2_train_forward_flags: every legal shape, no fall-back; the bit comes from their own `flags` argument only).
 * Shapes outside fall back to the fp32 kernels silently (same results to rounding).  Results agree with the fp32 kernels to fp32 rounding, not
 * bitwise (another summation order); every parity test of the suite passes at its unchanged tolerance with the bit set (NCX_X6=1 in the
 * environment of the Python binding sets it for a whole process). */
#define NCX_F_X6       (1u << 7)
/* (v_emb / q_emb / z_emb lesions replace INPUTS by uniform noise: the host does that before the call) */

typedef struct ncx_dims {
    int32_t B;        /* triplets in this (local) batch                                             */
    int32_t K;        /* candidates per triplet, knn_size (24 in the reference; 3..64 supported)     */
    int32_t dv;       /* dim_v  image feature width (2048)                                          */
    int32_t dq;       /* dim_q  question embedding width (2400)                                     */
    int32_t dz;       /* dim_mm multimodal fusion width (360)                                       */
    int32_t da;       /* dim_a  answer embedding width (2400, cx.py:235)                            */
    int32_t A;        /* ans_size, rows of answer_embedding (2000)                                  */
    int32_t H;        /* dim_h                                                                      */
    int32_t L;        /* n_layers, 1..3                                                             */
    int32_t n_img;    /* rows of the image feature table                                            */
    uint32_t flags;   /* NCX_F_*                                                                    */
    int32_t training; /* 1: apply dropout (cx.py:322-326), 0: eval                                  */
    float   drop_p;   /* nn.Dropout p (cx.py:259)                                                   */
    float   loss_scale; /* multiplies dscores/loss: 1/B_global (counterexamples.py:334); 0 => 1/B   */
    uint64_t seed;    /* per-step dropout seed (counter-based generator, see oracle/ncx_oracle.py)  */
} ncx_dims;

/* Inputs of NeuralModel.forward after vqa_forward (cx.py:261-285); all DEVICE pointers.
 * The reference gathers image_features[B,K+1,dv] on the host (counterexamples.py:540-541); here the
 * gather is folded into the kernels: `feats` is the resident table and img_idx the rows.  A caller
 * holding an already gathered [B,K+1,dv] block passes it as feats with img_idx = 0..B*(K+1)-1. */
typedef struct ncx_inputs {
    const float*   feats;        /* [n_img, dv]                                                    */
    const int32_t* img_idx;      /* [B, K+1]  column 0 = original image, 1..K = the K candidates   */
    const float*   q_emb;        /* [B, dq]                                                        */
    const float*   z_orig;       /* [B, dz]                                                        */
    const float*   z_knns;       /* [B, K, dz]                                                     */
    const float*   a_knns;       /* NCX_F_A_EMB: [B, K, A] answer LOGITS; else [B, K, da] noise    */
    const int32_t* answer_aids;  /* [B]   (NCX_F_A_EMB)                                            */
    const float*   a_emb_gt;     /* [B, da] noise block, only without NCX_F_A_EMB                  */
    const float*   v_rank;       /* [B, K, K] noise block, only without NCX_F_V_RANK               */
    const float*   keep_mask;    /* optional explicit dropout keep masks [L][B*K][H] (0/1 floats);
                                    NULL => counter-based generator keyed by dims->seed            */
} ncx_inputs;

/* Trainable tensors, state_dict names of the reference (cx.py:240-257). */
typedef struct ncx_params {
    const float* answer_embedding;  /* [A, da]                                   */
    const float* w1;  const float* b1;   /* linear_1.weight [H, Din], .bias [H]  */
    const float* w2;  const float* b2;   /* linear_2 [H,H],[H]   (L >= 2)        */
    const float* w3;  const float* b3;   /* linear_3 [H,H],[H]   (L >= 3)        */
    const float* w_out; const float* b_out; /* out.weight [1,H], out.bias [1]    */
} ncx_params;

typedef struct ncx_grads {          /* same shapes; OVERWRITTEN (not accumulated) by ncx_backward */
    float* answer_embedding;
    float* w1;  float* b1;
    float* w2;  float* b2;
    float* w3;  float* b3;
    float* w_out; float* b_out;
} ncx_grads;

/* Din = 3*dv + 2*da + 2*dz + dq + K + 1   (cx.py:245-251) */
int64_t ncx_input_size(const ncx_dims* d);

/* Bytes of scratch + saved activations ncx_forward/ncx_backward need for `d` (256-byte aligned base
 * required).  The same buffer must be passed to the ncx_backward that follows an ncx_forward. */
size_t ncx_workspace_bytes(const ncx_dims* d);

/* Replaces NeuralModel.forward (vqa/models/cx.py:261-333) from the answer-embedding lookups down:
 * K3/K4 softmax(a_knns) x answer_embedding and embedding(answer_aids) (cx.py:280-282), the per
 * candidate feature synthesis (cx.py:295-307), the concat (cx.py:309-320, never materialised),
 * linear_1..3 + ReLU + Dropout (cx.py:322-326) and `out` (cx.py:327).  scores: [B, K]. */
int ncx_forward(const ncx_dims* d, const ncx_inputs* in, const ncx_params* p,
                void* workspace, size_t workspace_bytes, float* scores, void* stream);

/* The same forward cut where the data ends and the weights begin (net-new; the reference is single-GPU: the cut exists for
 * the data-parallel step, counterexamples.py:334-339 being where a DP job sums gradients):
 *   NCX_FWD_PRELUDE  everything that is a function of the batch alone -- the feature-table row ids of every candidate row,
 *                    the pairwise distance (cx.py:300), the rank one-hot (cx.py:304-305), the softmax statistics of the
 *                    answer logits (cx.py:281); in the bf16 variant also the packed candidate rows.  Reads no weight
 *                    (`p` is validated like in ncx_forward but not dereferenced on the device; `scores` may be NULL).
 *   NCX_FWD_REST     everything that reads the weights (padded weight copies, Gt, Sh, linear_1..3, out).
 * PRELUDE then REST == ncx_forward bit for bit, on the same workspace.  A DP job enqueues step n + 1's PRELUDE before it waits
 * for step n's last gradient bucket and applies that bucket's Adam slice: the exchange hides under it. */
#define NCX_FWD_ALL     0
#define NCX_FWD_PRELUDE 1
#define NCX_FWD_REST    2
int ncx_forward_phase(const ncx_dims* d, const ncx_inputs* in, const ncx_params* p,
                      void* workspace, size_t workspace_bytes, float* scores, int32_t phase, void* stream);

/* Replaces nn.CrossEntropyLoss(size_average=False)(scores, comp_idxs) / len(batch)
 * (counterexamples.py:310,334) and recallAtK (counterexamples.py:501-506) in one pass.
 *   loss_rows[B]  per-triplet CE * scale          (nullable)
 *   loss[1]       sum of loss_rows                (nullable)
 *   dscores[B,K]  (softmax - onehot) * scale      (nullable)   == d loss / d scores
 *   rank[B]       #{k: s_k > s_gt} + #{k < gt: s_k == s_gt}    (nullable)
 *   hits[2]       OVERWRITTEN with #{rank < 1}, #{rank < 5}    (nullable)
 * scale = 1/B when scale <= 0.   K <= 64.
 * Precondition: every gt[b] lies in [0, K); the kernel does not check it (unlike ncx_ce_loss's targets). */
int ncx_loss_rank(const float* scores, const int32_t* gt, int32_t B, int32_t K, float scale,
                  float* loss_rows, float* loss, float* dscores, int32_t* rank, int32_t* hits,
                  void* stream);

/* Replaces loss.backward() (counterexamples.py:338) for the tensors of ncx_params: given
 * dscores[B,K] = d loss / d scores, writes every gradient.  vqa_model is frozen in the reference
 * (cx.py:73-80), so no input gradients are produced. */
int ncx_backward(const ncx_dims* d, const ncx_inputs* in, const ncx_params* p,
                 void* workspace, size_t workspace_bytes, const float* dscores,
                 const ncx_grads* g, void* stream);

/* ncx_backward in halves, for overlapping the gradient exchange of a data-parallel job with compute
 * (net-new: the reference is single-GPU).  Two ways to cut it, each bit-identical to ncx_backward (phase 0) when
 * both halves run in order on the same stream and workspace:
 *   phase 1 | 2:  1 = out.*, linear_2/3.*, linear_1.bias and the complete answer_embedding gradient;
 *                 2 = linear_1.weight.
 *   phase 3 | 4:  3 = everything except the answer_embedding gradient; it leaves the block dGt | dGgt (the gradient
 *                 w.r.t. W1[:, a_emb_other] . E^T and the scattered dSh; layout: see NCX_WS_DGT below) in the workspace
 *                 region ncx_ws_region(NCX_WS_DGT);  4 = answer_embedding gradient = dGt^T . W1ak + dGgt^T . W1agt.
 *                 The embedding gradient is linear in that region, so a DP job sums the 4 MB region over ranks
 *                 between 3 and 4 instead of all-reducing the 19 MB [A, da] gradient (every rank then computes the
 *                 same, complete gradient).
 *   phase 5 | 2 | 4:  5 = phase 1 without the answer_embedding product: out.*, linear_2/3.*, linear_1.bias, and the
 *                 region dGt | dGgt complete (as after phase 3) -- a DP job starts summing the region here, runs
 *                 phase 2 (linear_1.weight: most of the backward) under that exchange, starts the exchange of the
 *                 remaining gradients, and runs phase 4 under it. */
int ncx_backward_phase(const ncx_dims* d, const ncx_inputs* in, const ncx_params* p,
                       void* workspace, size_t workspace_bytes, const float* dscores,
                       const ncx_grads* g, int32_t phase, void* stream);

/* Byte offset (from the 256-byte aligned workspace base) and size of a named workspace region.
 * NCX_WS_DGT: the block the answer_embedding gradient is linear in, in the form the library's own phases produce and
 * consume it -- fp32 path: dGt^T | dGgt^T, 2 x [A][pad4(H)] fp32 (reduction index contiguous: the embedding gradient runs
 * in NT form; 4.1 MB at A = 2000, H = 256); bf16 variant: dGt | dGgt, 2 x [H][A] fp32.  A DP job sums exactly
 * [offset, offset + bytes) over ranks between phase 5 (or 3) and phase 4; size 0 when the a_emb segment is lesioned. */
#define NCX_WS_DGT 1
#define NCX_WS_H1 2     /* diagnostics / tests: post-dropout activations of linear_1, [B*K, H] (valid after ncx_forward) */
#define NCX_WS_DPRE1 3  /* diagnostics / tests: gradient of linear_1's pre-activations, [B*K, H] (valid after ncx_backward) */
/* diagnostics / tests: int32 [A + 1], valid after ncx_backward (and phase 1) on the fp32 path: the answer ids that occur in the batch's
 * answer_aids ascending, then the others ascending, and in [A] how many occur -- the row order of the answer_embedding gradient's product,
 * whose row tiles without an answer of the batch skip the dGgt^T operand (all zeros there).  Size 0 where the product keeps the full form. */
#define NCX_WS_DE_PERM 4
#define NCX_WS_H2 5     /* diagnostics / tests: post-dropout activations of linear_2, [B*K, H] (valid after ncx_forward; size 0 when L < 2) */
#define NCX_WS_H3 6     /* ... of linear_3 (size 0 when L < 3) */
/* diagnostics / tests: gradient of linear_2's pre-activations, [B*K, H], valid after ncx_backward when L == 2: the backward's two
 * ping-pong buffers then hold dpre_2 and dpre_1 (NCX_WS_DPRE1) side by side.  Size 0 for every other L (L == 1 has no such layer; the
 * region is kept to the one depth whose hidden-layer products the tests judge alone). */
#define NCX_WS_DPRE2 7
/* diagnostics / tests, NCX_F_BF16 only (size 0 without the flag): the packed bf16 operands of linear_1's candidate product, as raw uint16
 * bit patterns in the column layout ncx_bf16_layout reports.  NCX_WS_XC: the candidate rows, [B*K][kc], valid after ncx_forward or its
 * PRELUDE phase.  NCX_WS_WC: the weights [W1 column slices | Gt], [Hp][kc], valid after ncx_forward. */
#define NCX_WS_XC 8
#define NCX_WS_WC 9
/* diagnostics / tests: the fp32 Gt = W1[:, a_emb_other] . E^T the last ncx_forward produced, [H][ld] with the leading dimension
 * ld = A under NCX_F_BF16 and A rounded up to a multiple of 32 otherwise (bytes = H * ld * 4 tells which). */
#define NCX_WS_GT 10
int ncx_ws_region(const ncx_dims* d, int32_t which, size_t* offset, size_t* bytes);

/* NCX_F_FUSED_TAIL: replaces, in one pass over h_L, the tail of ncx_forward (`out`, cx.py:327), ncx_loss_rank
 * (counterexamples.py:310,334,501-506) and the head of ncx_backward (d out.weight, d out.bias, the gradient of the last
 * pre-activations; for L == 1 also d linear_1.bias).  Call order: ncx_forward, ncx_train_tail, ncx_backward[_phase], all with the
 * same dims (flag set) and workspace.  Outputs as ncx_loss_rank (scale = dims.loss_scale, 1/B when <= 0) plus `scores`
 * [B, K]; dscores is optional.  Bit-identical to the three separate calls except d out.bias (zero in maths; its partial sums
 * are taken in another order).  Precondition, as for ncx_loss_rank: every gt[b] lies in [0, K); it is not checked. */
int ncx_train_tail(const ncx_dims* d, const ncx_params* p, void* workspace, size_t workspace_bytes, const int32_t* gt,
                   float* scores, float* loss_rows, float* loss, float* dscores, int32_t* rank, int32_t* hits,
                   const ncx_grads* g, void* stream);

/* Gradient exchange of a data-parallel job (net-new: the reference is single-GPU; /root/reference/counterexamples.py:334-339
 * is where a DP job sums gradients between loss.backward() and optimizer.step()).  An opaque handle around one RCCL
 * communicator -- the library's only other state; RCCL is loaded on first use (NCX_E_UNSUPPORTED when it is absent).
 *   rank 0:      ncx_comm_unique_id(id)          -> 128 bytes the host hands to every rank (file, socket, MPI ...)
 *   every rank:  hipSetDevice(local GPU); ncx_comm_create(id, nranks, rank, &comm)
 *   per step:    ncx_allreduce(comm, buf, n, stream)   in-place fp32 SUM over ranks, ordered on `stream`
 *                (the engine's two buckets: the dGt | dGgt workspace region and the flat gradient tail)
 * The Python host uses torch.distributed's RCCL backend for the same collective. */
#define NCX_COMM_ID_BYTES 128
typedef struct ncx_comm ncx_comm;
int ncx_comm_unique_id(void* id128);
int ncx_comm_create(const void* id128, int32_t nranks, int32_t rank, ncx_comm** out);
int ncx_comm_destroy(ncx_comm* comm);
int ncx_allreduce(ncx_comm* comm, float* buf, size_t n, void* stream);

/* Replaces torch.optim.Adam(...).step() (counterexamples.py:275-276,339) on a flat fp32 buffer:
 * defaults betas (0.9, 0.999), eps 1e-8, no weight decay, no amsgrad.  `step` is the 1-based step
 * count; grad_scale multiplies g first (1/world_size after a sum all-reduce). */
int ncx_adam_step(float* param, const float* grad, float* exp_avg, float* exp_avg_sq, size_t n,
                  float lr, float beta1, float beta2, float eps, int32_t step, float grad_scale,
                  void* stream);

/* ncx_backward followed by ncx_adam_step over the model's flat parameter buffer, as one call (single-GPU training: nothing sums
 * gradients between the two).  `opt` describes the flat buffers: param / grad / exp_avg / exp_avg_sq of n floats each, 16-byte
 * aligned, answer_embedding first (n_emb = its A * da elements plus any padding behind it; the other tensors of ncx_params /
 * ncx_grads lie in [n_emb, n) of param / grad), the 1-based step and Adam's constants as in ncx_adam_step.
 * Where the answer_embedding gradient is the fp32 NT product on 64 x 64 tiles (the full model at training shapes), the launch that
 * produces it also applies Adam -- each tile updates the elements it has just produced, further workgroups of the same launch update
 * the rest of the buffer -- and no separate pass over the buffer runs.  Everywhere else (bf16 variant, a_emb lesion, small shapes,
 * padding behind the embedding, the internal side stream) the call runs ncx_backward then the ncx_adam_step kernel.  Gradients,
 * parameters and moments are bit-identical to the two separate calls either way.
 * NCX_E_NULL: a NULL argument or buffer.  NCX_E_DIMS: step < 1, n == 0, n_emb > n or < A * da, params->answer_embedding != param,
 * grads->answer_embedding != grad, or a tensor outside its flat buffer.  NCX_E_WORKSPACE: a misaligned buffer.  Nothing is enqueued then. */
typedef struct ncx_adam_state {
    float* param; const float* grad; float* exp_avg; float* exp_avg_sq;
    size_t n, n_emb;
    int32_t step;
    float lr, beta1, beta2, eps, grad_scale;
} ncx_adam_state;
int ncx_backward_adam(const ncx_dims* d, const ncx_inputs* in, const ncx_params* p,
                      void* workspace, size_t workspace_bytes, const float* dscores,
                      const ncx_grads* g, const ncx_adam_state* opt, void* stream);

/* ---- the frozen VQA producer upstream of NeuralCX -----------------------------------------
 * Replaces CXModelBase.vqa_forward (vqa/models/cx.py:64-104) for the MutanNoAtt model in eval mode:
 * MutanFusion.forward (vqa/models/fusion.py:78-121: linear_v/linear_q + activation, R x {linear_hv_i, linear_hq_i,
 * hadamard}, sum) and AbstractNoAtt._classif (vqa/models/noatt.py:24-29) on the original + K candidate images.
 * The question branch is evaluated once per question (the reference duplicates q K+1 times first, cx.py:83-87), the
 * image gather is folded into linear_v, and the R rank-1 terms are folded inside ONE chained GEMM.  q_emb comes
 * from the question encoder (seq2vec), which stays on the PyTorch side. */
typedef struct ncx_mutan_params {
    const float* wv;  const float* bv;    /* fusion.linear_v.weight [dhv, dv], .bias [dhv]                       */
    const float* wq;  const float* bq;    /* fusion.linear_q.weight [dhq, dq], .bias [dhq]                       */
    const float* whv; const float* bhv;   /* fusion.list_linear_hv.{0..R-1} stacked: [R*dz, dhv], [R*dz]         */
    const float* whq; const float* bhq;   /* fusion.list_linear_hq.{0..R-1} stacked: [R*dz, dhq], [R*dz]         */
    const float* wc;  const float* bc;    /* linear_classif.weight [A, dz], .bias [A]                            */
    int32_t dhv, dhq, R;                  /* R <= 10                                                             */
    int32_t act_v, act_q;                 /* activation_v / activation_q: 0 none, 2 tanh                         */
} ncx_mutan_params;

size_t ncx_vqa_workspace_bytes(const ncx_dims* d, const ncx_mutan_params* m);

/* z_orig [B,dz], z_knns [B,K,dz], a_knns [B,K,A] (logits), a_orig [B,A] (nullable: NeuralModel never reads it).
 * Uses d->B, K, dv, dq, dz, A, n_img only. */
int ncx_vqa_forward(const ncx_dims* d, const float* feats, const int32_t* img_idx, const float* q_emb,
                    const ncx_mutan_params* m, void* workspace, size_t workspace_bytes,
                    float* z_orig, float* z_knns, float* a_knns, float* a_orig, void* stream);
/* Diagnostics / tests: what ncx_vqa_forward launches for these dims and parameters, from the function the launcher itself asks
 * (experiment hooks applied).  Host only: launches nothing, needs no device (256 CUs are assumed without one).
 *   out4[0]  x_v:        1 the fused forward kernel (one gathered segment), 0 the generic engine's gather
 *   out4[1]  fusion:     1 k_mutan_fold (one product per question; K + 1 <= 32, dhv % 4 == 0), 0 the generic engine's fold chain of R pairs
 *   out4[2]  classifier: 0 the generic engine, 1 the fused forward kernel on linear_classif.weight in place (dz % 32 == 0),
 *                        2 the fused forward kernel on a copy with rows zero-padded to a multiple of 32
 *   out4[3]  the tile form of the fused x_v launch (the codes of NCX_QUERY_FWD_ROUTE), -1 on the generic engine
 * The fused forward kernel addresses its operands with 32-bit byte offsets: a feature table, weight matrix or z_knns of 4 GiB
 * or more takes the generic engine. */
int ncx_vqa_route(const ncx_dims* d, const ncx_mutan_params* m, int32_t* out4);
/* Diagnostics / tests: byte offset and size of the intermediate tensors ncx_vqa_forward leaves in the workspace. */
#define NCX_VQA_WS_XQ 1   /* x_q = act_q(q Wq^T + bq)                          [B, dhq]        */
#define NCX_VQA_WS_HQ 2   /* hq[b][r dz + j] = x_q[b] . Whq_r[j] + bhq_r[j]    [B, R dz]       */
#define NCX_VQA_WS_XV 3   /* x_v = act_v(feats[img_idx] Wv^T + bv)             [B (K + 1), dhv] */
int ncx_vqa_ws_region(const ncx_dims* d, const ncx_mutan_params* m, int32_t which, size_t* offset, size_t* bytes);

/* ---- the frozen MLB producer: the reference factory's second no-attention model (vqa/models/utils.py:7) ----
 * Replaces CXModelBase.vqa_forward (vqa/models/cx.py:64-104) for the MLBNoAtt model (vqa/models/noatt.py:38-46) in eval mode:
 * MLBFusion.forward (vqa/models/fusion.py:31-50: linear_v / linear_q + activation, hadamard product) and
 * AbstractNoAtt._classif (vqa/models/noatt.py:24-29: optional activation, linear_classif) on the original + K candidate images:
 *   x_q = act_q(q Wq^T + bq) once per question;  x_v = act_v(feats[img_idx] Wv^T + bv);  z = x_q * x_v;  a = act_c(z) Wc^T + bc
 * z_orig / z_knns are z BEFORE the classifier's activation, as the reference returns them (cx.py:94-104).  The image gather
 * is folded into linear_v and x_v is never stored: the product, the row split and act_c(z) happen in that GEMM's epilogue. */
typedef struct ncx_mlb_params {
    const float* wv;  const float* bv;    /* fusion.linear_v.weight [dh, dv], .bias [dh]                         */
    const float* wq;  const float* bq;    /* fusion.linear_q.weight [dh, dq], .bias [dh]                         */
    const float* wc;  const float* bc;    /* linear_classif.weight [A, dh], .bias [A]                            */
    int32_t dh;                           /* fusion.dim_h; must equal d->dz                                      */
    int32_t act_v, act_q, act_c;          /* activation_v / activation_q / classif.activation: 0 none, 2 tanh    */
} ncx_mlb_params;

/* 0 for invalid dims or parameters (as ncx_vqa_workspace_bytes). */
size_t ncx_mlb_workspace_bytes(const ncx_dims* d, const ncx_mlb_params* m);

/* z_orig [B,dh], z_knns [B,K,dh], a_knns [B,K,A] (logits), a_orig [B,A] (nullable: its B rows are multiplied only on request).
 * Uses d->B, K, dv, dq, dz (== m->dh), A, n_img only.  Status codes and workspace rules of ncx_vqa_forward; no allocation. */
int ncx_mlb_forward(const ncx_dims* d, const float* feats, const int32_t* img_idx, const float* q_emb,
                    const ncx_mlb_params* m, void* workspace, size_t workspace_bytes,
                    float* z_orig, float* z_knns, float* a_knns, float* a_orig, void* stream);
/* The sibling of ncx_vqa_route for ncx_mlb_forward (host only, launches nothing):
 *   out4[0]  x_v:        1 the fused forward kernel with the product, row split and tanh in its epilogue, 0 the generic engine + k_mlb_mul
 *   out4[1]  the tile form of that launch: 2 (96 x 128) or 0 (48 x 128), by the CU count; -1 on the generic engine
 *   out4[2]  classifier: 0 generic engine, 1 fused forward kernel on the weights in place, 2 ... on a zero-padded copy (as ncx_vqa_route)
 *   out4[3]  1 when t = act_c(z) is stored beside z (act_c != 0) */
int ncx_mlb_route(const ncx_dims* d, const ncx_mlb_params* m, int32_t* out4);
/* Intermediate tensors of ncx_mlb_forward in the workspace.  NCX_E_FLAGS for a tensor the route does not store: t_* without
 * act_c, x_v on the fused route (there it exists only inside the kernel). */
#define NCX_MLB_WS_XQ 1       /* x_q = act_q(q Wq^T + bq)                      [B, dh]         */
#define NCX_MLB_WS_T_KNNS 2   /* act_c(z_knns)                                 [B K, dh]       */
#define NCX_MLB_WS_T_ORIG 3   /* act_c(z_orig)                                 [B, dh]         */
#define NCX_MLB_WS_XV 4       /* x_v = act_v(feats[img_idx] Wv^T + bv)         [B (K + 1), dh] */
int ncx_mlb_ws_region(const ncx_dims* d, const ncx_mlb_params* m, int32_t which, size_t* offset, size_t* bytes);

/* ---- the MLB attention model (MLBAtt, vqa/models/att.py:11-192) in eval mode, below the question encoder -------------------
 * Every dropout is the identity.  V[b] = feats[img_idx[b]] is the image's NCHW map [dv, P] (P = W H positions, p = w H + h), read
 * in place: never transposed or copied.
 *   x_q[b]        = act_q_att(q[b] Wq_att^T + bq_att)                                                       [B, dh_att]
 *   x_att[b,p,h]  = act_mm(act_v_att(sum_c V[b,c,p] Wv_att[h,c] + bv_att[h]) * x_q[b,h])                    (never stored)
 *   att[b,g,:]    = softmax over p of (sum_h Wa[g,h] x_att[b,p,h] + ba[g])                                  [B, G, P]
 *   v_att[b,g,c]  = sum_p att[b,g,p] V[b,c,p]
 *   x_v[b, g dh_f + n] = act_v(v_att[b,g] Wg[g]^T + bg[g])        x_qf = act_q(q Wqf^T + bqf)               [B, G dh_f]
 *   logits        = act_c(x_v * x_qf) Wc^T + bc                                                             [B, A]
 * The partial position logits of the dh_att tiles go to a slab and are summed in a fixed order (no float atomics): two calls
 * on the same inputs are bit-identical. */
typedef struct ncx_mlb_att_dims {
    int32_t B, P, dv, dq, dh_att, G, dh_f, A, n_img;   /* B, P, n_img >= 1; 1 <= G <= 8; every width >= 4 */
} ncx_mlb_att_dims;
typedef struct ncx_mlb_att_params {
    const float* wv_att; const float* bv_att;   /* conv_v_att.weight [dh_att, dv(,1,1)], .bias [dh_att]                    */
    const float* wq_att; const float* bq_att;   /* linear_q_att.weight [dh_att, dq], .bias [dh_att]                        */
    const float* wa;     const float* ba;       /* conv_att.weight [G, dh_att(,1,1)], .bias [G]                            */
    const float* wg;     const float* bg;       /* list_linear_v_fusion.{g} stacked: [G, dh_f, dv], [G, dh_f]              */
    const float* wqf;    const float* bqf;      /* linear_q_fusion.weight [G dh_f, dq], .bias [G dh_f]                     */
    const float* wc;     const float* bc;       /* linear_classif.weight [A, G dh_f], .bias [A]                            */
    int32_t act_v_att, act_q_att, act_mm;       /* attention.activation_v / _q / _mm: 0 none, 2 tanh                       */
    int32_t act_v, act_q, act_c;                /* fusion.activation_v / _q, classif.activation: 0 none, 2 tanh            */
} ncx_mlb_att_params;

/* 0 for invalid dims or parameters. */
size_t ncx_mlb_att_workspace_bytes(const ncx_mlb_att_dims* d, const ncx_mlb_att_params* m);

/* feats [n_img, dv, P] (the table of NCHW maps); img_idx [B] int32 (an id outside [0, n_img) is clamped); q_emb [B, dq];
 * logits [B, A]; att [B, G, P] (always written).  NULL pointers and dims are rejected before any launch; no allocation; the
 * workspace is 256-byte aligned; every launch is enqueued on `stream`. */
int ncx_mlb_att_forward(const ncx_mlb_att_dims* d, const float* feats, const int32_t* img_idx, const float* q_emb,
                        const ncx_mlb_att_params* m, void* workspace, size_t workspace_bytes,
                        float* logits, float* att, void* stream);
/* ncx_mlb_att_forward (att.py:39-192) with `flags`: 0 (the same call) or NCX_F_X6, which puts the conv_v_att product (att.py:46-57) on
 * the bf16 matrix path with three-plane operands; P < 4 stays fp32.  Any other value is NCX_E_DIMS before any launch.  Same workspace,
 * same slab layout, same fixed summation order over the dh_att tiles; two calls are bit-identical.  Non-finite map or weight values are
 * outside the X6 contract. */
int ncx_mlb_att_forward_flags(const ncx_mlb_att_dims* d, const float* feats, const int32_t* img_idx, const float* q_emb,
                              const ncx_mlb_att_params* m, uint32_t flags, void* workspace, size_t workspace_bytes,
                              float* logits, float* att, void* stream);
/* Host only (no launch, no device access): the kernel the conv_v_att / conv_att stage (att.py:46-57,71-90) takes for these dims under
 * `flags` (0 or NCX_F_X6).  0 k_att_logits_small (P < 4), 1 fp32 64-row tiles, 2 fp32 208-row tiles, 3 X6 64-row, 4 X6 208-row;
 * negative: a status code for dims or flags the forward refuses. */
int ncx_mlb_att_logits_form(const ncx_mlb_att_dims* d, uint32_t flags);

/* ---- brute-force k nearest neighbours of feature rows --------------------------------------
 * Replaces knn.py:41-58 of the reference (sklearn NearestNeighbors(n_neighbors=k).fit(table).kneighbors(queries),
 * brute force, euclidean).  For each of the nq query rows: the k rows of `table` [n, dv] with the smallest
 * euclidean distance, ascending (ties by row index), as out_idx [nq, k] int64 and out_dist [nq, k] fp32.
 * One call handles one block of queries; the workspace holds -|x_j|^2/2 for the table (computed when
 * norms_ready == 0, reusable by later calls with the same table and workspace) and the nq x n product block.
 * 1 <= k <= min(n, 120); dv >= 4.
 * PRECONDITION: every element of table and queries is finite (neuralcx.knn.knn checks it; the C ABI does not).
 * Precision: the k + 8 candidates are chosen on the fp32 products V = q.x_j - |x_j|^2/2 and ranked exactly (fp64), so the
 * exact squared distance of a returned row exceeds the true k-th one by at most
 *   tau = 4 (dv + 2) 2^-24 max_j (sum_t |q_t x_jt| + |x_j|^2 / 2)      (0 where the gaps between neighbours exceed tau).
 * Status: two int32 words at byte ncx_knn_status_offset(n) of the workspace, zeroed by a call with norms_ready == 0 and
 * sticky over the calls that follow it.  Word 0 != 0: some query row kept more distinct products in one bin than the
 * candidate buffer holds after the last refinement level; word 1 != 0: a product was not finite.  Either way that
 * call's output is not to be used; the caller reads the words after its last block (one readback per table). */
size_t ncx_knn_status_offset(int32_t n);
size_t ncx_knn_workspace_bytes(int32_t n, int32_t block_rows);
int ncx_knn(const float* table, int32_t n, const float* queries, int32_t nq, int32_t dv, int32_t k,
            int32_t norms_ready, void* workspace, size_t workspace_bytes, int64_t* out_idx, float* out_dist,
            void* stream);

/* ---- the semantic baseline scorer (reference vqa/models/cx.py:159-210, SemanticBaseline) ---------------------------
 * ncx_cosine_gram replaces cx.py:174-175 (emb_pairs = sklearn cosine_similarity(emb)): gram [A, A] = E^ . E^^T with
 * E^ = emb [A, da] row-normalised in fp64 (a zero row stays zero: its similarities are all 0, the diagonal included), the
 * product on the library's fp32 MFMA engine in column chunks whose partial products are summed in fp64.
 * Workspace: ncx_cosine_gram_workspace_bytes (256-byte aligned; E^ plus an fp64 [A, A] accumulator).
 * 1 <= A <= 8192, 1 <= da, A x pad4(da) <= 2^28. */
size_t ncx_cosine_gram_workspace_bytes(int32_t A, int32_t da);
int ncx_cosine_gram(const float* emb, int32_t A, int32_t da, void* ws, size_t ws_bytes, float* gram, void* stream);
/* ncx_semantic_scores replaces the scorer's double loop (cx.py:182-209) for a batch, in one launch:
 *   p = softmax(a_knns[b, k, :]);  s = lam (gram[aid_b, :] . p - p[aid_b]) - (1 - lam) log(p[aid_b] + 1e-8)
 *   scores [B, K] = softmax over k of s (probabilities, as the reference returns);  raw [B, K] = s (nullable).
 * a_knns [B, K, A] logits; aid [B] int32.  An aid outside [0, A) is never read at: that question's row is NaN and
 * *bad_id_flag is set to 1 (never cleared here; the caller zeroes it).  Both softmaxes subtract the max (the reference's
 * do not: NaN there for a logit above ~88.7).  1 <= K <= 64, 1 <= A <= 4096, B >= 1.  Bit-identical from run to run. */
int ncx_semantic_scores(const float* a_knns, const int32_t* aid, int32_t B, int32_t K, int32_t A, const float* gram,
                        float lam, float* scores, float* raw, int32_t* bad_id_flag, void* stream);

/* ---- the similarity scorer (reference vqa/models/cx.py:490-518, SimilarityModel; no parameters) --------------------------
 * ncx_similarity_scores replaces the scorer's loop over the candidates (cx.py:511-516) for a batch, in one launch:
 *   scores[b, k] = cos(v_orig[b], v_knn[b, k]) + cos(z_orig[b], z_knn[b, k]) + CE(a_knns[b, k, :], aid[b])     (higher = better)
 *   cos(x, y) = x . y / (max(|x|, 1e-8) max(|y|, 1e-8))  -- each norm clamped on its own, as F.cosine_similarity of
 *               torch >= 1.12 does (tests/golden/g13_similarity.npz pins it with a row of norm < 1e-8 against one of norm
 *               100: the older rule max(|x| |y|, 1e-8) gives ten times the value); an all-zero row gives 0
 *   CE(a, aid) = logsumexp(a) - a[aid], the max subtracted first
 * feats [n_img, dv] is the resident feature table and img_idx [B, K + 1] its row ids (column 0 the original image, 1..K
 * the candidates): rows are gathered by id inside the kernel.  z_orig [B, dz], z_knns [B, K, dz], a_knns [B, K, A] logits,
 * aid [B].  scores [B, K]; parts [B, K, 3] = v_cos | z_cos | xent (nullable).  A row id outside [0, n_img) or an answer id
 * outside [0, A) is never read at: that question's row (and its parts) is NaN and *bad_id_flag is set to 1 (never cleared
 * here; the caller zeroes it).  16-byte loads where a base pointer is 16-byte aligned and the row length a multiple of 4,
 * dword loads otherwise.  1 <= K <= 64, 1 <= A <= 4096, dv, dz, n_img, B >= 1.  No atomics: bit-identical from run to run. */
int ncx_similarity_scores(const float* feats, const int32_t* img_idx, int32_t n_img, int32_t dv,
                          const float* z_orig, const float* z_knns, int32_t dz,
                          const float* a_knns, const int32_t* aid, int32_t A,
                          int32_t B, int32_t K,
                          float* scores /*[B,K]*/, float* parts /*[B,K,3] v_cos|z_cos|xent, nullable*/,
                          int32_t* bad_id_flag, void* stream);

/* ---- the question encoder (reference vqa/models/seq2vec.py; GRUEncoder: nn.Embedding -> one-layer nn.GRU -> last valid step) -----
 * Forward only (the encoder is frozen wherever the counterexample path calls it); eval mode (no dropout).  Semantics, gate order r, z, n
 * as torch.nn.GRU:
 *   len_b = max(1, #{t : wids[b, t] != 0})          process_lengths (seq2vec.py:11-17) for right-padded questions
 *   x_t = E[wids[b, t]]                              row 0 of E is read like any other row
 *   r = s(W_ir x + b_ir + W_hr h + b_hr);  z = s(W_iz x + b_iz + W_hz h + b_hz);  n = tanh(W_in x + b_in + r (W_hn h + b_hn))
 *   h' = (1 - z) n + z h, h_0 = 0;   q[b] = h after step len_b - 1          select_last (seq2vec.py:19-25)
 * A row is advanced only while t < len_b: the rows are ordered by length on the device and step t multiplies the n_t = #{len_b > t}
 * longest rows (one launch per step, always issued; nothing is read back).  The input projection E[wid] . W_ih^T rides in the same
 * launch, for the valid (row, t) pairs only.  No atomics, no inter-workgroup wait: bit-identical from run to run.
 * Unlike the rest of the ABI these four return -1 for ANY invalid argument (NULL pointer, dimension out of range, short or misaligned
 * buffer); 1 <= T <= 64, B, V1, dim_emb, dim_q >= 1.
 *
 * ncx_gru_pack takes the role of the encoder's construction in factory (seq2vec.py:79-97): nn.GRU's weight_ih_l0 [3 dim_q, dim_emb],
 * weight_hh_l0 [3 dim_q, dim_q], bias_ih_l0, bias_hh_l0 [3 dim_q] (gate blocks r | z | n) -> `packed` (ncx_gru_packed_bytes, 16-byte
 * aligned), once per weight set:
 *   W [ceil(dim_q / 32)][3 gates][32 units][kp] | bias [ceil(dim_q / 32)][6: ir iz in hr hz hn][32 units],  kp = pad32(dim_emb) + pad32(dim_q)
 *   W row (j, g, u) = W_i{g}[32 j + u, :] zero-padded to pad32(dim_emb), then W_h{g}[32 j + u, :] zero-padded to pad32(dim_q)
 * so a workgroup's 96 weight rows are the r, z and n rows of the SAME 32 hidden units and the gate arithmetic runs from registers. */
size_t ncx_gru_packed_bytes(int32_t dim_emb, int32_t dim_q);                               /* 0 for invalid dims */
int ncx_gru_pack(const float* w_ih, const float* w_hh, const float* b_ih, const float* b_hh, int32_t dim_emb, int32_t dim_q,
                 float* packed, void* stream);
/* Workspace of ncx_gru_encode (256-byte aligned: the length plan and the two h buffers); 0 for invalid dims. */
size_t ncx_gru_workspace_bytes(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q);
/* Takes the role of process_lengths + the GRU + select_last (seq2vec.py:11-25) in the encoder's forward: wids [B, T] int32, right-padded
 * with 0; E [V1, dim_emb] the embedding table; q_out [B, dim_q] in the input row order.  A word id outside [0, V1) is never used as an
 * address (it is clamped; that row's output is meaningless) and *bad_id_flag is set to 1 (never cleared here; the caller zeroes it). */
int ncx_gru_encode(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                   const float* packed, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream);
/* ncx_gru_encode (seq2vec.py:11-25) with `flags`: 0 (the same call, the same bits) or NCX_F_X6, which runs every step's product
 * [x_t | h_{t-1}] . [W_ih | W_hh]^T on the bf16 matrix path with three-plane operands (k_gru_step_x6, csrc/ncx_gru_x6.hip): the same packed
 * weights, the same workspace, the same T + 1 launches, the same epilogue; every legal shape, no fall-back to the fp32 kernel.  Results
 * agree with flags 0 to fp32 rounding, not bitwise; bit-identical from run to run.  Any other `flags` returns -1 before any launch or
 * pointer use. */
int ncx_gru_encode_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                         const float* packed, uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag,
                         void* stream);
/* Host only, no launch: which step kernel ncx_gru_encode_flags / ncx_gru_train_forward_flags take for these dims under `flags`:
 * 0 = the fp32 step kernel, 1 = the X6 step kernel, -1 = dims or flags refused. */
int ncx_gru_step_form(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q, uint32_t flags);

/* ---- training the question encoder: backward through time (csrc/ncx_gru_train.hip) -------------------------------------------------
 * Takes the role of torch autograd through GRUEncoder.forward -- nn.Embedding, nn.GRU and the last-step selection (the stand-in for the
 * encoder the reference builds in factory, seq2vec.py:79-97, and selects from in process_lengths + select_last, seq2vec.py:11-25); torch
 * walks all T steps of every row forward and backward, these entries walk the valid (row, t) pairs only.  len_b, the sorted row order
 * (perm) and n_t as above; for t from len_b - 1 down to 0, on the rows still inside their question:
 *   dh_t = [t == len_b - 1] dq_out[b] + (what step t + 1 sends back)
 *   dn = dh (1 - z);  dz = dh (h_{t-1} - n);  h_{-1} = 0
 *   da_n = dn (1 - n^2);  da_z = dz z (1 - z);  da_r = da_n hn r (1 - r);  da_hn = da_n r        hn = W_hn h_{t-1} + b_hn
 *   dh_{t-1} = dh z + [da_r | da_z | da_hn] . W_hh
 *   dGx_t = [da_r | da_z | da_n] -> dW_ih, db_ih, dX_t = dGx_t . W_ih;   dGh_t = [da_r | da_z | da_hn] -> dW_hh (t >= 1 only), db_hh
 * A row whose question is empty still takes its one step over wids[b, 0] = 0 and its gradients count; a zero id inside a question is
 * stepped over like any word.  dE[0] is ZERO whatever read E[0] in the forward (nn.Embedding(padding_idx=0): torch's embedding backward
 * skips that row); every other row of dE is the sum of dX_t[b] over the valid pairs with that word id.  Where no recurrent product ran
 * (all lengths 1, or T == 1) dW_hh is exactly 0.  No atomics: bit-identical from run to run.  Like the four entries above these return
 * -1 for ANY invalid argument.
 *
 * Workspace of one training step (256-byte aligned; 0 for invalid dims): the length plan, the word id of every valid pair, and the stash,
 * laid out [T][B] in the plan's sorted row order: h_t [dim_q]; the gates r | z | n | hn [4][dqp]; the gate gradients da_r | da_z | da_n |
 * da_hn [4][dqp] (dqp = pad32(dim_q), pad columns zero); two dh buffers [B][dim_q]; dX [T][B][dim_emb]. */
size_t ncx_gru_train_workspace_bytes(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q);
/* The backward's extra packed operands: weight_hh_l0 and weight_ih_l0 (seq2vec.py:79-97, as for ncx_gru_pack) with the contraction over the
 * 3 dim_q gate rows, once per weight set (16-byte aligned; ncx_gru_packed_t_bytes is 0 for invalid dims):
 *   WhhT [pad64(dim_q)][3 dqp] | WihT [pad64(dim_emb)][3 dqp],  WhhT[j][g dqp + u] = W_hh[g dim_q + u][j],  WihT[c][g dqp + u] = W_ih[g dim_q + u][c]
 * zero where u >= dim_q or the row does not exist. */
size_t ncx_gru_packed_t_bytes(int32_t dim_emb, int32_t dim_q);
int ncx_gru_pack_t(const float* w_ih, const float* w_hh, int32_t dim_emb, int32_t dim_q, float* packed_t, void* stream);
/* ncx_gru_encode's arguments, plan and step kernel (seq2vec.py:11-25), the kernel instantiated with a flag that also writes h_t, r, z, n and
 * hn of every valid (row, t) pair to the stash.  q_out is bit-identical to ncx_gru_encode's for the same inputs. */
int ncx_gru_train_forward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                          const float* packed, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream);
/* ncx_gru_train_forward with `flags`: 0 (the same call) or NCX_F_X6 (the KEEP instantiation of the X6 step kernel: the same stash layout,
 * so ncx_gru_train_backward consumes whichever stash the forward left).  q_out is bit-identical to ncx_gru_encode_flags's under the same
 * `flags`.  Any other `flags` returns -1 before any launch or pointer use. */
int ncx_gru_train_forward_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                                const float* packed, uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out,
                                int32_t* bad_id_flag, void* stream);
/* Takes the role of loss.backward() below q = seq2vec(wids) (torch's GRU, embedding and index backward).  `workspace` as the forward of
 * the same wids left it; dq_out [B, dim_q] in the input row order.  Outputs in torch's layouts: dW_ih [3 dim_q, dim_emb], dW_hh [3 dim_q,
 * dim_q], db_ih, db_hh [3 dim_q], dE [V1, dim_emb] (every row written).  dE == NULL: a fixed embedding (--st_fixed_emb), the dX product
 * and the scatter are skipped and the other four gradients are unchanged.  A word id outside [0, V1) was flagged by the forward; here it
 * is never used as an address either (its pair reads a clamped row of E and is left out of the dE sums). */
int ncx_gru_train_backward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                           const float* packed_t, void* workspace, size_t workspace_bytes, const float* dq_out,
                           float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, float* dE /*nullable*/, void* stream);
/* ncx_gru_train_backward with `flags`: 0 (the same call, the same launches, the same bits) or NCX_F_X6, which moves the matrix products of
 * the backward that ncx_gru_bwd_form names onto the bf16 matrix path with three-plane operands (csrc/ncx_gru_train_x6.hip): every operand
 * element is cut into three exact bf16 planes on its way to LDS, accumulation stays fp32, results agree with the fp32 kernels to fp32
 * rounding, not bitwise.  The packs, the workspace, its size and the stash layout are unchanged, so either form consumes whichever stash
 * the forward left (fp32 or X6 forward).  Still no atomics: bit-identical from run to run.  Any other `flags` returns -1 before any
 * launch or pointer use. */
int ncx_gru_train_backward_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t dim_emb, int32_t dim_q,
                                 const float* packed_t, uint32_t flags, void* workspace, size_t workspace_bytes, const float* dq_out,
                                 float* dW_ih, float* dW_hh, float* db_ih, float* db_hh, float* dE /*nullable*/, void* stream);
/* Host only, no launch: which products of ncx_gru_train_backward_flags take their X6 kernel for these dims under `flags`, as a bit mask:
 * bit 0 the reverse sweep (dh_{t-1} = dGh_t . W_hh), bit 1 dX = dGx . W_ih, bit 2 dW_hh, bit 3 dW_ih.  0 under flags 0; -1 = dims or
 * flags refused. */
int ncx_gru_bwd_form(int32_t B, int32_t T, int32_t dim_emb, int32_t dim_q, uint32_t flags);

/* ---- the two-layer LSTM question encoder: seq2vec arch `2-lstm` (csrc/ncx_lstm.hip) ------------------------------------------------
 * Takes the role of TwoLSTM.forward in eval mode (seq2vec.py:48-76).  Forward only; gate order i, f, g, o as torch.nn.LSTM:
 *   len_b = #{t : wids[b, t] != 0}, and T when that is 0      process_lengths (seq2vec.py:11-14); select_last's index len_b - 1 = -1 is the
 *                                                             LAST step (seq2vec.py:16-25), so an all-padding row runs T steps on E[0]
 *   x_t = tanh(E[wids[b, t]])                                 seq2vec.py:63-64; row 0 of E is read like any other row
 *   layer l in {0, 1}:  [i f g o] = W_ih^l x + b_ih^l + W_hh^l h + b_hh^l;  c' = s(f) c + s(i) tanh(g);  h' = s(o) tanh(c');  h_0 = c_0 = 0
 *   layer 1's x_t is layer 0's h_t                            seq2vec.py:65, 70
 *   q[b] = [h^0 | h^1] after step len_b - 1                   seq2vec.py:66, 71, 75
 * The recurrence runs over TIME.  The reference builds its nn.LSTMs without batch_first and feeds them [B, T, emb], so as written it runs
 * over the batch axis and a question's vector depends on its place in the batch; the parameters' names and shapes are the same either way.
 * A row is advanced only while t < len_b (length plan as ncx_gru_encode).  Launch s in [0, T] runs layer 0 at step s and layer 1 at step
 * s - 1 side by side: T + 2 launches with the plan, nothing read back, no atomics, no inter-workgroup wait, bit-identical from run to run.
 * Like the ncx_gru_* entries these return -1 for ANY invalid argument; emb, H, B, V1 >= 1, 1 <= T <= 64.
 *
 * ncx_lstm2_pack takes the role of TwoLSTM's construction in factory (seq2vec.py:86-89): rnn_0's weight_ih_l0 [4 H, emb], weight_hh_l0
 * [4 H, H], bias_ih_l0, bias_hh_l0 [4 H] and rnn_1's ([4 H, H] both) -> `packed` (ncx_lstm2_packed_bytes, 16-byte aligned), once per
 * weight set:  layer 0 | layer 1,  layer l = W [ceil(H / 32)][4 gates][32 units][kp_l] | bias [ceil(H / 32)][4][32 units]
 *   kp_0 = pad32(emb) + pad32(H), kp_1 = 2 pad32(H);  W row (j, g, u) = W_ih[g H + 32 j + u, :] zero-padded, then W_hh[g H + 32 j + u, :]
 *   zero-padded;  bias (j, g, u) = b_ih[g H + 32 j + u] + b_hh[g H + 32 j + u] (one fp32 addition) */
size_t ncx_lstm2_packed_bytes(int32_t emb, int32_t H);                                     /* 0 for invalid dims */
int ncx_lstm2_pack(const float* w_ih0, const float* w_hh0, const float* b_ih0, const float* b_hh0, const float* w_ih1, const float* w_hh1,
                   const float* b_ih1, const float* b_hh1, int32_t emb, int32_t H, float* packed, void* stream);
/* Workspace of ncx_lstm2_encode (256-byte aligned: the length plan, two h buffers and the cell state per layer); 0 for invalid dims. */
size_t ncx_lstm2_workspace_bytes(int32_t B, int32_t T, int32_t emb, int32_t H);
/* Takes the role of process_lengths, both nn.LSTMs and select_last (seq2vec.py:11-25, 61-76): wids [B, T] int32; E [V1, emb] the embedding
 * table; q_out [B, 2 H] in the input row order.  q_out does not depend on what the workspace held.  A word id outside [0, V1) is never
 * used as an address (clamped; that row's output is meaningless) and *bad_id_flag is set to 1, as by ncx_gru_encode. */
int ncx_lstm2_encode(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                     void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream);
/* ncx_lstm2_encode (seq2vec.py:11-25, 61-76) with `flags`: 0 (the same call, the same bits) or NCX_F_X6, which runs every step's product
 * [x_t | h_{t-1}] . [W_ih | W_hh]^T of both layers on the bf16 matrix path with three-plane operands (k_lstm_step_x6, csrc/ncx_lstm_x6.hip):
 * the same packed weights, the same workspace, the same T + 2 launches, the same epilogue; every legal shape, no fall-back to the fp32
 * kernel.  Results agree with flags 0 to fp32 rounding, not bitwise; bit-identical from run to run.  Any other `flags` returns -1 before
 * any launch or pointer use. */
int ncx_lstm2_encode_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                           uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream);
/* Host only, no launch: which step kernel ncx_lstm2_encode_flags / ncx_lstm2_train_forward_flags take for these dims under `flags`:
 * 0 = the fp32 step kernel, 1 = the X6 step kernel, -1 = dims or flags refused. */
int ncx_lstm2_step_form(int32_t B, int32_t T, int32_t emb, int32_t H, uint32_t flags);

/* ---- training the two-layer LSTM question encoder: backward through time (csrc/ncx_lstm_train.hip) ----------------------------------
 * Take the role of torch autograd through TwoLSTM.forward below its dropout (seq2vec.py:48-76: tanh(embedding), rnn_0, rnn_1, and the
 * selection of process_lengths + select_last, seq2vec.py:11-25); torch walks all T steps of every row forward and backward, these entries
 * walk the valid (row, t) pairs only.  len_b, the sorted row order (perm) and n_t as ncx_lstm2_encode; per layer l, for t from len_b - 1
 * down to 0, on the rows still inside their question:
 *   dh^l_t = [t == len_b - 1] dq_out[b, l H : (l + 1) H] + da^l_{t+1} . W_hh^l  (+ da^1_t . W_ih^1 when l == 0)
 *   dc_t   = dc_{t+1} f_{t+1} + dh_t o_t (1 - tanh(c_t)^2)
 *   da_o = dh_t tanh(c_t) o (1 - o);  da_i = dc_t g i (1 - i);  da_g = dc_t i (1 - g^2);  da_f = dc_t c_{t-1} f (1 - f)      c_{-1} = 0
 *   dW_ih^l = sum da^l_t^T x^l_t;  dW_hh^l = sum_{t >= 1} da^l_t^T h^l_{t-1};  db_ih^l = db_hh^l = sum da^l_t
 *   dX_t = da^0_t . W_ih^0;  dE[w] = (sum over the valid pairs with id w of dX_t) (1 - tanh(E[w])^2)
 * An all-padding row runs its T steps on E[0] and its weight gradients count; a zero id inside a question is stepped over like any word.
 * dE[0] is ZERO whatever read E[0] in the forward (nn.Embedding(padding_idx=0)).  Where no recurrent product ran (all lengths 1, or
 * T == 1) dW_hh^0 and dW_hh^1 are exactly 0; dW_ih^1 is not.  No atomics: bit-identical from run to run.  -1 for ANY invalid argument;
 * emb, H, B, V1 >= 1, 1 <= T <= 64.
 *
 * Workspace of one training step (256-byte aligned; 0 for invalid dims): the length plan, the word id of every valid pair, and per layer
 * the stash, laid out [T][B] in the plan's sorted row order: h_t [H]; c_t [H]; the gates i | f | g | o [4][Hp]; the gate gradients da_i |
 * da_f | da_g | da_o [4][Hp] (Hp = pad32(H), pad columns zero); dc_t f_t [B][H]; and dX [T][B][emb]. */
size_t ncx_lstm2_train_workspace_bytes(int32_t B, int32_t T, int32_t emb, int32_t H);
/* The backward's packed operands: rnn_0's weight_ih_l0, weight_hh_l0 and rnn_1's (seq2vec.py:86-89, as for ncx_lstm2_pack) with the
 * contraction over the 4 H gate rows contiguous, once per weight set (16-byte aligned; ncx_lstm2_packed_t_bytes is 0 for invalid dims):
 *   P0 [pad64(H)][8 Hp] | P1 [pad64(H)][4 Hp] | PX [pad64(emb)][4 Hp]
 *   P0[j][g Hp + u] = W_hh^0[g H + u][j],  P0[j][4 Hp + g Hp + u] = W_ih^1[g H + u][j],  P1[j][g Hp + u] = W_hh^1[g H + u][j],
 *   PX[c][g Hp + u] = W_ih^0[g H + u][c];  zero where u >= H or the row does not exist. */
size_t ncx_lstm2_packed_t_bytes(int32_t emb, int32_t H);
int ncx_lstm2_pack_t(const float* w_ih0, const float* w_hh0, const float* w_ih1, const float* w_hh1, int32_t emb, int32_t H, float* packed_t,
                     void* stream);
/* ncx_lstm2_encode's arguments, plan and step kernel (seq2vec.py:11-25, 61-76), the kernel instantiated with a flag that also writes h_t, c_t
 * and the four activated gates of every valid (row, t) pair of both layers to the stash.  q_out is bit-identical to ncx_lstm2_encode's. */
int ncx_lstm2_train_forward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed,
                            void* workspace, size_t workspace_bytes, float* q_out, int32_t* bad_id_flag, void* stream);
/* ncx_lstm2_train_forward with `flags`: 0 (the same call) or NCX_F_X6 (the KEEP instantiation of the X6 step kernel: the same stash layout,
 * pad columns zero, so ncx_lstm2_train_backward consumes whichever stash the forward left).  q_out is bit-identical to
 * ncx_lstm2_encode_flags's under the same `flags`.  Any other `flags` returns -1 before any launch or pointer use. */
int ncx_lstm2_train_forward_flags(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H,
                                  const float* packed, uint32_t flags, void* workspace, size_t workspace_bytes, float* q_out,
                                  int32_t* bad_id_flag, void* stream);
/* Takes the role of loss.backward() below q = seq2vec(wids) (torch's LSTM, tanh, embedding and index backward; seq2vec.py:61-76).
 * `workspace` as the forward of the same wids left it; dq_out [B, 2 H] in the input row order.  Outputs in torch's layouts: dW_ih0 [4 H,
 * emb], dW_hh0, dW_ih1, dW_hh1 [4 H, H], the four db [4 H], dE [V1, emb]; every element of every output is written.  dE == NULL: a fixed
 * embedding, the dX product and the scatter are skipped and the other eight gradients are unchanged.  A word id outside [0, V1) was
 * flagged by the forward; here it is never used as an address either (its pair reads a clamped row of E and is left out of the dE sums). */
int ncx_lstm2_train_backward(const int32_t* wids, int32_t B, int32_t T, const float* E, int32_t V1, int32_t emb, int32_t H, const float* packed_t,
                             void* workspace, size_t workspace_bytes, const float* dq_out, float* dW_ih0, float* dW_hh0, float* db_ih0,
                             float* db_hh0, float* dW_ih1, float* dW_hh1, float* db_ih1, float* db_hh1, float* dE /*nullable*/, void* stream);

/* ---- the trainable scorers LinearContext and PairwiseLinearModel (reference vqa/models/cx.py:139-156, 379-425) ---------
 * Both train with the library's loss (ncx_loss_rank) and optimiser (ncx_adam_step): forward -> scores, ncx_loss_rank ->
 * dscores, backward -> gradients (the reference's loop, counterexamples.py:330-339).  Neither model has dropout.
 * Dims: 1 <= K <= 64, B >= 1, K dz >= 4.  PairwiseLinearModel also needs dv, dq, dz >= 4, A >= 1 (answers), n_img >= 1 (rows of
 * the feature table); its hidden width and answer-embedding width are the reference's fixed 300 (cx.py:391-392). */
typedef struct ncx_scorer_dims {
    int32_t B, K, dv, dq, dz, A, n_img;
} ncx_scorer_dims;

/* PairwiseLinearModel's trainable tensors, state_dict names of the reference (cx.py:394-400). */
typedef struct ncx_pairlin_params {
    const float* answer_embedding;       /* answer_embedding.weight [A, 300]                         */
    const float* w;  const float* b;     /* linear.weight [300, Din], Din = 2 dv + dq + 2 dz + 300;  .bias [300]
                                            columns in the reference's concat order (cx.py:416):
                                            v_orig | v_other | q_emb | z_orig | z_other | a_emb      */
    const float* w_out; const float* b_out;  /* out.weight [1, 300], out.bias [1]                    */
} ncx_pairlin_params;
typedef struct ncx_pairlin_grads {
    float* answer_embedding; float* w; float* b; float* w_out; float* b_out;   /* shapes of ncx_pairlin_params; overwritten */
} ncx_pairlin_grads;

/* Workspace of ncx_pairlin_forward / _backward (256-byte aligned); 0 for unsupported dims.  The backward reads what the forward
 * left there: call both with the same dims, inputs and workspace. */
size_t ncx_pairlin_workspace_bytes(const ncx_scorer_dims* d);
/* Replaces PairwiseLinearModel.forward below vqa_forward (cx.py:401-425): scores [B, K] = relu(out(relu(linear(x_k)))).
 * Reads in->feats, img_idx, q_emb, z_orig, z_knns, answer_aids (the other fields are ignored).  A feature row or answer id out of
 * range is clamped and sets *bad_id_flag to 1 (never cleared here; the reference raises IndexError there). */
int ncx_pairlin_forward(const ncx_scorer_dims* d, const ncx_inputs* in, const ncx_pairlin_params* p, void* workspace,
                        size_t workspace_bytes, float* scores, int32_t* bad_id_flag, void* stream);
/* Replaces loss.backward() (counterexamples.py:338) for PairwiseLinearModel: every gradient of ncx_pairlin_grads from dscores
 * [B, K].  d answer_embedding is dense: rows no answer id points at are 0, duplicated ids are summed in batch order.
 * Reads in->feats, q_emb, z_orig, z_knns; the feature rows and answer ids are the clamped ones ncx_pairlin_forward left in the
 * workspace (in->img_idx and in->answer_aids are not read), as are h, P and the scores. */
int ncx_pairlin_backward(const ncx_scorer_dims* d, const ncx_inputs* in, const ncx_pairlin_params* p, void* workspace,
                         size_t workspace_bytes, const float* dscores, const ncx_pairlin_grads* g, void* stream);
/* LinearContext (cx.py:147-155): scores [B, K] = z_knns.view(B, K dz) . w^T + b, w = linear.weight [K, K dz], b = linear.bias [K]. */
size_t ncx_linctx_workspace_bytes(const ncx_scorer_dims* d);
int ncx_linctx_forward(const ncx_scorer_dims* d, const float* z_knns, const float* w, const float* b, void* workspace,
                       size_t workspace_bytes, float* scores, void* stream);
/* ... its loss.backward(): gw = dscores^T . z_flat [K, K dz], gb = sum over b of dscores [K] (overwritten). */
int ncx_linctx_backward(const ncx_scorer_dims* d, const float* z_knns, const float* dscores, void* workspace,
                        size_t workspace_bytes, float* gw, float* gb, void* stream);

/* ---- the contrastive training path (reference contrastive.py; ContrastiveModel, vqa/models/cx.py:428-487) --------------------
 * A siamese embedding h = relu(linear(cat(v, z))) of the P = knn_size + 1 images of an example (slot 0 the original), hidden
 * width 300 (cx.py:437), trained with a margin loss on distances.  linear.weight is [300, dv + dz], columns v | z (cx.py:445,
 * 471).  The model's answer_embedding.weight (cx.py:440-441) is never read and never receives a gradient: it has no entry here.
 * Dims: B >= 1, 1 <= P - 1 <= 64, dv >= 4, dz >= 4, n_img >= 1 (rows of the feature table). */
typedef struct ncx_contrastive_dims {
    int32_t B, P, dv, dz, n_img;
} ncx_contrastive_dims;
/* Workspace of the four entry points below (256-byte aligned); 0 for unsupported dims.  distances / loss / backward read what
 * the forward left there: call them with the same dims and workspace. */
size_t ncx_contrastive_workspace_bytes(const ncx_contrastive_dims* d);
/* Replaces ContrastiveModel.forward below vqa_forward (cx.py:448-472): h [B, P, 300] (nullable: it always stays in the workspace).
 * Reads in->feats, img_idx [B, P], z_orig [B, dz], z_knns [B, P - 1, dz]; w = linear.weight, b = linear.bias.  The feature rows are
 * gathered by id, never copied out dense.  A row id out of range is clamped and sets *bad_id_flag to 1 (never cleared here; the
 * reference's indexing raises there). */
int ncx_contrastive_forward(const ncx_contrastive_dims* d, const ncx_inputs* in, const float* w, const float* b, void* workspace,
                            size_t workspace_bytes, float* h, int32_t* bad_id_flag, void* stream);
/* Replaces ContrastiveModel.get_scores (cx.py:478-487): dist [B, P - 1], dist[b, k] = || h[b, 0] - h[b, k + 1] + 1e-6 ||_2
 * (F.pairwise_distance).  h [B, P, 300] (16-byte aligned), or NULL: the h the forward left in the workspace (with h given the
 * workspace is not read and may be NULL).  The evaluation (contrastive.py:274-279) ranks the distances with ncx_loss_rank: the
 * counterexample should be the farthest. */
int ncx_contrastive_distances(const ncx_contrastive_dims* d, const float* h, void* workspace, size_t workspace_bytes, float* dist,
                              void* stream);
/* Replaces the two ContrastiveLoss calls and loss.backward() down to the pre-activation (contrastive.py:217-219, 300-309), P = 3
 * (original, counterexample, one other neighbour):
 *   losses4 = scale x {sum_b max(margin - d_b1, 0)^2, sum_b d_b2^2, sum_b d_b1, sum_b d_b2}: with scale = 1 / B the reference's
 *   loss_comp, loss_other and the two mean distances it logs (contrastive.py:229-231); dist [B, 2] = the per-example distances
 *   (nullable).  The gradient with respect to the pre-activation stays in the workspace for ncx_contrastive_backward.
 * Sums over b run in a fixed order: bit-identical from run to run. */
int ncx_contrastive_loss(const ncx_contrastive_dims* d, void* workspace, size_t workspace_bytes, float margin, float scale,
                         float* losses4, float* dist, void* stream);
/* The rest of loss.backward() (contrastive.py:223): gw = d linear.weight [300, dv + dz], gb = d linear.bias [300] (overwritten).
 * dh == NULL: from the pre-activation gradient ncx_contrastive_loss left in the workspace.  dh [B, P, 300] (16-byte aligned): the
 * gradient with respect to h from outside (autograd of a caller's own loss); the ReLU mask is applied here.  Reads in->feats; the
 * row ids and z are the ones the forward left in the workspace. */
int ncx_contrastive_backward(const ncx_contrastive_dims* d, const ncx_inputs* in, void* workspace, size_t workspace_bytes,
                             const float* dh, float* gw, float* gb, void* stream);

/* ---- training the MutanNoAtt VQA model (reference train.py:136-145, vqa/lib/engine.py:6-56) -------------------------------------
 * The fusion and classifier of MutanNoAtt in TRAINING mode, one image per question (row b reads feats[img_idx[b]]; an id outside
 * [0, n_img) is clamped), with the stashes its backward needs; the cross-entropy head; the backward.  The question encoder stays
 * outside: q_emb comes in, d loss / d q_emb goes out on request (torch autograd carries it into the encoder).  Supported model:
 * what ncx_mutan_params expresses (activation_v / activation_q in {none, tanh}, no activation_hv / _hq / _mm, no
 * classif.activation, dropout_hv = dropout_hq = 0): every MutanNoAtt YAML of the reference.  The optimiser is ncx_adam_step.
 * Dims: B >= 1; dv, dq, dz, A, dhv, dhq >= 4; 1 <= R <= 10; 0 <= p < 1.  Status codes as the rest of the ABI, checked before any
 * launch; no allocation, no atomics, no host read-back; bit-identical from run to run. */
typedef struct ncx_vqa_train_dims {
    int32_t B, dv, dq, dz, A, n_img;
    float   p_v, p_q, p_c;     /* fusion.dropout_v, fusion.dropout_q (fusion.py:82,88), classif.dropout on z (noatt.py:27)        */
    int32_t dropout_mode;      /* 0 off (the eval forward), 1 counter-based generator keyed by `seed` (layer ids 1 v, 2 q, 3 z;
                                  element index row * width + column; oracle/ncx_oracle.py:dropout_keep_mask), 2 explicit masks  */
    int32_t want_dq;           /* backward also writes d loss / d q_emb                                                         */
    int32_t pad_;
    uint64_t seed;
} ncx_vqa_train_dims;
typedef struct ncx_mutan_grads {          /* shapes of ncx_mutan_params' tensors; OVERWRITTEN by ncx_vqa_train_backward */
    float* wv;  float* bv;  float* wq;  float* bq;  float* whv; float* bhv; float* whq; float* bhq; float* wc;  float* bc;
} ncx_mutan_grads;
/* Workspace of the forward / backward pair (256-byte aligned); 0 for invalid dims or an unsupported activation.  R, dhv, dhq,
 * act_v, act_q are read from `m` (its pointers are not). */
size_t ncx_vqa_train_workspace_bytes(const ncx_vqa_train_dims* d, const ncx_mutan_params* m);
/* Replaces model(input_visual, input_question) of the train step (engine.py:22) below seq2vec: MutanFusion.forward
 * (fusion.py:78-121) and AbstractNoAtt._classif (noatt.py:24-29) with F.dropout active.  logits [B, A]; z [B, dz] is the fusion
 * output before the classifier's dropout.  masks (dropout_mode 2 only, else nullable): keep masks as 0 / 1 floats,
 * [B, dv] | [B, dq] | [B, dz] back to back; a kept element is scaled by 1 / (1 - p).  dropout_mode 0 is the eval forward. */
int ncx_vqa_train_forward(const ncx_vqa_train_dims* d, const float* feats, const int32_t* img_idx, const float* q_emb,
                          const ncx_mutan_params* m, const float* masks, void* workspace, size_t workspace_bytes,
                          float* logits, float* z, void* stream);
/* Replaces nn.CrossEntropyLoss()(output, target) (train.py:136, engine.py:24), its gradient, and utils.accuracy(topk=(1, 5))
 * (vqa/lib/utils.py:23-38) as hit COUNTS:
 *   loss[1] = scale sum_b (logsumexp(logits[b]) - logits[b][target[b]])            scale = 1 / B when scale <= 0   (nullable)
 *   dlogits [B, A] = (softmax - onehot) scale                                                                        (nullable)
 *   hits_top1[1], hits_top5[1] = #{b : rank_b < 1}, #{b : rank_b < 5}, rank_b = #{c : x_c > x_t} + #{c < t : x_c == x_t}   (nullable)
 * rows: [2 B] words of scratch (the per-example terms; the sums over b are taken from it in a fixed order by one workgroup).
 * A target outside [0, A) is never used as an address: that example contributes 0 to every output, its dlogits row is 0 and
 * *bad_flag is set to 1 (never cleared here; the caller zeroes it). */
int ncx_ce_loss(const float* logits, const int32_t* target, int32_t B, int32_t A, float scale, float* loss, float* dlogits,
                int32_t* hits_top1, int32_t* hits_top5, int32_t* bad_flag, float* rows, void* stream);
/* Replaces loss.backward() (engine.py:36) for the tensors of ncx_mutan_params: every field of `g` is overwritten; dq_emb [B, dq]
 * = d loss / d q_emb when d->want_dq (else nullable).  No gradient is taken with respect to the image features.  Reads what the
 * forward left in the workspace: same dims, params, masks and workspace. */
int ncx_vqa_train_backward(const ncx_vqa_train_dims* d, const ncx_mutan_params* m, const float* masks, void* workspace,
                           size_t workspace_bytes, const float* dlogits, const ncx_mutan_grads* g, float* dq_emb, void* stream);
/* Diagnostics / tests: byte offset and size of the tensors the forward dropped, valid after ncx_vqa_train_forward. */
#define NCX_VT_WS_VD 1   /* drop_v(feats[img_idx]) [B, dv] */
#define NCX_VT_WS_QD 2   /* drop_q(q_emb)          [B, dq] */
#define NCX_VT_WS_ZC 3   /* drop_c(z)              [B, dz] */
int ncx_vqa_train_ws_region(const ncx_vqa_train_dims* d, const ncx_mutan_params* m, int32_t which, size_t* offset, size_t* bytes);

/* ---- training the MLBNoAtt VQA model: the sibling of the block above for the factory's second no-attention model ------------------
 * The fusion and classifier of MLBNoAtt in TRAINING mode (MLBFusion.forward vqa/models/fusion.py:31-50, AbstractNoAtt._classif
 * vqa/models/noatt.py:24-29), one image per question (row b reads feats[img_idx[b]]; an id outside [0, n_img) is clamped):
 *   vd = drop_v(feats[img_idx])   qd = drop_q(q_emb)   x_v = act_v(vd Wv^T + bv)   x_q = act_q(qd Wq^T + bq)          [B, dh]
 *   z = x_q * x_v (returned: the fusion output, BEFORE act_c)   t = act_c(z)   tc = drop_c(t)   logits = tc Wc^T + bc   [B, A]
 * Every activation in {none, tanh} (0 / 2), classif.activation included.  Takes ncx_vqa_train_dims with d->dz == m->dh (else
 * NCX_E_DIMS) and its dropout modes: layer ids 1 (v), 2 (q), 3 (the classifier's input); explicit masks [B, dv] | [B, dq] | [B, dh].
 * The loss is ncx_ce_loss, the optimiser ncx_adam_step.  Dims: B >= 1; dv, dq, dh, A >= 4; 0 <= p < 1.  Status codes as the rest
 * of the ABI, checked before any launch; no allocation, no atomics, no host read-back; bit-identical from run to run. */
typedef struct ncx_mlb_grads {            /* shapes of ncx_mlb_params' tensors; OVERWRITTEN by ncx_mlb_train_backward */
    float* wv;  float* bv;  float* wq;  float* bq;  float* wc;  float* bc;
} ncx_mlb_grads;
/* Workspace of the forward / backward pair (256-byte aligned); 0 for invalid dims or an unsupported activation.  dh and the
 * activation codes are read from `m` (its pointers are not). */
size_t ncx_mlb_train_workspace_bytes(const ncx_vqa_train_dims* d, const ncx_mlb_params* m);
/* logits [B, A]; z [B, dh].  masks: dropout_mode 2 only, else nullable.  dropout_mode 0 is the eval forward.  x_v, x_q, t and the
 * dropped tensors stay in the workspace for the backward. */
int ncx_mlb_train_forward(const ncx_vqa_train_dims* d, const float* feats, const int32_t* img_idx, const float* q_emb,
                          const ncx_mlb_params* m, const float* masks, void* workspace, size_t workspace_bytes,
                          float* logits, float* z, void* stream);
/* Every field of `g` is overwritten; dq_emb [B, dq] = d loss / d q_emb when d->want_dq (else nullable).  No gradient is taken with
 * respect to the image features.  Reads what the forward left in the workspace: same dims, params, masks and workspace. */
int ncx_mlb_train_backward(const ncx_vqa_train_dims* d, const ncx_mlb_params* m, const float* masks, void* workspace,
                           size_t workspace_bytes, const float* dlogits, const ncx_mlb_grads* g, float* dq_emb, void* stream);
/* which: NCX_VT_WS_VD, NCX_VT_WS_QD, NCX_VT_WS_ZC (here tc = drop_c(act_c(z)) [B, dh]); valid after ncx_mlb_train_forward. */
int ncx_mlb_train_ws_region(const ncx_vqa_train_dims* d, const ncx_mlb_params* m, int32_t which, size_t* offset, size_t* bytes);

/* ---- training the MLBAtt attention model: the step below the question encoder -----------------------------------------
 * MLBAtt in TRAINING mode (reference vqa/models/att.py:39-163) on ncx_mlb_att_dims / ncx_mlb_att_params: forward with the six dropouts
 * active, backward through the classifier, the glimpse fusion, the pooling, the softmax over positions and the attention head.  No
 * gradient goes to the feature table.  Dropout layers (generator layer id; element index = linear index in the tensor named):
 *   1 the map fed to conv_v_att [B, dv, P] (the pooled map is NOT dropped)   2 q_emb fed to linear_q_att [B, dq]
 *   3 x_att after activation_mm [B, P, dh_att]                               4 v_att fed to the glimpse Linears [B, G, dv]
 *   5 q_emb fed to linear_q_fusion [B, dq]                                   6 act_c(x_v * x_qf) [B, G dh_f]
 * dropout_mode as in ncx_vqa_train_dims: 0 off, 1 the counter-based generator under `seed` (keep <=> u >= p, scale 1 / (1 - p)),
 * 2 explicit keep masks (0 / 1 floats), the six tensors concatenated in that order.  0 <= p < 1.  Status codes as the rest of the ABI,
 * all checked before any launch (NULL pointers, dims, modes, p's); no allocation; every launch on `stream`; no host read-back; no
 * float atomics, every reduction in a fixed order: two calls on the same inputs are bit-identical.  The loss is ncx_ce_loss. */
typedef struct ncx_mlb_att_train {
    float    p_att_v, p_att_q, p_att_mm, p_v, p_q, p_c;   /* layers 1 .. 6 */
    int32_t  dropout_mode;
    int32_t  want_dq;          /* backward also writes d loss / d q_emb */
    uint64_t seed;
} ncx_mlb_att_train;
typedef struct ncx_mlb_att_grads {        /* shapes of ncx_mlb_att_params' tensors; OVERWRITTEN by ncx_mlb_att_train_backward */
    float* wv_att; float* bv_att; float* wq_att; float* bq_att; float* wa; float* ba;
    float* wg;     float* bg;     float* wqf;    float* bqf;    float* wc; float* bc;
} ncx_mlb_att_grads;
/* Workspace of the forward / backward pair (256-byte aligned); 0 for invalid dims, modes, p's or activations (m's pointers are not read). */
size_t ncx_mlb_att_train_workspace_bytes(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const ncx_mlb_att_params* m);
/* feats, img_idx, q_emb as ncx_mlb_att_forward; logits [B, A]; att [B, G, P].  masks: dropout_mode 2 only, else nullable.  Xv, x_q,
 * v_att, x_v, x_qf, t and the dropped tensors stay in the workspace for the backward. */
int ncx_mlb_att_train_forward(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const float* feats, const int32_t* img_idx,
                              const float* q_emb, const ncx_mlb_att_params* m, const float* masks, void* workspace,
                              size_t workspace_bytes, float* logits, float* att, void* stream);
/* ncx_mlb_att_train_forward (att.py:39-163) with `flags`: 0 (the same call) or NCX_F_X6 (the Xv stash, the position logits and the maps
 * come from the X6 form of the conv_v_att product); any other value is NCX_E_DIMS before any launch.  ncx_mlb_att_train_backward[_flags]
 * runs after either, whatever its own flags. */
int ncx_mlb_att_train_forward_flags(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const float* feats, const int32_t* img_idx,
                                    const float* q_emb, const ncx_mlb_att_params* m, const float* masks, uint32_t flags, void* workspace,
                                    size_t workspace_bytes, float* logits, float* att, void* stream);
/* After ncx_mlb_att_train_forward[_flags] on the same workspace, inputs and `att`.  Every field of `g` is overwritten; dq_emb [B, dq] when
 * t->want_dq (else nullable).  The Xv stash is overwritten with dXv: one backward per forward. */
int ncx_mlb_att_train_backward(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const float* feats, const int32_t* img_idx,
                               const float* q_emb, const ncx_mlb_att_params* m, const float* masks, void* workspace,
                               size_t workspace_bytes, const float* att, const float* dlogits, const ncx_mlb_att_grads* g,
                               float* dq_emb, void* stream);
/* ncx_mlb_att_train_backward with `flags`: 0 (the same call) or NCX_F_X6, which puts d conv_v_att.weight[h, c] = sum over b, p of
 * dXv[b, p, h] V[b, c, p] (the twin of the forward's conv_v_att product; V is the dropped map when layer 1 is on, else the table read
 * through img_idx) on the bf16 matrix path with three-plane operands; P < 4 stays fp32; every other gradient and dq_emb are the bits
 * of the fp32 call.  Any other value is NCX_E_DIMS before any launch.  Same workspace and the same partial-sum slab (NCX_AT_WS_DWV),
 * written without atomics and summed in the same order: two calls are bit-identical.  d conv_v_att.weight agrees with the fp32 form
 * to fp32 rounding, not bitwise.  A non-finite map or dXv value is outside the X6 contract (the cut computes Inf - Inf). */
int ncx_mlb_att_train_backward_flags(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const float* feats, const int32_t* img_idx,
                                     const float* q_emb, const ncx_mlb_att_params* m, const float* masks, uint32_t flags, void* workspace,
                                     size_t workspace_bytes, const float* att, const float* dlogits, const ncx_mlb_att_grads* g,
                                     float* dq_emb, void* stream);
/* Host only, no launch: which kernel ncx_mlb_att_train_backward_flags takes for d conv_v_att.weight under `flags` (0 or NCX_F_X6).
 * 0 k_att_dwv_small (P < 4), 1 fp32 k_att_dwv, 2 k_att_dwv_x6; negative: the status the backward returns for these dims or flags. */
int ncx_mlb_att_dwv_form(const ncx_mlb_att_dims* d, uint32_t flags);
/* Diagnostics / tests: byte offset and size of a workspace region. */
#define NCX_AT_WS_XV     1   /* Xv = act_v_att(conv_v_att(drop(V))) [B, P, dh_att]; dXv after the backward               */
#define NCX_AT_WS_VATT   2   /* v_att [B, G, dv], before layer 4's dropout                                                 */
#define NCX_AT_WS_T      3   /* t = act_c(x_v * x_qf) [B, G dh_f], before layer 6's dropout                                */
#define NCX_AT_WS_VD     4   /* drop(V) [B, dv, P]; 0 bytes when layer 1 is off (the table is read in place)               */
#define NCX_AT_WS_DWV    5   /* partial sums of d conv_v_att.weight [S][dh_att][dv], one per group of ceil(B / S) images   */
int ncx_mlb_att_train_ws_region(const ncx_mlb_att_dims* d, const ncx_mlb_att_train* t, const ncx_mlb_att_params* m, int32_t which,
                                size_t* offset, size_t* bytes);

/* ---- diagnostics (bench.py / tests only; the only process-global state, off by default) --------------
 * GEMM ids: 0 Gt = W1[:,a_other].E^T, 1 Sh (shared segments), 2 MAIN (candidate segments, the dominant
 * forward kernel), 3 hidden layer l>=2 forward, 4 dW1 candidate columns (+dGt; the dominant backward
 * kernel; the shared columns ride in the same launch), 5 (unused: merged into 4), 6 dE, 7 dW1[:,a_other], 8 dA_gt, 9 dW_l (l>=2), 10 dX_l (l>=2).
 * ncx_profile_begin arms HIP-event timing (on the launch stream) of every launch of the gemm ids in the mask,
 * including a split-K fix-up; ncx_profile_end synchronises those events, writes up to `cap` (duration ms, id)
 * pairs and returns how many, then disarms.  Not thread safe; do not arm during graph capture. */
#define NCX_GEMM_GT 0
#define NCX_GEMM_SH 1
#define NCX_GEMM_MAIN 2
#define NCX_GEMM_FWD_L 3
#define NCX_GEMM_DW1C 4
#define NCX_GEMM_DW1S 5
#define NCX_GEMM_DE 6
#define NCX_GEMM_DW1AK 7
#define NCX_GEMM_DAGT 8
#define NCX_GEMM_DWL 9
#define NCX_GEMM_DXL 10
/* Not a GEMM id: ncx_plan_query(d, NCX_QUERY_DW1_ROUTE, out6) reports the routes of linear_1's weight gradient for a whole backward.
 * out6 = {v columns: 0 none (bf16 variant: in its bf16 candidate product), 1 k_dw_km8, 2 k_dw_km_x6, 3 k_dw_km (per-triplet fold
 *         kernels), 4 the grouped generic GEMM;
 *         dGt + every other column block (bf16 variant: its fp32 shared segments): 0 grouped generic GEMM, 1 k_dw_tn8, 2 k_dw_tn8_x6;
 *         pieces per workgroup of that TN launch's plan and its grid (reported even when the route is rejected; 0 / 0 where the
 *         kernel's shape rules exclude it); dW1[:, a_other] on the TN kernel (1) or the chain GEMM (0); the piece limit (out6[2] above
 *         it: grouped)} */
#define NCX_QUERY_DW1_ROUTE 32
/* Not a GEMM id either: out6 = {1 when ncx_backward_adam applies Adam inside the answer_embedding gradient's launch for these dims (given an
 * unpadded embedding slice), else 0; the passenger workgroups of that launch; 0, 0, 0, 0} */
#define NCX_QUERY_FUSED_ADAM 33
/* Not a GEMM id either: the route ncx_forward takes through its Linear layers for these dims, as launched (experiment hooks applied; read
 * from the functions the launchers themselves call).
 * out6 = {linear_1's engine: 0 the generic segmented GEMM, 1 the fused forward kernel on a chain of segments, 2 the fused forward kernel with
 *         the per-triplet fold of the two v segments, 3 the bf16 variant's product;
 *         its tile form -- chain: 0 48x128, 1 96x64, 2 96x128, 3 160x128, 4 64x64 (short chains); fold: the tile rows 48 / 96 / 192; generic
 *         engine: the tile cfg code of ncx_plan_query(NCX_GEMM_MAIN); bf16: 0;
 *         k-chunks per output tile (1 = no split; bf16: 0);
 *         1 when the pairwise distance is computed inside the fused forward kernel, else 0 (k_prep computes it);
 *         the hidden layers' engine: 0 generic, 1 the fused forward kernel, -1 when L == 1;
 *         their k-chunks per output tile (0 when L == 1)} */
#define NCX_QUERY_FWD_ROUTE 34
/* Not a GEMM id either: the kernels the bf16 variant (NCX_F_BF16) launches for these dims, as launched (experiment hooks applied; read
 * from the one function its launchers call).  Without the flag out6 = {-1, 0, 0, 0, 0, 0}.
 * out6 = {h_1 = Xc . Wc^T: gemm_bf16_nt_kernel on 0 128x128, 1 64x128, 2 128x64, 3 64x64 tiles, or 8 gemm_bf16_nt8_kernel (192x256);
 *         dWc = dpre_1^T . Xc: 1 gemm_bf16_tn8_kernel (256x128 tiles), 0 gemm_bf16_tn_kernel (128x128);
 *         the k-chunks of that launch's grid; the rows per k-chunk; the chunks that hold rows (= the slabs the reduction sums);
 *         bits 1 / 2 / 4 / 8: the 4-columns-per-thread form of k_dpre_to_bf16 / of k_pack2d on E / on [W1ak; W1agt] / on [dGt; dGgt] --
 *         the part of that choice the SHAPE decides; the launchers also require 16-byte aligned pointers, which a workspace region
 *         always is and a caller's weight tensor need not be} */
#define NCX_QUERY_BF16_ROUTE 35
/* Not a GEMM id either: Gt and Sh, the two short products in front of linear_1, as ONE launch of the fused forward kernel's 64 x 64 form with
 * one fix-up behind it (fp32 path with the a_emb segment, widths multiples of 4, no NCX_F_REUSE_GT, no side stream, a joint plan that splits at
 * least one of the two; hook NCX_NO_GTSH_PAIR: off).
 * out6 = {1 when ncx_forward takes that launch for these dims, else 0 (the two launches of the generic engine);
 *         the k-chunks per 64 x 64 tile of Gt and of Sh: those of the two launches (ncx_plan_query NCX_GEMM_GT / NCX_GEMM_SH), so that the
 *         results are theirs bit for bit;
 *         the workgroups that share a tile's chunks, for Gt and for Sh (divisors of the chunk counts: a workgroup runs chunks / workgroups
 *         consecutive chunks; 0, 0: no joint plan); the workgroup slots of one round (3 per CU)} */
#define NCX_QUERY_GTSH_PAIR 36
int ncx_profile_begin(uint32_t gemm_mask /* bit i = gemm id i */, int32_t max_launches);
int ncx_profile_end(float* ms, int32_t* ids, int32_t cap);
/* In-kernel clock diagnostics of the MAIN launch (the fused forward kernel of linear_1): while `stamps` is non-NULL
 * every fp32 MAIN launch makes thread 0 of each workgroup write 16 uint64 words to stamps[16 * workgroup id ...]:
 * word 0 = shader-cycle counter (s_memtime) at kernel entry, word 8 = the same at exit, words 14 / 15 = the 100 MHz
 * constant-rate counter (s_memrealtime) at entry / exit, word 13 = XCC id.  The clock a workgroup held is
 * (w8 - w0) / (w15 - w14) x 100 MHz.  `words` = capacity of the device buffer in uint64 (>= 16 x workgroups of the
 * launch, else the launch is not stamped).  Armed for the CURRENT device only (the buffer lives there; forwards on other
 * devices of the process never see it); ncx_profile_stamps(NULL, 0) disarms it.  The timed product path never arms it
 * (bench.py stamps a separate diagnostic pass after its timed region). */
int ncx_profile_stamps(unsigned long long* stamps, int64_t words);
/* out6 = {form (0 NT,1 TN,2 NN), M, N, 32-deep k-steps, tile cfg (0 64x64, 1 128x128, 2 96x128, 3 96x64, 4 128x64; the fused forward
 *         kernel: 5 48x128, 6 / 7 / 8 the per-triplet fold on 48x64 / 96x64 / 192x64 tiles), aligned k-chunks per output tile (1 = no split)} */
int ncx_plan_query(const ncx_dims* d, int32_t gemm_id, int32_t* out6);
/* The column layout of the bf16 variant's packed operands (NCX_WS_XC, NCX_WS_WC) and the padded extents of its other bf16 images:
 * out10 = {c_vk, c_vm, c_misc, c_z, c_p: the first column of v_k | v_o * v_k | dist, one-hot rank | z_k | softmax(a_k) (weights: of the
 *          matching W1 slices and Gt), each a multiple of 8, the gaps zero; raw: one past the last used column; kc: the row length (raw
 *          rounded up to 128, zero beyond raw); Hp: rows of Wc and columns of the bf16 dpre_1 image (H rounded up to 128); dap, Ap: da and A
 *          rounded up to 128}.  Defined for any valid dims, with or without NCX_F_BF16. */
int ncx_bf16_layout(const ncx_dims* d, int32_t* out10);
/* Host-only self-check of the workgroup-id <-> (tile, k-chunk) maps (XCD-aware interleaved layout, chunk-per-XCD
 * layout with its padding ids): 0 when decode/encode are mutually inverse and cover every (tile, chunk) exactly once. */
int ncx_wgmap_check(int32_t tiles_m, int32_t tiles_n, int32_t S);

/* The generic segmented GEMM engine (csrc/ncx_gemm.h) called directly, for tests: one launch through the driver every caller in the
 * library uses, with the tile config, the mode and the k-split given instead of planned.  Forms: 0 NT  C = sum_p A_p[M, k] . B_p[N, k]^T,
 * 1 TN  C = A[k, M]^T . B[k, N], 2 NN  C = A[M, k] . B[k, N].  Operand kinds: 0 plain x(r, c) = base[r ld + c]; 1 gather
 * base[idx[r idx_stride] ld + c]; 2 gather-mul base[idx[..] ld + c] * base[idx2[..] ld + c]; 3 softmax exp2(base[r ld + c] log2(e) - lse2[r]).
 * mode 0: a CHAIN of nseg (a, b, klen) pairs summed into out[0] ([M, n_cols[0]], split[0] k-chunks); mode 1: a GROUP of nseg problems
 * that share M, each with its own operands, n_cols, split, out and ldo.  fold != 0: the FOLD kernel (NT chain on 64 x 64 tiles): after
 * pair s, z += (acc + fold_bias[s N + n]) * fold_mul[(r / fold_div) ld_fold + s N + n]; the output is z.
 * Epilogue, in this order: + rowadd[(r / rowdiv) ld_rowadd + n]; + bias[n]; act (0 none, 1 relu, 2 tanh); dropout (0 none, 1 the
 * counter-based generator on index r n_cols + n, 2 keep_mask[r ld_mask + n] != 0) times drop_scale; gate[r ld_gate + n] > 0 ? times
 * gate_scale : 0.  rowsplit_g = g > 0: row r = g b + j goes to out0[b ldo0 + n] when j == 0, else to out[((g - 1) b + j - 1) ldo + n].
 * split > 1 puts partial tiles in `slab` (ncx_diag_gemm_slab_bytes; NCX_E_WORKSPACE when slab_bytes is short) and a fix-up kernel sums
 * them and applies bias and act.  no_fast != 0: the generic k-loop only (what the hook NCX_NO_FAST selects).  The entry writes a->grid.
 * NCX_E_DIMS, before any launch, for what the engine does not implement: a cfg the form has no instantiation for (NT 0 1 2 3, TN 0 1 4,
 * NN 0 1); an operand with cols < 4; klen or M or n_cols disagreeing with the operands' extents; ld < cols; nseg outside
 * 1 .. NCX_DIAG_MAX_SEG; a kind, form, mode, act or dropout code out of range; split > 1 together with rowadd, dropout, gate, rowsplit_g
 * or fold; fold outside an NT chain on cfg 0; rowdiv / fold_div < 1 where used.  NCX_E_NULL: a pointer the description needs is NULL.
 * Indices are not clamped: every idx entry must name a row of its table. */
#define NCX_DIAG_MAX_SEG 10
typedef struct ncx_diag_operand {
    const float* base; const int32_t* idx; const int32_t* idx2; const float* lse2;
    int64_t ld;
    int32_t kind, rows, cols, idx_stride;
} ncx_diag_operand;
typedef struct ncx_diag_gemm_args {
    int32_t form, cfg, mode, nseg, M, fold, no_fast;
    int32_t grid;                /* out: workgroups the GEMM launch was given (fewer than its work items under the persistent loop) */
    ncx_diag_operand a[NCX_DIAG_MAX_SEG], b[NCX_DIAG_MAX_SEG];
    int32_t klen[NCX_DIAG_MAX_SEG], n_cols[NCX_DIAG_MAX_SEG], split[NCX_DIAG_MAX_SEG];
    float* out[NCX_DIAG_MAX_SEG];
    int64_t ldo[NCX_DIAG_MAX_SEG];
    const float* rowadd; int64_t ld_rowadd; int32_t rowdiv; int32_t act;
    const float* bias;
    int32_t dropout; float drop_p, drop_scale; uint32_t seed_lo, seed_hi, layer;
    const float* keep_mask; int64_t ld_mask;
    const float* gate; int64_t ld_gate; float gate_scale; int32_t fold_div;
    const float* fold_mul; const float* fold_bias; int64_t ld_fold;
    int32_t rowsplit_g; int32_t pad2_; float* out0; int64_t ldo0;
    float* slab; size_t slab_bytes;
} ncx_diag_gemm_args;
int ncx_diag_gemm(ncx_diag_gemm_args* a, void* stream);
/* Bytes of the split-K slab that launch needs (0: unsplit, or the arguments are ones ncx_diag_gemm rejects). */
size_t ncx_diag_gemm_slab_bytes(const ncx_diag_gemm_args* a);
/* 1 when the form instantiates the tile config, else 0 (the predicate ncx_diag_gemm and the NCX_CFG_<id> hook ask). */
int ncx_diag_cfg_supported(int32_t form, int32_t cfg);
/* plan_gemm, the planner behind every launch on the generic engine that is not placed by hand: out2 = {tile cfg, k-chunks per tile} for
 * an M x N product of `ksteps` 32-deep steps; allow_96: the caller takes the big NT tiles (the forward layers).  Depends on the device's
 * CU count (256 without a device). */
int ncx_diag_plan_gemm(int32_t form, int64_t M, int64_t N, int64_t ksteps, int32_t allow_96, int32_t* out2);

/* Library build id ("neuralcx-hip gfx950 <date>"). */
const char* ncx_version(void);

#ifdef __cplusplus
}
#endif
#endif /* NEURALCX_H */
