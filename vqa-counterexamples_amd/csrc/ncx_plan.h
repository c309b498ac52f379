// ncx_plan.h -- the planner of one step (ncx_plan.hip): what forward, backward, the workspace size and the plan query agree on.
#pragma once
#include "ncx_internal.h"

#pragma GCC visibility push(hidden)
namespace ncx {
constexpr int NCX_SCATTER_MAX_B = 32768;     // k_scatter_dsh_by_answer / k_emb_prep keep one bit per triplet in LDS
constexpr int NCX_PERM_MAX_A = 32768;        // k_emb_prep keeps one bit per answer in LDS while it builds the presence permutation
int check_dims(const ncx_dims* d);

// The route decisions of a step that more than one site needs, taken ONCE from the predicates of the kernels that own them
// (ncx_dwkm.hip, ncx_dwtn.hip): list_uses, ws_layout, forward_impl, ncx_train_tail, backward_impl, ncx_ws_region and
// ncx_plan_query read this struct and never ask the predicates themselves, so they cannot disagree.
struct StepRoutes {
    bool km;                // d linear_1.weight[:, v_other | v_mult] on the per-triplet fold (ncx_dwkm.hip); never in the bf16 variant
    int km_form;            // ... the DwKmForm code NCX_QUERY_DW1_ROUTE reports (KM_FORM_GROUPED: the generic engine's grouped launch)
    bool tn8;               // dGt + every other column block of dW1 on the balanced TN launch (ncx_dwtn.hip); fp32 path
    bool tn8_shared;        // the per-triplet shared segments take that kernel (bf16 variant: on a launch of their own)
    bool tn8_x6;            // ... on the bf16 matrix path with three-plane operands (NCX_F_X6)
    bool emb_nt;            // the answer-embedding gradient runs in NT form (operands dGt^T | dGgt^T, ncx_main.h)
    bool de_skip;           // ... over permuted rows, the row tiles without an answer of the batch stopping after the dGt^T segment (one-call backward and phase 1)
    long long cand_ksteps;  // k-steps of linear_1's candidate chain: v_other (| v_mult) | dist, rank | z_other | softmax(a) or a_other
    // dW1[:, a_other] = dGt . E on the balanced TN kernel (not with the side stream: the kernel's slab is the main stream's)
    bool dw1ak_on_tn8(bool side) const { return tn8 && emb_nt && !side; }
    // Gt and Sh as one launch of the fused forward kernel's 64 x 64 form (main_forward_pair).  pair_ok: what the shape, the variant and the hook
    // decide -- the workspace is sized by it, with or without NCX_F_REUSE_GT (an evaluation pass finds the padded weights where the step left
    // them); pair_s_gt / pair_s_sh: k-chunks per tile (the generic engine's plans); pair_w_gt / pair_w_sh: the joint plan's workgroups per tile
    bool pair_ok; int pair_s_gt, pair_s_sh, pair_w_gt, pair_w_sh;
    bool gtsh_pair(const ncx_dims& d, bool side) const { return pair_ok && !(d.flags & NCX_F_REUSE_GT) && !side; }
};
// The joint plan of the pair (ncx_plan.hip): s_gt / s_sh k-chunks per tile as on the generic engine, shared by w_gt / w_sh workgroups per
// tile such that the workgroups of both problems fill at most one round of the 3 x CUs slots ON EVERY XCD.  w_gt == 0: no plan.
struct PairPlan { int s_gt, s_sh, w_gt, w_sh; long long tiles_gt, tiles_sh, t_gt, t_sh, slots; };
PairPlan plan_gtsh_pair(const ncx_dims& d, const StepRoutes& r);
// padded copies of the weight sides of the pair whose width is not a multiple of 32 (ncx_main.h reads whole k-steps): slot 0 .. 3 the W1 slices
// v_orig, q_emb, z_orig, a_gt ([H] rows), 4 answer_embedding ([A] rows); 0: used in place
constexpr int PAIR_WPAD_N = 5;
int pair_wpad_width(const ncx_dims& d, const StepRoutes& r, int i);
StepRoutes routes(const ncx_dims& d);
// linear_1 on the fused forward kernel (ncx_forward.hip), with the experiment hooks applied: the two v segments as one pass with the
// per-triplet fold, and the pairwise distance computed by that kernel.  forward_impl launches by it, NCX_QUERY_FWD_ROUTE reports it.
struct FwdRoute { bool vfold, dist_in_fold, dist_in_main; };
FwdRoute forward_route(const ncx_dims& d, const StepRoutes& r);

// The GEMMs of one step, so that ws_layout and forward/backward agree on split-K slab sizes.
struct GemmUse { int form; long long M, N, ksteps; bool allow96; GemmPlan plan; long long slab_elems; long long tiles; long long wgs; };
enum { U_GT = 0, U_SH, U_MAIN, U_FWD_L, U_DW1C, U_DW1S, U_DE, U_DW1AK, U_DAGT, U_DWL, U_DXL, U_COUNT };
void list_uses(const ncx_dims& d, const StepRoutes& r, GemmUse* u);
int dw1c_seg_split(long long cols, int S, long long ksteps);
WsLayout ws_layout(const ncx_dims& d, const StepRoutes& r);

constexpr int WPAD_N = 7;                    // padded weight copies of the fused forward kernel (slots: ncx_plan.hip)
int wpad_cols(const ncx_dims& d, int i);
int wpad_width(const ncx_dims& d, int i);
}  // namespace ncx
#pragma GCC visibility pop
