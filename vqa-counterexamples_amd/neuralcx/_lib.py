"""ctypes binding of libneuralcx_hip.so (C ABI: include/neuralcx.h).

This is the stub a maintainer of the reference would add: plain pointers and
sizes in, status code out.  There is NO fallback: if the HIP library is missing or fails to load,
importing a symbol raises -- the product path never routes through a CPU implementation.
"""
import ctypes as C
import os

_HERE = os.path.dirname(os.path.abspath(__file__))
LIB_PATH = os.environ.get("NCX_LIB") or os.path.join(os.path.dirname(_HERE), "lib", "libneuralcx_hip.so")   # (NCX_LIB: A/B builds, tools/)

NCX_F_V_MULT, NCX_F_V_DIST, NCX_F_V_RANK, NCX_F_A_EMB = 1, 2, 4, 8
NCX_F_ALL = 15
NCX_F_REUSE_GT = 32   # evaluation: Gt in the workspace is still valid (same weights)
NCX_F_FUSED_TAIL = 64  # training: out layer + loss / Recall + head of the backward in one pass (ncx_train_tail)
NCX_F_X6 = 128         # NOT the default: the balanced TN weight-gradient launch on the bf16 matrix path with three-plane (fp32-grade) operands
NCX_F_BF16 = 16       # BASELINE configs[4]: bf16 operands for the two dominant GEMMs (include/neuralcx.h)

EXPORTS = ("ncx_input_size", "ncx_workspace_bytes", "ncx_forward", "ncx_forward_phase", "ncx_loss_rank", "ncx_backward", "ncx_backward_phase",
           "ncx_adam_step", "ncx_backward_adam", "ncx_version", "ncx_profile_begin", "ncx_profile_end", "ncx_plan_query",
           "ncx_vqa_workspace_bytes", "ncx_vqa_forward", "ncx_mlb_workspace_bytes", "ncx_mlb_forward",
           "ncx_vqa_route", "ncx_vqa_ws_region", "ncx_mlb_route", "ncx_mlb_ws_region", "ncx_mlb_att_workspace_bytes", "ncx_mlb_att_forward", "ncx_mlb_att_forward_flags", "ncx_mlb_att_logits_form", "ncx_knn_workspace_bytes", "ncx_knn_status_offset", "ncx_knn", "ncx_cosine_gram_workspace_bytes", "ncx_cosine_gram", "ncx_semantic_scores",
           "ncx_similarity_scores",
           "ncx_gru_packed_bytes", "ncx_gru_pack", "ncx_gru_workspace_bytes", "ncx_gru_encode", "ncx_gru_encode_flags", "ncx_gru_step_form",
           "ncx_gru_train_workspace_bytes", "ncx_gru_packed_t_bytes", "ncx_gru_pack_t", "ncx_gru_train_forward", "ncx_gru_train_forward_flags", "ncx_gru_train_backward",
           "ncx_gru_train_backward_flags", "ncx_gru_bwd_form",
           "ncx_lstm2_packed_bytes", "ncx_lstm2_pack", "ncx_lstm2_workspace_bytes", "ncx_lstm2_encode", "ncx_lstm2_encode_flags", "ncx_lstm2_step_form",
           "ncx_lstm2_train_workspace_bytes", "ncx_lstm2_packed_t_bytes", "ncx_lstm2_pack_t", "ncx_lstm2_train_forward", "ncx_lstm2_train_forward_flags", "ncx_lstm2_train_backward",
           "ncx_ws_region", "ncx_wgmap_check", "ncx_bf16_layout",
           "ncx_comm_unique_id", "ncx_comm_create", "ncx_comm_destroy", "ncx_allreduce", "ncx_train_tail", "ncx_profile_stamps",
           "ncx_pairlin_workspace_bytes", "ncx_pairlin_forward", "ncx_pairlin_backward",
           "ncx_linctx_workspace_bytes", "ncx_linctx_forward", "ncx_linctx_backward",
           "ncx_contrastive_workspace_bytes", "ncx_contrastive_forward", "ncx_contrastive_distances", "ncx_contrastive_loss",
           "ncx_contrastive_backward",
           "ncx_vqa_train_workspace_bytes", "ncx_vqa_train_forward", "ncx_ce_loss", "ncx_vqa_train_backward", "ncx_vqa_train_ws_region",
           "ncx_mlb_train_workspace_bytes", "ncx_mlb_train_forward", "ncx_mlb_train_backward", "ncx_mlb_train_ws_region",
           "ncx_mlb_att_train_workspace_bytes", "ncx_mlb_att_train_forward", "ncx_mlb_att_train_forward_flags", "ncx_mlb_att_train_backward", "ncx_mlb_att_train_ws_region",
           "ncx_mlb_att_train_backward_flags", "ncx_mlb_att_dwv_form",
           "ncx_diag_gemm", "ncx_diag_gemm_slab_bytes", "ncx_diag_cfg_supported", "ncx_diag_plan_gemm")


class NcxDims(C.Structure):
    _fields_ = [("B", C.c_int32), ("K", C.c_int32), ("dv", C.c_int32), ("dq", C.c_int32),
                ("dz", C.c_int32), ("da", C.c_int32), ("A", C.c_int32), ("H", C.c_int32),
                ("L", C.c_int32), ("n_img", C.c_int32), ("flags", C.c_uint32),
                ("training", C.c_int32), ("drop_p", C.c_float), ("loss_scale", C.c_float),
                ("seed", C.c_uint64)]


class NcxInputs(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("feats", "img_idx", "q_emb", "z_orig", "z_knns", "a_knns",
                                           "answer_aids", "a_emb_gt", "v_rank", "keep_mask")]


_PNAMES = ("answer_embedding", "w1", "b1", "w2", "b2", "w3", "b3", "w_out", "b_out")


class NcxParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _PNAMES]


class NcxGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _PNAMES]


class NcxAdamState(C.Structure):             # ncx_adam_state (include/neuralcx.h): the flat buffers of ncx_backward_adam
    _fields_ = [("param", C.c_void_p), ("grad", C.c_void_p), ("exp_avg", C.c_void_p), ("exp_avg_sq", C.c_void_p),
                ("n", C.c_size_t), ("n_emb", C.c_size_t), ("step", C.c_int32),
                ("lr", C.c_float), ("beta1", C.c_float), ("beta2", C.c_float), ("eps", C.c_float), ("grad_scale", C.c_float)]


class NcxMutanParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wv", "bv", "wq", "bq", "whv", "bhv", "whq", "bhq", "wc", "bc")] + \
               [(n, C.c_int32) for n in ("dhv", "dhq", "R", "act_v", "act_q")]


class NcxMutanGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wv", "bv", "wq", "bq", "whv", "bhv", "whq", "bhq", "wc", "bc")]


class NcxVqaTrainDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "dv", "dq", "dz", "A", "n_img")] + [(n, C.c_float) for n in ("p_v", "p_q", "p_c")] + \
               [("dropout_mode", C.c_int32), ("want_dq", C.c_int32), ("pad_", C.c_int32), ("seed", C.c_uint64)]


class NcxMlbParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wv", "bv", "wq", "bq", "wc", "bc")] + \
               [(n, C.c_int32) for n in ("dh", "act_v", "act_q", "act_c")]


class NcxMlbAttDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "P", "dv", "dq", "dh_att", "G", "dh_f", "A", "n_img")]


class NcxMlbAttParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wv_att", "bv_att", "wq_att", "bq_att", "wa", "ba", "wg", "bg", "wqf", "bqf", "wc", "bc")] + \
               [(n, C.c_int32) for n in ("act_v_att", "act_q_att", "act_mm", "act_v", "act_q", "act_c")]


class NcxMlbAttTrain(C.Structure):
    _fields_ = [(n, C.c_float) for n in ("p_att_v", "p_att_q", "p_att_mm", "p_v", "p_q", "p_c")] + \
               [("dropout_mode", C.c_int32), ("want_dq", C.c_int32), ("seed", C.c_uint64)]


class NcxMlbAttGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wv_att", "bv_att", "wq_att", "bq_att", "wa", "ba", "wg", "bg", "wqf", "bqf", "wc", "bc")]


class NcxMlbGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in ("wv", "bv", "wq", "bq", "wc", "bc")]


class NcxScorerDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "K", "dv", "dq", "dz", "A", "n_img")]


class NcxContrastiveDims(C.Structure):
    _fields_ = [(n, C.c_int32) for n in ("B", "P", "dv", "dz", "n_img")]


NCX_DIAG_MAX_SEG = 10


class NcxDiagOperand(C.Structure):           # ncx_diag_operand (include/neuralcx.h)
    _fields_ = [(n, C.c_void_p) for n in ("base", "idx", "idx2", "lse2")] + [("ld", C.c_int64)] + \
               [(n, C.c_int32) for n in ("kind", "rows", "cols", "idx_stride")]


class NcxDiagGemmArgs(C.Structure):          # ncx_diag_gemm_args: one launch of the generic GEMM engine, described field by field
    _fields_ = [(n, C.c_int32) for n in ("form", "cfg", "mode", "nseg", "M", "fold", "no_fast", "grid")] + \
               [("a", NcxDiagOperand * NCX_DIAG_MAX_SEG), ("b", NcxDiagOperand * NCX_DIAG_MAX_SEG)] + \
               [(n, C.c_int32 * NCX_DIAG_MAX_SEG) for n in ("klen", "n_cols", "split")] + \
               [("out", C.c_void_p * NCX_DIAG_MAX_SEG), ("ldo", C.c_int64 * NCX_DIAG_MAX_SEG),
                ("rowadd", C.c_void_p), ("ld_rowadd", C.c_int64), ("rowdiv", C.c_int32), ("act", C.c_int32),
                ("bias", C.c_void_p),
                ("dropout", C.c_int32), ("drop_p", C.c_float), ("drop_scale", C.c_float),
                ("seed_lo", C.c_uint32), ("seed_hi", C.c_uint32), ("layer", C.c_uint32),
                ("keep_mask", C.c_void_p), ("ld_mask", C.c_int64),
                ("gate", C.c_void_p), ("ld_gate", C.c_int64), ("gate_scale", C.c_float), ("fold_div", C.c_int32),
                ("fold_mul", C.c_void_p), ("fold_bias", C.c_void_p), ("ld_fold", C.c_int64),
                ("rowsplit_g", C.c_int32), ("pad2_", C.c_int32), ("out0", C.c_void_p), ("ldo0", C.c_int64),
                ("slab", C.c_void_p), ("slab_bytes", C.c_size_t)]


_PL_NAMES = ("answer_embedding", "w", "b", "w_out", "b_out")


class NcxPairlinParams(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _PL_NAMES]


class NcxPairlinGrads(C.Structure):
    _fields_ = [(n, C.c_void_p) for n in _PL_NAMES]


class NcxError(RuntimeError):
    pass


_ERR = {-1: "NCX_E_NULL (required pointer is NULL)", -2: "NCX_E_DIMS (dimension out of range)",
        -3: "NCX_E_WORKSPACE (workspace too small or misaligned)", -4: "NCX_E_FLAGS (inconsistent lesion inputs)",
        -5: "NCX_E_UNSUPPORTED (RCCL could not be loaded)", -6: "NCX_E_COMM (RCCL reported an error)"}

_lib = None


def lib():
    """The loaded library; raises with a build hint when it is absent (never falls back)."""
    global _lib
    if _lib is not None:
        return _lib
    if not os.path.exists(LIB_PATH):
        raise NcxError("HIP library not built: %s is missing. Run `python -c 'import __graft_entry__ as g; "
                       "g.build()'` or `make -C vqa-counterexamples_amd`." % LIB_PATH)
    # The library shares the process's HIP runtime with PyTorch (streams and device pointers cross the boundary), and
    # PyTorch-ROCm ships its own libamdhip64: import torch FIRST so that the dynamic linker resolves this library's
    # libamdhip64.so.7 to the copy torch already loaded.  Loaded the other way round, the process ends up with two HIP
    # runtimes and every launch on a torch stream fails with hipErrorNoDevice.
    import torch  # noqa: F401
    L = C.CDLL(LIB_PATH)
    L.ncx_version.restype = C.c_char_p
    L.ncx_input_size.restype = C.c_int64
    L.ncx_input_size.argtypes = [C.POINTER(NcxDims)]
    L.ncx_workspace_bytes.restype = C.c_size_t
    L.ncx_workspace_bytes.argtypes = [C.POINTER(NcxDims)]
    L.ncx_forward.restype = C.c_int
    L.ncx_forward.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxInputs), C.POINTER(NcxParams), C.c_void_p,
                              C.c_size_t, C.c_void_p, C.c_void_p]
    L.ncx_forward_phase.restype = C.c_int
    L.ncx_forward_phase.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxInputs), C.POINTER(NcxParams), C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.c_int32, C.c_void_p]
    L.ncx_loss_rank.restype = C.c_int
    L.ncx_loss_rank.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float, C.c_void_p,
                                C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_backward.restype = C.c_int
    L.ncx_backward.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxInputs), C.POINTER(NcxParams), C.c_void_p,
                               C.c_size_t, C.c_void_p, C.POINTER(NcxGrads), C.c_void_p]
    L.ncx_backward_phase.restype = C.c_int
    L.ncx_backward_phase.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxInputs), C.POINTER(NcxParams), C.c_void_p,
                                     C.c_size_t, C.c_void_p, C.POINTER(NcxGrads), C.c_int32, C.c_void_p]
    L.ncx_adam_step.restype = C.c_int
    L.ncx_adam_step.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_float,
                                C.c_float, C.c_float, C.c_float, C.c_int32, C.c_float, C.c_void_p]
    L.ncx_backward_adam.restype = C.c_int
    L.ncx_backward_adam.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxInputs), C.POINTER(NcxParams), C.c_void_p,
                                    C.c_size_t, C.c_void_p, C.POINTER(NcxGrads), C.POINTER(NcxAdamState), C.c_void_p]
    L.ncx_vqa_workspace_bytes.restype = C.c_size_t
    L.ncx_vqa_workspace_bytes.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxMutanParams)]
    L.ncx_vqa_forward.restype = C.c_int
    L.ncx_vqa_forward.argtypes = [C.POINTER(NcxDims), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcxMutanParams), C.c_void_p,
                                  C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_mlb_workspace_bytes.restype = C.c_size_t
    L.ncx_mlb_workspace_bytes.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxMlbParams)]
    L.ncx_mlb_forward.restype = C.c_int
    L.ncx_mlb_forward.argtypes = [C.POINTER(NcxDims), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcxMlbParams), C.c_void_p,
                                  C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    for name, P_M in (("vqa", C.POINTER(NcxMutanParams)), ("mlb", C.POINTER(NcxMlbParams))):
        route, region = getattr(L, "ncx_%s_route" % name), getattr(L, "ncx_%s_ws_region" % name)
        route.restype = region.restype = C.c_int
        route.argtypes = [C.POINTER(NcxDims), P_M, C.POINTER(C.c_int32)]
        region.argtypes = [C.POINTER(NcxDims), P_M, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ncx_mlb_att_workspace_bytes.restype = C.c_size_t
    L.ncx_mlb_att_workspace_bytes.argtypes = [C.POINTER(NcxMlbAttDims), C.POINTER(NcxMlbAttParams)]
    L.ncx_mlb_att_forward.restype = C.c_int
    L.ncx_mlb_att_forward.argtypes = [C.POINTER(NcxMlbAttDims), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcxMlbAttParams), C.c_void_p,
                                      C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_mlb_att_forward_flags.restype = C.c_int
    L.ncx_mlb_att_forward_flags.argtypes = [C.POINTER(NcxMlbAttDims), C.c_void_p, C.c_void_p, C.c_void_p, C.POINTER(NcxMlbAttParams), C.c_uint32,
                                            C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_mlb_att_logits_form.restype = C.c_int
    L.ncx_mlb_att_logits_form.argtypes = [C.POINTER(NcxMlbAttDims), C.c_uint32]
    L.ncx_knn_workspace_bytes.restype = C.c_size_t
    L.ncx_knn_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.ncx_knn_status_offset.restype = C.c_size_t
    L.ncx_knn_status_offset.argtypes = [C.c_int32]
    L.ncx_knn.restype = C.c_int
    L.ncx_knn.argtypes = [C.c_void_p, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_void_p,
                          C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_cosine_gram_workspace_bytes.restype = C.c_size_t
    L.ncx_cosine_gram_workspace_bytes.argtypes = [C.c_int32, C.c_int32]
    L.ncx_cosine_gram.restype = C.c_int
    L.ncx_cosine_gram.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ncx_semantic_scores.restype = C.c_int
    L.ncx_semantic_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_float,
                                      C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_similarity_scores.restype = C.c_int
    L.ncx_similarity_scores.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_int32, C.c_void_p,
                                        C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_gru_packed_bytes.restype = C.c_size_t
    L.ncx_gru_packed_bytes.argtypes = [C.c_int32, C.c_int32]
    L.ncx_gru_pack.restype = C.c_int
    L.ncx_gru_pack.argtypes = [C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.ncx_gru_workspace_bytes.restype = C.c_size_t
    L.ncx_gru_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.ncx_gru_encode.restype = C.c_int
    L.ncx_gru_encode.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                 C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_gru_encode_flags.restype = C.c_int
    L.ncx_gru_encode_flags.argtypes = L.ncx_gru_encode.argtypes[:8] + [C.c_uint32] + L.ncx_gru_encode.argtypes[8:]
    L.ncx_gru_step_form.restype = C.c_int
    L.ncx_gru_step_form.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    L.ncx_gru_train_workspace_bytes.restype = C.c_size_t
    L.ncx_gru_train_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.ncx_gru_packed_t_bytes.restype = C.c_size_t
    L.ncx_gru_packed_t_bytes.argtypes = [C.c_int32, C.c_int32]
    L.ncx_gru_pack_t.restype = C.c_int
    L.ncx_gru_pack_t.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.ncx_gru_train_forward.restype = C.c_int
    L.ncx_gru_train_forward.argtypes = L.ncx_gru_encode.argtypes
    L.ncx_gru_train_forward_flags.restype = C.c_int
    L.ncx_gru_train_forward_flags.argtypes = L.ncx_gru_encode_flags.argtypes
    L.ncx_gru_train_backward.restype = C.c_int
    L.ncx_gru_train_backward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                         C.c_size_t] + [C.c_void_p] * 7
    L.ncx_gru_train_backward_flags.restype = C.c_int
    L.ncx_gru_train_backward_flags.argtypes = L.ncx_gru_train_backward.argtypes[:8] + [C.c_uint32] + L.ncx_gru_train_backward.argtypes[8:]
    L.ncx_gru_bwd_form.restype = C.c_int
    L.ncx_gru_bwd_form.argtypes = L.ncx_gru_step_form.argtypes
    L.ncx_lstm2_packed_bytes.restype = C.c_size_t
    L.ncx_lstm2_packed_bytes.argtypes = [C.c_int32, C.c_int32]
    L.ncx_lstm2_pack.restype = C.c_int
    L.ncx_lstm2_pack.argtypes = [C.c_void_p] * 8 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.ncx_lstm2_workspace_bytes.restype = C.c_size_t
    L.ncx_lstm2_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.ncx_lstm2_encode.restype = C.c_int
    L.ncx_lstm2_encode.argtypes = L.ncx_gru_encode.argtypes
    L.ncx_lstm2_encode_flags.restype = C.c_int
    L.ncx_lstm2_encode_flags.argtypes = L.ncx_gru_encode_flags.argtypes
    L.ncx_lstm2_step_form.restype = C.c_int
    L.ncx_lstm2_step_form.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32, C.c_uint32]
    L.ncx_lstm2_train_workspace_bytes.restype = C.c_size_t
    L.ncx_lstm2_train_workspace_bytes.argtypes = [C.c_int32, C.c_int32, C.c_int32, C.c_int32]
    L.ncx_lstm2_packed_t_bytes.restype = C.c_size_t
    L.ncx_lstm2_packed_t_bytes.argtypes = [C.c_int32, C.c_int32]
    L.ncx_lstm2_pack_t.restype = C.c_int
    L.ncx_lstm2_pack_t.argtypes = [C.c_void_p] * 4 + [C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    L.ncx_lstm2_train_forward.restype = C.c_int
    L.ncx_lstm2_train_forward.argtypes = L.ncx_gru_encode.argtypes
    L.ncx_lstm2_train_forward_flags.restype = C.c_int
    L.ncx_lstm2_train_forward_flags.argtypes = L.ncx_gru_encode_flags.argtypes
    L.ncx_lstm2_train_backward.restype = C.c_int
    L.ncx_lstm2_train_backward.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_int32, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p,
                                           C.c_size_t] + [C.c_void_p] * 11
    L.ncx_ws_region.restype = C.c_int
    L.ncx_ws_region.argtypes = [C.POINTER(NcxDims), C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ncx_profile_begin.restype = C.c_int
    L.ncx_profile_begin.argtypes = [C.c_uint32, C.c_int32]
    L.ncx_profile_end.restype = C.c_int
    L.ncx_profile_end.argtypes = [C.POINTER(C.c_float), C.POINTER(C.c_int32), C.c_int32]
    L.ncx_profile_stamps.restype = C.c_int
    L.ncx_profile_stamps.argtypes = [C.c_void_p, C.c_int64]
    L.ncx_train_tail.restype = C.c_int
    L.ncx_train_tail.argtypes = [C.POINTER(NcxDims), C.POINTER(NcxParams), C.c_void_p, C.c_size_t] + [C.c_void_p] * 7 + [C.POINTER(NcxGrads), C.c_void_p]
    L.ncx_comm_unique_id.restype = C.c_int; L.ncx_comm_unique_id.argtypes = [C.c_void_p]
    L.ncx_comm_create.restype = C.c_int; L.ncx_comm_create.argtypes = [C.c_void_p, C.c_int32, C.c_int32, C.POINTER(C.c_void_p)]
    L.ncx_comm_destroy.restype = C.c_int; L.ncx_comm_destroy.argtypes = [C.c_void_p]
    L.ncx_allreduce.restype = C.c_int; L.ncx_allreduce.argtypes = [C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p]
    L.ncx_bf16_layout.restype = C.c_int
    L.ncx_bf16_layout.argtypes = [C.POINTER(NcxDims), C.POINTER(C.c_int32)]
    L.ncx_plan_query.restype = C.c_int
    L.ncx_plan_query.argtypes = [C.POINTER(NcxDims), C.c_int32, C.POINTER(C.c_int32)]
    P_SD = C.POINTER(NcxScorerDims)
    L.ncx_pairlin_workspace_bytes.restype = C.c_size_t
    L.ncx_pairlin_workspace_bytes.argtypes = [P_SD]
    L.ncx_pairlin_forward.restype = C.c_int
    L.ncx_pairlin_forward.argtypes = [P_SD, C.POINTER(NcxInputs), C.POINTER(NcxPairlinParams), C.c_void_p, C.c_size_t,
                                      C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_pairlin_backward.restype = C.c_int
    L.ncx_pairlin_backward.argtypes = [P_SD, C.POINTER(NcxInputs), C.POINTER(NcxPairlinParams), C.c_void_p, C.c_size_t,
                                       C.c_void_p, C.POINTER(NcxPairlinGrads), C.c_void_p]
    L.ncx_linctx_workspace_bytes.restype = C.c_size_t
    L.ncx_linctx_workspace_bytes.argtypes = [P_SD]
    L.ncx_linctx_forward.restype = C.c_int
    L.ncx_linctx_forward.argtypes = [P_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ncx_linctx_backward.restype = C.c_int
    L.ncx_linctx_backward.argtypes = [P_SD, C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    P_CD = C.POINTER(NcxContrastiveDims)
    L.ncx_contrastive_workspace_bytes.restype = C.c_size_t
    L.ncx_contrastive_workspace_bytes.argtypes = [P_CD]
    L.ncx_contrastive_forward.restype = C.c_int
    L.ncx_contrastive_forward.argtypes = [P_CD, C.POINTER(NcxInputs), C.c_void_p, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                          C.c_void_p, C.c_void_p]
    L.ncx_contrastive_distances.restype = C.c_int
    L.ncx_contrastive_distances.argtypes = [P_CD, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p]
    L.ncx_contrastive_loss.restype = C.c_int
    L.ncx_contrastive_loss.argtypes = [P_CD, C.c_void_p, C.c_size_t, C.c_float, C.c_float, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_contrastive_backward.restype = C.c_int
    L.ncx_contrastive_backward.argtypes = [P_CD, C.POINTER(NcxInputs), C.c_void_p, C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p,
                                           C.c_void_p]
    P_VT, P_MP = C.POINTER(NcxVqaTrainDims), C.POINTER(NcxMutanParams)
    L.ncx_vqa_train_workspace_bytes.restype = C.c_size_t
    L.ncx_vqa_train_workspace_bytes.argtypes = [P_VT, P_MP]
    L.ncx_vqa_train_forward.restype = C.c_int
    L.ncx_vqa_train_forward.argtypes = [P_VT, C.c_void_p, C.c_void_p, C.c_void_p, P_MP, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.ncx_ce_loss.restype = C.c_int
    L.ncx_ce_loss.argtypes = [C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_float] + [C.c_void_p] * 7
    L.ncx_vqa_train_backward.restype = C.c_int
    L.ncx_vqa_train_backward.argtypes = [P_VT, P_MP, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(NcxMutanGrads), C.c_void_p,
                                         C.c_void_p]
    L.ncx_vqa_train_ws_region.restype = C.c_int
    L.ncx_vqa_train_ws_region.argtypes = [P_VT, P_MP, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    P_LP = C.POINTER(NcxMlbParams)
    L.ncx_mlb_train_workspace_bytes.restype = C.c_size_t
    L.ncx_mlb_train_workspace_bytes.argtypes = [P_VT, P_LP]
    L.ncx_mlb_train_forward.restype = C.c_int
    L.ncx_mlb_train_forward.argtypes = [P_VT, C.c_void_p, C.c_void_p, C.c_void_p, P_LP, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p,
                                        C.c_void_p, C.c_void_p]
    L.ncx_mlb_train_backward.restype = C.c_int
    L.ncx_mlb_train_backward.argtypes = [P_VT, P_LP, C.c_void_p, C.c_void_p, C.c_size_t, C.c_void_p, C.POINTER(NcxMlbGrads), C.c_void_p,
                                         C.c_void_p]
    L.ncx_mlb_train_ws_region.restype = C.c_int
    L.ncx_mlb_train_ws_region.argtypes = [P_VT, P_LP, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    P_AD, P_AT, P_AP = C.POINTER(NcxMlbAttDims), C.POINTER(NcxMlbAttTrain), C.POINTER(NcxMlbAttParams)
    L.ncx_mlb_att_train_workspace_bytes.restype = C.c_size_t
    L.ncx_mlb_att_train_workspace_bytes.argtypes = [P_AD, P_AT, P_AP]
    L.ncx_mlb_att_train_forward.restype = C.c_int
    L.ncx_mlb_att_train_forward.argtypes = [P_AD, P_AT, C.c_void_p, C.c_void_p, C.c_void_p, P_AP, C.c_void_p, C.c_void_p, C.c_size_t,
                                            C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_mlb_att_train_forward_flags.restype = C.c_int
    L.ncx_mlb_att_train_forward_flags.argtypes = [P_AD, P_AT, C.c_void_p, C.c_void_p, C.c_void_p, P_AP, C.c_void_p, C.c_uint32, C.c_void_p,
                                                  C.c_size_t, C.c_void_p, C.c_void_p, C.c_void_p]
    L.ncx_mlb_att_train_backward.restype = C.c_int
    L.ncx_mlb_att_train_backward.argtypes = [P_AD, P_AT, C.c_void_p, C.c_void_p, C.c_void_p, P_AP, C.c_void_p, C.c_void_p, C.c_size_t,
                                             C.c_void_p, C.c_void_p, C.POINTER(NcxMlbAttGrads), C.c_void_p, C.c_void_p]
    L.ncx_mlb_att_train_backward_flags.restype = C.c_int
    L.ncx_mlb_att_train_backward_flags.argtypes = [P_AD, P_AT, C.c_void_p, C.c_void_p, C.c_void_p, P_AP, C.c_void_p, C.c_uint32, C.c_void_p,
                                                   C.c_size_t, C.c_void_p, C.c_void_p, C.POINTER(NcxMlbAttGrads), C.c_void_p, C.c_void_p]
    L.ncx_mlb_att_dwv_form.restype = C.c_int
    L.ncx_mlb_att_dwv_form.argtypes = [P_AD, C.c_uint32]
    L.ncx_mlb_att_train_ws_region.restype = C.c_int
    L.ncx_mlb_att_train_ws_region.argtypes = [P_AD, P_AT, P_AP, C.c_int32, C.POINTER(C.c_size_t), C.POINTER(C.c_size_t)]
    L.ncx_diag_gemm.restype = C.c_int
    L.ncx_diag_gemm.argtypes = [C.POINTER(NcxDiagGemmArgs), C.c_void_p]
    L.ncx_diag_gemm_slab_bytes.restype = C.c_size_t
    L.ncx_diag_gemm_slab_bytes.argtypes = [C.POINTER(NcxDiagGemmArgs)]
    L.ncx_diag_cfg_supported.restype = C.c_int
    L.ncx_diag_cfg_supported.argtypes = [C.c_int32, C.c_int32]
    L.ncx_diag_plan_gemm.restype = C.c_int
    L.ncx_diag_plan_gemm.argtypes = [C.c_int32, C.c_int64, C.c_int64, C.c_int64, C.c_int32, C.POINTER(C.c_int32)]
    _lib = L
    return L


def check(rc, what):
    if rc == 0:
        return
    if rc < 0:
        raise NcxError("%s failed: %s" % (what, _ERR.get(rc, rc)))
    raise NcxError("%s failed: hipError_t %d" % (what, rc))


def version():
    return lib().ncx_version().decode()


GEMM_IDS = dict(GT=0, SH=1, MAIN=2, FWD_L=3, DW1C=4, DW1S=5, DE=6, DW1AK=7, DAGT=8, DWL=9, DXL=10)


def profile_begin(names, max_launches=4096):
    mask = 0
    for n in names:
        mask |= 1 << GEMM_IDS[n]
    check(lib().ncx_profile_begin(mask, max_launches), "ncx_profile_begin")


def profile_end(cap=4096):
    """-> {gemm name: [ms, ...]} (synchronises the recorded events)."""
    ms = (C.c_float * cap)()
    ids = (C.c_int32 * cap)()
    n = lib().ncx_profile_end(ms, ids, cap)
    if n < 0:
        check(n, "ncx_profile_end")
    inv = {v: k for k, v in GEMM_IDS.items()}
    out = {}
    for i in range(n):
        out.setdefault(inv[ids[i]], []).append(float(ms[i]))
    return out


def profile_stamps(buf=None):
    """Arm (int64 device tensor, >= 16 words per workgroup of MAIN) or disarm (None) the in-kernel clock stamps of MAIN."""
    if buf is None:
        check(lib().ncx_profile_stamps(None, 0), "ncx_profile_stamps")
    else:
        check(lib().ncx_profile_stamps(C.c_void_p(buf.data_ptr()), buf.numel()), "ncx_profile_stamps")


NCX_QUERY_DW1_ROUTE = 32        # include/neuralcx.h
DW1_FOLD_FORMS = ("none", "k_dw_km8", "k_dw_km_x6", "k_dw_km", "grouped")
DW1_TN_FORMS = ("grouped", "k_dw_tn8", "k_dw_tn8_x6")


NCX_QUERY_FUSED_ADAM = 33       # include/neuralcx.h


NCX_QUERY_FWD_ROUTE = 34        # include/neuralcx.h
FWD_ENGINES = ("generic", "chain", "fold", "bf16")
FWD_CHAIN_FORMS = ("48x128", "96x64", "96x128", "160x128", "64x64")


NCX_QUERY_BF16_ROUTE = 35       # include/neuralcx.h
BF16_NT_FORMS = {0: "128x128", 1: "64x128", 2: "128x64", 3: "64x64", 8: "nt8"}


NCX_QUERY_GTSH_PAIR = 36        # include/neuralcx.h


def bf16_layout(d):
    """ncx_bf16_layout: the column layout of the packed bf16 operands and the padded extents, by name."""
    out = (C.c_int32 * 10)()
    check(lib().ncx_bf16_layout(C.byref(d), out), "ncx_bf16_layout")
    return dict(zip(("c_vk", "c_vm", "c_misc", "c_z", "c_p", "raw", "kc", "Hp", "dap", "Ap"), (int(v) for v in out)))


def plan_query(d, name):
    out = (C.c_int32 * 6)()
    if name == "BF16_ROUTE":
        check(lib().ncx_plan_query(C.byref(d), NCX_QUERY_BF16_ROUTE, out), "ncx_plan_query")
        if out[0] < 0:
            return None
        return dict(nt=out[0], nt_name=BF16_NT_FORMS[out[0]], tn8=bool(out[1]), S=out[2], chunk=out[3], nz=out[4],
                    vec_dpre=bool(out[5] & 1), vec_e=bool(out[5] & 2), vec_w1a=bool(out[5] & 4), vec_dg=bool(out[5] & 8))
    if name == "FWD_ROUTE":
        check(lib().ncx_plan_query(C.byref(d), NCX_QUERY_FWD_ROUTE, out), "ncx_plan_query")
        return dict(engine=out[0], engine_name=FWD_ENGINES[out[0]], tile=out[1],
                    tile_name=FWD_CHAIN_FORMS[out[1]] if out[0] == 1 else ("%dx64" % out[1] if out[0] == 2 else None),
                    split=out[2], dist_in_main=bool(out[3]), hidden_engine=out[4], hidden_split=out[5])
    if name == "GTSH_PAIR":
        check(lib().ncx_plan_query(C.byref(d), NCX_QUERY_GTSH_PAIR, out), "ncx_plan_query")
        return dict(taken=bool(out[0]), s_gt=out[1], s_sh=out[2], w_gt=out[3], w_sh=out[4], slots=out[5])
    if name == "FUSED_ADAM":
        check(lib().ncx_plan_query(C.byref(d), NCX_QUERY_FUSED_ADAM, out), "ncx_plan_query")
        return dict(fused=bool(out[0]), passengers=out[1])
    if name == "DW1_ROUTE":
        check(lib().ncx_plan_query(C.byref(d), NCX_QUERY_DW1_ROUTE, out), "ncx_plan_query")
        return dict(fold=DW1_FOLD_FORMS[out[0]], tn=DW1_TN_FORMS[out[1]], tn_pieces=out[2], tn_grid=out[3],
                    a_other_on_tn=bool(out[4]), tn_max_pieces=out[5])
    check(lib().ncx_plan_query(C.byref(d), GEMM_IDS[name], out), "ncx_plan_query")
    return dict(form=("NT", "TN", "NN")[out[0]], M=out[1], N=out[2], ksteps=out[3],
                tile=("64x64", "128x128", "96x128", "96x64", "128x64", "48x128", "48x64 (per-triplet fold of the two v segments)",
                      "96x64 (per-triplet fold of the two v segments, four triplets per workgroup)",
                      "192x64 (per-triplet fold of the two v segments, eight triplets per 8-wave workgroup, one workgroup per CU)")[out[4]], ksplit=out[5])


NCX_VQA_WS = dict(xq=1, hq=2, xv=3)                          # include/neuralcx.h: NCX_VQA_WS_*
NCX_MLB_WS = dict(xq=1, t_knns=2, t_orig=3, xv=4)            # NCX_MLB_WS_*


def vqa_route(d, m):
    """ncx_vqa_route: what ncx_vqa_forward launches for the dims and ncx_mutan_params (host only)."""
    out = (C.c_int32 * 4)()
    check(lib().ncx_vqa_route(C.byref(d), C.byref(m), out), "ncx_vqa_route")
    return dict(main_v=bool(out[0]), fold_kernel=bool(out[1]), classifier=("generic", "main", "main_padded")[out[2]],
                v_tile=FWD_CHAIN_FORMS[out[3]] if out[3] >= 0 else None)


def mlb_route(d, m):
    """ncx_mlb_route: what ncx_mlb_forward launches for the dims and ncx_mlb_params (host only)."""
    out = (C.c_int32 * 4)()
    check(lib().ncx_mlb_route(C.byref(d), C.byref(m), out), "ncx_mlb_route")
    return dict(main_v=bool(out[0]), v_tile=FWD_CHAIN_FORMS[out[1]] if out[1] >= 0 else None,
                classifier=("generic", "main", "main_padded")[out[2]], t_stored=bool(out[3]))


# ---- the C ABI's RCCL handle (include/neuralcx.h: ncx_comm_*, ncx_allreduce) ---------------------------------------------
# The engine exchanges gradients through torch.distributed (backend "nccl" = RCCL); these wrappers are the same collective
# for a host that binds the C ABI without torch.distributed, and what the GPU test drives.
def comm_unique_id() -> bytes:
    buf = C.create_string_buffer(128)
    check(lib().ncx_comm_unique_id(buf), "ncx_comm_unique_id")
    return buf.raw


def comm_create(unique_id: bytes, nranks: int, rank: int) -> C.c_void_p:
    """Binds the CURRENT device (torch.cuda.set_device first).  Collective: every rank calls it with the same id."""
    if len(unique_id) != 128:
        raise ValueError("unique id must be the 128 bytes ncx_comm_unique_id produced on rank 0")
    comm = C.c_void_p()
    check(lib().ncx_comm_create(C.create_string_buffer(unique_id, 128), int(nranks), int(rank), C.byref(comm)), "ncx_comm_create")
    return comm


def allreduce(comm: C.c_void_p, t, stream_ptr=None) -> None:
    """In-place fp32 sum over the ranks of `comm`, ordered on the given HIP stream (default: torch's current stream)."""
    import torch
    if t.dtype != torch.float32 or not t.is_contiguous() or not t.is_cuda:
        raise TypeError("ncx_allreduce takes a contiguous fp32 device tensor")
    sp = torch.cuda.current_stream(t.device).cuda_stream if stream_ptr is None else stream_ptr
    check(lib().ncx_allreduce(comm, C.c_void_p(t.data_ptr()), t.numel(), C.c_void_p(sp)), "ncx_allreduce")


def comm_destroy(comm: C.c_void_p) -> None:
    check(lib().ncx_comm_destroy(comm), "ncx_comm_destroy")

