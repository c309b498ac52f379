"""Host-side operators over the C ABI: torch tensors in, HIP kernels enqueued on torch's current stream.

PyTorch is plumbing here (device memory, streams, autograd bookkeeping); every arithmetic step of the
hot path runs in libneuralcx_hip.so.  Reference surface these mirror:

  neuralcx_forward / NeuralCXFunction   vqa/models/cx.py:279-333 (NeuralModel.forward below vqa_forward)
  ranking_loss                           counterexamples.py:310,334 + recallAtK (counterexamples.py:501-506)
  adam_step                              torch.optim.Adam as used at counterexamples.py:275-276,339
  cosine_gram / semantic_scores          SemanticBaseline.set_answer_embedding / forward (vqa/models/cx.py:174-175,182-209)
  similarity_scores                      SimilarityModel.forward (vqa/models/cx.py:496-518)
  pairlin_* / linctx_*                   PairwiseLinearModel / LinearContext forward and loss.backward() (cx.py:139-156,379-425)
  contrastive_*                          ContrastiveModel.forward / get_scores, ContrastiveLoss and loss.backward()
                                         (cx.py:428-487, contrastive.py:217-223,293-309)
"""
import ctypes as C
from dataclasses import dataclass
from typing import Dict, Optional

import torch

import os

from . import _lib
from ._lib import (NCX_F_A_EMB, NCX_F_ALL, NCX_F_V_DIST, NCX_F_V_MULT, NCX_F_V_RANK, NcxDims, NcxGrads,
                   NcxInputs, NcxMlbParams, NcxMutanParams, NcxParams)

PARAM_FIELDS = ("answer_embedding", "w1", "b1", "w2", "b2", "w3", "b3", "w_out", "b_out")
# state_dict names of the reference (vqa/models/cx.py:240-257) -> C ABI field
STATE_TO_FIELD = {"answer_embedding.weight": "answer_embedding", "linear_1.weight": "w1", "linear_1.bias": "b1",
                  "linear_2.weight": "w2", "linear_2.bias": "b2", "linear_3.weight": "w3", "linear_3.bias": "b3",
                  "out.weight": "w_out", "out.bias": "b_out"}


def flags_from_spec(spec: Optional[dict]) -> int:
    """model_spec lesion switches (cx.py:265-307) -> NCX_F_* bits handled inside the kernels."""
    if spec is None:
        return NCX_F_ALL
    f = 0
    if spec.get("v_mult", True): f |= NCX_F_V_MULT
    if spec.get("v_dist", True): f |= NCX_F_V_DIST
    if spec.get("v_rank", True): f |= NCX_F_V_RANK
    if spec.get("a_emb", True): f |= NCX_F_A_EMB
    return f


def _stream():
    return C.c_void_p(torch.cuda.current_stream().cuda_stream)


def _ptr(t: Optional[torch.Tensor], dtype, name):
    if t is None:
        return None
    if not t.is_cuda:
        raise _lib.NcxError("%s must be a device tensor (the HIP path has no CPU fallback)" % name)
    if t.dtype != dtype or not t.is_contiguous():
        raise _lib.NcxError("%s must be contiguous %s, got %s%s" % (name, dtype, t.dtype, "" if t.is_contiguous() else " (strided)"))
    return C.c_void_p(t.data_ptr())


@dataclass
class Batch:
    """Device-resident inputs of one forward (ncx_inputs).  int32 indices, fp32 everything else."""
    feats: torch.Tensor            # [n_img, dv]
    img_idx: torch.Tensor          # [B, K+1] int32
    q_emb: torch.Tensor            # [B, dq]
    z_orig: torch.Tensor           # [B, dz]
    z_knns: torch.Tensor           # [B, K, dz]
    a_knns: torch.Tensor           # [B, K, A] logits (or [B, K, da] noise without a_emb)
    answer_aids: Optional[torch.Tensor] = None   # [B] int32
    a_emb_gt: Optional[torch.Tensor] = None      # lesion
    v_rank: Optional[torch.Tensor] = None        # lesion
    keep_mask: Optional[torch.Tensor] = None     # [L, B*K, H] explicit dropout masks (tests)

    @staticmethod
    def from_dense(image_features, q_emb, z_orig, z_knns, a_knns, answer_aids, **kw):
        """The reference hands NeuralModel a gathered [B, K+1, dv] block (counterexamples.py:540-541)."""
        B, K1, dv = image_features.shape
        feats = image_features.reshape(B * K1, dv).contiguous()
        idx = torch.arange(B * K1, device=feats.device, dtype=torch.int32).view(B, K1)
        aids = None if answer_aids is None else answer_aids.to(torch.int32).contiguous()
        return Batch(feats, idx, q_emb.contiguous(), z_orig.contiguous(), z_knns.contiguous(),
                     a_knns.contiguous(), aids, **kw)

    def c_struct(self) -> NcxInputs:
        s = NcxInputs()
        s.feats = _ptr(self.feats, torch.float32, "feats")
        s.img_idx = _ptr(self.img_idx, torch.int32, "img_idx")
        s.q_emb = _ptr(self.q_emb, torch.float32, "q_emb")
        s.z_orig = _ptr(self.z_orig, torch.float32, "z_orig")
        s.z_knns = _ptr(self.z_knns, torch.float32, "z_knns")
        s.a_knns = _ptr(self.a_knns, torch.float32, "a_knns")
        s.answer_aids = _ptr(self.answer_aids, torch.int32, "answer_aids")
        s.a_emb_gt = _ptr(self.a_emb_gt, torch.float32, "a_emb_gt")
        s.v_rank = _ptr(self.v_rank, torch.float32, "v_rank")
        s.keep_mask = _ptr(self.keep_mask, torch.float32, "keep_mask")
        return s


# Flag bits OR-ed into every ncx_dims built here.  NCX_X6=1 in the environment puts the whole process on the split-bf16 ("bf16 x 6") variant
# of the balanced TN weight-gradient launch (include/neuralcx.h: NCX_F_X6; not the default) -- how the unchanged GPU suite is run against it.
# The attention model's forwards read the bit at call time (mlb_att_flags).
EXTRA_FLAGS = _lib.NCX_F_X6 if os.environ.get("NCX_X6", "0") not in ("", "0") else 0


def make_dims(batch: Batch, H: int, L: int, da: int, A: int, flags: int = NCX_F_ALL, training: bool = False,
              drop_p: float = 0.0, loss_scale: float = 0.0, seed: int = 0) -> NcxDims:
    B, K1 = batch.img_idx.shape
    d = NcxDims()
    d.B, d.K = B, K1 - 1
    d.dv, d.dq, d.dz = batch.feats.shape[1], batch.q_emb.shape[1], batch.z_orig.shape[1]
    d.da, d.A, d.H, d.L = da, A, H, L
    d.n_img = batch.feats.shape[0]
    d.flags, d.training, d.drop_p, d.loss_scale, d.seed = flags | EXTRA_FLAGS, int(training), float(drop_p), float(loss_scale), int(seed) & (2 ** 64 - 1)
    # shape validation before any launch (the reference's asserts: cx.py:65,263)
    K = d.K
    assert batch.z_knns.shape == (B, K, d.dz), batch.z_knns.shape
    assert batch.q_emb.shape[0] == B and batch.z_orig.shape == (B, d.dz)
    if flags & NCX_F_A_EMB:
        assert batch.a_knns.shape == (B, K, A), (batch.a_knns.shape, (B, K, A))
        assert batch.answer_aids is not None and batch.answer_aids.shape == (B,)
    else:
        assert batch.a_knns.shape == (B, K, da) and batch.a_emb_gt is not None and batch.a_emb_gt.shape == (B, da)
    if not (flags & NCX_F_V_RANK):
        assert batch.v_rank is not None and batch.v_rank.shape == (B, K, K)
    if batch.keep_mask is not None:
        assert batch.keep_mask.shape == (L, B * K, H)
    return d


def _params_struct(params: Dict[str, torch.Tensor], cls):
    s = cls()
    for f in PARAM_FIELDS:
        setattr(s, f, _ptr(params.get(f), torch.float32, f))
    return s


def workspace_bytes(d: NcxDims) -> int:
    n = _lib.lib().ncx_workspace_bytes(C.byref(d))
    if n == 0:
        raise _lib.NcxError("ncx_workspace_bytes: invalid dims")
    return n


def alloc_workspace(d: NcxDims, device) -> torch.Tensor:
    return torch.empty(workspace_bytes(d) + 256, dtype=torch.uint8, device=device)


def _ws_ptr(ws: torch.Tensor):
    base = ws.data_ptr()
    aligned = (base + 255) // 256 * 256
    return C.c_void_p(aligned), ws.numel() - (aligned - base)


def fused_tail_ok(d: NcxDims) -> bool:
    """Shapes ncx_train_tail takes (the K rows of a triplet live in registers, one lane per 4 columns)."""
    return d.K <= 32 and d.H <= 256


def train_tail(d: NcxDims, params: Dict[str, torch.Tensor], ws: torch.Tensor, scores: torch.Tensor, gt: torch.Tensor,
               grads: Dict[str, torch.Tensor], want_dscores: bool = False):
    """NCX_F_FUSED_TAIL: `out` + listwise loss / rank / Recall hits + the head of the backward in one pass (ncx_train_tail).
    Fills `scores` (the tensor ops.forward returned untouched) and d out.weight / d out.bias (/ d linear_1.bias)."""
    dev = scores.device
    loss_rows = torch.empty(d.B, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dscores = torch.empty_like(scores) if want_dscores else None
    rank = torch.empty(d.B, dtype=torch.int32, device=dev)
    hits = torch.empty(2, dtype=torch.int32, device=dev)
    p, n = _ws_ptr(ws)
    ps, gs = _params_struct(params, NcxParams), _params_struct(grads, NcxGrads)
    _lib.check(_lib.lib().ncx_train_tail(C.byref(d), C.byref(ps), p, n, _ptr(gt, torch.int32, "gt"), C.c_void_p(scores.data_ptr()),
                                         C.c_void_p(loss_rows.data_ptr()), C.c_void_p(loss.data_ptr()),
                                         _ptr(dscores, torch.float32, "dscores"), C.c_void_p(rank.data_ptr()),
                                         C.c_void_p(hits.data_ptr()), C.byref(gs), _stream()), "ncx_train_tail")
    return dict(loss=loss, loss_rows=loss_rows, dscores=dscores, rank=rank, hits=hits)


FWD_ALL, FWD_PRELUDE, FWD_REST = 0, 1, 2


def forward(d: NcxDims, batch: Batch, params: Dict[str, torch.Tensor], ws: torch.Tensor, phase: int = FWD_ALL) -> Optional[torch.Tensor]:
    """-> scores [B, K] (with NCX_F_FUSED_TAIL in d.flags: allocated here, written by train_tail).
    phase (ncx_forward_phase): FWD_PRELUDE = the data-only part (returns None), FWD_REST = everything that reads the weights;
    PRELUDE then REST on the same workspace == the whole forward, bit for bit."""
    p, n = _ws_ptr(ws)
    ins, ps = batch.c_struct(), _params_struct(params, NcxParams)
    if phase == FWD_PRELUDE:
        _lib.check(_lib.lib().ncx_forward_phase(C.byref(d), C.byref(ins), C.byref(ps), p, n, None, FWD_PRELUDE, _stream()), "ncx_forward_phase")
        return None
    scores = torch.empty(d.B, d.K, dtype=torch.float32, device=batch.feats.device)
    if phase == FWD_ALL:
        _lib.check(_lib.lib().ncx_forward(C.byref(d), C.byref(ins), C.byref(ps), p, n,
                                          C.c_void_p(scores.data_ptr()), _stream()), "ncx_forward")
    else:
        _lib.check(_lib.lib().ncx_forward_phase(C.byref(d), C.byref(ins), C.byref(ps), p, n,
                                                C.c_void_p(scores.data_ptr()), int(phase), _stream()), "ncx_forward_phase")
    return scores


def backward(d: NcxDims, batch: Batch, params: Dict[str, torch.Tensor], ws: torch.Tensor, dscores: torch.Tensor,
             grads: Dict[str, torch.Tensor], phase: int = 0) -> None:
    """phase 0: whole backward.  phases 1 | 2, 3 | 4 and 5 | 2 | 4: the ways to cut it for comm overlap (ncx_backward_phase)."""
    p, n = _ws_ptr(ws)
    ins, ps, gs = batch.c_struct(), _params_struct(params, NcxParams), _params_struct(grads, NcxGrads)
    if phase == 0:
        _lib.check(_lib.lib().ncx_backward(C.byref(d), C.byref(ins), C.byref(ps), p, n,
                                           _ptr(dscores, torch.float32, "dscores"), C.byref(gs), _stream()), "ncx_backward")
    else:
        _lib.check(_lib.lib().ncx_backward_phase(C.byref(d), C.byref(ins), C.byref(ps), p, n,
                                                 _ptr(dscores, torch.float32, "dscores"), C.byref(gs), int(phase), _stream()),
                   "ncx_backward_phase")


def ws_dgt_view(d: NcxDims, ws: torch.Tensor) -> torch.Tensor:
    """fp32 view of the workspace block dGt | dGgt (2 x [H, A]) that phase 3 of backward leaves and phase 4 consumes:
    the bucket a data-parallel job sums over ranks instead of the [A, da] embedding gradient."""
    off, nbytes = C.c_size_t(0), C.c_size_t(0)
    _lib.check(_lib.lib().ncx_ws_region(C.byref(d), 1, C.byref(off), C.byref(nbytes)), "ncx_ws_region")
    base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    return ws[base + off.value: base + off.value + nbytes.value].view(torch.float32)


def ws_de_perm_view(d: NcxDims, ws: torch.Tensor) -> torch.Tensor:
    """int32 view [A + 1] of the presence permutation the last backward (phase 0 or 1) built for the answer_embedding gradient: the
    answer ids of the batch ascending, then the others ascending, and in [A] how many occur.  Empty where the product keeps the full form."""
    off, nbytes = C.c_size_t(0), C.c_size_t(0)
    _lib.check(_lib.lib().ncx_ws_region(C.byref(d), 4, C.byref(off), C.byref(nbytes)), "ncx_ws_region")
    base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    return ws[base + off.value: base + off.value + nbytes.value].view(torch.int32)


def ws_h_view(d: NcxDims, ws: torch.Tensor, l: int) -> torch.Tensor:
    """fp32 view [B*K, H] of the post-dropout activations of linear_l (l = 1 .. L) that the last forward left in the workspace
    (NCX_WS_H1 / NCX_WS_H2 / NCX_WS_H3): what the tests compare element by element."""
    if not 1 <= l <= d.L:
        raise _lib.NcxError("ws_h_view: layer %d of a model with %d" % (l, d.L))
    off, nbytes = C.c_size_t(0), C.c_size_t(0)
    _lib.check(_lib.lib().ncx_ws_region(C.byref(d), (2, 5, 6)[l - 1], C.byref(off), C.byref(nbytes)), "ncx_ws_region")
    base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    return ws[base + off.value: base + off.value + nbytes.value].view(torch.float32).view(d.B * d.K, d.H)


def ws_dpre_view(d: NcxDims, ws: torch.Tensor, l: int) -> torch.Tensor:
    """fp32 view [B*K, H] of the gradient of linear_l's pre-activations that the last backward left in the workspace: l = 1
    (NCX_WS_DPRE1, any L) or l = 2 (NCX_WS_DPRE2, a model with L == 2 only): what the weight-gradient kernels were handed."""
    if l not in (1, 2) or (l == 2 and d.L != 2):
        raise _lib.NcxError("ws_dpre_view: layer %d of a model with %d" % (l, d.L))
    off, nbytes = C.c_size_t(0), C.c_size_t(0)
    _lib.check(_lib.lib().ncx_ws_region(C.byref(d), (3, 7)[l - 1], C.byref(off), C.byref(nbytes)), "ncx_ws_region")
    base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    return ws[base + off.value: base + off.value + nbytes.value].view(torch.float32).view(d.B * d.K, d.H)


def bf16_layout(d: NcxDims) -> dict:
    """The column layout of the bf16 variant's packed operands (ncx_bf16_layout): c_vk, c_vm, c_misc, c_z, c_p, raw, kc, Hp, dap, Ap."""
    return _lib.bf16_layout(d)


def _ws_region(d: NcxDims, ws: torch.Tensor, which: int) -> torch.Tensor:
    off, nbytes = C.c_size_t(0), C.c_size_t(0)
    _lib.check(_lib.lib().ncx_ws_region(C.byref(d), which, C.byref(off), C.byref(nbytes)), "ncx_ws_region")
    base = (ws.data_ptr() + 255) // 256 * 256 - ws.data_ptr()
    return ws[base + off.value: base + off.value + nbytes.value]


def ws_xc_view(d: NcxDims, ws: torch.Tensor) -> torch.Tensor:
    """int16 view [B*K, kc] of the bf16 bit patterns of the packed candidate rows (NCX_WS_XC; NCX_F_BF16 only, else empty)."""
    return _ws_region(d, ws, 8).view(torch.int16).view(-1, bf16_layout(d)["kc"])


def ws_wc_view(d: NcxDims, ws: torch.Tensor) -> torch.Tensor:
    """int16 view [Hp, kc] of the bf16 bit patterns of the packed weights [W1 slices | Gt] (NCX_WS_WC; NCX_F_BF16 only, else empty)."""
    return _ws_region(d, ws, 9).view(torch.int16).view(-1, bf16_layout(d)["kc"])


def ws_gt_view(d: NcxDims, ws: torch.Tensor) -> torch.Tensor:
    """fp32 view [H, ld] of the Gt the last forward produced (NCX_WS_GT): ld = A under NCX_F_BF16, A rounded up to 32 otherwise."""
    return _ws_region(d, ws, 10).view(torch.float32).view(d.H, -1)


def ranking_loss(scores: torch.Tensor, gt: torch.Tensor, scale: float = 0.0, want_grad: bool = True):
    """Listwise softmax-CE / B + rank of the ground truth + Recall@1/@5 hit counts in one pass."""
    B, K = scores.shape
    dev = scores.device
    loss_rows = torch.empty(B, dtype=torch.float32, device=dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    dscores = torch.empty_like(scores) if want_grad else None
    rank = torch.empty(B, dtype=torch.int32, device=dev)
    hits = torch.empty(2, dtype=torch.int32, device=dev)
    _lib.check(_lib.lib().ncx_loss_rank(_ptr(scores, torch.float32, "scores"), _ptr(gt, torch.int32, "gt"), B, K,
                                        float(scale), C.c_void_p(loss_rows.data_ptr()), C.c_void_p(loss.data_ptr()),
                                        _ptr(dscores, torch.float32, "dscores"), C.c_void_p(rank.data_ptr()),
                                        C.c_void_p(hits.data_ptr()), _stream()), "ncx_loss_rank")
    return dict(loss=loss, loss_rows=loss_rows, dscores=dscores, rank=rank, hits=hits)


def adam_step(param, grad, exp_avg, exp_avg_sq, step, lr=1e-4, betas=(0.9, 0.999), eps=1e-8, grad_scale=1.0):
    n = param.numel()
    assert grad.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n
    _lib.check(_lib.lib().ncx_adam_step(_ptr(param, torch.float32, "param"), _ptr(grad, torch.float32, "grad"),
                                        _ptr(exp_avg, torch.float32, "exp_avg"), _ptr(exp_avg_sq, torch.float32, "exp_avg_sq"),
                                        n, lr, betas[0], betas[1], eps, int(step), float(grad_scale), _stream()),
               "ncx_adam_step")


def backward_adam(d: NcxDims, batch: Batch, params: Dict[str, torch.Tensor], ws: torch.Tensor, dscores: torch.Tensor,
                  grads: Dict[str, torch.Tensor], param, grad, exp_avg, exp_avg_sq, n_emb, step, lr=1e-4, betas=(0.9, 0.999),
                  eps=1e-8, grad_scale=1.0) -> None:
    """backward (phase 0) + adam_step over the flat buffers as one call (ncx_backward_adam): `params` / `grads` are views into the flat
    `param` / `grad`, answer_embedding first, n_emb = where the next tensor starts.  Where the route allows, the launch of the
    answer_embedding gradient applies Adam itself; everywhere else the call runs the two steps.  Same bits either way."""
    n = param.numel()
    assert grad.numel() == n and exp_avg.numel() == n and exp_avg_sq.numel() == n
    p, nb = _ws_ptr(ws)
    ins, ps, gs = batch.c_struct(), _params_struct(params, NcxParams), _params_struct(grads, NcxGrads)
    st = _lib.NcxAdamState(_ptr(param, torch.float32, "param"), _ptr(grad, torch.float32, "grad"),
                           _ptr(exp_avg, torch.float32, "exp_avg"), _ptr(exp_avg_sq, torch.float32, "exp_avg_sq"),
                           n, int(n_emb), int(step), lr, betas[0], betas[1], eps, float(grad_scale))
    _lib.check(_lib.lib().ncx_backward_adam(C.byref(d), C.byref(ins), C.byref(ps), p, nb, _ptr(dscores, torch.float32, "dscores"),
                                            C.byref(gs), C.byref(st), _stream()), "ncx_backward_adam")


class MutanWeights:
    """Frozen MutanNoAtt parameters in the layout ncx_vqa_forward wants: the R rank-1 projections stacked
    (fusion.list_linear_hv.{i} -> [R*dim_mm, dim_hv]).  Built once per model; re-stack after loading a checkpoint."""

    def __init__(self, vqa_model):
        f, opt = vqa_model.fusion, vqa_model.opt["fusion"]
        for k in ("activation_hv", "activation_hq", "activation_mm"):
            if k in opt:
                raise _lib.NcxError("ncx_vqa_forward supports the options/cx/*.yaml MUTAN (no %s)" % k)
        if "activation" in vqa_model.opt.get("classif", {}):
            raise _lib.NcxError("ncx_vqa_forward: classif.activation is not supported")
        act = {None: 0, "tanh": 2}
        if opt.get("activation_v") not in act or opt.get("activation_q") not in act:
            raise _lib.NcxError("ncx_vqa_forward supports activation_v/q in {none, tanh}")
        c = lambda t: t.detach().float().contiguous()
        self.t = dict(wv=c(f.linear_v.weight), bv=c(f.linear_v.bias), wq=c(f.linear_q.weight), bq=c(f.linear_q.bias),
                      whv=c(torch.cat([l.weight for l in f.list_linear_hv])), bhv=c(torch.cat([l.bias for l in f.list_linear_hv])),
                      whq=c(torch.cat([l.weight for l in f.list_linear_hq])), bhq=c(torch.cat([l.bias for l in f.list_linear_hq])),
                      wc=c(vqa_model.linear_classif.weight), bc=c(vqa_model.linear_classif.bias))
        self.dhv, self.dhq, self.R, self.dz = opt["dim_hv"], opt["dim_hq"], opt["R"], opt["dim_mm"]
        self.A = self.t["wc"].shape[0]
        self.act_v, self.act_q = act[opt.get("activation_v")], act[opt.get("activation_q")]

    @classmethod
    def from_tensors(cls, t: Dict[str, torch.Tensor], R: int, act_v: int = 2, act_q: int = 2):
        """The same object around caller-owned tensors in the stacked layout (the VQA trainer's flat buffer views: a model
        trained there feeds vqa_forward without re-stacking)."""
        self = cls.__new__(cls)
        self.t = dict(t)
        self.dhv, self.dhq, self.R = t["wv"].shape[0], t["wq"].shape[0], int(R)
        self.A, self.dz = t["wc"].shape
        self.act_v, self.act_q = int(act_v), int(act_q)
        return self

    def c_struct(self):
        m = NcxMutanParams()
        for k, v in self.t.items():
            setattr(m, k, _ptr(v, torch.float32, k))
        m.dhv, m.dhq, m.R, m.act_v, m.act_q = self.dhv, self.dhq, self.R, self.act_v, self.act_q
        return m


class MlbWeights:
    """Frozen MLBNoAtt parameters as ncx_mlb_forward wants them (contiguous fp32: fusion.linear_v / linear_q, linear_classif).
    Built once per model; rebuild after loading a checkpoint.  Activations in {none, tanh}; a fusion block without dim_v or dim_q
    (the reference then passes that input through, fusion.py:33-47) is refused."""
    WS_BYTES, FORWARD = "ncx_mlb_workspace_bytes", "ncx_mlb_forward"

    def __init__(self, vqa_model):
        f, opt = vqa_model.fusion, vqa_model.opt["fusion"]
        for k in ("dim_v", "dim_q", "dim_h"):
            if k not in opt:
                raise _lib.NcxError("ncx_mlb_forward needs fusion.%s (a block that passes an input through is not supported)" % k)
        act = {None: 0, "tanh": 2}
        acts = (opt.get("activation_v"), opt.get("activation_q"), vqa_model.opt.get("classif", {}).get("activation"))
        for name, a in zip(("fusion.activation_v", "fusion.activation_q", "classif.activation"), acts):
            if a not in act:
                raise _lib.NcxError("ncx_mlb_forward supports %s in {none, tanh}, got %r" % (name, a))
        c = lambda t: t.detach().float().contiguous()
        self.t = dict(wv=c(f.linear_v.weight), bv=c(f.linear_v.bias), wq=c(f.linear_q.weight), bq=c(f.linear_q.bias),
                      wc=c(vqa_model.linear_classif.weight), bc=c(vqa_model.linear_classif.bias))
        self.dz = opt["dim_h"]
        self.A = self.t["wc"].shape[0]
        self.act_v, self.act_q, self.act_c = (act[a] for a in acts)

    @classmethod
    def from_tensors(cls, t: Dict[str, torch.Tensor], act_v: int = 2, act_q: int = 2, act_c: int = 2):
        """The same object around caller-owned tensors (the MLB trainer's flat buffer views: a model trained there feeds
        vqa_forward without a copy).  Activation codes: 0 none, 2 tanh."""
        self = cls.__new__(cls)
        self.t = dict(t)
        self.A, self.dz = t["wc"].shape
        self.act_v, self.act_q, self.act_c = int(act_v), int(act_q), int(act_c)
        return self

    def c_struct(self):
        m = NcxMlbParams()
        for k, v in self.t.items():
            setattr(m, k, _ptr(v, torch.float32, k))
        m.dh, m.act_v, m.act_q, m.act_c = self.dz, self.act_v, self.act_q, self.act_c
        return m


def vqa_weights(vqa_model):
    """The weights object of the HIP producer for a frozen no-attention VQA model: MlbWeights for an MLB fusion, else MutanWeights."""
    from vqa.models.fusion import MLBFusion
    return MlbWeights(vqa_model) if isinstance(vqa_model.fusion, MLBFusion) else MutanWeights(vqa_model)


def vqa_dims(B: int, K1: int, dv: int, dq: int, n_img: int, mw) -> NcxDims:
    """The dims the frozen producers read (B, K, dv, dq, dz, A, n_img) for B questions of K1 = K + 1 images each."""
    d = NcxDims()
    d.B, d.K, d.dv, d.dq, d.dz, d.da, d.A, d.H, d.L = B, K1 - 1, dv, dq, mw.dz, 4, mw.A, 4, 1
    d.n_img = n_img
    return d


def vqa_workspace(d: NcxDims, mw, device) -> torch.Tensor:
    """A workspace of the size the producer `mw` belongs to asks for (+ the alignment slack of _ws_ptr)."""
    ws_name = getattr(mw, "WS_BYTES", "ncx_vqa_workspace_bytes")
    m = mw.c_struct()
    need = getattr(_lib.lib(), ws_name)(C.byref(d), C.byref(m))
    if need == 0:
        raise _lib.NcxError("%s: invalid dims" % ws_name)
    return torch.empty(need + 256, dtype=torch.uint8, device=device)


def vqa_route(d: NcxDims, mw) -> dict:
    """What vqa_forward launches for the dims (ncx_vqa_route / ncx_mlb_route; tests, diagnostics)."""
    return (_lib.mlb_route if isinstance(mw, MlbWeights) else _lib.vqa_route)(d, mw.c_struct())


def vqa_ws_view(d: NcxDims, mw, ws: torch.Tensor, name: str) -> torch.Tensor:
    """An intermediate tensor of the last vqa_forward on `ws` as a 2-d view of the workspace: MutanWeights "xq" [B, dhq], "hq" [B, R dz],
    "xv" [B (K + 1), dhv]; MlbWeights "xq" [B, dh], "t_knns" [B K, dh], "t_orig" [B, dh] (with classif.activation), "xv" [B (K + 1), dh]
    (generic route only).  NcxError for a tensor the route does not store."""
    mlb = isinstance(mw, MlbWeights)
    sym, ids = ("ncx_mlb_ws_region", _lib.NCX_MLB_WS) if mlb else ("ncx_vqa_ws_region", _lib.NCX_VQA_WS)
    rows = dict(xq=d.B, hq=d.B, t_orig=d.B, t_knns=d.B * d.K, xv=d.B * (d.K + 1))[name]
    m = mw.c_struct()
    off, nb = C.c_size_t(), C.c_size_t()
    _lib.check(getattr(_lib.lib(), sym)(C.byref(d), C.byref(m), ids[name], C.byref(off), C.byref(nb)), sym)
    pad = (-ws.data_ptr()) % 256
    return ws[pad + off.value: pad + off.value + nb.value].view(torch.float32).view(rows, -1)


def vqa_forward(feats: torch.Tensor, img_idx: torch.Tensor, q_emb: torch.Tensor, mw, want_a_orig=False, ws=None, out=None):
    """HIP replacement of CXModelBase.vqa_forward below the question encoder (cx.py:64-104), for the producer `mw`
    belongs to (MutanWeights: ncx_vqa_forward; MlbWeights: ncx_mlb_forward).  out: caller-owned contiguous
    (a_orig or None, z_orig, a_knns, z_knns) to write into instead of fresh tensors.
    -> (a_orig or None, z_orig [B,dz], a_knns [B,K,A], z_knns [B,K,dz])."""
    B, K1 = img_idx.shape
    d = vqa_dims(B, K1, feats.shape[1], q_emb.shape[1], feats.shape[0], mw)
    m = mw.c_struct()
    ws_name, fwd_name = getattr(mw, "WS_BYTES", "ncx_vqa_workspace_bytes"), getattr(mw, "FORWARD", "ncx_vqa_forward")
    need = getattr(_lib.lib(), ws_name)(C.byref(d), C.byref(m))
    if need == 0:
        raise _lib.NcxError("%s: invalid dims" % ws_name)
    if ws is None or ws.numel() < need + 256:
        ws = torch.empty(need + 256, dtype=torch.uint8, device=feats.device)
    dev = feats.device
    if out is not None:
        a_o, z_o, a_k, z_k = out
        for t, shape in ((z_o, (B, mw.dz)), (z_k, (B, K1 - 1, mw.dz)), (a_k, (B, K1 - 1, mw.A))) + (((a_o, (B, mw.A)),) if want_a_orig else ()):
            if tuple(t.shape) != shape:
                raise _lib.NcxError("vqa_forward: an output of shape %r where %r is written" % (tuple(t.shape), shape))
            _ptr(t, torch.float32, "out")
        a_o = a_o if want_a_orig else None
    else:
        z_o = torch.empty(B, mw.dz, device=dev); z_k = torch.empty(B, K1 - 1, mw.dz, device=dev)
        a_k = torch.empty(B, K1 - 1, mw.A, device=dev)
        a_o = torch.empty(B, mw.A, device=dev) if want_a_orig else None
    p, n = _ws_ptr(ws)
    _lib.check(getattr(_lib.lib(), fwd_name)(C.byref(d), _ptr(feats, torch.float32, "feats"), _ptr(img_idx, torch.int32, "img_idx"),
                                             _ptr(q_emb, torch.float32, "q_emb"), C.byref(m), p, n, C.c_void_p(z_o.data_ptr()),
                                             C.c_void_p(z_k.data_ptr()), C.c_void_p(a_k.data_ptr()),
                                             C.c_void_p(a_o.data_ptr()) if a_o is not None else None, _stream()), fwd_name)
    return a_o, z_o, a_k, z_k


MLB_ATT_FIELDS = ("wv_att", "bv_att", "wq_att", "bq_att", "wa", "ba", "wg", "bg", "wqf", "bqf", "wc", "bc")
MLB_ATT_ACTS = ("act_v_att", "act_q_att", "act_mm", "act_v", "act_q", "act_c")


def mlb_att_acts(opt) -> Optional[Dict[str, int]]:
    """The six activation codes of ncx_mlb_att_params for a model's options (0 absent, 2 tanh); None when one is neither."""
    att, fus, cla = opt["attention"], opt["fusion"], opt.get("classif", {})
    names = (att.get("activation_v"), att.get("activation_q"), att.get("activation_mm"), fus.get("activation_v"), fus.get("activation_q"),
             cla.get("activation"))
    code = {None: 0, "tanh": 2}
    if any(a not in code for a in names):
        return None
    return {k: code[a] for k, a in zip(MLB_ATT_ACTS, names)}


class MlbAttWeights:
    """An MLBAtt's frozen parameters as ncx_mlb_att_forward wants them: contiguous fp32, the two 1 x 1 convolutions as matrices,
    the G glimpse Linears stacked ([G, dh_f, dv], [G, dh_f]).  Built once per weight set; MLBAtt rebuilds it when a parameter changes."""

    def __init__(self, model):
        acts = mlb_att_acts(model.opt)
        if acts is None:
            raise _lib.NcxError("ncx_mlb_att_forward supports activations in {none, tanh}")
        c = lambda t: t.detach().float().contiguous()
        lin = list(model.list_linear_v_fusion)
        self.t = dict(wv_att=c(model.conv_v_att.weight.flatten(1)), bv_att=c(model.conv_v_att.bias),
                      wq_att=c(model.linear_q_att.weight), bq_att=c(model.linear_q_att.bias),
                      wa=c(model.conv_att.weight.flatten(1)), ba=c(model.conv_att.bias),
                      wg=c(torch.stack([l.weight for l in lin])), bg=c(torch.stack([l.bias for l in lin])),
                      wqf=c(model.linear_q_fusion.weight), bqf=c(model.linear_q_fusion.bias),
                      wc=c(model.linear_classif.weight), bc=c(model.linear_classif.bias))
        self.acts = acts
        self._set_dims()

    @classmethod
    def from_tensors(cls, t: Dict[str, torch.Tensor], **acts):
        """The same object around caller-owned tensors in the stacked layout.  Activation codes (0 none, 2 tanh) default to tanh."""
        self = cls.__new__(cls)
        self.t = dict(t)
        self.acts = {k: int(acts.get(k, 2)) for k in MLB_ATT_ACTS}
        self._set_dims()
        return self

    def _set_dims(self):
        t = self.t
        self.dh_att, self.dv = t["wv_att"].shape
        self.dq = t["wq_att"].shape[1]
        self.G, self.dh_f = t["wg"].shape[:2]
        self.A = t["wc"].shape[0]
        want = dict(wv_att=(self.dh_att, self.dv), bv_att=(self.dh_att,), wq_att=(self.dh_att, self.dq), bq_att=(self.dh_att,),
                    wa=(self.G, self.dh_att), ba=(self.G,), wg=(self.G, self.dh_f, self.dv), bg=(self.G, self.dh_f),
                    wqf=(self.G * self.dh_f, self.dq), bqf=(self.G * self.dh_f,), wc=(self.A, self.G * self.dh_f), bc=(self.A,))
        for k, shp in want.items():
            if tuple(t[k].shape) != shp:
                raise _lib.NcxError("MlbAttWeights: %s has shape %s, expected %s" % (k, tuple(t[k].shape), shp))

    def dims(self, B: int, P: int, n_img: int) -> _lib.NcxMlbAttDims:
        d = _lib.NcxMlbAttDims()
        d.B, d.P, d.dv, d.dq, d.dh_att, d.G, d.dh_f, d.A, d.n_img = B, P, self.dv, self.dq, self.dh_att, self.G, self.dh_f, self.A, n_img
        return d

    def c_struct(self, check_device=True):
        m = _lib.NcxMlbAttParams()
        for k in MLB_ATT_FIELDS:
            setattr(m, k, _ptr(self.t[k], torch.float32, k) if check_device else C.c_void_p(self.t[k].data_ptr()))
        for k, v in self.acts.items():
            setattr(m, k, v)
        return m


def mlb_att_weights(module) -> MlbAttWeights:
    """The weights object of the HIP attention forward for an MLBAtt (vqa/models/att.py)."""
    return MlbAttWeights(module)


def mlb_att_dims_ok(mw: MlbAttWeights, B: int, P: int, n_img: int) -> bool:
    """The library's own check of the shape (host only: no launch, no device access)."""
    d = mw.dims(B, P, n_img)
    return _lib.lib().ncx_mlb_att_workspace_bytes(C.byref(d), C.byref(mw.c_struct(check_device=False))) != 0


_MLB_ATT_WS: Dict[torch.device, tuple] = {}          # device -> (shape key, workspace): the last shape's buffer is reused


def mlb_att_workspace(mw: MlbAttWeights, B: int, P: int, n_img: int, device) -> torch.Tensor:
    """The cached workspace of ncx_mlb_att_forward for this shape on `device` (calls on one stream are ordered, so they share it)."""
    d, m = mw.dims(B, P, n_img), mw.c_struct()
    need = _lib.lib().ncx_mlb_att_workspace_bytes(C.byref(d), C.byref(m))
    if need == 0:
        raise _lib.NcxError("ncx_mlb_att_workspace_bytes: invalid dims")
    device = torch.device(device)
    key = tuple(getattr(d, f) for f, _ in d._fields_ if f != "n_img")
    hit = _MLB_ATT_WS.get(device)
    if hit is None or hit[0] != key or hit[1].numel() < need + 256:
        hit = _MLB_ATT_WS[device] = (key, torch.empty(need + 256, dtype=torch.uint8, device=device))
    return hit[1]


def mlb_att_flags(x6=None) -> int:
    """The flags of the attention model's ..._flags entry points: x6 None = the process-wide choice (EXTRA_FLAGS, read now: NCX_X6=1
    in the environment), True / False force the form."""
    return _lib.NCX_F_X6 if (bool(EXTRA_FLAGS & _lib.NCX_F_X6) if x6 is None else bool(x6)) else 0


MLB_ATT_LOGITS_FORMS = ("small", "fp32_64", "fp32_208", "x6_64", "x6_208")


def mlb_att_logits_form(mw: MlbAttWeights, B: int, P: int, n_img: int, x6=None) -> str:
    """Which kernel the conv_v_att stage takes for this shape (ncx_mlb_att_logits_form; host only: no launch, no device access)."""
    d = mw.dims(B, P, n_img)
    rc = _lib.lib().ncx_mlb_att_logits_form(C.byref(d), mlb_att_flags(x6))
    if rc < 0:
        _lib.check(rc, "ncx_mlb_att_logits_form")
    return MLB_ATT_LOGITS_FORMS[rc]


def mlb_att_forward(feats: torch.Tensor, img_idx: Optional[torch.Tensor], q_emb: torch.Tensor, mw: MlbAttWeights, ws=None, x6=None):
    """MLBAtt.forward below the question encoder, in eval mode (ncx_mlb_att_forward_flags; reference vqa/models/att.py:39-163), on the
    current stream.  feats: the table of NCHW maps [n_img, dv, W, H] (or [n_img, dv, P]), read in place; img_idx [B] int32 picks
    each question's image, None = the dense input (question b reads feats[b]).  q_emb [B, dq].  x6: mlb_att_flags.
    -> (logits [B, A], att [B, G, P]); att[:, g] is the module's list_att[g], position p = w H + h."""
    if feats.dim() not in (3, 4):
        raise ValueError("feats must be [n_img, dv, W, H] or [n_img, dv, P], got %s" % (tuple(feats.shape),))
    n_img, dv = feats.shape[:2]
    P = feats[0, 0].numel()
    dev = feats.device
    B = q_emb.shape[0]
    if img_idx is None:
        if n_img != B:
            raise ValueError("dense input: %d maps for %d questions" % (n_img, B))
        img_idx = torch.arange(B, dtype=torch.int32, device=dev)
    if img_idx.shape != (B,):
        raise ValueError("img_idx must be [B] = [%d], got %s" % (B, tuple(img_idx.shape)))
    if dv != mw.dv or q_emb.shape[1] != mw.dq:
        raise ValueError("feats / q_emb widths (%d, %d) do not match the weights (%d, %d)" % (dv, q_emb.shape[1], mw.dv, mw.dq))
    d, m = mw.dims(B, P, n_img), mw.c_struct()
    if ws is None:
        ws = mlb_att_workspace(mw, B, P, n_img, dev)
    logits = torch.empty(B, mw.A, dtype=torch.float32, device=dev)
    att = torch.empty(B, mw.G, P, dtype=torch.float32, device=dev)
    p, n = _ws_ptr(ws)
    with torch.cuda.device(dev):
        _lib.check(_lib.lib().ncx_mlb_att_forward_flags(C.byref(d), _ptr(feats, torch.float32, "feats"), _ptr(img_idx, torch.int32, "img_idx"),
                                                        _ptr(q_emb, torch.float32, "q_emb"), C.byref(m), mlb_att_flags(x6), p, n,
                                                        C.c_void_p(logits.data_ptr()), C.c_void_p(att.data_ptr()), _stream()),
                   "ncx_mlb_att_forward_flags")
    return logits, att


def cosine_gram(emb: torch.Tensor) -> torch.Tensor:
    """sklearn cosine_similarity(emb) on the device (ncx_cosine_gram; reference cx.py:174-175): [A, da] fp32 -> [A, A] fp32.
    A zero row stays zero (its similarities are 0, the diagonal included), as sklearn's normalisation leaves it."""
    if emb.dim() != 2:
        raise ValueError("cosine_gram takes a 2-d [A, da] embedding, got %s" % (tuple(emb.shape),))
    emb = emb.contiguous()
    A, da = emb.shape
    need = _lib.lib().ncx_cosine_gram_workspace_bytes(A, da)
    if need == 0:
        raise _lib.NcxError("ncx_cosine_gram_workspace_bytes: unsupported shape %s" % (tuple(emb.shape),))
    ws = torch.empty(need + 256, dtype=torch.uint8, device=emb.device)
    gram = torch.empty(A, A, dtype=torch.float32, device=emb.device)
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_cosine_gram(_ptr(emb, torch.float32, "emb"), A, da, p, n, C.c_void_p(gram.data_ptr()), _stream()),
               "ncx_cosine_gram")
    return gram


_SEM_FLAGS: Dict[torch.device, torch.Tensor] = {}


def semantic_bad_flag(device) -> torch.Tensor:
    """The per-device int32 flag ncx_semantic_scores sets on an answer id outside [0, A) (sticky until checked)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    f = _SEM_FLAGS.get(device)
    if f is None:
        f = _SEM_FLAGS[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


def semantic_scores(a_knns: torch.Tensor, aids: torch.Tensor, gram: torch.Tensor, lam: float, want_raw: bool = False,
                    bad_flag: Optional[torch.Tensor] = None):
    """The semantic baseline scorer (ncx_semantic_scores; reference cx.py:182-209) on the current stream, no host sync:
    a_knns [B, K, A] logits, aids [B] answer ids, gram [A, A] (cosine_gram) -> scores [B, K] (softmax over k: probabilities,
    as the reference returns), and with want_raw the pre-softmax s [B, K] as well: (scores, raw).
    An id outside [0, A) leaves NaN in its row and sets `bad_flag` (default: semantic_bad_flag(device)); the IndexError is
    raised by check_semantic_ids -- deferred, so that an evaluation loop pays one host sync at its end, not one per batch."""
    if a_knns.dim() != 3:
        raise ValueError("a_knns must be [B, K, A], got %s" % (tuple(a_knns.shape),))
    B, K, A = a_knns.shape
    if tuple(aids.shape) != (B,):
        raise ValueError("aids must be [%d], got %s" % (B, tuple(aids.shape)))
    if tuple(gram.shape) != (A, A):
        raise ValueError("gram must be [%d, %d] (the logits' width), got %s" % (A, A, tuple(gram.shape)))
    a_knns, gram = a_knns.float().contiguous(), gram.contiguous()
    aids = aids.to(torch.int32).contiguous()
    if bad_flag is None:
        bad_flag = semantic_bad_flag(a_knns.device)
    scores = torch.empty(B, K, dtype=torch.float32, device=a_knns.device)
    raw = torch.empty(B, K, dtype=torch.float32, device=a_knns.device) if want_raw else None
    _lib.check(_lib.lib().ncx_semantic_scores(_ptr(a_knns, torch.float32, "a_knns"), _ptr(aids, torch.int32, "aids"), B, K, A,
                                              _ptr(gram, torch.float32, "gram"), float(lam), C.c_void_p(scores.data_ptr()),
                                              _ptr(raw, torch.float32, "raw"), _ptr(bad_flag, torch.int32, "bad_flag"), _stream()),
               "ncx_semantic_scores")
    return (scores, raw) if want_raw else scores


def check_semantic_ids(bad_flag: Optional[torch.Tensor] = None, device=None) -> None:
    """Raises IndexError (what the reference's numpy indexing emb_pairs[aid, :] raises, cx.py:194) if a semantic_scores call
    since the last check saw an answer id outside [0, A); clears the flag.  Synchronises with the flag's stream."""
    if bad_flag is None:
        bad_flag = semantic_bad_flag(device if device is not None else "cuda")
    if int(bad_flag.item()):
        bad_flag.zero_()
        raise IndexError("answer_aids outside [0, A) in a semantic_scores call")


def similarity_scores(feats: torch.Tensor, img_idx: torch.Tensor, z_orig: torch.Tensor, z_knns: torch.Tensor, a_knns: torch.Tensor,
                      aids: torch.Tensor, bad_flag: Optional[torch.Tensor] = None, want_parts: bool = False):
    """The similarity scorer (ncx_similarity_scores; reference cx.py:496-518) on the current stream, no host sync:
    feats [n_img, dv] feature table, img_idx [B, K + 1] its row ids (column 0 the original image), z_orig [B, dz], z_knns
    [B, K, dz], a_knns [B, K, A] logits, aids [B] -> scores [B, K] = cos(v) + cos(z) + cross-entropy (higher = better), and with
    want_parts the three terms [B, K, 3] as well: (scores, parts).  The rows are gathered by id inside the kernel.
    A row id outside [0, n_img) or an answer id outside [0, A) leaves NaN in its question's row and sets `bad_flag` (default:
    semantic_bad_flag(device)); check_similarity_ids raises the IndexError -- deferred, as for semantic_scores."""
    if feats.dim() != 2 or img_idx.dim() != 2 or a_knns.dim() != 3:
        raise ValueError("similarity_scores takes feats [n_img, dv], img_idx [B, K + 1], a_knns [B, K, A]; got %s, %s, %s"
                         % (tuple(feats.shape), tuple(img_idx.shape), tuple(a_knns.shape)))
    B, K, A = a_knns.shape
    n_img, dv = feats.shape
    if tuple(img_idx.shape) != (B, K + 1):
        raise ValueError("img_idx must be [%d, %d], got %s" % (B, K + 1, tuple(img_idx.shape)))
    if z_orig.dim() != 2 or z_orig.shape[0] != B or tuple(z_knns.shape) != (B, K, z_orig.shape[1]):
        raise ValueError("z_orig must be [%d, dz] and z_knns [%d, %d, dz], got %s and %s" % (B, B, K, tuple(z_orig.shape), tuple(z_knns.shape)))
    if tuple(aids.shape) != (B,):
        raise ValueError("aids must be [%d], got %s" % (B, tuple(aids.shape)))
    dev = a_knns.device
    feats, z_orig, z_knns, a_knns = (t.float().contiguous() for t in (feats, z_orig, z_knns, a_knns))
    img_idx, aids = img_idx.to(torch.int32).contiguous(), aids.to(torch.int32).contiguous()
    if bad_flag is None:
        bad_flag = semantic_bad_flag(dev)
    scores = torch.empty(B, K, dtype=torch.float32, device=dev)
    parts = torch.empty(B, K, 3, dtype=torch.float32, device=dev) if want_parts else None
    _lib.check(_lib.lib().ncx_similarity_scores(_ptr(feats, torch.float32, "feats"), _ptr(img_idx, torch.int32, "img_idx"), n_img, dv,
                                                _ptr(z_orig, torch.float32, "z_orig"), _ptr(z_knns, torch.float32, "z_knns"),
                                                z_orig.shape[1], _ptr(a_knns, torch.float32, "a_knns"), _ptr(aids, torch.int32, "aids"),
                                                A, B, K, C.c_void_p(scores.data_ptr()), _ptr(parts, torch.float32, "parts"),
                                                _ptr(bad_flag, torch.int32, "bad_flag"), _stream()),
               "ncx_similarity_scores")
    return (scores, parts) if want_parts else scores


def check_similarity_ids(bad_flag: Optional[torch.Tensor] = None, device=None) -> None:
    """Raises IndexError (what the reference's indexing of the feature table and F.cross_entropy's target check raise) if a
    similarity_scores call since the last check saw a feature row id outside [0, n_img) or an answer id outside [0, A);
    clears the flag.  Synchronises with the flag's stream."""
    if bad_flag is None:
        bad_flag = semantic_bad_flag(device if device is not None else "cuda")
    if int(bad_flag.item()):
        bad_flag.zero_()
        raise IndexError("feature row ids outside [0, n_img) or answer_aids outside [0, A) in a similarity_scores call")


# ---- the question encoder (include/neuralcx.h: ncx_gru_*) -----------------------------------------------------------------------
GRU_UNITS = 32          # hidden units per workgroup of the step kernel: the packed layout's block (csrc/ncx_gru.hip)


def _pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def gru_pack_layout(w_ih: torch.Tensor, w_hh: torch.Tensor, b_ih: torch.Tensor, b_hh: torch.Tensor) -> torch.Tensor:
    """The packed layout of ncx_gru_pack restated with tensor ops (any device; not on the product path: GruWeights packs device
    weights with the kernel, this is what a test or a host without the kernel compares against):
    W [nj][3][32][kp] | bias [nj][6: ir iz in hr hz hn][32], kp = pad32(dim_emb) + pad32(dim_q), zero padded."""
    dim_q, dim_emb = w_hh.shape[1], w_ih.shape[1]
    kx, nj = _pad32(dim_emb), (dim_q + GRU_UNITS - 1) // GRU_UNITS
    W = torch.zeros(nj * GRU_UNITS, 3, kx + _pad32(dim_q), dtype=torch.float32, device=w_ih.device)
    W[:dim_q, :, :dim_emb] = w_ih.detach().float().view(3, dim_q, dim_emb).transpose(0, 1)
    W[:dim_q, :, kx:kx + dim_q] = w_hh.detach().float().view(3, dim_q, dim_q).transpose(0, 1)
    b = torch.zeros(nj * GRU_UNITS, 6, dtype=torch.float32, device=w_ih.device)
    b[:dim_q, :3] = b_ih.detach().float().view(3, dim_q).t()
    b[:dim_q, 3:] = b_hh.detach().float().view(3, dim_q).t()
    W = W.view(nj, GRU_UNITS, 3, -1).transpose(1, 2)
    b = b.view(nj, GRU_UNITS, 6).transpose(1, 2)
    return torch.cat([W.reshape(-1), b.reshape(-1)])


def gru_unpack_layout(packed: torch.Tensor, dim_emb: int, dim_q: int):
    """-> (w_ih [3 dim_q, dim_emb], w_hh [3 dim_q, dim_q], b_ih [3 dim_q], b_hh [3 dim_q]) read back out of the packed layout."""
    kx, nj = _pad32(dim_emb), (dim_q + GRU_UNITS - 1) // GRU_UNITS
    kp = kx + _pad32(dim_q)
    nw = nj * 3 * GRU_UNITS * kp
    W = packed[:nw].view(nj, 3, GRU_UNITS, kp).transpose(1, 2).reshape(nj * GRU_UNITS, 3, kp)[:dim_q]
    b = packed[nw:].view(nj, 6, GRU_UNITS).transpose(1, 2).reshape(nj * GRU_UNITS, 6)[:dim_q]
    return (W[:, :, :dim_emb].transpose(0, 1).reshape(3 * dim_q, dim_emb), W[:, :, kx:kx + dim_q].transpose(0, 1).reshape(3 * dim_q, dim_q),
            b[:, :3].t().reshape(-1), b[:, 3:].t().reshape(-1))


class GruWeights:
    """A GRUEncoder's frozen parameters as ncx_gru_encode wants them: the embedding table E [V + 1, dim_emb] (the parameter itself
    when it is contiguous fp32) and the GRU's weights in the packed layout (ncx_gru_pack on the device; for a CPU encoder the same
    layout from gru_pack_layout, which only inspection and tests use: gru_encode refuses host tensors).  Built once per weight set;
    GRUEncoder rebuilds it when a parameter changes."""

    def __init__(self, encoder):
        g = encoder.gru
        if not isinstance(g, torch.nn.GRU) or g.num_layers != 1 or g.bidirectional or not g.bias or not g.batch_first:
            raise _lib.NcxError("ncx_gru_encode takes a one-layer unidirectional batch_first nn.GRU with biases")
        E = encoder.embedding.weight.detach()
        ws = [p.detach() for p in (g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0)]
        if any(t.dtype != torch.float32 for t in [E] + ws):
            raise _lib.NcxError("ncx_gru_encode takes fp32 parameters")
        self.E = E.contiguous()
        self.V1, self.dim_emb = self.E.shape
        self.dim_q = g.hidden_size
        nbytes = _lib.lib().ncx_gru_packed_bytes(self.dim_emb, self.dim_q)
        if nbytes == 0:
            raise _lib.NcxError("ncx_gru_pack: dims out of range (dim_emb %d, dim_q %d)" % (self.dim_emb, self.dim_q))
        if self.E.is_cuda:
            ws = [t.contiguous() for t in ws]
            self.packed = torch.empty(nbytes // 4, dtype=torch.float32, device=self.E.device)
            with torch.cuda.device(self.E.device):
                _lib.check(_lib.lib().ncx_gru_pack(*[_ptr(t, torch.float32, "gru weight") for t in ws], self.dim_emb, self.dim_q,
                                                   C.c_void_p(self.packed.data_ptr()), _stream()), "ncx_gru_pack")
        else:
            self.packed = gru_pack_layout(*ws)
            assert self.packed.numel() * 4 == nbytes
        self.t = {"E": self.E, "packed": self.packed}

    def unpack(self):
        return gru_unpack_layout(self.packed, self.dim_emb, self.dim_q)


def gru_weights(encoder) -> GruWeights:
    """The weights object of the HIP question encoder for a GRUEncoder (vqa/models/seq2vec.py)."""
    return GruWeights(encoder)


_GRU_FLAGS: Dict[torch.device, torch.Tensor] = {}


def gru_bad_flag(device) -> torch.Tensor:
    """The per-device int32 flag ncx_gru_encode sets on a word id outside [0, V + 1) (sticky until checked)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    f = _GRU_FLAGS.get(device)
    if f is None:
        f = _GRU_FLAGS[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


GRU_STEP_FORMS = ("fp32", "x6")


def gru_step_form(dim_emb: int, dim_q: int, B: int, T: int, x6=None) -> str:
    """Which step kernel gru_encode / gru_train_forward take for this shape (ncx_gru_step_form; host only: no launch, no device
    access).  x6: as mlb_att_flags -- None = the process-wide choice (EXTRA_FLAGS, read now: NCX_X6=1), True / False force the form."""
    rc = _lib.lib().ncx_gru_step_form(B, T, dim_emb, dim_q, mlb_att_flags(x6))
    if rc < 0:
        raise _lib.NcxError("ncx_gru_step_form: dims out of range (B %d, T %d, dim_emb %d, dim_q %d)" % (B, T, dim_emb, dim_q))
    return GRU_STEP_FORMS[rc]


def gru_encode(wids: torch.Tensor, gw: GruWeights, bad_flag: Optional[torch.Tensor] = None, x6=None) -> torch.Tensor:
    """The question encoder (ncx_gru_encode_flags; GRUEncoder.forward in eval mode) on the current stream, no host sync: wids [B, T] word
    ids right-padded with 0 -> q [B, dim_q], the hidden state after each question's last word.  Padded steps are not computed.
    x6 (gru_step_form): the bf16 x 6 form of the step kernel -- fp32-grade, not bit-equal to the fp32 form.
    A word id outside [0, V + 1) is never used as an address; it sets `bad_flag` (default: gru_bad_flag(device)) and
    check_gru_ids raises the IndexError -- deferred, as for semantic_scores."""
    if wids.dim() != 2:
        raise ValueError("wids must be [B, T], got %s" % (tuple(wids.shape),))
    if wids.is_floating_point():
        raise TypeError("wids must be an integer tensor, got %s" % wids.dtype)
    B, T = wids.shape
    if B < 1 or not 1 <= T <= 64:
        raise ValueError("gru_encode takes B >= 1 questions of 1 <= T <= 64 steps, got [%d, %d]" % (B, T))
    dev = wids.device
    if gw.packed.device != dev:
        raise _lib.NcxError("wids are on %s, the encoder's weights on %s" % (dev, gw.packed.device))
    wids = wids.to(torch.int32).contiguous()
    if bad_flag is None:
        bad_flag = gru_bad_flag(dev)
    n = _lib.lib().ncx_gru_workspace_bytes(B, T, gw.dim_emb, gw.dim_q)
    if n == 0:
        raise _lib.NcxError("ncx_gru_workspace_bytes: dims out of range")
    ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
    p, n = _ws_ptr(ws)
    q = torch.empty(B, gw.dim_q, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ncx_gru_encode_flags(_ptr(wids, torch.int32, "wids"), B, T, _ptr(gw.E, torch.float32, "E"), gw.V1, gw.dim_emb,
                                               gw.dim_q, _ptr(gw.packed, torch.float32, "packed"), mlb_att_flags(x6), p, n,
                                               C.c_void_p(q.data_ptr()), _ptr(bad_flag, torch.int32, "bad_flag"), _stream()), "ncx_gru_encode")
    return q


def check_gru_ids(bad_flag: Optional[torch.Tensor] = None, device=None) -> None:
    """Raises IndexError (what nn.Embedding raises for such an id) if a gru_encode call since the last check saw a word id outside
    [0, V + 1); clears the flag.  Synchronises with the flag's stream."""
    if bad_flag is None:
        bad_flag = gru_bad_flag(device if device is not None else "cuda")
    if int(bad_flag.item()):
        bad_flag.zero_()
        raise IndexError("question_wids outside [0, V + 1) in a gru_encode call")


# ---- the two-layer LSTM question encoder (include/neuralcx.h: ncx_lstm2_*) ----------------------------------------------------------
LSTM_KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def _lstm_layer_layout(w_ih, w_hh, b_ih, b_hh):
    H, n_in = w_hh.shape[1], w_ih.shape[1]
    kx, nj = _pad32(n_in), (H + GRU_UNITS - 1) // GRU_UNITS
    W = torch.zeros(nj * GRU_UNITS, 4, kx + _pad32(H), dtype=torch.float32, device=w_ih.device)
    W[:H, :, :n_in] = w_ih.detach().float().view(4, H, n_in).transpose(0, 1)
    W[:H, :, kx:kx + H] = w_hh.detach().float().view(4, H, H).transpose(0, 1)
    b = torch.zeros(nj * GRU_UNITS, 4, dtype=torch.float32, device=w_ih.device)
    b[:H] = (b_ih.detach().float() + b_hh.detach().float()).view(4, H).t()
    return torch.cat([W.view(nj, GRU_UNITS, 4, -1).transpose(1, 2).reshape(-1), b.view(nj, GRU_UNITS, 4).transpose(1, 2).reshape(-1)])


def lstm_pack_layout(layer0, layer1) -> torch.Tensor:
    """The packed layout of ncx_lstm2_pack restated with tensor ops (any device; what a test compares the kernel against).  layer0 and
    layer1 are (w_ih, w_hh, b_ih, b_hh) of rnn_0 and rnn_1, gate blocks i | f | g | o:
    layer 0 | layer 1, layer l = W [nj][4][32][kp_l] | bias [nj][4][32] (b_ih + b_hh), kp_l = pad32(in_l) + pad32(H), zero padded."""
    return torch.cat([_lstm_layer_layout(*layer0), _lstm_layer_layout(*layer1)])


def lstm_unpack_layout(packed: torch.Tensor, emb: int, H: int):
    """-> ((w_ih, w_hh, b) of layer 0, (w_ih, w_hh, b) of layer 1) read back out of the packed layout; b = b_ih + b_hh [4 H]."""
    nj, out, off = (H + GRU_UNITS - 1) // GRU_UNITS, [], 0
    for n_in in (emb, H):
        kx = _pad32(n_in)
        kp = kx + _pad32(H)
        nw, nb = nj * 4 * GRU_UNITS * kp, nj * 4 * GRU_UNITS
        W = packed[off:off + nw].view(nj, 4, GRU_UNITS, kp).transpose(1, 2).reshape(nj * GRU_UNITS, 4, kp)[:H]
        b = packed[off + nw:off + nw + nb].view(nj, 4, GRU_UNITS).transpose(1, 2).reshape(nj * GRU_UNITS, 4)[:H]
        out.append((W[:, :, :n_in].transpose(0, 1).reshape(4 * H, n_in), W[:, :, kx:kx + H].transpose(0, 1).reshape(4 * H, H), b.t().reshape(-1)))
        off += nw + nb
    return tuple(out)


class LstmWeights:
    """A TwoLSTM's frozen parameters as ncx_lstm2_encode wants them: the embedding table E [V + 1, emb] (the parameter itself when it
    is contiguous fp32; tanh is taken in the kernel's loader) and both layers' weights in the packed layout (ncx_lstm2_pack on the device;
    for a CPU encoder lstm_pack_layout, for inspection and tests only).  Built once per weight set; TwoLSTM rebuilds it when a
    parameter changes."""

    def __init__(self, encoder):
        r0, r1 = encoder.rnn_0, encoder.rnn_1
        for r in (r0, r1):
            if not isinstance(r, torch.nn.LSTM) or r.num_layers != 1 or r.bidirectional or not r.bias or not r.batch_first or r.proj_size:
                raise _lib.NcxError("ncx_lstm2_encode takes two one-layer unidirectional batch_first nn.LSTMs with biases")
        if r0.hidden_size != r1.hidden_size or r1.input_size != r0.hidden_size:
            raise _lib.NcxError("ncx_lstm2_encode takes rnn_1 = LSTM(H -> H) on rnn_0 = LSTM(emb -> H)")
        E = encoder.embedding.weight.detach()
        ws = [getattr(r, k).detach() for r in (r0, r1) for k in LSTM_KEYS]
        if any(t.dtype != torch.float32 for t in [E] + ws):
            raise _lib.NcxError("ncx_lstm2_encode takes fp32 parameters")
        self.E = E.contiguous()
        self.V1, self.emb = self.E.shape
        self.H = r0.hidden_size
        if r0.input_size != self.emb:
            raise _lib.NcxError("rnn_0 takes %d inputs, the embedding gives %d" % (r0.input_size, self.emb))
        nbytes = _lib.lib().ncx_lstm2_packed_bytes(self.emb, self.H)
        if nbytes == 0:
            raise _lib.NcxError("ncx_lstm2_pack: dims out of range (emb %d, H %d)" % (self.emb, self.H))
        if self.E.is_cuda:
            ws = [t.contiguous() for t in ws]
            self.packed = torch.empty(nbytes // 4, dtype=torch.float32, device=self.E.device)
            with torch.cuda.device(self.E.device):
                _lib.check(_lib.lib().ncx_lstm2_pack(*[_ptr(t, torch.float32, "lstm weight") for t in ws], self.emb, self.H,
                                                     C.c_void_p(self.packed.data_ptr()), _stream()), "ncx_lstm2_pack")
        else:
            self.packed = lstm_pack_layout(ws[:4], ws[4:])
            assert self.packed.numel() * 4 == nbytes
        self.t = {"E": self.E, "packed": self.packed}

    def unpack(self):
        return lstm_unpack_layout(self.packed, self.emb, self.H)


def lstm_weights(encoder) -> LstmWeights:
    """The weights object of the HIP question encoder for a TwoLSTM (vqa/models/seq2vec.py)."""
    return LstmWeights(encoder)


def lstm_step_form(emb: int, H: int, B: int, T: int, x6=None) -> str:
    """Which step kernel lstm_encode / lstm_train_forward take for this shape (ncx_lstm2_step_form; host only: no launch, no device
    access).  x6: as gru_step_form -- None = the process-wide choice (EXTRA_FLAGS, read now: NCX_X6=1), True / False force the form."""
    rc = _lib.lib().ncx_lstm2_step_form(B, T, emb, H, mlb_att_flags(x6))
    if rc < 0:
        raise _lib.NcxError("ncx_lstm2_step_form: dims out of range (B %d, T %d, emb %d, H %d)" % (B, T, emb, H))
    return GRU_STEP_FORMS[rc]


def lstm_encode(wids: torch.Tensor, lw: LstmWeights, bad_flag: Optional[torch.Tensor] = None, x6=None) -> torch.Tensor:
    """The two-layer LSTM question encoder (ncx_lstm2_encode_flags; TwoLSTM.forward in eval mode) on the current stream, no host sync: wids
    [B, T] -> q [B, 2 H], layer 0's and layer 1's hidden state after each question's last word.  len = the number of nonzero ids, T for
    an all-padding row; padded steps are not computed.  x6 (lstm_step_form): the bf16 x 6 form of the step kernel -- fp32-grade, not
    bit-equal to the fp32 form.  A word id outside [0, V + 1) is never used as an address; it sets `bad_flag`
    (default: gru_bad_flag(device), the flag check_gru_ids reads)."""
    if wids.dim() != 2:
        raise ValueError("wids must be [B, T], got %s" % (tuple(wids.shape),))
    if wids.is_floating_point():
        raise TypeError("wids must be an integer tensor, got %s" % wids.dtype)
    B, T = wids.shape
    if B < 1 or not 1 <= T <= 64:
        raise ValueError("lstm_encode takes B >= 1 questions of 1 <= T <= 64 steps, got [%d, %d]" % (B, T))
    dev = wids.device
    if lw.packed.device != dev:
        raise _lib.NcxError("wids are on %s, the encoder's weights on %s" % (dev, lw.packed.device))
    wids = wids.to(torch.int32).contiguous()
    if bad_flag is None:
        bad_flag = gru_bad_flag(dev)
    n = _lib.lib().ncx_lstm2_workspace_bytes(B, T, lw.emb, lw.H)
    if n == 0:
        raise _lib.NcxError("ncx_lstm2_workspace_bytes: dims out of range")
    ws = torch.empty(n + 256, dtype=torch.uint8, device=dev)
    p, n = _ws_ptr(ws)
    q = torch.empty(B, 2 * lw.H, dtype=torch.float32, device=dev)
    _lib.check(_lib.lib().ncx_lstm2_encode_flags(_ptr(wids, torch.int32, "wids"), B, T, _ptr(lw.E, torch.float32, "E"), lw.V1, lw.emb, lw.H,
                                                 _ptr(lw.packed, torch.float32, "packed"), mlb_att_flags(x6), p, n, C.c_void_p(q.data_ptr()),
                                                 _ptr(bad_flag, torch.int32, "bad_flag"), _stream()), "ncx_lstm2_encode")
    return q


# ---- training the question encoder (include/neuralcx.h: ncx_gru_train_*, ncx_gru_pack_t) -----------------------------------------
GRU_T_ROWS = 64         # output columns per workgroup of the backward's products: the rows of the transposed pack come in whole tiles


def _pad64(n: int) -> int:
    return (n + GRU_T_ROWS - 1) // GRU_T_ROWS * GRU_T_ROWS


def gru_pack_t_layout(w_ih: torch.Tensor, w_hh: torch.Tensor) -> torch.Tensor:
    """The layout of ncx_gru_pack_t restated with tensor ops (any device; what a test compares the kernel against): the contraction
    runs over the 3 dim_q gate rows, WhhT [pad64(dim_q)][3 dqp] | WihT [pad64(dim_emb)][3 dqp], WhhT[j][g dqp + u] = w_hh[g dim_q + u][j],
    WihT[c][g dqp + u] = w_ih[g dim_q + u][c], dqp = pad32(dim_q), zero padded."""
    dim_q, dim_emb = w_hh.shape[1], w_ih.shape[1]
    dqp = _pad32(dim_q)
    out = []
    for w, n in ((w_hh, dim_q), (w_ih, dim_emb)):
        t = torch.zeros(_pad64(n), 3, dqp, dtype=torch.float32, device=w.device)
        t[:n, :, :dim_q] = w.detach().float().view(3, dim_q, n).permute(2, 0, 1)
        out.append(t.reshape(-1))
    return torch.cat(out)


def gru_unpack_t_layout(packed_t: torch.Tensor, dim_emb: int, dim_q: int):
    """-> (w_ih [3 dim_q, dim_emb], w_hh [3 dim_q, dim_q]) read back out of the transposed pack."""
    dqp = _pad32(dim_q)
    nh = _pad64(dim_q) * 3 * dqp
    hh = packed_t[:nh].view(_pad64(dim_q), 3, dqp)[:dim_q, :, :dim_q].permute(1, 2, 0).reshape(3 * dim_q, dim_q)
    ih = packed_t[nh:].view(_pad64(dim_emb), 3, dqp)[:dim_emb, :, :dim_q].permute(1, 2, 0).reshape(3 * dim_q, dim_emb)
    return ih, hh


class GruTrainWeights:
    """One weight set of the trainable encoder as ncx_gru_train_forward / _backward want it: E, the forward's pack (ncx_gru_pack) and
    the backward's transposed pack (ncx_gru_pack_t).  Built from the five tensors, on their device."""

    def __init__(self, E, w_ih, w_hh, b_ih, b_hh):
        ts = [t.detach() for t in (E, w_ih, w_hh, b_ih, b_hh)]
        if any(t.dtype != torch.float32 for t in ts):
            raise _lib.NcxError("ncx_gru_train_* take fp32 parameters")
        E, w_ih, w_hh, b_ih, b_hh = (t.contiguous() for t in ts)
        if E.dim() != 2 or w_ih.dim() != 2 or w_hh.dim() != 2 or w_ih.shape[1] != E.shape[1] or w_hh.shape[0] != 3 * w_hh.shape[1] or \
                w_ih.shape[0] != w_hh.shape[0] or tuple(b_ih.shape) != (w_hh.shape[0],) or tuple(b_hh.shape) != (w_hh.shape[0],):
            raise ValueError("gru_train_weights takes E [V + 1, de], w_ih [3 dq, de], w_hh [3 dq, dq], b_ih, b_hh [3 dq]; got %s"
                             % ([tuple(t.shape) for t in ts],))
        self.E = E
        self.V1, self.dim_emb = E.shape
        self.dim_q = w_hh.shape[1]
        L = _lib.lib()
        n, nt = L.ncx_gru_packed_bytes(self.dim_emb, self.dim_q), L.ncx_gru_packed_t_bytes(self.dim_emb, self.dim_q)
        if n == 0 or nt == 0:
            raise _lib.NcxError("ncx_gru_pack_t: dims out of range (dim_emb %d, dim_q %d)" % (self.dim_emb, self.dim_q))
        self.packed = torch.empty(n // 4, dtype=torch.float32, device=E.device)
        self.packed_t = torch.empty(nt // 4, dtype=torch.float32, device=E.device)
        with torch.cuda.device(E.device):
            _lib.check(L.ncx_gru_pack(*[_ptr(t, torch.float32, "gru weight") for t in (w_ih, w_hh, b_ih, b_hh)], self.dim_emb, self.dim_q,
                                      C.c_void_p(self.packed.data_ptr()), _stream()), "ncx_gru_pack")
            _lib.check(L.ncx_gru_pack_t(_ptr(w_ih, torch.float32, "w_ih"), _ptr(w_hh, torch.float32, "w_hh"), self.dim_emb, self.dim_q,
                                        C.c_void_p(self.packed_t.data_ptr()), _stream()), "ncx_gru_pack_t")


def gru_train_weights(E, w_ih, w_hh, b_ih, b_hh) -> GruTrainWeights:
    return GruTrainWeights(E, w_ih, w_hh, b_ih, b_hh)


def _gru_train_args(wids: torch.Tensor, gw: GruTrainWeights, what: str):
    if wids.dim() != 2:
        raise ValueError("wids must be [B, T], got %s" % (tuple(wids.shape),))
    if wids.is_floating_point():
        raise TypeError("wids must be an integer tensor, got %s" % wids.dtype)
    B, T = wids.shape
    if B < 1 or not 1 <= T <= 64:
        raise ValueError("%s takes B >= 1 questions of 1 <= T <= 64 steps, got [%d, %d]" % (what, B, T))
    if gw.packed.device != wids.device:
        raise _lib.NcxError("wids are on %s, the encoder's weights on %s" % (wids.device, gw.packed.device))
    return B, T, wids.to(torch.int32).contiguous()


def gru_train_workspace(B: int, T: int, gw: GruTrainWeights, device) -> torch.Tensor:
    """The workspace of one training step (ncx_gru_train_workspace_bytes): the length plan and the stash the backward needs."""
    n = _lib.lib().ncx_gru_train_workspace_bytes(B, T, gw.dim_emb, gw.dim_q)
    if n == 0:
        raise _lib.NcxError("ncx_gru_train_workspace_bytes: dims out of range")
    return torch.empty(n + 256, dtype=torch.uint8, device=device)


def gru_train_forward(wids: torch.Tensor, gw: GruTrainWeights, ws: torch.Tensor, bad_flag: Optional[torch.Tensor] = None, x6=None) -> torch.Tensor:
    """ncx_gru_train_forward_flags: gru_encode's q under the same x6 (bit for bit), with the stash of the valid (row, t) pairs left in
    `ws`.  x6: gru_step_form; the backward takes whichever stash the forward left."""
    B, T, wids = _gru_train_args(wids, gw, "gru_train_forward")
    if bad_flag is None:
        bad_flag = gru_bad_flag(wids.device)
    p, n = _ws_ptr(ws)
    q = torch.empty(B, gw.dim_q, dtype=torch.float32, device=wids.device)
    _lib.check(_lib.lib().ncx_gru_train_forward_flags(_ptr(wids, torch.int32, "wids"), B, T, _ptr(gw.E, torch.float32, "E"), gw.V1, gw.dim_emb,
                                                      gw.dim_q, _ptr(gw.packed, torch.float32, "packed"), mlb_att_flags(x6), p, n,
                                                      C.c_void_p(q.data_ptr()), _ptr(bad_flag, torch.int32, "bad_flag"), _stream()),
               "ncx_gru_train_forward")
    return q


GRU_BWD_SWEEP, GRU_BWD_DX, GRU_BWD_DWHH, GRU_BWD_DWIH = 1, 2, 4, 8      # ncx_gru_bwd_form's bits


def gru_bwd_form(dim_emb: int, dim_q: int, B: int, T: int, x6=None) -> int:
    """Which products of gru_train_backward take their bf16 x 6 kernel for this shape (ncx_gru_bwd_form; host only: no launch, no device
    access), as a bit mask: GRU_BWD_SWEEP | GRU_BWD_DX | GRU_BWD_DWHH | GRU_BWD_DWIH; 0 for the fp32 form.  x6: as gru_step_form."""
    rc = _lib.lib().ncx_gru_bwd_form(B, T, dim_emb, dim_q, mlb_att_flags(x6))
    if rc < 0:
        raise _lib.NcxError("ncx_gru_bwd_form: dims out of range (B %d, T %d, dim_emb %d, dim_q %d)" % (B, T, dim_emb, dim_q))
    return rc


def gru_train_backward(wids: torch.Tensor, gw: GruTrainWeights, ws: torch.Tensor, dq_out: torch.Tensor, want_dE: bool = True,
                       dE: Optional[torch.Tensor] = None, x6=None) -> Dict[str, Optional[torch.Tensor]]:
    """ncx_gru_train_backward_flags on the workspace gru_train_forward left for the same wids (under either x6): dq_out [B, dim_q] ->
    {"w_ih", "w_hh", "b_ih", "b_hh", "E"} in torch's layouts; "E" is None when want_dE is off (a fixed embedding).  `dE`: a caller's
    [V + 1, dim_emb] buffer.  x6 (gru_bwd_form): the bf16 x 6 form of the products it names -- fp32-grade, not bit-equal to the fp32 form."""
    B, T, wids = _gru_train_args(wids, gw, "gru_train_backward")
    if tuple(dq_out.shape) != (B, gw.dim_q):
        raise ValueError("dq_out must be [%d, %d], got %s" % (B, gw.dim_q, tuple(dq_out.shape)))
    dev = wids.device
    g = {"w_ih": torch.empty(3 * gw.dim_q, gw.dim_emb, dtype=torch.float32, device=dev),
         "w_hh": torch.empty(3 * gw.dim_q, gw.dim_q, dtype=torch.float32, device=dev),
         "b_ih": torch.empty(3 * gw.dim_q, dtype=torch.float32, device=dev), "b_hh": torch.empty(3 * gw.dim_q, dtype=torch.float32, device=dev),
         "E": None}
    if want_dE:
        g["E"] = dE if dE is not None else torch.empty(gw.V1, gw.dim_emb, dtype=torch.float32, device=dev)
        if tuple(g["E"].shape) != (gw.V1, gw.dim_emb):
            raise ValueError("dE must be [%d, %d], got %s" % (gw.V1, gw.dim_emb, tuple(g["E"].shape)))
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_gru_train_backward_flags(_ptr(wids, torch.int32, "wids"), B, T, _ptr(gw.E, torch.float32, "E"), gw.V1, gw.dim_emb,
                                                       gw.dim_q, _ptr(gw.packed_t, torch.float32, "packed_t"), mlb_att_flags(x6), p, n,
                                                       _ptr(dq_out.float().contiguous(), torch.float32, "dq_out"),
                                                       *[_ptr(g[k], torch.float32, "d" + k) for k in ("w_ih", "w_hh", "b_ih", "b_hh", "E")],
                                                       _stream()),
               "ncx_gru_train_backward")
    return g


# ---- training the two-layer LSTM question encoder (include/neuralcx.h: ncx_lstm2_train_*, ncx_lstm2_pack_t) ------------------------
LSTM_GRADS = ("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1")


def _lstm_t_block(w: torch.Tensor, H: int) -> torch.Tensor:
    """w [4 H, n] -> [pad64(n)][4][Hp] with [j][g][u] = w[g H + u][j], zero padded."""
    n = w.shape[1]
    t = torch.zeros(_pad64(n), 4, _pad32(H), dtype=torch.float32, device=w.device)
    t[:n, :, :H] = w.detach().float().view(4, H, n).permute(2, 0, 1)
    return t


def lstm_pack_t_layout(w_ih0: torch.Tensor, w_hh0: torch.Tensor, w_ih1: torch.Tensor, w_hh1: torch.Tensor) -> torch.Tensor:
    """The layout of ncx_lstm2_pack_t restated with tensor ops (any device; what a test compares the kernel against): the contraction
    runs over the 4 H gate rows, P0 [pad64(H)][8 Hp] | P1 [pad64(H)][4 Hp] | PX [pad64(emb)][4 Hp], P0[j] = W_hh^0[:, j] then W_ih^1[:, j],
    P1[j] = W_hh^1[:, j], PX[c] = W_ih^0[:, c], each as [4 gates][Hp], Hp = pad32(H), zero padded."""
    H = w_hh0.shape[1]
    p0 = torch.cat([_lstm_t_block(w_hh0, H), _lstm_t_block(w_ih1, H)], 1)
    return torch.cat([p0.reshape(-1), _lstm_t_block(w_hh1, H).reshape(-1), _lstm_t_block(w_ih0, H).reshape(-1)])


def lstm_unpack_t_layout(packed_t: torch.Tensor, emb: int, H: int):
    """-> (w_ih0 [4 H, emb], w_hh0, w_ih1, w_hh1 [4 H, H]) read back out of the transposed pack."""
    Hp, rh, rx = _pad32(H), _pad64(H), _pad64(emb)
    n0, n1 = rh * 8 * Hp, rh * 4 * Hp
    back = lambda t, n: t[:n, :, :H].permute(1, 2, 0).reshape(4 * H, n)
    p0 = packed_t[:n0].view(rh, 8, Hp)
    p1 = packed_t[n0:n0 + n1].view(rh, 4, Hp)
    px = packed_t[n0 + n1:].view(rx, 4, Hp)
    return back(px, emb), back(p0[:, :4], H), back(p0[:, 4:], H), back(p1, H)


class LstmTrainWeights:
    """One weight set of the trainable TwoLSTM as ncx_lstm2_train_forward / _backward want it: E, the forward's pack (ncx_lstm2_pack) and the
    backward's transposed pack (ncx_lstm2_pack_t).  Built from E and the eight tensors (rnn_0's w_ih, w_hh, b_ih, b_hh, then rnn_1's), on
    their device."""

    def __init__(self, E, *ws):
        if len(ws) != 8:
            raise ValueError("lstm_train_weights takes E and eight tensors (w_ih, w_hh, b_ih, b_hh of rnn_0, then of rnn_1), got %d" % len(ws))
        ts = [t.detach() for t in (E,) + tuple(ws)]
        if any(t.dtype != torch.float32 for t in ts):
            raise _lib.NcxError("ncx_lstm2_train_* take fp32 parameters")
        E, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1 = ts = [t.contiguous() for t in ts]
        H = w_hh0.shape[1] if w_hh0.dim() == 2 else -1
        ok = E.dim() == 2 and w_ih0.dim() == 2 and tuple(w_ih0.shape) == (4 * H, E.shape[1]) and \
            all(tuple(t.shape) == (4 * H, H) for t in (w_hh0, w_ih1, w_hh1)) and all(tuple(t.shape) == (4 * H,) for t in (b_ih0, b_hh0, b_ih1, b_hh1))
        if not ok:
            raise ValueError("lstm_train_weights takes E [V + 1, emb], w_ih0 [4 H, emb], w_hh0, w_ih1, w_hh1 [4 H, H] and four biases [4 H]; got %s"
                             % ([tuple(t.shape) for t in ts],))
        self.E = E
        self.V1, self.emb = E.shape
        self.H = H
        L = _lib.lib()
        n, nt = L.ncx_lstm2_packed_bytes(self.emb, self.H), L.ncx_lstm2_packed_t_bytes(self.emb, self.H)
        if n == 0 or nt == 0:
            raise _lib.NcxError("ncx_lstm2_pack_t: dims out of range (emb %d, H %d)" % (self.emb, self.H))
        self.packed = torch.empty(n // 4, dtype=torch.float32, device=E.device)
        self.packed_t = torch.empty(nt // 4, dtype=torch.float32, device=E.device)
        with torch.cuda.device(E.device):
            _lib.check(L.ncx_lstm2_pack(*[_ptr(t, torch.float32, "lstm weight") for t in ts[1:]], self.emb, self.H,
                                        C.c_void_p(self.packed.data_ptr()), _stream()), "ncx_lstm2_pack")
            _lib.check(L.ncx_lstm2_pack_t(*[_ptr(t, torch.float32, "lstm weight") for t in (w_ih0, w_hh0, w_ih1, w_hh1)], self.emb, self.H,
                                          C.c_void_p(self.packed_t.data_ptr()), _stream()), "ncx_lstm2_pack_t")


def lstm_train_weights(E, *ws) -> LstmTrainWeights:
    return LstmTrainWeights(E, *ws)


def _lstm_train_args(wids: torch.Tensor, lw: LstmTrainWeights, what: str):
    if wids.dim() != 2:
        raise ValueError("wids must be [B, T], got %s" % (tuple(wids.shape),))
    if wids.is_floating_point():
        raise TypeError("wids must be an integer tensor, got %s" % wids.dtype)
    B, T = wids.shape
    if B < 1 or not 1 <= T <= 64:
        raise ValueError("%s takes B >= 1 questions of 1 <= T <= 64 steps, got [%d, %d]" % (what, B, T))
    if lw.packed.device != wids.device:
        raise _lib.NcxError("wids are on %s, the encoder's weights on %s" % (wids.device, lw.packed.device))
    return B, T, wids.to(torch.int32).contiguous()


def lstm_train_workspace(B: int, T: int, lw: LstmTrainWeights, device) -> torch.Tensor:
    """The workspace of one training step (ncx_lstm2_train_workspace_bytes): the length plan and the stash the backward needs."""
    n = _lib.lib().ncx_lstm2_train_workspace_bytes(B, T, lw.emb, lw.H)
    if n == 0:
        raise _lib.NcxError("ncx_lstm2_train_workspace_bytes: dims out of range")
    return torch.empty(n + 256, dtype=torch.uint8, device=device)


def lstm_train_forward(wids: torch.Tensor, lw: LstmTrainWeights, ws: torch.Tensor, bad_flag: Optional[torch.Tensor] = None, x6=None) -> torch.Tensor:
    """ncx_lstm2_train_forward_flags: lstm_encode's q [B, 2 H] under the same x6 (bit for bit), with the stash of the valid (row, t) pairs
    left in `ws`.  x6: lstm_step_form; the backward takes whichever stash the forward left."""
    B, T, wids = _lstm_train_args(wids, lw, "lstm_train_forward")
    if bad_flag is None:
        bad_flag = gru_bad_flag(wids.device)
    p, n = _ws_ptr(ws)
    q = torch.empty(B, 2 * lw.H, dtype=torch.float32, device=wids.device)
    _lib.check(_lib.lib().ncx_lstm2_train_forward_flags(_ptr(wids, torch.int32, "wids"), B, T, _ptr(lw.E, torch.float32, "E"), lw.V1, lw.emb,
                                                        lw.H, _ptr(lw.packed, torch.float32, "packed"), mlb_att_flags(x6), p, n,
                                                        C.c_void_p(q.data_ptr()), _ptr(bad_flag, torch.int32, "bad_flag"), _stream()),
               "ncx_lstm2_train_forward")
    return q


def lstm_train_backward(wids: torch.Tensor, lw: LstmTrainWeights, ws: torch.Tensor, dq_out: torch.Tensor, want_dE: bool = True,
                        dE: Optional[torch.Tensor] = None, out: Optional[Dict[str, torch.Tensor]] = None) -> Dict[str, Optional[torch.Tensor]]:
    """ncx_lstm2_train_backward on the workspace lstm_train_forward left for the same wids: dq_out [B, 2 H] -> {LSTM_GRADS..., "E"} in
    torch's layouts; "E" is None when want_dE is off (a fixed embedding).  `dE`: a caller's [V + 1, emb] buffer; `out`: caller's buffers
    for the eight weight gradients."""
    B, T, wids = _lstm_train_args(wids, lw, "lstm_train_backward")
    if tuple(dq_out.shape) != (B, 2 * lw.H):
        raise ValueError("dq_out must be [%d, %d], got %s" % (B, 2 * lw.H, tuple(dq_out.shape)))
    dev = wids.device
    shape = {"w_ih0": (4 * lw.H, lw.emb), "w_hh0": (4 * lw.H, lw.H), "w_ih1": (4 * lw.H, lw.H), "w_hh1": (4 * lw.H, lw.H)}
    g = {k: torch.empty(shape.get(k, (4 * lw.H,)), dtype=torch.float32, device=dev) for k in LSTM_GRADS}
    if out is not None:
        for k in LSTM_GRADS:
            if tuple(out[k].shape) != tuple(g[k].shape):
                raise ValueError("d%s must be %s, got %s" % (k, tuple(g[k].shape), tuple(out[k].shape)))
            g[k] = out[k]
    g["E"] = None
    if want_dE:
        g["E"] = dE if dE is not None else torch.empty(lw.V1, lw.emb, dtype=torch.float32, device=dev)
        if tuple(g["E"].shape) != (lw.V1, lw.emb):
            raise ValueError("dE must be [%d, %d], got %s" % (lw.V1, lw.emb, tuple(g["E"].shape)))
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_lstm2_train_backward(_ptr(wids, torch.int32, "wids"), B, T, _ptr(lw.E, torch.float32, "E"), lw.V1, lw.emb, lw.H,
                                                   _ptr(lw.packed_t, torch.float32, "packed_t"), p, n,
                                                   _ptr(dq_out.float().contiguous(), torch.float32, "dq_out"),
                                                   *[_ptr(g[k], torch.float32, "d" + k) for k in LSTM_GRADS + ("E",)], _stream()),
               "ncx_lstm2_train_backward")
    return g


# ---- the trainable scorers LinearContext and PairwiseLinearModel (include/neuralcx.h) -----------------------------------------
PAIRLIN_H = 300                     # dim_h = dim_a = 300 in the reference (cx.py:391-392)
PAIRLIN_FIELDS = ("answer_embedding", "w", "b", "w_out", "b_out")
PAIRLIN_STATE_TO_FIELD = {"answer_embedding.weight": "answer_embedding", "linear.weight": "w", "linear.bias": "b",
                          "out.weight": "w_out", "out.bias": "b_out"}
LINCTX_STATE_TO_FIELD = {"linear.weight": "w", "linear.bias": "b"}


def pairlin_shapes(K, dv, dq, dz, A):
    din = 2 * dv + dq + 2 * dz + PAIRLIN_H                      # cx.py:397-398
    return {"answer_embedding.weight": (A, PAIRLIN_H), "linear.weight": (PAIRLIN_H, din), "linear.bias": (PAIRLIN_H,),
            "out.weight": (1, PAIRLIN_H), "out.bias": (1,)}


def linctx_shapes(K, dz):
    return {"linear.weight": (K, K * dz), "linear.bias": (K,)}        # cx.py:145


def pairlin_dims(batch: Batch, A: int) -> _lib.NcxScorerDims:
    B, K1 = batch.img_idx.shape
    d = _lib.NcxScorerDims()
    d.B, d.K, d.dz, d.A = B, K1 - 1, batch.z_orig.shape[1], A
    d.dv, d.n_img, d.dq = batch.feats.shape[1], batch.feats.shape[0], batch.q_emb.shape[1]
    assert batch.z_knns.shape == (B, d.K, d.dz), batch.z_knns.shape
    assert batch.q_emb.shape[0] == B and batch.z_orig.shape == (B, d.dz)
    assert batch.answer_aids is not None and batch.answer_aids.shape == (B,)
    return d


def linctx_dims(z_knns: torch.Tensor) -> _lib.NcxScorerDims:
    assert z_knns.dim() == 3, z_knns.shape
    d = _lib.NcxScorerDims()
    d.B, d.K, d.dz = z_knns.shape
    return d


def _pl_struct(tensors: Dict[str, torch.Tensor], cls):
    s = cls()
    for f in PAIRLIN_FIELDS:
        setattr(s, f, _ptr(tensors.get(f), torch.float32, f))
    return s


def pairlin_workspace(d, device) -> torch.Tensor:
    n = _lib.lib().ncx_pairlin_workspace_bytes(C.byref(d))
    if n == 0:
        raise _lib.NcxError("ncx_pairlin_workspace_bytes: unsupported dims")
    return torch.empty(n + 256, dtype=torch.uint8, device=device)


def pairlin_forward(d, batch: Batch, params: Dict[str, torch.Tensor], ws: torch.Tensor, bad_flag: Optional[torch.Tensor] = None):
    """PairwiseLinearModel scores [B, K] (ncx_pairlin_forward); leaves h / P / clamped ids in `ws` for pairlin_backward.
    A feature row or answer id out of range sets `bad_flag` (default: semantic_bad_flag(device); check_semantic_ids raises)."""
    dev = batch.z_knns.device
    if bad_flag is None:
        bad_flag = semantic_bad_flag(dev)
    scores = torch.empty(d.B, d.K, dtype=torch.float32, device=dev)
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_pairlin_forward(C.byref(d), C.byref(batch.c_struct()), C.byref(_pl_struct(params, _lib.NcxPairlinParams)),
                                              p, n, C.c_void_p(scores.data_ptr()), _ptr(bad_flag, torch.int32, "bad_flag"), _stream()),
               "ncx_pairlin_forward")
    return scores


def pairlin_backward(d, batch: Batch, params: Dict[str, torch.Tensor], ws: torch.Tensor, dscores: torch.Tensor,
                     grads: Dict[str, torch.Tensor]) -> None:
    """Every gradient of PairwiseLinearModel (ncx_pairlin_backward) into `grads` (field names), after pairlin_forward on `ws`."""
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_pairlin_backward(C.byref(d), C.byref(batch.c_struct()), C.byref(_pl_struct(params, _lib.NcxPairlinParams)),
                                               p, n, _ptr(dscores, torch.float32, "dscores"),
                                               C.byref(_pl_struct(grads, _lib.NcxPairlinGrads)), _stream()),
               "ncx_pairlin_backward")


def linctx_workspace(d, device) -> torch.Tensor:
    n = _lib.lib().ncx_linctx_workspace_bytes(C.byref(d))
    if n == 0:
        raise _lib.NcxError("ncx_linctx_workspace_bytes: unsupported dims")
    return torch.empty(n + 256, dtype=torch.uint8, device=device)


def linctx_forward(d, z_knns: torch.Tensor, w: torch.Tensor, b: torch.Tensor, ws: torch.Tensor) -> torch.Tensor:
    """LinearContext scores [B, K] = z_knns.view(B, K dz) . w^T + b (ncx_linctx_forward)."""
    scores = torch.empty(d.B, d.K, dtype=torch.float32, device=z_knns.device)
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_linctx_forward(C.byref(d), _ptr(z_knns, torch.float32, "z_knns"), _ptr(w, torch.float32, "w"),
                                             _ptr(b, torch.float32, "b"), p, n, C.c_void_p(scores.data_ptr()), _stream()),
               "ncx_linctx_forward")
    return scores


def linctx_backward(d, z_knns: torch.Tensor, dscores: torch.Tensor, ws: torch.Tensor, gw: torch.Tensor, gb: torch.Tensor) -> None:
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_linctx_backward(C.byref(d), _ptr(z_knns, torch.float32, "z_knns"), _ptr(dscores, torch.float32, "dscores"),
                                              p, n, _ptr(gw, torch.float32, "gw"), _ptr(gb, torch.float32, "gb"), _stream()),
               "ncx_linctx_backward")

# ---- the contrastive path: ContrastiveModel + ContrastiveLoss (include/neuralcx.h) ----------------------------------------------
CONTRASTIVE_H = 300                 # dim_h = dim_a = 300 (cx.py:437-439)
CONTRASTIVE_MARGIN = 2.0            # ContrastiveLoss(margin=2.0), contrastive.py:300
# answer_embedding.weight is constructed and saved but never read (cx.py:440-441, 458): it has no C ABI field
CONTRASTIVE_STATE_TO_FIELD = {"linear.weight": "w", "linear.bias": "b"}


def contrastive_shapes(dv, dz, A):
    """state_dict of ContrastiveModel, in the order Adam's span is cut: linear.* first (trained), the embedding last (never)."""
    return {"linear.weight": (CONTRASTIVE_H, dv + dz), "linear.bias": (CONTRASTIVE_H,), "answer_embedding.weight": (A, CONTRASTIVE_H)}


def contrastive_dims(batch: Batch) -> _lib.NcxContrastiveDims:
    """batch.img_idx [B, P], z_orig [B, dz], z_knns [B, P - 1, dz]; q_emb / a_knns / answer_aids are not read."""
    B, P = batch.img_idx.shape
    d = _lib.NcxContrastiveDims()
    d.B, d.P, d.dv, d.dz, d.n_img = B, P, batch.feats.shape[1], batch.z_orig.shape[1], batch.feats.shape[0]
    assert batch.z_orig.shape == (B, d.dz) and batch.z_knns.shape == (B, P - 1, d.dz), (batch.z_orig.shape, batch.z_knns.shape)
    return d


def contrastive_workspace(d, device) -> torch.Tensor:
    n = _lib.lib().ncx_contrastive_workspace_bytes(C.byref(d))
    if n == 0:
        raise _lib.NcxError("ncx_contrastive_workspace_bytes: unsupported dims (1 <= P - 1 <= 64, dv >= 4, dz >= 4)")
    return torch.empty(n + 256, dtype=torch.uint8, device=device)


def _contrastive_inputs(batch: Batch) -> NcxInputs:
    s = NcxInputs()
    s.feats = _ptr(batch.feats, torch.float32, "feats")
    s.img_idx = _ptr(batch.img_idx, torch.int32, "img_idx")
    s.z_orig = _ptr(batch.z_orig, torch.float32, "z_orig")
    s.z_knns = _ptr(batch.z_knns, torch.float32, "z_knns")
    return s


def contrastive_forward(d, batch: Batch, w: torch.Tensor, b: torch.Tensor, ws: torch.Tensor, bad_flag: Optional[torch.Tensor] = None,
                        want_h: bool = True) -> Optional[torch.Tensor]:
    """h [B, P, 300] = relu(linear(cat(v, z))) (ncx_contrastive_forward); h, the clamped row ids and z stay in `ws` for
    contrastive_distances / _loss / _backward.  want_h = False: nothing is copied out (the engine's steps read the workspace).
    A feature row out of range sets `bad_flag` (default: semantic_bad_flag(device); check_semantic_ids raises)."""
    dev = batch.z_knns.device
    if bad_flag is None:
        bad_flag = semantic_bad_flag(dev)
    h = torch.empty(d.B, d.P, CONTRASTIVE_H, dtype=torch.float32, device=dev) if want_h else None
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_contrastive_forward(C.byref(d), C.byref(_contrastive_inputs(batch)), _ptr(w, torch.float32, "w"),
                                                  _ptr(b, torch.float32, "b"), p, n, _ptr(h, torch.float32, "h"),
                                                  _ptr(bad_flag, torch.int32, "bad_flag"), _stream()), "ncx_contrastive_forward")
    return h


def contrastive_distances(d, ws: Optional[torch.Tensor] = None, h: Optional[torch.Tensor] = None) -> torch.Tensor:
    """dist [B, P - 1] = ||h_0 - h_k + 1e-6|| (get_scores, cx.py:478-487) from the h contrastive_forward left in `ws`, or from a
    given h [B, P, 300]."""
    dev = h.device if h is not None else ws.device
    dist = torch.empty(d.B, d.P - 1, dtype=torch.float32, device=dev)
    p, n = _ws_ptr(ws) if ws is not None else (None, 0)
    _lib.check(_lib.lib().ncx_contrastive_distances(C.byref(d), _ptr(h, torch.float32, "h"), p, n, C.c_void_p(dist.data_ptr()), _stream()),
               "ncx_contrastive_distances")
    return dist


def contrastive_loss(d, ws: torch.Tensor, scale: Optional[float] = None, margin: float = CONTRASTIVE_MARGIN):
    """The two ContrastiveLoss terms of a P = 3 batch (contrastive.py:217-219) and the gradient down to the pre-activation (left in
    `ws`).  -> dict(loss_comp, loss_other, loss, dist_comp, dist_other: 0-d device tensors; dist [B, 2])."""
    dev = ws.device
    out = torch.empty(4, dtype=torch.float32, device=dev)
    dist = torch.empty(d.B, 2, dtype=torch.float32, device=dev)
    p, n = _ws_ptr(ws)
    _lib.check(_lib.lib().ncx_contrastive_loss(C.byref(d), p, n, float(margin), float(1.0 / d.B if scale is None else scale),
                                               C.c_void_p(out.data_ptr()), C.c_void_p(dist.data_ptr()), _stream()), "ncx_contrastive_loss")
    return dict(loss_comp=out[0], loss_other=out[1], loss=out[0] + out[1], dist_comp=out[2], dist_other=out[3], dist=dist)


def contrastive_backward(d, batch: Batch, ws: torch.Tensor, gw: torch.Tensor, gb: torch.Tensor, dh: Optional[torch.Tensor] = None) -> None:
    """d linear.weight / d linear.bias (ncx_contrastive_backward) from the pre-activation gradient contrastive_loss left in `ws`, or
    from an outside gradient dh [B, P, 300] with respect to h."""
    p, n = _ws_ptr(ws)
    s = NcxInputs()
    s.feats = _ptr(batch.feats, torch.float32, "feats")
    _lib.check(_lib.lib().ncx_contrastive_backward(C.byref(d), C.byref(s), p, n, _ptr(dh, torch.float32, "dh"), _ptr(gw, torch.float32, "gw"),
                                                   _ptr(gb, torch.float32, "gb"), _stream()), "ncx_contrastive_backward")


# ---- training the MutanNoAtt VQA model (include/neuralcx.h: ncx_vqa_train_*, ncx_ce_loss) ---------------------------------
MUTAN_FIELDS = ("wv", "bv", "wq", "bq", "whv", "bhv", "whq", "bhq", "wc", "bc")
VT_WS_VD, VT_WS_QD, VT_WS_ZC = 1, 2, 3
VT_LAYERS = dict(v=1, q=2, z=3)          # layer ids of the counter-based dropout generator


def mutan_shapes(dv, dq, dhv, dhq, dz, R, A):
    """Field -> shape of the stacked MutanNoAtt layout (MutanWeights / ncx_mutan_params), in flat-buffer order."""
    return dict(wv=(dhv, dv), bv=(dhv,), wq=(dhq, dq), bq=(dhq,), whv=(R * dz, dhv), bhv=(R * dz,), whq=(R * dz, dhq), bhq=(R * dz,),
                wc=(A, dz), bc=(A,))


def vqa_train_dims(B, dv, dq, dz, A, n_img, p=(0.0, 0.0, 0.0), dropout_mode=0, seed=0, want_dq=False) -> _lib.NcxVqaTrainDims:
    d = _lib.NcxVqaTrainDims()
    d.B, d.dv, d.dq, d.dz, d.A, d.n_img = int(B), int(dv), int(dq), int(dz), int(A), int(n_img)
    d.p_v, d.p_q, d.p_c = (float(x) for x in p)
    d.dropout_mode, d.want_dq, d.seed = int(dropout_mode), int(bool(want_dq)), int(seed) & 0xFFFFFFFFFFFFFFFF
    return d


def _train_workspace(sym, d, mw, device) -> torch.Tensor:
    m = mw.c_struct()
    need = getattr(_lib.lib(), sym)(C.byref(d), C.byref(m))
    if need == 0:
        raise _lib.NcxError("%s: unsupported dims or activation" % sym)
    return torch.empty(need + 256, dtype=torch.uint8, device=device)


def _train_forward(sym, d, feats, img_idx, q_emb, mw, ws, masks):
    m = mw.c_struct()
    logits = torch.empty(d.B, d.A, dtype=torch.float32, device=feats.device)
    z = torch.empty(d.B, d.dz, dtype=torch.float32, device=feats.device)
    p, n = _ws_ptr(ws)
    _lib.check(getattr(_lib.lib(), sym)(C.byref(d), _ptr(feats, torch.float32, "feats"), _ptr(img_idx, torch.int32, "img_idx"),
                                        _ptr(q_emb, torch.float32, "q_emb"), C.byref(m), _ptr(masks, torch.float32, "masks"), p, n,
                                        C.c_void_p(logits.data_ptr()), C.c_void_p(z.data_ptr()), _stream()), sym)
    return logits, z


def _train_backward(sym, grads_cls, fields, d, mw, ws, dlogits, grads, masks):
    m = mw.c_struct()
    g = grads_cls()
    for k in fields:
        setattr(g, k, _ptr(grads[k], torch.float32, "grad " + k))
    dq = torch.empty(d.B, d.dq, dtype=torch.float32, device=dlogits.device) if d.want_dq else None
    p, n = _ws_ptr(ws)
    _lib.check(getattr(_lib.lib(), sym)(C.byref(d), C.byref(m), _ptr(masks, torch.float32, "masks"), p, n,
                                        _ptr(dlogits, torch.float32, "dlogits"), C.byref(g), _ptr(dq, torch.float32, "dq_emb"), _stream()), sym)
    return dq


def _train_ws_view(sym, d, mw, ws, which) -> torch.Tensor:
    m = mw.c_struct()
    off, nb = C.c_size_t(), C.c_size_t()
    _lib.check(getattr(_lib.lib(), sym)(C.byref(d), C.byref(m), which, C.byref(off), C.byref(nb)), sym)
    pad = (-ws.data_ptr()) % 256
    return ws[pad + off.value: pad + off.value + nb.value].view(torch.float32).view(d.B, -1)


def vqa_train_workspace(d, mw, device) -> torch.Tensor:
    return _train_workspace("ncx_vqa_train_workspace_bytes", d, mw, device)


def vqa_train_forward(d, feats, img_idx, q_emb, mw, ws, masks=None):
    """Training-mode fusion + classifier (ncx_vqa_train_forward) -> (logits [B, A], z [B, dz]); the stashes stay in ws."""
    return _train_forward("ncx_vqa_train_forward", d, feats, img_idx, q_emb, mw, ws, masks)


def vqa_train_backward(d, mw, ws, dlogits, grads: Dict[str, torch.Tensor], masks=None):
    """Every gradient of MUTAN_FIELDS into `grads` (overwritten); -> d loss / d q_emb [B, dq] when d.want_dq, else None."""
    return _train_backward("ncx_vqa_train_backward", _lib.NcxMutanGrads, MUTAN_FIELDS, d, mw, ws, dlogits, grads, masks)


def vqa_train_ws_view(d, mw, ws, which) -> torch.Tensor:
    """The tensor the forward dropped (VT_WS_VD / _QD / _ZC) as a [B, width] view of the workspace (tests, diagnostics)."""
    return _train_ws_view("ncx_vqa_train_ws_region", d, mw, ws, which)


# ---- training the MLBNoAtt VQA model (include/neuralcx.h: ncx_mlb_train_*): the same dims struct, loss and optimiser ----------
MLB_FIELDS = ("wv", "bv", "wq", "bq", "wc", "bc")
MlbGrads = _lib.NcxMlbGrads


def mlb_shapes(dv, dq, dh, A):
    """Field -> shape of the MLBNoAtt layout (MlbWeights / ncx_mlb_params), in flat-buffer order."""
    return dict(wv=(dh, dv), bv=(dh,), wq=(dh, dq), bq=(dh,), wc=(A, dh), bc=(A,))


def mlb_train_workspace(d, mw, device) -> torch.Tensor:
    return _train_workspace("ncx_mlb_train_workspace_bytes", d, mw, device)


def mlb_train_forward(d, feats, img_idx, q_emb, mw, ws, masks=None):
    """Training-mode MLB fusion + classifier (ncx_mlb_train_forward) -> (logits [B, A], z [B, dh] before classif.activation)."""
    return _train_forward("ncx_mlb_train_forward", d, feats, img_idx, q_emb, mw, ws, masks)


def mlb_train_backward(d, mw, ws, dlogits, grads: Dict[str, torch.Tensor], masks=None):
    """Every gradient of MLB_FIELDS into `grads` (overwritten); -> d loss / d q_emb [B, dq] when d.want_dq, else None."""
    return _train_backward("ncx_mlb_train_backward", MlbGrads, MLB_FIELDS, d, mw, ws, dlogits, grads, masks)


def mlb_train_ws_region(d, mw, ws, which) -> torch.Tensor:
    """The tensor the forward dropped (VT_WS_VD / _QD; VT_WS_ZC: drop_c(act_c(z))) as a [B, width] view of the workspace."""
    return _train_ws_view("ncx_mlb_train_ws_region", d, mw, ws, which)


# ---- training the MLBAtt attention model (include/neuralcx.h: ncx_mlb_att_train_*) ---------------------------------------------
AT_WS_XV, AT_WS_VATT, AT_WS_T, AT_WS_VD, AT_WS_DWV = 1, 2, 3, 4, 5
AT_LAYERS = dict(att_v=1, att_q=2, att_mm=3, v=4, q=5, c=6)      # layer ids of the counter-based dropout generator


def mlb_att_dropouts(opt):
    """The six dropout p's of an MLBAtt's options in layer order (attention.dropout_v/_q/_mm, fusion.dropout_v/_q, classif.dropout)."""
    att, fus, cla = opt["attention"], opt["fusion"], opt.get("classif", {})
    return tuple(float(x or 0.0) for x in (att.get("dropout_v"), att.get("dropout_q"), att.get("dropout_mm"), fus.get("dropout_v"),
                                           fus.get("dropout_q"), cla.get("dropout")))


def mlb_att_mask_sizes(B, P, dv, dq, dh_att, G, dh_f):
    """Element counts of the six keep masks of dropout_mode 2, in the order they are concatenated."""
    return (B * dv * P, B * dq, B * P * dh_att, B * G * dv, B * dq, B * G * dh_f)


def mlb_att_train_dims(mw: MlbAttWeights, B, P, n_img, p=(0.0,) * 6, dropout_mode=0, seed=0, want_dq=False):
    """-> (ncx_mlb_att_dims, ncx_mlb_att_train) of one training step."""
    t = _lib.NcxMlbAttTrain()
    t.p_att_v, t.p_att_q, t.p_att_mm, t.p_v, t.p_q, t.p_c = (float(x) for x in p)
    t.dropout_mode, t.want_dq, t.seed = int(dropout_mode), int(bool(want_dq)), int(seed) & 0xFFFFFFFFFFFFFFFF
    return mw.dims(int(B), int(P), int(n_img)), t


def mlb_att_train_dims_ok(mw: MlbAttWeights, dt) -> bool:
    """The library's own check of the shape and the dropout settings (host only)."""
    return _lib.lib().ncx_mlb_att_train_workspace_bytes(C.byref(dt[0]), C.byref(dt[1]), C.byref(mw.c_struct(check_device=False))) != 0


def mlb_att_train_workspace(dt, mw: MlbAttWeights, device) -> torch.Tensor:
    need = _lib.lib().ncx_mlb_att_train_workspace_bytes(C.byref(dt[0]), C.byref(dt[1]), C.byref(mw.c_struct()))
    if need == 0:
        raise _lib.NcxError("ncx_mlb_att_train_workspace_bytes: unsupported dims, dropout settings or activation")
    return torch.empty(need + 256, dtype=torch.uint8, device=device)


def mlb_att_train_forward(dt, feats, img_idx, q_emb, mw: MlbAttWeights, ws, masks=None, x6=None):
    """Training-mode MLBAtt below the question encoder (ncx_mlb_att_train_forward_flags) -> (logits [B, A], att [B, G, P]); the stashes
    stay in ws.  feats [n_img, dv, W, H] or [n_img, dv, P], read in place; img_idx [B] int32.  x6: mlb_att_flags."""
    d, t = dt
    logits = torch.empty(d.B, d.A, dtype=torch.float32, device=feats.device)
    att = torch.empty(d.B, d.G, d.P, dtype=torch.float32, device=feats.device)
    p, n = _ws_ptr(ws)
    with torch.cuda.device(feats.device):
        _lib.check(_lib.lib().ncx_mlb_att_train_forward_flags(C.byref(d), C.byref(t), _ptr(feats, torch.float32, "feats"),
                                                              _ptr(img_idx, torch.int32, "img_idx"), _ptr(q_emb, torch.float32, "q_emb"),
                                                              C.byref(mw.c_struct()), _ptr(masks, torch.float32, "masks"), mlb_att_flags(x6),
                                                              p, n, C.c_void_p(logits.data_ptr()), C.c_void_p(att.data_ptr()), _stream()),
                   "ncx_mlb_att_train_forward_flags")
    return logits, att


MLB_ATT_DWV_FORMS = ("small", "fp32", "x6")


def mlb_att_dwv_form(mw: MlbAttWeights, B: int, P: int, n_img: int, x6=None) -> str:
    """Which kernel d conv_v_att.weight takes for this shape (ncx_mlb_att_dwv_form; host only: no launch, no device access)."""
    d = mw.dims(B, P, n_img)
    rc = _lib.lib().ncx_mlb_att_dwv_form(C.byref(d), mlb_att_flags(x6))
    if rc < 0:
        _lib.check(rc, "ncx_mlb_att_dwv_form")
    return MLB_ATT_DWV_FORMS[rc]


def mlb_att_train_backward(dt, feats, img_idx, q_emb, mw: MlbAttWeights, ws, att, dlogits, grads: Dict[str, torch.Tensor], masks=None, x6=None):
    """Every gradient of MLB_ATT_FIELDS into `grads` (overwritten) after mlb_att_train_forward on the same workspace and inputs
    (ncx_mlb_att_train_backward_flags; x6: mlb_att_flags, independent of the forward's); -> d loss / d q_emb [B, dq] when want_dq,
    else None."""
    d, t = dt
    g = _lib.NcxMlbAttGrads()
    for k in MLB_ATT_FIELDS:
        setattr(g, k, _ptr(grads[k], torch.float32, "grad " + k))
    dq = torch.empty(d.B, d.dq, dtype=torch.float32, device=dlogits.device) if t.want_dq else None
    p, n = _ws_ptr(ws)
    with torch.cuda.device(dlogits.device):
        _lib.check(_lib.lib().ncx_mlb_att_train_backward_flags(C.byref(d), C.byref(t), _ptr(feats, torch.float32, "feats"),
                                                               _ptr(img_idx, torch.int32, "img_idx"), _ptr(q_emb, torch.float32, "q_emb"),
                                                               C.byref(mw.c_struct()), _ptr(masks, torch.float32, "masks"), mlb_att_flags(x6),
                                                               p, n, _ptr(att, torch.float32, "att"), _ptr(dlogits, torch.float32, "dlogits"),
                                                               C.byref(g), _ptr(dq, torch.float32, "dq_emb"), _stream()),
                   "ncx_mlb_att_train_backward_flags")
    return dq


def mlb_att_train_ws_region(dt, mw: MlbAttWeights, ws, which) -> torch.Tensor:
    """A region of the workspace (AT_WS_XV / _VATT / _T / _VD / _DWV) as a flat fp32 view (tests, diagnostics)."""
    off, nb = C.c_size_t(), C.c_size_t()
    _lib.check(_lib.lib().ncx_mlb_att_train_ws_region(C.byref(dt[0]), C.byref(dt[1]), C.byref(mw.c_struct()), which, C.byref(off), C.byref(nb)),
               "ncx_mlb_att_train_ws_region")
    pad = (-ws.data_ptr()) % 256
    return ws[pad + off.value: pad + off.value + nb.value].view(torch.float32)


_VQA_FLAGS: Dict[torch.device, torch.Tensor] = {}


def vqa_bad_flag(device) -> torch.Tensor:
    """The per-device int32 flag ncx_ce_loss sets on a target outside [0, A) (sticky until checked)."""
    device = torch.device(device)
    if device.type == "cuda" and device.index is None:
        device = torch.device("cuda", torch.cuda.current_device())
    f = _VQA_FLAGS.get(device)
    if f is None:
        f = _VQA_FLAGS[device] = torch.zeros(1, dtype=torch.int32, device=device)
    return f


def ce_loss(logits: torch.Tensor, target: torch.Tensor, scale: float = 0.0, want_grad: bool = True, bad_flag=None):
    """Mean cross-entropy, its gradient and the top-1 / top-5 hit counts (ncx_ce_loss) on the current stream, no host sync.
    -> dict(loss [1], dlogits [B, A] or None, hits1 [1] int32, hits5 [1] int32).  scale <= 0: 1 / B."""
    B, A = logits.shape
    dev = logits.device
    if bad_flag is None:
        bad_flag = vqa_bad_flag(dev)
    loss = torch.empty(1, dtype=torch.float32, device=dev)
    hits = torch.empty(2, dtype=torch.int32, device=dev)
    rows = torch.empty(2 * B, dtype=torch.float32, device=dev)
    dlogits = torch.empty(B, A, dtype=torch.float32, device=dev) if want_grad else None
    _lib.check(_lib.lib().ncx_ce_loss(_ptr(logits, torch.float32, "logits"), _ptr(target, torch.int32, "target"), B, A, float(scale),
                                      C.c_void_p(loss.data_ptr()), _ptr(dlogits, torch.float32, "dlogits"), C.c_void_p(hits.data_ptr()),
                                      C.c_void_p(hits.data_ptr() + 4), _ptr(bad_flag, torch.int32, "bad_flag"), C.c_void_p(rows.data_ptr()),
                                      _stream()), "ncx_ce_loss")
    return dict(loss=loss, dlogits=dlogits, hits1=hits[0:1], hits5=hits[1:2])


def check_vqa_targets(bad_flag: Optional[torch.Tensor] = None, device=None) -> None:
    """Raises IndexError (nn.CrossEntropyLoss raises there) if a ce_loss call since the last check saw a target outside [0, A);
    clears the flag.  Synchronises with the flag's stream."""
    if bad_flag is None:
        bad_flag = vqa_bad_flag(device if device is not None else "cuda")
    if int(bad_flag.item()):
        bad_flag.zero_()
        raise IndexError("target outside [0, A) in a ce_loss call")


class WorkspacePool:
    """Workspaces (saved activations + scratch of ncx_forward / ncx_backward) of one module.  A workspace is OWNED by the
    call that took it until that call's backward has been enqueued (or, for a call that needs no gradient, until its
    forward has been enqueued -- the stream orders the reuse); only then does it return to the pool.  Two forwards
    before a backward therefore never share saved activations (the reference module has no such limit either:
    counterexamples.py:357-361 evaluates inside the train loop)."""

    def __init__(self):
        self.free = []

    def take(self, nbytes: int, device) -> torch.Tensor:
        for i, w in enumerate(self.free):
            if w.numel() >= nbytes and w.device == device:
                return self.free.pop(i)
        self.free.clear()                       # (sizes changed: drop the stale buffers)
        return torch.empty(nbytes, dtype=torch.uint8, device=device)

    def give(self, ws: torch.Tensor) -> None:
        if len(self.free) < 2:
            self.free.append(ws)


class NeuralCXFunction(torch.autograd.Function):
    """scores = NeuralCX(batch; params) with the hand-written backward (ncx_backward).
    `call` = {dims, batch, names, pool, record}: a per-call snapshot -- backward reads the dims / inputs / workspace of ITS
    forward from ctx, never from shared module state."""

    @staticmethod
    def forward(ctx, call, *param_tensors):
        d, batch, names, pool = call["dims"], call["batch"], call["names"], call["pool"]
        params = dict(zip(names, param_tensors))
        ws = pool.take(workspace_bytes(d) + 256, batch.feats.device)
        scores = forward(d, batch, params, ws)
        if call["record"]:                      # (ctx.needs_input_grad stays True under torch.no_grad: the caller tells)
            ctx.call, ctx.ws = dict(call), ws
            ctx.save_for_backward(*param_tensors)
        else:
            pool.give(ws)                       # no graph is recorded (torch.no_grad / frozen parameters)
        return scores

    @staticmethod
    def backward(ctx, dscores):
        call = ctx.call
        if ctx.ws is None:
            raise RuntimeError("NeuralCXFunction: backward ran twice on one forward (retain_graph is not supported: "
                               "the saved activations live in a workspace that has been released)")
        d, batch, names = call["dims"], call["batch"], call["names"]
        params = dict(zip(names, ctx.saved_tensors))
        gbuf = {n: torch.empty_like(t) for n, t in params.items()}
        backward(d, batch, params, ctx.ws, dscores.contiguous(), gbuf)
        call["pool"].give(ctx.ws)
        ctx.ws = None
        return (None,) + tuple(gbuf[n] for n in names)


# ---- diagnostics: the generic GEMM engine called directly (include/neuralcx.h: ncx_diag_gemm) ------------------------------------
GEMM_FORMS = ("NT", "TN", "NN")
GEMM_TILES = ("64x64", "128x128", "96x128", "96x64", "128x64")          # tile cfg codes


def diag_cfg_supported(form: int, cfg: int) -> bool:
    return bool(_lib.lib().ncx_diag_cfg_supported(form, cfg))


def diag_plan_gemm(form: int, M: int, N: int, ksteps: int, allow_96: bool = False) -> dict:
    """plan_gemm: the tile config and k-split the planner gives an M x N product of `ksteps` 32-deep steps (host only)."""
    out = (C.c_int32 * 2)()
    _lib.check(_lib.lib().ncx_diag_plan_gemm(form, M, N, ksteps, int(allow_96), out), "ncx_diag_plan_gemm")
    return dict(cfg=int(out[0]), tile=GEMM_TILES[out[0]], split=int(out[1]))


def diag_gemm_slab_bytes(a: _lib.NcxDiagGemmArgs) -> int:
    return int(_lib.lib().ncx_diag_gemm_slab_bytes(C.byref(a)))


def diag_gemm_rc(a: _lib.NcxDiagGemmArgs, stream=None) -> int:
    """One launch of the engine as `a` describes it, on torch's current stream; -> the status code (a rejected description launches nothing,
    so this needs no device for one)."""
    return int(_lib.lib().ncx_diag_gemm(C.byref(a), _stream() if stream is None else stream))


def diag_gemm(a: _lib.NcxDiagGemmArgs) -> None:
    _lib.check(diag_gemm_rc(a), "ncx_diag_gemm")
