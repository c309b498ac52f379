"""Training the no-attention VQA models, MutanNoAtt and MLBNoAtt (reference train.py:136-145, vqa/lib/engine.py:6-56): the producers
of the best_model.pth.tar the counterexample pipeline loads.

MutanTrainFunction is the differentiable fusion + classifier (ncx_vqa_train_forward / _backward) for a caller that keeps torch
autograd around it -- the module route of vqa.models.noatt.MutanNoAtt (`use_hip_train`), where the question encoder trains under
autograd from the d loss / d q_emb the backward returns.  VqaTrainEngine is the whole step in HIP on flat buffers: forward,
cross-entropy (ncx_ce_loss), backward, Adam (ncx_adam_step), for a frozen or externally trained encoder.  MlbTrainFunction,
mlb_module_forward and MlbTrainEngine are the same three for MLBNoAtt (ncx_mlb_train_forward / _backward); the two engines share
everything but their parameter layout.
"""
import math
from typing import Dict, Optional

import torch

from . import ops
from .engine import FlatParams

ACT_CODE = {None: 0, "tanh": 2}


def route_for(opt) -> str:
    """"hip" when the MutanNoAtt options `opt` are the model ncx_vqa_train_* supports, else "torch path: <why>".  Reads the
    options only (never touches the library)."""
    f = opt.get("fusion", {})
    for k in ("activation_hv", "activation_hq", "activation_mm"):
        if k in f:
            return "torch path: fusion.%s is not supported in HIP" % k
    for k in ("activation_v", "activation_q"):
        if f.get(k) not in ACT_CODE:
            return "torch path: fusion.%s = %r (HIP supports none / tanh)" % (k, f.get(k))
    for k in ("dropout_hv", "dropout_hq"):
        if float(f.get(k, 0.0)) > 0:
            return "torch path: fusion.%s > 0 is not supported in HIP" % k
    if "activation" in opt.get("classif", {}):
        return "torch path: classif.activation is not supported in HIP"
    for k in ("dim_v", "dim_q", "dim_hv", "dim_hq", "dim_mm", "R"):
        if k not in f:
            return "torch path: fusion.%s is missing" % k
    if not 1 <= int(f["R"]) <= 10:
        return "torch path: fusion.R outside 1..10"
    return "hip"


def dropouts(opt):
    return (float(opt["fusion"].get("dropout_v", 0.0)), float(opt["fusion"].get("dropout_q", 0.0)), float(opt["classif"].get("dropout", 0.0)))


class MutanTrainFunction(torch.autograd.Function):
    """logits = classif(fusion(feats[img_idx], q_emb)) with the ten parameter tensors in the stacked MutanWeights layout
    (ops.MUTAN_FIELDS order).  Gradients: the parameters, and q_emb when it requires grad.  cfg = (R, act_v, act_q, (p_v, p_q,
    p_c), seed, training): dropout runs on the counter-based generator under `seed` when training."""

    @staticmethod
    def forward(ctx, feats, img_idx, q_emb, wv, bv, wq, bq, whv, bhv, whq, bhq, wc, bc, cfg):
        R, act_v, act_q, p, seed, training = cfg
        t = {k: x.detach().float().contiguous() for k, x in zip(ops.MUTAN_FIELDS, (wv, bv, wq, bq, whv, bhv, whq, bhq, wc, bc))}
        mw = ops.MutanWeights.from_tensors(t, R, act_v, act_q)
        mode = 1 if training and any(x > 0 for x in p) else 0
        d = ops.vqa_train_dims(img_idx.shape[0], feats.shape[1], q_emb.shape[1], mw.dz, mw.A, feats.shape[0], p=p if mode else (0, 0, 0),
                               dropout_mode=mode, seed=seed, want_dq=ctx.needs_input_grad[2])
        ws = ops.vqa_train_workspace(d, mw, feats.device)
        logits, z = ops.vqa_train_forward(d, feats.detach().float().contiguous(), img_idx, q_emb.detach().float().contiguous(), mw, ws)
        ctx.hip = (d, mw, ws)
        ctx.z = z
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        d, mw, ws = ctx.hip
        grads = {k: torch.empty_like(v) for k, v in mw.t.items()}
        dq = ops.vqa_train_backward(d, mw, ws, dlogits.float().contiguous(), grads)
        return (None, None, dq) + tuple(grads[k] for k in ops.MUTAN_FIELDS) + (None,)


class GruTrainFunction(torch.autograd.Function):
    """q = the hidden state after each question's last word (GRUEncoder below its dropout) through ncx_gru_train_forward / _backward.
    Inputs: wids, E, w_ih, w_hh, b_ih, b_hh and the encoder module, on which the packs are cached (keyed on data_ptr / _version of the
    five tensors, like GRUEncoder._hip_weights: rebuilt after an optimizer step).  Gradients: the five tensors; None for E when it does
    not require grad (a fixed embedding: the dX product is skipped).  module.hip_x6 is read once, in forward, and picks the form of the
    forward's step kernel (ops.gru_step_form) and of the backward's products (ops.gru_bwd_form): one step runs under one choice."""

    @staticmethod
    def weights(module, tensors):
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        hit = module.__dict__.get("_hip_gru_train") if module is not None else None
        if hit is None or hit[0] != key:
            hit = (key, ops.gru_train_weights(*tensors))
            if module is not None:
                module.__dict__["_hip_gru_train"] = hit
        return hit[1]

    @staticmethod
    def forward(ctx, wids, E, w_ih, w_hh, b_ih, b_hh, module=None):
        gw = GruTrainFunction.weights(module, (E, w_ih, w_hh, b_ih, b_hh))
        ws = ops.gru_train_workspace(wids.shape[0], wids.shape[1], gw, wids.device)
        x6 = getattr(module, "hip_x6", None)
        q = ops.gru_train_forward(wids, gw, ws, x6=x6)
        ctx.hip = (wids, gw, ws, x6)
        return q

    @staticmethod
    def backward(ctx, dq):
        wids, gw, ws, x6 = ctx.hip
        g = ops.gru_train_backward(wids, gw, ws, dq, want_dE=ctx.needs_input_grad[1], x6=x6)
        ctx.hip = None                                            # the stash is the step's largest buffer: let go of it here
        return None, g["E"], g["w_ih"], g["w_hh"], g["b_ih"], g["b_hh"], None


class LstmTrainFunction(torch.autograd.Function):
    """q = [h^0 | h^1] after each question's last word (TwoLSTM below its dropout) through ncx_lstm2_train_forward / _backward.
    Inputs: wids, E, rnn_0's w_ih, w_hh, b_ih, b_hh, rnn_1's four and the encoder module, on which the packs are cached (keyed on
    data_ptr / _version of the nine tensors, like GruTrainFunction: rebuilt after an optimizer step).  Gradients: the nine tensors;
    None for E when it does not require grad (a fixed embedding: the dX product is skipped).  The forward's step kernel follows
    module.hip_x6 (ops.lstm_step_form)."""

    @staticmethod
    def weights(module, tensors):
        key = tuple((t.data_ptr(), t._version) for t in tensors)
        hit = module.__dict__.get("_hip_lstm_train") if module is not None else None
        if hit is None or hit[0] != key:
            hit = (key, ops.lstm_train_weights(*tensors))
            if module is not None:
                module.__dict__["_hip_lstm_train"] = hit
        return hit[1]

    @staticmethod
    def forward(ctx, wids, E, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1, module=None):
        lw = LstmTrainFunction.weights(module, (E, w_ih0, w_hh0, b_ih0, b_hh0, w_ih1, w_hh1, b_ih1, b_hh1))
        ws = ops.lstm_train_workspace(wids.shape[0], wids.shape[1], lw, wids.device)
        q = ops.lstm_train_forward(wids, lw, ws, x6=getattr(module, "hip_x6", None))
        ctx.hip = (wids, lw, ws)
        return q

    @staticmethod
    def backward(ctx, dq):
        wids, lw, ws = ctx.hip
        g = ops.lstm_train_backward(wids, lw, ws, dq, want_dE=ctx.needs_input_grad[1])
        ctx.hip = None                                            # the stash is the step's largest buffer: let go of it here
        return (None, g["E"]) + tuple(g[k] for k in ops.LSTM_GRADS) + (None,)


def module_forward(model, input_v: torch.Tensor, q_emb: torch.Tensor) -> torch.Tensor:
    """The HIP route of MutanNoAtt.forward below seq2vec: the rows of input_v are the feature table, the index the identity."""
    f, opt = model.fusion, model.opt
    idx = torch.arange(input_v.shape[0], dtype=torch.int32, device=input_v.device)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if model.training else 0      # torch's CPU generator: torch.manual_seed reproduces it
    cfg = (int(opt["fusion"]["R"]), ACT_CODE[opt["fusion"].get("activation_v")], ACT_CODE[opt["fusion"].get("activation_q")],
           dropouts(opt), seed, bool(model.training))
    return MutanTrainFunction.apply(input_v, idx, q_emb, f.linear_v.weight, f.linear_v.bias, f.linear_q.weight, f.linear_q.bias,
                                    torch.cat([l.weight for l in f.list_linear_hv]), torch.cat([l.bias for l in f.list_linear_hv]),
                                    torch.cat([l.weight for l in f.list_linear_hq]), torch.cat([l.bias for l in f.list_linear_hq]),
                                    model.linear_classif.weight, model.linear_classif.bias, cfg)


def mlb_route_for(opt) -> str:
    """"hip" when the MLBNoAtt options `opt` are the model ncx_mlb_train_* supports, else "torch path: <why>".  Reads the options
    only (never touches the library)."""
    f = opt.get("fusion", {})
    for k in ("dim_v", "dim_q", "dim_h"):
        if k not in f:
            return "torch path: fusion.%s is missing" % k
    for where, a in (("fusion.activation_v", f.get("activation_v")), ("fusion.activation_q", f.get("activation_q")),
                     ("classif.activation", opt.get("classif", {}).get("activation"))):
        if a not in ACT_CODE:
            return "torch path: %s = %r (HIP supports none / tanh)" % (where, a)
    return "hip"


def mlb_acts(opt):
    return (ACT_CODE[opt["fusion"].get("activation_v")], ACT_CODE[opt["fusion"].get("activation_q")],
            ACT_CODE[opt.get("classif", {}).get("activation")])


class MlbTrainFunction(torch.autograd.Function):
    """logits = classif(fusion(feats[img_idx], q_emb)) of MLBNoAtt with the six parameter tensors in ops.MLB_FIELDS order.
    Gradients: the parameters, and q_emb when it requires grad.  cfg = ((act_v, act_q, act_c), (p_v, p_q, p_c), seed, training):
    dropout runs on the counter-based generator under `seed` when training."""

    @staticmethod
    def forward(ctx, feats, img_idx, q_emb, wv, bv, wq, bq, wc, bc, cfg):
        acts, p, seed, training = cfg
        t = {k: x.detach().float().contiguous() for k, x in zip(ops.MLB_FIELDS, (wv, bv, wq, bq, wc, bc))}
        mw = ops.MlbWeights.from_tensors(t, *acts)
        mode = 1 if training and any(x > 0 for x in p) else 0
        d = ops.vqa_train_dims(img_idx.shape[0], feats.shape[1], q_emb.shape[1], mw.dz, mw.A, feats.shape[0], p=p if mode else (0, 0, 0),
                               dropout_mode=mode, seed=seed, want_dq=ctx.needs_input_grad[2])
        ws = ops.mlb_train_workspace(d, mw, feats.device)
        logits, z = ops.mlb_train_forward(d, feats.detach().float().contiguous(), img_idx, q_emb.detach().float().contiguous(), mw, ws)
        ctx.hip = (d, mw, ws)
        ctx.z = z
        return logits

    @staticmethod
    def backward(ctx, dlogits):
        d, mw, ws = ctx.hip
        grads = {k: torch.empty_like(v) for k, v in mw.t.items()}
        dq = ops.mlb_train_backward(d, mw, ws, dlogits.float().contiguous(), grads)
        return (None, None, dq) + tuple(grads[k] for k in ops.MLB_FIELDS) + (None,)


def mlb_module_forward(model, input_v: torch.Tensor, q_emb: torch.Tensor) -> torch.Tensor:
    """The HIP route of MLBNoAtt.forward below seq2vec: the rows of input_v are the feature table, the index the identity."""
    f, opt = model.fusion, model.opt
    idx = torch.arange(input_v.shape[0], dtype=torch.int32, device=input_v.device)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if model.training else 0      # torch's CPU generator: torch.manual_seed reproduces it
    cfg = (mlb_acts(opt), dropouts(opt), seed, bool(model.training))
    return MlbTrainFunction.apply(input_v, idx, q_emb, f.linear_v.weight, f.linear_v.bias, f.linear_q.weight, f.linear_q.bias,
                                  model.linear_classif.weight, model.linear_classif.bias, cfg)


class MlbAttTrainFunction(torch.autograd.Function):
    """(logits, att) = MLBAtt below the question encoder in training mode (ncx_mlb_att_train_forward / _backward) with the twelve
    parameter tensors in ops.MLB_ATT_FIELDS order (the two 1 x 1 convolutions as matrices, the glimpse Linears stacked).  feats is the
    table of NCHW maps, read in place; no gradient goes to it.  Gradients: the parameters, and q_emb when it requires grad; att
    [B, G, P] is not differentiable.  cfg = (acts, p, seed, training): acts the dict of ops.mlb_att_acts, p the six dropout p's in
    layer order; dropout runs on the counter-based generator under `seed` when training.  An optional fifth entry is the x6 choice of
    ops.mlb_att_flags for the forward and the backward (absent or None: the process-wide one)."""

    @staticmethod
    def forward(ctx, feats, img_idx, q_emb, wv_att, bv_att, wq_att, bq_att, wa, ba, wg, bg, wqf, bqf, wc, bc, cfg):
        acts, p, seed, training = cfg[:4]
        x6 = cfg[4] if len(cfg) > 4 else None
        t = {k: x.detach().float().contiguous() for k, x in zip(ops.MLB_ATT_FIELDS, (wv_att, bv_att, wq_att, bq_att, wa, ba, wg, bg, wqf, bqf, wc, bc))}
        mw = ops.MlbAttWeights.from_tensors(t, **acts)
        mode = 1 if training and any(x > 0 for x in p) else 0
        feats = feats.detach().float().contiguous()
        q = q_emb.detach().float().contiguous()
        dt = ops.mlb_att_train_dims(mw, img_idx.shape[0], feats[0, 0].numel(), feats.shape[0], p=p if mode else (0.0,) * 6, dropout_mode=mode,
                                    seed=seed, want_dq=ctx.needs_input_grad[2])
        ws = ops.mlb_att_train_workspace(dt, mw, feats.device)
        logits, att = ops.mlb_att_train_forward(dt, feats, img_idx, q, mw, ws, x6=x6)
        ctx.hip = (dt, mw, ws, feats, img_idx, q, att, x6)
        ctx.mark_non_differentiable(att)
        return logits, att

    @staticmethod
    def backward(ctx, dlogits, _datt=None):
        dt, mw, ws, feats, img_idx, q, att, x6 = ctx.hip
        grads = {k: torch.empty_like(v) for k, v in mw.t.items()}
        dq = ops.mlb_att_train_backward(dt, feats, img_idx, q, mw, ws, att, dlogits.float().contiguous(), grads, x6=x6)
        ctx.hip = None                                            # the stash is the step's largest buffer: let go of it here
        return (None, None, dq) + tuple(grads[k] for k in ops.MLB_ATT_FIELDS) + (None,)


def mlb_att_module_forward(model, input_v: torch.Tensor, q_emb: torch.Tensor):
    """The HIP training route of MLBAtt.forward below seq2vec -> (logits, att [B, G, P]): input_v [B, dv, W, H] is the table of maps,
    the index the identity.  The module's hip_x6 picks the form of the attention kernel and of its weight-gradient twin (ops.mlb_att_flags)."""
    idx = torch.arange(input_v.shape[0], dtype=torch.int32, device=input_v.device)
    seed = int(torch.randint(0, 2 ** 62, (1,)).item()) if model.training else 0      # torch's CPU generator: torch.manual_seed reproduces it
    cfg = (ops.mlb_att_acts(model.opt), ops.mlb_att_dropouts(model.opt), seed, bool(model.training), getattr(model, "hip_x6", None))
    lin = list(model.list_linear_v_fusion)
    return MlbAttTrainFunction.apply(input_v, idx, q_emb, model.conv_v_att.weight.flatten(1), model.conv_v_att.bias,
                                     model.linear_q_att.weight, model.linear_q_att.bias, model.conv_att.weight.flatten(1), model.conv_att.bias,
                                     torch.stack([l.weight for l in lin]), torch.stack([l.bias for l in lin]),
                                     model.linear_q_fusion.weight, model.linear_q_fusion.bias,
                                     model.linear_classif.weight, model.linear_classif.bias, cfg)


class _TrainEngine:
    """What the two engines share: one flat parameter buffer, one flat gradient buffer (both in the layout of the model's weights
    object) and two Adam state buffers; the reference's state_dict keys over views of the flat buffer, seq2vec.* entries carried
    through untouched; the step.  A subclass gives the layout (the shapes it hands to _setup), the names (_named_views), the weights object (_weights)
    and the three operators (_OPS)."""
    _OPS = None            # (workspace, forward, backward) of neuralcx.ops

    def _setup(self, shapes, dropout, lr, device, seed):
        self.dropout, self.lr, self.seed = tuple(float(x) for x in dropout), lr, int(seed)
        self.device = torch.device(device)
        self.params = FlatParams(shapes, self.device)
        self.grads = self.params.like()
        self.exp_avg = torch.zeros_like(self.params.flat)
        self.exp_avg_sq = torch.zeros_like(self.params.flat)
        self.step_count = 0
        self.seq2vec_state: Dict[str, torch.Tensor] = {}
        self._ws, self._ws_key = None, None

    # ---- parameters ----------------------------------------------------------------------------------------
    def init_parameters(self, seed=42):
        """nn.Linear's default: weight and bias U(+-1/sqrt(fan_in)), from a seed."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        for n, v in self._named_views().items():
            fan_in = v.shape[1] if v.dim() == 2 else self._named_views()[n.replace("bias", "weight")].shape[1]
            v.copy_((torch.rand(v.shape, generator=g) * 2 - 1) / math.sqrt(fan_in))

    def state_dict(self, views=False):
        sd = {n: (v if views else v.detach().clone()) for n, v in self._named_views().items()}
        sd.update({k: v for k, v in self.seq2vec_state.items()})
        return sd

    def load_state_dict(self, sd, strict=True):
        mine = self._named_views()
        extra = [k for k in sd if k not in mine and not k.startswith("seq2vec.")]
        missing = [k for k in mine if k not in sd]
        if strict and (extra or missing):
            raise KeyError("load_state_dict: missing %s, unexpected %s" % (missing, extra))
        for k, v in mine.items():
            if k in sd:
                v.copy_(torch.as_tensor(sd[k]).to(self.device))
        self.seq2vec_state = {k: torch.as_tensor(v).detach().clone() for k, v in sd.items() if k.startswith("seq2vec.")}

    def optimizer_state(self):
        return {"exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(), "step": self.step_count,
                "numel": self.params.numel}

    def load_optimizer_state(self, st):
        if st["numel"] != self.params.numel:
            raise ValueError("optimizer state of another model (%d vs %d parameters)" % (st["numel"], self.params.numel))
        self.exp_avg.copy_(st["exp_avg"].to(self.device)); self.exp_avg_sq.copy_(st["exp_avg_sq"].to(self.device))
        self.step_count = int(st["step"])

    # ---- steps ---------------------------------------------------------------------------------------------
    def _dims(self, feats, B, mode, seed, want_dq):
        c = self.cfg
        d = ops.vqa_train_dims(B, c["dv"], c["dq"], c["dz"], c["A"], feats.shape[0], p=self.dropout if mode else (0, 0, 0), dropout_mode=mode,
                               seed=seed, want_dq=want_dq)
        key = (B, feats.shape[0])
        if self._ws_key != key:
            self._ws = self._OPS[0](d, self._weights(), self.device)
            self._ws_key = key
        return d

    def forward_backward(self, feats, img_idx, q_emb, target, want_dq=False, masks=None, train=True):
        """forward + loss + backward into self.grads; -> dict(loss, hits1, hits5, logits, dq_emb).  No host sync."""
        mode = 2 if masks is not None else (1 if train and any(p > 0 for p in self.dropout) else 0)
        d = self._dims(feats, img_idx.shape[0], mode, self.seed * 1000003 + self.step_count, want_dq)
        mw = self._weights()
        logits, z = self._OPS[1](d, feats, img_idx, q_emb, mw, self._ws, masks=masks)
        r = ops.ce_loss(logits, target)
        dq = self._OPS[2](d, mw, self._ws, r["dlogits"], self.grads.views, masks=masks)
        return dict(loss=r["loss"], hits1=r["hits1"], hits5=r["hits5"], logits=logits, dq_emb=dq)

    def train_step(self, feats, img_idx, q_emb, target, want_dq=False, masks=None):
        """One optimisation step (engine.py:22-37).  Returns device tensors: loss [1], hits1 / hits5 [1] (counts; acc = 100 hits / B)."""
        self.step_count += 1
        r = self.forward_backward(feats, img_idx, q_emb, target, want_dq=want_dq, masks=masks)
        ops.adam_step(self.params.flat, self.grads.flat, self.exp_avg, self.exp_avg_sq, self.step_count, lr=self.lr)
        return r

    def evaluate(self, feats, img_idx, q_emb, target):
        """Eval forward + loss + hit counts (engine.py:59-100), dropout off."""
        d = self._dims(feats, img_idx.shape[0], 0, 0, False)
        logits, z = self._OPS[1](d, feats, img_idx, q_emb, self._weights(), self._ws)
        r = ops.ce_loss(logits, target, want_grad=False)
        return dict(loss=r["loss"], hits1=r["hits1"], hits5=r["hits5"], logits=logits, z=z)

    def check_targets(self):
        ops.check_vqa_targets(device=self.device)


class VqaTrainEngine(_TrainEngine):
    """The MutanNoAtt trainer: buffers in the stacked MutanWeights layout.  state_dict keys are the reference's (fusion.linear_v.*,
    fusion.list_linear_hv.{i}.* as row views of the stacked block, linear_classif.*)."""
    _OPS = (ops.vqa_train_workspace, ops.vqa_train_forward, ops.vqa_train_backward)

    def __init__(self, dv=2048, dq=2400, dhv=360, dhq=360, dz=360, R=10, A=2000, activation_v="tanh", activation_q="tanh",
                 dropout=(0.5, 0.5, 0.5), lr=1e-4, device="cuda:0", seed=0):
        self.cfg = dict(dv=dv, dq=dq, dhv=dhv, dhq=dhq, dz=dz, R=R, A=A)
        self.act_v, self.act_q = ACT_CODE[activation_v], ACT_CODE[activation_q]
        self._setup(ops.mutan_shapes(dv, dq, dhv, dhq, dz, R, A), dropout, lr, device, seed)

    @classmethod
    def from_options(cls, opt, num_answers, **kw):
        r = route_for(opt)
        if r != "hip":
            raise ops._lib.NcxError("VqaTrainEngine: " + r)
        f = opt["fusion"]
        return cls(dv=f["dim_v"], dq=f["dim_q"], dhv=f["dim_hv"], dhq=f["dim_hq"], dz=f["dim_mm"], R=f["R"], A=num_answers,
                   activation_v=f.get("activation_v"), activation_q=f.get("activation_q"), dropout=dropouts(opt), **kw)

    def _named_views(self) -> Dict[str, torch.Tensor]:
        v, dz, R = self.params.views, self.cfg["dz"], self.cfg["R"]
        out = {"fusion.linear_v.weight": v["wv"], "fusion.linear_v.bias": v["bv"], "fusion.linear_q.weight": v["wq"], "fusion.linear_q.bias": v["bq"]}
        for name, w, b in (("hv", "whv", "bhv"), ("hq", "whq", "bhq")):
            for i in range(R):
                out["fusion.list_linear_%s.%d.weight" % (name, i)] = v[w][i * dz:(i + 1) * dz]
                out["fusion.list_linear_%s.%d.bias" % (name, i)] = v[b][i * dz:(i + 1) * dz]
        out["linear_classif.weight"], out["linear_classif.bias"] = v["wc"], v["bc"]
        return out

    def mutan_weights(self, flat: Optional[FlatParams] = None) -> ops.MutanWeights:
        """The SAME buffers in the form the frozen producer takes (ops.vqa_forward): nothing is re-stacked."""
        return ops.MutanWeights.from_tensors((flat or self.params).views, self.cfg["R"], self.act_v, self.act_q)

    _weights = mutan_weights


class MlbTrainEngine(_TrainEngine):
    """The MLBNoAtt trainer: buffers in the MlbWeights layout.  state_dict keys are the reference's (fusion.linear_v.*,
    fusion.linear_q.*, linear_classif.*)."""
    _OPS = (ops.mlb_train_workspace, ops.mlb_train_forward, ops.mlb_train_backward)

    def __init__(self, dv=2048, dq=2400, dh=1200, A=2000, activation_v="tanh", activation_q="tanh", activation_c="tanh",
                 dropout=(0.5, 0.5, 0.5), lr=1e-4, device="cuda:0", seed=0):
        self.cfg = dict(dv=dv, dq=dq, dz=dh, A=A)
        self.act_v, self.act_q, self.act_c = ACT_CODE[activation_v], ACT_CODE[activation_q], ACT_CODE[activation_c]
        self._setup(ops.mlb_shapes(dv, dq, dh, A), dropout, lr, device, seed)

    @classmethod
    def from_options(cls, opt, num_answers, **kw):
        r = mlb_route_for(opt)
        if r != "hip":
            raise ops._lib.NcxError("MlbTrainEngine: " + r)
        f = opt["fusion"]
        return cls(dv=f["dim_v"], dq=f["dim_q"], dh=f["dim_h"], A=num_answers, activation_v=f.get("activation_v"),
                   activation_q=f.get("activation_q"), activation_c=opt.get("classif", {}).get("activation"), dropout=dropouts(opt), **kw)

    def _named_views(self) -> Dict[str, torch.Tensor]:
        v = self.params.views
        return {"fusion.linear_v.weight": v["wv"], "fusion.linear_v.bias": v["bv"], "fusion.linear_q.weight": v["wq"],
                "fusion.linear_q.bias": v["bq"], "linear_classif.weight": v["wc"], "linear_classif.bias": v["bc"]}

    def mlb_weights(self, flat: Optional[FlatParams] = None) -> ops.MlbWeights:
        """The SAME buffers in the form the frozen producer takes (ops.vqa_forward -> ncx_mlb_forward): nothing is copied."""
        return ops.MlbWeights.from_tensors((flat or self.params).views, self.act_v, self.act_q, self.act_c)

    _weights = mlb_weights
