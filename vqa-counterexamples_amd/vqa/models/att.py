"""Attention VQA models (reference: vqa/models/att.py:11-192).  MLBAtt is built; MutanAtt (MutanFusion2d on the same attention)
is not.  state_dict names and shapes are the reference's, so its checkpoints load:
  seq2vec.*, conv_v_att [dh_att, dv, 1, 1], linear_q_att [dh_att, dq], conv_att [G, dh_att, 1, 1],
  list_linear_v_fusion.{g} [dh_f, dv], linear_q_fusion [G dh_f, dq], linear_classif [A, G dh_f].
The image input is the NCHW map [B, dv, W, H]; spatial position p = w H + h, i.e. the map's memory order."""
import torch
import torch.nn as nn
import torch.nn.functional as F

from . import seq2vec


def _act(x, name):
    return getattr(F, name)(x) if name else x


class AbstractAtt(nn.Module):
    """seq2vec + the attention head (a 1 x 1 convolution of the map, a Linear of the question, a fusion set by the subclass, a 1 x 1
    convolution to G glimpses, a softmax over positions) + attention-weighted pooling.  The subclass adds the glimpse fusion and
    the classifier.  After every forward, `list_att` holds the G attention maps [B, W H] (detached)."""

    def __init__(self, opt=None, vocab_words=(), vocab_answers=()):
        super().__init__()
        opt = opt or {}
        self.opt, self.vocab_words, self.vocab_answers = opt, vocab_words, vocab_answers
        self.num_classes = len(vocab_answers)
        att = opt["attention"]
        self.seq2vec = seq2vec.factory(vocab_words, opt["seq2vec"], dim_q=opt["dim_q"])
        self.conv_v_att = nn.Conv2d(opt["dim_v"], att["dim_v"], 1, 1)
        self.linear_q_att = nn.Linear(opt["dim_q"], att["dim_q"])
        self.conv_att = nn.Conv2d(att["dim_mm"], att["nb_glimpses"], 1, 1)
        self.list_att = []

    def _fusion_att(self, x_v, x_q):
        raise NotImplementedError

    def _fusion_classif(self, x_v, x_q):
        raise NotImplementedError

    def _attention(self, input_v, q_vec):
        att = self.opt["attention"]
        train = self.training
        x_v = _act(self.conv_v_att(F.dropout(input_v, p=att["dropout_v"], training=train)), att.get("activation_v"))     # [B, dh, W, H]
        x_q = _act(self.linear_q_att(F.dropout(q_vec, p=att["dropout_q"], training=train)), att.get("activation_q"))   # [B, dh]
        x = _act(self._fusion_att(x_v, x_q[:, :, None, None]), att.get("activation_mm"))
        x = F.dropout(x, p=att["dropout_mm"], training=train)
        maps = F.softmax(self.conv_att(x).flatten(2), dim=2)                  # [B, G, P], positions in memory order
        self.list_att = [m.detach() for m in maps.unbind(1)]
        v = input_v.flatten(2)                                                # [B, dv, P]
        pooled = torch.einsum("bgp,bcp->bgc", maps, v)                        # [B, G, dv]
        return list(pooled.unbind(1))

    def _fusion_glimpses(self, list_v_att, q_vec):
        fus = self.opt["fusion"]
        train = self.training
        xs = [_act(lin(F.dropout(v, p=fus["dropout_v"], training=train)), fus.get("activation_v"))
              for lin, v in zip(self.list_linear_v_fusion, list_v_att)]
        x_v = torch.cat(xs, 1)
        x_q = _act(self.linear_q_fusion(F.dropout(q_vec, p=fus["dropout_q"], training=train)), fus.get("activation_q"))
        return self._fusion_classif(x_v, x_q)

    def _classif(self, x):
        cla = self.opt["classif"]
        x = F.dropout(_act(x, cla.get("activation")), p=cla["dropout"], training=self.training)
        return self.linear_classif(x)

    def _torch_forward(self, input_v, q_vec):
        return self._classif(self._fusion_glimpses(self._attention(input_v, q_vec), q_vec))

    def forward(self, input_v, input_q):
        if input_v.dim() != 4 or input_q.dim() != 2:
            raise ValueError("input_v must be [B, dim_v, W, H] and input_q [B, T]")
        return self._torch_forward(input_v, self.seq2vec(input_q))


class MLBAtt(AbstractAtt):
    """The reference's MLBAtt (att.py:166-192): both fusions are element-wise products; attention.dim_h is the width of the
    attention head, fusion.dim_h the width of each glimpse's Linear.

    On a CUDA device in eval mode, when no gradient can be wanted, everything below the question encoder runs in the HIP library
    (ops.mlb_att_forward: the convolution reads the NCHW map in place, the attention head lives in its epilogue); `use_hip = False`
    keeps it in PyTorch, and so do training mode, grad mode with a parameter that requires grad, an activation other than tanh,
    non-fp32 tensors and shapes the library refuses.  It trains under torch autograd, unless `use_hip_train` is set: then the
    training step below the encoder runs in HIP too (neuralcx.vqa_train.MlbAttTrainFunction: forward with the six dropouts on the
    counter-based generator, backward through the attention), the encoder training from the d loss / d q_emb it returns.
    `hip_x6` picks the form of the attention kernel on both HIP routes, and of its weight-gradient twin in the training route's backward: None the process-wide choice (ops.EXTRA_FLAGS, NCX_X6=1 in
    the environment), True / False force NCX_F_X6 on / off.  It changes no routing decision."""
    use_hip = True
    use_hip_train = False
    hip_x6 = None

    def __init__(self, opt=None, vocab_words=(), vocab_answers=()):
        opt = opt or {}
        att = opt["attention"]
        att["dim_v"] = att["dim_q"] = att["dim_mm"] = att["dim_h"]
        super().__init__(opt, vocab_words, vocab_answers)
        G, dh_f = att["nb_glimpses"], opt["fusion"]["dim_h"]
        self.list_linear_v_fusion = nn.ModuleList([nn.Linear(opt["dim_v"], dh_f) for _ in range(G)])
        self.linear_q_fusion = nn.Linear(opt["dim_q"], dh_f * G)
        self.linear_classif = nn.Linear(dh_f * G, self.num_classes)

    def _fusion_att(self, x_v, x_q):
        return x_v * x_q

    def _fusion_classif(self, x_v, x_q):
        return x_v * x_q

    def _head_params(self):
        return [p for n, p in self.named_parameters() if not n.startswith("seq2vec.")]

    def _hip_weights(self):
        """ops.MlbAttWeights of the current parameters; repacked when a parameter moved or was written to (GRUEncoder's key)."""
        from neuralcx import ops
        key = tuple((p.data_ptr(), p._version) for p in self._head_params())
        hit = self.__dict__.get("_hip_att")
        if hit is None or hit[0] != key:
            hit = self.__dict__["_hip_att"] = (key, ops.mlb_att_weights(self))
        return hit[1]

    def _hip_ok(self, input_v, q_vec):
        if not (self.use_hip and input_v.is_cuda and q_vec.is_cuda and not self.training):
            return False
        params = self._head_params()
        if torch.is_grad_enabled() and (q_vec.requires_grad or input_v.requires_grad or any(p.requires_grad for p in params)):
            return False
        if input_v.dtype != torch.float32 or q_vec.dtype != torch.float32 or q_vec.device != input_v.device:
            return False
        if not all(p.dtype == torch.float32 and p.device == input_v.device for p in params):
            return False
        from neuralcx import ops
        if ops.mlb_att_acts(self.opt) is None:
            return False
        return ops.mlb_att_dims_ok(self._hip_weights(), input_v.shape[0], input_v.shape[2] * input_v.shape[3], input_v.shape[0])

    def forward(self, input_v, input_q):
        if input_v.dim() != 4 or input_q.dim() != 2:
            raise ValueError("input_v must be [B, dim_v, W, H] and input_q [B, T]")
        return self.forward_from_q(input_v, self.seq2vec(input_q))

    def _hip_train_ok(self, input_v, q_vec):
        """The opt-in HIP training route (`use_hip_train`): training mode, or grad mode with a parameter that requires grad; CUDA, fp32,
        activations in {none, tanh}, a shape the library accepts.  Anything else keeps the torch path."""
        if not (self.use_hip_train and input_v.is_cuda and q_vec.is_cuda):
            return False
        params = self._head_params()
        if not (self.training or (torch.is_grad_enabled() and any(p.requires_grad for p in params))):
            return False
        if input_v.dtype != torch.float32 or q_vec.dtype != torch.float32 or q_vec.device != input_v.device:
            return False
        if not all(p.dtype == torch.float32 and p.device == input_v.device for p in params):
            return False
        from neuralcx import ops
        if ops.mlb_att_acts(self.opt) is None:
            return False
        mw = self._hip_weights()
        p = ops.mlb_att_dropouts(self.opt) if self.training else (0.0,) * 6
        if not all(0.0 <= x < 1.0 for x in p):
            return False
        mode = 1 if any(x > 0 for x in p) else 0
        B = input_v.shape[0]
        return ops.mlb_att_train_dims_ok(mw, ops.mlb_att_train_dims(mw, B, input_v.shape[2] * input_v.shape[3], B, p=p, dropout_mode=mode))

    def forward_from_q(self, input_v, q_vec):
        """forward below the question encoder: q_vec [B, dim_q] is the encoder's output (a caller with a frozen encoder keeps it)."""
        if self._hip_train_ok(input_v, q_vec):
            from neuralcx import vqa_train
            logits, att = vqa_train.mlb_att_module_forward(self, input_v, q_vec)
            self.list_att = list(att.detach().unbind(1))
            return logits
        if self._hip_ok(input_v, q_vec):
            from neuralcx import ops
            logits, att = ops.mlb_att_forward(input_v.contiguous(), None, q_vec.contiguous(), self._hip_weights(), x6=self.hip_x6)
            self.list_att = list(att.unbind(1))
            return logits
        return self._torch_forward(input_v, q_vec)
