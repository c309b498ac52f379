"""The fusions of the two no-attention VQA models, the producers of the multimodal vector z consumed by NeuralCX.
MutanFusion (Ben-younes et al.): same arithmetic and state_dict keys as the reference's (vqa/models/fusion.py:53-121):
tanh(linear_v(v)), tanh(linear_q(q)), R rank-1 terms linear_hv_i(x_v) * linear_hq_i(x_q), summed.
MLBFusion (Kim et al.): the reference's (vqa/models/fusion.py:16-50): act(linear_v(v)) * act(linear_q(q)).
These modules are the plain PyTorch-ROCm statement (the torch path of CXModelBase.vqa_forward and the yardstick of the tests);
on the GPU the frozen models run in the HIP library (ncx_vqa_forward / ncx_mlb_forward)."""
import torch
import torch.nn as nn
import torch.nn.functional as F


def out_dim(fusion_opt):
    """Width of z, the fusion block's output: dim_mm (MUTAN) when the block has it, else dim_h (MLB).  The reference's scorers read
    opt['fusion']['dim_mm'] and would raise KeyError on an MLB config (cx.py:168,228); accepting both is a deliberate superset."""
    if "dim_mm" in fusion_opt:
        return fusion_opt["dim_mm"]
    if "dim_h" in fusion_opt:
        return fusion_opt["dim_h"]
    raise KeyError("fusion options have neither dim_mm nor dim_h")


class MLBFusion(nn.Module):
    """x_mm = act_q(linear_q(q)) * act_v(linear_v(v)) (reference fusion.py:16-50; parameter names linear_v.*, linear_q.*).  A block without
    dim_v / dim_q passes that input through, as the reference does."""

    def __init__(self, opt):
        super().__init__()
        self.opt = opt
        if "dim_v" in opt:
            self.linear_v = nn.Linear(opt["dim_v"], opt["dim_h"])
        if "dim_q" in opt:
            self.linear_q = nn.Linear(opt["dim_q"], opt["dim_h"])

    def _embed(self, x, name):
        if "dim_" + name not in self.opt:
            return x
        x = getattr(self, "linear_" + name)(F.dropout(x, p=self.opt["dropout_" + name], training=self.training))
        return getattr(torch, self.opt["activation_" + name])(x) if "activation_" + name in self.opt else x

    def forward(self, input_v, input_q):
        return torch.mul(self._embed(input_q, "q"), self._embed(input_v, "v"))


class MutanFusion(nn.Module):
    def __init__(self, opt, visual_embedding=True, question_embedding=True):
        super().__init__()
        self.opt = opt
        self.visual_embedding, self.question_embedding = visual_embedding, question_embedding
        if visual_embedding:
            self.linear_v = nn.Linear(opt["dim_v"], opt["dim_hv"])
        if question_embedding:
            self.linear_q = nn.Linear(opt["dim_q"], opt["dim_hq"])
        self.list_linear_hv = nn.ModuleList([nn.Linear(opt["dim_hv"], opt["dim_mm"]) for _ in range(opt["R"])])
        self.list_linear_hq = nn.ModuleList([nn.Linear(opt["dim_hq"], opt["dim_mm"]) for _ in range(opt["R"])])

    def _act(self, x, key):
        return getattr(torch, self.opt[key])(x) if key in self.opt else x

    def embed_v(self, v):
        if not self.visual_embedding:
            return v
        v = F.dropout(v, p=self.opt["dropout_v"], training=self.training)
        return self._act(self.linear_v(v), "activation_v")

    def embed_q(self, q):
        if not self.question_embedding:
            return q
        q = F.dropout(q, p=self.opt["dropout_q"], training=self.training)
        return self._act(self.linear_q(q), "activation_q")

    def forward(self, input_v, input_q):
        if input_v.dim() != 2 or input_q.dim() != 2:
            raise ValueError("MutanFusion expects 2-D inputs")
        x_v, x_q = self.embed_v(input_v), self.embed_q(input_q)
        x_mm = None
        for lin_v, lin_q in zip(self.list_linear_hv, self.list_linear_hq):
            hv = self._act(lin_v(F.dropout(x_v, p=self.opt["dropout_hv"], training=self.training)), "activation_hv")
            hq = self._act(lin_q(F.dropout(x_q, p=self.opt["dropout_hq"], training=self.training)), "activation_hq")
            x_mm = hq * hv if x_mm is None else x_mm + hq * hv
        return self._act(x_mm, "activation_mm")
