"""Training / evaluation engines of the two trainable scorers besides NeuralModel: LinearContext (reference
vqa/models/cx.py:139-156) and PairwiseLinearModel (cx.py:379-425).

They expose the surface the CLI's Runner uses of NeuralCXEngine (init_parameters, train_step, eval_step, state_dict,
load_state, optimizer_state, load_optimizer_state, flush) and reuse its pieces: the flat parameter buffer (FlatParams), the
listwise loss / Recall kernel (ncx_loss_rank) and the fused Adam (ncx_adam_step).  Forward and backward are the HIP entry
points ncx_pairlin_* / ncx_linctx_*.  Data parallelism: every rank scales its loss by 1 / B_global and the flat gradient is
summed with one all_reduce before Adam.  Neither model has dropout (the reference's LinearContext has a TODO there, cx.py:154).
"""
import math
from typing import Dict, Optional

import torch

from . import ops
from .engine import FlatParams


class _ScorerEngine:
    state_to_field: Dict[str, str] = {}

    def __init__(self, shapes, lr=1e-4, device="cuda:0", world_size=1, process_group=None):
        self.lr = lr
        self.device = torch.device(device)
        self.params = FlatParams(shapes, self.device)
        self.grads = self.params.like()
        self.exp_avg = torch.zeros_like(self.params.flat)
        self.exp_avg_sq = torch.zeros_like(self.params.flat)
        self.step_count = 0
        self.world_size, self.pg = world_size, process_group
        self.rank = 0
        self._ws = None
        self._ws_key = None

    # ---- parameters ----------------------------------------------------------------------------------------
    def init_parameters(self, seed=42, emb=None):
        """torch default init distributions: Embedding N(0, 1), Linear weight and bias U(+-1/sqrt(fan_in))."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        for n, v in self.params.views.items():
            if n == "answer_embedding.weight":
                t = torch.randn(v.shape, generator=g) if emb is None else torch.as_tensor(emb, dtype=torch.float32)
            else:
                fan_in = v.shape[1] if v.dim() == 2 else self.params.shapes[n.replace("bias", "weight")][1]
                b = 1.0 / math.sqrt(fan_in)
                t = (torch.rand(v.shape, generator=g) * 2 - 1) * b
            v.copy_(t)

    def load_state(self, state: Dict[str, torch.Tensor]):
        for n, v in self.params.views.items():
            v.copy_(state[n].to(self.device))

    def state_dict(self):
        return {n: v.detach().clone() for n, v in self.params.views.items()}

    def optimizer_state(self):
        return {"exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(), "step": self.step_count,
                "numel": self.params.numel}

    def load_optimizer_state(self, st):
        if st["numel"] != self.params.numel:
            raise ValueError("optimizer state of another model (%d vs %d parameters)" % (st["numel"], self.params.numel))
        self.exp_avg.copy_(st["exp_avg"].to(self.device)); self.exp_avg_sq.copy_(st["exp_avg_sq"].to(self.device))
        self.step_count = int(st["step"])

    def flush(self):
        """Nothing is deferred here (no pipelined gradient exchange); kept for the Runner's interface."""

    def fields(self, flat: FlatParams):
        return {self.state_to_field[n]: v for n, v in flat.views.items()}

    # ---- steps ---------------------------------------------------------------------------------------------
    def eval_step(self, batch: ops.Batch, gt: torch.Tensor):
        scores = self.forward(batch)
        r = ops.ranking_loss(scores, gt, want_grad=False)
        r["scores"] = scores
        return r

    def train_step(self, batch: ops.Batch, gt: torch.Tensor, global_batch: Optional[int] = None, active: bool = True):
        """forward + loss (CrossEntropyLoss(size_average=False) / B, counterexamples.py:334) + backward + (all-reduce) + Adam.
        Returns device tensors; never syncs the host.  active = False: a padding triplet with loss weight 0 (dp.epoch_plan)."""
        B = batch.img_idx.shape[0]
        gb = global_batch if global_batch is not None else B * self.world_size
        self.step_count += 1
        scores = self.forward(batch)
        r = ops.ranking_loss(scores, gt, scale=1.0 / gb)
        if not active:
            for k in ("dscores", "loss", "loss_rows", "hits"):
                r[k].zero_()
        self.backward(batch, r["dscores"])
        if self.world_size > 1:
            torch.distributed.all_reduce(self.grads.flat, group=self.pg)
        ops.adam_step(self.params.flat, self.grads.flat, self.exp_avg, self.exp_avg_sq, self.step_count, lr=self.lr)
        r["scores"] = scores
        return r


class PairwiseLinearEngine(_ScorerEngine):
    """PairwiseLinearModel (cx.py:379-425); H = dim_a = 300 as in the reference.  State keys answer_embedding.weight,
    linear.weight, linear.bias, out.weight, out.bias."""
    state_to_field = ops.PAIRLIN_STATE_TO_FIELD

    def __init__(self, K=24, dv=2048, dq=2400, dz=360, A=2000, lr=1e-4, device="cuda:0", world_size=1, process_group=None):
        self.cfg = dict(K=K, dv=dv, dq=dq, dz=dz, A=A)
        super().__init__(ops.pairlin_shapes(K, dv, dq, dz, A), lr=lr, device=device, world_size=world_size, process_group=process_group)
        self.bad_flag = torch.zeros(1, dtype=torch.int32, device=self.device)

    def _dims(self, batch):
        d = ops.pairlin_dims(batch, self.cfg["A"])
        key = (d.B, d.K, d.dv, d.dq, d.dz, d.A, d.n_img)
        if self._ws_key != key:
            self._ws = ops.pairlin_workspace(d, self.device)
            self._ws_key = key
        return d

    def forward(self, batch: ops.Batch):
        self._d = self._dims(batch)
        return ops.pairlin_forward(self._d, batch, self.fields(self.params), self._ws, bad_flag=self.bad_flag)

    def backward(self, batch: ops.Batch, dscores: torch.Tensor):
        ops.pairlin_backward(self._d, batch, self.fields(self.params), self._ws, dscores, self.fields(self.grads))

    def check_ids(self):
        """Raises IndexError if a step since the last check saw a feature row or answer id out of range (host sync)."""
        ops.check_semantic_ids(self.bad_flag)


class LinearContextEngine(_ScorerEngine):
    """LinearContext (cx.py:139-156).  State keys linear.weight [K, K dz], linear.bias [K]."""
    state_to_field = ops.LINCTX_STATE_TO_FIELD

    def __init__(self, K=24, dz=360, lr=1e-4, device="cuda:0", world_size=1, process_group=None):
        self.cfg = dict(K=K, dz=dz)
        super().__init__(ops.linctx_shapes(K, dz), lr=lr, device=device, world_size=world_size, process_group=process_group)

    def _dims(self, z_knns):
        d = ops.linctx_dims(z_knns)
        key = (d.B, d.K, d.dz)
        if self._ws_key != key:
            self._ws = ops.linctx_workspace(d, self.device)
            self._ws_key = key
        return d

    def forward(self, batch: ops.Batch):
        self._d = self._dims(batch.z_knns)
        f = self.fields(self.params)
        return ops.linctx_forward(self._d, batch.z_knns, f["w"], f["b"], self._ws)

    def backward(self, batch: ops.Batch, dscores: torch.Tensor):
        g = self.fields(self.grads)
        ops.linctx_backward(self._d, batch.z_knns, dscores, self._ws, g["w"], g["b"])

    def check_ids(self):
        pass
