"""Training / evaluation engine of the contrastive path: the reference's second script, contrastive.py, with its model
(ContrastiveModel, vqa/models/cx.py:428-487) and loss (ContrastiveLoss, contrastive.py:293-309).

ContrastiveEngine exposes the surface the CLI's Runner uses of the scorer engines (init_parameters, train_step, eval_step,
state_dict, load_state, optimizer_state, load_optimizer_state, flush, check_ids) and reuses their pieces: the flat parameter buffer
(FlatParams), the rank / Recall kernel (ncx_loss_rank, fed with distances: "farthest first") and the fused Adam (ncx_adam_step).
Forward, distances, loss and backward are the HIP entry points ncx_contrastive_*.

A training step has no scores and no listwise loss: three images per example -- [original, counterexample, one other neighbour]
-- are embedded by one shared Linear + ReLU, the counterexample is pushed beyond a margin and the other neighbour pulled in.
The triple is drawn ON THE DEVICE (sample_positions): `other` is uniform over the K - 1 neighbour POSITIONS that are not the
counterexample's.  The reference removes the counterexample from the neighbour list BY VALUE (list.remove, contrastive.py:347-350;
neuralcx.data.examples_to_arrays(pairwise=True) keeps that rule on the host): the two differ only when a neighbour list holds the
same image twice.

answer_embedding.weight is constructed by the reference (cx.py:440-441) but never read: it sits in the flat state for state_dict
and checkpoints, outside the span Adam touches, and is bit-equal to its initial value after any number of steps.
Single GPU: a data-parallel contrastive step does not exist yet.
"""
import math
from typing import Dict, Optional

import torch

from . import ops
from .engine import FlatParams

TRAINED = ("linear.weight", "linear.bias")


def sample_positions(gt: torch.Tensor, K: int, gen: torch.Generator) -> torch.Tensor:
    """-> pos [B, 2] int64: neighbour positions (0-based, in 0..K-1) of [counterexample, other]; `other` uniform over the K - 1
    positions != gt[b], drawn from the device generator `gen` (no host round trip)."""
    if K < 2:
        raise ValueError("the training triple needs at least 2 neighbours, got K = %d" % K)
    comp = gt.long()
    u = torch.randint(0, K - 1, comp.shape, generator=gen, device=comp.device)
    other = u + (u >= comp).long()                      # skips the counterexample's position
    return torch.stack([comp, other], dim=1)


def triple_img_idx(img_idx: torch.Tensor, pos: torch.Tensor) -> torch.Tensor:
    """img_idx [B, K + 1] int32 (slot 0 the original), pos [B, 2] -> [B, 3] feature-table rows [orig, comp, other]."""
    cols = torch.cat([torch.zeros_like(pos[:, :1]), pos + 1], dim=1)
    return torch.gather(img_idx, 1, cols).contiguous()


def triple_z(z_knns: torch.Tensor, pos: torch.Tensor, sel: Optional[torch.Tensor] = None) -> torch.Tensor:
    """z of the two chosen neighbours [B, 2, dz]: from a batch block z_knns [B, K, dz], or (sel given: example ids [B]) from a
    per-split cache z_knns [N, K, dz] without gathering the other K - 2 rows."""
    K, dz = z_knns.shape[1], z_knns.shape[2]
    base = (torch.arange(pos.shape[0], device=pos.device) if sel is None else sel.long())[:, None] * K
    return z_knns.reshape(-1, dz).index_select(0, (base + pos).reshape(-1)).view(pos.shape[0], 2, dz)


def triple_batch(feats, img_idx, z_orig, z_knns, gt, gen, sel=None) -> ops.Batch:
    """The P = 3 training batch of contrastive.py:213 (getDataFromBatch(pairwise=True)) from a K-neighbour batch, on the device."""
    pos = sample_positions(gt, img_idx.shape[1] - 1, gen)
    return ops.Batch(feats, triple_img_idx(img_idx, pos), None, z_orig.contiguous(), triple_z(z_knns, pos, sel), None)


class ContrastiveEngine:
    """ContrastiveModel (cx.py:428-487), H = 300.  State keys answer_embedding.weight [A, 300] (never trained), linear.weight
    [300, dv + dz] (columns v | z), linear.bias [300]."""
    state_to_field = ops.CONTRASTIVE_STATE_TO_FIELD

    def __init__(self, dv=2048, dz=360, A=2000, lr=1e-4, margin=ops.CONTRASTIVE_MARGIN, device="cuda:0", world_size=1, process_group=None):
        if world_size > 1:
            raise NotImplementedError("the contrastive path runs on one GPU: its step has no gradient exchange yet (world_size = %d)"
                                      % world_size)
        self.cfg = dict(dv=dv, dz=dz, A=A)
        self.lr, self.margin = lr, margin
        self.device = torch.device(device)
        self.params = FlatParams(ops.contrastive_shapes(dv, dz, A), self.device)
        self.n_trained = self.params.offsets["answer_embedding.weight"]       # Adam's span: linear.* only
        self.grads = FlatParams({n: self.params.shapes[n] for n in TRAINED}, self.device)
        assert self.grads.numel == self.n_trained
        self.exp_avg = torch.zeros(self.n_trained, dtype=torch.float32, device=self.device)
        self.exp_avg_sq = torch.zeros_like(self.exp_avg)
        self.step_count = 0
        self.world_size, self.pg, self.rank = 1, None, 0
        self.bad_flag = torch.zeros(1, dtype=torch.int32, device=self.device)
        self._ws: Dict[tuple, torch.Tensor] = {}

    # ---- parameters ----------------------------------------------------------------------------------------
    def init_parameters(self, seed=42, emb=None):
        """torch default init distributions: Embedding N(0, 1), Linear weight and bias U(+-1/sqrt(fan_in))."""
        g = torch.Generator(device="cpu").manual_seed(seed)
        fan_in = self.params.shapes["linear.weight"][1]
        for n, v in self.params.views.items():
            if n == "answer_embedding.weight":
                t = torch.randn(v.shape, generator=g)
            else:
                t = (torch.rand(v.shape, generator=g) * 2 - 1) / math.sqrt(fan_in)
            v.copy_(t)

    def load_state(self, state: Dict[str, torch.Tensor]):
        for n, v in self.params.views.items():
            v.copy_(state[n].to(self.device))

    def state_dict(self):
        order = ("answer_embedding.weight",) + TRAINED                           # the reference module's own order
        return {n: self.params.views[n].detach().clone() for n in order}

    def optimizer_state(self):
        return {"exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(), "step": self.step_count,
                "numel": self.n_trained}

    def load_optimizer_state(self, st):
        if st["numel"] != self.n_trained:
            raise ValueError("optimizer state of another model (%d vs %d parameters)" % (st["numel"], self.n_trained))
        self.exp_avg.copy_(st["exp_avg"].to(self.device)); self.exp_avg_sq.copy_(st["exp_avg_sq"].to(self.device))
        self.step_count = int(st["step"])

    def flush(self):
        """Nothing is deferred here; kept for the Runner's interface."""

    def check_ids(self):
        """Raises IndexError if a step since the last check saw a feature row out of range (host sync)."""
        ops.check_semantic_ids(self.bad_flag)

    # ---- steps ---------------------------------------------------------------------------------------------
    def _dims(self, batch: ops.Batch):
        d = ops.contrastive_dims(batch)
        key = (d.B, d.P, d.dv, d.dz, d.n_img)
        if key not in self._ws:                         # (training P = 3 and evaluation P = 25 alternate: keep both)
            if len(self._ws) >= 4:
                self._ws.clear()
            self._ws[key] = ops.contrastive_workspace(d, self.device)
        return d, self._ws[key]

    def forward(self, batch: ops.Batch, want_h: bool = True):
        """h [B, P, 300] (None with want_h = False: it stays in the workspace)."""
        self._d, self._w = self._dims(batch)
        v = self.params.views
        return ops.contrastive_forward(self._d, batch, v["linear.weight"], v["linear.bias"], self._w, bad_flag=self.bad_flag,
                                       want_h=want_h)

    def eval_step(self, batch: ops.Batch, gt: torch.Tensor):
        """contrastive.py:270-279: distances of every neighbour to the original, ranked farthest first; r["hits"] = Recall@1 / @5
        hit counts, r["rank"] the counterexample's rank, r["scores"] the distances [B, P - 1]."""
        self.forward(batch, want_h=False)
        dist = ops.contrastive_distances(self._d, ws=self._w)
        r = ops.ranking_loss(dist, gt, want_grad=False)           # (its loss output is not a quantity of this path)
        r["scores"] = dist
        return r

    def train_step(self, batch: ops.Batch, gt: Optional[torch.Tensor] = None, global_batch: Optional[int] = None, active: bool = True):
        """forward + both ContrastiveLoss terms + backward + Adam over linear.* (contrastive.py:215-224) on a P = 3 batch.
        Returns device tensors (loss_comp, loss_other, loss, dist_comp, dist_other, dist [B, 2]); never syncs the host."""
        if not active:
            raise NotImplementedError("padding steps belong to data parallelism, which the contrastive path does not have")
        B = batch.img_idx.shape[0]
        self.step_count += 1
        self.forward(batch, want_h=False)
        r = ops.contrastive_loss(self._d, self._w, scale=1.0 / (global_batch or B), margin=self.margin)
        g = self.grads.views
        ops.contrastive_backward(self._d, batch, self._w, g["linear.weight"], g["linear.bias"])
        ops.adam_step(self.params.flat[:self.n_trained], self.grads.flat, self.exp_avg, self.exp_avg_sq, self.step_count, lr=self.lr)
        return r
