"""Training / evaluation engine of the NeuralCX hot path on one MI355X per process.

Replaces the inner body of the reference's train loop (counterexamples.py:322-339) and of eval_model
(counterexamples.py:460-468): forward, listwise loss + recall, backward, Adam -- all HIP kernels behind the
C ABI.  Data parallelism (net-new; the reference is single-GPU): one process per GPU, every
rank scales its loss by 1/B_global so a plain SUM all-reduce of the flat gradient buffer over RCCL
reproduces the single-GPU gradient of the global batch; parameters stay replicated.

Memory layout in HBM: all trainable tensors live back to back in ONE flat fp32 buffer (answer_embedding,
linear_1.weight [H, 14089], biases, out), gradients and the two Adam moments mirror it, so the optimizer
is one fused launch and the gradient exchange is one (bucketed) collective.
"""
import math
from typing import Dict, Optional

import torch

from . import dp, ops
from ._lib import NCX_F_ALL, NCX_F_A_EMB, NCX_F_BF16, NCX_F_FUSED_TAIL, NCX_F_REUSE_GT, NCX_F_X6

STATE_NAMES = ("answer_embedding.weight", "linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias",
               "linear_3.weight", "linear_3.bias", "out.weight", "out.bias")


def param_shapes(K, dv, dq, dz, da, A, H, L):
    din = 3 * dv + 2 * da + 2 * dz + dq + K + 1          # cx.py:245-251
    s = {"answer_embedding.weight": (A, da), "linear_1.weight": (H, din), "linear_1.bias": (H,)}
    if L >= 2: s["linear_2.weight"] = (H, H); s["linear_2.bias"] = (H,)
    if L >= 3: s["linear_3.weight"] = (H, H); s["linear_3.bias"] = (H,)
    s["out.weight"] = (1, H); s["out.bias"] = (1,)
    return s


class FlatParams:
    """One flat buffer + named views (state_dict names of the reference, cx.py:240-257)."""

    def __init__(self, shapes: Dict[str, tuple], device):
        self.shapes = shapes
        self.offsets, off = {}, 0
        for n, shp in shapes.items():
            self.offsets[n] = off
            off += (math.prod(shp) + 3) // 4 * 4          # keep every tensor 16-byte aligned
        self.numel = off
        self.flat = torch.zeros(off, dtype=torch.float32, device=device)
        self.views = {n: self.flat[o:o + math.prod(shapes[n])].view(shapes[n]) for n, o in self.offsets.items()}

    def like(self):
        other = FlatParams.__new__(FlatParams)
        other.shapes, other.offsets, other.numel = self.shapes, self.offsets, self.numel
        other.flat = torch.zeros_like(self.flat)
        other.views = {n: other.flat[o:o + math.prod(self.shapes[n])].view(self.shapes[n]) for n, o in self.offsets.items()}
        return other

    def fields(self):
        return {ops.STATE_TO_FIELD[n]: v for n, v in self.views.items()}


class NeuralCXEngine:
    def __init__(self, K=24, dv=2048, dq=2400, dz=360, da=2400, A=2000, H=256, L=1, drop_p=0.25, lr=1e-4,
                 device="cuda:0", spec: Optional[dict] = None, world_size=1, process_group=None, bf16: bool = False, x6: bool = False):
        self.cfg = dict(K=K, dv=dv, dq=dq, dz=dz, da=da, A=A, H=H, L=L)
        self.drop_p, self.lr = drop_p, lr
        self.device = torch.device(device)
        self.flags = ops.flags_from_spec(spec) if spec is not None else NCX_F_ALL
        if bf16:                                  # BASELINE configs[4]: bf16 MFMA operands, fp32 master weights / Adam
            if self.flags != NCX_F_ALL:
                raise ValueError("the bf16 variant supports the full model_spec only (no lesions)")
            self.flags |= NCX_F_BF16
        if x6:                                    # NOT the default: fp32-grade split-bf16 operands for the balanced TN weight-gradient launch
            self.flags |= NCX_F_X6
        self.params = FlatParams(param_shapes(**self.cfg), self.device)
        self.grads = self.params.like()
        self.exp_avg = torch.zeros_like(self.params.flat)
        self.exp_avg_sq = torch.zeros_like(self.params.flat)
        self.step_count = 0
        self.world_size, self.pg = world_size, process_group
        self.fused_tail = True                    # train_step: ncx_train_tail where the shape allows (tests switch it off to compare)
        self._ws = None
        self._ws_key = None
        self.seed = 42
        self.rank = 0
        self._weights_version = 0
        self._gt_key = None
        # data parallelism: when set (bench.py), every step records events around the two waits for the gradient exchange on the
        # compute stream: comm_events = [(before wait 1, after wait 1, before wait 2, after wait 2), ...] -- how long the step
        # stalls for each bucket, i.e. the part of the all-reduce the backward did NOT hide
        self.comm_profile = False
        self.comm_events = []
        # data parallelism: the last gradient bucket (linear_1.weight .. out.bias) has nothing of its own step left to hide behind
        # except the embedding's dE GEMM + Adam slice.  With `pipeline` its wait and the Adam slice it feeds are DEFERRED: the
        # next train_step first enqueues its data-only forward prelude (ncx_forward_phase PRELUDE: k_prep, a function of the batch
        # alone), then waits, applies the slice and runs the rest of the forward.  Same kernels on the same operands in an order
        # that respects every dependency: weights bit-identical to the unpipelined engine.  Anything that reads the weights from
        # outside a train_step (eval, state_dict, checkpoints) goes through flush() first.
        self.pipeline = True
        self._pending = None                      # (work handle of bucket 2, Adam step number, timing events)

    # ---- parameters --------------------------------------------------------------------------------------
    def init_parameters(self, seed=42, emb=None):
        """torch default init distributions: Embedding N(0,1), Linear U(+-1/sqrt(fan_in)) (cx.py:240-257)."""
        self.flush()
        g = torch.Generator(device="cpu").manual_seed(seed)
        for n, v in self.params.views.items():
            if n == "answer_embedding.weight":
                t = torch.randn(v.shape, generator=g) if emb is None else torch.as_tensor(emb, dtype=torch.float32)
            else:
                fan_in = v.shape[1] if v.dim() == 2 else self.params.shapes[n.replace("bias", "weight")][1]
                b = 1.0 / math.sqrt(fan_in)
                t = (torch.rand(v.shape, generator=g) * 2 - 1) * b
            v.copy_(t)
        self._weights_version += 1

    def load_state(self, state: Dict[str, torch.Tensor]):
        self.flush()
        for n, v in self.params.views.items():
            v.copy_(state[n].to(self.device))
        self._weights_version += 1

    def state_dict(self):
        self.flush()
        return {n: v.detach().clone() for n, v in self.params.views.items()}

    def optimizer_state(self):
        """Adam moments + step counter (net-new: the reference checkpoints the model only, counterexamples.py:550-560, so
        its --resume restarts Adam; with this a resumed run continues bit for bit)."""
        self.flush()
        return {"exp_avg": self.exp_avg.detach().cpu(), "exp_avg_sq": self.exp_avg_sq.detach().cpu(), "step": self.step_count,
                "numel": self.params.numel}

    def load_optimizer_state(self, st):
        self.flush()
        if st["numel"] != self.params.numel:
            raise ValueError("optimizer state of another model (%d vs %d parameters)" % (st["numel"], self.params.numel))
        self.exp_avg.copy_(st["exp_avg"].to(self.device)); self.exp_avg_sq.copy_(st["exp_avg_sq"].to(self.device))
        self.step_count = int(st["step"])

    # ---- steps -------------------------------------------------------------------------------------------
    def _dims(self, batch: ops.Batch, training: bool, loss_scale: float):
        c = self.cfg
        d = ops.make_dims(batch, H=c["H"], L=c["L"], da=c["da"], A=c["A"], flags=self.flags, training=training,
                          drop_p=self.drop_p if training else 0.0, loss_scale=loss_scale,
                          seed=(self.seed << 32) ^ (self.rank << 24) ^ self.step_count)
        need = ops.workspace_bytes(d) + 256
        if self._ws is None or self._ws.numel() < need:
            self._ws = torch.empty(need, dtype=torch.uint8, device=self.device)
        return d

    def flush(self):
        """Complete a deferred tail of the last train_step (data parallelism with `pipeline`): wait for its last gradient bucket
        and apply the Adam slice it feeds.  No-op otherwise.  Every rank calls it at the same points (it holds no collective)."""
        if self._pending is None:
            return
        h2, step, ev = self._pending
        self._pending = None
        n_emb = self.params.offsets["linear_1.weight"]
        if ev: ev[2].record()
        h2.wait()
        if ev: ev[3].record(); self.comm_events.append(ev)
        ops.adam_step(self.params.flat[n_emb:], self.grads.flat[n_emb:], self.exp_avg[n_emb:], self.exp_avg_sq[n_emb:], step, lr=self.lr)

    def forward(self, batch: ops.Batch, training=False):
        self.flush()
        d = self._dims(batch, training, 0.0)
        # evaluation passes: Gt = W1[:, a_other] . E^T only depends on the weights -- reuse it while neither the weights
        # (train_step / load_state / init_parameters bump _weights_version) nor the workspace changed
        key = (self._weights_version, self._ws.data_ptr(), d.B, d.K, d.H, d.A)       # (the workspace layout depends on B, K)
        if not training and (self.flags & NCX_F_A_EMB) and self._gt_key == key:
            d.flags |= NCX_F_REUSE_GT
        scores = ops.forward(d, batch, self.params.fields(), self._ws)
        self._gt_key = key
        return scores, d

    def eval_step(self, batch: ops.Batch, gt: torch.Tensor):
        scores, _ = self.forward(batch, training=False)
        r = ops.ranking_loss(scores, gt, want_grad=False)
        r["scores"] = scores
        return r

    def train_step(self, batch: ops.Batch, gt: torch.Tensor, global_batch: Optional[int] = None, active: bool = True):
        """forward + loss + backward + (all-reduce) + Adam.  Returns device tensors; never syncs the host.
        active = False (data parallelism, dp.epoch_plan): `batch` is a padding triplet -- the step runs with loss weight 0,
        i.e. this rank adds exact zeros to every gradient sum but enters every collective and steps its optimizer."""
        B = batch.img_idx.shape[0]
        gb = global_batch if global_batch is not None else B * self.world_size
        self.step_count += 1
        self._weights_version += 1
        d = self._dims(batch, True, 1.0 / gb)
        # out layer + loss / Recall + head of the backward as one pass over h_L (ncx_train_tail) where the shape allows; a
        # padding step (loss weight 0) takes the three separate calls
        fused = active and self.fused_tail and ops.fused_tail_ok(d)
        if fused:
            d.flags |= NCX_F_FUSED_TAIL
        if self._pending is not None:
            # the previous step's last bucket is still on the wire: this step's data-only prelude runs under it
            ops.forward(d, batch, self.params.fields(), self._ws, phase=ops.FWD_PRELUDE)
            self.flush()
            scores = ops.forward(d, batch, self.params.fields(), self._ws, phase=ops.FWD_REST)
        else:
            scores = ops.forward(d, batch, self.params.fields(), self._ws)
        if fused:
            r = ops.train_tail(d, self.params.fields(), self._ws, scores, gt, self.grads.fields())
        else:
            r = ops.ranking_loss(scores, gt, scale=1.0 / gb)
        if not active:
            for k in ("dscores", "loss", "loss_rows", "hits"):
                r[k].zero_()
        if self.world_size > 1:
            # The embedding gradient dE = dGt^T.W1ak + dGgt^T.W1agt is linear in the 2 x [H, A] block dGt | dGgt: the
            # ranks sum THAT block (4 MB at H=256) and each computes the complete dE itself, so the 19 MB [A, da]
            # gradient never crosses xGMI.  Order (ncx_backward_phase 5 | 2 | 4): the block is produced FIRST and is on
            # the wire while the bulk of the backward (linear_1.weight: ~0.35 ms at configs[1]) runs; bucket 2
            # (linear_1.weight .. out.bias, 14.4 MB; only answer_embedding, first in the flat buffer, is excluded) is on
            # the wire while the dE GEMM and answer_embedding's Adam slice run.
            n_emb = self.params.offsets["linear_1.weight"]
            f = self.params.fields()
            if self.flags & NCX_F_A_EMB:
                ops.backward(d, batch, f, self._ws, r["dscores"], self.grads.fields(), phase=5)
                h1 = torch.distributed.all_reduce(ops.ws_dgt_view(d, self._ws), group=self.pg, async_op=True)
                ops.backward(d, batch, f, self._ws, r["dscores"], self.grads.fields(), phase=2)
                h2 = torch.distributed.all_reduce(self.grads.flat[n_emb:], group=self.pg, async_op=True)
                ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)] if self.comm_profile else None
                if ev: ev[0].record()
                h1.wait()
                if ev: ev[1].record()
                ops.backward(d, batch, f, self._ws, r["dscores"], self.grads.fields(), phase=4)
                # answer_embedding's gradient is complete on every rank: its Adam slice also runs under bucket 2
                ops.adam_step(self.params.flat[:n_emb], self.grads.flat[:n_emb], self.exp_avg[:n_emb], self.exp_avg_sq[:n_emb],
                              self.step_count, lr=self.lr)
                self._pending = (h2, self.step_count, ev)
                if not self.pipeline:
                    self.flush()                     # wait for bucket 2 + the tail Adam slice now
                r["scores"] = scores
                return r
            else:                                   # a_emb lesion: the embedding gradient is zero everywhere
                ops.backward(d, batch, f, self._ws, r["dscores"], self.grads.fields())
                torch.distributed.all_reduce(self.grads.flat[n_emb:], group=self.pg)
        else:
            # one GPU: nothing sums gradients between the backward and the optimiser, so they are one call (the launch of the
            # answer_embedding gradient applies Adam where the route allows, ncx_backward_adam)
            ops.backward_adam(d, batch, self.params.fields(), self._ws, r["dscores"], self.grads.fields(), self.params.flat,
                              self.grads.flat, self.exp_avg, self.exp_avg_sq, self.params.offsets["linear_1.weight"], self.step_count,
                              lr=self.lr)
            r["scores"] = scores
            return r
        ops.adam_step(self.params.flat, self.grads.flat, self.exp_avg, self.exp_avg_sq, self.step_count, lr=self.lr)
        r["scores"] = scores
        return r


    # ---- configs[2]: MUTAN multimodal features produced on the fly ---------------------------------
    def make_batch_from_vqa(self, feats, img_idx, q_emb, answer_aids, mutan_weights):
        """Inputs of NeuralCX from the frozen MUTAN producer (ncx_vqa_forward) instead of precomputed z / a blocks."""
        _, z_o, a_k, z_k = ops.vqa_forward(feats, img_idx, q_emb, mutan_weights, want_a_orig=False)
        return ops.Batch(feats, img_idx, q_emb, z_o, z_k, a_k, answer_aids)
