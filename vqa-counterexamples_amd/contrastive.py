#!/usr/bin/env python3
"""Contrastive training / evaluation driver -- CLI drop-in for the reference's contrastive.py.

Keeps the reference's flags (contrastive.py:36-69), seeds, run-directory layout and checkpoint files (`logs/cx/<run>/{ckpt,best}/
{model,info}.ckpt`, :366-396), the five `contrastive/*` training metrics printed every --print_freq steps (:228-239), the
`contrastive/recall` evaluation metric (:259-290, Recall@5 of the counterexample among the 24 neighbours ranked FARTHEST first),
the best-checkpoint rule on it (:247-253) and the closing `test` line (:255-256).  The per-batch bodies -- ContrastiveModel's
forward, both ContrastiveLoss terms, backward, Adam (:213-224) and the distance ranking (:270-281) -- run on the HIP engine
(neuralcx.contrastive.ContrastiveEngine).  The training triple [original, counterexample, one other neighbour] is drawn on the
device, once per example and step, from a generator seeded with 42.

Net-new, as in counterexamples.py: --synthetic / --syn_*, --max_steps, --no_vqa_cache, --path_trainset, --path_features,
--project_dir; `optim.ckpt` (Adam moments) next to the reference's two files; scalars in `runs/<run>/{train,val}.jsonl`.
Tolerated defects of the reference: --pairwise cannot be turned off there (store_true with default True, :60): accepted and
ignored; load_cx_checkpoint reads info[-1]['recall'] although the key written is 'contrastive/recall' (:396): --resume accepts both.
Single GPU.
"""
import argparse
import os
import random
import sys
import time

import torch

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

import counterexamples as cxcli                                   # noqa: E402  (Runner: data loading, checkpoints, logging)
from neuralcx import dp, ops                                      # noqa: E402
from vqa.models.fusion import out_dim as fusion_out_dim          # noqa: E402
from neuralcx.contrastive import ContrastiveEngine, sample_positions, triple_img_idx, triple_z   # noqa: E402

RECALL_KEY = "contrastive/recall"
TRAIN_METRICS = ("contrastive/loss_comp", "contrastive/loss_other", "contrastive/loss", "contrastive/dist_comp", "contrastive/dist_other")


def build_parser():
    p = argparse.ArgumentParser(description="Train/Evaluate the contrastive counterexample model (MI355X HIP path)")
    p.add_argument("--path_opt", default=os.path.join(HERE, "options", "cx", "neuralcx_256_1_all.yaml"), type=str)
    p.add_argument("-lr", "--learning_rate", type=float, help="initial learning rate")
    p.add_argument("-b", "--batch_size", type=int, help="mini-batch size")
    p.add_argument("--epochs", type=int, help="number of total epochs to run")
    p.add_argument("--resume", default="", type=str, help="run name to resume")
    p.add_argument("--best", action="store_true", help="whether to resume best checkpoint")
    p.add_argument("-c", "--comment", type=str, default="")
    p.add_argument("-p", "--print_freq", default=100, type=int)
    p.add_argument("-v", "--eval_freq", default=-1, type=int)
    p.add_argument("--pairwise", action="store_true", default=True, help="accepted and ignored: always on, as in the reference")
    g = p.add_mutually_exclusive_group(required=False)
    g.add_argument("--pretrained_vqa", dest="pretrained_vqa", action="store_true")
    g.add_argument("--untrained_vqa", dest="pretrained_vqa", action="store_false")
    p.set_defaults(pretrained_vqa=None)
    p.add_argument("--trainable_vqa", action="store_true")
    p.add_argument("-dev", "--dev_mode", action="store_true")
    # net-new (as in counterexamples.py)
    p.add_argument("--project_dir", default=os.getcwd(), type=str)
    p.add_argument("--synthetic", action="store_true", help="synthetic data of the real shapes (no datasets offline)")
    p.add_argument("--syn_train", type=int, default=16384)
    p.add_argument("--syn_val", type=int, default=4096)
    p.add_argument("--syn_images", type=int, default=82783)
    p.add_argument("--max_steps", type=int, default=-1, help="stop an epoch early (smoke runs)")
    p.add_argument("--no_vqa_cache", action="store_true", help="produce z per batch instead of once per split")
    p.add_argument("--path_trainset", type=str, default=None, help="overrides vqa.path_trainset of the YAML")
    p.add_argument("--path_features", type=str, default=None, help="overrides coco.path_features / path_raw of the YAML")
    return p


def last_recall(info):
    """Best-so-far seed of a resumed run: the last epoch's recall under the key contrastive.py writes or the one it reads (:284, :396)."""
    last = info[-1]
    if RECALL_KEY in last:
        return last[RECALL_KEY]
    return last["recall"]


class ContrastiveRunner(cxcli.Runner):
    def __init__(self, args, options):
        self.args, self.opt = args, options
        if int(os.environ.get("WORLD_SIZE", "1")) > 1:
            raise SystemExit("contrastive.py runs on one GPU (no data-parallel contrastive step yet): launch it without torch.distributed.run")
        self.rank, self.world, self.local = 0, 1, 0
        if not torch.cuda.is_available():
            raise SystemExit("contrastive.py: an MI355X is required (the HIP path has no CPU fallback)")
        torch.cuda.set_device(self.local)
        self.dev = torch.device("cuda", self.local)
        random.seed(42); torch.manual_seed(42); torch.cuda.manual_seed(42)
        fus = options["model"]["fusion"]
        self.K = 24                                                      # contrastive.py:270
        self.engine = ContrastiveEngine(dv=fus["dim_v"], dz=fusion_out_dim(fus), A=options["vqa"]["nans"], lr=options["optim"]["lr"],
                                        device=self.dev)
        self.engine.init_parameters(seed=42)
        self.gb = options["optim"]["batch_size"]
        self.baseline = None
        self.runs_dir = None
        self.sem_gram = self.sem_flag = None
        self.gen = torch.Generator(device=self.dev)
        self.gen.manual_seed(42)

    # ---- data -----------------------------------------------------------------------------------------------
    def load_real(self):
        """Runner.load_real with a cache of z alone: this path never reads q or the answer logits (98 MB per 512 examples)."""
        want_cache, self.args.no_vqa_cache = not self.args.no_vqa_cache, True
        try:
            super().load_real()
        finally:
            self.args.no_vqa_cache = not want_cache
        if want_cache:
            for name, ds in (("train", self.train), ("val", self.val)):
                z_o, z_k = [], []
                for i in range(0, ds.N, 2048):
                    sel = torch.arange(i, min(i + 2048, ds.N), device=self.dev)
                    img_idx, wids, _, _ = ds.batch_indices(sel)
                    _, zo, zk, _ = self._vqa_outputs(ds, img_idx, wids)
                    z_o.append(zo); z_k.append(zk)
                ds.z_cache = (torch.cat(z_o), torch.cat(z_k))
                self.log("=> cached z of the {} split: {} examples, {:.2f} GB".format(name, ds.N, sum(t.numel() for t in ds.z_cache) * 4 / 1e9))

    def _synthetic_z(self, data, B, first_id, K):
        g = data._gen
        g.manual_seed(data.seed * 1000003 + int(first_id) * 7919 + B)
        return (torch.randn(B, data.dz, generator=g, device=self.dev), torch.randn(B, K, data.dz, generator=g, device=self.dev))

    def train_batch(self, data, sel, first_id):
        """The P = 3 batch [original, counterexample, other] (contrastive.py:213, 346-351), sampled on the device."""
        img_idx, gt = data.img_idx.index_select(0, sel), data.gt.index_select(0, sel)
        pos = sample_positions(gt, self.K, self.gen)
        idx3 = triple_img_idx(img_idx, pos)
        if self.vqa is None:
            z_o, z_k = self._synthetic_z(data, sel.numel(), first_id, 2)
        elif getattr(data, "z_cache", None) is not None:
            z_o, z_k = data.z_cache[0].index_select(0, sel), triple_z(data.z_cache[1], pos, sel)
        else:                                                            # --no_vqa_cache: the frozen VQA model on the three images
            _, z_o, z_k, _ = self._vqa_outputs(data, idx3, data.question_wids.index_select(0, sel))
        return ops.Batch(data.feats, idx3, None, z_o.contiguous(), z_k.contiguous(), None)

    def eval_batch(self, data, sel, first_id):
        img_idx, gt = data.img_idx.index_select(0, sel), data.gt.index_select(0, sel)
        if self.vqa is None:
            z_o, z_k = self._synthetic_z(data, sel.numel(), first_id, self.K)
        elif getattr(data, "z_cache", None) is not None:
            z_o, z_k = data.z_cache[0].index_select(0, sel), data.z_cache[1].index_select(0, sel)
        else:
            _, z_o, z_k, _ = self._vqa_outputs(data, img_idx, data.question_wids.index_select(0, sel))
        return ops.Batch(data.feats, img_idx, None, z_o.contiguous(), z_k.contiguous(), None), gt

    # ---- loops ----------------------------------------------------------------------------------------------
    def run_epoch(self, epoch):
        """-> (examples / s, the epoch's last evaluation result): contrastive.py:190-245."""
        eng, tr = self.engine, self.train
        ids, plan = dp.epoch_plan(tr.N, self.gb, epoch, 0, 1, self.dev, seed=42)
        if self.args.max_steps >= 0:
            plan = plan[:self.args.max_steps]
        t0 = time.time(); seen = 0; res = None
        for bi, (lo, hi, n_global, first_id, active) in enumerate(plan):
            r = eng.train_step(self.train_batch(tr, ids[lo:hi], first_id))
            seen += hi - lo
            if (bi + 1) % self.args.print_freq == 0:
                m = {k: float(r[k.split("/")[1]]) for k in TRAIN_METRICS}          # (the host syncs here only)
                self.report("train", epoch, m, step=(epoch - 1) * len(plan) + bi + 1)
            if (self.args.eval_freq > 0 and (bi + 1) % self.args.eval_freq == 0) or bi + 1 == len(plan):
                res = self.evaluate(self.val)
                self.report("val", epoch, res, step=(epoch - 1) * len(plan) + bi + 1)
        torch.cuda.synchronize()
        return seen / max(time.time() - t0, 1e-9), (res if res is not None else self.evaluate(self.val))

    def evaluate(self, data):
        tot = torch.zeros(2, dtype=torch.float64, device=self.dev)
        ids, plan = dp.epoch_plan(data.N, self.gb, 0, 0, 1, self.dev, shuffle=False)
        for lo, hi, n_global, first_id, active in plan:
            b, gt = self.eval_batch(data, ids[lo:hi], first_id)
            r = self.engine.eval_step(b, gt)
            tot[0] += r["hits"][1]; tot[1] += hi - lo
        h5, n = tot.tolist()
        return {RECALL_KEY: h5 / max(n, 1)}

    def load(self, save_dir, best):
        sub = "best" if best else "ckpt"
        state = torch.load(os.path.join(save_dir, sub, "model.ckpt"), map_location="cpu")
        self.engine.load_state({k: v for k, v in state.items() if not k.startswith("vqa_model.")})
        info = torch.load(os.path.join(save_dir, sub, "info.ckpt"))
        assert len(info) > 0
        po = os.path.join(save_dir, sub, "optim.ckpt")
        if os.path.isfile(po):                      # (absent in checkpoints written by the reference: Adam restarts, as there)
            self.engine.load_optimizer_state(torch.load(po, map_location="cpu"))
        self.log("Epoch {}: {}".format(len(info), info[-1]))
        return info, len(info) + 1, last_recall(info)


def main(argv=None):
    args = build_parser().parse_args(argv)
    if args.trainable_vqa:
        raise SystemExit("--trainable_vqa is outside the accelerated path (frozen VQA model only)")
    args.cx_model, args.test, args.viz, args.bf16, args.x6, args.sb_lambda = "ContrastiveModel", False, False, False, False, None
    options = cxcli.load_options(args)
    r = ContrastiveRunner(args, options)
    run = args.resume or "contrastive_{}{}".format(time.strftime("%m%d_%H%M%S"), "_" + args.comment if args.comment else "")
    save_dir = os.path.join(args.project_dir, "logs", "cx", run)
    r.runs_dir = os.path.join(args.project_dir, "runs", run)
    if args.synthetic:
        r.load_synthetic()
    else:
        r.load_real()
    info, start_epoch, best_recall = [], 1, 0.0
    if args.resume:
        info, start_epoch, best_recall = r.load(save_dir, args.best)
    r.log("=> Starting training... (1 GPU, batch {}, {} train / {} val examples)".format(r.gb, r.train.N, r.val.N))
    r.log("==> Pairwise training")
    for epoch in range(start_epoch, options["optim"]["epochs"] + 1):
        eps, res = r.run_epoch(epoch)
        r.engine.check_ids()
        r.log("Epoch {} throughput: {:.0f} examples/s".format(epoch, eps))
        info.append(res)
        is_best = res[RECALL_KEY] > best_recall
        best_recall = max(best_recall, res[RECALL_KEY])
        r.save(save_dir, info, is_best)
    res = r.evaluate(r.val)                                                   # contrastive.py:255-256
    r.report("test", 0, res, step=0)
    if torch.distributed.is_initialized():
        torch.distributed.barrier(); torch.distributed.destroy_process_group()
    return res


if __name__ == "__main__":
    main()
