"""Trains a no-attention VQA model (model.arch: MutanNoAtt, the default YAML, or MLBNoAtt): the producer of
<logs.dir_logs>/best_model.pth.tar, the checkpoint counterexamples.py and contrastive.py load with pretrained_vqa.  Also trains the
MLBAtt attention model (options/vqa2/mlb_att_train.yaml, --synthetic only) on the module route: see below.

Keeps the reference's flags where they apply (train.py:20-67), its loop (vqa/lib/engine.py:6-100: CrossEntropyLoss, Adam over the
parameters that require grad, acc1 / acc5) and its checkpoint files (train.py:290-367: <dir_logs>/{ckpt,best}_{info,model,optim}
.pth.tar, best by val acc1, --resume ckpt|best).  Data: what counterexamples.py already reads (pickle_old/*.pickle and the
feature tables through neuralcx.formats; each example is its original image, question_wids and answer_aid) or --synthetic.

Three routes:
  --freeze_seq2vec          q_emb is computed ONCE per split by the (frozen) question encoder and kept resident; the whole step is HIP
                            (neuralcx.vqa_train.VqaTrainEngine, MlbTrainEngine for MLBNoAtt: forward, cross-entropy, backward, Adam).
  (default)                 the module route: the model's use_hip_train = True, the fusion and classifier run in HIP inside torch
                            autograd, the encoder trains under autograd, torch.optim.Adam steps.  With --hip_seq2vec_train the encoder's
                            forward and backward through time run in HIP too (GRUEncoder.use_hip_train, neuralcx.vqa_train.GruTrainFunction);
                            --hip_2lstm_train is the same for the 2-lstm encoder (TwoLSTM.use_hip_bptt, neuralcx.vqa_train.LstmTrainFunction).
  --no_hip                  the same loop on the plain PyTorch modules (also runs on a CPU).
model.arch MLBAtt: training is the module under torch autograd by default (there is no flat-parameter engine for the attention model,
with or without --freeze_seq2vec); --hip_att_train sets the model's use_hip_train: the step below the question encoder (attention head,
glimpse fusion, classifier; forward with dropout and backward) then runs in HIP inside torch autograd
(neuralcx.vqa_train.MlbAttTrainFunction), the encoder trains under autograd unless --freeze_seq2vec, torch.optim.Adam steps.  evaluate() / --evaluate run the module in eval mode under no_grad, i.e. its HIP forward
(ncx_mlb_att_forward), unless --no_hip.  --x6 sets the model's hip_x6: both HIP routes of the attention model then run the conv_v_att
product on the bf16 matrix path with three-plane operands (NCX_F_X6: same results to fp32 rounding; not the default), and with
--hip_att_train the backward runs its twin, d conv_v_att.weight, there as well.  --x6_seq2vec is the same choice for the GRU question
encoder (any arch): it sets GRUEncoder.hip_x6, and the encoder's HIP forward (eval mode and --hip_seq2vec_train) runs the bf16 x 6 form of
its step kernel, and with --hip_seq2vec_train its backward through time runs the bf16 x 6 form of its four matrix products -- the
reverse sweep, dX, dW_hh, dW_ih (ncx_gru_train_backward_flags, ops.gru_bwd_form); --x6_2lstm is that choice for the 2-lstm encoder (TwoLSTM.hip_x6: its eval-mode forward and --hip_2lstm_train run
k_lstm_step_x6).  The images are a seeded synthetic attention table [syn_images, dim_v, syn_grid, syn_grid].
"""
import argparse
import json
import os
import shutil
import sys
import time

import torch
import torch.nn as nn
import yaml

HERE = os.path.dirname(os.path.abspath(__file__))
if HERE not in sys.path:
    sys.path.insert(0, HERE)

from vqa import models                                       # noqa: E402
from vqa.lib import utils                                    # noqa: E402

CKPT_PARTS = ("info", "model", "optim")
ATT_ARCHS = ("MLBAtt",)                                      # models whose image input is the NCHW map [B, dim_v, W, H]


def build_parser():
    p = argparse.ArgumentParser(description="Train / evaluate a no-attention VQA model (MutanNoAtt, MLBNoAtt)", formatter_class=argparse.ArgumentDefaultsHelpFormatter)
    p.add_argument("--path_opt", default=os.path.join(HERE, "options", "vqa2", "mutan_noatt_train.yaml"), type=str)
    p.add_argument("--dir_logs", type=str, help="dir logs")
    p.add_argument("--st_dropout", type=float)
    p.add_argument("--st_fixed_emb", default=None, type=utils.str2bool, help="do not backprop into the word embedding")
    p.add_argument("-lr", "--learning_rate", type=float, help="initial learning rate")
    p.add_argument("-b", "--batch_size", type=int, help="mini-batch size")
    p.add_argument("--epochs", type=int, help="number of total epochs to run")
    p.add_argument("--start_epoch", default=0, type=int, help="manual epoch number (useful on restarts)")
    p.add_argument("--resume", default="", type=str, help="ckpt | best: resume <dir_logs>/<resume>_{info,model,optim}.pth.tar")
    p.add_argument("--save_model", default=True, type=utils.str2bool, help="save model and optim state")
    p.add_argument("-e", "--evaluate", dest="evaluate", action="store_true", help="evaluate on the validation set and exit")
    p.add_argument("--print_freq", "-p", default=10, type=int, help="print frequency")
    # net-new
    p.add_argument("--synthetic", action="store_true", help="synthetic data (neuralcx.synth.SyntheticVQA): no datasets offline")
    p.add_argument("--syn_examples", type=int, default=8192)
    p.add_argument("--syn_images", type=int, default=1024)
    p.add_argument("--syn_vocab", type=int, default=1000)
    p.add_argument("--syn_grid", type=int, default=14, help="attention archs only: the synthetic maps are [dim_v, syn_grid, syn_grid]")
    p.add_argument("--path_trainset", type=str, default=None, help="overrides vqa.path_trainset of the YAML")
    p.add_argument("--path_features", type=str, default=None, help="overrides coco.path_features of the YAML")
    p.add_argument("--freeze_seq2vec", action="store_true", help="freeze the question encoder: q_emb once per split, the whole step in HIP")
    p.add_argument("--hip_seq2vec_train", action="store_true", help="default route only: train the question encoder in HIP as well (backward through time)")
    p.add_argument("--hip_2lstm_train", action="store_true", help="default route only: train the 2-lstm question encoder (TwoLSTM) in HIP as well (backward through time)")
    p.add_argument("--hip_att_train", action="store_true", help="attention archs only: the training step below the question encoder in HIP as well "
                   "(MLBAtt.use_hip_train: attention head, glimpse fusion, classifier; torch.optim.Adam steps)")
    p.add_argument("--x6", action="store_true", help="attention archs only: NCX_F_X6 on the attention kernel, same results to fp32 rounding; not the default")
    p.add_argument("--x6_seq2vec", action="store_true", help="GRU question encoder only: NCX_F_X6 on its HIP step kernel, same results to fp32 rounding; not the default")
    p.add_argument("--x6_2lstm", action="store_true", help="2-lstm question encoder only: NCX_F_X6 on its HIP step kernel, same results to fp32 rounding; not the default")
    p.add_argument("--no_hip", action="store_true", help="the plain PyTorch modules (no HIP library; runs on a CPU too)")
    p.add_argument("--seed", type=int, default=1337)
    return p


def load_options(args):
    options = {"logs": {"dir_logs": args.dir_logs},
               "model": {"seq2vec": {"dropout": args.st_dropout, "fixed_emb": args.st_fixed_emb}},
               "optim": {"lr": args.learning_rate, "batch_size": args.batch_size, "epochs": args.epochs}}
    with open(args.path_opt) as f:
        from_yaml = yaml.safe_load(f)
    return utils.update_values(options, from_yaml)


def ckpt_paths(dir_logs, tag):
    """train.py:293-298 / 333-335: <dir_logs>/<tag>_{info,model,optim}.pth.tar, tag in {ckpt, best}"""
    return {part: os.path.join(dir_logs, "%s_%s.pth.tar" % (tag, part)) for part in CKPT_PARTS}


class _Split:
    def __init__(self, feats, img_idx, wids, aids):
        self.feats, self.img_idx, self.wids, self.aids = feats, img_idx, wids, aids
        self.N = img_idx.shape[0]
        self.q_emb = None


def load_data(args, opt, dev):
    """-> (train split, val split, vocab_words, vocab_answers)"""
    att = opt["model"].get("arch") in ATT_ARCHS
    if att and not args.synthetic:
        raise SystemExit("train.py: model.arch %s reads attention tables (hdf5 'att', [n_img, dim_v, 14, 14]); real-data attention tables "
                         "are not supported, use --synthetic" % opt["model"]["arch"])
    if args.synthetic:
        from neuralcx.synth import SyntheticVQA
        dv = opt["model"]["dim_v"] if att else opt["model"]["fusion"]["dim_v"]
        s = SyntheticVQA(n_examples=args.syn_examples, n_img=args.syn_images, dv=dv, vocab=args.syn_vocab,
                         T=opt["vqa"].get("maxlength", 26), A=opt["vqa"]["nans"], seed=1234, device=dev)
        feats = s.feats
        if att:             # the attention table: every image row spread over a syn_grid x syn_grid map by seeded factors in [0, 2)
            g = torch.Generator(device=dev).manual_seed(1234 + 1)
            feats = s.feats[:, :, None, None] * (2.0 * torch.rand(args.syn_images, dv, args.syn_grid, args.syn_grid, generator=g, device=dev))
        n = s.n_train
        return (_Split(feats, s.img_idx[:n], s.question_wids[:n], s.answer_aids[:n]),
                _Split(feats, s.img_idx[n:], s.question_wids[n:], s.answer_aids[n:]), s.vocab_words, s.vocab_answers)
    from neuralcx import formats
    vqa_dir = args.path_trainset or opt["vqa"].get("path_trainset")
    feat_dir = args.path_features or opt["coco"].get("path_features")
    if not vqa_dir or not feat_dir:
        raise SystemExit("real-data mode needs vqa.path_trainset and coco.path_features (YAML or --path_trainset / --path_features)")
    pk = lambda fn: formats.load_cx_pickle(os.path.join(vqa_dir, "pickle_old", fn))
    trainset, valset = pk("trainset_augmented.pickle"), pk("valset_augmented_small.pickle")
    tr = formats.CXDeviceDataset(trainset, formats.load_feature_table(feat_dir, "train"), dev)
    va = formats.CXDeviceDataset(valset, formats.load_feature_table(feat_dir, "val"), dev)
    mk = lambda d: _Split(d.feats, d.img_idx[:, 0].contiguous(), d.question_wids, d.answer_aids)       # the original image of each example
    return mk(tr), mk(va), trainset["vocab_words"], trainset["vocab_answers"]


class Trainer:
    def __init__(self, args, opt):
        self.args, self.opt = args, opt
        cuda = torch.cuda.is_available()
        if args.hip_seq2vec_train and args.no_hip:
            raise SystemExit("train.py: --hip_seq2vec_train trains the encoder in HIP; it cannot be combined with --no_hip")
        if args.hip_seq2vec_train and args.freeze_seq2vec:
            raise SystemExit("train.py: --hip_seq2vec_train has nothing to train under --freeze_seq2vec")
        if args.hip_2lstm_train and args.no_hip:
            raise SystemExit("train.py: --hip_2lstm_train trains the encoder in HIP; it cannot be combined with --no_hip")
        if args.hip_2lstm_train and args.freeze_seq2vec:
            raise SystemExit("train.py: --hip_2lstm_train has nothing to train under --freeze_seq2vec")
        if args.hip_att_train and args.no_hip:
            raise SystemExit("train.py: --hip_att_train trains the attention model in HIP; it cannot be combined with --no_hip")
        if args.hip_att_train and opt["model"].get("arch") not in ATT_ARCHS:
            raise SystemExit("train.py: --hip_att_train needs an attention arch (%s); this YAML builds %r" % (", ".join(ATT_ARCHS), opt["model"].get("arch")))
        if args.x6 and args.no_hip:
            raise SystemExit("train.py: --x6 picks a form of the HIP attention kernel; it cannot be combined with --no_hip")
        if args.x6 and opt["model"].get("arch") not in ATT_ARCHS:
            raise SystemExit("train.py: --x6 needs an attention arch (%s); this YAML builds %r" % (", ".join(ATT_ARCHS), opt["model"].get("arch")))
        s2v = opt["model"]["seq2vec"]
        if getattr(args, "x6_seq2vec", False) and args.no_hip:
            raise SystemExit("train.py: --x6_seq2vec picks a form of the HIP step kernel of the GRU encoder; it cannot be combined with --no_hip")
        if getattr(args, "x6_seq2vec", False) and s2v.get("arch") == "2-lstm" and "hidden_size" in s2v:                   # seq2vec.factory's TwoLSTM branch
            raise SystemExit("train.py: --x6_seq2vec needs the GRU encoder; this YAML builds the 2-lstm encoder, whose bf16 x 6 step kernel is picked with --x6_2lstm")
        if getattr(args, "x6_2lstm", False) and args.no_hip:
            raise SystemExit("train.py: --x6_2lstm picks a form of the HIP step kernel of the 2-lstm encoder; it cannot be combined with --no_hip")
        if getattr(args, "x6_2lstm", False) and not (s2v.get("arch") == "2-lstm" and "hidden_size" in s2v):     # seq2vec.factory's TwoLSTM branch
            raise SystemExit("train.py: --x6_2lstm needs the 2-lstm encoder (seq2vec: {arch: 2-lstm, hidden_size: ...}); this YAML builds %r"
                             % s2v.get("arch", "skipthoughts"))
        if args.hip_2lstm_train and not (s2v.get("arch") == "2-lstm" and "hidden_size" in s2v):       # seq2vec.factory's TwoLSTM branch
            raise SystemExit("train.py: --hip_2lstm_train needs the 2-lstm encoder (seq2vec: {arch: 2-lstm, hidden_size: ...}); this YAML builds %r"
                             % s2v.get("arch", "skipthoughts"))
        if not cuda and not args.no_hip:
            raise SystemExit("train.py: the HIP routes need an MI355X (use --no_hip for the PyTorch modules)")
        self.dev = torch.device("cuda:0" if cuda else "cpu")
        torch.manual_seed(args.seed)
        self.train, self.val, vw, va = load_data(args, opt, self.dev)
        self.model = models.factory(opt["model"], vw, va, cuda=cuda, data_parallel=False)
        self.lr, self.B = opt["optim"]["lr"], opt["optim"]["batch_size"]
        self.freeze = args.freeze_seq2vec
        from neuralcx import vqa_train
        mlb = opt["model"].get("arch") == "MLBNoAtt"
        self.att = opt["model"].get("arch") in ATT_ARCHS
        route_for, engine_cls = (vqa_train.mlb_route_for, vqa_train.MlbTrainEngine) if mlb else (vqa_train.route_for, vqa_train.VqaTrainEngine)
        if self.att:            # no HIP training step for the attention model: the module trains under autograd, its eval forward is HIP
            self.route = "torch path: --no_hip" if args.no_hip else \
                "module under torch autograd; eval-mode forward in HIP (ncx_mlb_att_forward)%s" % (
                    "; --freeze_seq2vec: the encoder is frozen, there is no HIP engine for this model" if self.freeze else "")
            self.model.use_hip = not args.no_hip
            if args.hip_att_train:
                from neuralcx import ops
                if ops.mlb_att_acts(opt["model"]) is None:
                    raise SystemExit("train.py: --hip_att_train needs the HIP route: an activation of this YAML is neither absent nor tanh")
                self.model.use_hip_train = True
                self.route = "attention head, glimpse fusion and classifier train in HIP (ncx_mlb_att_train_forward / _backward, --hip_att_train); " \
                    "torch.optim.Adam steps; eval-mode forward in HIP (ncx_mlb_att_forward)%s" % (
                        "; --freeze_seq2vec: the encoder is frozen, no d loss / d q_emb is taken" if self.freeze else "")
            if args.x6:
                self.model.hip_x6 = True
                self.route += " (bf16 x 6 attention kernel)"
                if args.hip_att_train:
                    self.route += " (and its weight-gradient twin in the backward)"
        else:
            self.route = "torch path: --no_hip" if args.no_hip else route_for(opt["model"])
        if getattr(args, "x6_seq2vec", False):
            if not isinstance(self.model.seq2vec, models.seq2vec.GRUEncoder):
                raise SystemExit("train.py: --x6_seq2vec needs the GRU encoder; this YAML builds %s" % type(self.model.seq2vec).__name__)
            self.model.seq2vec.hip_x6 = True
        if getattr(args, "x6_2lstm", False):
            if not isinstance(self.model.seq2vec, models.seq2vec.TwoLSTM):
                raise SystemExit("train.py: --x6_2lstm needs the TwoLSTM encoder; this YAML builds %s" % type(self.model.seq2vec).__name__)
            self.model.seq2vec.hip_x6 = True
        self.hip = self.route == "hip"
        self.engine = None
        if self.freeze or opt["model"]["seq2vec"].get("fixed_emb"):
            for n, p_ in self.model.seq2vec.named_parameters():
                if self.freeze or "embedding" in n:
                    p_.requires_grad_(False)
        if self.hip and self.freeze:
            self.engine = engine_cls.from_options(opt["model"], len(va), lr=self.lr, device=self.dev, seed=args.seed)
            self.engine.load_state_dict(self.model.state_dict())          # nn.Linear's init under --seed; seq2vec.* carried through
        else:
            if not self.att:
                self.model.use_hip_train = self.hip
            self.hip_seq2vec = bool(args.hip_seq2vec_train and self.hip and hasattr(type(self.model.seq2vec), "use_hip_train"))
            if args.hip_seq2vec_train and not self.hip_seq2vec:
                raise SystemExit("train.py: --hip_seq2vec_train needs the HIP route and the GRU encoder (%s); the 2-lstm encoder trains in HIP "
                                 "with --hip_2lstm_train" % self.route)
            if self.hip_seq2vec:
                self.model.seq2vec.use_hip_train = True
            self.hip_2lstm = bool(args.hip_2lstm_train and self.hip and isinstance(self.model.seq2vec, models.seq2vec.TwoLSTM))
            if args.hip_2lstm_train and not self.hip_2lstm:
                raise SystemExit("train.py: --hip_2lstm_train needs the HIP route and the TwoLSTM encoder (%s)" % self.route)
            if self.hip_2lstm:
                self.model.seq2vec.use_hip_bptt = True
            self.optim = torch.optim.Adam([p_ for p_ in self.model.parameters() if p_.requires_grad], self.lr)     # train.py:143-144
            self.criterion = nn.CrossEntropyLoss()
        self.best_acc1, self.history = 0.0, []
        print("=> route: %s%s%s%s%s" % ("hip" if self.hip else self.route, " (engine: whole step in HIP)" if self.engine else "",
                                    " (question encoder: HIP forward + backward through time)" if getattr(self, "hip_seq2vec", False) else
                                    " (2-lstm question encoder: HIP forward + backward through time, --hip_2lstm_train)" if getattr(self, "hip_2lstm", False)
                                    else "", (" (question encoder: bf16 x 6 step kernel)" + (" (and the bf16 x 6 products of its backward)" if getattr(self, "hip_seq2vec", False) else ""))
                                    if getattr(args, "x6_seq2vec", False) else "",
                                      " (2-lstm question encoder: bf16 x 6 step kernel)" if getattr(args, "x6_2lstm", False) else ""), flush=True)

    # ---- data ------------------------------------------------------------------------------------------------
    def q_emb_of(self, split):
        """--freeze_seq2vec: the encoder's output for a whole split, computed once (eval mode: its dropout is off) and kept resident."""
        if split.q_emb is None:
            self.model.seq2vec.eval()
            with torch.no_grad():
                split.q_emb = torch.cat([self.model.seq2vec(split.wids[i:i + 2048]).float() for i in range(0, split.N, 2048)]).contiguous()
        return split.q_emb

    # ---- steps -----------------------------------------------------------------------------------------------
    def _step(self, split, sel, train):
        idx, aids = split.img_idx.index_select(0, sel), split.aids.index_select(0, sel)
        if self.engine is not None:
            q = self.q_emb_of(split).index_select(0, sel)
            r = self.engine.train_step(split.feats, idx, q, aids) if train else self.engine.evaluate(split.feats, idx, q, aids)
            return r["loss"][0], r["hits1"][0].float(), r["hits5"][0].float()
        v = split.feats.index_select(0, idx.long())
        wids = split.wids.index_select(0, sel)
        with torch.set_grad_enabled(train):
            if self.freeze and self.att:
                logits = self.model.forward_from_q(v, self.q_emb_of(split).index_select(0, sel))
            elif self.freeze:                                     # (torch path only: the HIP route with a frozen encoder is the engine)
                logits = self.model._classif(self.model._fusion(v, self.q_emb_of(split).index_select(0, sel)))
            else:
                logits = self.model(v, wids)
            loss = self.criterion(logits, aids.long())
        if train:
            self.optim.zero_grad()
            loss.backward()
            self.optim.step()
        top = logits.detach().topk(min(5, logits.shape[1]), 1).indices                       # utils.accuracy (vqa/lib/utils.py:23-38), as counts
        hit = top == aids.long()[:, None]
        return loss.detach(), hit[:, :1].sum().float(), hit.sum().float()

    def run_epoch(self, epoch):
        torch.manual_seed(self.args.seed * 7919 + epoch)          # shuffle + torch dropout: an epoch depends on (seed, epoch, state) only
        if self.engine is None:
            self.model.train()
            if self.freeze:
                self.model.seq2vec.eval()
        perm = torch.randperm(self.train.N).to(self.dev)
        tot = torch.zeros(3, device=self.dev)
        t0, n = time.time(), 0
        for i, s in enumerate(range(0, self.train.N, self.B)):
            sel = perm[s:s + self.B]
            loss, h1, h5 = self._step(self.train, sel, True)
            tot += torch.stack([loss * sel.numel(), h1, h5])
            n += sel.numel()
            if self.args.print_freq > 0 and (i + 1) % self.args.print_freq == 0:
                l, a1, a5 = (tot / n).tolist()
                print("Epoch: [%d][%d/%d] loss %.4f acc1 %.2f acc5 %.2f (%.1f ex/s)" % (epoch, i + 1, -(-self.train.N // self.B), l, 100 * a1, 100 * a5,
                                                                                       n / (time.time() - t0)), flush=True)
        l, a1, a5 = (tot / n).tolist()
        return dict(loss=l, acc1=100 * a1, acc5=100 * a5)

    def evaluate(self):
        if self.engine is None:
            self.model.eval()
        tot, n = torch.zeros(3, device=self.dev), 0
        for s in range(0, self.val.N, self.B):
            sel = torch.arange(s, min(s + self.B, self.val.N), device=self.dev)
            loss, h1, h5 = self._step(self.val, sel, False)
            tot += torch.stack([loss * sel.numel(), h1, h5])
            n += sel.numel()
        if self.engine is not None:
            self.engine.check_targets()
        l, a1, a5 = (tot / max(n, 1)).tolist()
        return dict(loss=l, acc1=100 * a1, acc5=100 * a5)

    # ---- checkpoints (train.py:290-367) -------------------------------------------------------------------------
    def state_dict(self):
        sd = self.engine.state_dict() if self.engine is not None else self.model.state_dict()
        return {k: v.detach().cpu() for k, v in sd.items()}

    def save(self, dir_logs, info, is_best):
        os.makedirs(dir_logs, exist_ok=True)
        ck, best = ckpt_paths(dir_logs, "ckpt"), ckpt_paths(dir_logs, "best")
        with open(os.path.join(dir_logs, "logger.json"), "w") as f:
            json.dump(self.history, f)
        torch.save(info, ck["info"])
        parts = ["info"]
        if self.args.save_model:
            torch.save(self.state_dict(), ck["model"])
            torch.save(self.engine.optimizer_state() if self.engine is not None else self.optim.state_dict(), ck["optim"])
            parts += ["model", "optim"]
        else:
            print("Warning train.py: checkpoint not saved")
        if is_best:
            for part in parts:
                shutil.copyfile(ck[part], best[part])

    def load(self, dir_logs, tag):
        pth = ckpt_paths(dir_logs, tag)
        info = torch.load(pth["info"]) if os.path.isfile(pth["info"]) else {}
        if os.path.isfile(pth["model"]):
            sd = torch.load(pth["model"], map_location=self.dev)
            if self.engine is not None:
                self.engine.load_state_dict(sd)
            self.model.load_state_dict(sd)
        else:
            print("Warning train.py: no model checkpoint found at '%s'" % pth["model"])
        if os.path.isfile(pth["optim"]):
            st = torch.load(pth["optim"], map_location="cpu")
            self.engine.load_optimizer_state(st) if self.engine is not None else self.optim.load_state_dict(st)
        self.best_acc1 = float(info.get("best_acc1", 0.0))
        self.history = list(info.get("history", []))
        print("=> loaded checkpoint '%s' (epoch %d, best_acc1 %.4f)" % (tag, info.get("epoch", 0), self.best_acc1))
        return int(info.get("epoch", 0))


def main(argv=None):
    args = build_parser().parse_args(argv)
    opt = load_options(args)
    dir_logs = opt["logs"]["dir_logs"]
    t = Trainer(args, opt)
    start = args.start_epoch
    if args.resume:
        start = t.load(dir_logs, args.resume)
    if args.evaluate:
        val = t.evaluate()
        print("Val: loss %.4f acc1 %.2f acc5 %.2f" % (val["loss"], val["acc1"], val["acc5"]), flush=True)
        return dict(val=val, history=t.history, trainer=t)
    for epoch in range(start + 1, opt["optim"]["epochs"] + 1):
        tr = t.run_epoch(epoch)
        val = t.evaluate()
        print("Epoch %d: train loss %.4f acc1 %.2f | val loss %.4f acc1 %.2f acc5 %.2f" % (epoch, tr["loss"], tr["acc1"], val["loss"], val["acc1"],
                                                                                      val["acc5"]), flush=True)
        t.history.append(dict(epoch=epoch, train=tr, val=val))
        is_best = val["acc1"] >= t.best_acc1                      # (>=: the first epoch always writes best_*)
        t.best_acc1 = max(t.best_acc1, val["acc1"])
        t.save(dir_logs, dict(epoch=epoch, best_acc1=t.best_acc1, history=t.history, route=t.route, options=opt), is_best)
    return dict(history=t.history, trainer=t)


if __name__ == "__main__":
    main()
