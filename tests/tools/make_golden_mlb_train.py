"""Generate tests/golden/g17_mlb_train.npz by RUNNING THE REFERENCE's training step on its MLBNoAtt: model.train() with every
dropout probability 0 (vqa/models/noatt.py:24-46, fusion.py:31-50), criterions.factory's loss (vqa/lib/criterions.py), loss.backward(),
utils.accuracy(topk=(1, 5)) (vqa/lib/utils.py:23-38) and one torch.optim.Adam(lr=1e-4) step (train.py:143-144, engine.py:22-37).

Uses oracle/make_golden.py's shims (imported, not changed) and a stored q_emb in place of the encoder, so that d loss / d q_emb is
the gradient of a leaf.  Cases at reduced widths, numpy-seeded weights wide enough to bend the tanh:
  c0  tanh / tanh / classif tanh, dv 64, dq 48, dh 32, A 40, B 5
  c1  activation_v absent, no classif.activation, dv 96, dq 40, dh 44, A 36, B 37
Planted in each: table row 3 all zero (question 2's image), the same image in questions 0 and 1, a duplicated answer id
(questions 0 and 3), question 1 with q_emb x 300 (linear_q saturates).

The fixture is data: inputs and the reference's outputs.  This script needs the reference checkout (build container only).
Usage:  python tests/tools/make_golden_mlb_train.py
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import oracle.make_golden as mg  # noqa: E402  (the shims; puts the reference first on sys.path)
import torch  # noqa: E402

import vqa.models as ref_models  # noqa: E402  (the reference package)
from vqa.lib import criterions, utils  # noqa: E402

assert ref_models.__file__.startswith(mg.REF), ref_models.__file__


class _Stored(torch.nn.Module):
    def __init__(self, q):
        super().__init__()
        self.q = q

    def forward(self, wids):
        return self.q


def run_case(seed, dv, dq, dh, A, B, act_v, act_c, gain):
    mg._StandInSeq2Vec.hidden = dq
    vocab_words = ["w%d" % i for i in range(40)]
    vocab_answers = ["a%d" % i for i in range(A)]
    fus = dict(dim_v=dv, dim_q=dq, dim_h=dh, dropout_v=0.0, dropout_q=0.0, activation_q="tanh")
    if act_v:
        fus["activation_v"] = act_v
    classif = dict(dropout=0.0)
    if act_c:
        classif["activation"] = act_c
    opt = dict(arch="MLBNoAtt", seq2vec=dict(arch="skipthoughts", dir_st="", type="BayesianUniSkip", dropout=0.25, fixed_emb=False),
               fusion=fus, classif=classif)
    torch.manual_seed(seed)
    vqa = ref_models.factory(copy.deepcopy(opt), vocab_words, vocab_answers, cuda=False, data_parallel=False)
    assert type(vqa).__name__ == "MLBNoAtt"
    rng = np.random.default_rng(seed)
    named = {n: p for n, p in vqa.named_parameters() if not n.startswith("seq2vec.")}
    with torch.no_grad():
        for name, p in named.items():
            fan_in = p.shape[1] if p.dim() == 2 else named[name.replace("bias", "weight")].shape[1]
            b = gain / np.sqrt(fan_in)
            p.copy_(torch.from_numpy(rng.uniform(-b, b, size=tuple(p.shape)).astype(np.float32)))
    names = sorted(named)
    init = {n: named[n].detach().numpy().copy() for n in names}

    n_img = B + 6
    feats = (np.abs(rng.standard_normal((n_img, dv))) * 0.45).astype(np.float32)
    feats[3] = 0.0
    img_idx = rng.permutation(n_img)[:B].astype(np.int32)
    img_idx[img_idx == 3] = 5
    img_idx[2] = 3
    img_idx[1] = img_idx[0]
    target = rng.integers(0, A, size=B).astype(np.int64)
    target[3] = target[0]
    q = (rng.standard_normal((B, dq)) * 0.3).astype(np.float32)
    q[1] *= 300.0
    q_t = torch.from_numpy(q.copy()).requires_grad_(True)
    vqa.seq2vec = _Stored(q_t)

    vqa.train()
    criterion = criterions.factory({}, cuda=False)
    optim = torch.optim.Adam([p for p in named.values()], lr=1e-4)
    out = vqa(torch.from_numpy(feats[img_idx]), torch.zeros(B, 4, dtype=torch.long))
    loss = criterion(out, torch.from_numpy(target))
    # utils.accuracy calls .view(-1) on a slice of a transposed tensor, which torch >= 1.x refuses: for the duration of the call
    # Tensor.view falls back to reshape (a shim of the same kind as make_golden's `.cuda()`; the reference's code is what runs)
    _view = torch.Tensor.view
    torch.Tensor.view = lambda t, *a: t.reshape(*a)
    try:
        acc1, acc5 = utils.accuracy(out.data, torch.from_numpy(target), topk=(1, 5))
    finally:
        torch.Tensor.view = _view
    optim.zero_grad()
    loss.backward()
    grads = {n: named[n].grad.detach().numpy().copy() for n in names}
    optim.step()
    res = dict(names=np.array(names), feats=feats, img_idx=img_idx, q_emb=q, target=target.astype(np.int32), logits=out.detach().numpy(),
               loss=np.float32(loss.item()), acc1=np.float32(float(acc1)), acc5=np.float32(float(acc5)), grad_q_emb=q_t.grad.numpy().copy(),
               dims=np.array([B, dv, dq, dh, A], np.int32))
    for n in names:
        res["init/" + n] = init[n]
        res["grad/" + n] = grads[n]
        res["after/" + n] = named[n].detach().numpy().copy()
    xq = np.tanh(q.astype(np.float64) @ init["fusion.linear_q.weight"].astype(np.float64).T + init["fusion.linear_q.bias"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5, "question 1 is meant to saturate linear_q"
    assert all(np.isfinite(v).all() for k, v in res.items() if v.dtype.kind == "f")
    return res


def main():
    out = {}
    for name, kw in (("c0", dict(seed=170, dv=64, dq=48, dh=32, A=40, B=5, act_v="tanh", act_c="tanh", gain=2.0)),
                     ("c1", dict(seed=171, dv=96, dq=40, dh=44, A=36, B=37, act_v=None, act_c=None, gain=2.0))):
        case = run_case(**kw)
        for k, v in case.items():
            out[name + "/" + k] = v
        print(name, "loss", float(case["loss"]), "acc1", float(case["acc1"]), "acc5", float(case["acc5"]), "max|logit|", float(np.abs(case["logits"]).max()),
              "max|dq|", float(np.abs(case["grad_q_emb"]).max()))
    path = os.path.join(GOLDEN, "g17_mlb_train.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
