"""Generate tests/golden/g14_mlb.npz by RUNNING THE REFERENCE's MLBNoAtt (vqa/models/noatt.py:38-46, fusion.py:16-50) through the
reference's CXModelBase.vqa_forward (vqa/models/cx.py:64-104).

Uses oracle/make_golden.py's shims (imported, not changed: stub modules for the absent third-party imports, `.cuda()` as the
identity) and its stand-in question encoder.  The encoder is an input producer: its output q_emb is stored, and the planted
question is written into it before the fusion sees it.

Cases, at reduced widths (each: feature table [n_img, dv], img_idx [B, K + 1], question ids, q_emb, the reference model's
state_dict, and the reference's a_orig, z_orig, a_knns, z_knns):
  c0  tanh everywhere (activation_v, activation_q, classif.activation): dv 64, dq 48, dh 32, A 40, B 5, K 24
  c1  classif.activation absent, dh = 44 (not a multiple of 32): dv 96, dq 40, A 36, B 4, K 24
Both with planted rows: table row 3 all zero (used by question 0 as a candidate and by question 2 as the original image),
question 1 with q_emb x 300 (linear_q saturates tanh), the same image id twice in question 0's list (candidates 4 and 9).

The fixture is data: inputs and the reference's outputs.  This script needs the reference checkout (build container only).
Usage:  python tests/tools/make_golden_mlb.py
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
from vqa.models.cx import CXModelBase  # noqa: E402

assert ref_models.__file__.startswith(mg.REF), ref_models.__file__


class _Stored(torch.nn.Module):
    """Hands the stored (planted) q_emb to vqa_forward in place of the encoder that produced it."""

    def __init__(self, q):
        super().__init__()
        self.q = q

    def forward(self, wids):
        return self.q


def run_case(seed, dv, dq, dh, A, B, K, classif_act, gain):
    mg._StandInSeq2Vec.hidden = dq
    vocab_words = ["w%d" % i for i in range(40)]
    vocab_answers = ["a%d" % i for i in range(A)]
    classif = dict(dropout=0.5)
    if classif_act:
        classif["activation"] = classif_act
    opt = dict(arch="MLBNoAtt",
               seq2vec=dict(arch="skipthoughts", dir_st="", type="BayesianUniSkip", dropout=0.25, fixed_emb=False),
               fusion=dict(dim_v=dv, dim_q=dq, dim_h=dh, dropout_v=0.5, dropout_q=0.5, activation_v="tanh", activation_q="tanh"),
               classif=classif)
    torch.manual_seed(seed)
    vqa = ref_models.factory(copy.deepcopy(opt), vocab_words, vocab_answers, cuda=False, data_parallel=False)
    assert type(vqa).__name__ == "MLBNoAtt"
    vqa.eval()
    rng = np.random.default_rng(seed)
    with torch.no_grad():           # numpy-seeded weights (stable across torch builds), wide enough to bend the tanh
        for name, p in vqa.named_parameters():
            if name.startswith("seq2vec."):
                continue
            fan_in = p.shape[1] if p.dim() == 2 else dict(vqa.named_parameters())[name.replace("bias", "weight")].shape[1]
            b = gain / np.sqrt(fan_in)
            p.copy_(torch.from_numpy(rng.uniform(-b, b, size=tuple(p.shape)).astype(np.float32)))
    state = {k: v.detach().numpy().copy() for k, v in vqa.state_dict().items()}

    n_img = B * (K + 1) + 7
    feats = (np.abs(rng.standard_normal((n_img, dv))) * 0.45).astype(np.float32)
    feats[3] = 0.0
    img_idx = rng.permutation(n_img)[:B * (K + 1)].reshape(B, K + 1).astype(np.int32)
    img_idx[img_idx == 3] = 5
    img_idx[0, 1 + 2] = 3
    img_idx[2, 0] = 3
    img_idx[0, 1 + 9] = img_idx[0, 1 + 4]
    wids = np.zeros((B, 9), np.int64)
    for b in range(B):
        n = int(rng.integers(3, 9))
        wids[b, :n] = rng.integers(1, len(vocab_words) + 1, size=n)
    with torch.no_grad():
        q = vqa.seq2vec(torch.from_numpy(wids)).clone()
    q[1] *= 300.0
    vqa.seq2vec = _Stored(q)

    m = CXModelBase(vqa, knn_size=K, trainable_vqa=False)
    dense = torch.from_numpy(feats[img_idx.reshape(-1)].reshape(B, K + 1, dv))
    a_o, z_o, a_k, z_k, q_out = m.vqa_forward(dense, torch.from_numpy(wids))
    assert torch.equal(q_out, q)
    out = dict(feats=feats, img_idx=img_idx, question_wids=wids.astype(np.int32), q_emb=q.numpy().copy(),
               a_orig=a_o.detach().numpy(), z_orig=z_o.detach().numpy(), a_knns=a_k.detach().numpy(), z_knns=z_k.detach().numpy(),
               state_keys=np.array(sorted(state)), dims=np.array([dv, dq, dh, A, B, K], np.int32),
               classif_activation=np.array(classif_act or ""))
    for k, v in state.items():
        out["state/" + k] = v
    for k in ("a_orig", "z_orig", "a_knns", "z_knns"):
        assert out[k].dtype == np.float32 and np.isfinite(out[k]).all()
    xq = np.tanh(q.numpy().astype(np.float64) @ state["fusion.linear_q.weight"].astype(np.float64).T + state["fusion.linear_q.bias"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5, "question 1 is meant to saturate linear_q"
    return out


def main():
    out = {}
    for name, kw in (("c0", dict(seed=140, dv=64, dq=48, dh=32, A=40, B=5, K=24, classif_act="tanh", gain=3.0)),
                     ("c1", dict(seed=141, dv=96, dq=40, dh=44, A=36, B=4, K=24, classif_act=None, gain=3.0))):
        case = run_case(**kw)
        for k, v in case.items():
            out[name + "/" + k] = v
        print(name, {k: case[k].shape for k in ("feats", "img_idx", "q_emb", "a_knns", "z_knns")}, "max|z|", float(np.abs(case["z_knns"]).max()),
              "max|a|", float(np.abs(case["a_knns"]).max()))
    path = os.path.join(GOLDEN, "g14_mlb.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
