"""Generate tests/golden/g11_scorers.npz and g11_scorers_adam.npz by RUNNING THE REFERENCE's LinearContext (vqa/models/cx.py:
139-156) and PairwiseLinearModel (cx.py:379-425) themselves, on CPU.

Uses oracle/make_golden.py's shims (imported, not changed).  A stub VQA model carries what the constructors read (opt['fusion'],
vocab_answers); the model's `vqa_forward` is replaced by one that returns stored q_emb, z_orig and z_knns (leaf tensors that
require grad, as cx.py:98-102 makes them).  The loss is the reference's, CrossEntropyLoss(size_average=False) / B
(counterexamples.py:310,334), and the optimiser torch.optim.Adam(model.parameters(), lr) (counterexamples.py:275).

Cases
  lc    LinearContext, B = 6, K = 24, dz = 8
  pl    PairwiseLinearModel, B = 5, K = 24 (the reference asserts it), dv = dq = dz = 4, A = 10, H = dim_a = 300:
        answer ids of triplets 1 and 3 are equal (the embedding gradient sums them); triplet 0's answer row is set so that
        every hidden unit with a positive out.weight sits 5 below 0 for it, and out.bias <= 0, so the whole triplet scores exactly 0
g11_scorers.npz holds inputs, initial state, scores, loss and every gradient after loss.backward(); g11_scorers_adam.npz the
parameters after 1 and 3 Adam steps (lr 1e-3) on the same batch (two files: each stays under 1 MiB).
Usage:  python tests/tools/make_golden_scorers.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import oracle.make_golden  # noqa: E402,F401  (the shims; puts the reference first on sys.path)
import torch  # noqa: E402

import vqa.models as ref_models  # noqa: E402  (the reference package)
from vqa.models.cx import LinearContext, PairwiseLinearModel  # noqa: E402

assert ref_models.__file__.startswith(oracle.make_golden.REF), ref_models.__file__

LR = 1e-3


class _StubVQA(torch.nn.Module):
    def __init__(self, dv, dq, dz, A):
        super().__init__()
        self.opt = {"fusion": {"dim_v": dv, "dim_q": dq, "dim_mm": dz}}
        self.vocab_answers = ["a%d" % i for i in range(A)]


def _stub_forward(q, z_o, z_k):
    def f(image_features, question_wids):
        return (None, torch.from_numpy(z_o).requires_grad_(True), None, torch.from_numpy(z_k).requires_grad_(True),
                torch.from_numpy(q))
    return f


def run(model, feats, q, z_o, z_k, aids, gt, prefix, out, adam_out):
    model.vqa_forward = _stub_forward(q, z_o, z_k)
    names = [n for n, _ in model.named_parameters()]
    out[prefix + "init/names"] = np.array(names)
    for n, p in model.named_parameters():
        out[prefix + "init/" + n] = p.detach().numpy().copy()
    crit = torch.nn.CrossEntropyLoss(reduction="sum")                          # size_average=False
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    B = feats.shape[0]
    for step in range(1, 4):
        scores = model(torch.from_numpy(feats), None, torch.from_numpy(aids))
        loss = crit(scores, torch.from_numpy(gt)) / B
        opt.zero_grad()
        loss.backward()
        if step == 1:
            out[prefix + "scores"] = scores.detach().numpy()
            out[prefix + "loss"] = np.float32(loss.item())
            for n, p in model.named_parameters():
                out[prefix + "grad/" + n] = p.grad.numpy().copy()
        opt.step()
        if step in (1, 3):
            for n, p in model.named_parameters():
                adam_out[prefix + "step%d/" % step + n] = p.detach().numpy().copy()


def main():
    torch.manual_seed(11)
    rng = np.random.default_rng(11)
    out, adam_out = {}, {}

    # ---- LinearContext ----
    B, K, dz = 6, 24, 8
    z_k = rng.standard_normal((B, K, dz)).astype(np.float32)
    gt = rng.integers(0, K, B).astype(np.int64)
    m = LinearContext(_StubVQA(4, 4, dz, 3), knn_size=K, trainable_vqa=False)
    feats = np.zeros((B, K + 1, 4), np.float32)
    out["lc/z_knns"], out["lc/gt"] = z_k, gt.astype(np.int32)
    run(m, feats, np.zeros((B, 4), np.float32), np.zeros((B, dz), np.float32), z_k, np.zeros(B, np.int64), gt, "lc/", out, adam_out)

    # ---- PairwiseLinearModel ----
    B, K, dv, dq, dz, A = 5, 24, 4, 4, 4, 10
    feats = rng.standard_normal((B, K + 1, dv)).astype(np.float32)
    q = rng.standard_normal((B, dq)).astype(np.float32)
    z_o = rng.standard_normal((B, dz)).astype(np.float32)
    z_k = rng.standard_normal((B, K, dz)).astype(np.float32)
    aids = np.array([7, 2, 5, 2, 0], np.int64)                              # triplets 1 and 3 share an answer id
    gt = rng.integers(0, K, B).astype(np.int64)
    m = PairwiseLinearModel(_StubVQA(dv, dq, dz, A), knn_size=K, trainable_vqa=False)
    with torch.no_grad():
        W = m.linear.weight.double().numpy()
        a0 = 2 * dv + dq + 2 * dz
        # E[aid_0]: the min-norm solution that puts every hidden unit with a positive out.weight 5 below 0 for triplet 0's
        # per-question part (the candidate part stays below 2 here); with out.bias <= 0 the triplet then scores exactly 0,
        # and the row stays small enough (entries below ~30) for fp32 sums over it to stay accurate through the Adam steps
        pos = m.out.weight.double().numpy()[0] > 0
        rest = W[:, :dv] @ feats[0, 0] + W[:, 2 * dv:2 * dv + dq] @ q[0] + W[:, 2 * dv + dq:2 * dv + dq + dz] @ z_o[0] + \
            m.linear.bias.double().numpy()
        e = np.linalg.lstsq(W[pos, a0:], -5.0 - rest[pos], rcond=None)[0]
        m.answer_embedding.weight[aids[0]] = torch.from_numpy(e.astype(np.float32))
        m.out.bias.fill_(-abs(float(m.out.bias)))
    for n, v in (("feats", feats), ("q_emb", q), ("z_orig", z_o), ("z_knns", z_k)):
        out["pl/" + n] = v
    out["pl/aids"], out["pl/gt"] = aids.astype(np.int32), gt.astype(np.int32)
    run(m, feats, q, z_o, z_k, aids, gt, "pl/", out, adam_out)
    assert (out["pl/scores"][0] == 0).all() and (out["pl/scores"][1:] > 0).any(), out["pl/scores"]

    for name, d in (("g11_scorers.npz", out), ("g11_scorers_adam.npz", adam_out)):
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **d)
        print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
