"""Writes tests/golden/g18_gru_train.npz: the project's GRUEncoder on the CPU in eval mode under torch autograd (torch's own nn.Embedding +
nn.GRU and their backward, which is what pins this encoder) -- inputs, weights, a random dq_out, q and the five gradients of
sum(q * dq_out).  c0: the "ragged" case of tests/test_gru_gpu.py (dim_emb 22, dim_q 100, B 5, T 7: lengths {0, 1, 3, 7, 7}, a zero
inside a question, E[0] nonzero).  c1: dim_emb 22, dim_q 48, B 9, T 7, weights x 3 (gates that leave the linear range)."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
from vqa.models.seq2vec import GRUEncoder  # noqa: E402

V, DE, T = 50, 22, 7
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def main():
    out = {}
    for ci, (dq, lens, scale) in enumerate(((100, [0, 1, 3, 7, 7], 1.0), (48, [7, 1, 0, 5, 7, 2, 6, 4, 3], 3.0))):
        torch.manual_seed(ci)
        rng = np.random.default_rng(ci)
        enc = GRUEncoder(["w%d" % i for i in range(V)], dim_q=dq, dim_emb=DE, dropout=0.25).eval()
        with torch.no_grad():
            enc.embedding.weight[0] = torch.randn(DE) * 0.5          # padding_idx only zeroes the row at construction
            for p in enc.gru.parameters():
                p.mul_(scale)
        wids = np.zeros((len(lens), T), np.int64)
        for b, n in enumerate(lens):
            wids[b, :n] = rng.integers(1, V + 1, size=n)
        wids[3, 4 if ci == 0 else 2] = 0                              # a zero inside the question
        dq_out = rng.standard_normal((len(lens), dq)).astype(np.float32)
        q = enc(torch.from_numpy(wids))
        (q * torch.from_numpy(dq_out)).sum().backward()
        c = "c%d/" % ci
        out[c + "wids"], out[c + "dq_out"], out[c + "q"] = wids, dq_out, q.detach().numpy()
        out[c + "E"], out[c + "dE"] = enc.embedding.weight.detach().numpy(), enc.embedding.weight.grad.numpy()
        for k in WKEYS:
            out[c + k], out[c + "d" + k] = getattr(enc.gru, k).detach().numpy(), getattr(enc.gru, k).grad.numpy()
    path = os.path.join(ROOT, "tests", "golden", "g18_gru_train.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
