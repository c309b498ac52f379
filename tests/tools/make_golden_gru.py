"""Writes tests/golden/g15_gru.npz: small cases of the project's GRUEncoder on the CPU in eval mode (torch's own nn.Embedding + nn.GRU,
which is what pins this encoder) -- inputs, weights and q.  dim_emb 22, dim_q 100, B 9, T 7.
Rows: full length, length 1, all padding (length counts as 1; E[0] is made nonzero), a zero in the middle of a question, the rest random."""
import os
import sys

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
from vqa.models.seq2vec import GRUEncoder  # noqa: E402

V, DE, DQ, B, T = 30, 22, 100, 9, 7


def main():
    out = {}
    for ci, seed in enumerate((0, 1)):
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        enc = GRUEncoder(["w%d" % i for i in range(V)], dim_q=DQ, dim_emb=DE, dropout=0.25).eval()
        with torch.no_grad():
            enc.embedding.weight[0] = torch.randn(DE) * 0.5          # padding_idx only zeroes the row at construction
            for p in enc.gru.parameters():                            # beyond the default +-0.1 init: gates that leave the linear range
                p.mul_(3.0 if ci else 1.0)
        wids = np.zeros((B, T), np.int64)
        lens = [7, 1, 0, 5, 7] + list(rng.integers(1, T + 1, size=B - 5))
        for b, n in enumerate(lens):
            wids[b, :n] = rng.integers(1, V + 1, size=n)
        wids[3, 2] = 0                                                # a zero inside the question: 4 nonzero ids, stepped over t < 4
        with torch.no_grad():
            q = enc(torch.from_numpy(wids)).numpy()
        c = "c%d/" % ci
        out[c + "wids"] = wids
        out[c + "q"] = q
        out[c + "E"] = enc.embedding.weight.detach().numpy()
        for k in ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0"):
            out[c + k] = getattr(enc.gru, k).detach().numpy()
    path = os.path.join(ROOT, "tests", "golden", "g15_gru.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
