"""Generate tests/golden/g10_semantic.npz by RUNNING THE REFERENCE's SemanticBaseline (vqa/models/cx.py:159-210) itself.

Uses oracle/make_golden.py's shims (imported, not changed: stub modules for the absent third-party imports, `.cuda()` as
the identity) plus `torch.cuda.FloatTensor` mapped to a CPU fp32 tensor (cx.py:208 builds its result there).  The
scorer's `vqa_forward` is fed stored logits: the reference-produced `a_knns` of the g1 / g2 fixtures (scaled, so that
the answer distributions are not all near uniform), with a few entries planted for the edge cases below.

Cases (each: a_knns [B, K, A], answer ids, an fp32 answer embedding [A, da], scores for several lambdas):
  c0  g1_small_L1 logits x 20 (A = 20): lambda in {0, 0.25, 0.5, 1}; embedding row 3 zero and some aid = 3; rows 5 and 7
      equal and some aid = 5; candidate (0, 0) with p[aid] near 1, candidate (0, 1) with p[aid] below 1e-8
  c1  g1_small_H20_L2 logits x 30 (A = 37, K = 24): lambda 0.7
  c2  g2_full_B4_H256_L1 logits x 40, first two questions (A = 2000, the real width): lambda 0.5, embedding da = 24

The fixture is data: inputs and the reference's outputs.  This script needs the reference checkout (build container only).
Usage:  python tests/tools/make_golden_semantic.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import oracle.make_golden  # noqa: E402,F401  (the shims; puts the reference first on sys.path)
import torch  # noqa: E402

torch.cuda.FloatTensor = lambda a: torch.tensor(np.asarray(a), dtype=torch.float32)

import vqa.models as ref_models  # noqa: E402  (the reference package)
from vqa.models.cx import SemanticBaseline  # noqa: E402

assert ref_models.__file__.startswith(oracle.make_golden.REF), ref_models.__file__


class _StubVQA(torch.nn.Module):
    """What SemanticBaseline's constructor reads of the VQA model (cx.py:165-166)."""
    opt = {"fusion": {"dim_mm": 16}}


def run_reference(a_knns, aids, emb, lam):
    m = SemanticBaseline(_StubVQA(), knn_size=a_knns.shape[1], trainable_vqa=False)
    m.set_lambda(lam)
    m.set_answer_embedding(emb)
    B, K, A = a_knns.shape
    m.vqa_forward = lambda image_features, question_wids: (torch.zeros(B, A), None, torch.from_numpy(a_knns), None, None)
    out = m(torch.zeros(B, K + 1, 1), None, torch.from_numpy(aids))
    assert out.requires_grad and out.dtype == torch.float32
    s = out.detach().numpy()
    assert np.isfinite(s).all()
    return s


def main():
    rng = np.random.default_rng(10)
    cases = {}

    g = np.load(os.path.join(GOLDEN, "g1_small_L1.npz"))
    a = g["a_knns"].astype(np.float32) * 20
    aids = g["answer_aids"].astype(np.int64).copy()
    A = a.shape[2]
    aids[1], aids[2] = 3, 5                                   # a zero row, a duplicated row
    emb = rng.standard_normal((A, 12)).astype(np.float32)
    emb[3] = 0
    emb[7] = emb[5]
    a[0, 0, :] = rng.standard_normal(A).astype(np.float32)
    a[0, 0, aids[0]] = 30.0                                   # p[aid] ~ 1 - 1e-12
    a[0, 1, aids[0]] = -30.0                                  # p[aid] ~ 5e-15 < 1e-8
    cases["c0"] = (a, aids, emb, [0.0, 0.25, 0.5, 1.0])

    g = np.load(os.path.join(GOLDEN, "g1_small_H20_L2.npz"))
    a = g["a_knns"].astype(np.float32) * 30
    emb = rng.standard_normal((a.shape[2], 30)).astype(np.float32)
    cases["c1"] = (a, g["answer_aids"].astype(np.int64), emb, [0.7])

    g = np.load(os.path.join(GOLDEN, "g2_full_B4_H256_L1.npz"))
    a = g["a_knns"][:2].astype(np.float32) * 40
    emb = rng.standard_normal((a.shape[2], 24)).astype(np.float32)
    cases["c2"] = (a, g["answer_aids"][:2].astype(np.int64), emb, [0.5])

    out = {}
    for name, (a, aids, emb, lams) in cases.items():
        out[name + "/a_knns"], out[name + "/aids"], out[name + "/emb"] = a, aids.astype(np.int32), emb
        out[name + "/lams"] = np.asarray(lams, np.float64)
        out[name + "/scores"] = np.stack([run_reference(a, aids, emb, lam) for lam in lams])
        print(name, a.shape, "lams", lams)
    path = os.path.join(GOLDEN, "g10_semantic.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
