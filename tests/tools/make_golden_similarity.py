"""Generate tests/golden/g13_similarity.npz by RUNNING THE REFERENCE's SimilarityModel (vqa/models/cx.py:490-518) itself.

Uses oracle/make_golden.py's shims (imported, not changed: stub modules for the absent third-party imports, `.cuda()` as
the identity).  The scorer's `vqa_forward` is replaced by a lambda that returns stored arrays (z and logits of the g1 / g2
fixtures, which the reference's VQA model produced).  The reference returns the sum only; its three terms are recorded as it
computes them, by wrapping F.cosine_similarity and F.cross_entropy for the duration of its forward (the calls come in the
order v, z, a per candidate, cx.py:511-514).

Cases (each: v [B, K + 1, dv], z_orig, z_knns, a_knns, answer ids; the reference's scores [B, K] and parts [B, K, 3]):
  c0  g1_small_L1 (dv = 64, dz = 16, A = 20), logits x 20, with planted rows:
        candidate (1, 3): an all-zero v row                  question 2: an all-zero z_orig
        candidate (3, 2): v and z identical to the original (both cosines 1)
        candidate (0, 0): a[aid] 30 above the rest           candidate (0, 1): a[aid] 30 below the rest
        candidate (0, 5): |v| = 1e-10 < eps along v_orig, and |v_orig| ~ 100 -- this pins the clamp rule: every norm clamped
                          on its own gives cos = |v| / eps = 0.01, the older max(|x| |y|, eps) would give 1
  c1  g1_small_H20_L2 cut to odd widths: dv = 37, dz = 5, A = 37; logits x 30
  c2  g2_full_B4_H256_L1, first two questions, the real widths: dv = 2048, dz = 360, A = 2000, K = 24; logits x 40

The fixture is data: inputs and the reference's outputs.  This script needs the reference checkout (build container only).
Usage:  python tests/tools/make_golden_similarity.py
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import oracle.make_golden  # noqa: E402,F401  (the shims; puts the reference first on sys.path)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

import vqa.models as ref_models  # noqa: E402  (the reference package)
from vqa.models.cx import SimilarityModel  # noqa: E402

assert ref_models.__file__.startswith(oracle.make_golden.REF), ref_models.__file__


class _StubVQA(torch.nn.Module):
    """What SimilarityModel's constructor reads of the VQA model (cx.py:494)."""
    opt = {"fusion": {"dim_mm": 16}}


def run_reference(v, z_orig, z_knns, a_knns, aids):
    B, K = a_knns.shape[:2]
    m = SimilarityModel(_StubVQA(), knn_size=K, trainable_vqa=False)
    t = torch.from_numpy
    m.vqa_forward = lambda image_features, question_wids: (torch.zeros(B, a_knns.shape[2]), t(z_orig), t(a_knns), t(z_knns), None)
    calls = []
    cos, ce = F.cosine_similarity, F.cross_entropy

    def rec(fn):
        def wrapped(*a, **k):
            out = fn(*a, **k)
            calls.append(out.detach().numpy().copy())
            return out
        return wrapped

    F.cosine_similarity, F.cross_entropy = rec(cos), rec(ce)
    try:
        out = m(t(v), None, t(aids))
    finally:
        F.cosine_similarity, F.cross_entropy = cos, ce
    assert out.dtype == torch.float32 and tuple(out.shape) == (B, K) and not out.requires_grad
    assert len(calls) == 3 * K
    parts = np.stack([np.stack(calls[3 * i:3 * i + 3], -1) for i in range(K)], 1)          # [B, K, 3]
    s = out.numpy()
    assert np.isfinite(s).all() and np.abs(parts.sum(-1) - s).max() < 1e-4
    return s, parts.astype(np.float32)


def main():
    rng = np.random.default_rng(13)
    cases = {}

    g = np.load(os.path.join(GOLDEN, "g1_small_L1.npz"))
    v, zo, zk = g["image_features"].astype(np.float32).copy(), g["z_orig"].astype(np.float32).copy(), g["z_knns"].astype(np.float32).copy()
    a, aids = g["a_knns"].astype(np.float32) * 20, g["answer_aids"].astype(np.int64).copy()
    v[1, 1 + 3] = 0
    zo[2] = 0
    v[3, 1 + 2], zk[3, 2] = v[3, 0], zo[3]
    a[0, 0] = rng.standard_normal(a.shape[2]).astype(np.float32)
    a[0, 0, aids[0]] = a[0, 0].max() + 30.0
    a[0, 1] = rng.standard_normal(a.shape[2]).astype(np.float32)
    a[0, 1, aids[0]] = a[0, 1].min() - 30.0
    v[0, 0] *= np.float32(100.0 / np.linalg.norm(v[0, 0]))
    v[0, 1 + 5] = v[0, 0] * np.float32(1e-12)
    cases["c0"] = (v, zo, zk, a, aids)

    g = np.load(os.path.join(GOLDEN, "g1_small_H20_L2.npz"))
    cases["c1"] = (np.ascontiguousarray(g["image_features"][:, :, :37], np.float32), np.ascontiguousarray(g["z_orig"][:, :5], np.float32),
                   np.ascontiguousarray(g["z_knns"][:, :, :5], np.float32), g["a_knns"].astype(np.float32) * 30, g["answer_aids"].astype(np.int64))

    g = np.load(os.path.join(GOLDEN, "g2_full_B4_H256_L1.npz"))
    cases["c2"] = (g["image_features"][:2].astype(np.float32), g["z_orig"][:2].astype(np.float32), g["z_knns"][:2].astype(np.float32),
                   g["a_knns"][:2].astype(np.float32) * 40, g["answer_aids"][:2].astype(np.int64))

    out = {}
    for name, (v, zo, zk, a, aids) in cases.items():
        s, parts = run_reference(v, zo, zk, a, aids)
        out[name + "/v"], out[name + "/z_orig"], out[name + "/z_knns"], out[name + "/a_knns"] = v, zo, zk, a
        out[name + "/aids"], out[name + "/scores"], out[name + "/parts"] = aids.astype(np.int32), s, parts
        print(name, "v", v.shape, "z", zk.shape, "a", a.shape, "scores", float(s.min()), "..", float(s.max()))
    path = os.path.join(GOLDEN, "g13_similarity.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
