"""fp64 numpy restatement of the reference's SemanticBaseline (vqa/models/cx.py:159-210), line by line; test infrastructure.

Differences from the reference, all below the tests' tolerances: fp64 throughout except `p[aid] + 1e-8` and its log,
which stay fp32 as in the reference (cx.py:201-202: a float32 numpy scalar plus a Python float is float32), so that the
floor log(1e-8) behaves identically; both softmaxes subtract the max (equal wherever the reference is finite)."""
import numpy as np


def cosine_similarity(emb):
    """sklearn.metrics.pairwise.cosine_similarity(emb) in fp64: rows divided by their L2 norm, a zero row left zero."""
    x = np.asarray(emb, np.float64)
    n = np.sqrt((x * x).sum(1))
    n[n == 0] = 1.0
    xn = x / n[:, None]
    return xn @ xn.T


def softmax(w):                                              # cx.py:177-180
    w = np.asarray(w, np.float64)
    e = np.exp(w - w.max())
    return e / e.sum()


def semantic_raw(a_knns, aids, emb_pairs, lam):
    """-> s [B, K] before the softmax over candidates (cx.py:188-205)."""
    a_knns = np.asarray(a_knns)
    B, K, _ = a_knns.shape
    s = np.empty((B, K), np.float64)
    for b in range(B):
        aid = int(aids[b])
        for k in range(K):
            nb = softmax(a_knns[b, k])                       # cx.py:193
            weighted_sim = emb_pairs[aid, :].dot(nb)          # cx.py:194
            weighted_sim -= nb[aid]                           # cx.py:197
            p = np.float32(nb[aid]) + np.float32(1e-8)        # cx.py:201 (fp32)
            logp = np.float64(np.log(p))                      # cx.py:202 (fp32 log)
            s[b, k] = (lam * weighted_sim) - ((1 - lam) * logp)   # cx.py:204
    return s


def semantic_scores(a_knns, aids, emb_pairs, lam):
    """-> (scores [B, K] = softmax_k(s), s)   (cx.py:206-209)."""
    s = semantic_raw(a_knns, aids, emb_pairs, lam)
    return np.stack([softmax(r) for r in s]), s
