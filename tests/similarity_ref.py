"""fp64 numpy restatement of the reference's SimilarityModel (vqa/models/cx.py:490-518); test infrastructure.

    scores[b, k] = cos(v_orig[b], v_knn[b, k]) + cos(z_orig[b], z_knn[b, k]) + CE(a_knns[b, k, :], aid[b])      (cx.py:511-516)

cos is F.cosine_similarity's rule on the installed torch: x . y / (max(|x|, eps) max(|y|, eps)), eps = 1e-8, each norm
clamped on its own (tests/golden/g13_similarity.npz pins it: candidate (0, 5) of case c0 has a norm below eps against an
original of norm ~100).  CE is F.cross_entropy without reduction: logsumexp(a) - a[aid], the max subtracted first."""
import numpy as np

EPS = 1e-8


def cosine(x, y):
    """Row-wise cosine of two [..., d] arrays in fp64."""
    x, y = np.asarray(x, np.float64), np.asarray(y, np.float64)
    nx = np.maximum(np.sqrt((x * x).sum(-1)), EPS)
    ny = np.maximum(np.sqrt((y * y).sum(-1)), EPS)
    return (x * y).sum(-1) / (nx * ny)


def xent(a_knns, aids):
    """[B, K, A] logits, [B] ids -> [B, K] cross-entropy of every candidate's logits against the question's answer id."""
    a = np.asarray(a_knns, np.float64)
    m = a.max(-1, keepdims=True)
    lse = m[..., 0] + np.log(np.exp(a - m).sum(-1))
    B = a.shape[0]
    return lse - a[np.arange(B), :, np.asarray(aids, np.int64)]


def similarity_parts(v, z_orig, z_knns, a_knns, aids):
    """v [B, K + 1, dv] (row 0 the original image) -> parts [B, K, 3] = v_cos | z_cos | xent."""
    v = np.asarray(v, np.float64)
    return np.stack([cosine(v[:, :1], v[:, 1:]), cosine(np.asarray(z_orig)[:, None], z_knns), xent(a_knns, aids)], -1)


def similarity_scores(v, z_orig, z_knns, a_knns, aids):
    """-> (scores [B, K], parts [B, K, 3])."""
    p = similarity_parts(v, z_orig, z_knns, a_knns, aids)
    return p.sum(-1), p


def similarity_scores_table(feats, img_idx, z_orig, z_knns, a_knns, aids):
    """The same with the rows gathered from a feature table: feats [n_img, dv], img_idx [B, K + 1]."""
    return similarity_scores(np.asarray(feats)[np.asarray(img_idx, np.int64)], z_orig, z_knns, a_knns, aids)
