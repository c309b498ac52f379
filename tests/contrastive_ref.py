"""fp64 restatement of the contrastive path (reference vqa/models/cx.py:428-487, contrastive.py:217-219, 293-309), for the
tests: forward, distances, both losses and every gradient, and the farthest-first rank of the counterexample."""
import numpy as np

H, MARGIN, EPS = 300, 2.0, 1e-6


def pre(feats, z_orig, z_knns, params):
    """Pre-activations [B, P, 300] of linear(cat(v_i, z_i)); feats [B, P, dv], z_orig [B, dz], z_knns [B, P - 1, dz]."""
    W, b = np.asarray(params["linear.weight"], np.float64), np.asarray(params["linear.bias"], np.float64)
    z = np.concatenate([np.asarray(z_orig, np.float64)[:, None], np.asarray(z_knns, np.float64)], 1)
    x = np.concatenate([np.asarray(feats, np.float64), z], 2)                 # columns v | z (cx.py:471)
    return x @ W.T + b, x


def forward(feats, z_orig, z_knns, params):
    p, _ = pre(feats, z_orig, z_knns, params)
    return np.maximum(p, 0.0)


def distances(h):
    """[B, P - 1]: ||h_0 - h_k + eps|| (F.pairwise_distance, eps inside the norm; cx.py:478-487)."""
    return np.sqrt(((h[:, :1] - h[:, 1:] + EPS) ** 2).sum(2))


def rank_farthest(dist, comp):
    """Rank of the counterexample when the neighbours are ordered by DESCENDING distance (ties by index): recallAtK's topk."""
    dist, comp = np.asarray(dist), np.asarray(comp)
    g = dist[np.arange(len(comp)), comp][:, None]
    k = np.arange(dist.shape[1])[None, :]
    return ((dist > g) | ((dist == g) & (k < comp[:, None]))).sum(1)


def loss_and_grads(feats, z_orig, z_knns, params, margin=MARGIN):
    """P = 3.  -> dict(h, loss_comp, loss_other, dist [B, 2], grads {linear.weight, linear.bias})."""
    p, x = pre(feats, z_orig, z_knns, params)
    h = np.maximum(p, 0.0)
    B = h.shape[0]
    e1, e2 = h[:, 0] - h[:, 1] + EPS, h[:, 0] - h[:, 2] + EPS
    d1, d2 = np.sqrt((e1 ** 2).sum(1)), np.sqrt((e2 ** 2).sum(1))
    hinge = np.maximum(margin - d1, 0.0)
    loss_comp, loss_other = (hinge ** 2).mean(), (d2 ** 2).mean()
    g1 = (-2.0 * hinge / d1 / B)[:, None] * e1                              # d loss_comp / d h0
    g2 = (2.0 / B) * e2                                                     # d loss_other / d h0
    dh = np.stack([g1 + g2, -g1, -g2], 1)
    dpre = dh * (p > 0)
    return dict(h=h, loss_comp=loss_comp, loss_other=loss_other, dist=np.stack([d1, d2], 1), dpre=dpre,
                grads={"linear.weight": np.einsum("bph,bpc->hc", dpre, x), "linear.bias": dpre.sum((0, 1))})
