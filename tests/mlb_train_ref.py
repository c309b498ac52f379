"""fp64 restatement of one MLBNoAtt training step below the question encoder (test infrastructure): the forward with explicit
dropout keep masks and every combination of the three activations, mean cross-entropy, every gradient and the top-k ranks.
Parameters use the layout of neuralcx.ops.MLB_FIELDS.  Adam and rank_safe are the Mutan restatement's (vqa_train_ref)."""
import numpy as np

from vqa_train_ref import adam, rank_safe  # noqa: F401  (re-exported: model-independent)

FIELDS = ("wv", "bv", "wq", "bq", "wc", "bc")
STATE_KEYS = dict(wv="fusion.linear_v.weight", bv="fusion.linear_v.bias", wq="fusion.linear_q.weight", bq="fusion.linear_q.bias",
                  wc="linear_classif.weight", bc="linear_classif.bias")


def shapes(dv, dq, dh, A):
    return dict(wv=(dh, dv), bv=(dh,), wq=(dh, dq), bq=(dh,), wc=(A, dh), bc=(A,))


def init_params(seed, dv, dq, dh, A, gain=1.0):
    """nn.Linear-style uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)) x gain, fp32."""
    rng = np.random.default_rng(seed)
    out = {}
    sh = shapes(dv, dq, dh, A)
    for w, b in (("wv", "bv"), ("wq", "bq"), ("wc", "bc")):
        k = gain / np.sqrt(sh[w][1])
        out[w] = rng.uniform(-k, k, sh[w]).astype(np.float32)
        out[b] = rng.uniform(-k, k, sh[b]).astype(np.float32)
    return out


def state_to_fields(sd):
    """reference state_dict (fusion.linear_v.*, fusion.linear_q.*, linear_classif.*) -> fields"""
    return {f: np.asarray(sd[k]) for f, k in STATE_KEYS.items()}


def _act(x, a):
    return np.tanh(x) if a else x


def step(P, v, q, target, act_v=True, act_q=True, act_c=True, masks=None, p=(0.0, 0.0, 0.0), scale=None):
    """v [B, dv] (the gathered feature rows), q [B, dq], target [B].  masks: (mv, mq, mc) 0/1 arrays or None.
    -> dict(logits, z (before act_c), loss, grads{field}, dq, rank [B], dlogits)"""
    P = {k: np.asarray(x, np.float64) for k, x in P.items()}
    v, q = np.asarray(v, np.float64), np.asarray(q, np.float64)
    B = v.shape[0]
    A, dh = P["wc"].shape
    if masks is None:
        masks, p = (np.ones_like(v), np.ones_like(q), np.ones((B, dh))), (0.0, 0.0, 0.0)
    mv, mq, mc = (np.asarray(m, np.float64) / (1.0 - pp) for m, pp in zip(masks, p))
    vd, qd = v * mv, q * mq
    xv = _act(vd @ P["wv"].T + P["bv"], act_v)
    xq = _act(qd @ P["wq"].T + P["bq"], act_q)
    z = xq * xv
    t = _act(z, act_c)
    tc = t * mc
    logits = tc @ P["wc"].T + P["bc"]
    mx = logits.max(1, keepdims=True)
    lse = np.log(np.exp(logits - mx).sum(1)) + mx[:, 0]
    tg = np.asarray(target).astype(np.int64)
    scale = 1.0 / B if scale is None else scale
    xt = logits[np.arange(B), tg]
    loss = float(((lse - xt) * scale).sum())
    rank = (logits > xt[:, None]).sum(1) + ((logits == xt[:, None]) & (np.arange(A)[None, :] < tg[:, None])).sum(1)
    dl = np.exp(logits - lse[:, None])
    dl[np.arange(B), tg] -= 1.0
    dl *= scale
    G = {}
    G["wc"] = dl.T @ tc; G["bc"] = dl.sum(0)
    dt = (dl @ P["wc"]) * mc
    dz = dt * (1.0 - t * t) if act_c else dt
    dpv, dpq = dz * xq, dz * xv
    if act_v:
        dpv = dpv * (1.0 - xv * xv)
    if act_q:
        dpq = dpq * (1.0 - xq * xq)
    G["wv"] = dpv.T @ vd; G["bv"] = dpv.sum(0)
    G["wq"] = dpq.T @ qd; G["bq"] = dpq.sum(0)
    dq = (dpq @ P["wq"]) * mq
    return dict(logits=logits, z=z, loss=loss, grads=G, dq=dq, rank=rank, dlogits=dl)
