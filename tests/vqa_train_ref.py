"""fp64 restatement of one MutanNoAtt training step below the question encoder (test infrastructure): the forward with explicit
dropout keep masks, mean cross-entropy, every gradient, the top-k ranks and Adam.  Parameters use the stacked layout of
neuralcx.ops.MUTAN_FIELDS (whv / whq: the R projections stacked along the output rows)."""
import numpy as np

FIELDS = ("wv", "bv", "wq", "bq", "whv", "bhv", "whq", "bhq", "wc", "bc")


def shapes(dv, dq, dhv, dhq, dz, R, A):
    return dict(wv=(dhv, dv), bv=(dhv,), wq=(dhq, dq), bq=(dhq,), whv=(R * dz, dhv), bhv=(R * dz,), whq=(R * dz, dhq), bhq=(R * dz,),
                wc=(A, dz), bc=(A,))


def init_params(seed, dv, dq, dhv, dhq, dz, R, A, gain=1.0):
    """nn.Linear-style uniform(-1/sqrt(fan_in), 1/sqrt(fan_in)) x gain, fp32."""
    rng = np.random.default_rng(seed)
    out = {}
    sh = shapes(dv, dq, dhv, dhq, dz, R, A)
    for w, b in (("wv", "bv"), ("wq", "bq"), ("whv", "bhv"), ("whq", "bhq"), ("wc", "bc")):
        k = gain / np.sqrt(sh[w][1])
        out[w] = rng.uniform(-k, k, sh[w]).astype(np.float32)
        out[b] = rng.uniform(-k, k, sh[b]).astype(np.float32)
    return out


def state_to_fields(sd, R):
    """reference state_dict (fusion.linear_v.*, fusion.list_linear_hv.{i}.*, linear_classif.*) -> stacked fields"""
    g = lambda k: np.asarray(sd[k])
    return dict(wv=g("fusion.linear_v.weight"), bv=g("fusion.linear_v.bias"), wq=g("fusion.linear_q.weight"), bq=g("fusion.linear_q.bias"),
                whv=np.concatenate([g("fusion.list_linear_hv.%d.weight" % i) for i in range(R)]),
                bhv=np.concatenate([g("fusion.list_linear_hv.%d.bias" % i) for i in range(R)]),
                whq=np.concatenate([g("fusion.list_linear_hq.%d.weight" % i) for i in range(R)]),
                bhq=np.concatenate([g("fusion.list_linear_hq.%d.bias" % i) for i in range(R)]),
                wc=g("linear_classif.weight"), bc=g("linear_classif.bias"))


def _act(x, a):
    return np.tanh(x) if a else x


def step(P, v, q, target, act_v=True, act_q=True, masks=None, p=(0.0, 0.0, 0.0), scale=None):
    """v [B, dv] (the gathered feature rows), q [B, dq], target [B].  masks: (mv, mq, mz) 0/1 arrays or None.
    -> dict(logits, z, loss, grads{field}, dq, rank [B])"""
    P = {k: np.asarray(x, np.float64) for k, x in P.items()}
    v, q = np.asarray(v, np.float64), np.asarray(q, np.float64)
    B = v.shape[0]
    A, dz = P["wc"].shape
    R = P["whv"].shape[0] // dz
    if masks is None:
        masks, p = (np.ones_like(v), np.ones_like(q), np.ones((B, dz))), (0.0, 0.0, 0.0)
    mv, mq, mz = (np.asarray(m, np.float64) / (1.0 - pp) for m, pp in zip(masks, p))
    vd, qd = v * mv, q * mq
    xv = _act(vd @ P["wv"].T + P["bv"], act_v)
    xq = _act(qd @ P["wq"].T + P["bq"], act_q)
    hv = xv @ P["whv"].T + P["bhv"]
    hq = xq @ P["whq"].T + P["bhq"]
    z = (hv * hq).reshape(B, R, dz).sum(1)
    zc = z * mz
    logits = zc @ P["wc"].T + P["bc"]
    mx = logits.max(1, keepdims=True)
    lse = np.log(np.exp(logits - mx).sum(1)) + mx[:, 0]
    t = np.asarray(target).astype(np.int64)
    scale = 1.0 / B if scale is None else scale
    xt = logits[np.arange(B), t]
    loss = float(((lse - xt) * scale).sum())
    rank = (logits > xt[:, None]).sum(1) + ((logits == xt[:, None]) & (np.arange(A)[None, :] < t[:, None])).sum(1)
    dl = np.exp(logits - lse[:, None])
    dl[np.arange(B), t] -= 1.0
    dl *= scale
    G = {}
    G["wc"] = dl.T @ zc; G["bc"] = dl.sum(0)
    dzz = (dl @ P["wc"]) * mz
    dzr = np.tile(dzz, (1, R))
    dhv, dhq = dzr * hq, dzr * hv
    G["whv"] = dhv.T @ xv; G["bhv"] = dhv.sum(0)
    G["whq"] = dhq.T @ xq; G["bhq"] = dhq.sum(0)
    dxv, dxq = dhv @ P["whv"], dhq @ P["whq"]
    if act_v:
        dxv = dxv * (1.0 - xv * xv)
    if act_q:
        dxq = dxq * (1.0 - xq * xq)
    G["wv"] = dxv.T @ vd; G["bv"] = dxv.sum(0)
    G["wq"] = dxq.T @ qd; G["bq"] = dxq.sum(0)
    dq = (dxq @ P["wq"]) * mq
    return dict(logits=logits, z=z, loss=loss, grads=G, dq=dq, rank=rank, dlogits=dl)


def rank_safe(logits, target, gap=2e-4):
    """rows whose target logit is further than `gap` from every other logit: their rank does not depend on rounding"""
    B = logits.shape[0]
    t = np.asarray(target).astype(np.int64)
    d = np.abs(logits - logits[np.arange(B), t][:, None])
    d[np.arange(B), t] = np.inf
    return d.min(1) > gap


def adam(P, G, m, v, step_no, lr=1e-4, b1=0.9, b2=0.999, eps=1e-8):
    """torch.optim.Adam (no weight decay, no amsgrad) in fp64, in place on the dicts; step_no is 1-based."""
    for k in P:
        g = np.asarray(G[k], np.float64)
        m[k] = b1 * m[k] + (1 - b1) * g
        v[k] = b2 * v[k] + (1 - b2) * g * g
        P[k] = P[k] - (lr / (1 - b1 ** step_no)) * m[k] / (np.sqrt(v[k]) / np.sqrt(1 - b2 ** step_no) + eps)
    return P
