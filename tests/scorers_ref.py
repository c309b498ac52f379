"""fp64 restatement of LinearContext (reference vqa/models/cx.py:139-156) and PairwiseLinearModel (cx.py:379-425): forward, the
listwise loss CrossEntropyLoss(size_average=False) / B (counterexamples.py:310,334) and every gradient, written out by hand.
tests/test_scorers_cpu.py pins it to the reference-produced fixture tests/golden/g11_scorers.npz; the GPU tests compare the HIP
kernels with it at full widths.  Pure numpy (no GPU)."""
import numpy as np

H = 300


def _softmax(s):
    e = np.exp(s - s.max(1, keepdims=True))
    return e / e.sum(1, keepdims=True)


def loss_and_dscores(scores, gt):
    B = scores.shape[0]
    p = _softmax(scores)
    loss = -np.log(p[np.arange(B), gt]).sum() / B
    d = p.copy()
    d[np.arange(B), gt] -= 1.0
    return loss, d / B


def linctx(z_knns, p, gt):
    """-> scores, loss, grads {linear.weight, linear.bias}."""
    B = z_knns.shape[0]
    z = z_knns.reshape(B, -1).astype(np.float64)
    W, b = p["linear.weight"].astype(np.float64), p["linear.bias"].astype(np.float64)
    s = z @ W.T + b
    loss, ds = loss_and_dscores(s, gt)
    return s, loss, {"linear.weight": ds.T @ z, "linear.bias": ds.sum(0)}


def pairlin_pre(feats, q, z_o, z_k, aids, p):
    """feats [B, K+1, dv] (column 0 the original image) -> hidden pre-activations [B, K, H], score pre-activations [B, K]."""
    f = lambda a: np.asarray(a, np.float64)
    feats, q, z_o, z_k = f(feats), f(q), f(z_o), f(z_k)
    B, K1, dv = feats.shape
    K = K1 - 1
    W, b = f(p["linear.weight"]), f(p["linear.bias"])
    E = f(p["answer_embedding.weight"])
    a = E[np.asarray(aids)]
    dq, dz = q.shape[1], z_o.shape[1]
    Wv_o, Wv_k = W[:, :dv], W[:, dv:2 * dv]
    Wq = W[:, 2 * dv:2 * dv + dq]
    Wz_o, Wz_k = W[:, 2 * dv + dq:2 * dv + dq + dz], W[:, 2 * dv + dq + dz:2 * dv + dq + 2 * dz]
    Wa = W[:, 2 * dv + dq + 2 * dz:]
    P = feats[:, 0] @ Wv_o.T + q @ Wq.T + z_o @ Wz_o.T + a @ Wa.T + b           # [B, H]
    pre_h = feats[:, 1:] @ Wv_k.T + z_k @ Wz_k.T + P[:, None, :]
    h = np.maximum(pre_h, 0.0)
    pre_s = h @ f(p["out.weight"])[0] + f(p["out.bias"])[0]
    return pre_h, pre_s


def pairlin(feats, q, z_o, z_k, aids, p, gt):
    """-> scores, loss, grads (state_dict names), pre_h, pre_s."""
    f = lambda a: np.asarray(a, np.float64)
    pre_h, pre_s = pairlin_pre(feats, q, z_o, z_k, aids, p)
    s = np.maximum(pre_s, 0.0)
    loss, ds = loss_and_dscores(s, gt)
    feats, q, z_o, z_k = f(feats), f(q), f(z_o), f(z_k)
    B, K1, dv = feats.shape
    dq, dz = q.shape[1], z_o.shape[1]
    W, w_out = f(p["linear.weight"]), f(p["out.weight"])[0]
    E = f(p["answer_embedding.weight"])
    h = np.maximum(pre_h, 0.0)
    g = ds * (pre_s > 0)                                      # [B, K]
    dpre = g[:, :, None] * w_out[None, None, :] * (pre_h > 0)  # [B, K, H]
    dP = dpre.sum(1)
    a = E[np.asarray(aids)]
    gW = np.zeros_like(W)
    gW[:, :dv] = dP.T @ feats[:, 0]
    K = K1 - 1
    dpre2 = dpre.reshape(B * K, -1)
    gW[:, dv:2 * dv] = dpre2.T @ feats[:, 1:].reshape(B * K, dv)
    gW[:, 2 * dv:2 * dv + dq] = dP.T @ q
    gW[:, 2 * dv + dq:2 * dv + dq + dz] = dP.T @ z_o
    gW[:, 2 * dv + dq + dz:2 * dv + dq + 2 * dz] = dpre2.T @ z_k.reshape(B * K, dz)
    gW[:, 2 * dv + dq + 2 * dz:] = dP.T @ a
    dA = dP @ W[:, 2 * dv + dq + 2 * dz:]
    gE = np.zeros_like(E)
    np.add.at(gE, np.asarray(aids), dA)
    grads = {"answer_embedding.weight": gE, "linear.weight": gW, "linear.bias": dP.sum(0),
             "out.weight": (g.reshape(-1) @ h.reshape(B * K, -1))[None, :], "out.bias": np.array([g.sum()])}
    return s, loss, grads, pre_h, pre_s


def adam(params, grads_seq, lr, betas=(0.9, 0.999), eps=1e-8):
    """torch.optim.Adam (no weight decay) over a sequence of gradient dicts, fp64."""
    m = {k: np.zeros_like(v, np.float64) for k, v in params.items()}
    v2 = {k: np.zeros_like(v, np.float64) for k, v in params.items()}
    p = {k: np.asarray(v, np.float64).copy() for k, v in params.items()}
    for t, g in enumerate(grads_seq, 1):
        for k in p:
            m[k] = betas[0] * m[k] + (1 - betas[0]) * g[k]
            v2[k] = betas[1] * v2[k] + (1 - betas[1]) * g[k] ** 2
            denom = np.sqrt(v2[k]) / np.sqrt(1 - betas[1] ** t) + eps
            p[k] = p[k] - lr / (1 - betas[0] ** t) * m[k] / denom
    return p
