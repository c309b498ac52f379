"""fp64 restatement of one training step of MLBAtt below the question encoder (reference vqa/models/att.py:39-163 in training mode,
mean cross-entropy): forward with explicit dropout masks, every parameter gradient and d loss / d q_emb.  numpy only; builds on
mlb_att_ref (the eval forward).  Spatial position p = w H + h.

Dropout layers, in the order the masks are concatenated for the library (generator layer id = position + 1; element index = linear
index in the tensor named):
  1 the map fed to conv_v_att [B, dv, P] (the pooled map is NOT dropped)   2 q fed to linear_q_att [B, dq]
  3 x_att after activation_mm [B, P, dh_att]                               4 v_att fed to the glimpse Linears [B, G, dv]
  5 q fed to linear_q_fusion [B, dq]                                       6 t = act_c(x_v * x_qf) [B, G dh_f]"""
import numpy as np

from mlb_att_ref import ACT_KEYS

LAYERS = ("att_v", "att_q", "att_mm", "v", "q", "c")


def mask_shapes(B, P, dv, dq, dh_att, G, dh_f):
    return ((B, dv, P), (B, dq), (B, P, dh_att), (B, G, dv), (B, dq), (B, G * dh_f))


def generator_masks(seed, p, B, P, dv, dq, dh_att, G, dh_f):
    """The six keep masks (0 / 1, fp32) the library's counter-based generator draws under `seed` for the p's `p` (layer order)."""
    from oracle.ncx_oracle import dropout_keep_mask
    out = []
    for layer, (shp, pr) in enumerate(zip(mask_shapes(B, P, dv, dq, dh_att, G, dh_f), p), start=1):
        n = int(np.prod(shp))
        if pr <= 0:
            out.append(np.ones(shp, np.float32))
            continue
        m = dropout_keep_mask(seed, layer, n, 1, float(pr))
        out.append(np.asarray(m, np.float32).reshape(shp))
    return out


def random_masks(rng, p, B, P, dv, dq, dh_att, G, dh_f):
    return [(rng.random(shp) >= pr).astype(np.float32) for shp, pr in zip(mask_shapes(B, P, dv, dq, dh_att, G, dh_f), p)]


def concat_masks(masks):
    return np.concatenate([np.asarray(m, np.float32).reshape(-1) for m in masks])


def _tanh_or_id(name):
    if name in (None, ""):
        return (lambda x: x), (lambda y: 1.0)
    assert name == "tanh", name
    return np.tanh, (lambda y: 1.0 - y * y)


def step(state, maps, q_emb, target, acts=None, masks=None, p=(0.0,) * 6):
    """state, maps [B, dv, W, H] (or [B, dv, P]), q_emb as mlb_att_ref.mlb_att_forward; target [B] class ids; masks: six keep masks
    (None = no dropout) that are scaled by 1 / (1 - p[i]).
    -> dict(logits, att, pos, loss, grads {state_dict key: array of that key's shape}, dq_emb, Xv, v_att, t), all fp64."""
    a = {k: "tanh" for k in ACT_KEYS}
    a.update(acts or {})
    f64 = lambda k: np.asarray(state[k], np.float64)
    V = np.asarray(maps, np.float64)
    V = V.reshape(V.shape[0], V.shape[1], -1)                                   # [B, dv, P]
    B, dv, P = V.shape
    q = np.asarray(q_emb, np.float64)
    wv = f64("conv_v_att.weight").reshape(len(state["conv_v_att.bias"]), -1)    # [dh, dv]
    wa = f64("conv_att.weight").reshape(len(state["conv_att.bias"]), -1)        # [G, dh]
    G, dh = wa.shape
    wq, wqf, wc = f64("linear_q_att.weight"), f64("linear_q_fusion.weight"), f64("linear_classif.weight")
    wg = np.stack([f64("list_linear_v_fusion.%d.weight" % g) for g in range(G)])      # [G, dh_f, dv]
    bg = np.stack([f64("list_linear_v_fusion.%d.bias" % g) for g in range(G)])
    dh_f = wg.shape[1]
    if masks is None:
        m = [1.0] * 6
    else:
        m = [np.asarray(mk, np.float64).reshape(shp) / (1.0 - pr) for mk, shp, pr in zip(masks, mask_shapes(B, P, dv, q.shape[1], dh, G, dh_f), p)]
    act_va, d_va = _tanh_or_id(a["att_v"]); act_qa, d_qa = _tanh_or_id(a["att_q"]); act_mm, d_mm = _tanh_or_id(a["att_mm"])
    act_v, d_v = _tanh_or_id(a["v"]); act_q, d_q = _tanh_or_id(a["q"]); act_c, d_c = _tanh_or_id(a["c"])

    # ---- forward
    Vd = V * m[0]
    Xv = act_va(np.matmul(Vd.transpose(0, 2, 1), wv.T) + f64("conv_v_att.bias"))      # [B, P, dh]
    q2 = q * m[1]
    xq = act_qa(q2 @ wq.T + f64("linear_q_att.bias"))                           # [B, dh]
    av = act_mm(Xv * xq[:, None, :])
    ad = av * m[2]
    pos = np.matmul(ad, wa.T).transpose(0, 2, 1) + f64("conv_att.bias")[None, :, None]
    e = np.exp(pos - pos.max(2, keepdims=True))
    att = e / e.sum(2, keepdims=True)
    v_att = np.matmul(att, V.transpose(0, 2, 1))                                  # the undropped map
    v4 = v_att * m[3]
    x_v = act_v(np.stack([v4[:, g] @ wg[g].T for g in range(G)], 1) + bg[None]).reshape(B, G * dh_f)
    q5 = q * m[4]
    x_qf = act_q(q5 @ wqf.T + f64("linear_q_fusion.bias"))
    t = act_c(x_v * x_qf)
    tc = t * m[5]
    logits = tc @ wc.T + f64("linear_classif.bias")
    z = logits - logits.max(1, keepdims=True)
    lse = np.log(np.exp(z).sum(1, keepdims=True))
    tgt = np.asarray(target, np.int64)
    loss = float(-(z - lse)[np.arange(B), tgt].mean())

    # ---- backward
    dlogits = np.exp(z - lse)
    dlogits[np.arange(B), tgt] -= 1.0
    dlogits /= B
    g = {}
    g["linear_classif.weight"], g["linear_classif.bias"] = dlogits.T @ tc, dlogits.sum(0)
    dt = (dlogits @ wc) * m[5]
    dz = dt * d_c(t)
    dpv = dz * x_qf * d_v(x_v)
    dpqf = dz * x_v * d_q(x_qf)
    dpv3 = dpv.reshape(B, G, dh_f)
    for gi in range(G):
        g["list_linear_v_fusion.%d.weight" % gi] = dpv3[:, gi].T @ v4[:, gi]
        g["list_linear_v_fusion.%d.bias" % gi] = dpv3[:, gi].sum(0)
    g["linear_q_fusion.weight"], g["linear_q_fusion.bias"] = dpqf.T @ q5, dpqf.sum(0)
    dv_att = np.stack([dpv3[:, g] @ wg[g] for g in range(G)], 1) * m[3]
    datt = np.matmul(dv_att, V)
    ds = att * (datt - (att * datt).sum(2, keepdims=True))
    g["conv_att.bias"] = ds.sum((0, 2))
    g["conv_att.weight"] = np.tensordot(ds, ad, axes=([0, 2], [0, 1])).reshape(np.shape(state["conv_att.weight"]))
    da = np.matmul(ds.transpose(0, 2, 1), wa) * m[2]
    du = da * d_mm(av)
    dxq = (du * Xv).sum(1)
    dXv = du * xq[:, None, :] * d_va(Xv)
    g["conv_v_att.weight"] = np.tensordot(dXv, Vd, axes=([0, 1], [0, 2])).reshape(np.shape(state["conv_v_att.weight"]))
    g["conv_v_att.bias"] = dXv.sum((0, 1))
    dpq = dxq * d_qa(xq)
    g["linear_q_att.weight"], g["linear_q_att.bias"] = dpq.T @ q2, dpq.sum(0)
    dq = (dpq @ wq) * m[1] + (dpqf @ wqf) * m[4]
    return dict(logits=logits, att=att, pos=pos, loss=loss, grads=g, dq_emb=dq, Xv=Xv, v_att=v_att, t=t)


# state_dict key -> (field of ops.MLB_ATT_FIELDS, glimpse index or None)
def field_of(key):
    simple = {"conv_v_att.weight": "wv_att", "conv_v_att.bias": "bv_att", "linear_q_att.weight": "wq_att", "linear_q_att.bias": "bq_att",
              "conv_att.weight": "wa", "conv_att.bias": "ba", "linear_q_fusion.weight": "wqf", "linear_q_fusion.bias": "bqf",
              "linear_classif.weight": "wc", "linear_classif.bias": "bc"}
    if key in simple:
        return simple[key], None
    assert key.startswith("list_linear_v_fusion."), key
    _, gi, kind = key.split(".")
    return ("wg" if kind == "weight" else "bg"), int(gi)


def grads_by_field(grads, G):
    """The restatement's gradients in the stacked layout of ops.MLB_ATT_FIELDS (twelve tensors)."""
    out = {}
    for k, v in grads.items():
        f, gi = field_of(k)
        if gi is None:
            out[f] = v.reshape(v.shape[0], -1) if f in ("wv_att", "wa") else v
    out["wg"] = np.stack([grads["list_linear_v_fusion.%d.weight" % g] for g in range(G)])
    out["bg"] = np.stack([grads["list_linear_v_fusion.%d.bias" % g] for g in range(G)])
    return out
