"""fp64 restatement of MLBAtt.forward below the question encoder (reference vqa/models/att.py:39-192; eval mode, every dropout the
identity).  numpy only.  Spatial position p = w H + h: the map's memory order."""
import numpy as np

_ACT = {None: lambda x: x, "": lambda x: x, "tanh": np.tanh}
ACT_KEYS = ("att_v", "att_q", "att_mm", "v", "q", "c")      # attention.activation_v/_q/_mm, fusion.activation_v/_q, classif.activation


def mlb_att_forward(state, maps, q_emb, acts=None, want_logits=False):
    """state: the model's state_dict as arrays (conv_v_att.*, linear_q_att.*, conv_att.*, list_linear_v_fusion.{g}.*, linear_q_fusion.*,
    linear_classif.*); maps [B, dv, W, H] (or [B, dv, P]); q_emb [B, dq]; acts: dict over ACT_KEYS (missing = tanh).
    -> (logits [B, A], att [B, G, P]) in fp64; with want_logits also the position logits [B, G, P] before the softmax."""
    a = {k: "tanh" for k in ACT_KEYS}
    a.update(acts or {})
    f64 = lambda k: np.asarray(state[k], np.float64)
    v = np.asarray(maps, np.float64)
    v = v.reshape(v.shape[0], v.shape[1], -1)                                                    # [B, dv, P]
    q = np.asarray(q_emb, np.float64)
    wv = f64("conv_v_att.weight").reshape(len(state["conv_v_att.bias"]), -1)                     # [dh, dv]
    wa = f64("conv_att.weight").reshape(len(state["conv_att.bias"]), -1)                         # [G, dh]
    G = wa.shape[0]
    vt = v.transpose(0, 2, 1)                                                                    # [B, P, dv]
    x_v = _ACT[a["att_v"]](vt @ wv.T + f64("conv_v_att.bias"))                                   # [B, P, dh]
    x_q = _ACT[a["att_q"]](q @ f64("linear_q_att.weight").T + f64("linear_q_att.bias"))          # [B, dh]
    x_att = _ACT[a["att_mm"]](x_v * x_q[:, None, :])
    pos = (x_att @ wa.T).transpose(0, 2, 1) + f64("conv_att.bias")[None, :, None]                # [B, G, P]
    e = np.exp(pos - pos.max(2, keepdims=True))
    att = e / e.sum(2, keepdims=True)
    v_att = att @ vt                                                                             # [B, G, dv]
    xs = [_ACT[a["v"]](v_att[:, g] @ f64("list_linear_v_fusion.%d.weight" % g).T + f64("list_linear_v_fusion.%d.bias" % g)) for g in range(G)]
    x_qf = _ACT[a["q"]](q @ f64("linear_q_fusion.weight").T + f64("linear_q_fusion.bias"))
    t = _ACT[a["c"]](np.concatenate(xs, 1) * x_qf)
    logits = t @ f64("linear_classif.weight").T + f64("linear_classif.bias")
    return (logits, att, pos) if want_logits else (logits, att)


def peaked(pos, att):
    """The condition every parity input must meet (else uniform attention hides an indexing or softmax error): some (b, g) whose
    position logits span >= 8, and some map whose maximum is >= 0.3."""
    return bool((pos.max(2) - pos.min(2)).max() >= 8.0 and att.max() >= 0.3)


def random_state(rng, dv, dq, dh_att, G, dh_f, A, gain=3.0, gain_att=None):
    """numpy-seeded parameters with the reference's names and shapes, uniform(+-gain / sqrt(fan_in)); conv_att.weight gets
    `gain_att` instead when it is given (peaked_case raises it until the attention is peaked)."""
    shapes = {"conv_v_att": (dh_att, dv, 1, 1), "linear_q_att": (dh_att, dq), "conv_att": (G, dh_att, 1, 1),
              "linear_q_fusion": (G * dh_f, dq), "linear_classif": (A, G * dh_f)}
    for g in range(G):
        shapes["list_linear_v_fusion.%d" % g] = (dh_f, dv)
    st = {}
    for name, shp in shapes.items():
        g_ = gain_att if (name == "conv_att" and gain_att is not None) else gain
        b = g_ / np.sqrt(shp[1])
        st[name + ".weight"] = rng.uniform(-b, b, size=shp).astype(np.float32)
        st[name + ".bias"] = rng.uniform(-b, b, size=shp[:1]).astype(np.float32)
    return st


def peaked_case(seed, B, dv, dq, dh_att, G, dh_f, A, W, H, acts=None):
    """A seeded parity case whose attention is peaked: conv_att.weight (gain 12) is scaled by the smallest power of two at which
    `peaked` holds in fp64 (the position logits are linear in it, so the factor is found without re-running the model).  P == 1
    cannot be peaked (one position: attention == 1) and is returned as it is.
    -> (state, maps [B, dv, W, H] fp32, q_emb [B, dq] fp32, (logits, att, pos) fp64)."""
    rng = np.random.default_rng(seed)
    st = random_state(rng, dv, dq, dh_att, G, dh_f, A, gain=3.0, gain_att=12.0)
    maps = (np.abs(rng.standard_normal((B, dv, W, H))) * 0.45).astype(np.float32)
    q = (rng.standard_normal((B, dq)) * 0.3).astype(np.float32)
    ref = mlb_att_forward(st, maps, q, acts, want_logits=True)
    if W * H == 1 or peaked(ref[2], ref[1]):
        return st, maps, q, ref
    ba = st["conv_att.bias"].astype(np.float64)[None, :, None]
    lin = ref[2] - ba
    for f in 2.0 ** np.arange(1, 13):
        pos = f * lin + ba
        e = np.exp(pos - pos.max(2, keepdims=True))
        if peaked(pos, e / e.sum(2, keepdims=True)):
            st["conv_att.weight"] = (st["conv_att.weight"] * np.float32(f)).astype(np.float32)       # exact: a power of two
            ref = mlb_att_forward(st, maps, q, acts, want_logits=True)
            assert peaked(ref[2], ref[1])
            return st, maps, q, ref
    raise AssertionError("could not make the attention peaked")
