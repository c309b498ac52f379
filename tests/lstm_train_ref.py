"""fp64 restatement of training the two-layer LSTM question encoder (tests/lstm_ref.py's forward, then backward through time), in numpy.

With len_b = #{t : wids[b, t] != 0} (T when that is 0), per layer l, for t from len_b - 1 down to 0, on the rows still inside their question:

    dh^l_t = [t == len_b - 1] dq_out[b, l H : (l + 1) H] + da^l_{t+1} W_hh^l  (+ da^1_t W_ih^1 when l == 0)
    dc_t   = dc_{t+1} f_{t+1} + dh_t o_t (1 - tanh(c_t)^2)
    da_o = dh_t tanh(c_t) o (1 - o);  da_i = dc_t g i (1 - i);  da_g = dc_t i (1 - g^2);  da_f = dc_t c_{t-1} f (1 - f)      c_{-1} = 0
    dW_ih^l = sum da^l_t^T x^l_t;  dW_hh^l = sum_{t >= 1} da^l_t^T h^l_{t-1};  db_ih^l = db_hh^l = sum da^l_t
    dX_t = da^0_t W_ih^0;  dE[w] = sum over the valid pairs with id w of dX_t (1 - tanh(E[w])^2);  dE[0] = 0 (nn.Embedding(padding_idx=0))

A layer is the tuple (w_ih, w_hh, b_ih, b_hh), gate blocks i | f | g | o."""
import numpy as np

from lstm_ref import lengths

GRADS = ("E", "w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1")


def _sig(a):
    return 1.0 / (1.0 + np.exp(-a))


def lstm_train(wids, E, layer0, layer1, dq_out, lens=None):
    """-> {"q": [B, 2 H], "E", "w_ih0", ..., "b_hh1": the gradients of sum(q * dq_out)}, all float64."""
    wids = np.asarray(wids)
    E, dq_out = np.asarray(E, np.float64), np.asarray(dq_out, np.float64)
    layers = [tuple(np.asarray(a, np.float64) for a in layer) for layer in (layer0, layer1)]
    B, T = wids.shape
    H = layers[0][1].shape[1]
    lens = lengths(wids) if lens is None else np.asarray(lens)
    h = [np.zeros((B, H)), np.zeros((B, H))]
    c = [np.zeros((B, H)), np.zeros((B, H))]
    q = np.zeros((B, 2 * H))
    stash = [[], []]
    for t in range(T):
        act = lens > t
        x = np.tanh(E[wids[act, t]])
        for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
            hp, cp = h[l][act].copy(), c[l][act].copy()
            a = x @ w_ih.T + b_ih + hp @ w_hh.T + b_hh
            gi, gf, gg, go = _sig(a[:, :H]), _sig(a[:, H:2 * H]), np.tanh(a[:, 2 * H:3 * H]), _sig(a[:, 3 * H:])
            cn = gf * cp + gi * gg
            hn = go * np.tanh(cn)
            stash[l].append((act, x, hp, cp, gi, gf, gg, go, cn))
            h[l][act], c[l][act] = hn, cn
            x = hn
        last = lens - 1 == t
        q[last, :H], q[last, H:] = h[0][last], h[1][last]
    g = {"q": q, "E": np.zeros_like(E)}
    for l, (w_ih, w_hh, b_ih, b_hh) in enumerate(layers):
        g["w_ih%d" % l], g["w_hh%d" % l] = np.zeros_like(w_ih), np.zeros_like(w_hh)
        g["b_ih%d" % l], g["b_hh%d" % l] = np.zeros_like(b_ih), np.zeros_like(b_hh)
    dh = [np.zeros((B, H)), np.zeros((B, H))]          # what step t + 1 sent back to h^l_t
    dc = [np.zeros((B, H)), np.zeros((B, H))]          # dc_{t+1} f_{t+1}
    for t in range(T - 1, -1, -1):
        last = lens - 1 == t
        dh[0][last] += dq_out[last, :H]
        dh[1][last] += dq_out[last, H:]
        for l in (1, 0):
            w_ih, w_hh = layers[l][0], layers[l][1]
            act, x, hp, cp, gi, gf, gg, go, cn = stash[l][t]
            d = dh[l][act]
            tc = np.tanh(cn)
            dcell = dc[l][act] + d * go * (1.0 - tc * tc)
            da = np.concatenate([dcell * gg * gi * (1.0 - gi), dcell * cp * gf * (1.0 - gf), dcell * gi * (1.0 - gg * gg),
                                 d * tc * go * (1.0 - go)], 1)
            g["w_ih%d" % l] += da.T @ x
            g["b_ih%d" % l] += da.sum(0)
            g["b_hh%d" % l] += da.sum(0)
            if t >= 1:
                g["w_hh%d" % l] += da.T @ hp
            dc[l][act] = dcell * gf
            dh[l][act] = da @ w_hh
            if l == 1:
                dh[0][act] += da @ w_ih
            else:
                np.add.at(g["E"], wids[act, t], (da @ w_ih) * (1.0 - x * x))
    g["E"][0] = 0.0
    return g
