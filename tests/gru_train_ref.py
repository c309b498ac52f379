"""fp64 restatement of training the question encoder (tests/gru_ref.py's forward, then backward through time), in numpy.

With len_b = max(1, #{t : wids[b, t] != 0}), for t from len_b - 1 down to 0, on the rows still inside their question:

    dh_t  = [t == len_b - 1] dq_out[b] + (what step t + 1 sends back)
    dn = dh (1 - z);  dz = dh (h_{t-1} - n);  h_{-1} = 0
    da_n = dn (1 - n^2);  da_z = dz z (1 - z);  da_r = da_n hn r (1 - r);  da_hn = da_n r          hn = W_hn h_{t-1} + b_hn
    dh_{t-1} = dh z + [da_r | da_z | da_hn] W_hh
    dGx_t = [da_r | da_z | da_n]  -> dW_ih, db_ih, dX_t = dGx_t W_ih;   dGh_t = [da_r | da_z | da_hn] -> dW_hh (t >= 1 only), db_hh

dE[v] is the sum of dX_t[b] over the valid pairs with wids[b, t] == v, and dE[0] = 0 (nn.Embedding(padding_idx=0))."""
import numpy as np

from gru_ref import lengths

GRADS = ("E", "w_ih", "w_hh", "b_ih", "b_hh")


def gru_train(wids, E, w_ih, w_hh, b_ih, b_hh, dq_out):
    """-> {"q": [B, dq], "E", "w_ih", "w_hh", "b_ih", "b_hh": the gradients of sum(q * dq_out)}, all float64."""
    wids = np.asarray(wids)
    E, w_ih, w_hh, b_ih, b_hh, dq_out = (np.asarray(a, np.float64) for a in (E, w_ih, w_hh, b_ih, b_hh, dq_out))
    B, T = wids.shape
    dq = w_hh.shape[1]
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    lens = lengths(wids)
    h = np.zeros((B, dq))
    q = np.zeros((B, dq))
    stash = []
    for t in range(T):
        act = lens > t
        x = E[wids[act, t]]
        gx = x @ w_ih.T + b_ih
        gh = h[act] @ w_hh.T + b_hh
        r = sig(gx[:, :dq] + gh[:, :dq])
        z = sig(gx[:, dq:2 * dq] + gh[:, dq:2 * dq])
        hn = gh[:, 2 * dq:]
        n = np.tanh(gx[:, 2 * dq:] + r * hn)
        stash.append((act, x, h[act].copy(), r, z, n, hn))
        h[act] = (1.0 - z) * n + z * h[act]
        last = lens - 1 == t
        q[last] = h[last]
    g = {"q": q, "E": np.zeros_like(E), "w_ih": np.zeros_like(w_ih), "w_hh": np.zeros_like(w_hh), "b_ih": np.zeros_like(b_ih),
         "b_hh": np.zeros_like(b_hh)}
    dh = np.zeros((B, dq))
    for t in range(T - 1, -1, -1):
        act, x, hp, r, z, n, hn = stash[t]
        last = lens - 1 == t
        dh[last] += dq_out[last]
        d = dh[act]
        dn, dz = d * (1.0 - z), d * (hp - n)
        da_n, da_z = dn * (1.0 - n * n), dz * z * (1.0 - z)
        da_r, da_hn = da_n * hn * r * (1.0 - r), da_n * r
        dgx = np.concatenate([da_r, da_z, da_n], 1)
        dgh = np.concatenate([da_r, da_z, da_hn], 1)
        g["w_ih"] += dgx.T @ x
        g["b_ih"] += dgx.sum(0)
        g["b_hh"] += dgh.sum(0)
        if t >= 1:
            g["w_hh"] += dgh.T @ hp
        np.add.at(g["E"], wids[act, t], dgx @ w_ih)
        dh[act] = d * z + dgh @ w_hh
    g["E"][0] = 0.0
    return g
