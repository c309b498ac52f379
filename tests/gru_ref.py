"""fp64 restatement of the question encoder (embedding -> one-layer GRU -> hidden state after the last word), in numpy.

    len_b = max(1, #{t : wids[b, t] != 0});  x_t = E[wids[b, t]]   (row 0 of E is read like any other row)
    r = s(W_ir x + b_ir + W_hr h + b_hr);  z = s(W_iz x + b_iz + W_hz h + b_hz);  n = tanh(W_in x + b_in + r (W_hn h + b_hn))
    h' = (1 - z) n + z h,  h_0 = 0;  q[b] = h after step len_b - 1

Gate blocks of w_ih [3 dq, de], w_hh [3 dq, dq], b_ih, b_hh [3 dq] are r | z | n (torch.nn.GRU's order)."""
import numpy as np


def lengths(wids):
    return np.maximum((np.asarray(wids) != 0).sum(1), 1)


def gru_encode(wids, E, w_ih, w_hh, b_ih, b_hh):
    wids = np.asarray(wids)
    E, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in (E, w_ih, w_hh, b_ih, b_hh))
    B, T = wids.shape
    dq = w_hh.shape[1]
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    lens = lengths(wids)
    h = np.zeros((B, dq))
    q = np.zeros((B, dq))
    for t in range(T):
        gx = E[wids[:, t]] @ w_ih.T + b_ih
        gh = h @ w_hh.T + b_hh
        r = sig(gx[:, :dq] + gh[:, :dq])
        z = sig(gx[:, dq:2 * dq] + gh[:, dq:2 * dq])
        n = np.tanh(gx[:, 2 * dq:] + r * gh[:, 2 * dq:])
        h = (1.0 - z) * n + z * h
        last = lens - 1 == t
        q[last] = h[last]
    return q
