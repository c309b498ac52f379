"""fp64 restatement of the two-layer LSTM question encoder (TwoLSTM in eval mode, recurrence over time), in numpy.

    len_b = #{t : wids[b, t] != 0}, and T when that is 0 (the reference's select_last indexes step len_b - 1 = -1: the LAST step)
    x_t = tanh(E[wids[b, t]])   (row 0 of E is read like any other row)
    layer l:  [i f g o] = W_ih x + b_ih + W_hh h + b_hh;  c' = s(f) c + s(i) tanh(g);  h' = s(o) tanh(c');  h_0 = c_0 = 0
    layer 1's x_t is layer 0's h_t;  q[b] = [h^0 | h^1] after step len_b - 1

Gate blocks of w_ih [4 H, in], w_hh [4 H, H], b_ih, b_hh [4 H] are i | f | g | o (torch.nn.LSTM's order).  A layer is the tuple
(w_ih, w_hh, b_ih, b_hh)."""
import numpy as np


def lengths(wids):
    wids = np.asarray(wids)
    n = (wids != 0).sum(1)
    return np.where(n > 0, n, wids.shape[1])


def select_last(x, lens):
    """x [B, T, D] -> x[b, lens[b] - 1]; index -1 (a length of 0, as process_lengths itself gives for all padding) is step T - 1."""
    x = np.asarray(x)
    return x[np.arange(x.shape[0]), np.asarray(lens) - 1]


def lstm_layer(x, layer):
    """x [B, T, in] -> h [B, T, H], every step of every row."""
    w_ih, w_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in layer)
    B, T, _ = x.shape
    H = w_hh.shape[1]
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    h, c = np.zeros((B, H)), np.zeros((B, H))
    out = np.zeros((B, T, H))
    for t in range(T):
        g = x[:, t] @ w_ih.T + b_ih + h @ w_hh.T + b_hh
        c = sig(g[:, H:2 * H]) * c + sig(g[:, :H]) * np.tanh(g[:, 2 * H:3 * H])
        h = sig(g[:, 3 * H:]) * np.tanh(c)
        out[:, t] = h
    return out


def lstm_layers(wids, E, layer0, layer1):
    """-> (x_0 [B, T, H], x_1 [B, T, H]): both layers' outputs at every step."""
    x = np.tanh(np.asarray(E, np.float64)[np.asarray(wids)])
    x_0 = lstm_layer(x, layer0)
    return x_0, lstm_layer(x_0, layer1)


def lstm_encode(wids, E, layer0, layer1, lens=None):
    x_0, x_1 = lstm_layers(wids, E, layer0, layer1)
    lens = lengths(wids) if lens is None else lens
    return np.concatenate([select_last(x_0, lens), select_last(x_1, lens)], 1)
