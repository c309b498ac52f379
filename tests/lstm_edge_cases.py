"""Recipes of the two-layer LSTM encoder's edge cases: the eight shapes of tests/gru_edge_cases.py read as (emb, H, B, T), with the same
planted nonzero counts and the 2-lstm length rule (an all-padding row runs T steps, not one).  Plain data and numpy;
tests/test_lstm_edges_cpu.py checks what the table claims, tests/test_lstm_edges_gpu.py runs the kernels on them.

The kernels' constants the cases are placed around (csrc/ncx_rnn.h, csrc/ncx_rnn.hip, csrc/ncx_lstm.hip, csrc/ncx_lstm_train.hip) are the GRU's, so no case moved: 32-deep
k-steps (Hp = H rounded up to 32, kx likewise for emb), 64-row x 32-unit step tiles, 64 x 64 sweep / dX tiles, 128 x 64 weight-gradient
tiles, 256 threads in the one-workgroup length plan, RNN_MAX_T = 64, 1024 columns per pass of the embedding gradient.  One difference:
the weight-gradient tiles run over the 4 Hp gate rows, always a whole number of 128-row tiles, so `over64` has no ragged row tile there
(the GRU's 3 dqp = 288 had); its 65 columns still give a second, one-column tile."""
import numpy as np

from gru_edge_cases import CASES, SEED, V, full_wids, make_wids  # noqa: F401  (re-exported: the shapes and the ids are the GRU suite's)
from lstm_ref import lengths

#  name      emb    H    B    T     what it is there for (gru_edge_cases.py has the GRU's reading)
#  unit      1      1    2    2     smallest legal dims; every guarded load
#  odd       7      37   5    7     H % 4 != 0: rows of h, c, dq_out, q are unaligned from row 1 on (and E's); q's layer-1 half starts unaligned
#  over32    33     33   9    3     one past the 32-deep k-step in kx and Hp; a second unit tile holding one unit; two all-padding rows of length T
#  over64    65     65   65   4     one past the 64-column and the 64-row tiles; the all-padding row 64 sorts to the front
#  narrow    5      20   3    4     Hp = 32 < the 64-wide sweep tile; 4 Hp = 128: one weight-gradient row tile
#  wide_e    1030   12   4    3     the embedding gradient's second 1024-column pass; 17 dX column tiles; tanh in the dW_ih0 loader on a ragged tile
#  long      6      24   300  64    T = RNN_MAX_T; B > 256 (a second trip of the plan's row loop); n_t falls at every step
#  steps     10     40   65   12    n_t = 65, 64, 32, 0: one over / exactly on the row tile, on the k-step, then empty steps before T


def make(name, seed=SEED):
    """-> (wids [B, T] int64, E [V + 1, emb], layer0, layer1, dq_out [B, 2 H]); a layer is (w_ih, w_hh, b_ih, b_hh), fp32, nn.LSTM's
    default init U(-1/sqrt(H), 1/sqrt(H)); E = 0.5 randn with a nonzero padding row; dq_out = randn."""
    emb, H, B, T = CASES[name]
    rng = np.random.default_rng([seed, sorted(CASES).index(name)])
    wids = make_wids(name, rng)
    k = 1.0 / np.sqrt(H)
    E = (0.5 * rng.standard_normal((V + 1, emb))).astype(np.float32)         # E[0] is nonzero: the padding row is READ
    layers = []
    for n_in in (emb, H):
        layers.append(tuple(rng.uniform(-k, k, size=s).astype(np.float32) for s in ((4 * H, n_in), (4 * H, H), (4 * H,), (4 * H,))))
    dq_out = rng.standard_normal((B, 2 * H)).astype(np.float32)
    return wids, E, layers[0], layers[1], dq_out


def plan(wids):
    """The device plan restated: (lens, perm, n_t) -- rows sorted by length descending, input order inside a length (k_rnn_plan)."""
    lens = lengths(wids)
    perm = np.argsort(-lens, kind="stable")
    n_t = np.array([(lens > t).sum() for t in range(wids.shape[1])])
    return lens, perm, n_t
