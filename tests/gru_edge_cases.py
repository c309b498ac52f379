"""Recipes of the GRU encoder's edge cases: shapes OFF the six that tests/test_gru_gpu.py and tests/test_gru_train_gpu.py share.  Plain
data and numpy; tests/test_gru_edges_cpu.py checks what the table claims, tests/test_gru_edges_gpu.py runs the kernels on them.

The kernels' constants the cases are placed around (csrc/ncx_rnn.h, csrc/ncx_rnn.hip, csrc/ncx_gru.hip, csrc/ncx_gru_train.hip): 32-deep k-steps (dqp = dim_q rounded up
to 32, kx likewise for dim_emb), 64-row x 32-unit step tiles, 64 x 64 sweep / dX tiles, 128 x 64 weight-gradient tiles over the 3 dqp
gate rows, 256 threads in the one-workgroup length plan, RNN_MAX_T = 64, 1024 columns per pass of the embedding gradient.

`long` asks for every length 0 .. 64 several times over in B = 300 rows: 65 lengths fit four times (260 rows), not five (325), so each
length is planted four times and the remaining 40 rows are uniform 1 .. 64."""
import numpy as np

V = 30          # words; E has V + 1 rows, row 0 is the padding row
SEED = 3

#        name      dim_emb dim_q  B   T
CASES = {"unit":   (1,     1,     2,   2),    # smallest legal dims; every guarded load
         "odd":    (7,     37,    5,   7),    # dim_q % 4 != 0: rows of h, dq_out, q, dh are unaligned from row 1 on (and E's: dim_emb = 7)
         "over32": (33,    33,    9,   3),    # one past the 32-deep k-step in kx and dqp; a second unit tile holding one unit
         "over64": (65,    65,    65,  4),    # one past the 64-column and the 64-row tiles
         "narrow": (5,     20,    3,   4),    # dqp = 32 < the 64-wide sweep tile; 3 dqp = 96 < the 128-row weight-gradient tile
         "wide_e": (1030,  12,    4,   3),    # the embedding gradient's second 1024-column pass; 17 dX column tiles
         "long":   (6,     24,    300, 64),   # T = RNN_MAX_T; B > 256 (a second trip of the plan's row loop); n_t falls at every step
         "steps":  (10,    40,    65,  12)}   # n_t = 65, 64, 32, 0: one over / exactly on the row tile, on the k-step, then empty steps before T


def planted_lengths(name, rng):
    """The number of nonzero word ids of every row, in input order (0: an all-padding row, which still runs one step)."""
    de, dq, B, T = CASES[name]
    if name == "unit":
        return [2, 1]
    if name == "odd":
        return [0, 1, 3, 7, 7]                              # row 3 then gets a zero inside: 6 nonzero ids
    if name == "over32":
        return [3, 0, 1, 2, 3, 2, 1, 3, 0]
    if name == "over64":
        lens = [T] * B
        lens[20], lens[40], lens[64] = 2, 3, 0            # n_t = 65, 64, 63, 62
        return lens
    if name == "narrow":
        return [4, 2, 1]
    if name == "wide_e":
        return [3, 3, 2, 1]
    if name == "long":
        lens = rng.permutation(np.concatenate([np.repeat(np.arange(T + 1), 4), rng.integers(1, T + 1, size=B - 4 * (T + 1))]))
        for at, n in ((260, T), (299, 0)):                  # a row of length T and an all-padding row in the plan's second trip (b >= 256)
            i = int(np.flatnonzero(lens == n)[0])
            lens[i], lens[at] = lens[at], lens[i]
        return list(lens)
    if name == "steps":
        return list(rng.permutation([9] * 32 + [5] * 32 + [2]))
    raise KeyError(name)


def make_wids(name, rng):
    de, dq, B, T = CASES[name]
    lens = planted_lengths(name, rng)
    assert len(lens) == B
    wids = np.zeros((B, T), np.int64)
    for b, n in enumerate(lens):
        wids[b, :n] = rng.integers(1, V + 1, size=n)
    if name == "odd":
        wids[3, 4] = 0                                      # a zero inside the question: 6 nonzero ids, stepped over t < 6
    return wids


def full_wids(name):
    """The case's wids with every length replaced by T (other ids): a step on them leaves every row, step and pad position of a
    workspace's stash finite and unrelated to the case."""
    de, dq, B, T = CASES[name]
    return np.random.default_rng(SEED + 1000).integers(1, V + 1, size=(B, T)).astype(np.int64)


def make(name, seed=SEED):
    """-> (wids [B, T] int64, E [V + 1, de], w_ih [3 dq, de], w_hh [3 dq, dq], b_ih [3 dq], b_hh [3 dq], dq_out [B, dq]), fp32."""
    de, dq, B, T = CASES[name]
    rng = np.random.default_rng([seed, sorted(CASES).index(name)])
    wids = make_wids(name, rng)
    k = 1.0 / np.sqrt(dq)
    E = (0.5 * rng.standard_normal((V + 1, de))).astype(np.float32)          # E[0] is nonzero: the padding row is READ
    w_ih, w_hh, b_ih, b_hh = (rng.uniform(-k, k, size=s).astype(np.float32) for s in ((3 * dq, de), (3 * dq, dq), (3 * dq,), (3 * dq,)))
    dq_out = rng.standard_normal((B, dq)).astype(np.float32)
    return wids, E, w_ih, w_hh, b_ih, b_hh, dq_out


def plan(wids):
    """The device plan restated: (lens, perm, n_t) -- rows sorted by length descending, input order inside a length (k_rnn_plan)."""
    from gru_ref import lengths
    lens = lengths(wids)
    perm = np.argsort(-lens, kind="stable")
    n_t = np.array([(lens > t).sum() for t in range(wids.shape[1])])
    return lens, perm, n_t
