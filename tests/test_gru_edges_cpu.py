"""CPU: the recipes of tests/gru_edge_cases.py reach what their table claims, and every row of every case counts.

Sensitivity condition (on the inputs, not a measurement): for every row b of a case (every 7th where B > 70) the fp64 gradients with
dq_out[b] zeroed differ from the full fp64 gradients, in at least one tensor, by at least 100 times the GPU bound of that tensor
(1e-4 of its max).  A kernel that loses any one row therefore fails tests/test_gru_edges_gpu.py."""
import numpy as np
import pytest

from gru_edge_cases import CASES, SEED, V, full_wids, make, plan
from gru_ref import lengths
from gru_train_ref import GRADS, gru_train

GPU_TOL = 1e-4
pad = lambda n, m: (n + m - 1) // m * m
cdiv = lambda n, m: (n + m - 1) // m

_MADE = {}


def made(name):
    if name not in _MADE:
        _MADE[name] = make(name)
    return _MADE[name]


@pytest.mark.parametrize("name", list(CASES))
def test_recipe_is_legal_and_fixed(name):
    de, dq, B, T = CASES[name]
    wids, E, w_ih, w_hh, b_ih, b_hh, dq_out = made(name)
    assert wids.shape == (B, T) and wids.min() >= 0 and wids.max() <= V and 1 <= T <= 64
    assert E.shape == (V + 1, de) and w_ih.shape == (3 * dq, de) and w_hh.shape == (3 * dq, dq) and b_ih.shape == b_hh.shape == (3 * dq,)
    assert dq_out.shape == (B, dq) and all(a.dtype == np.float32 for a in (E, w_ih, w_hh, b_ih, b_hh, dq_out))
    assert E[0].all()                                            # the padding row is nonzero, everywhere
    k = 1.0 / np.sqrt(dq)
    assert all(np.abs(a).max() <= k for a in (w_ih, w_hh, b_ih, b_hh))
    again = make(name, SEED)
    assert all(np.array_equal(a, b) for a, b in zip(made(name), again))
    full = full_wids(name)
    assert full.shape == (B, T) and full.min() >= 1 and full.max() <= V and (lengths(full) == T).all()
    if T > 1:
        assert not np.array_equal(full, wids)


def test_each_case_reaches_what_the_table_claims():
    n_t = {name: plan(made(name)[0])[2] for name in CASES}
    lens = {name: lengths(made(name)[0]) for name in CASES}

    assert CASES["unit"] == (1, 1, 2, 2) and list(n_t["unit"]) == [2, 1]

    de, dq, B, T = CASES["odd"]
    w = made("odd")[0]
    assert dq % 4 and de % 4 and (dq * 4) % 16                   # row 1 of h, dq_out, q, dh and E starts off a 16-byte boundary
    assert not w[0].any() and w[3, 4] == 0 and w[3, 5] != 0 and list(lens["odd"]) == [1, 1, 3, 6, 7]
    assert list(n_t["odd"]) == [5, 3, 3, 2, 2, 2, 1]

    de, dq, B, T = CASES["over32"]
    assert pad(de, 32) == 64 and pad(dq, 32) == 64 and cdiv(dq, 32) == 2 and dq - 32 == 1      # second unit tile of one unit
    assert sorted(set((made("over32")[0] != 0).sum(1))) == [0, 1, 2, 3] and list(n_t["over32"]) == [9, 5, 3]

    de, dq, B, T = CASES["over64"]
    assert de == dq == B == 65 and cdiv(B, 64) == 2 and cdiv(dq, 64) == 2 and cdiv(de, 64) == 2
    assert list(n_t["over64"]) == [65, 64, 63, 62]
    assert 3 * pad(dq, 32) == 288 and 288 % 128 == 32            # a ragged third weight-gradient row tile: the column clamp and the m >= kp skip

    de, dq, B, T = CASES["narrow"]
    assert pad(dq, 32) == 32 < 64 and 3 * pad(dq, 32) == 96 < 128 and list(n_t["narrow"]) == [3, 2, 1, 1]

    de, dq, B, T = CASES["wide_e"]
    assert de > 1024 and cdiv(de, 64) == 17 and de % 4 and list(n_t["wide_e"]) == [4, 3, 2]

    de, dq, B, T = CASES["long"]
    w = made("long")[0]
    raw = (w != 0).sum(1)
    assert T == 64 and B > 256
    assert all((raw == n).sum() >= 4 for n in range(T + 1))      # 65 lengths x 5 > 300: four of each is what fits
    assert (np.diff(n_t["long"]) < 0).all() and n_t["long"][0] == B and n_t["long"][T - 1] >= 4     # n_t falls at EVERY step
    perm = plan(w)[1]
    b64, b0 = 260, 299                                           # the planted rows of the plan's second trip
    assert raw[b64] == T and raw[b0] == 0
    assert int(np.flatnonzero(perm == b0)[0]) >= 256             # (a row of length T sorts to the front whatever its input index)
    assert int(np.flatnonzero(perm == b64)[0]) < n_t["long"][T - 1]

    de, dq, B, T = CASES["steps"]
    assert list(n_t["steps"]) == [65] * 2 + [64] * 3 + [32] * 4 + [0] * 3
    perm = plan(made("steps")[0])[1]
    assert lens["steps"][perm[64]] == 2 and (lens["steps"] == 2).sum() == 1      # sorted row 64, alone in the second row tile


_FULL = {}


def full_grads(name):
    if name not in _FULL:
        _FULL[name] = gru_train(*made(name))
    return _FULL[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_row_moves_a_gradient_by_100_bounds(name):
    de, dq, B, T = CASES[name]
    wids, E, w_ih, w_hh, b_ih, b_hh, dq_out = made(name)
    full = full_grads(name)
    worst = np.inf
    for b in range(0, B, 7 if B > 70 else 1):
        d = dq_out.copy()
        d[b] = 0.0
        g = gru_train(wids, E, w_ih, w_hh, b_ih, b_hh, d)
        ratio = max(float(np.abs(g[k] - full[k]).max()) / (GPU_TOL * float(np.abs(full[k]).max())) for k in GRADS if full[k].any())
        worst = min(worst, ratio)
        assert ratio >= 100.0, (name, b, ratio)
    print("%s: the least visible row moves a gradient by %.0f GPU bounds" % (name, worst))
