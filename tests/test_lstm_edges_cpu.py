"""CPU: the recipes of tests/lstm_edge_cases.py reach what their table claims, and every half-row of every case counts.

Sensitivity condition (on the inputs, not a measurement of the kernels): for every row b of a case (every 7th where B > 70, plus the
planted rows) and each half of it (dq_out[b, 0:H], the layer-0 half, and dq_out[b, H:2H], the layer-1 half) the fp64 gradients with that
half zeroed differ from the full fp64 gradients, in at least one tensor, by at least 100 times the GPU bound of that tensor (1e-4 of its
max).  A kernel that loses any one row of either layer's injection therefore fails tests/test_lstm_edges_gpu.py."""
import numpy as np
import pytest

from lstm_edge_cases import CASES, SEED, V, full_wids, make, plan
from lstm_ref import lengths
from lstm_train_ref import GRADS, lstm_train

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
    emb, H, B, T = CASES[name]
    wids, E, l0, l1, dq_out = made(name)
    assert wids.shape == (B, T) and wids.min() >= 0 and wids.max() <= V and 1 <= T <= 64
    assert E.shape == (V + 1, emb) and l0[0].shape == (4 * H, emb) and l1[0].shape == (4 * H, H)
    assert l0[1].shape == l1[1].shape == (4 * H, H) and all(a.shape == (4 * H,) for l in (l0, l1) for a in l[2:])
    assert dq_out.shape == (B, 2 * H) and all(a.dtype == np.float32 for a in (E, dq_out) + l0 + l1)
    assert E[0].all()                                            # the padding row is nonzero, everywhere
    k = 1.0 / np.sqrt(H)
    assert all(np.abs(a).max() <= k for a in l0 + l1)
    again = make(name, SEED)
    same = lambda a, b: all(same(x, y) for x, y in zip(a, b)) if isinstance(a, tuple) else np.array_equal(a, b)
    assert same(tuple(made(name)), tuple(again))
    full = full_wids(name)
    assert full.shape == (B, T) and full.min() >= 1 and full.max() <= V and (lengths(full) == T).all()
    if T > 1:
        assert not np.array_equal(full, wids)


def test_each_case_reaches_what_the_table_claims():
    n_t = {name: plan(made(name)[0])[2] for name in CASES}
    lens = {name: lengths(made(name)[0]) for name in CASES}

    assert CASES["unit"] == (1, 1, 2, 2) and list(n_t["unit"]) == [2, 1]

    emb, H, B, T = CASES["odd"]
    w = made("odd")[0]
    assert H % 4 and emb % 4 and (H * 4) % 16                    # row 1 of h, c and E, and q's layer-1 half, start off a 16-byte boundary
    assert not w[0].any() and w[3, 4] == 0 and w[3, 5] != 0 and list(lens["odd"]) == [7, 1, 3, 6, 7]      # the all-padding row runs T steps
    assert list(n_t["odd"]) == [5, 4, 4, 3, 3, 3, 2]

    emb, H, B, T = CASES["over32"]
    assert pad(emb, 32) == 64 and pad(H, 32) == 64 and cdiv(H, 32) == 2 and H - 32 == 1        # second unit tile of one unit
    assert sorted(set((made("over32")[0] != 0).sum(1))) == [0, 1, 2, 3] and list(n_t["over32"]) == [9, 7, 5]

    emb, H, B, T = CASES["over64"]
    assert emb == H == B == 65 and cdiv(B, 64) == 2 and cdiv(H, 64) == 2 and cdiv(emb, 64) == 2
    assert list(n_t["over64"]) == [65, 65, 64, 63]
    assert 4 * pad(H, 32) == 384 and 384 % 128 == 0              # the weight-gradient row tiles are whole for every H

    emb, H, B, T = CASES["narrow"]
    assert pad(H, 32) == 32 < 64 and 4 * pad(H, 32) == 128 and list(n_t["narrow"]) == [3, 2, 1, 1]

    emb, H, B, T = CASES["wide_e"]
    assert emb > 1024 and cdiv(emb, 64) == 17 and emb % 4 and list(n_t["wide_e"]) == [4, 3, 2]

    emb, H, B, T = CASES["long"]
    w = made("long")[0]
    raw = (w != 0).sum(1)
    assert T == 64 and B > 256
    assert all((raw == n).sum() >= 4 for n in range(T + 1))      # 65 counts x 5 > 300: four of each is what fits
    assert (np.diff(n_t["long"]) < 0).all() and n_t["long"][0] == B and n_t["long"][T - 1] >= 8     # n_t falls at EVERY step
    assert (lens["long"] == 1).sum() >= 4                        # length-1 rows: their only step is the injection
    perm = plan(w)[1]
    b64, b0 = 260, 299                                           # the planted rows of the plan's second trip (input index >= 256)
    assert raw[b64] == T and raw[b0] == 0 and lens["long"][b0] == T
    pos = lambda b: int(np.flatnonzero(perm == b)[0])
    assert pos(b64) < n_t["long"][T - 1] and pos(b0) < n_t["long"][T - 1]       # both run all 64 steps: rows of length T sort to the front
    assert lens["long"][perm[280]] < 10                          # sorted rows >= 256 are the short ones

    emb, H, B, T = CASES["steps"]
    assert list(n_t["steps"]) == [65] * 2 + [64] * 3 + [32] * 4 + [0] * 3
    perm = plan(made("steps")[0])[1]
    assert lens["steps"][perm[64]] == 2 and (lens["steps"] == 2).sum() == 1      # sorted row 64, alone in the second row tile


_FULL = {}


def full_grads(name):
    if name not in _FULL:
        _FULL[name] = lstm_train(*made(name))
    return _FULL[name]


@pytest.mark.parametrize("name", list(CASES))
def test_every_half_row_moves_a_gradient_by_100_bounds(name):
    emb, H, B, T = CASES[name]
    wids, E, l0, l1, dq_out = made(name)
    full = full_grads(name)
    worst = np.inf
    rows = sorted(set(range(0, B, 7 if B > 70 else 1)) | ({260, 299} if name == "long" else set()))
    for b in rows:
        for half in (0, 1):
            d = dq_out.copy()
            d[b, half * H:(half + 1) * H] = 0.0
            g = lstm_train(wids, E, l0, l1, d)
            ratio = max(float(np.abs(g[k] - full[k]).max()) / (GPU_TOL * float(np.abs(full[k]).max())) for k in GRADS if full[k].any())
            worst = min(worst, ratio)
            assert ratio >= 100.0, (name, b, half, ratio)
    print("%s: the least visible half-row moves a gradient by %.0f GPU bounds" % (name, worst))
