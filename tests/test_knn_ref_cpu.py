"""The kNN reference of tests/knn_ref.py checks itself here, without a GPU: the oracle against the scikit-learn fixture, the
refinement path each table of tests/test_knn_select_gpu.py drives (so that a GPU pass means the path was taken), and the
exact-order precondition of every case that claims it."""
import os

import numpy as np
import pytest

import knn_ref as R
from conftest import GOLDEN

G8 = dict(np.load(os.path.join(GOLDEN, "g8_knn.npz")))
WIDE = {"offset50_dv2048", "cluster_1e-2", "cluster_1e-3", "cluster_1e-4"}       # dv 2048, tau rule only: no fp64 distances needed here


@pytest.mark.parametrize("case", ["a", "c"])
def test_exact_knn_agrees_with_fixture(case):
    seed, n, dv, k, dup = [int(v) for v in G8[case + "_spec"]]
    assert dup == 0
    x = R.abs_normal(seed, n, dv)
    idx, d2, dist = R.exact_knn(x, x, k)
    assert np.array_equal(idx, G8[case + "_indices"].astype(np.int64))
    assert np.all(dist[:, 0] == 0.0) and np.abs(dist - G8[case + "_distances"]).max() <= 2e-3


def test_tau_and_exact_products_on_known_rows():
    q = np.array([[1.0, 2.0, -3.0, 0.5]], np.float32)
    x = np.array([[2.0, 0.0, 1.0, 4.0], [0.1, 0.2, 0.3, 0.4]], np.float32)
    s = np.array([2 + 0 + 3 + 2 + 21 / 2, 0.1 + 0.4 + 0.9 + 0.2 + 0.15])
    assert np.allclose(R.tau(q, x), 4 * 6 * 2.0 ** -24 * s.max()) and np.allclose(R.tau(q[0], x), R.tau(q, x))
    assert R.exact_products(q, x).tolist() == [[True, False]]          # 0.1 is no short binary fraction
    big = np.array([[2.0 ** 12 + 1, 1.0, 1.0, 1.0]], np.float32)       # its square needs 25 bits
    assert R.exact_products(q, big).tolist() == [[False]]


def _v32(q, x, order):
    """V = q.x - |x|^2/2 evaluated in fp32, one rounding per operation, the terms taken in `order`."""
    f = np.float32
    dot, sq = f(0), f(0)
    for t in order:
        dot = f(dot + f(q[t] * x[t]))
        sq = f(sq + f(x[t] * x[t]))
    return f(dot + f(f(-0.5) * sq))


def test_exact_products_against_fp32_evaluation():
    """Signed dyadic rows of 3 to 16 significant bits.  Wherever exact_products holds, V evaluated in fp32 is the fp64 value bit
    for bit in every order tried; it must refuse the wide rows, and among those a product does round although every entry is
    dyadic (so the refusal is needed, not mere caution)."""
    rng = np.random.default_rng(21)
    dv = 16
    rows = np.concatenate([rng.integers(-2 ** b + 1, 2 ** b, (4, dv)) * 2.0 ** -b for b in (3, 6, 9, 10, 11, 13, 16)]).astype(np.float32)
    rows[5, :8] = 0                                                     # zeros carry no bits
    ex = R.exact_products(rows, rows)
    V = rows.astype(np.float64) @ rows.astype(np.float64).T - 0.5 * (rows.astype(np.float64) ** 2).sum(1)[None, :]   # exact: < 2^-32 steps, 40 bits
    orders = [np.arange(dv), np.arange(dv)[::-1], rng.permutation(dv)]
    rounded = np.zeros_like(ex)
    for i in range(len(rows)):
        for j in range(len(rows)):
            got = [float(_v32(rows[i], rows[j], o)) for o in orders]
            rounded[i, j] = any(g != V[i, j] for g in got)
    assert not (ex & rounded).any(), np.argwhere(ex & rounded)[:4]
    assert ex[:12, :12].all() and not ex[20:, 20:].any()                # up to 9 bits: 18-bit terms, 16 of them; from 13 bits: no
    assert rounded[~ex].any()


def test_select_trace_on_hand_made_rows():
    v = np.arange(3000, dtype=np.float32)
    assert tuple(R.select_trace(v, 25)) == (1, 3, False)               # 3000 values over 1024 bins: 3 in the top-33 bin
    v[1:] = 1e9 + np.arange(2999)                                     # one far minimum: all others share the top bin
    t = R.select_trace(v, 25)
    assert t[0] == 2 and t.in_bin[0] == 2999 and not t[2]
    z = np.zeros(3000, np.float32)
    t = R.select_trace(z, 25)
    assert tuple(t) == (1, 3000, True) and t.tied                      # ties: overflow of one value


@pytest.mark.parametrize("name", sorted(R.CASES))
def test_case_drives_its_path_and_meets_its_precondition(name):
    if name in WIDE:
        c = R.CASES[name]()
        c["queries"] = c["x"] if c["q"] is None else c["q"]
        assert not c["exact"].any()
    else:
        c = R.case(name)
    V = R.products(c["queries"][c["trace_rows"]], c["x"])
    # no path is claimed for cluster_1e-4 alone: its products are a handful of values and which rows tie turns on their last bits
    assert (c["current"] is None) == (name == "cluster_1e-4")
    for mode, want in (("minmax", c["current"]), ("lo_arith", c["parent"])):
        if want is None:
            continue
        for r, v in zip(c["trace_rows"], V):
            if r in c.get("outliers", ()):
                continue                                               # an outlier's own query sees another table
            t = R.select_trace(v, c["k"], mode)
            assert (t[0], t[2]) == want, (name, mode, int(r), tuple(t), t.in_bin)
            # far from the threshold KNN_CAP - kc = 991: the GPU's products differ in the last bits and must not change the path
            # (the members of a bin of exact ties are one value there too: their count cannot move)
            assert all(h <= 500 or h >= 2000 or (t.tied and h == t.in_bin[-1]) for h in t.in_bin), (name, mode, int(r), t.in_bin)
            if "level0_in_bin" in c:
                assert t.in_bin[0] >= c["level0_in_bin"]
    rows = np.nonzero(c["exact"])[0]
    if rows.size:
        R.assert_exact_index_precondition(c["queries"], c["x"], c["k"], rows, c["d2"], c["order"])
    else:
        assert name in WIDE or name in ("depth_exhausted", "signed_normal", "offset50_dv64")


def test_precondition_refuses_an_unguaranteed_table():
    """Real-valued rows at one distance from the query, closer together than the rounding of their products."""
    x = (1.0 + 1e-6 * np.random.default_rng(0).standard_normal((200, 64))).astype(np.float32)
    q = np.zeros((1, 64), np.float32) + np.float32(0.3)
    d2 = R.exact_d2(q, x)
    with pytest.raises(AssertionError):
        R.assert_exact_index_precondition(q, x, 25, np.arange(1), d2)


def test_check_knn_rejects_wrong_answers():
    c = R.case("edge_n257_k25")
    idx, d2, dist = R.exact_knn(c["queries"], c["x"], 25, c["d2"], c["order"])
    R.check_knn(idx, dist, c["queries"], c["x"], 25, True, d2)
    far = idx.copy(); far[3, 24] = c["order"][3, 200]                  # a far row in the last place
    swapped = idx.copy(); swapped[5, [1, 2]] = swapped[5, [2, 1]]
    repeat = idx.copy(); repeat[7, 4] = repeat[7, 3]
    off = dist.copy(); off[9, 6] = np.nextafter(np.nextafter(off[9, 6], np.float32(9)), np.float32(9))
    for bad_idx, bad_dist in ((far, dist), (swapped, dist), (repeat, dist), (idx, off)):
        with pytest.raises(AssertionError):
            R.check_knn(bad_idx, bad_dist, c["queries"], c["x"], 25, True, d2)
