"""fp64 reference, precision contract and input generators for the kNN selector (ncx_knn; DESIGN f4).

Plain numpy.  Nothing here runs the kernel: `exact_knn` is the oracle, `tau` the bound the kernel is held to, `check_knn`
the comparison, `select_trace` a description of which refinement path a row of products drives, and CASES the tables the
CPU and GPU tests share.
"""
import functools

import numpy as np

KNN_BINS, KNN_CAP, KNN_LEVELS, KNN_MARGIN = 1024, 1024, 3, 8          # csrc/ncx_knn.hip
U = 2.0 ** -24                                                         # fp32 unit roundoff


# ---- the oracle ------------------------------------------------------------------------------------------------------------
def exact_d2(q, x):
    """d2[i, j] = sum_t (float64(q_it) - float64(x_jt))**2: the differences of fp32 values are exact in fp64."""
    q64, x64 = np.asarray(q, np.float64), np.asarray(x, np.float64)
    out = np.empty((q64.shape[0], x64.shape[0]))
    step = max(1, (1 << 22) // max(1, x64.size))                       # ~32 MB of differences at a time
    for i in range(0, q64.shape[0], step):
        d = q64[i:i + step, None, :] - x64[None, :, :]
        out[i:i + step] = np.einsum("ijt,ijt->ij", d, d)
    return out


def exact_order(d2):
    """All table rows per query, ordered by (d2, j)."""
    return np.argsort(d2, axis=1, kind="stable")


def exact_knn(q, x, k, d2=None, order=None):
    """-> (indices int64 [nq, k], d2 float64 [nq, n], distances float32 [nq, k]); neighbours ordered by (d2, j)."""
    d2 = exact_d2(q, x) if d2 is None else d2
    idx = (exact_order(d2) if order is None else order)[:, :k]
    return idx.astype(np.int64), d2, np.sqrt(np.take_along_axis(d2, idx, 1)).astype(np.float32)


def _err_terms(q, x):
    """S[i, j] = sum_t |q_it x_jt| + |x_j|^2 / 2: the sum of the magnitudes of the terms of V[i, j] = q_i.x_j - |x_j|^2/2."""
    q64, x64 = np.abs(np.asarray(q, np.float64)), np.abs(np.asarray(x, np.float64))
    return np.atleast_2d(q64) @ x64.T + 0.5 * (x64 * x64).sum(1)[None, :]


def tau(q, x):
    """The precision contract: how far the exact d2 of a returned neighbour may exceed the true k-th d2.  q one row or [nq, dv].

        tau_i = 4 (dv + 2) 2^-24 max_j ( sum_t |q_it x_jt| + |x_j|^2 / 2 )

    Derivation.  The kernel picks its k + 8 candidates on V32, the fp32 value of V(j) = q.x_j - |x_j|^2/2, ordered by
    (V32 descending, j ascending), and ranks those exactly.  Let r be a returned row and t a true neighbour that was left out.
    If t was a candidate it lost to r in the exact ranking and d2(r) <= d2(t).  Otherwise r passed the candidate cut and t did
    not: V32(r) >= V32(t).  Since d2(j) = |q|^2 - 2 V(j),
        d2(r) - d2(t) = 2 (V(t) - V(r)) <= 2 (V(t) - V32(t)) + 2 (V32(r) - V(r)) <= 4 max_j |V32(j) - V(j)|.
    V32(j) is a dot product of dv + 1 terms plus one halving and one addition; the standard bound
    |fl(sum) - sum| <= (dv + 2) u sum|terms| (u = 2^-24) holds for every summation order, fused or not.
    """
    dv = np.asarray(x).shape[1]
    return 4.0 * (dv + 2) * U * _err_terms(q, x).max(axis=1)


def _lsb_exp(a):
    """Per row of a (fp32): the exponent e of the largest power of two 2^e that divides every entry (None-like +inf for 0)."""
    a = np.asarray(a, np.float32).astype(np.float64)
    m, e = np.frexp(a)
    mi = np.abs(m * 2.0 ** 24).astype(np.int64)
    tz = np.zeros_like(mi)
    nz = mi != 0
    low = mi[nz] & -mi[nz]
    tz[nz] = np.round(np.log2(low.astype(np.float64))).astype(np.int64)
    lsb = np.where(nz, e - 24 + tz, 10 ** 6)
    return lsb.min(axis=1)


def exact_products(q, x, S=None):
    """[nq, n] bool: V32[i, j] carries no rounding error.  Every term q_it x_jt, x_jt^2 / 2 and every partial sum of them is a
    multiple of 2^L (L from the lowest set bits of the two rows) and at most S[i, j] in magnitude; below 2^(L + 24) all of
    them are fp32 numbers, so no operation rounds, in any order."""
    S = _err_terms(q, x) if S is None else S
    lq, lx = _lsb_exp(q).astype(np.float64), _lsb_exp(x).astype(np.float64)
    L = np.minimum(lq[:, None] + lx[None, :], 2 * lx[None, :] - 1)
    return S < np.exp2(np.minimum(L + 24, 1000))


def assert_exact_index_precondition(q, x, k, rows, d2, order=None):
    """The inputs guarantee that the kernel's answer for the query rows `rows` is exactly exact_knn's.

    The issue's form: every gap between distinct d2 values in the first k + 9 places exceeds tau_i.  This asserts the same
    argument pair by pair, with each row's own error bound e_j = (dv + 2) u S[i, j] (0 where exact_products holds) in place
    of the table-wide maximum in tau_i (4 max_j e_j = tau_i, so the issue's form implies this one).  An outlier row then
    widens only its own bound.  For every true neighbour t (place <= k) and every row r beyond place k + 8:
        r and t are the same vector, or both products are exact, or d2(r) - d2(t) > 2 (e_r + e_t).
    Then V32(r) < V32(t), or they tie and the index decides as in the exact order; so fewer than k + 8 rows precede t in the
    candidate order and t is a candidate.  Raises AssertionError otherwise: a case cannot pass by skipping it."""
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    n, dv = x.shape
    if n <= k + KNN_MARGIN:
        return                                                         # every row is a candidate
    rows = np.asarray(rows)
    S = _err_terms(q[rows], x)
    ex = exact_products(q[rows], x, S)
    e = np.where(ex, 0.0, (dv + 2) * U * S)
    order = exact_order(d2) if order is None else order
    same = np.unique(x, axis=0, return_inverse=True)[1].reshape(-1)       # equal label <=> the same vector
    for a, i in enumerate(rows):
        top, rest = order[i, :k], order[i, k + KNN_MARGIN:]
        dk, emax = d2[i, top[-1]], e[a, top].max()
        r = rest[d2[i, rest] - dk <= 2 * (e[a, rest] + emax)][:, None]   # the few rows that need the pairwise look
        t = top[None, :]
        ok = (ex[a, r] & ex[a, t]) | (d2[i, r] - d2[i, t] > 2 * (e[a, r] + e[a, t])) | (same[r] == same[t])
        assert ok.all(), "exact_index precondition fails for query %d: rows %s against its neighbours %s" % (
            i, r[~ok.all(1), 0][:8], top)


def check_knn(idx, dist, q, x, k, exact_index, d2=None, order=None):
    """Asserts the kernel's (idx [nq, k], dist [nq, k]) against fp64.  exact_index: False, True, or a bool mask over the query
    rows that must equal exact_knn's indices (the rest are held to the tau rule, which is asserted for every row).
    -> (largest d2 - D_k over all returned neighbours, smallest tau_i): what DESIGN f4 records."""
    idx, dist = np.asarray(idx), np.asarray(dist)
    q, x = np.asarray(q, np.float32), np.asarray(x, np.float32)
    nq, n = q.shape[0], x.shape[0]
    assert idx.shape == (nq, k) and dist.shape == (nq, k) and idx.dtype == np.int64 and dist.dtype == np.float32
    assert idx.min() >= 0 and idx.max() < n, (idx.min(), idx.max())
    srt = np.sort(idx, axis=1)
    assert np.all(srt[:, 1:] != srt[:, :-1]), "repeated index in rows %s" % np.nonzero((srt[:, 1:] == srt[:, :-1]).any(1))[0][:8]
    ref_idx, d2, _ = exact_knn(q, x, k, d2, order)
    got = np.take_along_axis(d2, idx, 1)
    want = np.sqrt(got).astype(np.float32)                             # the distance of the row actually returned
    assert np.all(np.abs(dist.astype(np.float64) - want) <= np.spacing(want)), float(np.abs(dist - want).max())
    dd, di = np.diff(got, axis=1), np.diff(idx, axis=1)
    assert np.all((dd > 0) | ((dd == 0) & (di > 0))), "rows not ordered by (d2, index): %s" % np.nonzero(~((dd > 0) | ((dd == 0) & (di > 0))).all(1))[0][:8]
    t = tau(q, x)
    excess = got - np.take_along_axis(d2, ref_idx[:, -1:], 1)
    assert np.all(excess <= t[:, None]), "tau rule: excess %.6g, tau %.6g (row %d)" % (
        excess.max(), t[np.argmax(excess.max(1) - t)], int(np.argmax(excess.max(1) - t)))
    mask = np.full(nq, bool(exact_index)) if np.isscalar(exact_index) or isinstance(exact_index, bool) else np.asarray(exact_index, bool)
    if mask.any():
        rows = np.nonzero(mask)[0]
        assert_exact_index_precondition(q, x, k, rows, d2, order)
        bad = rows[(idx[rows] != ref_idx[rows]).any(1)]
        assert bad.size == 0, "%d of %d rows differ from the exact order; first: row %d\n got %s\n ref %s" % (
            bad.size, rows.size, bad[0], idx[bad[0]], ref_idx[bad[0]])
    return float(excess.max()), float(t.min())


# ---- which path a row of products drives -----------------------------------------------------------------------------------
def products(q, x):
    """V[i, j] = q_i.x_j - |x_j|^2/2 as the fp32 rounding of the fp64 value (the kernel's differs in the last bits)."""
    q64, x64 = np.asarray(q, np.float64), np.asarray(x, np.float64)
    with np.errstate(all="ignore"):
        return (q64 @ x64.T - 0.5 * (x64 * x64).sum(1)[None, :]).astype(np.float32)


class Trace(tuple):
    """(levels used, hist[chosen] at exit, members of the last bin exceed KNN_CAP - kc) + .in_bin (per level) and .tied."""
    def __new__(cls, levels, in_bin, tied, kc):
        t = tuple.__new__(cls, (levels, in_bin[-1], in_bin[-1] > KNN_CAP - kc))
        t.in_bin, t.tied = list(in_bin), tied
        return t


def _bins(v, lo, scale):
    f32 = np.float32
    with np.errstate(all="ignore"):
        f = (v - f32(lo)) * f32(scale)
    f = np.where(np.isnan(f), 0.0, f)
    return np.clip(np.trunc(f), 0, KNN_BINS - 1).astype(np.int64)


def _choose(hist, need):
    """The bin holding the need-th largest member: (chosen, members in the bins above it)."""
    acc = 0
    for b in range(KNN_BINS - 1, -1, -1):
        if acc + hist[b] >= need:
            return b, acc
        acc += hist[b]
    raise AssertionError("fewer members than needed")


def select_trace(V_row, k, refine="minmax"):
    """numpy-float32 restatement of k_knn_select's three-level histogram select of the kc = min(k + 8, n) largest values.

    refine="minmax": the kernel as it is.  A level histograms the members (values inside [lo, hi]) into 1024 bins over
    [lo, hi] and picks the bin of the kc-th largest.  It stops when that bin's members fit the buffer (<= KNN_CAP - kc), when
    they are all one value, or at the last level; otherwise [lo, hi] becomes the smallest and largest member of the bin.
    refine="lo_arith": the selector before that, which recomputed the chosen bin's edges as lo + w * chosen (widened by 1e-6)
    and stopped on `scale == 0`.
    A description of the input, not an oracle for the kernel: a test uses it to prove which path its table drives."""
    f32 = np.float32
    v = np.asarray(V_row, np.float32)
    kc = min(k + KNN_MARGIN, v.size)
    lo, hi = v.min(), v.max()
    member = np.ones(v.size, bool)
    above_total, in_bin = 0, []
    with np.errstate(all="ignore"):
        for level in range(KNN_LEVELS):
            rng = f32(hi) - f32(lo)
            scale = min(f32(KNN_BINS) / rng, np.finfo(f32).max) if rng > 0 else f32(0)
            b = _bins(v, lo, scale)
            hist = np.bincount(b[member], minlength=KNN_BINS)
            chosen, acc = _choose(hist, kc - above_total)
            in_bin.append(int(hist[chosen]))
            inside = member & (b == chosen)
            tied = bool(v[inside].min() == v[inside].max())
            last = level == KNN_LEVELS - 1
            if refine == "minmax":
                if hist[chosen] <= KNN_CAP - kc or tied or last:
                    return Trace(level + 1, in_bin, tied, kc)
                lo, hi = v[inside].min(), v[inside].max()
            else:
                if hist[chosen] <= KNN_CAP - kc or scale == 0 or last:
                    return Trace(level + 1, in_bin, tied, kc)
                w = rng / f32(KNN_BINS)
                e0, e1 = f32(lo) + w * f32(chosen), f32(lo) + w * f32(chosen + 1)
                lo, hi = e0 - f32(1e-6) * abs(e0), e1 + f32(1e-6) * abs(e1)
            above_total += acc
            member = inside


# ---- the tables ------------------------------------------------------------------------------------------------------------
def lattice(seed, n, dv, g=0.125, top=8):
    """Rows of multiples of g in [0, top g): every product against such a row is exact in fp32 (exact_products), so the exact
    order is guaranteed whatever the gaps, ties included."""
    return (np.random.default_rng(seed).integers(0, top, (n, dv)) * g).astype(np.float32)


def abs_normal(seed, n, dv):                                            # the distribution of tests/test_knn.py
    return (np.abs(np.random.default_rng(seed).standard_normal((n, dv))) * 0.45).astype(np.float32)


def _case(x, k=25, q=None, exact=True, parent=None, current=(1, False), trace_rows=None, **kw):
    nq = (x if q is None else q).shape[0]
    exact = np.full(nq, exact) if isinstance(exact, bool) else exact
    return dict(x=x, q=q, k=k, exact=exact, parent=parent, current=current,
                trace_rows=np.arange(0, nq, max(1, nq // 24)) if trace_rows is None else trace_rows, **kw)


OUTLIER_ROW = 1234


def _outliers(scales):
    x = lattice(2, 3000, 64)
    rows = [OUTLIER_ROW + 100 * i for i in range(len(scales))]
    for r, s in zip(rows, scales):
        x[r] *= np.float32(s)
    exact = np.ones(3000, bool)
    exact[rows] = False                       # an outlier's own query sees every row at almost one distance: tau rule
    return x, exact, rows


def depth_a():
    return _case(lattice(1, 3000, 64), parent=(1, False), current=(1, False))


def depth_b():
    """2900 rows packed around the centre (1, ..., 1) with relative spread 2^-8 (the nearest grid to the issue's 1e-3 on which
    the packed rows' products stay exact in fp32) and 100 spread rows, one of them far, so that level 0's bins are wider than
    the packed rows' products.  The queries have 36 ones: the packed rows are at d2 ~ 28, about one spread row in seven nearer."""
    rng = np.random.default_rng(3)
    spread = rng.integers(0, 2, (100, 64)).astype(np.float32)
    spread[99] = 4.0
    packed = np.ones((2900, 64), np.float32)
    for r in packed:
        c = rng.permutation(64)[:16]
        r[c[:8]] += np.float32(2.0 ** -8); r[c[8:]] -= np.float32(2.0 ** -8)
    x = np.concatenate([spread, packed])[rng.permutation(3000)]
    q = np.zeros((64, 64), np.float32)
    for r in q:
        r[rng.permutation(64)[:36]] = 1.0
    return _case(x, q=q, parent=(2, False), current=(2, False), level0_in_bin=2000)


def depth_c():
    x, exact, rows = _outliers([30.0])
    return _case(x, exact=exact, parent=(2, False), current=(2, False), outliers=rows)


def depth_d():
    x, exact, rows = _outliers([1e3])
    return _case(x, exact=exact, parent=(3, False), current=(2, False), outliers=rows)


def depth_e():
    x, exact, rows = _outliers([1e5])
    return _case(x, exact=exact, parent=(3, True), current=(2, False), outliers=rows)


def depth_three():
    """Two outliers a factor 100 apart: each level sheds one of them, the third resolves the rest."""
    x, exact, rows = _outliers([1e2, 1e4])
    return _case(x, exact=exact, current=(3, False), outliers=rows)


def depth_exhausted():
    """Three outliers a factor 100 apart: after the last level the chosen bin still holds all the other rows, with distinct
    products.  The call must raise, not answer."""
    x, exact, rows = _outliers([1e2, 1e4, 1e6])
    return _case(x, exact=False, current=(3, True), outliers=rows, raises=True)


def signed_normal():
    return _case(np.random.default_rng(4).standard_normal((1000, 64)).astype(np.float32), exact=False)


def _offset(dv):
    x = (50.0 + 0.5 * np.random.default_rng(5).standard_normal((1000, dv))).astype(np.float32)
    return _case(x, q=x[:64].copy(), exact=False)


def _cluster(eps):
    rng = np.random.default_rng(6)
    c = np.abs(rng.standard_normal(2048)) * 0.45
    x = (c[None, :] + eps * rng.standard_normal((2000, 2048))).astype(np.float32)
    # at 1e-4 the 1999 other rows' products are two or three fp32 values: whether they tie beyond the buffer turns on last bits
    return _case(x, q=x[:48].copy(), exact=False, current=(1, False) if eps > 2e-4 else None)


def tie_groups():
    """Rows on a line t v (t = 1..59): from the query at t = 0 the 40 copies of t = 11 take places 11..50 (across k = 25 and
    k + 8); from the query at t = 60 the 40 copies of t = 31 take places 29..68 (across k + 8 only).  Lowest indices win."""
    rng = np.random.default_rng(7)
    v = (rng.integers(0, 4, 64) * 0.25).astype(np.float32)
    t = np.concatenate([np.arange(1, 60), np.full(39, 11), np.full(39, 31)])[rng.permutation(137)]
    x = (t[:, None] * v[None, :]).astype(np.float32)
    return _case(x, q=np.stack([0 * v, 60 * v]).astype(np.float32), trace_rows=np.arange(2))


def zero_table():
    """tests/test_knn.py::test_knn_mass_ties: 1460 zero rows tie in the last bin of every query; k = 30."""
    x = np.zeros((1500, 64), np.float32)
    x[:40] = abs_normal(5, 40, 64)
    return _case(x, k=30, parent=(3, True), current=(1, True), trace_rows=np.arange(40, 1500, 61))


def near_block():
    """1200 copies of one row, nearer to every query than any other row (itself apart)."""
    rng = np.random.default_rng(8)
    x = lattice(8, 2000, 64, g=0.5)
    x[rng.permutation(2000)[:1200]] = 1.75
    return _case(x, current=(1, True))


def _edge(n, k):
    return _case(lattice(100 + n, n, 64), k=k)


def _dv(dv):
    return _case(lattice(200 + dv, 300, dv))


CASES = {"depth_a": depth_a, "depth_b": depth_b, "depth_c": depth_c, "depth_d": depth_d, "depth_e": depth_e,
         "depth_three": depth_three, "depth_exhausted": depth_exhausted, "signed_normal": signed_normal,
         "offset50_dv64": lambda: _offset(64), "offset50_dv2048": lambda: _offset(2048),
         "cluster_1e-2": lambda: _cluster(1e-2), "cluster_1e-3": lambda: _cluster(1e-3), "cluster_1e-4": lambda: _cluster(1e-4),
         "tie_groups": tie_groups, "zero_table": zero_table, "near_block": near_block,
         "one_query": lambda: _case(lattice(9, 300, 64), q=lattice(10, 1, 64)),
         "other_queries": lambda: _case(lattice(9, 300, 64), q=lattice(11, 37, 64))}
for _n in (1, 2, 9, 33, 255, 256, 257):
    for _k in sorted({1, min(_n, 25), min(_n, 120)}):
        CASES["edge_n%d_k%d" % (_n, _k)] = functools.partial(_edge, _n, _k)
for _d in (4, 5, 7, 63, 65):
    CASES["dv%d" % _d] = functools.partial(_dv, _d)


@functools.lru_cache(maxsize=None)
def case(name):
    """The case and its fp64 distances, computed once and shared (treat both as read-only)."""
    c = CASES[name]()
    c["queries"] = c["x"] if c["q"] is None else c["q"]
    c["d2"] = exact_d2(c["queries"], c["x"])
    c["order"] = exact_order(c["d2"])
    return c
