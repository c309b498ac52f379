"""CPU: what tests/gemm_ref.py claims about the generic GEMM engine's restatement, its bound and its cases, and the host-only entries
ncx_diag_gemm (its NCX_E_DIMS list), ncx_diag_gemm_slab_bytes, ncx_diag_cfg_supported and ncx_diag_plan_gemm.  No kernel runs here;
tests/test_gemm_engine_gpu.py runs them."""
import ctypes
import json
import math
import os

import numpy as np
import pytest

import gemm_ref as G
from conftest import ROOT

PROFILE = os.path.join(ROOT, "profiles", "gemm_engine_edges.json")
NULL_STREAM = ctypes.c_void_p(0)
_INPUTS = {}


def inputs(c):
    if c["id"] not in _INPUTS:
        _INPUTS[c["id"]] = G.build(c)
    return _INPUTS[c["id"]]


# ---- the restatement against plain numpy and against a scalar walk over the raw buffers -------------------------------------------------
def _x_at(X, i, side, r, col):
    """x(r, col) of an operand, read element by element from the flat buffers."""
    d = X.ops[i][side]
    buf, base = X.bufs[d["name"]]
    at = lambda row: float(buf[base + row * d["ld"] + col])
    if d["kind"] == G.PLAIN:
        return at(r)
    if d["kind"] == G.GATHER:
        return at(int(X.bufs[d["name"] + ".idx"][0][r * d["stride"]]))
    if d["kind"] == G.GMUL:
        return at(int(X.bufs[d["name"] + ".idx"][0][r * d["stride"]])) * at(int(X.bufs[d["name"] + ".idx2"][0][r * d["stride"]]))
    lbuf, lbase = X.bufs[d["name"] + ".lse"]
    return 2.0 ** (at(r) * G.LOG2E - float(lbuf[lbase + r]))


def _scalar_element(c, X, p, r, n):
    """One output element of problem p, term by term in Python floats, epilogue in the kernel's order."""
    form, e, M = c["form"], c["epi"], c["M"]
    N = c["segs"][p]["n_cols"]
    n_max = max(s["n_cols"] for s in c["segs"][:G.n_problems(c)])
    get = lambda name, row, ld, col: float(X.bufs[name][0][X.bufs[name][1] + row * ld + col])
    total = 0.0
    for i in G.problem_segs(c, p):
        acc = 0.0
        for k in range(c["segs"][i]["klen"]):
            a = _x_at(X, i, "a", r, k) if G.colk(form, "a") else _x_at(X, i, "a", k, r)
            b = _x_at(X, i, "b", n, k) if G.colk(form, "b") else _x_at(X, i, "b", k, n)
            acc += a * b
        if c["fold"]:
            R = len(c["segs"])
            acc = (acc + get("fold_bias", 0, 0, i * N + n)) * get("fold_mul", r // c["fold"]["div"], R * N + 5, i * N + n)
        total += acc
    v = total
    if e.get("rowadd"):
        v += get("rowadd", r // e["rowadd"][0], n_max + e["rowadd"][1], n)
    if e.get("bias"):
        v += get("bias", 0, 0, n)
    if e.get("act") == 1:
        v = max(v, 0.0)
    elif e.get("act") == 2:
        v = math.tanh(v)
    if e.get("dropout"):
        v = v * G.drop_scale(e["dropout"][1]) if G.keep_matrix(c, X, N)[r, n] else 0.0
    if e.get("gate"):
        v = v * e["gate"][1] if get("gate", r, n_max + e["gate"][0], n) > 0 else 0.0
    return v


@pytest.mark.parametrize("group", G.GROUPS)
def test_restatement_matches_a_scalar_walk(group):
    """Sampled elements (the corners and a few inside) of every fifth case of the group, and of every case with an epilogue, a fold, a
    chain, a group or a split, agree with a term-by-term evaluation from the raw buffers to fp64 rounding."""
    cases = [c for c in G.CASES if c["group"] == group and c["id"] != "persistent-nt-64x64-M2561-N2561-k4"]
    picked = cases if group not in ("tiles", "kinds") else cases[::5]
    for c in picked:
        X = inputs(c)
        ref = G.restate(c, X)
        rng = np.random.default_rng(len(c["id"]))
        for p, (v, S) in enumerate(ref):
            M, N = v.shape
            pts = {(0, 0), (M - 1, N - 1), (0, N - 1), (M - 1, 0)} | {(int(rng.integers(M)), int(rng.integers(N))) for _ in range(3)}
            for r, n in pts:
                want = _scalar_element(c, X, p, r, n)
                assert abs(v[r, n] - want) <= 1e-12 * max(S[r, n], abs(want), 1e-300), (c["id"], p, r, n, v[r, n], want)


def test_restatement_matches_numpy_matmul_on_dense_copies():
    """A chain is one matmul over the concatenated reduction axis; a split problem's chunks add up to the unsplit product."""
    for c in G.CASES:
        if c["fold"] or c["epi"] or c["group"] == "persistent":
            continue
        X = inputs(c)
        for p, (v, S) in enumerate(G.restate(c, X)):
            A = [G.dense(X, i, "a")[0] for i in G.problem_segs(c, p)]
            B = [G.dense(X, i, "b")[0] for i in G.problem_segs(c, p)]
            ka, kb = (1 if G.colk(c["form"], "a") else 0), (1 if G.colk(c["form"], "b") else 0)
            a, b = np.concatenate(A, axis=ka), np.concatenate(B, axis=kb)
            a = a if ka == 1 else a.T
            b = b if kb == 1 else b.T
            want = a @ b.T
            assert np.abs(v - want).max() <= 1e-12 * max(S.max(), 1e-300), c["id"]
            assert (S >= np.abs(want) * (1 - 1e-12)).all(), c["id"]


def test_case_table_covers_what_it_says():
    by_inst = {}
    for c in G.CASES:
        by_inst.setdefault(G.instance_of(c), []).append(c)
    assert sorted(by_inst) == sorted(n for n, _, _, _ in G.INSTANCES)
    for name, form, cfg, fold in G.INSTANCES:
        bm, bn = G.TILE[cfg]
        tiles = [c for c in by_inst[name] if c["group"] == "tiles"]
        klens = set(G.TILE_KLEN) | (set(G.TILE_KLEN_96x128) if cfg == 2 else set())
        assert {(c["M"], c["segs"][0]["n_cols"], c["segs"][0]["klen"]) for c in tiles} == {(M, N, k) for M, N in G.tile_shapes(bm, bn) for k in klens}
        offs = {s[side]["off"] for c in by_inst[name] for s in c["segs"] for side in "ab"}
        assert {1, 2, 3} <= offs, name
    # every operand row is wider than its columns
    for c in G.CASES[::17]:
        X = inputs(c)
        assert all(d["ld"] > d["cols"] for ops in X.ops for d in ops.values())
    # the operand kinds where the form takes them
    for name, form, cfg, fold in G.INSTANCES:
        if not fold:
            side = "b" if form == G.TN else "a"
            assert {s[side]["kind"] for c in by_inst[name] if c["group"] == "kinds" for s in c["segs"]} == {0, 1, 2, 3}, name
    assert any(s["a"]["stride"] == 3 for c in G.CASES for s in c["segs"])
    assert {len(c["segs"]) for c in G.CASES if c["group"] == "chains"} == {2, 3, 10}
    assert {len(c["segs"]) for c in G.CASES if c["group"] == "groups"} >= {3, 10}
    assert {c["segs"][0]["split"] for c in G.CASES if c["group"] == "split" and c["mode"] == G.CHAIN} >= {2, 3, 4, 5, 8, 16, 24}
    mixed = [c for c in G.CASES if c["mode"] == G.GROUP and {min(s["split"], 2) for s in c["segs"]} == {1, 2}]
    assert mixed
    assert {(len(c["segs"]), c["fold"]["div"], c["M"]) for c in G.CASES if c["group"] == "fold"} == {(R, d, M) for R in (1, 2, 10) for d in (1, 25) for M in (63, 64, 65)}
    # (the GPU test reads the grid the launch was given back from ncx_diag_gemm and fails if the loop was not taken: at four workgroups per
    # CU, which the tile's LDS would allow, 1681 items would no longer be more than twice the 1024 slots)
    pers = G.BY_ID["persistent-nt-64x64-M2561-N2561-k4"]
    assert G.work_items(pers) == 1681 > 2 * 3 * 256


def test_gather_ids_stay_in_range_and_repeat():
    for c in G.CASES:
        if c["group"] not in ("kinds", "chains", "groups"):
            continue
        X = inputs(c)
        for ops in X.ops:
            for d in ops.values():
                if d["kind"] in (G.GATHER, G.GMUL):
                    ids = X.bufs[d["name"] + ".idx"][0].reshape(d["rows"], d["stride"])[:, 0]
                    assert ids.min() >= 1 and ids.max() == d["T"] - 1
                    assert d["rows"] <= 2 or len(set(ids.tolist())) < d["rows"]


def test_split_cases_hit_empty_chunks_and_padding_ids():
    from neuralcx import _lib
    L = _lib.lib()
    pads, empties = 0, 0
    for c in G.CASES:
        if c["group"] != "split":
            continue
        bm, bn = G.TILE[c["cfg"]]
        for p in range(G.n_problems(c)):
            S = c["segs"][p]["split"]
            tm, tn = -(-c["M"] // bm), -(-c["segs"][p]["n_cols"] // bn)
            assert L.ncx_wgmap_check(tm, tn, S) == 0, (c["id"], p)
            pads += G.wgmap_count(tm, tn, S) > tm * tn * S
            steps, chunks = G.chunk_steps(c, p)
            empties += any(s0 == s1 for s0, s1 in chunks)
            assert chunks[0][0] == 0 and chunks[-1][1] == len(steps) and all(a[1] == b[0] for a, b in zip(chunks, chunks[1:]))
    assert pads >= 4 and empties >= 6
    shapes = {(c["M"] > c["segs"][0]["n_cols"]) for c in G.CASES if c["group"] == "split" and c["mode"] == G.CHAIN and c["cfg"] == 0}
    assert shapes == {True, False}                            # tiles_m < tiles_n and the reverse


# ---- mutations: what the bound must catch -------------------------------------------------------------------------------------------------
def _worst(c, X, got, ref):
    w = 0.0
    for (g, _), (r, S) in zip(got, ref):
        err = np.abs(g - r)
        if (err[S == 0] > 0).any():
            return math.inf
        w = max(w, float((err[S > 0] / (G.U24 * S[S > 0])).max()))
    return w


def _argmax_term(c, X, i, r, n):
    a, b = G.dense(X, i, "a")[0], G.dense(X, i, "b")[0]
    ar = a[r] if G.colk(c["form"], "a") else a[:, r]
    bn = b[n] if G.colk(c["form"], "b") else b[:, n]
    return int(np.abs(ar * bn).argmax())


MUTATIONS = [
    ("tiles-nt-64x64-M81-N135-k160", lambda c, X: dict(mut=("drop_k", 0, 80, 134, _argmax_term(c, X, 0, 80, 134)))),
    ("tiles-tn-128x64-M145-N135-k160", lambda c, X: dict(mut=("drop_k", 0, 144, 0, _argmax_term(c, X, 0, 144, 0)))),
    ("tiles-nn-128x128-M145-N263-k103", lambda c, X: dict(mut=("drop_k", 0, 0, 262, _argmax_term(c, X, 0, 0, 262)))),
    ("chains-nt-96x128-10", lambda c, X: dict(mut=("drop_k", 5, 112, 0, _argmax_term(c, X, 5, 112, 0)))),
    ("tiles-nt-96x128-M97-N127-k97", lambda c, X: dict(mut=("lose_row", 96))),
    ("tiles-tn-64x64-M63-N65-k33", lambda c, X: dict(mut=("lose_col", 64))),
    ("tiles-nt-64x64-M81-N135-k33", lambda c, X: dict(mut=("shift_window", (0, "a")))),
    ("tiles-nn-64x64-M81-N135-k65", lambda c, X: dict(mut=("shift_window", (0, "b")))),
    ("kinds-tn-64x64-softmax-k5", lambda c, X: dict(mut=("shift_window", (0, "b")))),
    ("chains-nt-64x64-10", lambda c, X: dict(mut=("skip_seg", 5))),
    ("chains-tn-128x128-3", lambda c, X: dict(mut=("skip_seg", 2))),
    ("split-nt-64x64-M70-N200-S5", lambda c, X: dict(mut=("chunk_twice", 2))),
    ("split-nt-64x64-M70-N200-S5", lambda c, X: dict(mut=("chunk_omit", 4))),
    ("split-tn-64x64-M200-N70-S24", lambda c, X: dict(mut=("chunk_omit", 2))),
    ("split-tn-128x64-group-mixed", lambda c, X: dict(mut=("chunk_twice", 0))),
    ("epilogue-nt-64x64-all", lambda c, X: dict(order=("rowadd", "act", "bias", "dropout", "gate"))),
    ("epilogue-nt-128x128-all-gen", lambda c, X: dict(order=("rowadd", "bias", "dropout", "act", "gate"))),
    ("epilogue-nt-64x64-all", lambda c, X: dict(order=("bias", "act", "rowadd", "dropout", "gate"))),
]


@pytest.mark.parametrize("case_id,make", MUTATIONS, ids=["%s-%d" % (m[0], i) for i, m in enumerate(MUTATIONS)])
def test_mutations_break_the_bound_a_hundredfold(case_id, make):
    c = G.BY_ID[case_id]
    X = inputs(c)
    ref = G.restate(c, X)
    got = G.restate(c, X, **make(c, X))
    w = _worst(c, X, got, ref)
    print("mutation on %s: ratio %.3g against c = %.1f" % (case_id, w, G.bound_c(c["group"])))
    assert w >= 100 * G.bound_c(c["group"]), (case_id, w)


# ---- the float32 restatement: where c comes from ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("group", G.GROUPS)
def test_recorded_float32_ratios_reproduce(group):
    """ORACLE32_RATIO is the float32 restatement's worst ratio on the host that wrote profiles/gemm_engine_edges.json, rounded up: it stays at
    above the measurement there, and c = 4 x the constant does not move with the host.  Another host's BLAS sums in another order, which moves
    a group's maximum by tens of percent either way: what is asked here is the same size, within a factor of three on both sides."""
    got = max(G.float32_ratio(c, inputs(c)) for c in G.CASES if c["group"] == group)
    const = G.ORACLE32_RATIO[group]
    print("float32 ratio group %s measured %.3f constant %.3f c %.3f" % (group, got, const, G.bound_c(group)))
    assert const / 3.0 <= got <= 3.0 * const, (group, got, const)
    prof = json.load(open(PROFILE))["groups"][group]
    assert prof["float32_ratio_constant"] == const and prof["c"] == G.bound_c(group)
    assert prof["float32_ratio_measured"] <= const
    assert prof["gpu_max_ratio"] is None or prof["gpu_max_ratio"] <= prof["c"]


def _fma_chain(terms, order):
    acc = np.float32(0)
    for k in order:
        acc = np.float32(np.float64(acc) + terms[k])          # one rounding per term: a chain of fused multiply-adds
    return acc


@pytest.mark.parametrize("case_id,r,n", [("kinds-nn-128x128-gather-k160", 69, 29), ("fold-R1-div25-M64", 38, 38), ("tiles-nt-64x64-M64-N64-k160", 23, 34),
                                         ("persistent-nt-64x64-M2561-N2561-k4", 304, 1561)])
def test_kernel_k_order_keeps_the_float32_worst_elements(case_id, r, n):
    """Why three groups' kernel maxima in profiles/gemm_engine_edges.json equal the float32 restatement's to every printed digit.  The kernel
    feeds a 32-deep step's MFMAs k = 8 t + 2 (lane group) + e, i.e. 0 2 4 6 1 3 5 7 inside each run of eight, where BLAS walks k upwards.
    The worst element of a case is one whose partial sums grow large early, so its error is made of a few roundings at large partial sums,
    and a permutation inside runs of eight passes through nearly the same partial sums: at these elements a chain of fused multiply-adds in
    the kernel's order and in ascending order round to the SAME float (elsewhere they differ: the GPU test reports that the kernel and the
    float32 restatement agree in about a quarter of a K = 160 output's elements).  So the equal maxima are a property of the data."""
    c = G.BY_ID[case_id]
    X = inputs(c)
    a, b = G.dense(X, 0, "a", np.float32)[0], G.dense(X, 0, "b", np.float32)[0]
    terms = a[r].astype(np.float64) * (b[n] if G.colk(c["form"], "b") else b[:, n]).astype(np.float64)
    K = len(terms)
    x32 = G.restate(c, X, np.float32)[0][0][r, n] if not c["fold"] else None
    up = _fma_chain(terms, range(K))
    assert _fma_chain(terms, G.kernel_k_order(K)) == up
    if x32 is not None:
        assert up == x32                                       # ... and that ascending chain is what the float32 restatement's BLAS computes here


# ---- the host-only entries ------------------------------------------------------------------------------------------------------------------
def test_struct_layout_matches_header():
    from neuralcx._lib import NcxDiagGemmArgs, NcxDiagOperand
    assert ctypes.sizeof(NcxDiagOperand) == 56 and ctypes.sizeof(NcxDiagGemmArgs) == 1592
    assert NcxDiagGemmArgs.klen.offset == 32 + 20 * 56 and NcxDiagGemmArgs.out.offset == 32 + 20 * 56 + 120
    assert NcxDiagGemmArgs.slab_bytes.offset == 1584


def test_cfg_supported():
    from neuralcx import ops
    for form in (G.NT, G.TN, G.NN):
        for cfg in range(-1, 7):
            assert ops.diag_cfg_supported(form, cfg) == (cfg in G.SUPPORTED[form]), (form, cfg)
    assert not ops.diag_cfg_supported(3, 0) and not ops.diag_cfg_supported(-1, 0)


def _args(case_id, **kw):
    c = G.BY_ID[case_id]
    return c, G.fill_args(c, inputs(c), G.fake_addr, **kw)


def test_every_case_passes_or_fails_the_entry_as_the_table_says():
    """A case the engine does not implement (an operand narrower than four columns: M = 1 on the TN forms) is NCX_E_DIMS before any launch;
    every other case's description is accepted by the same check (ncx_diag_gemm_slab_bytes runs it) and sized as WgMap sizes it."""
    from neuralcx import ops
    rejected = 0
    for c in G.CASES:
        a = G.fill_args(c, inputs(c), G.fake_addr, slab=G.fake_addr(""), slab_bytes=1 << 40)
        if G.expected_rc(c) == G.E_DIMS:
            assert ops.diag_gemm_rc(a, NULL_STREAM) == G.E_DIMS, c["id"]
            rejected += 1
        else:
            assert ops.diag_gemm_slab_bytes(a) == 4 * G.slab_floats(c), c["id"]
    assert rejected == 3 * len(G.TILE_KLEN)


def test_entry_rejects_what_the_engine_does_not_implement():
    from neuralcx import ops
    rc = lambda a: ops.diag_gemm_rc(a, NULL_STREAM)
    # a cfg the form has no instantiation for
    for form, case_id in ((G.NT, "tiles-nt-64x64-M64-N64-k64"), (G.TN, "tiles-tn-64x64-M64-N64-k64"), (G.NN, "tiles-nn-64x64-M64-N64-k64")):
        for cfg in range(-1, 7):
            if cfg not in G.SUPPORTED[form]:
                c, a = _args(case_id)
                a.cfg = cfg
                assert rc(a) == G.E_DIMS, (form, cfg)
    # an operand with cols < 4 (either side)
    for side in "ab":
        c, a = _args("tiles-nt-64x64-M64-N64-k4")
        getattr(a, side)[0].cols = 3
        a.klen[0] = 3
        assert rc(a) == G.E_DIMS
    # klen, M, n_cols disagreeing with the operands' extents; ld below cols
    for field, delta in (("klen", 1), ("klen", -1), ("n_cols", 1)):
        c, a = _args("tiles-tn-64x64-M64-N64-k64")
        getattr(a, field)[0] += delta
        assert rc(a) == G.E_DIMS, field
    c, a = _args("tiles-nn-64x64-M64-N64-k64")
    a.M += 1
    assert rc(a) == G.E_DIMS
    c, a = _args("tiles-nn-64x64-M64-N64-k64")
    a.a[0].ld = a.a[0].cols - 1
    assert rc(a) == G.E_DIMS
    c, a = _args("chains-nt-64x64-3")
    a.klen[2] += 1
    assert rc(a) == G.E_DIMS
    # nseg outside 1 .. NCX_MAX_SEG
    for nseg in (0, 11, -1):
        c, a = _args("chains-nt-64x64-10")
        a.nseg = nseg
        assert rc(a) == G.E_DIMS
    # split > 1 with anything the fix-up drops
    for term in ("rowadd", "mask", "gen", "gate", "rowsplit4"):
        c, a = _args("epilogue-nt-64x64-%s" % term)
        assert ops.diag_gemm_slab_bytes(a) == 0
        a.split[0] = 2
        assert rc(a) == G.E_DIMS, term
    c, a = _args("fold-R2-div1-M64")
    a.split[0] = 2
    assert rc(a) == G.E_DIMS
    # ... while bias and activation may split
    c, a = _args("split-nt-64x64-bias-tanh-S5")
    assert ops.diag_gemm_slab_bytes(a) == 4 * G.slab_floats(c) > 0
    # FOLD outside an NT chain on 64 x 64 tiles
    for change in (dict(form=G.NN), dict(mode=G.GROUP), dict(cfg=1)):
        c, a = _args("fold-R1-div1-M64")
        for k, v in change.items():
            setattr(a, k, v)
        assert rc(a) == G.E_DIMS, change
    # code ranges, rowdiv, missing pointers
    for field, v in (("form", 3), ("mode", 2), ("act", 3), ("dropout", 3)):
        c, a = _args("epilogue-nt-64x64-bias")
        setattr(a, field, v)
        assert rc(a) == G.E_DIMS, field
    c, a = _args("epilogue-nt-64x64-rowadd")
    a.rowdiv = 0
    assert rc(a) == G.E_DIMS
    c, a = _args("kinds-nt-64x64-gmul-k33")
    a.a[0].idx2 = None
    assert rc(a) == -1
    c, a = _args("split-nt-64x64-M70-N200-S4")                  # a split launch without its slab
    assert rc(a) == -1
    c, a = _args("split-nt-64x64-M70-N200-S4", slab=G.fake_addr(""), slab_bytes=4 * G.slab_floats(G.BY_ID["split-nt-64x64-M70-N200-S4"]) - 4)
    assert rc(a) == -3


# The products the library plans with plan_gemm, at full widths (B = 512, K = 24, dv 2048, dq 2400, dz 360, A 2000, H 256; MUTAN dhv = dhq =
# 360, R = 10; MLB dh 1200; the scorers' H = da = 300): (who, form, M, N, reduction extent(s), allow_96) -> the tile config it gets on a
# chip of 256 CUs.  The k-split depends on the measured occupancy and is printed, not pinned.
_B, _K, _DV, _DQ, _DZ, _A, _H = 512, 24, 2048, 2400, 360, 2000, 256
_MK, _MV = _B * _K, _B * (_K + 1)
_ks = lambda *ks: sum(-(-k // 32) for k in ks)
PLANNED = [
    ("step Gt (U_GT)", G.NT, _H, _A, _ks(300), False, "64x64"),
    ("step Sh (U_SH)", G.NT, _B, _H, _ks(_DV, _DQ, _DZ, 300), False, "64x64"),
    ("step linear_1 fallback (U_MAIN)", G.NT, _MK, _H, _ks(_DV, _DV, _K + 1, _DZ, _A), True, "96x128"),
    ("step hidden layer fallback (U_FWD_L), H = 1024", G.NT, _MK, 1024, _ks(1024), True, "64x64"),
    ("step dE (U_DE)", G.TN, _A, 300, 2 * _ks(_H), False, "64x64"),
    ("step dW1[:, a_other] (U_DW1AK)", G.NN, _H, 300, _ks(_A), False, "64x64"),
    ("step dW_l (U_DWL), H = 1024", G.TN, 1024, 1024, _ks(_MK), False, "64x64"),
    ("step dX_l (U_DXL), H = 1024", G.NN, _MK, 1024, _ks(1024), False, "64x64"),
    ("producers x_q", G.NT, _B, 360, _ks(_DQ), True, "64x64"),
    ("mutan h_q", G.NT, _B, 3600, _ks(360), True, "64x64"),
    ("mutan x_v (generic route)", G.NT, _MV, 360, _ks(_DV), True, "96x128"),
    ("producers classifier (generic route)", G.NT, _MK, _A, _ks(360), True, "64x64"),
    ("mlb x_v (generic route)", G.NT, _MV, 1200, _ks(_DV), True, "128x128"),
    ("mutan trainer x_v", G.NT, _B, 360, _ks(_DV), True, "64x64"),
    ("mutan trainer h_v / h_q", G.NT, _B, 3600, _ks(360), True, "64x64"),
    ("trainers logits", G.NT, _B, _A, _ks(360), True, "64x64"),
    ("mutan trainer dWc", G.TN, _A, 360, _ks(_B), False, "64x64"),
    ("mutan trainer dWhv | dWhq", G.TN, 3600, 720, _ks(_B), False, "64x64"),
    ("mutan trainer dx_v", G.NN, _B, 360, _ks(3600), False, "64x64"),
    ("mutan trainer dWv", G.TN, 360, _DV, _ks(_B), False, "64x64"),
    ("mlb trainer x_v", G.NT, _B, 1200, _ks(_DV), True, "64x64"),
    ("mlb trainer logits", G.NT, _B, _A, _ks(1200), True, "64x64"),
    ("mlb trainer dWv | dWq", G.TN, 1200, _DV + _DQ, _ks(_B), False, "64x64"),
    ("pairlin shared part", G.NT, _B, 300, _ks(_DV, _DQ, _DZ, 300), False, "64x64"),
    ("pairlin hidden", G.NT, _MK, 300, _ks(_DV, _DZ), True, "96x128"),
    ("pairlin dW candidate columns", G.TN, 300, _DV + _DZ, _ks(_MK), False, "64x64"),
    ("pairlin dW shared columns", G.TN, 300, _DV + _DQ + _DZ + 300, _ks(_B), False, "64x64"),
    ("pairlin dA", G.NN, _B, 300, _ks(300), False, "64x64"),
    ("linctx scores", G.NT, _B, _K, _ks(_K * _DZ), False, "64x64"),
    ("contrastive hidden", G.NT, _MK, 300, _ks(_DV, _DZ), True, "96x128"),
]


def test_planner_table_at_full_widths():
    """Which instantiation plan_gemm gives the library's products at full widths (DESIGN.md 4b carries this table)."""
    from neuralcx import ops
    seen = set()
    for who, form, M, N, ksteps, allow96, tile in PLANNED:
        p = ops.diag_plan_gemm(form, M, N, ksteps, allow96)
        print("%-50s %s %6d x %5d, %4d k-steps -> %s x %d" % (who, G.FORM_NAME[form], M, N, ksteps, p["tile"], p["split"]))
        assert p["tile"] == tile, (who, p)
        assert ops.diag_cfg_supported(form, p["cfg"])
        seen.add((form, p["cfg"]))
    # no planner rule selects the 96 x 64 NT tile, and at these widths none selects the big TN tile
    assert (G.NT, 3) not in seen and (G.TN, 1) not in seen
    # the planner's own rules: big NT tiles need M >= 96, N >= 128 and 0.75 of the CUs in tiles; the edge shapes of the suite run 64 x 64
    for M, N in ((95, 4096), (4096, 127), (1056, 1056)):
        assert ops.diag_plan_gemm(G.NT, M, N, 64, True)["tile"] == "64x64"
    assert ops.diag_plan_gemm(G.TN, 2048, 2048, 64, False)["tile"] == "128x128"          # 256 big tiles, 64 k-steps: where TN 128 x 128 begins
    assert ops.diag_plan_gemm(G.TN, 2048, 2048, 63, False)["tile"] == "64x64"
    assert ops.diag_plan_gemm(G.NN, 2048, 2048, 64, False)["tile"] == "128x128"
    # choose_split cuts from 16 k-steps on: the trainers' and scorers' edge shapes (K <= 132) never split
    for ks in range(1, 16):
        assert ops.diag_plan_gemm(G.NT, 70, 37, ks, False)["split"] == 1
    assert ops.diag_plan_gemm(G.NT, 70, 37, 16, False)["split"] == 2


def test_cfg_hook_ignores_a_tile_the_form_does_not_instantiate(monkeypatch):
    """NCX_CFG_<id> (NCX_EXPERIMENT=1) takes a config the use's form instantiates and ignores any other: dW_l is a TN product, which has no
    96 x 64 tile (the value used to run 64 x 64 tiles behind a slab sized for 96 x 64)."""
    from neuralcx import _lib
    d = _lib.NcxDims(B=64, K=24, dv=64, dq=64, dz=64, da=64, A=64, H=256, L=2, n_img=2048, flags=15)
    base = _lib.plan_query(d, "DWL")
    monkeypatch.setenv("NCX_EXPERIMENT", "1")
    monkeypatch.setenv("NCX_CFG_9", "3")
    assert _lib.plan_query(d, "DWL")["tile"] == base["tile"]
    monkeypatch.setenv("NCX_CFG_9", "4")
    assert _lib.plan_query(d, "DWL")["tile"] == "128x64"
    monkeypatch.setenv("NCX_CFG_9", "7")
    assert _lib.plan_query(d, "DWL")["tile"] == base["tile"]
