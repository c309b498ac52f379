"""CPU: what tests/producers_ref.py claims -- the case table covers the constants of the frozen producers' kernels, the fp64 restatement
chained end to end is oracle.mutan_vqa_forward / mlb_ref.mlb_vqa_forward, the float32 ratios behind every c reproduce, and the route
entries (ncx_vqa_route / ncx_mlb_route: host only, nothing is launched) answer as the table expects."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import producers_ref as P
from conftest import ROOT
from mlb_ref import mlb_vqa_forward
from oracle import ncx_oracle as orc

PROFILE = os.path.join(ROOT, "profiles", "producer_edges.json")
MUTAN = [c for c in P.CASES if c["kind"] == "mutan"]
MLB = [c for c in P.CASES if c["kind"] == "mlb"]


def test_table_covers_what_the_issue_lists():
    shape = lambda c: (c["B"], c["K1"], c["dv"], c["dq"], c["dhv"], c["dhq"], c["dz"], c["R"], c["A"])
    fold, engine = [c for c in MUTAN if c["group"] == "fold"], [c for c in MUTAN if c["group"] == "engine"]
    assert {shape(c) for c in fold} == {(1, 2, 64, 8, 4, 4, 4, 1, 4), (8, 4, 64, 20, 32, 12, 32, 2, 8), (9, 32, 96, 48, 36, 20, 36, 10, 40),
                                       (65, 25, 96, 48, 68, 20, 100, 3, 52), (13, 25, 96, 48, 64, 20, 37, 4, 42)}
    assert {shape(c) for c in engine} == {(5, 33, 96, 48, 28, 20, 44, 4, 52), (3, 49, 96, 48, 40, 20, 70, 10, 40), (13, 25, 96, 48, 30, 20, 44, 1, 52),
                                         (65, 25, 96, 48, 68, 20, 100, 3, 52)}
    assert all(c["route"]["fold_kernel"] for c in fold) and not any(c["route"]["fold_kernel"] for c in engine)
    assert any(c["act"] is None for c in fold)
    assert {c["K1"] for c in MUTAN} >= {2, 4, 25, 32, 33, 49} and {c["K1"] for c in MLB} >= {2, 4, 25, 32, 33, 49}
    assert {c["ksteps"] % 2 for c in fold} == {0, 1} and {c["ksteps"] for c in fold} >= {1, 2, 3}
    assert any(c["dhv"] == 4 for c in fold) and any(c["dz"] % 4 for c in fold) and any(c["dhv"] % 4 for c in engine) and any(c["B"] == 1 for c in fold)
    hook = P.BY_ID["engine-nine-groups-hook"]
    assert hook["env"] == {"NCX_NO_MUTAN_FOLD": "1"} and P.shape_key(hook) == P.shape_key(P.BY_ID["fold-nine-groups"])
    for cases in (MUTAN, MLB):
        assert {c["route"]["main_v"] for c in cases} == {True, False}
        assert {c["route"]["classifier"] for c in cases} == {"generic", "main", "main_padded"}
        assert {c["a_orig"] for c in cases} == {True, False}
    assert {c["dv"] for c in MUTAN if c["route"]["main_v"]} >= {64, 96} and {c["dv"] for c in MUTAN if not c["route"]["main_v"]} >= {32, 70, 72, 2048}
    # both x_v routes in front of both fusions
    assert {(c["route"]["main_v"], c["route"]["fold_kernel"]) for c in MUTAN} == {(True, True), (True, False), (False, True), (False, False)}
    assert {(c["K1"], c["dv"], c["A"]) for c in MLB} >= {(k, dv, A) for k in (2, 4, 32, 33, 49) for dv in (96, 72) for A in (40, 42)}
    assert {c["act_c"] for c in MLB} == {None, "tanh"} and any(c["act"] is None for c in MLB) and any(c["B"] == 1 for c in MLB)
    wide = P.BY_ID["mlb-tiles-96x128"]
    assert (wide["B"], wide["K1"], wide["dv"], wide["dq"], wide["dz"], wide["A"], wide["act_c"]) == (89, 25, 64, 48, 1240, 40, "tanh")
    assert wide["cu_dependent"] and wide["route"]["v_tile"] == "96x128" and {c["route"]["v_tile"] for c in MLB} == {None, "48x128", "96x128"}
    big = P.BY_ID["big-table-beyond-4GiB"]
    off = big["ids"].astype(np.int64) * big["dv"] * 4
    assert big["n_img"] == 525000 and big["dv"] == 2048 and (big["B"], big["K1"]) == (2, 4) and not big["route"]["main_v"]
    assert ((off > 2 ** 30) & (off < 2 ** 31)).any() and ((off > 2 ** 31) & (off < 2 ** 32)).any() and (off > 2 ** 32).any()
    assert big["ids"].max() == big["n_img"] - 1 and big["n_img"] * big["dv"] * 4 > 2 ** 32


@pytest.mark.parametrize("case", [c for c in P.CASES if c["B"] * c["K1"] * c["dz"] <= 200000], ids=lambda c: c["id"])
def test_inputs_are_as_the_issue_asks(case):
    state, table, idx, q_emb = P.build(case)
    B, K1 = case["B"], case["K1"]
    assert idx.shape == (B, K1) and idx.min() >= 0 and idx.max() < table.shape[0] and float(table.min()) >= 0
    assert len(set(idx[0])) < K1                                                   # an image twice inside a question
    if B > 1:
        assert set(idx[0]) & set(idx[B - 1])                                       # an image in two questions
    if case["ids"] is None:
        assert table.shape[0] > B * K1 and not np.array_equal(idx.reshape(-1), np.arange(B * K1))
        # tanh stays off saturation: no pre-activation beyond 3 (|tanh| < 0.9951)
        if case["act"] == "tanh":
            ref = (P.MutanRef if case["kind"] == "mutan" else P.MlbRef)(state, case)
            v_rows = table[torch.from_numpy(idx.reshape(-1).astype(np.int64))]
            assert np.abs(ref.xv(v_rows)[0]).max() < 0.9951 and np.abs(ref.xq(q_emb)[0]).max() < 0.9951


@pytest.mark.parametrize("case", [c for c in P.CASES if c["B"] * c["K1"] * c["dz"] <= 200000], ids=lambda c: c["id"])
def test_restatement_chained_is_the_oracle_in_float64(case):
    state, table, idx, q_emb = P.build(case)
    v_rows = table[torch.from_numpy(idx.reshape(-1).astype(np.int64))]
    B, K1 = case["B"], case["K1"]
    if case["kind"] == "mutan":
        got = P.MutanRef(state, case).chain(v_rows, q_emb)
        s64 = {k: v.double() for k, v in state.items()}
        if case["act"] == "tanh":
            want = orc.mutan_vqa_forward(s64, v_rows.double().reshape(B, K1, -1), q_emb.double(), R=case["R"])
        else:                                                                      # (the oracle writes tanh: the same operations without it)
            x = P.mutan_float32(s64, v_rows.double(), q_emb.double(), case["R"], None)
            a, z = x["a"].reshape(B, K1, -1), x["z"].reshape(B, K1, -1)
            want = (a[:, 0], z[:, 0], a[:, 1:], z[:, 1:])
        want = [w.numpy() for w in want]
    else:
        got = P.MlbRef(state, case).chain(v_rows, q_emb)
        want = mlb_vqa_forward({k: v.numpy() for k, v in state.items()}, table.numpy(), idx, q_emb.numpy(), act_v=case["act"], act_q=case["act"],
                               act_c=case["act_c"])
    for g, w, name in zip(got, want, ("a_orig", "z_orig", "a_knns", "z_knns")):
        assert g.shape == w.shape and np.abs(g - w).max() <= 1e-12 * max(1.0, np.abs(w).max()), (case["id"], name)


def test_stages_are_judged_alone_and_S_bounds_the_terms():
    c = P.BY_ID["fold-K1-32-no-padding"]
    state, table, idx, q_emb = P.build(c)
    ref = P.MutanRef(state, c)
    v_rows = table[torch.from_numpy(idx.reshape(-1).astype(np.int64))]
    xq, xv = ref.xq(q_emb)[0], ref.xv(v_rows)[0]
    hq = ref.hq(xq)[0]
    z, S = ref.z(xv, hq)
    assert (np.abs(z) <= S * (1 + 1e-12)).all()
    bump = np.zeros_like(hq); bump[2, 5] = 0.25                                   # rank 0, column 5 of question 2: moves z[rows of question 2, 5] only
    dz_ = ref.z(xv, hq + bump)[0] - z
    rows = np.arange(2 * c["K1"], 3 * c["K1"])
    hv = xv[rows] @ ref.Whv[0, 5] + ref.bhv[0, 5]
    assert np.abs(dz_[rows, 5] - 0.25 * hv).max() <= 1e-14
    dz_[rows, 5] = 0
    assert np.abs(dz_).max() == 0


@pytest.mark.parametrize("case", P.CASES, ids=lambda c: c["id"])
def test_route_entries_answer_as_the_table_expects(case, monkeypatch):
    """ncx_vqa_route / ncx_mlb_route on the case's dims (no device: 256 CUs assumed, which is what the CU-dependent case is placed for)."""
    from neuralcx import _lib
    monkeypatch.delenv("NCX_EXPERIMENT", raising=False)
    for k, v in case["env"].items():
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        monkeypatch.setenv(k, v)
    got = P.query_route(case)
    assert {k: got[k] for k in case["route"]} == case["route"], (case["id"], got)
    d, m = P.c_dims_and_params(case)
    size = getattr(_lib.lib(), "ncx_vqa_workspace_bytes" if case["kind"] == "mutan" else "ncx_mlb_workspace_bytes")(ctypes.byref(d), ctypes.byref(m))
    assert size > 0
    # the regions lie inside the workspace; a tensor the route does not store is refused
    sym, ids = ("ncx_vqa_ws_region", _lib.NCX_VQA_WS) if case["kind"] == "mutan" else ("ncx_mlb_ws_region", _lib.NCX_MLB_WS)
    B, K1, dz = case["B"], case["K1"], case["dz"]
    want = dict(xq=B * (case.get("dhq") or dz), hq=B * (case.get("R") or 0) * dz, xv=B * K1 * (case.get("dhv") or dz), t_knns=B * (K1 - 1) * dz, t_orig=B * dz)
    stored = set(ids) if case["kind"] == "mutan" else {"xq"} | ({"t_knns", "t_orig"} if case["act_c"] else set()) | (set() if got["main_v"] else {"xv"})
    spans = []
    for name, which in ids.items():
        off, nb = ctypes.c_size_t(), ctypes.c_size_t()
        rc = getattr(_lib.lib(), sym)(ctypes.byref(d), ctypes.byref(m), which, ctypes.byref(off), ctypes.byref(nb))
        assert rc == (0 if name in stored else -4), (case["id"], name, rc)
        if rc == 0:
            assert nb.value == 4 * want[name] and off.value % 256 == 0 and off.value + nb.value <= size
            spans.append((off.value, off.value + nb.value))
    spans.sort()
    assert all(a[1] <= b[0] for a, b in zip(spans, spans[1:]))


def test_route_hooks_and_guards(monkeypatch):
    """The hooks move the routes; the extents the fused kernel addresses with 32-bit offsets keep a shape off it; check_mutan has
    check_mlb's integer-range rule."""
    from neuralcx import _lib
    monkeypatch.delenv("NCX_EXPERIMENT", raising=False)
    c = dict(P.BY_ID["fold-K1-32-no-padding"])
    assert P.query_route(c) == dict(main_v=True, fold_kernel=True, classifier="main_padded", v_tile="48x128")
    for n_img, main_v in ((11184639, True), (11184640, False)):                   # 96 x 4 bytes a row: the first table at 2^32 - 65536 bytes
        assert P.query_route(dict(c, n_img=n_img))["main_v"] == main_v
    m = dict(P.BY_ID["mlb-K1-4-dv96-A40"])
    for n_img, main_v in ((11184639, True), (11184640, False)):
        assert P.query_route(dict(m, n_img=n_img))["main_v"] == main_v
    # z_knns of 4 GiB: the classifier leaves the fused kernel (B K dz 4 bytes), for both producers
    for case in (c, m):
        wide = dict(case, B=2 ** 20, K1=33, dz=36)
        assert P.query_route(dict(wide, B=2 ** 19))["classifier"] == "main_padded" and P.query_route(wide)["classifier"] == "generic"
    # B (K + 1) max(dz, A) >= 2^31: NCX_E_DIMS, no workspace
    for kind, sym in ((c, "ncx_vqa_workspace_bytes"), (m, "ncx_mlb_workspace_bytes")):
        for B, ok in ((2 ** 31 // (33 * 40) , True), (2 ** 31 // (33 * 40) + 1, False)):
            d, p = P.c_dims_and_params(dict(kind, B=B, K1=33, dz=36, A=40))
            assert (getattr(_lib.lib(), sym)(ctypes.byref(d), ctypes.byref(p)) > 0) == ok, (sym, B)
            out = (ctypes.c_int32 * 4)()
            assert getattr(_lib.lib(), sym.replace("workspace_bytes", "route"))(ctypes.byref(d), ctypes.byref(p), out) == (0 if ok else -2)
    monkeypatch.setenv("NCX_EXPERIMENT", "1")
    monkeypatch.setenv("NCX_VQA_NO_MAIN", "1")
    assert P.query_route(c) == dict(main_v=False, fold_kernel=True, classifier="generic", v_tile=None)
    assert P.query_route(m)["main_v"] is False and P.query_route(m)["classifier"] == "generic"
    monkeypatch.delenv("NCX_VQA_NO_MAIN")
    monkeypatch.setenv("NCX_NO_MUTAN_FOLD", "1")
    assert P.query_route(c) == dict(main_v=True, fold_kernel=False, classifier="main_padded", v_tile="48x128")


def test_benchmark_shapes_keep_their_routes():
    """The producers at the benchmark's widths (configs[2]: B = 512, K = 24, dv = 2048, dq = 2400; Mutan dim_hv = dim_mm = 360, R = 10; MLB dim_h =
    1200; 2000 answers; the VQA2 table of 82 783 images): fused x_v (Mutan on the 160-row tile), the fold kernel, the fused classifier."""
    mutan = dict(kind="mutan", B=512, K1=25, dv=2048, dq=2400, dhv=360, dhq=360, dz=360, R=10, A=2000, act="tanh", act_c=None, n_img=82783)
    assert P.query_route(mutan) == dict(main_v=True, fold_kernel=True, classifier="main_padded", v_tile="160x128")
    mlb = dict(kind="mlb", B=512, K1=25, dv=2048, dq=2400, dz=1200, A=2000, act="tanh", act_c=None, n_img=82783)
    assert P.query_route(mlb) == dict(main_v=True, v_tile="96x128", classifier="main_padded", t_stored=False)


def _measured(group):
    seen, worst = set(), 0.0
    for c in P.CASES:
        if c["group"] == group and P.shape_key(c) not in seen:
            seen.add(P.shape_key(c))
            worst = max(worst, P.oracle32_ratio(c))
    return worst


@pytest.mark.parametrize("group", P.GROUPS)
def test_recorded_oracle32_ratios_reproduce(group):
    """ORACLE32_RATIO is the float32 restatement's ratio on the machine that wrote profiles/producer_edges.json, rounded up.  It stays at
    or below the constant here; and since another host's BLAS sums these small products in another order, the constant must also be of
    the measured size (within a factor of three), not a loose one.  The kernels' c = 4 x the constant does not move with the host."""
    got = _measured(group)
    const = P.ORACLE32_RATIO[group]
    print("oracle32 ratio group %s measured %.3f constant %.3f c %.3f" % (group, got, const, P.bound_c(group)))
    assert const / 3.0 <= got <= const, (group, got, const)
    prof = json.load(open(PROFILE))["groups"][group]
    assert prof["oracle32_ratio_constant"] == const and prof["c"] == P.bound_c(group)
    assert prof["gpu_max_ratio"] is None or prof["gpu_max_ratio"] <= prof["c"]
