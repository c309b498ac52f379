"""CPU: what tests/main_bwd_ref.py claims -- the restatement's parts, summed, are orc.loss_and_grads in float64; the yardstick constants
(the source of the kernels' bound) reproduce and match profiles/main_bwd_edges.json; every case is a shape the library accepts and routes
as its id says; and the harness fails on five subtly wrong kernels, emulated in numpy from correct float32 inputs."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import main_bwd_ref as Bw
import main_fwd_ref as R
from conftest import ROOT
from helpers import ZERO_GRAD_FLOOR, ZERO_GRAD_TENSORS
from oracle import ncx_oracle as orc

PROFILE = os.path.join(ROOT, "profiles", "main_bwd_edges.json")


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("L", [1, 2, 3])
@pytest.mark.parametrize("lesion", [None, "no_a_emb", "no_v_mult", "all_off"])
@pytest.mark.parametrize("train", [False, True])
def test_restatement_summed_is_the_oracle_in_float64(lesion, L, train):
    """Every gradient within 1e-12 of its block's max (linear_1.weight: of each column block's own max)."""
    c = dict(R.BASE, L=L, H=13, lesion=lesion, drop=None, p=0.25 if train else 0.0)
    d, params, batch, spec, _ = R.build(c)
    masks = [torch.from_numpy((np.random.default_rng(l).random((c["B"] * d.K, d.H)) >= 0.25).astype(np.float32)) for l in range(L)] if train else None
    p64 = {k: v.double() for k, v in params.items()}
    b64 = {k: (v.double() if v.is_floating_point() else v) for k, v in batch.items()}
    _, _, want = orc.loss_and_grads(p64, d, b64, spec=spec, drop_p=c["p"], keep_masks=None if masks is None else [m.double() for m in masks])
    ref = Bw.MainBwdRef(R.MainFwdRef(params, d, batch, spec, c["p"], masks), params, batch)
    got = ref.whole(batch["gt"])
    assert set(got) == set(want)
    o, widths = d.offsets(), dict(v_orig=d.dv, v_other=d.dv, v_mult=d.dv, v_dist=1, v_rank=d.K, q_emb=d.dq, z_orig=d.dz, z_other=d.dz, a_emb_gt=d.da, a_emb_other=d.da)
    for k, w in want.items():
        w = w.numpy()
        blocks = [np.s_[:, o[n]: o[n] + wd] for n, wd in widths.items()] if k == "linear_1.weight" else [np.s_[...]]
        for sl in blocks:
            floor = ZERO_GRAD_FLOOR if k in ZERO_GRAD_TENSORS else 0.0          # (out.bias: zero in maths, both sides hold round-off of 1e-17)
            assert np.abs(got[k].reshape(w.shape)[sl] - w[sl]).max() <= 1e-12 * max(np.abs(w[sl]).max(), floor), (k, sl)
    if lesion in ("no_v_mult", "all_off"):
        assert (got["linear_1.weight"][:, o["v_mult"]: o["v_mult"] + d.dv] == 0).all()


def test_products_are_judged_alone():
    """from_dpre1 restates the products on the dpre_1 it is given: a bump in one element moves one row of every block by the bump's product."""
    c = dict(R.BASE, L=1, H=9, lesion=None, drop=None, p=0.0)
    d, params, batch, spec, _ = R.build(c)
    fwd = R.MainFwdRef(params, d, batch, spec)
    ref = Bw.MainBwdRef(fwd, params, batch)
    ref.whole(batch["gt"])
    g = ref.last_dpre1
    bump = np.zeros_like(g); bump[7, 4] = 0.5
    a, b = ref.from_dpre1(g), ref.from_dpre1(g + bump)
    for name, off, w in ref.cand_cols:
        delta = b[name][0] - a[name][0]
        assert np.abs(delta[4] - 0.5 * fwd.x[7, off: off + w]).max() <= 1e-13 and np.abs(np.delete(delta, 4, 0)).max() == 0, name
    assert abs((b["b1"][0] - a["b1"][0])[4] - 0.5) <= 1e-13


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
def test_table_covers_what_the_issue_lists():
    shape = lambda c: (c["B"], c["K"], c["H"], c["L"], c["dv"])
    fold8 = {shape(c) for c in Bw.CASES if c["fold"] == "fold8"}
    km = {shape(c) for c in Bw.CASES if c["fold"] == "km"}
    assert fold8 == {(1, 24, 256, 1, 64), (7, 24, 256, 2, 128), (13, 48, 256, 1, 192), (37, 24, 512, 1, 64)}
    assert km == {(1, 24, 16, 1, 70), (7, 24, 20, 2, 64), (13, 48, 48, 1, 130), (40, 24, 200, 1, 96)}
    for c in Bw.CASES:
        if c["fold"] != "grouped":
            assert (c["dq"], c["dz"], c["A"], c["env"]) == (50, 18, 45, {"NCX_KM_FORCE": "1"})
    tn = [c for c in Bw.CASES if c["tn"] == "tn8"]
    assert all((c["dv"], c["dq"], c["dz"]) == (96, 64, 24) for c in tn)
    assert {(c["B"], c["H"], c["L"], c["K"]) for c in tn} >= {(128, 256, 1, 24), (160, 256, 1, 24), (128, 512, 2, 24), (128, 256, 1, 48)}
    assert {c["lesion"] for c in tn} == {None, "no_a_emb", "no_v_mult"} and {c["drop"] for c in tn} == {None, "rng"}
    assert {c["A"] for c in Bw.CASES if c["dv"] == 96} >= {33, 36, 40, 200}
    gemm = [c for c in Bw.CASES if (c["fold"], c["tn"]) == ("grouped", "grouped")]
    assert {(c["B"], c["H"], c["L"]) for c in gemm} >= {(96, 256, 1), (7, 20, 2), (33, 96, 2), (44, 128, 2)}
    assert {c["env"].get("NCX_SPLIT_4") for c in gemm} >= {"3", "8"} and {c["emb_nt"] for c in gemm} == {True, False}
    for c in Bw.CASES:                                   # every case carries a duplicated answer id, and the id names the route
        assert c["id"].startswith("%s-%s-" % (c["fold"], c["tn"]))
        if c["B"] > 1:
            aid = Bw.build(c)[2]["answer_aids"]
            assert aid[0] == aid[c["B"] - 1]
    assert Bw.PLANTED["B"] * Bw.PLANTED["K"] == 312


@pytest.mark.parametrize("form", ["fp32", "x6"])
@pytest.mark.parametrize("case", Bw.CASES, ids=lambda c: c["id"])
def test_case_is_accepted_and_routes_as_its_id_says(case, form, monkeypatch):
    """The planner's answer on this host (the weight-gradient predicates do not ask for the device); the GPU file asserts it again there."""
    from neuralcx import _lib, ops
    c = case
    if c["env"]:
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        for k, v in c["env"].items():
            monkeypatch.setenv(k, v)
    spec = dict(orc.DEFAULT_SPEC, **R.LESIONS[c["lesion"]]) if c["lesion"] else None
    n = _lib.NcxDims()
    n.B, n.K, n.dv, n.dq, n.dz, n.da, n.A, n.H, n.L = (c[k] for k in ("B", "K", "dv", "dq", "dz", "da", "A", "H", "L"))
    n.n_img = c["B"] * (c["K"] + 1)
    x6 = form == "x6"
    n.flags = ops.flags_from_spec(spec) | (_lib.NCX_F_X6 if x6 else 0)
    assert _lib.lib().ncx_workspace_bytes(ctypes.byref(n)) > 0
    r = _lib.plan_query(n, "DW1_ROUTE")
    assert r["fold"] == {"fold8": "k_dw_km_x6" if x6 else "k_dw_km8", "km": "k_dw_km", "grouped": "grouped"}[c["fold"]], r
    assert r["tn"] == {"tn8": "k_dw_tn8_x6" if x6 else "k_dw_tn8", "grouped": "grouped"}[c["tn"]], r
    off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert _lib.lib().ncx_ws_region(ctypes.byref(n), 7, ctypes.byref(off), ctypes.byref(nb)) == 0          # NCX_WS_DPRE2
    assert nb.value == (c["B"] * c["K"] * c["H"] * 4 if c["L"] == 2 else 0)
    o1, n1 = ctypes.c_size_t(0), ctypes.c_size_t(0)
    assert _lib.lib().ncx_ws_region(ctypes.byref(n), 3, ctypes.byref(o1), ctypes.byref(n1)) == 0           # NCX_WS_DPRE1
    assert c["L"] != 2 or abs(o1.value - off.value) >= nb.value                                             # two buffers, side by side


# ---- the yardstick -----------------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def _measured():
    if not _MEASURED:
        seen = set()
        for c in Bw.CASES:
            if Bw.shape_key(c) not in seen:
                seen.add(Bw.shape_key(c))
                for g, (t, r) in Bw.yardstick(c).items():
                    old = _MEASURED.get(g, (0.0, 0.0))
                    _MEASURED[g] = (max(old[0], t), max(old[1], r))
    return _MEASURED


@pytest.mark.parametrize("group", Bw.GROUPS)
def test_recorded_yardsticks_reproduce(group):
    """YARDSTICK is the larger of the two CPU ratios, rounded up, on the host that wrote the profile.  The row-order figure is plain numpy
    float32 and does not move; torch's comes from its BLAS, which blocks by the CPU it finds: the constant must be of the measured size,
    within a factor of three either way.  The kernels' c = 4 x the constant does not move with the host, and stays under the length of
    every long reduction of the table (for the short ones the test applies n + 2, which is tighter)."""
    t, r = _measured()[group]
    const = Bw.YARDSTICK[group]
    print("yardstick group %s torch32 %.3f row order %.3f constant %.3f c %.3f" % (group, t, r, const, Bw.C_MARGIN * const))
    assert const / 3.0 <= max(t, r) <= 3.0 * const, (group, t, r, const)
    prof = json.load(open(PROFILE))["groups"][group]
    assert prof["constant"] == const and prof["c"] == Bw.C_MARGIN * const
    assert prof["torch32_ratio"] / 3.0 <= t <= 3.0 * prof["torch32_ratio"] and prof["row_order_ratio"] / 3.0 <= r <= 3.0 * prof["row_order_ratio"]
    for form in ("hip_fp32_max_ratio", "hip_x6_max_ratio"):
        assert prof[form] is None or prof[form] <= prof["c"]
    assert Bw.C_MARGIN * const < 128                      # the shortest reduction of the TN cases: B = 128 rows of dSh x K


# ---- planted errors ----------------------------------------------------------------------------------------------------------------------
def _planted(case):
    """Correct float32 inputs of product a .. c at the planted shape: dpre_1, the candidate row in float32, the references."""
    d, params, batch, spec, masks = Bw.build(case)
    fwd = R.MainFwdRef(params, d, batch, spec, case["p"], masks)
    ref = Bw.MainBwdRef(fwd, params, batch)
    ref.whole(batch["gt"])
    dpre = Bw.f32(ref.last_dpre1)
    xc, _ = Bw.operands32(fwd, batch)
    cols = {name: np.s_[:, o: o + w] for name, o, w in ref.cand_cols}
    return d, batch, dpre, xc, cols, ref.from_dpre1(dpre)


def _over(name, got, prod):
    r, S, extra, n = prod
    return Bw.ratio(got, r, S, extra), Bw.bound_c(name, n)


def _bf16(a):
    return torch.from_numpy(np.ascontiguousarray(a, np.float32)).bfloat16().float().numpy()


def test_planted_errors_break_the_bound():
    """M = 312 (B = 13, K = 24, H = 256, dv = 64, dz = 18, A = 45: main_bwd_ref.PLANTED).  The correct float32 product passes; each wrong one
    breaks the bound of its product -- the lost plane breaks the fp32-grade rule, which is what holds the X6 forms to more than c."""
    d, batch, dpre, xc, cols, parts = _planted(Bw.PLANTED)
    assert dpre.shape[0] == 312 and np.abs(dpre[-1]).max() > 0
    good = {n: Bw.torch32(dpre, xc[cols[n]]) for n in ("v_other", "z_other")}
    for n, g in good.items():
        r, c = _over(n, g, parts[n])
        assert r <= c, (n, r, c)
    # 1. one reduction row dropped from product a (the last row: what a ragged tile would lose)
    r, c = _over("v_other", Bw.torch32(dpre[:-1], xc[:-1][cols["v_other"]]), parts["v_other"])
    assert r > c, ("dropped row", r, c)
    # 2. one operand of product c rounded to bf16
    r, c = _over("z_other", Bw.torch32(dpre, _bf16(xc[cols["z_other"]])), parts["z_other"])
    assert r > c, ("bf16 operand", r, c)
    # 3. the third bf16 plane of one operand dropped from a three-plane product: v_k = p1 + p2 + p3, the p3 products missing, everything
    #    else exact.  Within c (it is fp32-sized, about 2^-17 per term), over the fp32-grade rule against the correct float32 product.
    x = xc[cols["v_other"]]
    p1 = _bf16(x); p2 = _bf16(x - p1)
    lost = (dpre.astype(np.float64).T @ (p1.astype(np.float64) + p2)).astype(np.float32)
    r, c = _over("v_other", lost, parts["v_other"])
    r32, _ = _over("v_other", good["v_other"], parts["v_other"])
    print("lost plane: ratio %.2f, correct float32 %.2f, c %.1f" % (r, r32, c))
    assert not Bw.x6_rule(r, r32), ("lost plane", r, r32)
    # 4. one 64-row k-step added twice
    r, c = _over("z_other", good["z_other"] + Bw.torch32(dpre[64:128], xc[64:128][cols["z_other"]]), parts["z_other"])
    assert r > c, ("k-step twice", r, c)


def test_planted_distance_without_its_epsilon_breaks_the_bound():
    """5. the dist column taken as ||v_o - v_k|| without the 1e-6.  On the table's random features the 1e-6 moves a distance of ~3 by a few
    2^-24 of random sign, which a sum over rows hides from ANY rounding-level bound; it shows where the neighbours nearly equal the original
    (v_k = v_o + 5e-4 N(0, 1): PLANTED_NEARDUP, and one TN case of the GPU table), so that is where it is planted.  The correct float32
    distance passes there, derived term included."""
    d, batch, dpre, xc, cols, parts = _planted(Bw.PLANTED_NEARDUP)
    r, c = _over("v_dist", Bw.torch32(dpre, xc[cols["v_dist"]]), parts["v_dist"])
    assert r <= c, (r, c)
    f = batch["image_features"].float()
    wrong = torch.linalg.vector_norm(f[:, :1] - f[:, 1:], dim=-1).reshape(-1, 1).numpy()
    r, c = _over("v_dist", Bw.torch32(dpre, wrong), parts["v_dist"])
    print("distance without 1e-6: ratio %.1f beyond the derived term, c %.1f" % (r, c))
    assert r > c, (r, c)
