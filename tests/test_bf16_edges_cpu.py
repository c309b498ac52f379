"""CPU: what tests/bf16_ref.py claims -- its bf16 rounding is torch.bfloat16's; fed the oracle's own operands its products are the oracle's
(orc.forward_bf16, orc.loss_and_grads_bf16) to fp32 rounding, and those operands pass its operand checks; every case meets the two ambiguity
caps, is accepted by the library and routed as the table says; the recorded yardsticks and tau_soft reproduce and match
profiles/bf16_edges.json; the table covers the listed values; and the harness rejects four subtly wrong kernels, emulated in numpy."""
import ctypes
import json
import os

import numpy as np
import pytest
import torch

import bf16_ref as F
from conftest import ROOT
from oracle import ncx_oracle as orc

PROFILE = os.path.join(ROOT, "profiles", "bf16_edges.json")


# ---- rounding ----------------------------------------------------------------------------------------------------------------------------
def _torch_bits(x32):
    return torch.from_numpy(np.ascontiguousarray(x32, np.float32)).bfloat16().view(torch.int16).numpy().view(np.uint16)


def test_rne_helper_is_torch_bfloat16():
    rng = np.random.default_rng(0)
    rand = (rng.standard_normal(20000) * np.exp(rng.uniform(-80, 80, 20000))).astype(np.float32)
    # ties: every bf16 pattern of a few exponents, plus exactly half a bf16 ulp (low 16 bits 0x8000), and its float32 neighbours
    hi = np.concatenate([np.arange(0x3F00, 0x4100), np.arange(0x0000, 0x0200), np.arange(0x7E80, 0x7F80), np.arange(0xBF00, 0xC000)]).astype(np.uint32) << 16
    ties = np.concatenate([(hi | lo).astype(np.uint32) for lo in (0x8000, 0x7FFF, 0x8001, 0x0000, 0x0001, 0xFFFF)]).view(np.float32)
    special = np.array([0.0, -0.0, 1.0, -1.0, 2.0 ** -126, 2.0 ** -133, 2.0 ** -134, -2.0 ** -134, 1.5 * 2.0 ** -133, 2.0 ** -149, 3.3e38, 3.4e38], np.float32)
    for x in (rand, ties, special):
        x = x[np.isfinite(x)]
        assert np.array_equal(F.rne_bits(x), _torch_bits(x))
    assert F.rne_bits(np.float32(-0.0)) == 0x8000 and F.rne_bits(0.0) == 0
    assert np.array_equal(F.bf_val(F.rne_bits(rand)), torch.from_numpy(rand).bfloat16().double().numpy())
    # one rounding from float64: a value that float32 would first round onto a bf16 tie goes the right way
    x = 1.0 + 2.0 ** -8 + 2.0 ** -40                     # just above the tie between 1 and 1 + 2^-7
    assert F.rne_bits(x) == 0x3F81 and F.rne_bits(np.float32(x)) == 0x3F80


# ---- the restatement against the oracle --------------------------------------------------------------------------------------------------
def _oracle_with_its_operands(case):
    """orc.loss_and_grads_bf16 with orc._bf wrapped so that every tensor it rounds is recorded, in call order."""
    d, params, batch, masks = F.build(case)
    seen, real = [], orc._bf

    def spy(x):
        seen.append(x.detach().clone())
        return real(x)
    orc._bf = spy
    try:
        taps = {}
        with F.one_thread():
            orc.forward_bf16(params, d, *[batch[k] for k in F.R.FEATS], drop_p=case["p"], keep_masks=masks, taps=taps)
            n_fwd = len(seen)
            _, _, grads = orc.loss_and_grads_bf16(params, d, batch, drop_p=case["p"], keep_masks=masks)
    finally:
        orc._bf = real
    fwd, bwd = seen[:n_fwd], seen[2 * n_fwd:]
    assert len(fwd) == 4 and [tuple(t.shape) for t in fwd[:2]] == [(d.H, d.da), (d.A, d.da)] and fwd[3].shape == (d.H, fwd[2].shape[1])
    xc32, wc32 = fwd[2].numpy(), fwd[3].numpy()
    dpre1 = bwd[0].numpy()
    assert dpre1.shape == (xc32.shape[0], d.H) and d.A != d.da
    rest = bwd[1:]
    # _Bf16GtProduct.backward rounds dGt [H, A] alone; _SharedAnswerEmbedding.backward rounds dGgt [H, A] and then W1agt [H, da]
    i = [j for j, t in enumerate(rest) if tuple(t.shape) == (d.H, d.da)][0]
    dggt = rest[i - 1].numpy()
    dgt = [t for j, t in enumerate(rest) if tuple(t.shape) == (d.H, d.A) and j != i - 1][0].numpy()
    return d, params, batch, masks, taps, grads, xc32, wc32, dpre1, dgt, dggt


@pytest.mark.parametrize("case_id", ["base", "K7", "dv70", "A45", "H130", "L2-masks"])
def test_restatement_on_the_oracles_operands_is_the_oracle(case_id):
    """The oracle's own float32 operands (torch's softmax and norm, its float32 Gt, dpre_1 and dGt | dGgt) pass the operand checks -- the
    two-sided ones included: another float32 evaluation inside tau -- and each product restated from them is the oracle's to fp32 rounding:
    within the product's own bound, which is what a float32 sum of the same exact products must meet in any order."""
    case = F.BY_ID[case_id]
    d, params, batch, masks, taps, grads, xc32, wc32, dpre1, dgt, dggt = _oracle_with_its_operands(case)
    ref = F.Bf16Ref(params, d, batch, F.layout_of(case), case["p"], masks)
    L = ref.lay
    # the oracle's operands in the packed layout
    xc = np.zeros((ref.M, L["kc"]), np.uint16)
    wc = np.zeros((L["Hp"], L["kc"]), np.uint16)
    o = 0
    for c0, w in ((L["c_vk"], d.dv), (L["c_vm"], d.dv), (L["c_misc"], d.K + 1), (L["c_z"], d.dz), (L["c_p"], d.A)):
        xc[:, c0: c0 + w] = F.rne_bits(xc32[:, o: o + w])
        wc[:d.H, c0: c0 + w] = F.rne_bits(wc32[:, o: o + w])
        o += w
    assert o == xc32.shape[1]
    gt32 = wc32[:, -d.A:]
    two_sided = ref.check_xc(xc)
    ref.check_wc(wc, gt32)
    assert two_sided <= F.SOFT_AMBIGUOUS_CAP * ref.M * d.A

    def same(name, got, prod):
        r, over, c = F.judge(name, got, prod)
        assert over.size == 0, (case_id, name, r, c)

    same("Gt", gt32, ref.gt())
    pre = ref.h1(xc, wc, want_pre=True)
    _, S, _, n = ref.h1(xc, wc)
    S = S * (1.0 - ref.fwd.p) if masks is not None else S
    assert (np.abs(taps["pre1"].reshape(ref.M, d.H).numpy() - pre) <= F.U24 * F.bound_c("h1", n) * S).all()
    w1 = grads["linear_1.weight"].numpy()
    parts = ref.dwc(dpre1, xc)
    for name, c0, o0, w in ref.segments:
        same(name, w1[:, o0: o0 + w], parts[name])
    same("dGt", dgt, parts["dGt"])
    blk = ref.from_block(dgt, dggt)
    oa = d.offsets()["a_emb_other"]
    same("a_other", w1[:, oa: oa + d.da], blk["a_other"])
    same("dE", grads["answer_embedding.weight"].numpy(), blk["dE"])
    # the fp32 products the variant keeps, from the same dpre_1 (main_bwd_ref's, unchanged)
    fp32 = ref.bwd.from_dpre1(dpre1)
    for name, off, w in ref.bwd.shared_cols:
        o0 = d.offsets()[name]
        same(name, w1[:, o0: o0 + w], fp32[name])
    same("dGgt", dggt, fp32["dGgt"])
    same("b1", grads["linear_1.bias"].numpy(), fp32["b1"])


def test_products_are_judged_alone():
    """dwc restates the product on the operands it is given: one bf16 ulp on one element of Xc moves one column of the result, by dpre's
    column times the step."""
    case = F.BY_ID["base"]
    ref, xc, wc, dpre1, dgt, dggt = F.ideal(case)
    r, c = 7, ref.lay["c_z"] + 3
    xc2 = xc.copy(); xc2[r, c] += 1
    a, b = ref.dwc(dpre1, xc), ref.dwc(dpre1, xc2)
    step = F.bf_val(xc2[r, c]) - F.bf_val(xc[r, c])
    delta = b["z_other"][0] - a["z_other"][0]
    assert np.abs(delta[:, 3] - F.bfr(dpre1)[r] * step).max() <= 1e-15 and np.abs(np.delete(delta, 3, 1)).max() == 0
    for name in ("v_other", "v_mult", "v_dist", "v_rank", "dGt"):
        assert np.array_equal(a[name][0], b[name][0])


# ---- the case table ----------------------------------------------------------------------------------------------------------------------
def test_case_table_covers_the_listed_values():
    one_off = [c for c in F.CASES if not c["env"]]
    for key in ("dv", "K", "dz", "A", "da", "H", "L"):
        assert {c[key] for c in one_off} >= set(F.LISTED[key]), key
    assert {c["M"] for c in F.CASES} >= set(F.LISTED["M"])
    assert {c["H"] for c in one_off} & {257, 260}
    lay = {c["id"]: F.layout_of(c) for c in F.CASES}
    assert lay["base"]["raw"] == 156 and lay["base"]["kc"] == 256 and lay["base"]["Hp"] == 128
    raws = {l["raw"] for l in lay.values()}
    assert any(r < 128 for r in raws) and any(r % 128 == 0 for r in raws) and any(r % 128 == 1 for r in raws)
    assert {l["kc"] for l in lay.values()} >= {128, 256, 384} and {l["Hp"] for l in lay.values()} >= {128, 256, 384}
    assert any(l["Ap"] == c["A"] for c, l in ((F.BY_ID[i], l) for i, l in lay.items())) and any(l["dap"] == F.BY_ID[i]["da"] for i, l in lay.items())
    assert {(c["route"]["chunk"], c["route"]["nz"]) for c in F.CASES} >= {(64, 1), (64, 2), (64, 4), (64, 8), (128, 5)}
    assert F.BY_ID["M513"]["route"]["chunk"] == 128 and 513 - 4 * 128 == 1
    # the forms: every NT form and both TN kernels at each form shape, form 8 and tn8 only where Hp == 256; the 192-row kernel's rows
    for tag, shape in F.FORM_SHAPES:
        forms = {(c["route"]["nt"], c["route"]["tn8"]) for c in F.CASES if c["id"].startswith("forms-%s-" % tag)}
        assert forms == {(nt, tn8) for nt in F.LISTED["nt"] for tn8 in (False, True)}
    for c in F.CASES:
        if c["route"]["nt"] == 8 or c["route"]["tn8"]:
            assert lay[c["id"]]["Hp"] == 256
    assert {c["M"] for c in F.CASES if c["route"]["nt"] == 8 and c["K"] == 3} == {189, 192, 195}
    assert {c["drop"] for c in F.CASES if c["L"] == 2} == {"masks", "rng"} and all(c["H"] % 4 for c in F.CASES if c["L"] == 2)
    wide = F.BY_ID["wide-dv2052-A2049"]
    assert (wide["dv"], wide["A"], wide["B"], wide["K"], wide["H"]) == (2052, 2049, 2, 3, 16)
    assert {c["route"]["vec_dpre"] for c in F.CASES} == {c["route"]["vec_dg"] for c in F.CASES} == {c["route"]["vec_w1a"] for c in F.CASES} == {False, True}


@pytest.mark.parametrize("case", F.CASES, ids=lambda c: c["id"])
def test_case_is_accepted_routed_and_within_the_ambiguity_caps(case, monkeypatch):
    """The library takes the shape; where the route does not depend on the CU count the planner answers on this host what the table states
    (without a device the planner assumes 256 CUs); no distance is ambiguous and at most 2 % of the softmax elements are."""
    from neuralcx import _lib
    if case["env"]:
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        for k, v in case["env"].items():
            monkeypatch.setenv(k, v)
    n = F.ncx_dims(case)
    assert _lib.lib().ncx_workspace_bytes(ctypes.byref(n)) > 0
    got = _lib.plan_query(n, "BF16_ROUTE")
    assert {k: got[k] for k in case["route"]} == case["route"], (case["id"], got)
    n.flags = _lib.NCX_F_ALL
    assert _lib.plan_query(n, "BF16_ROUTE") is None
    d, params, batch, masks = F.build(case)
    ref = F.Bf16Ref(params, d, batch, F.layout_of(case), case["p"], masks)
    dist, soft = ref.ambiguity()
    print("ambiguous %s dist %d softmax share %.5f" % (case["id"], dist, soft))
    assert dist == 0 and soft <= F.SOFT_AMBIGUOUS_CAP
    prof = json.load(open(PROFILE))
    assert abs(prof["ambiguous_softmax_share"][case["id"]] - soft) <= 1e-12


def test_regions_of_the_packed_operands():
    from neuralcx import _lib
    c = F.BY_ID["base"]
    n, lay = F.ncx_dims(c), F.layout_of(c)
    size = {}
    for which in (8, 9, 10):
        off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert _lib.lib().ncx_ws_region(ctypes.byref(n), which, ctypes.byref(off), ctypes.byref(nb)) == 0
        assert off.value % 256 == 0 and off.value + nb.value <= _lib.lib().ncx_workspace_bytes(ctypes.byref(n))
        size[which] = nb.value
    assert size == {8: c["M"] * lay["kc"] * 2, 9: lay["Hp"] * lay["kc"] * 2, 10: c["H"] * c["A"] * 4}
    n.flags = _lib.NCX_F_ALL
    for which, want in ((8, 0), (9, 0), (10, c["H"] * 64 * 4)):           # fp32 path: no packed operands; Gt's rows padded to 32 columns
        off, nb = ctypes.c_size_t(0), ctypes.c_size_t(0)
        assert _lib.lib().ncx_ws_region(ctypes.byref(n), which, ctypes.byref(off), ctypes.byref(nb)) == 0 and nb.value == want


# ---- the yardsticks ----------------------------------------------------------------------------------------------------------------------
_MEASURED = {}


def _measured():
    if not _MEASURED:
        seen, soft = set(), 0.0
        for c in F.CASES:
            if F.shape_key(c) not in seen:
                seen.add(F.shape_key(c))
                soft = max(soft, F.tau_soft_measure(c))
                for g, (t, r) in F.yardstick(c).items():
                    old = _MEASURED.get(g, (0.0, 0.0))
                    _MEASURED[g] = (max(old[0], t), max(old[1], r))
        _MEASURED["soft"] = soft
    return _MEASURED


@pytest.mark.parametrize("group", F.GROUPS)
def test_recorded_yardsticks_reproduce(group):
    """As test_main_bwd_edges_cpu.test_recorded_yardsticks_reproduce: the constant is of the measured size, within a factor of three either
    way (torch's figure moves with the host's BLAS, the row-order one does not); c = 4 x the constant does not move with the host."""
    t, r = _measured()[group]
    const = F.YARDSTICK[group]
    print("yardstick group %s torch32 %.3f row order %.3f constant %.3f c %.3f" % (group, t, r, const, F.C_MARGIN * const))
    assert const / 3.0 <= max(t, r) <= 3.0 * const, (group, t, r, const)
    prof = json.load(open(PROFILE))["groups"][group]
    assert prof["constant"] == const and prof["c"] == F.C_MARGIN * const
    assert prof["torch32_ratio"] / 3.0 <= t <= 3.0 * prof["torch32_ratio"] and prof["row_order_ratio"] / 3.0 <= r <= 3.0 * prof["row_order_ratio"]
    assert prof["hip_max_ratio"] is None or prof["hip_max_ratio"] <= prof["c"]


def test_recorded_tau_soft_reproduces():
    soft = _measured()["soft"]
    print("softmax32 worst relative deviation %.3f x 2^-24, recorded %.1f, tau_soft %.3g" % (soft, F.SOFT32_DEV_U24, F.TAU_SOFT))
    assert F.SOFT32_DEV_U24 / 3.0 <= soft <= F.SOFT32_DEV_U24
    prof = json.load(open(PROFILE))
    assert prof["softmax32_dev_u24"] == F.SOFT32_DEV_U24 and prof["tau_soft"] == F.TAU_SOFT == F.C_MARGIN * F.SOFT32_DEV_U24 * F.U24


# ---- the bound has teeth -----------------------------------------------------------------------------------------------------------------
def _rejected(name, got, prod):
    r, over, c = F.judge(name, got, prod)
    return over.size > 0


def _products_from(ref, xc, wc, dpre1, dgt, dggt):
    """{name: product} of the five groups from one set of operands."""
    out = {"Gt": ref.gt(), "h1": ref.h1(xc, wc)}
    out.update(ref.dwc(dpre1, xc))
    out.update(ref.from_block(dgt, dggt))
    return out


def test_the_bound_rejects_four_wrong_kernels():
    """At the base shape, from correct float32 results of the same exact bf16 products (torch float32: products32).  Each corruption is
    rejected on every group it applies to: p Gt, q h_1, r dWc (its six read-backs), s dW1[:, a_other], t dE."""
    case = F.BY_ID["base"]
    ref, xc, wc, dpre1, dgt, dggt = F.ideal(case)
    prods = F.products32(case)
    d, L = ref.d, ref.lay
    for name, (prod, g_t, g_r) in prods.items():
        assert not _rejected(name, g_t, prod) and not _rejected(name, g_r, prod), name
    X, W = F.bf_val(xc).astype(np.float32), F.bf_val(wc).astype(np.float32)[:d.H]
    g = F.bfr(dpre1).astype(np.float32)
    a, e = F.bfr(ref.w1ak).astype(np.float32), F.bfr(ref.E).astype(np.float32)
    gb = F.bfr(np.concatenate([dgt, dggt], 0)).astype(np.float32)
    wb = F.bfr(np.concatenate([ref.w1ak, ref.w1agt], 0)).astype(np.float32)
    shr = F.f32(np.repeat(ref.fwd.sh, d.K, axis=0))
    seg = {s[0]: np.s_[:, s[1]: s[1] + s[3]] for s in ref.segments}
    seg["dGt"] = np.s_[:, L["c_p"]: L["c_p"] + d.A]

    def results(X, W, g, a, e, gb, wb, drop=None):
        """The five groups' float32 results from the operands given; drop: one index of every reduction left out."""
        keep = lambda n, i=None: np.arange(n) if drop is None else np.delete(np.arange(n), drop % n if i is None else i)
        kq, kr, kp, ks, kt = keep(X.shape[1], L["c_vk"] + (drop or 0) % d.dv), keep(ref.M), keep(d.da), keep(d.A), keep(2 * d.H)       # (q: a v_k column)
        out = {"Gt": F.torch32(a[:, kp].T, e[:, kp].T), "h1": np.maximum(F.torch32(X[:, kq].T, W[:, kq].T) + shr, np.float32(0)),
               "a_other": F.torch32(gb[:d.H][:, ks].T, e[ks]), "dE": F.torch32(gb[kt], wb[kt])}
        dwc = F.torch32(g[kr], X[kr])
        out.update({n: dwc[sl] for n, sl in seg.items()})
        return out

    # 1. one operand element moved by one bf16 ulp (the element with the largest share of its products): the operand check sees the bits,
    #    and the product judged from the CORRECT operands is over its bound in every group that reads the operand
    def ulp_up(v32, idx):
        b = F.rne_bits(v32); b[idx] += 1
        return F.bf_val(b).astype(np.float32)
    big = lambda m: np.unravel_index(np.argmax(np.abs(m)), m.shape)
    ix = big(X[seg["v_other"]] * np.abs(g).sum(1, keepdims=True))
    xc_bad = xc.copy(); xc_bad[ix[0], L["c_vk"] + ix[1]] += 1
    with pytest.raises(AssertionError, match="Xc"):
        ref.check_xc(xc_bad)
    Xb = F.bf_val(xc_bad).astype(np.float32)
    bad = results(Xb, W, g, a, e, gb, wb)
    assert _rejected("h1", bad["h1"], prods["h1"][0]) and _rejected("v_other", bad["v_other"], prods["v_other"][0])
    iw = big(W[seg["v_other"]])
    wc_bad = wc.copy(); wc_bad[iw[0], L["c_vk"] + iw[1]] += 1
    with pytest.raises(AssertionError, match="Wc"):
        ref.check_wc(wc_bad, F.f32(ref.gt()[0]))
    assert _rejected("h1", results(X, F.bf_val(wc_bad).astype(np.float32)[:d.H], g, a, e, gb, wb)["h1"], prods["h1"][0])
    bad = results(X, W, ulp_up(g, big(g)), ulp_up(a, big(a)), ulp_up(e, big(e)), ulp_up(gb, big(gb[:d.H])), ulp_up(wb, big(wb)))
    for name in ("Gt", "a_other", "dE") + tuple(seg):
        assert _rejected(name, bad[name], prods[name][0]), ("one bf16 ulp", name)
    # 2. one k-row dropped from every reduction
    for drop in (0, 5):
        bad = results(X, W, g, a, e, gb, wb, drop=drop)
        for name in prods:
            assert _rejected(name, bad[name], prods[name][0]), ("dropped row %d" % drop, name)
    # 3. one padding column made non-zero: a gap column, a column beyond raw, a padding row of Wc
    for c in (L["c_vk"] + d.dv, L["raw"], L["kc"] - 1):
        xb = xc.copy(); xb[3, c] = 0x3C00
        with pytest.raises(AssertionError, match="Xc"):
            ref.check_xc(xb)
        wb_ = wc.copy(); wb_[2, c] = 0x3C00
        with pytest.raises(AssertionError, match="Wc"):
            ref.check_wc(wb_, F.f32(ref.gt()[0]))
    wb_ = wc.copy(); wb_[d.H, 0] = 0x3C00
    with pytest.raises(AssertionError, match="padding row"):
        ref.check_wc(wb_, F.f32(ref.gt()[0]))
    #    ... and where both operands are stale there, the product from the columns 0 .. raw alone is what the bound wants: h_1 moves
    Xs, Ws = X.copy(), W.copy()
    Xs[:, L["raw"]] = 1.0; Ws[:, L["raw"]] = 1.0
    assert _rejected("h1", results(Xs, Ws, g, a, e, gb, wb)["h1"], prods["h1"][0])
    # 4. one output element taken from the neighbouring tile: 16 columns over (16 rows where the block is narrower), at the place where
    #    the two differ most (two gated units of h_1 are both zero)
    good = results(X, W, g, a, e, gb, wb)
    for name, v in good.items():
        v = v.copy()
        if v.shape[1] > 16:
            i, j = np.unravel_index(np.argmax(np.abs(v[:, :-16] - v[:, 16:])), v[:, 16:].shape)
            v[i, j] = v[i, j + 16]
        else:
            i, j = np.unravel_index(np.argmax(np.abs(v[:-16] - v[16:])), v[16:].shape)
            v[i, j] = v[i + 16, j]
        assert _rejected(name, v, prods[name][0]), ("neighbouring tile", name)
