"""GPU: the backward's kernels product by product against the fp64 restatement of tests/main_bwd_ref.py -- the per-triplet fold kernels
(k_dw_km8, k_dw_km_x6, k_dw_km), the balanced TN launch (k_dw_tn8, k_dw_tn8_x6), the grouped and chain GEMMs, the dE routes, the column
sums and k_bwd_prelude -- at the smallest shapes that select each form.  Every case proves its route first (ncx_plan_query
NCX_QUERY_DW1_ROUTE, as test_backward_routes_gpu.expect: the form is part of the id), runs on a workspace filled with 0xFF and gradient
buffers filled with NaN, reads what the device handed to each kernel (dpre_1, dpre_2, h_l, the dGt | dGgt block) and holds every element of
every product to 2^-24 (c S + extra).  The columns are read from the tensors ops.backward returned, and together they cover every element
of every gradient.  Each case runs as the fp32 form (EXTRA_FLAGS 0) and under NCX_F_X6; the X6 run is also held, per product, to 1.5 x
the fp32 run's worst ratio + 1.  Each product prints its ratio: `pytest -s` gives the figures of profiles/main_bwd_edges.json."""
import numpy as np
import pytest
import torch

import main_bwd_ref as Bw
import main_fwd_ref as R
from helpers import FIELD, dev, to_dev_batch, to_dev_params
from test_backward_routes_gpu import expect

pytestmark = pytest.mark.gpu

_REFS, _RATIOS = {}, {}


def _reference(case):
    """Inputs and restatement of a shape, built once and shared by the cases and forms that run it; never modified."""
    key = Bw.shape_key(case)
    if key not in _REFS:
        d, params, batch, spec, masks = Bw.build(case)
        fwd = R.MainFwdRef(params, d, batch, spec, case["p"], masks)
        _REFS[key] = (d, params, batch, spec, masks, Bw.MainBwdRef(fwd, params, batch))
    return _REFS[key]


def _step(case):
    """One forward, loss and backward with the hooks already set -> what the checks read, as float32 numpy."""
    from neuralcx import ops
    d, params, batch, spec, masks, ref = _reference(case)
    extra = {k: batch[k] for k in ("v_rank", "a_emb_gt") if k in batch}
    b, p = to_dev_batch(batch, spec, None, extra), to_dev_params(params)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A, flags=ops.flags_from_spec(spec), training=bool(case["drop"]), drop_p=case["p"],
                         seed=R.DROP_SEED if case["drop"] else 0)
    expect(d, case["B"], spec, case["fold"], case["tn"])
    ws = ops.alloc_workspace(dims, dev())            # (after the hooks: the slabs are sized by the splits)
    ws.fill_(0xFF)
    scores = ops.forward(dims, b, p, ws)
    lr = ops.ranking_loss(scores, batch["gt"].to(dev()).to(torch.int32))
    grads = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    ops.backward(dims, b, p, ws, lr["dscores"], grads)
    torch.cuda.synchronize()
    np_ = lambda t: t.detach().cpu().numpy().copy()
    out = dict(dscores=np_(lr["dscores"]), h=[np_(ops.ws_h_view(dims, ws, l)) for l in range(1, d.L + 1)], dpre1=np_(ops.ws_dpre_view(dims, ws, 1)),
               dpre2=np_(ops.ws_dpre_view(dims, ws, 2)) if d.L == 2 else None, grads={k: np_(grads[f]) for k, f in FIELD.items() if f in grads})
    blk = np_(ops.ws_dgt_view(dims, ws))
    if not ref.spec["a_emb"]:
        assert blk.size == 0
    elif case["emb_nt"]:                              # dGt^T | dGgt^T, 2 x [A][pad4(H)]
        hp4 = (d.H + 3) // 4 * 4
        assert blk.size == 2 * d.A * hp4
        blk = blk.reshape(2, d.A, hp4)[:, :, :d.H]
        out["dgt"], out["dggt"] = blk[0].T.copy(), blk[1].T.copy()
    else:                                             # dGt | dGgt, 2 x [H][A]
        assert blk.size == 2 * d.H * d.A
        out["dgt"], out["dggt"] = blk.reshape(2, d.H, d.A)
    return out


def _check(case, form, dev_out):
    """Every product within its bound; -> {product: ratio}.  Asserts that the judged columns cover every gradient tensor exactly once."""
    d, params, batch, spec, masks, ref = _reference(case)
    g, ratios, bad = dev_out["grads"], {}, []
    covered = {k: np.zeros(v.shape, bool) for k, v in g.items()}
    for k, v in g.items():
        assert np.isfinite(v).all(), (case["id"], form, k, "a gradient element was not written, or a NaN of the workspace was read")

    def judge(name, got, prod, tensor=None, sl=None):
        r, S, extra, n = prod
        c = Bw.bound_c(name, n)
        got = np.asarray(got, np.float64).reshape(r.shape)
        assert np.isfinite(got).all(), (case["id"], form, name)
        ratios[name] = Bw.ratio(got, r, S, extra)
        over = np.abs(got - r) > Bw.U24 * (c * S + extra)
        print("bwd ratio %s %s %s %.3f (c %.1f)" % (case["id"], form, name, ratios[name], c))
        if over.any():
            bad.append("%s: %d elements over the bound, first %s, ratio %.3g, c %.1f" % (name, over.sum(), np.argwhere(over)[0].tolist(), ratios[name], c))
        if tensor is not None:
            assert not covered[tensor][sl].any()
            covered[tensor][sl] = True

    # h: the out layer, from dscores and the device's h_L
    hL = dev_out["h"][-1]
    top = ref.from_dscores(dev_out["dscores"], hL)
    dpre_top = dev_out["dpre2"] if d.L == 2 else dev_out["dpre1"]
    r, tol = top["dpreL"]
    assert np.isfinite(dpre_top).all() and (dpre_top[hL <= 0] == 0).all(), (case["id"], form, "dpre_L")
    err = np.abs(dpre_top.astype(np.float64) - r)
    print("bwd ratio %s %s dpreL %.3f (of its own bound)" % (case["id"], form, float((err / tol).max())))
    if (err > tol).any():
        bad.append("dpreL: %d elements over the bound, worst %.3g of it" % ((err > tol).sum(), (err / tol).max()))
    judge("w_out", g["out.weight"], top["w_out"], "out.weight", np.s_[:])
    judge("b_out", g["out.bias"], top["b_out"], "out.bias", np.s_[:])
    # i: the hidden layer, from the device's dpre_2 and h_1
    if d.L == 2:
        p = ref.from_dpre(2, dev_out["dpre2"], dev_out["h"][0])
        judge("w2", g["linear_2.weight"], p["w2"], "linear_2.weight", np.s_[:])
        judge("b2", g["linear_2.bias"], p["b2"], "linear_2.bias", np.s_[:])
        assert (dev_out["dpre1"][dev_out["h"][0] <= 0] == 0).all()
        judge("dpre1", dev_out["dpre1"], p["dpre1"])
    # a .. e, g: from the device's dpre_1
    parts = ref.from_dpre1(dev_out["dpre1"])
    o, w1 = d.offsets(), g["linear_1.weight"]
    width = dict(v_orig=d.dv, v_other=d.dv, v_mult=d.dv, v_dist=1, v_rank=d.K, q_emb=d.dq, z_orig=d.dz, z_other=d.dz, a_emb_gt=d.da)
    for name, w in width.items():
        sl = np.s_[:, o[name]: o[name] + w]
        if name in parts:
            judge(name, w1[sl], parts[name], "linear_1.weight", sl)
        else:                                         # the v_mult lesion's block: exactly zero
            assert name == "v_mult" and not ref.spec["v_mult"] and (w1[sl] == 0).all(), (case["id"], form, name)
            covered["linear_1.weight"][sl] = True
    judge("b1", g["linear_1.bias"], parts["b1"], "linear_1.bias", np.s_[:])
    sl = np.s_[:, o["a_emb_other"]: o["a_emb_other"] + d.da]
    if ref.spec["a_emb"]:
        judge("dGt", dev_out["dgt"], parts["dGt"])
        judge("dGgt", dev_out["dggt"], parts["dGgt"])
        # f: from the device's block
        blk = ref.from_block(dev_out["dgt"], dev_out["dggt"])
        judge("a_other", w1[sl], blk["a_other"], "linear_1.weight", sl)
        judge("dE", g["answer_embedding.weight"], blk["dE"], "answer_embedding.weight", np.s_[:])
    else:
        judge("a_other_lesion", w1[sl], parts["a_other_lesion"], "linear_1.weight", sl)
        assert (g["answer_embedding.weight"] == 0).all()
        covered["answer_embedding.weight"][:] = True
    for k, m in covered.items():
        assert m.all(), (case["id"], form, k, "columns of the returned gradient that no product was judged on")
    assert not bad, (case["id"], form, bad)
    return ratios


def _run(case, form, monkeypatch):
    from neuralcx import _lib, ops
    key = (case["id"], form)
    if key not in _RATIOS:
        with monkeypatch.context() as m:
            m.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6 if form == "x6" else 0)
            if case["env"]:
                m.setenv("NCX_EXPERIMENT", "1")
                for k, v in case["env"].items():
                    m.setenv(k, v)
            out = _step(case)
        _RATIOS[key] = _check(case, form, out)
    return _RATIOS[key]


@pytest.mark.parametrize("case_id", [c["id"] for c in Bw.CASES])
def test_fp32_form_products_against_fp64(case_id, monkeypatch):
    _run(Bw.BY_ID[case_id], "fp32", monkeypatch)


@pytest.mark.parametrize("case_id", [c["id"] for c in Bw.CASES])
def test_x6_form_products_against_fp64_and_the_fp32_form(case_id, monkeypatch):
    """The same bound under NCX_F_X6 (k_dw_km_x6, k_dw_tn8_x6 where the id's route names the 8-wave kernels), and fp32-grade per product.

    What this rule found (profiles/main_bwd_edges.json `found`): with six plane products on one accumulator k_dw_tn8_x6 reached 5.76 on z_orig
    against the fp32 kernel's 2.32 at grouped-tn8-B128-no_a_emb (allowed 4.48), 4.04 against 1.79 on z_other, 5.82 against 3.10 on a_other; with
    eight products on two accumulators it is at 1.32, 1.37 and 2.62."""
    case = Bw.BY_ID[case_id]
    x6 = _run(case, "x6", monkeypatch)
    fp32 = _run(case, "fp32", monkeypatch)
    worse = {k: (x6[k], fp32[k]) for k in x6 if not Bw.x6_rule(x6[k], fp32[k])}
    assert not worse, (case_id, "X6 ratio over 1.5 x the fp32 form's + 1 (x6, fp32):", worse)
