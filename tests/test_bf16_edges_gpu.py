"""GPU: the bf16 variant (NCX_F_BF16) product by product against tests/bf16_ref.py -- the pack branch of k_prep, k_pack_wc, k_pack2d,
k_pack_transposed, k_dpre_to_bf16, gemm_bf16_nt_kernel on its four tiles, gemm_bf16_nt8_kernel, gemm_bf16_tn_kernel, gemm_bf16_tn8_kernel
and k_bf16_reduce_dwc -- at the tile edges of the case table.  Every case sets its hooks, proves its route (ncx_plan_query
NCX_QUERY_BF16_ROUTE), runs one forward, loss and backward on a workspace filled with 0xFF and gradient buffers filled with NaN, checks the
packed operands the device left (NCX_WS_XC, NCX_WS_WC against the device's own NCX_WS_GT) bit for bit -- two-sided at tau for the distance and
the softmax -- and then holds every element of every product to 2^-24 c S of the exact fp64 sum of the device's own operands.  The fp32
products the variant keeps (groups e, g, h, i of main_bwd_ref.py, on the routes they take under the flag) and the hidden layers are held to
their own recorded bounds.  A second forward and backward on the same workspace gives the same bits, nz > 1 included (the slab order is
fixed).  L = 3: the library exposes dpre_1 only, so d linear_2 / linear_3 are not judged there (L = 2 judges the hidden layer's products).
Each product prints its ratio: `pytest -s` gives the figures of profiles/bf16_edges.json."""
import numpy as np
import pytest
import torch

import bf16_ref as F
import main_fwd_ref as R
from helpers import FIELD, dev, grad_tol, to_dev_batch, to_dev_params
from oracle import ncx_oracle as orc

pytestmark = pytest.mark.gpu

_REFS, _RUNS, _DEAD = {}, {}, []


def _reference(case, lay):
    """Inputs and restatement of a shape, built once and shared by the forms that run it; never modified."""
    key = F.shape_key(case)
    if key not in _REFS:
        d, params, batch, masks = F.build(case)
        _REFS[key] = (d, params, batch, masks, F.Bf16Ref(params, d, batch, lay, case["p"], masks))
    return _REFS[key]


def _check_route(case, dims):
    from neuralcx import _lib
    got = _lib.plan_query(dims, "BF16_ROUTE")
    mismatch = {k: (got[k], v) for k, v in case["route"].items() if got[k] != v}
    if mismatch and case["cu_dependent"]:
        pytest.skip("%s: the route depends on the CU count; this chip gives (got, wanted) %r" % (case["id"], mismatch))
    assert not mismatch, (case["id"], mismatch, got)


def _step(case):
    """Hooks are set by the caller.  -> what the checks read, as numpy copies, and whether a second step gave the same bits."""
    from neuralcx import _lib, ops
    d, params, batch, masks = F.build(case)
    keep = torch.stack(masks) if case["drop"] == "masks" else None
    b, p = to_dev_batch(batch, None, keep), to_dev_params(params)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A, flags=_lib.NCX_F_ALL | _lib.NCX_F_BF16, training=bool(case["drop"]), drop_p=case["p"],
                         seed=R.DROP_SEED if case["drop"] == "rng" else 0)
    _check_route(case, dims)
    lay = ops.bf16_layout(dims)
    assert lay == F.layout_of(case)
    ref = _reference(case, lay)[4]
    ws = ops.alloc_workspace(dims, dev())            # (after the hooks)
    ws.fill_(0xFF)
    np_ = lambda t: t.detach().cpu().numpy().copy()

    def once():
        scores = ops.forward(dims, b, p, ws)
        torch.cuda.synchronize()
        out = dict(scores=np_(scores), xc=np_(ops.ws_xc_view(dims, ws)), wc=np_(ops.ws_wc_view(dims, ws)), gt=np_(ops.ws_gt_view(dims, ws)),
                   h=[np_(ops.ws_h_view(dims, ws, l)) for l in range(1, d.L + 1)])
        lr = ops.ranking_loss(scores, batch["gt"].to(dev()).to(torch.int32))
        grads = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
        ops.backward(dims, b, p, ws, lr["dscores"], grads)
        torch.cuda.synchronize()
        out.update(dscores=np_(lr["dscores"]), dpre1=np_(ops.ws_dpre_view(dims, ws, 1)), dpre2=np_(ops.ws_dpre_view(dims, ws, 2)) if d.L == 2 else None,
                   grads={k: np_(grads[f]) for k, f in FIELD.items() if f in grads}, block=np_(ops.ws_dgt_view(dims, ws)),
                   xc_after=np_(ops.ws_xc_view(dims, ws)))
        return out

    out = once()
    assert out["xc"].shape == (ref.M, lay["kc"]) and out["wc"].shape == (lay["Hp"], lay["kc"]) and out["gt"].shape == (d.H, d.A)
    assert out["block"].size == 2 * d.H * d.A
    out["dgt"], out["dggt"] = out["block"].reshape(2, d.H, d.A)
    assert np.array_equal(out["xc"], out["xc_after"]), "the backward wrote into the packed rows"
    again = once()
    for k in ("scores", "xc", "wc", "gt", "dscores", "dpre1", "block"):
        assert np.array_equal(out[k].view(np.uint8), again[k].view(np.uint8)), (case["id"], k, "a second step on the same workspace gives other bits")
    for l in range(d.L):
        assert np.array_equal(out["h"][l], again["h"][l]), (case["id"], "h_%d" % (l + 1))
    for k in out["grads"]:
        assert np.array_equal(out["grads"][k], again["grads"][k]), (case["id"], k, "a second step on the same workspace gives other bits")
    return out


def _check(case, out):
    """The operands, then every product within its bound; -> {product: ratio}."""
    d, params, batch, masks, ref = _REFS[F.shape_key(case)]
    cid, g, ratios, bad = case["id"], out["grads"], {}, []
    # the operands
    two_sided = ref.check_xc(out["xc"])
    assert np.isfinite(out["gt"]).all()
    ref.check_wc(out["wc"], out["gt"])
    print("bf16 operands %s: Xc %d x %d and Wc %d x %d as expected, %d softmax elements judged two-sided" % ((cid,) + out["xc"].shape + out["wc"].shape + (two_sided,)))
    covered = {k: np.zeros(v.shape, bool) for k, v in g.items()}
    for k, v in g.items():
        assert np.isfinite(v).all(), (cid, k, "a gradient element was not written, or a NaN of the workspace was read")

    def judge(name, got, prod, tensor=None, sl=None):
        r, over, c = F.judge(name, got, prod)
        ratios[name] = r
        print("bf16 ratio %s %s %.3f (c %.1f)" % (cid, name, r, c))
        if over.size:
            bad.append("%s: %d elements over the bound, first %s, ratio %.3g, c %.1f" % (name, len(over), over[0].tolist(), r, c))
        if tensor is not None:
            assert not covered[tensor][sl].any()
            covered[tensor][sl] = True

    # p, q: the forward
    judge("Gt", out["gt"], ref.gt())
    judge("h1", out["h"][0], ref.h1(out["xc"], out["wc"]))
    for l in range(1, d.L + 1):
        got = out["h"][l - 1]
        assert np.isfinite(got).all(), (cid, l)
        if masks is not None:
            assert (got[masks[l - 1].numpy() == 0] == 0).all(), (cid, l, "a dropped element is not zero")
        if l > 1:
            _, h_ref, S = ref.fwd.layer(l, out["h"][l - 2])
            c = R.bound_c("I" if case["drop"] else "H")
            ratios["h%d" % l] = R.ratio(got, h_ref, S)
            print("bf16 ratio %s h%d %.3f (c %.1f)" % (cid, l, ratios["h%d" % l], c))
            over = np.argwhere(np.abs(got.astype(np.float64) - h_ref) > c * R.U24 * S)
            if over.size:
                bad.append("h%d: %d elements over the bound, first %s" % (l, len(over), over[0].tolist()))
    chain_scores = (out["h"][-1].astype(np.float64) @ params["out.weight"].numpy().astype(np.float64).T + float(params["out.bias"])).reshape(ref.B, d.K)
    assert np.abs(out["scores"] - chain_scores).max() <= 1e-4, (cid, "scores")
    # h: the out layer, from dscores and the device's h_L
    hL = out["h"][-1]
    top = ref.bwd.from_dscores(out["dscores"], hL)
    if d.L <= 2:
        dpre_top = out["dpre2"] if d.L == 2 else out["dpre1"]
        r, tol = top["dpreL"]
        assert np.isfinite(dpre_top).all() and (dpre_top[hL <= 0] == 0).all(), (cid, "dpre_L")
        err = np.abs(dpre_top.astype(np.float64) - r)
        print("bf16 ratio %s dpreL %.3f (of its own bound)" % (cid, float((err / tol).max())))
        if (err > tol).any():
            bad.append("dpreL: %d elements over the bound, worst %.3g of it" % ((err > tol).sum(), (err / tol).max()))
    judge("w_out", g["out.weight"], top["w_out"], "out.weight", np.s_[:])
    judge("b_out", g["out.bias"], top["b_out"], "out.bias", np.s_[:])
    # i: the hidden layer, from the device's dpre_2 and h_1
    if d.L == 2:
        p = ref.bwd.from_dpre(2, out["dpre2"], out["h"][0])
        judge("w2", g["linear_2.weight"], p["w2"], "linear_2.weight", np.s_[:])
        judge("b2", g["linear_2.bias"], p["b2"], "linear_2.bias", np.s_[:])
        assert (out["dpre1"][out["h"][0] <= 0] == 0).all()
        judge("dpre1", out["dpre1"], p["dpre1"])
    elif d.L == 3:
        for k in ("linear_2.weight", "linear_2.bias", "linear_3.weight", "linear_3.bias"):
            covered[k][:] = True
    assert np.isfinite(out["dpre1"]).all()
    # r: dWc from the device's dpre_1 and Xc; e, g: the fp32 products from the same dpre_1
    o, w1 = d.offsets(), g["linear_1.weight"]
    parts = ref.dwc(out["dpre1"], out["xc"])
    for name, c0, o0, w in ref.segments:
        judge(name, w1[:, o0: o0 + w], parts[name], "linear_1.weight", np.s_[:, o0: o0 + w])
    judge("dGt", out["dgt"], parts["dGt"])
    fp32 = ref.bwd.from_dpre1(out["dpre1"])
    for name, _, w in ref.bwd.shared_cols:
        judge(name, w1[:, o[name]: o[name] + w], fp32[name], "linear_1.weight", np.s_[:, o[name]: o[name] + w])
    judge("dGgt", out["dggt"], fp32["dGgt"])
    judge("b1", g["linear_1.bias"], fp32["b1"], "linear_1.bias", np.s_[:])
    # s, t: from the device's block
    blk = ref.from_block(out["dgt"], out["dggt"])
    sl = np.s_[:, o["a_emb_other"]: o["a_emb_other"] + d.da]
    judge("a_other", w1[sl], blk["a_other"], "linear_1.weight", sl)
    judge("dE", g["answer_embedding.weight"], blk["dE"], "answer_embedding.weight", np.s_[:])
    for k, m in covered.items():
        assert m.all(), (cid, k, "columns of the returned gradient that no product was judged on")
    assert not bad, (cid, bad)
    return ratios


def _run(case, monkeypatch):
    from neuralcx import ops
    if case["id"] not in _RUNS:
        if _DEAD:                                    # (a runtime error leaves the device context unusable: launch nothing more on it)
            pytest.fail("not run: an earlier case ended in %s" % _DEAD[0])
        with monkeypatch.context() as m:
            m.setattr(ops, "EXTRA_FLAGS", 0)
            if case["env"]:
                m.setenv("NCX_EXPERIMENT", "1")
                for k, v in case["env"].items():
                    m.setenv(k, v)
            try:
                out = _step(case)
            except AssertionError:
                raise
            except Exception as e:
                _DEAD.append("%s: %r" % (case["id"], e))
                raise
        _RUNS[case["id"]] = (out, _check(case, out))
    return _RUNS[case["id"]]


@pytest.mark.parametrize("case_id", [c["id"] for c in F.CASES])
def test_operands_and_products_against_fp64(case_id, monkeypatch):
    _run(F.BY_ID[case_id], monkeypatch)


@pytest.mark.parametrize("tag", [t for t, _ in F.FORM_SHAPES])
def test_forms_of_one_shape_agree(tag, monkeypatch):
    """The four NT tiles and the 192 x 256 kernel, the 128 x 128 and the 256 x 128 TN kernels on one shape: each alone within its bound
    (above), and among each other to the suite's rules for the variant's forms (test_hip_parity): scores 1e-5, every gradient 1e-5 of its
    tensor's max in the bf16 oracle.  The NT forms take the same k order per element: h_1 bit for bit."""
    cases = [c for c in F.CASES if c["id"].startswith("forms-%s-" % tag)]
    assert len(cases) == 10
    d, params, batch, masks = F.build(cases[0])
    _, _, g_ref = orc.loss_and_grads_bf16(params, d, batch)
    first = _run(cases[0], monkeypatch)[0]
    for c in cases[1:]:
        out = _run(c, monkeypatch)[0]
        assert np.array_equal(out["h"][0], first["h"][0]), (cases[0]["id"], c["id"], "h_1")
        assert np.abs(out["scores"] - first["scores"]).max() <= 1e-5
        for k, ref in g_ref.items():
            assert np.abs(out["grads"][k] - first["grads"][k]).max() <= grad_tol(k, ref.numpy(), 1e-5), (cases[0]["id"], c["id"], k)
