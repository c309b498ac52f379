"""GPU: the fused forward kernel family (csrc/ncx_main.h: k_main_fwd in its chain and fold tile forms, k_main_fixup) at the edge shapes of
tests/main_fwd_ref.py.  Every case proves its route (ncx_plan_query NCX_QUERY_FWD_ROUTE: a case that fell onto the generic engine fails),
runs on a workspace filled with 0xFF (a missing zero-pad column of a packed weight slice, or an unread slab chunk, is a NaN) and compares
the post-dropout activations of every layer (ops.ws_h_view) element by element with the fp64 restatement under the bound
c * 2^-24 * S of main_fwd_ref (layer l > 1 on the device's own h_{l-1}); scores keep the suite's rule (1e-4 against fp64).  Group J runs
whole steps through compare_with_oracle.  Each case prints its ratio: `pytest -s` gives the figures of profiles/main_fwd_edges.json."""
import numpy as np
import pytest
import torch

import main_fwd_ref as R
from helpers import compare_with_oracle, dev, to_dev_batch, to_dev_params

pytestmark = pytest.mark.gpu


_REFS = {}


def _reference(case):
    """Inputs and restatement of a shape, built once and shared by the cases (forms, splits) that run it; never modified."""
    key = R.shape_key(case)
    if key not in _REFS:
        d, params, batch, spec, masks = R.build(case)
        ref = R.MainFwdRef(params, d, batch, spec, case["p"], masks)
        _REFS[key] = (d, params, batch, spec, masks, ref, ref.chain())
    return _REFS[key]


def _set_hooks(case, monkeypatch):
    from neuralcx import ops
    if case["fp32"]:
        monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    if case["env"]:
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        for k, v in case["env"].items():
            monkeypatch.setenv(k, v)


def _check_route(case, dims):
    from neuralcx import _lib
    got = _lib.plan_query(dims, "FWD_ROUTE")
    want = case["route"]
    mismatch = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    if mismatch and case["cu_dependent"]:
        pytest.skip("%s: the route depends on the CU count; this chip gives (got, wanted) %r" % (case["id"], mismatch))
    assert not mismatch, (case["id"], mismatch, got)
    return got


def _forward(case):
    """Hooks are set by the caller.  -> dims, scores [B, K], [h_1 .. h_L] as fp32 numpy, after one forward on a NaN-filled workspace."""
    from neuralcx import ops
    d, params, batch, spec, masks, ref, chain = _reference(case)
    extra = {k: batch[k] for k in ("v_rank", "a_emb_gt") if k in batch}
    keep = torch.stack(masks) if case["drop"] == "masks" else None
    b, p = to_dev_batch(batch, spec, keep, extra), to_dev_params(params)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A, flags=ops.flags_from_spec(spec), training=bool(case["drop"]), drop_p=case["p"],
                         seed=R.DROP_SEED if case["drop"] == "rng" else 0)
    _check_route(case, dims)
    ws = ops.alloc_workspace(dims, dev())           # (after the hooks: the slab is sized by the split)
    ws.fill_(0xFF)
    scores = ops.forward(dims, b, p, ws)
    torch.cuda.synchronize()
    hs = [ops.ws_h_view(dims, ws, l).cpu().numpy().copy() for l in range(1, d.L + 1)]
    return dims, (b, p, ws), scores.cpu().numpy(), hs


def _check(case, scores, hs):
    """Every layer within c * 2^-24 * S of the restatement on the device's own input; dropped elements exact zeros; scores 1e-4."""
    d, params, batch, spec, masks, ref, chain = _reference(case)
    c, worst = R.bound_c(case["group"]), 0.0
    for l in range(1, d.L + 1):
        got = hs[l - 1]
        assert np.isfinite(got).all(), (case["id"], l, "non-finite activations: a NaN of the workspace was read")
        _, h_ref, S = ref.layer(l, hs[l - 2] if l > 1 else None)
        if masks is not None:
            assert (got[masks[l - 1].numpy() == 0] == 0).all(), (case["id"], l, "a dropped element is not zero")
        r = R.ratio(got, h_ref, S)
        worst = max(worst, r)
        err = np.abs(got.astype(np.float64) - h_ref)
        bad = np.argwhere(err > c * R.U24 * S)
        print("ratio %s layer %d %.3f (c %.1f)" % (case["id"], l, r, c))
        assert bad.size == 0, (case["id"], l, "elements over the bound: %d, first (row, col) %s, ratio %.3g, c %.1f" % (len(bad), bad[0].tolist(), r, c))
    assert np.isfinite(scores).all() and np.abs(scores - chain["scores"]).max() <= 1e-4, (case["id"], np.abs(scores - chain["scores"]).max())
    return worst


def _ids(group):
    return [c["id"] for c in R.CASES if c["group"] == group]


@pytest.mark.parametrize("case_id", _ids("A") + _ids("B") + _ids("C") + _ids("D") + _ids("E") + _ids("G") + _ids("H") + _ids("I"))
def test_edge_case_against_fp64(case_id, monkeypatch):
    """Groups A (column edges x epilogue / fix-up), B (reduction extents), C (rows per triplet), D (operand sequences), E (distance in the
    kernel), G (chain tile forms), H (hidden layers), I (dropout at ragged H).  A split run repeated is bit-identical."""
    from neuralcx import ops
    case = R.BY_ID[case_id]
    _set_hooks(case, monkeypatch)
    dims, (b, p, ws), scores, hs = _forward(case)
    _check(case, scores, hs)
    if case["route"]["split"] > 1:
        again = ops.forward(dims, b, p, ws).cpu().numpy()
        assert np.array_equal(scores, again)
        for l in range(1, dims.L + 1):
            assert np.array_equal(hs[l - 1], ops.ws_h_view(dims, ws, l).cpu().numpy())


_FOLD_SHAPES = sorted({(c["K"], c["dv"], c["H"], c["B"]) for c in R.CASES if c["group"] == "F"})


@pytest.mark.parametrize("K,dv,H,B", _FOLD_SHAPES)
def test_fold_forms_against_fp64_and_each_other(K, dv, H, B, monkeypatch):
    """Group F: the per-triplet fold on 48- (K = 24 only), 96- and 192-row tiles, partial row tiles (B triplets in tiles of 2 / 4 / 8) and
    partial 64-column tiles; the forms of a shape give the same bits (same expression, same k order)."""
    first = None
    for rows in (48, 96, 192):
        cid = "F-K%d-dv%d-H%d-B%d-%d" % (K, dv, H, B, rows)
        if cid not in R.BY_ID:
            continue
        case = R.BY_ID[cid]
        with monkeypatch.context() as m:
            _set_hooks(case, m)
            _, _, scores, hs = _forward(case)
        _check(case, scores, hs)
        if first is None:
            first = (cid, scores, hs)
        else:
            assert np.array_equal(first[1], scores) and np.array_equal(first[2][0], hs[0]), (first[0], cid)


@pytest.mark.parametrize("case_id", [c["id"] for c in R.J_CASES])
def test_whole_step_at_edge_shapes_vs_oracle(case_id, monkeypatch):
    """Group J: forward, loss and backward (NaN-filled gradients) through compare_with_oracle on cases of every group, at A in {36, 132} and
    da in {12, 100}; under NCX_MAIN_CFG the answer-embedding gradient's two-segment chain runs on the forced tile form too."""
    from neuralcx import ops
    case = R.BY_ID[case_id]
    _set_hooks(case, monkeypatch)
    d, params, batch, spec, masks = R.build(case)
    extra = {k: batch[k] for k in ("v_rank", "a_emb_gt") if k in batch}
    b = to_dev_batch(batch, spec, None, extra)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A, flags=ops.flags_from_spec(spec), training=bool(case["drop"]), drop_p=case["p"], seed=R.DROP_SEED)
    _check_route(case, dims)
    compare_with_oracle(d, spec, params, batch, training=bool(case["drop"]), drop_p=case["p"], masks=masks, seed=R.DROP_SEED, extra=extra,
                        use_rng=case["drop"] == "rng")
