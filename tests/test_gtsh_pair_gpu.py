"""GPU: Gt and Sh as one launch of the fused forward kernel's 64 x 64 form (the PAIR form of k_main_fwd + k_main_fixup_pair) at the edge
shapes of tests/gtsh_pair_ref.py.  Every shape runs with the route on and with the hook NCX_NO_GTSH_PAIR (today's two launches of the
generic engine + their merged fix-up) in one process, on workspaces filled with 0xFF, and both are held against the fp64 restatement of
tests/main_fwd_ref.py under that file's rule |x - x_ref| <= c * 2^-24 * S with its constant for the reduction-extent group (B): Gt
directly (ops.ws_gt_view; S = |W1[:, a_other]| . |E|^T), Sh through h_1 (its S includes |Sh| and |b1|), scores to 1e-4.  Where the route
must not be taken (NCX_F_REUSE_GT, the a_emb lesion) the planner says so and the results equal the hook-on run bit for bit.  The pair keeps
the k-chunks of the two launches, so its own results equal theirs bit for bit too; a case forces several chunks per workgroup."""
import numpy as np
import pytest
import torch

import gtsh_pair_ref as G
import main_fwd_ref as R
from helpers import dev, to_dev_params
from oracle import ncx_oracle as orc

pytestmark = pytest.mark.gpu

C = R.bound_c("B")
_REFS = {}


def _reference(sid, lesion=False):
    """Inputs and restatement of a shape: built once, shared by the runs, never modified."""
    key = (sid, lesion)
    if key not in _REFS:
        d, params, batch, table, img_idx = G.build(sid, lesion)
        spec = dict(orc.DEFAULT_SPEC, a_emb=False) if lesion else None
        ref = R.MainFwdRef(params, d, batch, spec)
        _, h_ref, S = ref.layer(1)
        W1, o = params["linear_1.weight"].double().numpy(), d.offsets()
        wak = W1[:, o["a_emb_other"]: o["a_emb_other"] + d.da]
        E = params["answer_embedding.weight"].double().numpy()
        _REFS[key] = dict(d=d, params=params, batch=batch, table=table, img_idx=img_idx, spec=spec, h=h_ref, S=S, scores=ref.chain()["scores"],
                          gt=wak @ E.T, S_gt=np.abs(wak) @ np.abs(E).T)
    return _REFS[key]


def _run(sid, monkeypatch, hook, lesion=False, reuse=False, gt_in=None, wpt=None):
    """One forward (two with `reuse`: the second with NCX_F_REUSE_GT on the first one's workspace, whose Gt is replaced by `gt_in` when that
    is given) -> dict(plan, scores, h, gt)."""
    from neuralcx import _lib, ops
    r = _reference(sid, lesion)
    d, b = r["d"], r["batch"]
    with monkeypatch.context() as m:
        if hook:
            m.setenv("NCX_EXPERIMENT", "1")
            m.setenv("NCX_NO_GTSH_PAIR", "1")
        if wpt:                                          # the workgroups per tile, forced (the natural plan of a small shape gives every chunk its own)
            m.setenv("NCX_EXPERIMENT", "1")
            m.setenv("NCX_PAIR_WPT", wpt)
        g = lambda k: b[k].to(dev()).contiguous()
        extra = dict(a_emb_gt=g("a_emb_gt")) if lesion else {}
        batch = ops.Batch(r["table"].to(dev()), r["img_idx"].to(dev()), g("q_emb"), g("z_orig"), g("z_knns"), g("a_knns"),
                          b["answer_aids"].to(torch.int32).to(dev()), **extra)
        p = to_dev_params(r["params"])
        dims = ops.make_dims(batch, H=d.H, L=1, da=d.da, A=d.A, flags=ops.flags_from_spec(r["spec"]))
        plan = _lib.plan_query(dims, "GTSH_PAIR")
        plan["splits"] = (_lib.plan_query(dims, "GT")["ksplit"], _lib.plan_query(dims, "SH")["ksplit"])
        ws = ops.alloc_workspace(dims, dev())           # (after the hook: the pair's slab and padded weights are sized by the route)
        ws.fill_(0xFF)
        scores = ops.forward(dims, batch, p, ws)
        if reuse:
            if gt_in is not None:
                ops.ws_gt_view(dims, ws).copy_(torch.from_numpy(gt_in).to(dev()))
            dims.flags |= _lib.NCX_F_REUSE_GT
            plan = _lib.plan_query(dims, "GTSH_PAIR")
            scores = ops.forward(dims, batch, p, ws)
        torch.cuda.synchronize()
        return dict(plan=plan, scores=scores.cpu().numpy(), h=ops.ws_h_view(dims, ws, 1).cpu().numpy().copy(),
                    gt=None if lesion else ops.ws_gt_view(dims, ws).cpu().numpy().copy())


def _check(sid, got, tag, lesion=False):
    r = _reference(sid, lesion)
    A = r["d"].A
    assert np.isfinite(got["h"]).all() and np.isfinite(got["scores"]).all(), (sid, tag, "a NaN of the workspace was read")
    if not lesion:
        assert np.isfinite(got["gt"]).all(), (sid, tag)
        assert (got["gt"][:, A:] == 0).all(), (sid, tag, "Gt's pad columns are not zero")
        rg = R.ratio(got["gt"][:, :A], r["gt"], r["S_gt"])
        print("ratio %s %s Gt %.3f (c %.1f)" % (sid, tag, rg, C))
        assert rg <= C, (sid, tag, "Gt", rg)
    rh = R.ratio(got["h"], r["h"], r["S"])
    es = float(np.abs(got["scores"] - r["scores"]).max())
    print("ratio %s %s h_1 %.3f (c %.1f), scores %.2e" % (sid, tag, rh, C, es))
    assert rh <= C, (sid, tag, "h_1", rh)
    assert es <= 1e-4, (sid, tag, es)


@pytest.mark.parametrize("sid", list(G.SHAPES))
def test_pair_and_old_path_against_fp64(sid, monkeypatch):
    """Route on: the planner reports it with the rules of the issue, a repeated run is bit-identical (no atomics, fixed order); route off by
    the hook: the old path.  Both within the bound of the fp64 restatement."""
    on = _run(sid, monkeypatch, hook=False)
    assert on["plan"]["taken"], on["plan"]
    G.check_plan(G.SHAPES[sid], on["plan"], *on["plan"]["splits"])
    if "da516" in sid:
        assert on["plan"]["s_gt"] > 1 and on["plan"]["s_sh"] > 1 and on["plan"]["s_gt"] != on["plan"]["s_sh"], on["plan"]
    _check(sid, on, "pair")
    again = _run(sid, monkeypatch, hook=False)
    assert np.array_equal(on["h"], again["h"]) and np.array_equal(on["gt"], again["gt"]) and np.array_equal(on["scores"], again["scores"])
    off = _run(sid, monkeypatch, hook=True)
    assert not off["plan"]["taken"], off["plan"]
    _check(sid, off, "hook")
    # the same chunks, the same order inside a step, the same order of the partial tiles: the pair computes the two launches' bits
    assert np.array_equal(on["gt"], off["gt"]) and np.array_equal(on["h"], off["h"]) and np.array_equal(on["scores"], off["scores"]), sid


@pytest.mark.parametrize("why", ["reuse_gt", "lesion"])
def test_route_not_taken_equals_old_path_bitwise(why, monkeypatch):
    """NCX_F_REUSE_GT (an evaluation pass on the step's Gt) and the a_emb lesion keep today's launches: the planner reports the route as not
    taken and the results are those of the hook-on run, bit for bit.  (Gt is an INPUT of a reuse pass: the hook-on run is handed the Gt the
    first run's step left, so both passes compute Sh and h_1 from the same bits.)"""
    sid = "B65-A70-H20-da516"
    kw = dict(reuse=True) if why == "reuse_gt" else dict(lesion=True)
    a = _run(sid, monkeypatch, hook=False, **kw)
    assert not a["plan"]["taken"], a["plan"]
    if why == "reuse_gt":
        kw["gt_in"] = a["gt"]
    b = _run(sid, monkeypatch, hook=True, **kw)
    assert not b["plan"]["taken"], b["plan"]
    _check(sid, a, why, lesion=why == "lesion")
    assert np.array_equal(a["h"], b["h"]) and np.array_equal(a["scores"], b["scores"])
    if why == "reuse_gt":
        assert np.array_equal(a["gt"], b["gt"])


def test_several_chunks_per_workgroup_keep_the_bits(monkeypatch):
    """At the workload's shape a workgroup of Sh runs two consecutive chunks (16 chunks, 8 workgroups per tile).  Here: Gt's 2 and Sh's 3
    chunks in ONE workgroup per tile each, against one chunk per workgroup and against the two launches: the same partial tiles, the same bits."""
    sid = "B65-A70-H20-da516"
    one = _run(sid, monkeypatch, hook=False, wpt="1,1")
    assert one["plan"]["taken"] and (one["plan"]["w_gt"], one["plan"]["w_sh"]) == (1, 1) and one["plan"]["s_gt"] == 2 and one["plan"]["s_sh"] == 3, one["plan"]
    _check(sid, one, "wpt 1,1")
    for other in (_run(sid, monkeypatch, hook=False), _run(sid, monkeypatch, hook=True)):
        assert np.array_equal(one["gt"], other["gt"]) and np.array_equal(one["h"], other["h"]) and np.array_equal(one["scores"], other["scores"])
