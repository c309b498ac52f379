"""CPU: the joint planner of the Gt + Sh pair launch (csrc/ncx_plan.hip: plan_gtsh_pair, reported by ncx_plan_query NCX_QUERY_GTSH_PAIR; host
only, 256 CUs assumed without a device) on the shapes of tests/gtsh_pair_ref.py, the benchmark's configs[1] and its 64-triplet shard:
the k-chunks of the two launches it replaces, workgroups within one round of slots on every XCD, no chunk under 8 steps unless the problem
is unsplit, each reduction covered exactly once; and the conditions under which the route is not taken."""
import ctypes

import pytest

import gtsh_pair_ref as G


def _query(s, flags=None, **kw):
    from neuralcx import _lib
    n = G.c_dims(s, _lib.NCX_F_ALL if flags is None else flags, **kw)
    assert _lib.lib().ncx_workspace_bytes(ctypes.byref(n)) > 0
    plan = _lib.plan_query(n, "GTSH_PAIR")
    plan["splits"] = (_lib.plan_query(n, "GT")["ksplit"], _lib.plan_query(n, "SH")["ksplit"])
    return plan


@pytest.mark.parametrize("sid", list(G.SHAPES))
def test_plan_of_edge_shapes(sid, monkeypatch):
    monkeypatch.delenv("NCX_EXPERIMENT", raising=False)
    plan = _query(G.SHAPES[sid])
    assert plan["taken"], plan
    G.check_plan(G.SHAPES[sid], plan, *plan["splits"])


@pytest.mark.parametrize("wid", list(G.WORKLOAD))
def test_plan_of_workload_shapes(wid, monkeypatch):
    monkeypatch.delenv("NCX_EXPERIMENT", raising=False)
    s = G.WORKLOAD[wid]
    plan = _query(s, n_img=82783)
    assert plan["taken"], plan
    G.check_plan(s, plan, *plan["splits"])
    if wid == "configs1" and plan["slots"] == 768:          # 256 CUs: 128 tiles x 4 chunks of 18-19 steps, one per workgroup + 32 tiles x 16 chunks of 14-15, two per workgroup: 96 on every XCD
        assert (plan["s_gt"], plan["s_sh"], plan["w_gt"], plan["w_sh"]) == (4, 16, 4, 8), plan


def test_route_conditions(monkeypatch):
    """Not taken: the hook, NCX_F_REUSE_GT, the a_emb lesion, the bf16 variant, a width that is no multiple of 4, nothing to split.  The
    X6 bit changes nothing.  The workspace is sized by the route, not by NCX_F_REUSE_GT."""
    from neuralcx import _lib
    monkeypatch.delenv("NCX_EXPERIMENT", raising=False)
    s = G.SHAPES["B65-A70-H20-da516"]
    base = _query(s)
    assert base["taken"]
    assert _query(s, _lib.NCX_F_ALL | _lib.NCX_F_X6) == base
    assert not _query(s, _lib.NCX_F_ALL | _lib.NCX_F_REUSE_GT)["taken"]
    assert not _query(s, _lib.NCX_F_ALL & ~_lib.NCX_F_A_EMB)["taken"]
    assert not _query(s, _lib.NCX_F_ALL | _lib.NCX_F_BF16)["taken"]
    assert not _query(dict(s, dq=102))["taken"]
    short = _query(dict(s, da=36, dq=8))                     # 1 and 2 + 1 + 1 + 2 steps: no chunk of 8 to cut
    assert (short["taken"], short["s_gt"], short["s_sh"]) == (False, 1, 1), short
    size = lambda flags: _lib.lib().ncx_workspace_bytes(ctypes.byref(G.c_dims(s, flags)))
    assert size(_lib.NCX_F_ALL) == size(_lib.NCX_F_ALL | _lib.NCX_F_REUSE_GT)
    monkeypatch.setenv("NCX_EXPERIMENT", "1")
    monkeypatch.setenv("NCX_NO_GTSH_PAIR", "1")
    off = _query(s)
    assert not off["taken"], off
