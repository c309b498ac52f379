"""GPU: the frozen VQA producers (ncx_vqa_forward: csrc/ncx_vqa.hip with k_mutan_fold of csrc/ncx_mutan.hip or the generic engine's FOLD chain;
ncx_mlb_forward: csrc/ncx_mlb.hip) at the edge shapes of tests/producers_ref.py.  Every case proves its route first (ncx_vqa_route /
ncx_mlb_route: the function the launcher asks), runs on a workspace filled with 0xFF into NaN-filled outputs that lie between sentinel
margins (a wrong row of the K + 1 row split lands in a margin or leaves a NaN), and compares every stage -- the intermediates through
ops.vqa_ws_view -- element by element with the fp64 restatement of that stage on the device's own inputs, under c * 2^-24 * S of
producers_ref.  A second run gives the same bits.  Each case prints its ratios: `pytest -s` gives the figures of
profiles/producer_edges.json."""
import numpy as np
import pytest
import torch

import producers_ref as P
from helpers import dev

pytestmark = pytest.mark.gpu

MARGIN = 256                    # floats on either side of every output
SENTINEL = 12345.0
_REFS = {}


def _reference(case):
    """Inputs and restatement of a shape, built once and shared by the cases that run it; never modified."""
    key = P.shape_key(case)
    if key not in _REFS:
        state, table, idx, q_emb = P.build(case)
        ref = (P.MutanRef if case["kind"] == "mutan" else P.MlbRef)(state, case)
        v_rows = table[torch.from_numpy(idx.reshape(-1).astype(np.int64))]
        _REFS[key] = (state, table, idx, q_emb, v_rows, ref)
    return _REFS[key]


def _weights(case, state):
    from neuralcx import ops
    t = {k: v.to(dev()).contiguous() for k, v in P.stacked(state, case).items()}
    a = P.ACT_CODE[case["act"]]
    if case["kind"] == "mutan":
        return ops.MutanWeights.from_tensors(t, R=case["R"], act_v=a, act_q=a)
    return ops.MlbWeights.from_tensors(t, act_v=a, act_q=a, act_c=P.ACT_CODE[case["act_c"]])


def _device_table(case, table, idx):
    """The feature table and img_idx on the device.  The case beyond 4 GiB: an uninitialised table of the full size with only the rows
    used filled in, and the ids of those rows."""
    rows = P.device_rows(case)
    if rows is None:
        return table.to(dev()), torch.from_numpy(idx).to(dev())
    feats = torch.empty(case["n_img"], case["dv"], dtype=torch.float32, device=dev())
    feats[torch.from_numpy(rows.astype(np.int64)).to(dev())] = table.to(dev())
    return feats, torch.from_numpy(case["ids"]).to(dev())


def _guarded(*shape):
    """A NaN-filled contiguous tensor inside a larger buffer, sentinel margins on both sides -> (buffer, view)."""
    n = int(np.prod(shape))
    buf = torch.full((n + 2 * MARGIN,), SENTINEL, dtype=torch.float32, device=dev())
    buf[MARGIN:MARGIN + n] = float("nan")
    return buf, buf[MARGIN:MARGIN + n].view(*shape)


def _check_route(case, d, mw):
    from neuralcx import ops
    got = ops.vqa_route(d, mw)
    want = case["route"]
    mismatch = {k: (got[k], v) for k, v in want.items() if got[k] != v}
    if mismatch and case["cu_dependent"]:
        pytest.skip("%s: the route depends on the CU count; this chip gives (got, wanted) %r" % (case["id"], mismatch))
    assert not mismatch, (case["id"], mismatch, got)
    return got


def _within(case, name, got, ref_S, worst):
    ref, S = ref_S
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), (case["id"], name, "non-finite: a NaN of the workspace or of the output buffer survived")
    c = P.bound_c(case["group"])
    r = P.ratio(got, ref, S)
    print("ratio %s %s %.3f (c %.1f)" % (case["id"], name, r, c))
    bad = np.argwhere(np.abs(got - ref) > c * P.U24 * S)
    assert bad.size == 0, (case["id"], name, "elements over the bound: %d, first (row, col) %s, ratio %.3g, c %.1f" % (len(bad), bad[0].tolist(), r, c))
    return max(worst, r)


def _run(case):
    """Hooks are set by the caller.  One forward, checked stage by stage; a second one, bit-identical.  -> the worst ratio."""
    from neuralcx import ops
    state, table, idx, q_emb, v_rows, ref = _reference(case)
    B, K1, dz, A = case["B"], case["K1"], case["dz"], case["A"]
    mw = _weights(case, state)
    feats, idx_d = _device_table(case, table, idx)
    q_d = q_emb.to(dev())
    d = ops.vqa_dims(B, K1, case["dv"], case["dq"], feats.shape[0], mw)
    route = _check_route(case, d, mw)                       # first: a case that fell onto another route proves nothing
    ws = ops.vqa_workspace(d, mw, dev())                     # (after the hooks)
    ws.fill_(0xFF)
    bufs, outs = zip(*[_guarded(*s) for s in ((B, A), (B, dz), (B, K1 - 1, A), (B, K1 - 1, dz))])
    res = ops.vqa_forward(feats, idx_d, q_d, mw, want_a_orig=case["a_orig"], ws=ws, out=outs)
    torch.cuda.synchronize()
    assert res[0] is (outs[0] if case["a_orig"] else None) and all(r is o for r, o in zip(res[1:], outs[1:]))
    for name, buf, o in zip(("a_orig", "z_orig", "a_knns", "z_knns"), bufs, outs):
        b = buf.cpu().numpy()
        assert (b[:MARGIN] == SENTINEL).all() and (b[MARGIN + o.numel():] == SENTINEL).all(), (case["id"], name, "a margin was written")
    a_o, z_o, a_k, z_k = (o.cpu().numpy() for o in outs)
    if not case["a_orig"]:
        assert np.isnan(a_o).all(), (case["id"], "a_orig was not asked for")
    view = lambda n: ops.vqa_ws_view(d, mw, ws, n).cpu().numpy()
    worst = 0.0
    xq = view("xq")
    worst = _within(case, "xq", xq, ref.xq(q_emb), worst)
    z_dev = np.concatenate([z_o[:, None, :], z_k], 1).reshape(B * K1, dz)
    if case["kind"] == "mutan":
        hq, xv = view("hq"), view("xv")
        worst = _within(case, "hq", hq, ref.hq(xq), worst)
        worst = _within(case, "xv", xv, ref.xv(v_rows), worst)
        worst = _within(case, "z", z_dev, ref.z(xv, hq), worst)
        ck, co = z_k, z_o
    else:
        if route["main_v"]:
            worst = _within(case, "z(feats, xq)", z_dev, ref.z_fused(v_rows, xq), worst)
        else:
            xv = view("xv")
            worst = _within(case, "xv", xv, ref.xv(v_rows), worst)
            worst = _within(case, "z", z_dev, ref.z(xv, xq), worst)
        ck, co = z_k, z_o
        if case["act_c"]:
            ck, co = view("t_knns"), view("t_orig")
            worst = _within(case, "t_knns", ck, ref.t(z_k.reshape(-1, dz)), worst)
            worst = _within(case, "t_orig", co, ref.t(z_o), worst)
    worst = _within(case, "a_knns", a_k.reshape(-1, A), ref.a(ck.reshape(-1, dz)), worst)
    if case["a_orig"]:
        worst = _within(case, "a_orig", a_o, ref.a(co), worst)
    # again, on the workspace the first run left: the same bits
    first = [o.clone() for o in outs]
    ops.vqa_forward(feats, idx_d, q_d, mw, want_a_orig=case["a_orig"], ws=ws, out=outs)
    torch.cuda.synchronize()
    for name, f, o in zip(("a_orig", "z_orig", "a_knns", "z_knns"), first, outs):
        assert torch.equal(f.view(torch.int32), o.view(torch.int32)), (case["id"], name, "the second run differs")
    return worst


def _set_hooks(case, monkeypatch):
    if case["env"]:
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        for k, v in case["env"].items():
            monkeypatch.setenv(k, v)


@pytest.mark.parametrize("case_id", [c["id"] for c in P.CASES if c["group"] != "big"])
def test_edge_case_against_fp64(case_id, monkeypatch):
    """Groups fold (k_mutan_fold), engine (the generic engine's FOLD chain), routes (x_v and the classifier on either engine), mlb."""
    case = P.BY_ID[case_id]
    _set_hooks(case, monkeypatch)
    _run(case)


def test_table_beyond_4_gib():
    """A Mutan feature table of 4.3 GB (dv = 2048, 525 000 images) with ids whose rows start past 2^30, 2^31 and 2^32 bytes: the route
    entry reports the generic engine's gather (64-bit addresses) for x_v, and every stage meets its bound."""
    case = P.BY_ID["big-table-beyond-4GiB"]
    free, _ = torch.cuda.mem_get_info()
    assert free > case["n_img"] * case["dv"] * 4 + (1 << 30), "the table of this case needs 4.3 GB of device memory"
    _run(case)
    torch.cuda.empty_cache()
