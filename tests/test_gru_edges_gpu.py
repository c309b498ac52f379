"""GPU: the GRU encoder's kernels (ncx_gru_encode, ncx_gru_train_forward / _backward) on the edge cases of tests/gru_edge_cases.py --
widths that are no multiple of 4, dims of 1, one past every tile and k-step, B > 256, T = 64, a second pass of the embedding gradient,
n_t exactly on and one over the row tile and the k-step -- against the fp64 restatements tests/gru_ref.py and tests/gru_train_ref.py,
and on workspaces whose previous contents must not matter.

Bounds, the project's standing ones: q within 1e-4 absolute; every gradient within 1e-4 of its fp64 tensor's max; a tensor whose fp64
max is 0 exactly 0; dE[0] exactly 0.  tests/test_gru_edges_cpu.py shows that losing any one row breaks a bound 100 times over.
torch's own fp32 nn.GRU forward and backward on the device are printed next to the HIP errors, for the record; nothing is asserted on
them."""
import ctypes as C

import numpy as np
import pytest
import torch

from gru_edge_cases import CASES, V, full_wids, make, plan
from gru_train_ref import GRADS, gru_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
GKEYS = ("w_ih", "w_hh", "b_ih", "b_hh", "E")                   # the C entry's order of the gradient buffers
STALE = ("odd", "narrow", "steps", "long")                      # the cases of the workspace tests


def make_encoder(name, dropout=0.25):
    """A GRUEncoder holding the recipe's weights (the module the product path packs its weights from)."""
    from vqa.models.seq2vec import GRUEncoder
    de, dq, _, _ = CASES[name]
    _, E, w_ih, w_hh, b_ih, b_hh, _ = make(name)
    enc = GRUEncoder(["w%d" % i for i in range(V)], dim_q=dq, dim_emb=de, dropout=dropout).eval()
    sd = {"embedding.weight": torch.from_numpy(E)}
    sd.update({"gru." + k: torch.from_numpy(a) for k, a in zip(WKEYS, (w_ih, w_hh, b_ih, b_hh))})
    enc.load_state_dict(sd, strict=True)
    return enc


def tensors_of(enc):
    return [enc.embedding.weight.detach()] + [getattr(enc.gru, k).detach() for k in WKEYS]


def to_np(q, g):
    return q.cpu().numpy(), {k: (None if v is None else v.cpu().numpy()) for k, v in g.items()}


def hip_step(gw, wids, dq_out, ws=None, want_dE=True):
    """-> (q, grads) of one forward + backward through the ops layer, as numpy; `ws`: the caller's workspace, used as it is."""
    from neuralcx import ops
    w = torch.from_numpy(wids).to(DEV)
    if ws is None:
        ws = ops.gru_train_workspace(w.shape[0], w.shape[1], gw, DEV)
    q = ops.gru_train_forward(w, gw, ws)
    g = ops.gru_train_backward(w, gw, ws, torch.from_numpy(dq_out).to(DEV), want_dE=want_dE)
    ops.check_gru_ids(device=DEV)
    return to_np(q, g)


def torch_step(name, wids, dq_out):
    """torch's own fp32 path of the same module on the device (nn.Embedding + nn.GRU + autograd; in training mode, which the device
    RNN backward insists on, with a dropout of 0)."""
    m = make_encoder(name, dropout=0.0).to(DEV).train()
    assert m.use_hip_train is False
    out = m(torch.from_numpy(wids).to(DEV))
    (out * torch.from_numpy(dq_out).to(DEV)).sum().backward()
    g = {"E": m.embedding.weight.grad}
    g.update({k: getattr(m.gru, w).grad for k, w in zip(("w_ih", "w_hh", "b_ih", "b_hh"), WKEYS)})
    return to_np(out.detach(), g)


_CASES = {}


def case(name):
    """(encoder on the device, its training weights, wids, dq_out, fp64 reference, q and gradients of the HIP path) -- computed once,
    shared, never modified."""
    if name not in _CASES:
        from neuralcx import ops
        wids, E, w_ih, w_hh, b_ih, b_hh, dq_out = make(name)
        ref = gru_train(wids, E, w_ih, w_hh, b_ih, b_hh, dq_out)
        enc = make_encoder(name).to(DEV)
        gw = ops.gru_train_weights(*tensors_of(enc))
        q, g = hip_step(gw, wids, dq_out)
        _CASES[name] = (enc, gw, wids, dq_out, ref, q, g)
    return _CASES[name]


def check_grads(tag, got, ref, other=None, keys=GRADS):
    for k in keys:
        m, err = float(np.abs(ref[k]).max()), float(np.abs(got[k] - ref[k]).max())
        line = "%s d%s: max|hip - fp64| = %.3e, max|fp64| = %.3e (%.2e of it)" % (tag, k, err, m, err / m if m else 0.0)
        if other is not None:
            oerr = float(np.abs(other[k] - ref[k]).max())
            line += "; torch fp32: %.3e (%.2e of it)" % (oerr, oerr / m if m else 0.0)
        print(line)
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
        if m == 0.0:
            assert not got[k].any(), k
        else:
            assert err <= TOL * m, k


@pytest.mark.parametrize("name", list(CASES))
def test_forward_and_gradients_match_fp64(name):
    from neuralcx import ops
    enc, gw, wids, dq_out, ref, q, g = case(name)
    plain = ops.gru_encode(torch.from_numpy(wids).to(DEV), ops.gru_weights(enc)).cpu().numpy()
    ops.check_gru_ids(device=DEV)
    tq, tg = torch_step(name, wids, dq_out)
    err, terr = float(np.abs(q - ref["q"]).max()), float(np.abs(tq - ref["q"]).max())
    print("%s dims %s q: max|hip - fp64| = %.3e, max|q| = %.3f; torch fp32: %.3e" % (name, CASES[name], err, float(np.abs(ref["q"]).max()), terr))
    assert q.shape == ref["q"].shape and q.dtype == np.float32 and np.isfinite(q).all() and float(np.abs(q).max()) < 1.0
    assert np.array_equal(q, plain)                             # the training forward is gru_encode, bit for bit
    assert err <= TOL
    check_grads(name, g, ref, other=tg)
    assert not g["E"][0].any()                                   # the padding row, whatever read E[0] in the forward


def _planted(name):
    """The rows a one-hot dq_out isolates, with their placement asserted from the plan restated in numpy."""
    wids = make(name)[0]
    lens, perm, n_t = plan(wids)
    raw = (wids != 0).sum(1)
    pos = lambda b: int(np.flatnonzero(perm == b)[0])
    if name == "long":
        # a row of length T sorts to the front whatever its input index: "position 256 or above" can hold for the empty row only
        b64, b0 = 260, 299
        assert raw[b64] == 64 and raw[b0] == 0 and min(b64, b0) >= 256 and pos(b0) >= 256 and pos(b64) < n_t[63]
        return [b64, b0]
    if name == "steps":
        b = int(perm[64])
        assert lens[b] == 2 and (lens == 2).sum() == 1 and n_t[1] == 65 and n_t[2] == 64     # alone in the second row tile, for two steps
        return [b]
    b = int(perm[64])                                            # over64: the one row of the second row tile
    assert name == "over64" and len(perm) == 65 and n_t[0] == 65 and n_t[1] == 64
    return [b]


@pytest.mark.parametrize("name", ["long", "steps", "over64"])
def test_planted_rows_isolated_by_a_one_hot_dq_out(name):
    enc, gw, wids, dq_out, _, _, _ = case(name)
    ts = [t.cpu().numpy() for t in tensors_of(enc)]
    for b in _planted(name):
        d = np.zeros_like(dq_out)
        d[b] = dq_out[b]
        ref = gru_train(wids, *ts, d)
        assert ref["w_ih"].any() and ref["b_hh"].any()
        q, g = hip_step(gw, wids, d)
        assert float(np.abs(q[b] - ref["q"][b]).max()) <= TOL
        check_grads("%s row %d" % (name, b), g, ref)
        assert not g["E"][0].any()


@pytest.mark.parametrize("name", ["unit", "odd", "narrow", "wide_e"])
def test_device_packs_equal_the_layout_restatements(name):
    from neuralcx import ops
    enc, gw, _, _, _, _, _ = case(name)
    ts = tensors_of(enc)
    de, dq, _, _ = CASES[name]
    assert torch.equal(gw.packed_t, ops.gru_pack_t_layout(ts[1], ts[2]))
    ih, hh = ops.gru_unpack_t_layout(gw.packed_t, de, dq)
    assert torch.equal(ih, ts[1]) and torch.equal(hh, ts[2])
    fw = ops.gru_weights(enc)
    assert torch.equal(gw.packed, fw.packed) and torch.equal(fw.packed, ops.gru_pack_layout(*ts[1:]))
    for got, want in zip(fw.unpack(), ts[1:]):
        assert torch.equal(got, want)


@pytest.mark.parametrize("name", STALE)
def test_training_does_not_depend_on_what_the_workspace_held(name):
    """(a) a zeroed workspace, (b) the same bytes all 0xFF (NaN as a float, -1 as an int), (c) a workspace a step of the same shape on
    other wids, every length T, has just used: rows beyond n_t, pad columns and steps past the longest question hold finite leftovers."""
    from neuralcx import ops
    _, gw, wids, dq_out, _, q0, g0 = case(name)
    de, dq, B, T = CASES[name]
    runs = {}
    for tag, byte in (("a", 0), ("b", 0xFF)):
        ws = ops.gru_train_workspace(B, T, gw, DEV)
        ws.fill_(byte)
        runs[tag] = hip_step(gw, wids, dq_out, ws=ws)
    ws = ops.gru_train_workspace(B, T, gw, DEV)
    ws.zero_()
    other = full_wids(name)
    qo, _ = hip_step(gw, other, dq_out, ws=ws)
    assert not np.array_equal(qo, runs["a"][0])                  # another step really ran there
    runs["c"] = hip_step(gw, wids, dq_out, ws=ws)
    qa, ga = runs["a"]
    assert np.array_equal(qa, q0)
    for tag in ("b", "c"):
        q, g = runs[tag]
        assert np.isfinite(q).all() and np.array_equal(q, qa), tag
        for k in GRADS:
            assert np.isfinite(g[k]).all() and np.array_equal(g[k], ga[k]), (name, tag, k)
    for k in GRADS:
        assert np.array_equal(ga[k], g0[k]), (name, k)


@pytest.mark.parametrize("name", STALE)
def test_encode_does_not_depend_on_what_the_workspace_held(name):
    """ncx_gru_encode through the C entry point on the caller's workspace: zeroed against all 0xFF, q pre-filled with NaN."""
    from neuralcx import _lib, ops
    enc, _, wids, _, _, q0, _ = case(name)
    de, dq, B, T = CASES[name]
    fw = ops.gru_weights(enc)
    L = _lib.lib()
    n = L.ncx_gru_workspace_bytes(B, T, de, dq)
    assert n > 0
    w = torch.from_numpy(wids).to(DEV).to(torch.int32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    got = []
    for byte in (0, 0xFF):
        ws = torch.empty(n + 256, dtype=torch.uint8, device=DEV)
        ws.fill_(byte)
        p, have = ops._ws_ptr(ws)
        q = torch.full((B, dq), float("nan"), device=DEV)
        assert L.ncx_gru_encode(ptr(w), B, T, ptr(fw.E), fw.V1, de, dq, ptr(fw.packed), p, have, ptr(q), ptr(flag), None) == 0
        torch.cuda.synchronize()
        got.append(q.cpu().numpy())
    assert int(flag.item()) == 0
    assert np.isfinite(got[0]).all() and np.isfinite(got[1]).all()
    assert np.array_equal(got[0], got[1]) and np.array_equal(got[0], q0)


@pytest.mark.parametrize("name", STALE)
def test_backward_overwrites_every_gradient_element(name):
    """ncx_gru_train_backward through the C entry point into five buffers pre-filled with NaN: nothing is accumulated into, nothing left."""
    from neuralcx import _lib, ops
    _, gw, wids, dq_out, _, _, g0 = case(name)
    de, dq, B, T = CASES[name]
    w = torch.from_numpy(wids).to(DEV)
    ws = ops.gru_train_workspace(B, T, gw, DEV)
    ops.gru_train_forward(w, gw, ws)
    ops.check_gru_ids(device=DEV)
    shapes = {"w_ih": (3 * dq, de), "w_hh": (3 * dq, dq), "b_ih": (3 * dq,), "b_hh": (3 * dq,), "E": (V + 1, de)}
    g = {k: torch.full(shapes[k], float("nan"), device=DEV) for k in GKEYS}
    p, have = ops._ws_ptr(ws)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    w32, d = w.to(torch.int32), torch.from_numpy(dq_out).to(DEV)
    rc = _lib.lib().ncx_gru_train_backward(ptr(w32), B, T, ptr(gw.E), gw.V1, de, dq, ptr(gw.packed_t), p, have, ptr(d), *[ptr(g[k]) for k in GKEYS], None)
    torch.cuda.synchronize()
    assert rc == 0
    for k in GKEYS:
        got = g[k].cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, g0[k]), (name, k)


@pytest.mark.parametrize("name", ["wide_e", "long"])
def test_null_de_leaves_the_other_gradients_bit_identical(name):
    _, gw, wids, dq_out, _, _, g = case(name)
    _, g0 = hip_step(gw, wids, dq_out, want_dE=False)
    assert g0["E"] is None
    for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
        assert np.array_equal(g0[k], g[k]), (name, k)
