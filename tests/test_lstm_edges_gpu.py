"""GPU: the two-layer LSTM encoder's training kernels (ncx_lstm2_train_forward / _backward) on the edge cases of tests/lstm_edge_cases.py
-- widths that are no multiple of 4, dims of 1, one past every tile and k-step, B > 256, T = 64, a second pass of the embedding gradient,
n_t exactly on and one over the row tile and the k-step -- against the fp64 restatements tests/lstm_ref.py and tests/lstm_train_ref.py,
and on workspaces whose previous contents must not matter.

Bounds, the project's standing ones: q within 1e-4 absolute; every gradient within 1e-4 of its fp64 tensor's max; a tensor whose fp64
max is 0 exactly 0; dE[0] exactly 0.  tests/test_lstm_edges_cpu.py shows that losing any one half-row breaks a bound 100 times over.
torch's own fp32 nn.LSTM forward and backward on the device are printed next to the HIP errors, for the record; nothing is asserted on
them."""
import ctypes as C

import numpy as np
import pytest
import torch

from lstm_edge_cases import CASES, V, full_wids, make, plan
from lstm_train_ref import GRADS, lstm_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
GKEYS = ("w_ih0", "w_hh0", "b_ih0", "b_hh0", "w_ih1", "w_hh1", "b_ih1", "b_hh1", "E")     # the C entry's order of the gradient buffers
STALE = ("odd", "over64", "long", "steps")                      # the cases of the workspace tests
TORCH_KEY = {"E": ("embedding", "weight")}
TORCH_KEY.update({"%s%d" % (s, l): ("rnn_%d" % l, k) for l in (0, 1) for s, k in zip(("w_ih", "w_hh", "b_ih", "b_hh"), WKEYS)})


def make_encoder(name):
    """A TwoLSTM holding the recipe's weights (the module the product path packs its weights from)."""
    from vqa.models.seq2vec import TwoLSTM
    emb, H, _, _ = CASES[name]
    _, E, l0, l1, _ = make(name)
    enc = TwoLSTM(["w%d" % i for i in range(V)], emb, H).eval()
    sd = {"embedding.weight": torch.from_numpy(E)}
    sd.update({"rnn_%d.%s" % (l, k): torch.from_numpy(a) for l, layer in enumerate((l0, l1)) for k, a in zip(WKEYS, layer)})
    enc.load_state_dict(sd, strict=True)
    return enc


def tensors_of(enc):
    return [enc.embedding.weight.detach()] + [getattr(r, k).detach() for r in (enc.rnn_0, enc.rnn_1) for k in WKEYS]


def to_np(q, g):
    return q.cpu().numpy(), {k: (None if v is None else v.cpu().numpy()) for k, v in g.items()}


def hip_step(lw, wids, dq_out, ws=None, want_dE=True):
    """-> (q, grads) of one forward + backward through the ops layer, as numpy; `ws`: the caller's workspace, used as it is."""
    from neuralcx import ops
    w = torch.from_numpy(wids).to(DEV)
    if ws is None:
        ws = ops.lstm_train_workspace(w.shape[0], w.shape[1], lw, DEV)
    q = ops.lstm_train_forward(w, lw, ws)
    g = ops.lstm_train_backward(w, lw, ws, torch.from_numpy(dq_out).to(DEV), want_dE=want_dE)
    ops.check_gru_ids(device=DEV)
    return to_np(q, g)


def torch_step(name, wids, dq_out):
    """torch's own fp32 path of the same module on the device (nn.Embedding + tanh + two nn.LSTMs + autograd; in training mode, which
    the device RNN backward insists on, with the dropout on q set to 0)."""
    m = make_encoder(name).to(DEV).train()
    m.p_drop = 0.0
    assert m.use_hip_bptt is False
    out = m(torch.from_numpy(wids).to(DEV))
    (out * torch.from_numpy(dq_out).to(DEV)).sum().backward()
    return to_np(out.detach(), {k: getattr(getattr(m, a), b).grad for k, (a, b) in TORCH_KEY.items()})


_CASES = {}


def case(name):
    """(encoder on the device, its training weights, wids, dq_out, fp64 reference, q and gradients of the HIP path) -- computed once,
    shared, never modified."""
    if name not in _CASES:
        from neuralcx import ops
        wids, E, l0, l1, dq_out = make(name)
        ref = lstm_train(wids, E, l0, l1, dq_out)
        enc = make_encoder(name).to(DEV)
        lw = ops.lstm_train_weights(*tensors_of(enc))
        q, g = hip_step(lw, wids, dq_out)
        _CASES[name] = (enc, lw, wids, dq_out, ref, q, g)
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
    enc, lw, wids, dq_out, ref, q, g = case(name)
    plain = ops.lstm_encode(torch.from_numpy(wids).to(DEV), ops.lstm_weights(enc)).cpu().numpy()
    ops.check_gru_ids(device=DEV)
    tq, tg = torch_step(name, wids, dq_out)
    err, terr = float(np.abs(q - ref["q"]).max()), float(np.abs(tq - ref["q"]).max())
    print("%s dims %s q: max|hip - fp64| = %.3e, max|q| = %.3f; torch fp32: %.3e" % (name, CASES[name], err, float(np.abs(ref["q"]).max()), terr))
    assert q.shape == ref["q"].shape and q.dtype == np.float32 and np.isfinite(q).all() and float(np.abs(q).max()) < 1.0
    assert np.array_equal(q, plain)                             # the training forward is lstm_encode, bit for bit
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
        # input rows >= 256 are the plan's second trip; the all-padding row 299 has length T here and sorts to the front like row 260;
        # sorted position 280 holds a short row of the fifth row tile
        b64, b0, short = 260, 299, int(perm[280])
        assert raw[b64] == 64 and raw[b0] == 0 and lens[b0] == 64 and min(b64, b0) >= 256 and max(pos(b64), pos(b0)) < n_t[63]
        assert 1 <= lens[short] < 10
        return [b64, b0, short]
    if name == "steps":
        b = int(perm[64])
        assert lens[b] == 2 and (lens == 2).sum() == 1 and n_t[1] == 65 and n_t[2] == 64     # alone in the second row tile, for two steps
        return [b]
    b = int(perm[64])                                            # over64: the one row of the second row tile
    assert name == "over64" and len(perm) == 65 and n_t[1] == 65 and n_t[2] == 64 and lens[b] == 2
    return [b]


@pytest.mark.parametrize("name", ["long", "steps", "over64"])
def test_planted_rows_isolated_by_a_one_hot_dq_out_on_each_half(name):
    enc, lw, wids, dq_out, _, _, _ = case(name)
    emb, H, B, T = CASES[name]
    _, E, l0, l1, _ = make(name)
    for b in _planted(name):
        for half in (0, 1):
            d = np.zeros_like(dq_out)
            d[b, half * H:(half + 1) * H] = dq_out[b, half * H:(half + 1) * H]
            ref = lstm_train(wids, E, l0, l1, d)
            assert ref["w_ih0"].any() and ref["b_hh0"].any()
            assert ref["b_hh1"].any() == (half == 1)            # the layer-0 half never reaches layer 1
            q, g = hip_step(lw, wids, d)
            assert float(np.abs(q[b] - ref["q"][b]).max()) <= TOL
            check_grads("%s row %d half %d" % (name, b, half), g, ref)
            assert not g["E"][0].any()


@pytest.mark.parametrize("name", ["unit", "odd", "narrow", "wide_e", "over64"])
def test_device_packs_equal_the_layout_restatements(name):
    from neuralcx import ops
    enc, lw, _, _, _, _, _ = case(name)
    ts = tensors_of(enc)
    emb, H, _, _ = CASES[name]
    assert torch.equal(lw.packed_t, ops.lstm_pack_t_layout(ts[1], ts[2], ts[5], ts[6]))
    for got, want in zip(ops.lstm_unpack_t_layout(lw.packed_t, emb, H), (ts[1], ts[2], ts[5], ts[6])):
        assert torch.equal(got, want)
    assert torch.equal(lw.packed, ops.lstm_weights(enc).packed)


@pytest.mark.parametrize("name", STALE)
def test_training_does_not_depend_on_what_the_workspace_held(name):
    """(a) a zeroed workspace, (b) the same bytes all 0xFF (NaN as a float, -1 as an int), (c) a workspace a step of the same shape on
    other wids, every length T, has just used: rows beyond n_t, pad columns and steps past the longest question hold finite leftovers."""
    from neuralcx import ops
    _, lw, wids, dq_out, _, q0, g0 = case(name)
    emb, H, B, T = CASES[name]
    runs = {}
    for tag, byte in (("a", 0), ("b", 0xFF)):
        ws = ops.lstm_train_workspace(B, T, lw, DEV)
        ws.fill_(byte)
        runs[tag] = hip_step(lw, wids, dq_out, ws=ws)
    ws = ops.lstm_train_workspace(B, T, lw, DEV)
    ws.zero_()
    other = full_wids(name)
    qo, _ = hip_step(lw, other, dq_out, ws=ws)
    assert not np.array_equal(qo, runs["a"][0])                  # another step really ran there
    runs["c"] = hip_step(lw, wids, dq_out, ws=ws)
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
def test_backward_overwrites_every_gradient_element(name):
    """ncx_lstm2_train_backward through the C entry point into nine buffers pre-filled with NaN: nothing is accumulated into, nothing left."""
    from neuralcx import _lib, ops
    _, lw, wids, dq_out, _, _, g0 = case(name)
    emb, H, B, T = CASES[name]
    w = torch.from_numpy(wids).to(DEV)
    ws = ops.lstm_train_workspace(B, T, lw, DEV)
    ops.lstm_train_forward(w, lw, ws)
    ops.check_gru_ids(device=DEV)
    shapes = {"w_ih0": (4 * H, emb), "w_hh0": (4 * H, H), "w_ih1": (4 * H, H), "w_hh1": (4 * H, H), "E": (V + 1, emb)}
    g = {k: torch.full(shapes.get(k, (4 * H,)), float("nan"), device=DEV) for k in GKEYS}
    p, have = ops._ws_ptr(ws)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    w32, d = w.to(torch.int32), torch.from_numpy(dq_out).to(DEV)
    rc = _lib.lib().ncx_lstm2_train_backward(ptr(w32), B, T, ptr(lw.E), lw.V1, emb, H, ptr(lw.packed_t), p, have, ptr(d), *[ptr(g[k]) for k in GKEYS], None)
    torch.cuda.synchronize()
    assert rc == 0
    for k in GKEYS:
        got = g[k].cpu().numpy()
        assert np.isfinite(got).all() and np.array_equal(got, g0[k]), (name, k)


@pytest.mark.parametrize("name", ["wide_e", "long"])
def test_null_de_leaves_the_other_gradients_bit_identical(name):
    _, lw, wids, dq_out, _, _, g = case(name)
    _, g0 = hip_step(lw, wids, dq_out, want_dE=False)
    assert g0["E"] is None
    for k in GKEYS[:-1]:
        assert np.array_equal(g0[k], g[k]), (name, k)
