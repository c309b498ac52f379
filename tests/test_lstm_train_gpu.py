"""GPU: training the two-layer LSTM question encoder in HIP (ops.lstm_train_forward / _backward, LstmTrainFunction, TwoLSTM.use_hip_bptt,
train.py --hip_2lstm_train) against the fp64 restatement tests/lstm_train_ref.py.

Bound: q within 1e-4 absolute; every gradient within 1e-4 of its fp64 tensor's max, the project's standing gradient bound; a tensor whose
fp64 max is 0 must be exactly 0.  Shapes: a T = 1 row, the ragged case of the fixture's kind (an all-padding row, a zero inside a
question), every length 1 over more than one row tile, and the real widths; tests/test_lstm_edges_gpu.py has the eight edge shapes."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG
from lstm_train_ref import GRADS, lstm_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
WGRADS = tuple(k for k in GRADS if k != "E")

#         name       emb    H     B   T
SHAPES = {"one":      (22,   48,   3,  1),     # T = 1: no recurrent product in either layer
          "ragged":   (22,  100,   5,  7),     # nonzero counts {0, 1, 3, 6, 7}: an all-padding row (T steps on E[0]), a zero inside a question
          "all1":     (40,  100,  70, 26),     # every length 1: no recurrent product runs; more than one row tile, ragged
          "real":     (620, 1200,  40, 26)}    # the real widths, lengths 3..26
V = 50


def make_wids(name, B, T, rng):
    if name == "one":
        lens = [1] * B
    elif name == "ragged":
        lens = [0, 1, 3, 7, 7]
    elif name == "all1":
        lens = [1] * B
    else:
        lens = list(rng.integers(3, T, size=B))
        lens[: 24] = range(3, 27)                              # 3..26, each at least once
    wids = np.zeros((B, T), np.int64)
    for b, n in enumerate(lens):
        wids[b, :n] = rng.integers(1, V + 1, size=n)
    if name == "ragged":
        wids[3, 4] = 0                                         # a zero inside the question: 6 nonzero ids, stepped over t < 6
    return wids


def make_encoder(emb, H, seed):
    from vqa.models.seq2vec import TwoLSTM
    torch.manual_seed(seed)
    enc = TwoLSTM(["w%d" % i for i in range(V)], emb, H).eval()
    with torch.no_grad():
        enc.embedding.weight.mul_(0.5)
        enc.embedding.weight[0] = torch.randn(emb) * 0.5       # the padding row is READ, never assumed zero
    return enc


def tensors_of(enc):
    return [enc.embedding.weight.detach()] + [getattr(r, k).detach() for r in (enc.rnn_0, enc.rnn_1) for k in WKEYS]


def ref_of(enc, wids, dq_out):
    ts = [t.cpu().numpy() for t in tensors_of(enc)]
    return lstm_train(wids, ts[0], tuple(ts[1:5]), tuple(ts[5:9]), dq_out)


def hip_step(enc, wids, dq_out, want_dE=True, dE=None):
    """-> (q, grads) of one forward + backward through the ops layer, as numpy."""
    from neuralcx import ops
    lw = ops.lstm_train_weights(*tensors_of(enc))
    w = torch.from_numpy(wids).to(DEV)
    ws = ops.lstm_train_workspace(w.shape[0], w.shape[1], lw, DEV)
    q = ops.lstm_train_forward(w, lw, ws)
    g = ops.lstm_train_backward(w, lw, ws, torch.from_numpy(dq_out).to(DEV), want_dE=want_dE, dE=dE)
    ops.check_gru_ids(device=DEV)
    return q.cpu().numpy(), {k: (None if v is None else v.cpu().numpy()) for k, v in g.items()}


_CASES = {}


def case(name):
    """(encoder on the device, wids, dq_out, fp64 reference, q and gradients of the HIP path) -- computed once, shared, never modified."""
    if name not in _CASES:
        emb, H, B, T = SHAPES[name]
        enc = make_encoder(emb, H, seed=sorted(SHAPES).index(name))
        rng = np.random.default_rng(7)
        wids = make_wids(name, B, T, rng)
        dq_out = rng.standard_normal((B, 2 * H)).astype(np.float32)
        ref = ref_of(enc, wids, dq_out)
        enc = enc.to(DEV)
        q, g = hip_step(enc, wids, dq_out)
        _CASES[name] = (enc, wids, dq_out, ref, q, g)
    return _CASES[name]


def check_grads(tag, got, ref, keys=GRADS):
    for k in keys:
        m, err = float(np.abs(ref[k]).max()), float(np.abs(got[k] - ref[k]).max())
        print("%s d%s: max|hip - fp64| = %.3e, max|fp64| = %.3e (%.2e of it)" % (tag, k, err, m, err / m if m else 0.0))
        assert got[k].shape == ref[k].shape and got[k].dtype == np.float32 and np.isfinite(got[k]).all(), k
        if m == 0.0:
            assert not got[k].any(), k
        else:
            assert err <= TOL * m, k


@pytest.mark.parametrize("name", list(SHAPES))
def test_forward_is_bit_equal_to_lstm_encode(name):
    from neuralcx import ops
    enc, wids, _, ref, q, _ = case(name)
    plain = ops.lstm_encode(torch.from_numpy(wids).to(DEV), ops.lstm_weights(enc)).cpu().numpy()
    err = float(np.abs(q - ref["q"]).max())
    print("%s dims %s q: max|hip - fp64| = %.3e" % (name, SHAPES[name], err))
    assert np.array_equal(q, plain)
    assert err <= TOL


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_match_fp64(name):
    enc, wids, _, ref, _, g = case(name)
    if name in ("one", "all1"):                                # no recurrent product ran: exactly 0 (checked in check_grads) ...
        assert not ref["w_hh0"].any() and not ref["w_hh1"].any() and ref["w_ih1"].any()
        assert not g["w_hh0"].any() and not g["w_hh1"].any() and g["w_ih1"].any()     # ... and dW_ih^1 is not
    check_grads(name, g, ref)
    assert not g["E"][0].any()                                 # the padding row, whatever read E[0] in the forward


def test_planted_rows_of_the_ragged_case():
    """The all-padding row (T steps on E[0]) and the row with a zero inside, each isolated by a one-hot dq_out."""
    enc, wids, dq_out, _, _, _ = case("ragged")
    assert not wids[0].any() and wids[3, 4] == 0 and wids[3, 5] != 0
    for b in (0, 3):
        d = np.zeros_like(dq_out)
        d[b] = dq_out[b]
        ref = ref_of(enc, wids, d)
        assert ref["w_ih0"].any() and ref["b_hh1"].any() and ref["w_hh0"].any() and ref["w_hh1"].any()
        _, g = hip_step(enc, wids, d)
        check_grads("ragged row %d" % b, g, ref)
        assert not g["E"][0].any()
        assert ref["E"].any() == (b == 3)                      # row 0 read only E[0]: its weight gradients count, its dE does not


def test_device_pack_equals_the_layout_restatement():
    from neuralcx import ops
    for name in ("ragged", "one"):
        enc = case(name)[0]
        ts = tensors_of(enc)
        lw = ops.lstm_train_weights(*ts)
        assert torch.equal(lw.packed_t, ops.lstm_pack_t_layout(ts[1], ts[2], ts[5], ts[6]))
        assert torch.equal(lw.packed, ops.lstm_weights(enc).packed)
        for got, want in zip(ops.lstm_unpack_t_layout(lw.packed_t, lw.emb, lw.H), (ts[1], ts[2], ts[5], ts[6])):
            assert torch.equal(got, want)


def test_null_de_leaves_the_other_gradients_bit_identical():
    for name in ("ragged", "all1"):
        enc, wids, dq_out, _, _, g = case(name)
        _, g0 = hip_step(enc, wids, dq_out, want_dE=False)
        assert g0["E"] is None
        for k in WGRADS:
            assert np.array_equal(g0[k], g[k]), (name, k)


def test_bit_identical_from_run_to_run():
    for name in ("real", "ragged"):
        enc, wids, dq_out, _, q, g = case(name)
        q2, g2 = hip_step(enc, wids, dq_out)
        assert np.array_equal(q2, q)
        for k in GRADS:
            assert np.array_equal(g2[k], g[k]), (name, k)


def test_out_of_range_word_id_raises_and_writes_nowhere_outside_de():
    from neuralcx import ops
    enc, wids, dq_out, _, _, g = case("ragged")
    emb, H, B, T = SHAPES["ragged"]
    for bad in (V + 1, -3, 2 ** 30):
        w = wids.copy()
        w[2, 1] = bad
        mine = make_encoder(emb, H, seed=sorted(SHAPES).index("ragged")).to(DEV).train()
        mine.use_hip_bptt = True
        out = mine(torch.from_numpy(w).to(DEV))                # through the module: the flag is raised by the forward
        with pytest.raises(IndexError):
            ops.check_gru_ids(device=DEV)
        ops.check_gru_ids(device=DEV)                          # cleared
        assert out.requires_grad
        # the backward never uses the id as an address: a guard band around dE stays as it was
        guard = torch.full((3 * (V + 1), emb), 7.5, device=DEV)
        dE = guard[V + 1:2 * (V + 1)]
        lw = ops.lstm_train_weights(*tensors_of(enc))
        wd = torch.from_numpy(w).to(DEV)
        ws = ops.lstm_train_workspace(B, T, lw, DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.lstm_train_forward(wd, lw, ws, bad_flag=flag)
        got = ops.lstm_train_backward(wd, lw, ws, torch.from_numpy(dq_out).to(DEV), dE=dE)
        assert int(flag.item()) == 1 and got["E"].data_ptr() == dE.data_ptr()
        assert bool((guard[:V + 1] == 7.5).all()) and bool((guard[2 * (V + 1):] == 7.5).all())
        assert bool(torch.isfinite(dE).all()) and not bool(dE[0].any())


def _module_pair(name):
    emb, H, _, _ = SHAPES[name]
    seed = sorted(SHAPES).index(name)
    a, b = (make_encoder(emb, H, seed).to(DEV).train() for _ in range(2))
    a.use_hip_bptt = True
    return a, b


def test_module_agrees_with_the_torch_path(monkeypatch):
    """Training mode, dropout p = 0.3 live on both halves, one seed: the same masks (identical zero patterns), every .grad within 1e-4 of
    torch's max, one LstmTrainFunction call."""
    from neuralcx import vqa_train
    _, wids, dq_out, _, _, _ = case("ragged")
    hip, ref = _module_pair("ragged")
    calls = []
    real = vqa_train.LstmTrainFunction.apply
    monkeypatch.setattr(vqa_train.LstmTrainFunction, "apply", staticmethod(lambda *a, **k: (calls.append(1), real(*a, **k))[1]))
    w, d = torch.from_numpy(wids).to(DEV), torch.from_numpy(dq_out).to(DEV)
    outs = []
    for m in (hip, ref):
        torch.manual_seed(11)                                  # the same dropout masks on the two halves for both
        out = m(w)
        (out * d).sum().backward()
        outs.append(out.detach())
    assert calls == [1] and ref.use_hip_bptt is False
    assert bool((outs[0] == 0).any()) and bool(((outs[0] == 0) == (outs[1] == 0)).all())
    assert float((outs[0] - outs[1]).abs().max()) <= TOL * float(outs[1].abs().max())
    for (n, p), (_, r) in zip(hip.named_parameters(), ref.named_parameters()):
        err, mx = float((p.grad - r.grad).abs().max()), float(r.grad.abs().max())
        print("%s: max|hip - torch| = %.3e of max %.3e" % (n, err, mx))
        assert mx > 0 and err <= TOL * mx, n
    with torch.no_grad():                                      # grad mode off: what the module did before (no training call)
        hip.eval()
        hip(w)
    assert calls == [1]


def test_fixed_embedding_gets_no_gradient_and_leaves_the_others_bit_identical():
    _, wids, dq_out, _, _, g = case("ragged")
    hip, _ = _module_pair("ragged")
    hip.p_drop = 0.0                                           # q itself, so that the gradients are the case's
    hip.embedding.weight.requires_grad_(False)
    out = hip(torch.from_numpy(wids).to(DEV))
    (out * torch.from_numpy(dq_out).to(DEV)).sum().backward()
    assert hip.embedding.weight.grad is None
    for l, r in enumerate((hip.rnn_0, hip.rnn_1)):
        for s, k in zip(("w_ih", "w_hh", "b_ih", "b_hh"), WKEYS):
            assert np.array_equal(getattr(r, k).grad.cpu().numpy(), g["%s%d" % (s, l)]), (l, k)


def test_optimizer_step_invalidates_the_pack_cache():
    from neuralcx import ops
    _, wids, dq_out, _, q0, _ = case("ragged")
    hip, _ = _module_pair("ragged")
    hip.p_drop = 0.0
    w, d = torch.from_numpy(wids).to(DEV), torch.from_numpy(dq_out).to(DEV)
    opt = torch.optim.SGD(hip.parameters(), lr=0.05)
    out = hip(w)
    assert np.array_equal(out.detach().cpu().numpy(), q0)
    first = hip.__dict__["_hip_lstm_train"][1]
    assert hip(w) is not None and hip.__dict__["_hip_lstm_train"][1] is first   # cached while nothing changes
    (out * d).sum().backward()
    opt.step()
    got = hip(w).detach()
    assert hip.__dict__["_hip_lstm_train"][1] is not first
    hip.eval()
    with torch.no_grad():
        fresh = hip(w)                                          # ops.lstm_encode on a fresh pack
    assert torch.equal(got, fresh)
    assert float((got.cpu() - torch.from_numpy(q0)).abs().max()) > 100 * TOL    # the step moved q: a stale pack would show


def test_valid_calls_through_the_c_entries_run_and_bad_ones_return_minus_one():
    import ctypes as C
    from neuralcx import _lib, ops
    enc, wids, dq_out, _, _, g0 = case("ragged")
    emb, H, B, T = SHAPES["ragged"]
    lw = ops.lstm_train_weights(*tensors_of(enc))
    w = torch.from_numpy(wids).to(DEV).to(torch.int32)
    ws = ops.lstm_train_workspace(B, T, lw, DEV)
    p, have = ops._ws_ptr(ws)
    L = _lib.lib()
    n = L.ncx_lstm2_train_workspace_bytes(B, T, emb, H)        # the exact size: one byte less is short
    assert 0 < n <= have
    q, d = torch.empty(B, 2 * H, device=DEV), torch.from_numpy(dq_out).to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    shapes = {"w_ih0": (4 * H, emb), "w_hh0": (4 * H, H), "w_ih1": (4 * H, H), "w_hh1": (4 * H, H)}
    g = [torch.empty(shapes.get(k, (4 * H,)), device=DEV) for k in WGRADS]
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def fwd(T_=T, ws_=p, n_=n, wids_=ptr(w)):
        return L.ncx_lstm2_train_forward(wids_, B, T_, ptr(lw.E), lw.V1, emb, H, ptr(lw.packed), ws_, n_, ptr(q), ptr(flag), None)

    def bwd(T_=T, ws_=p, n_=n, d_=ptr(d)):
        return L.ncx_lstm2_train_backward(ptr(w), B, T_, ptr(lw.E), lw.V1, emb, H, ptr(lw.packed_t), ws_, n_, d_, *[ptr(t) for t in g], None, None)

    for f in (fwd, bwd):
        assert f(T_=65) == -1 and f(n_=n - 1) == -1 and f(ws_=C.c_void_p(p.value + 16)) == -1 and f(ws_=None) == -1
    assert fwd(wids_=None) == -1 and bwd(d_=None) == -1
    assert fwd() == 0 and bwd() == 0                           # ... and the same calls with valid arguments run, on the exact size
    torch.cuda.synchronize()
    for k, t in zip(WGRADS, g):
        assert np.array_equal(t.cpu().numpy(), g0[k]), k


TINY_YAML = """
logs: {dir_logs: %s}
vqa: {nans: 40, maxlength: 8}
coco: {}
model:
  arch: MutanNoAtt
  seq2vec: {arch: 2-lstm, emb_size: 16, hidden_size: 24, dropout: 0.25, fixed_emb: False}
  fusion: {dim_v: 64, dim_q: 48, dim_hv: 32, dim_hq: 32, dim_mm: 24, R: 3, activation_v: tanh, activation_q: tanh, dropout_v: 0.1, dropout_q: 0.1, dropout_hv: 0, dropout_hq: 0}
  classif: {dropout: 0.1}
optim: {lr: 0.01, batch_size: 16, epochs: 1}
"""
CLI_ARGS = ["--synthetic", "--syn_examples", "384", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0", "--epochs", "1"]


def test_cli_trains_the_2lstm_encoder_in_hip(tmp_path, capsys):
    """train.py --synthetic --hip_2lstm_train --epochs 1 on 384 examples (21 steps of 16) of a tiny 2-lstm YAML: the route line names the
    flag, the losses are finite, the checkpoint loads strictly into a plain TwoLSTM and the encoder's weights moved.
    A single step's training loss is noise at this size, so "falls over the epoch" is measured on the validation split, before the epoch
    against after it, and it IS asserted: the same loop on the torch modules (--no_hip, on a CPU) goes from 3.690 to 3.660 under the
    default seed and falls under seeds 1, 2 and 3 as well (3.674 -> 3.615, 3.696 -> 3.586, 3.680 -> 3.626).  The existing refusal of
    --hip_seq2vec_train for this encoder is checked once more at the end."""
    import importlib.util
    from vqa.models.seq2vec import TwoLSTM
    spec = importlib.util.spec_from_file_location("vqa_train_cli_lstm_gpu", os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    y = tmp_path / "o.yaml"
    y.write_text(TINY_YAML % str(tmp_path / "logs"))
    losses, before, start = [], [], {}
    real_step, real_epoch = cli.Trainer._step, cli.Trainer.run_epoch

    def step(self, split, sel, train):
        r = real_step(self, split, sel, train)
        if train:
            losses.append(r[0])
        return r

    def run_epoch(self, epoch):
        before.append(self.evaluate()["loss"])
        start.update({k: v.detach().clone() for k, v in self.model.seq2vec.state_dict().items()})
        return real_epoch(self, epoch)
    cli.Trainer._step, cli.Trainer.run_epoch = step, run_epoch
    r = cli.main(["--path_opt", str(y)] + CLI_ARGS + ["--hip_2lstm_train"])
    out = capsys.readouterr().out
    assert "--hip_2lstm_train" in out and "2-lstm question encoder: HIP forward + backward through time" in out
    enc = r["trainer"].model.seq2vec
    assert type(enc) is TwoLSTM and enc.use_hip_bptt is True and TwoLSTM.use_hip_bptt is False
    ls = [float(x) for x in losses]
    after = r["history"][0]["val"]["loss"]
    print("train losses", ["%.3f" % x for x in ls], "val before %.4f after %.4f" % (before[0], after))
    assert len(ls) >= 8 and all(np.isfinite(ls)) and np.isfinite(after) and np.isfinite(before[0])
    assert after < before[0]
    sd = torch.load(str(tmp_path / "logs" / "best_model.pth.tar"))
    plain = TwoLSTM(["w%d" % i for i in range(30)], 16, 24)
    plain.load_state_dict({k[len("seq2vec."):]: v for k, v in sd.items() if k.startswith("seq2vec.")}, strict=True)
    assert plain.use_hip_bptt is False
    for k, v in enc.state_dict().items():                      # every tensor of the encoder moved (row 0 of E aside, it gets no gradient)
        assert float((v - start[k]).abs().max()) > 0, k
    assert torch.equal(enc.state_dict()["embedding.weight"][0], start["embedding.weight"][0])
    with pytest.raises(SystemExit):                            # the GRU's flag keeps refusing this encoder
        cli.main(["--path_opt", str(y)] + CLI_ARGS + ["--hip_seq2vec_train"])
