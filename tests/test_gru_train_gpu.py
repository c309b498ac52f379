"""GPU: training the question encoder in HIP (ops.gru_train_forward / _backward, GruTrainFunction, GRUEncoder.use_hip_train, train.py
--hip_seq2vec_train) against the fp64 restatement tests/gru_train_ref.py.

Bound: every gradient within 1e-4 of its fp64 tensor's max, the project's standing gradient bound; a tensor whose fp64 max is 0 must be
exactly 0.  torch's own fp32 nn.GRU backward sits at 1.1e-7 .. 4.5e-7 of each tensor's max against fp64 at these six shapes.
Shapes: those of tests/test_gru_gpu.py with their word-id recipes -- one tile and ragged tiles, no recurrent step, constant n_t, tiles
that empty out during the sweep, the real widths."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG
from gru_train_ref import GRADS, gru_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

#         name       dim_emb dim_q  B   T
SHAPES = {"one":      (22,   48,    1,  1),     # one row, one step: T = 1, no recurrent product
          "ragged":   (22,  100,    5,  7),     # lengths {0, 1, 3, 7, 7}, a zero inside a question, E[0] nonzero
          "all1":     (40,  100,   70, 26),     # every length 1: no recurrent product runs; more than one row tile, ragged
          "all26":    (40,  136,   70, 26),     # every length 26: n_t constant
          "fall":     (40,  136,  200, 26),     # uniform 3..26 with exactly one row of 26: n_t falls to 1, row tiles empty out during the sweep
          "real":     (620, 2400,  40, 26)}     # the real dims, uniform 3..26
V = 50


def make_wids(name, B, T, rng):
    if name == "one":
        lens = [1]
    elif name == "ragged":
        lens = [0, 1, 3, 7, 7]
    elif name == "all1":
        lens = [1] * B
    elif name == "all26":
        lens = [T] * B
    else:
        lens = list(rng.integers(3, T, size=B))               # 3..25
        if name == "fall":
            lens[B // 3] = T                                   # exactly one row of 26
        else:
            lens[: 24] = range(3, 27)                          # 3..26, each at least once
    wids = np.zeros((B, T), np.int64)
    for b, n in enumerate(lens):
        wids[b, :n] = rng.integers(1, V + 1, size=n)
    if name == "ragged":
        wids[3, 4] = 0                                         # a zero inside the question: 6 nonzero ids, stepped over t < 6
    return wids


def make_encoder(de, dq, seed, dropout=0.25):
    from vqa.models.seq2vec import GRUEncoder
    torch.manual_seed(seed)
    enc = GRUEncoder(["w%d" % i for i in range(V)], dim_q=dq, dim_emb=de, dropout=dropout).eval()
    with torch.no_grad():
        enc.embedding.weight[0] = torch.randn(de) * 0.5       # the padding row is READ, never assumed zero
    return enc


def tensors_of(enc):
    return [enc.embedding.weight.detach()] + [getattr(enc.gru, k).detach() for k in WKEYS]


def hip_step(enc, wids, dq_out, want_dE=True, dE=None):
    """-> (q, grads) of one forward + backward through the ops layer, as numpy."""
    from neuralcx import ops
    gw = ops.gru_train_weights(*tensors_of(enc))
    w = torch.from_numpy(wids).to(DEV)
    ws = ops.gru_train_workspace(w.shape[0], w.shape[1], gw, DEV)
    q = ops.gru_train_forward(w, gw, ws)
    g = ops.gru_train_backward(w, gw, ws, torch.from_numpy(dq_out).to(DEV), want_dE=want_dE, dE=dE)
    ops.check_gru_ids(device=DEV)
    return q.cpu().numpy(), {k: (None if v is None else v.cpu().numpy()) for k, v in g.items()}


_CASES = {}


def case(name):
    """(encoder on the device, wids, dq_out, fp64 reference, q and gradients of the HIP path) -- computed once, shared, never modified."""
    if name not in _CASES:
        de, dq, B, T = SHAPES[name]
        enc = make_encoder(de, dq, seed=sorted(SHAPES).index(name))
        rng = np.random.default_rng(7)
        wids = make_wids(name, B, T, rng)
        dq_out = rng.standard_normal((B, dq)).astype(np.float32)
        ref = gru_train(wids, *[t.numpy() for t in tensors_of(enc)], dq_out)
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
def test_forward_is_bit_equal_to_gru_encode(name):
    from neuralcx import ops
    enc, wids, _, ref, q, _ = case(name)
    plain = ops.gru_encode(torch.from_numpy(wids).to(DEV), ops.gru_weights(enc)).cpu().numpy()
    assert np.array_equal(q, plain)
    assert float(np.abs(q - ref["q"]).max()) <= TOL


@pytest.mark.parametrize("name", list(SHAPES))
def test_gradients_match_fp64(name):
    enc, wids, _, ref, _, g = case(name)
    if name in ("one", "all1"):
        assert not ref["w_hh"].any()                           # no recurrent product ran: exactly 0 (checked in check_grads)
    check_grads(name, g, ref)
    assert not g["E"][0].any()                                 # the padding row, whatever read E[0] in the forward


def test_planted_rows_of_the_ragged_case():
    """The empty row (one step over wids[b, 0] = 0) and the row with a zero inside, each isolated by a one-hot dq_out."""
    enc, wids, dq_out, _, _, _ = case("ragged")
    assert not wids[0].any() and wids[3, 4] == 0 and wids[3, 5] != 0
    ts = [t.cpu().numpy() for t in tensors_of(enc)]
    for b in (0, 3):
        d = np.zeros_like(dq_out)
        d[b] = dq_out[b]
        ref = gru_train(wids, *ts, d)
        assert ref["w_ih"].any() and ref["b_hh"].any()
        _, g = hip_step(enc, wids, d)
        check_grads("ragged row %d" % b, g, ref)
        assert not g["E"][0].any()
    assert not ref["E"][0].any() and ref["E"].any() and ref["w_hh"].any()       # row 3: E[0] was read at t = 4 and still gets nothing


def test_device_pack_equals_the_layout_restatement():
    from neuralcx import ops
    for name in ("ragged", "all26"):
        enc = case(name)[0]
        ts = tensors_of(enc)
        gw = ops.gru_train_weights(*ts)
        assert torch.equal(gw.packed_t, ops.gru_pack_t_layout(ts[1], ts[2]))
        assert torch.equal(gw.packed, ops.gru_weights(enc).packed)
        ih, hh = ops.gru_unpack_t_layout(gw.packed_t, gw.dim_emb, gw.dim_q)
        assert torch.equal(ih, ts[1]) and torch.equal(hh, ts[2])


def test_null_de_leaves_the_other_gradients_bit_identical():
    for name in ("ragged", "fall"):
        enc, wids, dq_out, _, _, g = case(name)
        _, g0 = hip_step(enc, wids, dq_out, want_dE=False)
        assert g0["E"] is None
        for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
            assert np.array_equal(g0[k], g[k]), (name, k)


def test_bit_identical_from_run_to_run():
    for name in ("fall", "ragged"):
        enc, wids, dq_out, _, q, g = case(name)
        q2, g2 = hip_step(enc, wids, dq_out)
        assert np.array_equal(q2, q)
        for k in GRADS:
            assert np.array_equal(g2[k], g[k]), (name, k)


def test_invalid_arguments_return_minus_one():
    import ctypes as C
    from neuralcx import _lib, ops
    enc, wids, dq_out, _, _, _ = case("ragged")
    de, dq, B, T = SHAPES["ragged"]
    gw = ops.gru_train_weights(*tensors_of(enc))
    w = torch.from_numpy(wids).to(DEV).to(torch.int32)
    ws = ops.gru_train_workspace(B, T, gw, DEV)
    p, have = ops._ws_ptr(ws)
    L = _lib.lib()
    n = L.ncx_gru_train_workspace_bytes(B, T, de, dq)          # the exact size: one byte less is short
    assert 0 < n <= have
    q, d = torch.empty(B, dq, device=DEV), torch.from_numpy(dq_out).to(DEV)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    g = [torch.empty(3 * dq, de, device=DEV), torch.empty(3 * dq, dq, device=DEV), torch.empty(3 * dq, device=DEV), torch.empty(3 * dq, device=DEV)]
    ptr = lambda t: C.c_void_p(t.data_ptr())

    def fwd(T_=T, ws_=p, n_=n, wids_=ptr(w)):
        return L.ncx_gru_train_forward(wids_, B, T_, ptr(gw.E), gw.V1, de, dq, ptr(gw.packed), ws_, n_, ptr(q), ptr(flag), None)

    def bwd(T_=T, ws_=p, n_=n, d_=ptr(d)):
        return L.ncx_gru_train_backward(ptr(w), B, T_, ptr(gw.E), gw.V1, de, dq, ptr(gw.packed_t), ws_, n_, d_, *[ptr(t) for t in g], None, None)

    for f in (fwd, bwd):
        assert f(T_=65) == -1                                  # T > 64
        assert f(n_=n - 1) == -1                               # short workspace
        assert f(ws_=C.c_void_p(p.value + 16)) == -1           # misaligned workspace
        assert f(ws_=None) == -1
    assert fwd(wids_=None) == -1 and bwd(d_=None) == -1
    assert fwd() == 0 and bwd() == 0                           # ... and the same calls with valid arguments run
    torch.cuda.synchronize()


def test_out_of_range_word_id_raises_and_writes_nowhere_outside_de():
    from neuralcx import ops
    enc, wids, dq_out, _, _, g = case("ragged")
    de, dq, B, T = SHAPES["ragged"]
    for bad in (V + 1, -3, 2 ** 30):
        w = wids.copy()
        w[2, 1] = bad
        mine = make_encoder(de, dq, seed=sorted(SHAPES).index("ragged")).to(DEV).train()
        mine.use_hip_train = True
        out = mine(torch.from_numpy(w).to(DEV))                # through the module: the flag is raised by the forward
        with pytest.raises(IndexError):
            ops.check_gru_ids(device=DEV)
        ops.check_gru_ids(device=DEV)                          # cleared
        assert out.requires_grad
        # the backward never uses the id as an address: a guard band around dE stays as it was
        guard = torch.full((3 * (V + 1), de), 7.5, device=DEV)
        dE = guard[V + 1:2 * (V + 1)]
        gw = ops.gru_train_weights(*tensors_of(enc))
        wd = torch.from_numpy(w).to(DEV)
        ws = ops.gru_train_workspace(B, T, gw, DEV)
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        ops.gru_train_forward(wd, gw, ws, bad_flag=flag)
        got = ops.gru_train_backward(wd, gw, ws, torch.from_numpy(dq_out).to(DEV), dE=dE)
        assert int(flag.item()) == 1 and got["E"].data_ptr() == dE.data_ptr()
        assert bool((guard[:V + 1] == 7.5).all()) and bool((guard[2 * (V + 1):] == 7.5).all())
        assert bool(torch.isfinite(dE).all()) and not bool(dE[0].any())


def _module_pair(name, dropout):
    de, dq, _, _ = SHAPES[name]
    seed = sorted(SHAPES).index(name)
    a, b = (make_encoder(de, dq, seed, dropout).to(DEV).train() for _ in range(2))
    a.use_hip_train = True
    return a, b


@pytest.mark.parametrize("dropout", [0.0, 0.25])
def test_module_agrees_with_the_torch_path(dropout, monkeypatch):
    from neuralcx import ops
    _, wids, dq_out, _, _, _ = case("ragged")
    hip, ref = _module_pair("ragged", dropout)
    calls = []
    real = ops.gru_train_forward
    monkeypatch.setattr(ops, "gru_train_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    w, d = torch.from_numpy(wids).to(DEV), torch.from_numpy(dq_out).to(DEV)
    outs = []
    for m in (hip, ref):
        torch.manual_seed(11)                                  # the same dropout mask on q for both
        out = m(w)
        (out * d).sum().backward()
        outs.append(out.detach())
    assert calls == [1] and ref.use_hip_train is False
    if dropout:
        assert bool((outs[0] == 0).any()) and bool(((outs[0] == 0) == (outs[1] == 0)).all())
    assert float((outs[0] - outs[1]).abs().max()) <= TOL * float(outs[1].abs().max())
    for (n, p), (_, r) in zip(hip.named_parameters(), ref.named_parameters()):
        err, mx = float((p.grad - r.grad).abs().max()), float(r.grad.abs().max())
        print("dropout %.2f %s: max|hip - torch| = %.3e of max %.3e" % (dropout, n, err, mx))
        assert mx > 0 and err <= TOL * mx, n
    with torch.no_grad():                                      # grad mode off: what the module did before (no training call)
        hip.eval()
        hip(w)
    assert calls == [1]


def test_fixed_embedding_gets_no_gradient():
    _, wids, dq_out, _, _, g = case("ragged")
    hip, _ = _module_pair("ragged", 0.0)
    hip.embedding.weight.requires_grad_(False)
    out = hip(torch.from_numpy(wids).to(DEV))
    (out * torch.from_numpy(dq_out).to(DEV)).sum().backward()
    assert hip.embedding.weight.grad is None
    assert np.array_equal(hip.gru.weight_hh_l0.grad.cpu().numpy(), g["w_hh"])
    assert np.array_equal(hip.gru.weight_ih_l0.grad.cpu().numpy(), g["w_ih"])


def test_optimizer_step_invalidates_the_pack_cache():
    from neuralcx import ops
    _, wids, dq_out, _, q0, _ = case("ragged")
    hip, _ = _module_pair("ragged", 0.0)
    w, d = torch.from_numpy(wids).to(DEV), torch.from_numpy(dq_out).to(DEV)
    opt = torch.optim.SGD(hip.parameters(), lr=0.05)
    out = hip(w)
    assert np.array_equal(out.detach().cpu().numpy(), q0)
    first = hip.__dict__["_hip_gru_train"][1]
    assert hip(w) is not None and hip.__dict__["_hip_gru_train"][1] is first    # cached while nothing changes
    (out * d).sum().backward()
    opt.step()
    got = hip(w).detach()
    assert hip.__dict__["_hip_gru_train"][1] is not first
    fresh = ops.gru_encode(w, ops.gru_weights(hip))
    assert torch.equal(got, fresh)
    assert float((got.cpu() - torch.from_numpy(q0)).abs().max()) > 100 * TOL    # the step moved q: a stale pack would show


TINY_YAML = """
logs: {dir_logs: %s}
vqa: {nans: 40, maxlength: 8}
coco: {}
model:
  arch: MutanNoAtt
  seq2vec: {arch: gru, emb_size: 16, dropout: 0.25, fixed_emb: False}
  fusion: {dim_v: 64, dim_q: 48, dim_hv: 32, dim_hq: 32, dim_mm: 24, R: 3, activation_v: tanh, activation_q: tanh, dropout_v: 0.1, dropout_q: 0.1, dropout_hv: 0, dropout_hq: 0}
  classif: {dropout: 0.1}
optim: {lr: 0.01, batch_size: 16, epochs: 1}
"""


def test_cli_trains_the_encoder_in_hip(tmp_path, capsys):
    """train.py --synthetic --hip_seq2vec_train --epochs 1 on 384 examples (21 steps of 16).  A single step's training loss is noise at
    this size, so "falls over the epoch" is measured on the validation split, before the epoch against after it; the same loop on the
    torch modules (--no_hip, on a CPU) goes from 3.702 to 3.581 under the default seed and falls under seeds 1, 2 and 3 as well."""
    import importlib.util
    from vqa.models.seq2vec import GRUEncoder
    spec = importlib.util.spec_from_file_location("vqa_train_cli_gru_gpu", os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    y = tmp_path / "o.yaml"
    y.write_text(TINY_YAML % str(tmp_path / "logs"))
    losses, before = [], []
    real_step, real_epoch = cli.Trainer._step, cli.Trainer.run_epoch

    def step(self, split, sel, train):
        r = real_step(self, split, sel, train)
        if train:
            losses.append(r[0])
        return r

    def run_epoch(self, epoch):
        before.append(self.evaluate()["loss"])
        return real_epoch(self, epoch)
    cli.Trainer._step, cli.Trainer.run_epoch = step, run_epoch
    r = cli.main(["--path_opt", str(y), "--synthetic", "--syn_examples", "384", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0",
                  "--hip_seq2vec_train", "--epochs", "1"])
    assert "question encoder: HIP forward + backward through time" in capsys.readouterr().out
    assert r["trainer"].model.seq2vec.use_hip_train is True
    ls = [float(x) for x in losses]
    after = r["history"][0]["val"]["loss"]
    print("train losses", ["%.3f" % x for x in ls], "val before %.4f after %.4f" % (before[0], after))
    assert len(ls) >= 8 and all(np.isfinite(ls)) and np.isfinite(after)
    assert after < before[0]
    sd = torch.load(str(tmp_path / "logs" / "best_model.pth.tar"))
    plain = GRUEncoder(["w%d" % i for i in range(30)], dim_q=48, dim_emb=16, dropout=0.25)
    plain.load_state_dict({k[len("seq2vec."):]: v for k, v in sd.items() if k.startswith("seq2vec.")}, strict=True)
    assert plain.use_hip_train is False
