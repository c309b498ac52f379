"""GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the 2-lstm encoder's step kernel (k_lstm_step_x6: ops.lstm_encode / lstm_train_forward with
x6=True, TwoLSTM.hip_x6, train.py --x6_2lstm) against the fp64 restatements tests/lstm_ref.py / tests/lstm_train_ref.py and against the
fp32 step kernel.

Bounds: q within 1e-4 absolute of fp64 (TOL of the LSTM suites, unchanged); X6 against fp32 within 1e-5 of max|q| (the bound of
test_hip_parity.py::test_x6_* and of the GRU's X6 suite); and the one that tells six plane products from three or five:
err_x6 <= 1.5 err_fp32 + 1e-7 max(1, max|ref|).  tests/test_lstm_x6_cpu.py emulates the cut on the CPU: six products land at 2.1e-7 /
2.7e-7 / 5.0e-7 on `fall` / `all26` / `real` beside fp32's 3.7e-7 / 3.9e-7 / 7.5e-7, three or five products at 1.5e-5 .. 6.6e-5.
Gradients: within 1e-4 of each fp64 tensor's max (check_grads of the LSTM training suites).
Shapes: the thirteen of test_lstm_gpu.py, the eight of lstm_edge_cases.py, and three around the X6 kernel's row tile (EXTRA below)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lstm_edge_cases as edges
import test_lstm_edges_gpu as edge_suite
import test_lstm_gpu as fwd_suite
import test_lstm_train_gpu as train_suite
from conftest import PKG
from lstm_ref import lengths, lstm_encode as ref_encode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = fwd_suite.TOL

#        name      emb  H    B    T
EXTRA = {"row129": (33, 65,  129, 3),     # one past 128 rows (n_t = 129, 129, 128: the fifth of the tile's six wave rows holds one row, then none
                                          # and skips its MFMAs); one past the 32-deep k-step in kx, one past two 32-unit blocks
         "row257": (40, 129, 257, 2),     # one past 256 rows (n_t = 257, 256: a second row tile, 65 / 64 rows of it) and one past four unit blocks
         "row193": (7,  33,  193, 2)}     # L6_BM, the kernel's 192-row tile: n_t = 193, 192 -- a second row tile of one row, gone at step 1
# a case is (suite, name): the two suites share names (`odd`, `over64`, `long` ...) for different weights and ids
ALL = [("fwd", n) for n in fwd_suite.SHAPES] + [("edge", n) for n in edges.CASES] + [("extra", n) for n in EXTRA]
NO_RECURRENCE = (("fwd", "one"), ("fwd", "all1"))      # T = 1 / every length 1: step 0 only, the h columns never run
ident = lambda c: "%s-%s" % c

_CASES = {}


def dims_of(c):
    return {"fwd": fwd_suite.SHAPES, "edge": edges.CASES, "extra": EXTRA}[c[0]][c[1]]


def case(c):
    """-> (LstmWeights on the device, wids, fp64 q) of a forward case."""
    if c not in _CASES:
        from neuralcx import ops
        suite, name = c
        if suite == "fwd":
            enc, wids, ref, _ = fwd_suite.case(name)
        elif suite == "edge":
            enc, _, wids, _, r, _, _ = edge_suite.case(name)
            ref = r["q"]
        else:
            emb, H, B, T = EXTRA[name]
            enc = fwd_suite.make_encoder(emb, H, seed=40 + sorted(EXTRA).index(name))
            rng = np.random.default_rng(11)
            lens = [T] * B
            lens[B // 2] = T - 1
            wids = np.zeros((B, T), np.int64)
            for b, n in enumerate(lens):
                wids[b, :n] = rng.integers(1, fwd_suite.V + 1, size=n)
            ref = ref_encode(wids, *fwd_suite.weights_of(enc))
            enc = enc.to(DEV)
        _CASES[c] = (ops.lstm_weights(enc), wids, ref)
    return _CASES[c]


def encode(c, x6):
    from neuralcx import ops
    lw, wids, _ = case(c)
    q = ops.lstm_encode(torch.from_numpy(wids).to(DEV), lw, x6=x6)
    ops.check_gru_ids(device=DEV)
    return q


@pytest.mark.parametrize("c", ALL, ids=ident)
def test_x6_matches_fp64_at_the_unchanged_tolerance(c):
    from neuralcx import ops
    lw, wids, ref = case(c)
    emb, H, B, T = dims_of(c)
    assert wids.shape == (B, T) and (lw.emb, lw.H) == (emb, H)
    assert ops.lstm_step_form(emb, H, B, T, x6=True) == "x6"
    q = encode(c, True)
    assert q.dtype == torch.float32 and tuple(q.shape) == (B, 2 * H)
    q = q.cpu().numpy()
    err = float(np.abs(q - ref).max())
    print("%s dims %s: max|x6 - fp64| = %.3e, max|q| = %.3f" % (ident(c), (emb, H, B, T), err, float(np.abs(ref).max())))
    assert q.shape == ref.shape and np.isfinite(q).all()
    assert err <= TOL


@pytest.mark.parametrize("c", [c for c in ALL if c not in NO_RECURRENCE], ids=ident)
def test_the_flag_switches_kernels_and_agrees_with_fp32(c):
    _, wids, _ = case(c)
    assert (lengths(wids) > 1).any()        # a recurrent product runs
    q6, q32 = encode(c, True), encode(c, False)
    diff, m = float((q6 - q32).abs().max()), float(q32.abs().max())
    print("%s: max|x6 - fp32| = %.3e, max|fp32| = %.3f" % (ident(c), diff, m))
    assert diff <= 1e-5 * m
    if c == ("fwd", "real"):
        assert not torch.equal(q6, q32)                          # another kernel ran: another summation order


@pytest.mark.parametrize("name", ["real", "fall", "all26"])
def test_x6_is_fp32_grade(name):
    """Six plane products, not three or five: the 1e-4 above would let those pass, this bound does not."""
    c = ("fwd", name)
    _, _, ref = case(c)
    e32 = float(np.abs(encode(c, False).cpu().numpy() - ref).max())
    e6 = float(np.abs(encode(c, True).cpu().numpy() - ref).max())
    bound = 1.5 * e32 + 1e-7 * max(1.0, float(np.abs(ref).max()))
    print("%s: max|fp32 - fp64| = %.3e, max|x6 - fp64| = %.3e (bound %.3e)" % (name, e32, e6, bound))
    assert e32 <= TOL
    assert e6 <= TOL
    assert e6 <= bound


@pytest.mark.parametrize("name", edge_suite.STALE)
def test_x6_is_deterministic_and_ignores_what_the_workspace_held(name):
    """Two calls through the binding, then ncx_lstm2_encode_flags on the caller's workspace: zeroed against all 0xFF, q pre-filled with NaN."""
    from neuralcx import _lib, ops
    c = ("edge", name)
    lw, wids, _ = case(c)
    emb, H, B, T = edges.CASES[name]
    q0 = encode(c, True)
    assert torch.equal(encode(c, True), q0)
    L = _lib.lib()
    n = L.ncx_lstm2_workspace_bytes(B, T, emb, H)
    assert n > 0
    w = torch.from_numpy(wids).to(DEV).to(torch.int32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for byte in (0, 0xFF):
        ws = torch.empty(n + 256, dtype=torch.uint8, device=DEV)
        ws.fill_(byte)
        p, have = ops._ws_ptr(ws)
        q = torch.full((B, 2 * H), float("nan"), device=DEV)
        assert L.ncx_lstm2_encode_flags(ptr(w), B, T, ptr(lw.E), lw.V1, emb, H, ptr(lw.packed), _lib.NCX_F_X6, p, have, ptr(q), ptr(flag), None) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(q).all()) and torch.equal(q, q0), byte
    assert int(flag.item()) == 0


def _train_case(name):
    """-> (encoder, LstmTrainWeights, wids, dq_out, fp64 reference) of a training case: SHAPES of test_lstm_train_gpu.py or an edge case."""
    from neuralcx import ops
    if name in train_suite.SHAPES:
        enc, wids, dq_out, ref, _, _ = train_suite.case(name)
        return enc, ops.lstm_train_weights(*train_suite.tensors_of(enc)), wids, dq_out, ref
    enc, lw, wids, dq_out, ref, _, _ = edge_suite.case(name)
    return enc, lw, wids, dq_out, ref


@pytest.mark.parametrize("name", list(train_suite.SHAPES) + ["odd", "over64", "steps"])
def test_training_forward_and_backward_on_the_x6_stash(name):
    """The workspace is all 0xFF (NaN as a float) before the forward: what the backward reads of it, the X6 forward wrote."""
    from neuralcx import ops
    enc, lw, wids, dq_out, ref = _train_case(name)
    w = torch.from_numpy(wids).to(DEV)
    ws = ops.lstm_train_workspace(w.shape[0], w.shape[1], lw, DEV)
    ws.fill_(0xFF)
    q = ops.lstm_train_forward(w, lw, ws, x6=True)
    g = ops.lstm_train_backward(w, lw, ws, torch.from_numpy(dq_out).to(DEV))
    ops.check_gru_ids(device=DEV)
    plain = ops.lstm_encode(w, ops.lstm_weights(enc), x6=True)
    assert torch.equal(q, plain)                                 # bit for bit, under the same flag
    assert float(np.abs(q.cpu().numpy() - ref["q"]).max()) <= TOL
    got = {k: v.cpu().numpy() for k, v in g.items()}
    train_suite.check_grads(name + " (x6 stash)", got, ref)       # finite, and within 1e-4 of each fp64 tensor's max
    assert not got["E"][0].any()


def test_module_hands_hip_x6_to_the_eval_route(monkeypatch):
    from neuralcx import _lib, ops
    enc, wids, _, _ = fwd_suite.case("ragged")
    w = torch.from_numpy(wids).to(DEV)
    lw = ops.lstm_weights(enc)
    q32, q6 = ops.lstm_encode(w, lw, x6=False), ops.lstm_encode(w, lw, x6=True)
    assert not torch.equal(q32, q6)
    try:
        with torch.no_grad():
            for process_wide, want_none in ((0, q32), (_lib.NCX_F_X6, q6)):
                monkeypatch.setattr(ops, "EXTRA_FLAGS", process_wide)
                enc.hip_x6 = True
                assert torch.equal(enc(w), q6)
                enc.hip_x6 = False
                assert torch.equal(enc(w), q32)
                enc.hip_x6 = None
                assert torch.equal(enc(w), want_none)            # None follows the process-wide flag, read at call time
            monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
            enc.hip_x6, enc.use_hip = True, False                # no routing decision changes: the torch path stays the torch path
            calls = []
            real = ops.lstm_encode
            monkeypatch.setattr(ops, "lstm_encode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
            out = enc(w)
            assert calls == [] and float((out - q32).abs().max()) <= TOL
    finally:
        for k in ("hip_x6", "use_hip"):
            enc.__dict__.pop(k, None)                            # back to the class defaults


def test_training_module_with_hip_x6_agrees_with_the_torch_path(monkeypatch):
    """Training mode, dropout p = 0.3 live on both halves, one seed: the same masks, every .grad within 1e-4 of torch's max."""
    from neuralcx import ops
    _, wids, dq_out, _, _, _ = train_suite.case("ragged")
    hip, ref = train_suite._module_pair("ragged")
    hip.hip_x6 = True
    seen = []
    real = ops.lstm_train_forward
    monkeypatch.setattr(ops, "lstm_train_forward", lambda *a, **k: (seen.append(k.get("x6")), real(*a, **k))[1])
    w, d = torch.from_numpy(wids).to(DEV), torch.from_numpy(dq_out).to(DEV)
    outs = []
    for m in (hip, ref):
        torch.manual_seed(11)                                  # the same dropout masks on the two halves for both
        out = m(w)
        (out * d).sum().backward()
        outs.append(out.detach())
    assert seen == [True] and hip.use_hip_bptt is True and ref.use_hip_bptt is False and ref.hip_x6 is None
    assert bool((outs[0] == 0).any()) and bool(((outs[0] == 0) == (outs[1] == 0)).all())
    assert float((outs[0] - outs[1]).abs().max()) <= train_suite.TOL * float(outs[1].abs().max())
    for (n, p), (_, r) in zip(hip.named_parameters(), ref.named_parameters()):
        err, mx = float((p.grad - r.grad).abs().max()), float(r.grad.abs().max())
        print("%s: max|hip x6 - torch| = %.3e of max %.3e" % (n, err, mx))
        assert mx > 0 and err <= train_suite.TOL * mx, n


def _train_cli(tmp_path, name):
    import importlib.util
    spec = importlib.util.spec_from_file_location(name, os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    y = tmp_path / "o.yaml"
    y.write_text(train_suite.TINY_YAML % str(tmp_path / "logs"))
    return cli, ["--path_opt", str(y), "--synthetic", "--syn_examples", "128", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0",
                 "--epochs", "1"]


def test_cli_trains_with_the_x6_step_kernel(tmp_path, capsys, monkeypatch):
    from neuralcx import ops
    cli, args = _train_cli(tmp_path, "vqa_train_cli_lstm_x6_gpu")
    losses, seen = [], []
    real_step, real_fwd = cli.Trainer._step, ops.lstm_train_forward

    def step(self, split, sel, train):
        r = real_step(self, split, sel, train)
        if train:
            losses.append(float(r[0]))
        return r
    monkeypatch.setattr(cli.Trainer, "_step", step)
    monkeypatch.setattr(ops, "lstm_train_forward", lambda *a, **k: (seen.append(k.get("x6")), real_fwd(*a, **k))[1])
    r = cli.main(args + ["--hip_2lstm_train", "--x6_2lstm"])
    text = capsys.readouterr().out
    assert "2-lstm question encoder: HIP forward + backward through time" in text and "(2-lstm question encoder: bf16 x 6 step kernel)" in text
    enc = r["trainer"].model.seq2vec
    assert enc.hip_x6 is True and enc.use_hip_bptt is True
    print("train losses", ["%.3f" % x for x in losses])
    assert len(losses) >= 4 and len(seen) == len(losses) and all(x is True for x in seen)
    assert all(np.isfinite(losses)) and np.isfinite(r["history"][0]["val"]["loss"])


def test_cli_freezes_the_encoder_on_the_x6_step_kernel(tmp_path, capsys, monkeypatch):
    from neuralcx import ops
    cli, args = _train_cli(tmp_path, "vqa_train_cli_lstm_x6_frozen_gpu")
    seen = []
    real = ops.lstm_encode
    monkeypatch.setattr(ops, "lstm_encode", lambda *a, **k: (seen.append(k.get("x6")), real(*a, **k))[1])
    r = cli.main(args + ["--freeze_seq2vec", "--x6_2lstm"])
    text = capsys.readouterr().out
    assert "(2-lstm question encoder: bf16 x 6 step kernel)" in text
    assert r["trainer"].model.seq2vec.hip_x6 is True
    assert len(seen) >= 2 and all(x is True for x in seen)       # one call per split, each on the X6 kernel
    assert np.isfinite(r["history"][0]["train"]["loss"]) and np.isfinite(r["history"][0]["val"]["loss"])
