"""GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the GRU encoder's step kernel (k_gru_step_x6: ops.gru_encode / gru_train_forward with
x6=True, GRUEncoder.hip_x6, train.py --x6_seq2vec) against the fp64 restatements tests/gru_ref.py / tests/gru_train_ref.py and against
the fp32 step kernel.

Bounds: q within 1e-4 absolute of fp64 (TOL of the GRU suites, unchanged); X6 against fp32 within 1e-5 of max|q| (the bound of
test_hip_parity.py::test_x6_* and test_mlb_att_x6_gpu.py); and the one that tells six plane products from three or five:
err_x6 <= 1.5 err_fp32 + 1e-7 max(1, max|ref|).  A CPU emulation of the cut (torch fp32 matmuls over the planes) puts six products at
9e-8 / 7e-8 on `real` / `fall` beside fp32's 1.9e-7 / 1.0e-7, and three or five products at 4e-6 .. 1.2e-5.
Gradients: within 1e-4 of each fp64 tensor's max (check_grads of test_gru_train_gpu.py).
Shapes: those of test_gru_gpu.py / test_gru_train_gpu.py, the eight of gru_edge_cases.py, two one past the 128 / 256 row and 64 / 128
unit boundaries, and one one past the X6 kernel's own row tile, 192 rows (EXTRA below)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gru_edge_cases as edges
import test_gru_edges_gpu as edge_suite
import test_gru_gpu as fwd_suite
import test_gru_train_gpu as train_suite
from conftest import PKG
from gru_ref import gru_encode as ref_encode
from gru_train_ref import gru_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = fwd_suite.TOL

#        name      dim_emb dim_q  B   T
EXTRA = {"row129": (33,    65,    129, 3),     # one past 128 rows (n_t = 129, 129, 128: the fifth of the tile's six wave rows holds one row, then
                                               # none and skips its MFMAs); one past the 32-deep k-step in kx, one past two 32-unit blocks
         "row257": (40,    129,   257, 2),     # one past 256 rows (n_t = 257, 256: a second row tile, 65 / 64 rows of it) and one past four unit blocks
         "row193": (7,     33,    193, 2)}     # G6_BM, the kernel's 192-row tile: n_t = 193, 192 -- a second row tile of one row, gone at step 1
# (its other constants, the 32-unit block and the 32-deep k-step: `over32` of the edge cases, 33 / 33, and row129 / row257 above)
NO_RECURRENCE = ("one", "all1")                # T = 1 / every length 1: step 0 only, the h columns never run

_CASES = {}


def case(name):
    """-> (GruWeights on the device, wids, fp64 q) of a forward case: SHAPES of test_gru_gpu.py, CASES of gru_edge_cases.py, EXTRA."""
    if name not in _CASES:
        from neuralcx import ops
        if name in fwd_suite.SHAPES:
            enc, wids, ref, _ = fwd_suite.case(name)
        elif name in edges.CASES:
            enc, _, wids, _, r, _, _ = edge_suite.case(name)
            ref = r["q"]
        else:
            de, dq, B, T = EXTRA[name]
            enc = fwd_suite.make_encoder(de, dq, seed=40 + sorted(EXTRA).index(name))
            rng = np.random.default_rng(11)
            lens = [T] * B
            lens[B // 2] = T - 1
            wids = np.zeros((B, T), np.int64)
            for b, n in enumerate(lens):
                wids[b, :n] = rng.integers(1, fwd_suite.V + 1, size=n)
            ref = ref_encode(wids, *fwd_suite.weights_of(enc))
            enc = enc.to(DEV)
        _CASES[name] = (ops.gru_weights(enc), wids, ref)
    return _CASES[name]


def dims_of(name):
    return (fwd_suite.SHAPES.get(name) or edges.CASES.get(name) or EXTRA[name])


def encode(name, x6):
    from neuralcx import ops
    gw, wids, _ = case(name)
    q = ops.gru_encode(torch.from_numpy(wids).to(DEV), gw, x6=x6)
    ops.check_gru_ids(device=DEV)
    return q


ALL = list(fwd_suite.SHAPES) + list(edges.CASES) + list(EXTRA)


@pytest.mark.parametrize("name", ALL)
def test_x6_matches_fp64_at_the_unchanged_tolerance(name):
    from neuralcx import ops
    gw, wids, ref = case(name)
    de, dq, B, T = dims_of(name)
    assert wids.shape == (B, T) and (gw.dim_emb, gw.dim_q) == (de, dq)
    assert ops.gru_step_form(de, dq, B, T, x6=True) == "x6"
    q = encode(name, True).cpu().numpy()
    err = float(np.abs(q - ref).max())
    print("%s dims %s: max|x6 - fp64| = %.3e, max|q| = %.3f" % (name, (de, dq, B, T), err, float(np.abs(ref).max())))
    assert q.shape == ref.shape and q.dtype == np.float32 and np.isfinite(q).all()
    assert err <= TOL


@pytest.mark.parametrize("name", [n for n in ALL if n not in NO_RECURRENCE])
def test_the_flag_switches_kernels_and_agrees_with_fp32(name):
    _, wids, _ = case(name)
    assert ((wids != 0).sum(1) > 1).any()                       # a recurrent product runs
    q6, q32 = encode(name, True), encode(name, False)
    diff, m = float((q6 - q32).abs().max()), float(q32.abs().max())
    print("%s: max|x6 - fp32| = %.3e, max|fp32| = %.3f" % (name, diff, m))
    assert diff <= 1e-5 * m
    if name == "real":
        assert not torch.equal(q6, q32)                          # another kernel ran: another summation order


@pytest.mark.parametrize("name", ["real", "fall", "all26"])
def test_x6_is_fp32_grade(name):
    """Six plane products, not three or five: the 1e-4 above would let those pass, this bound does not."""
    _, _, ref = case(name)
    e32 = float(np.abs(encode(name, False).cpu().numpy() - ref).max())
    e6 = float(np.abs(encode(name, True).cpu().numpy() - ref).max())
    bound = 1.5 * e32 + 1e-7 * max(1.0, float(np.abs(ref).max()))
    print("%s: max|fp32 - fp64| = %.3e, max|x6 - fp64| = %.3e (bound %.3e)" % (name, e32, e6, bound))
    assert e32 <= TOL
    assert e6 <= TOL
    assert e6 <= bound


@pytest.mark.parametrize("name", edge_suite.STALE)
def test_x6_is_deterministic_and_ignores_what_the_workspace_held(name):
    """Two calls through the binding, then ncx_gru_encode_flags on the caller's workspace: zeroed against all 0xFF, q pre-filled with NaN."""
    from neuralcx import _lib, ops
    gw, wids, _ = case(name)
    de, dq, B, T = edges.CASES[name]
    q0 = encode(name, True)
    assert torch.equal(encode(name, True), q0)
    L = _lib.lib()
    n = L.ncx_gru_workspace_bytes(B, T, de, dq)
    assert n > 0
    w = torch.from_numpy(wids).to(DEV).to(torch.int32)
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    for byte in (0, 0xFF):
        ws = torch.empty(n + 256, dtype=torch.uint8, device=DEV)
        ws.fill_(byte)
        p, have = ops._ws_ptr(ws)
        q = torch.full((B, dq), float("nan"), device=DEV)
        assert L.ncx_gru_encode_flags(ptr(w), B, T, ptr(gw.E), gw.V1, de, dq, ptr(gw.packed), _lib.NCX_F_X6, p, have, ptr(q), ptr(flag), None) == 0
        torch.cuda.synchronize()
        assert bool(torch.isfinite(q).all()) and torch.equal(q, q0), byte
    assert int(flag.item()) == 0


def _train_case(name):
    """-> (encoder, GruTrainWeights, wids, dq_out, fp64 reference) of a training case: SHAPES of test_gru_train_gpu.py or an edge case."""
    from neuralcx import ops
    if name in train_suite.SHAPES:
        enc, wids, dq_out, ref, _, _ = train_suite.case(name)
        return enc, ops.gru_train_weights(*train_suite.tensors_of(enc)), wids, dq_out, ref
    enc, gw, wids, dq_out, ref, _, _ = edge_suite.case(name)
    return enc, gw, wids, dq_out, ref


@pytest.mark.parametrize("name", list(train_suite.SHAPES) + ["odd", "over64", "steps"])
def test_training_forward_and_backward_on_the_x6_stash(name):
    """The workspace is all 0xFF (NaN as a float) before the forward: what the backward reads of it, the X6 forward wrote."""
    from neuralcx import ops
    enc, gw, wids, dq_out, ref = _train_case(name)
    w = torch.from_numpy(wids).to(DEV)
    ws = ops.gru_train_workspace(w.shape[0], w.shape[1], gw, DEV)
    ws.fill_(0xFF)
    q = ops.gru_train_forward(w, gw, ws, x6=True)
    g = ops.gru_train_backward(w, gw, ws, torch.from_numpy(dq_out).to(DEV))
    ops.check_gru_ids(device=DEV)
    plain = ops.gru_encode(w, ops.gru_weights(enc), x6=True)
    assert torch.equal(q, plain)                                 # bit for bit, under the same flag
    assert float(np.abs(q.cpu().numpy() - ref["q"]).max()) <= TOL
    got = {k: v.cpu().numpy() for k, v in g.items()}
    train_suite.check_grads(name + " (x6 stash)", got, ref)       # finite, and within 1e-4 of each fp64 tensor's max
    assert not got["E"][0].any()


def test_module_hands_hip_x6_to_both_routes(monkeypatch):
    from neuralcx import _lib, ops
    enc, wids, _, _ = fwd_suite.case("ragged")
    w = torch.from_numpy(wids).to(DEV)
    gw = ops.gru_weights(enc)
    q32, q6 = ops.gru_encode(w, gw, x6=False), ops.gru_encode(w, gw, x6=True)
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
            real = ops.gru_encode
            monkeypatch.setattr(ops, "gru_encode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
            out = enc(w)
            assert calls == [] and float((out - q32).abs().max()) <= TOL
    finally:
        for k in ("hip_x6", "use_hip"):
            enc.__dict__.pop(k, None)                            # back to the class defaults


@pytest.mark.parametrize("dropout", [0.0, 0.25])
def test_training_module_with_hip_x6_agrees_with_the_torch_path(dropout, monkeypatch):
    from neuralcx import ops
    _, wids, dq_out, _, _, _ = train_suite.case("ragged")
    hip, ref = train_suite._module_pair("ragged", dropout)
    hip.hip_x6 = True
    seen = []
    real = ops.gru_train_forward
    monkeypatch.setattr(ops, "gru_train_forward", lambda *a, **k: (seen.append(k.get("x6")), real(*a, **k))[1])
    w, d = torch.from_numpy(wids).to(DEV), torch.from_numpy(dq_out).to(DEV)
    outs = []
    for m in (hip, ref):
        torch.manual_seed(11)                                  # the same dropout mask on q for both
        out = m(w)
        (out * d).sum().backward()
        outs.append(out.detach())
    assert seen == [True] and ref.use_hip_train is False and ref.hip_x6 is None
    if dropout:
        assert bool((outs[0] == 0).any()) and bool(((outs[0] == 0) == (outs[1] == 0)).all())
    assert float((outs[0] - outs[1]).abs().max()) <= train_suite.TOL * float(outs[1].abs().max())
    for (n, p), (_, r) in zip(hip.named_parameters(), ref.named_parameters()):
        err, mx = float((p.grad - r.grad).abs().max()), float(r.grad.abs().max())
        print("dropout %.2f %s: max|hip x6 - torch| = %.3e of max %.3e" % (dropout, n, err, mx))
        assert mx > 0 and err <= train_suite.TOL * mx, n


def test_cli_trains_with_the_x6_step_kernel(tmp_path, capsys, monkeypatch):
    import importlib.util
    from neuralcx import ops
    spec = importlib.util.spec_from_file_location("vqa_train_cli_gru_x6_gpu", os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    y = tmp_path / "o.yaml"
    y.write_text(train_suite.TINY_YAML % str(tmp_path / "logs"))
    losses, seen = [], []
    real_step, real_fwd = cli.Trainer._step, ops.gru_train_forward

    def step(self, split, sel, train):
        r = real_step(self, split, sel, train)
        if train:
            losses.append(float(r[0]))
        return r
    monkeypatch.setattr(cli.Trainer, "_step", step)
    monkeypatch.setattr(ops, "gru_train_forward", lambda *a, **k: (seen.append(k.get("x6")), real_fwd(*a, **k))[1])
    r = cli.main(["--path_opt", str(y), "--synthetic", "--syn_examples", "128", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0",
                  "--hip_seq2vec_train", "--x6_seq2vec", "--epochs", "1"])
    text = capsys.readouterr().out
    assert "question encoder: HIP forward + backward through time" in text and "(question encoder: bf16 x 6 step kernel)" in text
    enc = r["trainer"].model.seq2vec
    assert enc.hip_x6 is True and enc.use_hip_train is True
    print("train losses", ["%.3f" % x for x in losses])
    assert len(losses) >= 4 and len(seen) == len(losses) and all(x is True for x in seen)
    assert all(np.isfinite(losses)) and np.isfinite(r["history"][0]["val"]["loss"])
