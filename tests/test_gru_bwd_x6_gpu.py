"""GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the GRU encoder's backward through time (csrc/ncx_gru_train_x6.hip: ncx_gru_train_backward_flags,
ops.gru_train_backward x6=True, GruTrainFunction with GRUEncoder.hip_x6, train.py --x6_seq2vec --hip_seq2vec_train) against the fp64
restatement tests/gru_train_ref.py and against the fp32 backward on the same stash.

Bounds: every gradient within 1e-4 of its fp64 tensor's max (check_grads of test_gru_train_gpu.py, unchanged); X6 against fp32 within 1e-5
of each tensor's max; and the one that tells the shipped eight plane products from five or three, per gradient tensor:
    err_x6 <= 1.5 err_fp32 + 1e-7 max|ref|
The CPU emulation of the cut (tests/test_gru_bwd_x6_cpu.py, tests/gru_bwd_x6_ref.py) puts the shipped form at or below the fp32 error on
every tensor of `real`, `fall` and `all26` (dW_ih / dW_hh on `real`: 4.7e-6 / 5.8e-7 beside fp32's 5.5e-6 / 5.8e-7; it needs c = 0), five
products at 2.3e-4 / 2.5e-5 and three at 6.9e-4 / 7.7e-5 there (they would need c >= 9.4e-6 on those tensors of every shape, c >= 1.8e-6
on db_ih, db_hh and dE): c = 1e-7 separates them.
Shapes: the six of test_gru_train_gpu.py, the eight of gru_edge_cases.py, and EXTRA: the smallest shapes one past each constant of the
X6 kernels (the sweep / dX: 128 rows x 64 columns per workgroup; the walk: 256 gate rows x 64 feature columns, 32-row k-steps, work items
dealt to the XCDs in blocks of 4 gate-row tiles)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import gru_bwd_x6_ref as x6ref
import gru_edge_cases as edges
import test_gru_edges_gpu as edge_suite
import test_gru_train_gpu as train_suite
from conftest import PKG
from gru_train_ref import GRADS, gru_train

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = train_suite.TOL
GKEYS = edge_suite.GKEYS
MASK = x6ref.SHIPPED_MASK                       # what ncx_gru_bwd_form reports under NCX_F_X6: every product, 0xF
C_FLOOR = 1e-7

#        name       dim_emb dim_q  B   T    lengths
EXTRA = {"row129":  (7,     33,    129, 3, [3] * 128 + [1]),               # n_t = 129, 128, 128: one row past the sweep's 128-row tile, a second row tile that
                                                                          # holds one row at step 0 and empties at step 1 (its launch still injects dq_out)
         "gate257": (65,    65,    6,  3,  [3, 3, 2, 3, 1, 3]),            # 65 columns: one past the sweep's and dX's 64-column tile.  3 dqp = 288 gate rows:
                                                                          # a second gate-row tile of the walk whose only live row is gate row 256 (unit
                                                                          # 64 of block n / hn); 65 feature columns: a second column tile of one
                                                                          # column, in dW_hh (stash rows) and in dW_ih (gathered rows) both
         "kstep":   (9,     20,    33, 4,  [4] * 31 + [2, 1]),             # n_t = 33, 32, 31, 31: the dW_ih walk crosses the 32-row k-step (k-step + 1, k-step,
                                                                          # k-step - 1 on consecutive steps), the dW_hh walk starts exactly on it
         "group5":  (5,     400,   3,  3,  [3, 2, 1])}                     # 3 dqp = 1248 gate rows: five gate-row tiles, one past the work order's block of 4
NO_RECURRENCE = ("one", "all1")                 # T = 1 / every length 1: no recurrent product runs, dW_hh is exactly 0
ALL = list(train_suite.SHAPES) + list(edges.CASES) + list(EXTRA)

_CASES = {}


def case(name):
    """-> (encoder on the device, GruTrainWeights, wids, dq_out, fp64 reference): SHAPES of test_gru_train_gpu.py, CASES of gru_edge_cases.py, EXTRA."""
    if name not in _CASES:
        from neuralcx import ops
        if name in train_suite.SHAPES:
            enc, wids, dq_out, ref, _, _ = train_suite.case(name)
            gw = ops.gru_train_weights(*train_suite.tensors_of(enc))
        elif name in edges.CASES:
            enc, gw, wids, dq_out, ref, _, _ = edge_suite.case(name)
        else:
            de, dq, B, T, lens = EXTRA[name]
            enc = train_suite.make_encoder(de, dq, seed=60 + sorted(EXTRA).index(name))
            rng = np.random.default_rng(13)
            wids = np.zeros((B, T), np.int64)
            for b, n in enumerate(lens):
                wids[b, :n] = rng.integers(1, train_suite.V + 1, size=n)
            dq_out = rng.standard_normal((B, dq)).astype(np.float32)
            ref = gru_train(wids, *[t.numpy() for t in train_suite.tensors_of(enc)], dq_out)
            enc = enc.to(DEV)
            gw = ops.gru_train_weights(*train_suite.tensors_of(enc))
        _CASES[name] = (enc, gw, wids, dq_out, ref)
    return _CASES[name]


def dims_of(name):
    return (train_suite.SHAPES.get(name) or edges.CASES.get(name) or EXTRA[name][:4])


def forward(name, x6, ws=None, fill=None):
    """The training forward of a case -> (wids on the device, the workspace it left)."""
    from neuralcx import ops
    _, gw, wids, _, _ = case(name)
    w = torch.from_numpy(wids).to(DEV)
    if ws is None:
        ws = ops.gru_train_workspace(w.shape[0], w.shape[1], gw, DEV)
    if fill is not None:
        ws.fill_(fill)
    ops.gru_train_forward(w, gw, ws, x6=x6)
    ops.check_gru_ids(device=DEV)
    return w, ws


def backward_c(name, w, ws, flags, want_dE=True, entry="ncx_gru_train_backward_flags"):
    """The C entry point into five buffers pre-filled with NaN, on the caller's workspace -> {key: numpy}."""
    from neuralcx import _lib, ops
    _, gw, _, dq_out, _ = case(name)
    de, dq, B, T = dims_of(name)
    shapes = {"w_ih": (3 * dq, de), "w_hh": (3 * dq, dq), "b_ih": (3 * dq,), "b_hh": (3 * dq,), "E": (gw.V1, de)}
    g = {k: torch.full(shapes[k], float("nan"), device=DEV) for k in GKEYS}
    p, have = ops._ws_ptr(ws)
    ptr = lambda t: C.c_void_p(t.data_ptr())
    outs = [ptr(g[k]) if (k != "E" or want_dE) else None for k in GKEYS]
    w32, d = w.to(torch.int32), torch.from_numpy(dq_out).to(DEV)          # (named: a temporary's block would be handed to the next allocation)
    head = [ptr(w32), B, T, ptr(gw.E), gw.V1, de, dq, ptr(gw.packed_t)]
    tail = [p, have, ptr(d)] + outs + [None]
    L = _lib.lib()
    rc = L.ncx_gru_train_backward_flags(*head, flags, *tail) if entry == "ncx_gru_train_backward_flags" else L.ncx_gru_train_backward(*head, *tail)
    torch.cuda.synchronize()
    assert rc == 0
    return {k: g[k].cpu().numpy() for k in GKEYS if k != "E" or want_dE}


@pytest.mark.parametrize("stash", ["fp32", "x6"])
@pytest.mark.parametrize("name", ALL)
def test_gradients_match_fp64_at_the_unchanged_tolerance(name, stash):
    """The workspace is all 0xFF (NaN as a float, -1 as an int) before the forward, the five outputs all NaN before the backward."""
    from neuralcx import _lib, ops
    _, gw, wids, _, ref = case(name)
    de, dq, B, T = dims_of(name)
    assert wids.shape == (B, T) and (gw.dim_emb, gw.dim_q) == (de, dq)
    assert ops.gru_bwd_form(de, dq, B, T, x6=True) == MASK and ops.gru_bwd_form(de, dq, B, T, x6=False) == 0
    recurrent = bool(((wids != 0).sum(1) > 1).any())
    assert recurrent == (name not in NO_RECURRENCE)               # a recurrent product runs
    w, ws = forward(name, stash == "x6", fill=0xFF)
    g = backward_c(name, w, ws, _lib.NCX_F_X6)
    train_suite.check_grads("%s (%s stash)" % (name, stash), g, ref)      # finite, and within 1e-4 of each fp64 tensor's max
    assert not g["E"][0].any()                                    # the padding row, whatever read E[0] in the forward
    if not recurrent:
        assert not ref["w_hh"].any() and not g["w_hh"].any()      # no k-step at all: exactly 0


@pytest.mark.parametrize("name", ALL)
def test_the_flag_switches_kernels_and_agrees_with_fp32_on_the_same_stash(name):
    """The test that fails without the feature: ops.gru_train_backward has no x6 argument there, the library no ..._backward_flags."""
    from neuralcx import ops
    _, gw, _, dq_out, _ = case(name)
    w, ws = forward(name, False)
    d = torch.from_numpy(dq_out).to(DEV)
    g32 = ops.gru_train_backward(w, gw, ws, d, x6=False)
    g6 = ops.gru_train_backward(w, gw, ws, d, x6=True)
    for k in GRADS:
        diff, m = float((g6[k] - g32[k]).abs().max()), float(g32[k].abs().max())
        print("%s d%s: max|x6 - fp32| = %.3e, max|fp32| = %.3e" % (name, k, diff, m))
        assert diff <= 1e-5 * m, k
    if name == "real":
        for k, bit in (("w_hh", ops.GRU_BWD_DWHH), ("w_ih", ops.GRU_BWD_DWIH)):
            assert MASK & bit and not torch.equal(g6[k], g32[k]), k       # another kernel ran: another summation order


@pytest.mark.parametrize("name", ["real", "fall", "all26"])
def test_x6_backward_is_fp32_grade_product_by_product(name):
    """db_ih / db_hh depend on the sweep alone, dE adds dX, dW_hh and dW_ih add the walks: a truncated product shows in a tensor that names it."""
    from neuralcx import _lib
    _, _, _, _, ref = case(name)
    w, ws = forward(name, False)
    e32 = x6ref.errors(backward_c(name, w, ws, 0), ref)
    e6 = x6ref.errors(backward_c(name, w, ws, _lib.NCX_F_X6), ref)
    bound = x6ref.bound(e32, ref, C_FLOOR)
    for k in GRADS:
        print("%s d%s: max|fp32 - fp64| = %.3e, max|x6 - fp64| = %.3e (bound %.3e; max|fp64| %.3e)" % (name, k, e32[k], e6[k], bound[k], float(np.abs(ref[k]).max())))
    for k in GRADS:
        assert e6[k] <= bound[k], k


def test_bit_identical_from_run_to_run_and_without_de():
    from neuralcx import _lib
    for name in ("fall", "ragged", "gate257"):
        w, ws = forward(name, True)
        g = backward_c(name, w, ws, _lib.NCX_F_X6)
        g2 = backward_c(name, w, ws, _lib.NCX_F_X6)
        g0 = backward_c(name, w, ws, _lib.NCX_F_X6, want_dE=False)
        for k in GKEYS:
            assert np.array_equal(g2[k], g[k]), (name, k)
        assert "E" not in g0
        for k in ("w_ih", "w_hh", "b_ih", "b_hh"):
            assert np.array_equal(g0[k], g[k]), (name, k)


@pytest.mark.parametrize("name", edge_suite.STALE)
def test_x6_backward_ignores_what_the_workspace_held(name):
    """(a) a zeroed workspace, (b) the same bytes all 0xFF, (c) a workspace a step of the same shape on other wids, every length T, has
    just used (forward and X6 backward): rows beyond n_t, pad columns and steps past the longest question hold finite leftovers."""
    from neuralcx import _lib, ops
    _, gw, wids, dq_out, ref = case(name)
    de, dq, B, T = edges.CASES[name]
    runs = {}
    for tag, byte in (("a", 0), ("b", 0xFF)):
        w, ws = forward(name, True, fill=byte)
        runs[tag] = backward_c(name, w, ws, _lib.NCX_F_X6)
    ws = ops.gru_train_workspace(B, T, gw, DEV)
    ws.zero_()
    other = torch.from_numpy(edges.full_wids(name)).to(DEV)
    ops.gru_train_forward(other, gw, ws, x6=True)
    go = ops.gru_train_backward(other, gw, ws, torch.from_numpy(dq_out).to(DEV), x6=True)
    assert not np.array_equal(go["w_ih"].cpu().numpy(), runs["a"]["w_ih"])         # another step really ran there
    w, ws = forward(name, True, ws=ws)
    runs["c"] = backward_c(name, w, ws, _lib.NCX_F_X6)
    train_suite.check_grads(name + " (zeroed workspace)", runs["a"], ref)
    for tag in ("b", "c"):
        for k in GKEYS:
            assert np.isfinite(runs[tag][k]).all() and np.array_equal(runs[tag][k], runs["a"][k]), (name, tag, k)


@pytest.mark.parametrize("name", ["ragged", "fall", "steps"])
def test_flag_zero_is_the_flagless_entry_bit_for_bit(name):
    w, ws = forward(name, False)
    a = backward_c(name, w, ws, 0)
    b = backward_c(name, w, ws, None, entry="ncx_gru_train_backward")
    for k in GKEYS:
        assert np.array_equal(a[k], b[k]), (name, k)


@pytest.mark.parametrize("dropout", [0.0, 0.25])
def test_training_module_with_hip_x6_agrees_with_the_torch_path(dropout, monkeypatch):
    from neuralcx import ops
    _, wids, dq_out, _, _, _ = train_suite.case("ragged")
    hip, ref = train_suite._module_pair("ragged", dropout)
    hip.hip_x6 = True
    seen = []
    real = ops.gru_train_backward
    monkeypatch.setattr(ops, "gru_train_backward", lambda *a, **k: (seen.append(k.get("x6")), real(*a, **k))[1])
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
    assert float((outs[0] - outs[1]).abs().max()) <= TOL * float(outs[1].abs().max())
    for (n, p), (_, r) in zip(hip.named_parameters(), ref.named_parameters()):
        err, mx = float((p.grad - r.grad).abs().max()), float(r.grad.abs().max())
        print("dropout %.2f %s: max|hip x6 - torch| = %.3e of max %.3e" % (dropout, n, err, mx))
        assert mx > 0 and err <= TOL * mx, n


def test_cli_trains_with_the_x6_backward(tmp_path, capsys, monkeypatch):
    import importlib.util
    from neuralcx import ops
    spec = importlib.util.spec_from_file_location("vqa_train_cli_gru_bwd_x6_gpu", os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    y = tmp_path / "o.yaml"
    y.write_text(train_suite.TINY_YAML % str(tmp_path / "logs"))
    losses, seen, before = [], [], []
    real_step, real_epoch, real_bwd = cli.Trainer._step, cli.Trainer.run_epoch, ops.gru_train_backward

    def step(self, split, sel, train):
        r = real_step(self, split, sel, train)
        if train:
            losses.append(float(r[0]))
        return r

    def run_epoch(self, epoch):
        before.append(float(self.evaluate()["loss"]))
        return real_epoch(self, epoch)
    monkeypatch.setattr(cli.Trainer, "_step", step)
    monkeypatch.setattr(cli.Trainer, "run_epoch", run_epoch)
    monkeypatch.setattr(ops, "gru_train_backward", lambda *a, **k: (seen.append(k.get("x6")), real_bwd(*a, **k))[1])
    r = cli.main(["--path_opt", str(y), "--synthetic", "--syn_examples", "384", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0",
                  "--hip_seq2vec_train", "--x6_seq2vec", "--epochs", "1"])
    text = capsys.readouterr().out
    assert "question encoder: HIP forward + backward through time" in text
    assert "(question encoder: bf16 x 6 step kernel) (and the bf16 x 6 products of its backward)" in text
    enc = r["trainer"].model.seq2vec
    assert enc.hip_x6 is True and enc.use_hip_train is True
    after = float(r["history"][0]["val"]["loss"])
    print("train losses", ["%.3f" % x for x in losses], "val before %.4f after %.4f" % (before[0], after))
    assert len(losses) >= 8 and len(seen) == len(losses) and all(x is True for x in seen)      # the backward saw x6=True at every step
    assert all(np.isfinite(losses)) and np.isfinite(after)
    assert after <= before[0]                                   # falling or flat, on the validation split (a single step's training loss is noise)
