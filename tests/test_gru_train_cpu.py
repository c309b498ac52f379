"""CPU: training the question encoder in HIP, everything around the kernels -- the fp64 restatement against the fixture (torch autograd
through the project's GRUEncoder), the padding row, the transposed pack's layout, the C ABI's declarations and refusals, the module's
switch and the CLI flag.  No compute on a device."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT
from gru_ref import lengths
from gru_train_ref import GRADS, gru_train

CASES = ("c0", "c1")
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
GKEY = {"E": "dE", "w_ih": "dweight_ih_l0", "w_hh": "dweight_hh_l0", "b_ih": "dbias_ih_l0", "b_hh": "dbias_hh_l0"}
SYMS = ("ncx_gru_train_workspace_bytes", "ncx_gru_packed_t_bytes", "ncx_gru_pack_t", "ncx_gru_train_forward", "ncx_gru_train_backward")


def load_case(name):
    g = np.load(os.path.join(GOLDEN, "g18_gru_train.npz"))
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}


def ref_of(c):
    return gru_train(c["wids"], c["E"], *[c[k] for k in WKEYS], c["dq_out"])


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_reproduces_the_fixture(name):
    """torch's fp32 CPU autograd against fp64: 1e-6 on q (as g15), and 2e-6 of each gradient's max -- a few fp32 roundings through at most
    7 steps; the GPU bound is 1e-4 of the max."""
    c = load_case(name)
    ref = ref_of(c)
    assert float(np.abs(ref["q"] - c["q"]).max()) <= 1e-6
    for k in GRADS:
        err, m = float(np.abs(ref[k] - c[GKEY[k]]).max()), float(np.abs(ref[k]).max())
        print(name, k, "max|torch fp32 autograd - fp64| = %.3e of max %.3e" % (err, m))
        assert ref[k].shape == c[GKEY[k]].shape and m > 0
        assert err <= 2e-6 * m, k


def test_fixture_has_the_planted_rows_and_the_padding_row_gets_no_gradient():
    c = load_case("c0")
    w = c["wids"]
    assert c["E"].shape == (51, 22) and w.shape == (5, 7) and c["weight_hh_l0"].shape == (300, 100)
    assert c["E"][0].any()                                       # row 0 is nonzero and READ by the empty row and the inner zero ...
    assert not w[0].any() and lengths(w)[0] == 1
    assert w[3, 4] == 0 and w[3, 5] != 0 and lengths(w)[3] == 6
    for name in CASES:                                           # ... and still gets no gradient, from torch or from the restatement
        cc = load_case(name)
        assert not cc["dE"][0].any() and not ref_of(cc)["E"][0].any()
    # the empty row's gradient counts: a one-hot dq_out on it moves the weights
    d = np.zeros_like(c["dq_out"])
    d[0] = c["dq_out"][0]
    g = gru_train(w, c["E"], *[c[k] for k in WKEYS], d)
    assert np.abs(g["w_ih"]).max() > 0 and np.abs(g["b_hh"]).max() > 0 and not g["w_hh"].any() and not g["E"].any()


def test_all_lengths_one_leave_dw_hh_exactly_zero():
    c = load_case("c1")
    w = np.zeros_like(c["wids"])
    w[:, 0] = c["wids"][:, 0]
    g = gru_train(w, c["E"], *[c[k] for k in WKEYS], c["dq_out"])
    assert not g["w_hh"].any() and g["w_ih"].any()


@pytest.mark.parametrize("name", CASES)
def test_transposed_pack_layout_round_trips(name):
    from neuralcx import _lib, ops
    c = load_case(name)
    w_ih, w_hh = torch.from_numpy(c["weight_ih_l0"]), torch.from_numpy(c["weight_hh_l0"])
    dq, de = w_hh.shape[1], w_ih.shape[1]
    packed_t = ops.gru_pack_t_layout(w_ih, w_hh)
    assert packed_t.numel() * 4 == _lib.lib().ncx_gru_packed_t_bytes(de, dq)
    ih, hh = ops.gru_unpack_t_layout(packed_t, de, dq)
    assert torch.equal(ih, w_ih) and torch.equal(hh, w_hh)
    dqp, rows_h = (dq + 31) // 32 * 32, (dq + 63) // 64 * 64
    P = packed_t[:rows_h * 3 * dqp].view(rows_h, 3, dqp).numpy()
    assert P[5, 2, 7] == c["weight_hh_l0"][2 * dq + 7, 5]        # WhhT[j][g dqp + u] = w_hh[g dq + u][j]
    assert not P[:, :, dq:].any() and not P[dq:].any()
    X = packed_t[rows_h * 3 * dqp:].view(64, 3, dqp).numpy()
    assert X[21, 1, 3] == c["weight_ih_l0"][dq + 3, 21] and not X[22:].any()


def test_symbols_declared_exported_and_cited():
    from neuralcx import _lib
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = _lib.lib()
    for s in SYMS:
        assert s in _lib.EXPORTS and s + "(" in hdr
        assert getattr(L, s).argtypes is not None
    assert "ncx_gru_train" in open(os.path.join(PKG, "Makefile")).read()


def test_invalid_arguments_are_refused():
    from neuralcx import _lib
    L = _lib.lib()
    n = L.ncx_gru_train_workspace_bytes(4, 7, 22, 100)
    assert n > L.ncx_gru_workspace_bytes(4, 7, 22, 100)
    for bad in ((0, 7, 22, 100), (4, 0, 22, 100), (4, 65, 22, 100), (4, 7, 0, 100), (4, 7, 22, 0)):
        assert L.ncx_gru_train_workspace_bytes(*bad) == 0
    assert L.ncx_gru_packed_t_bytes(22, 100) == (128 + 64) * 3 * 128 * 4
    assert L.ncx_gru_packed_t_bytes(0, 100) == 0 and L.ncx_gru_packed_t_bytes(22, -1) == 0
    # the stash at the real shape: h + 4 gate blocks + 4 gate-gradient blocks + dX + the plan
    real = L.ncx_gru_train_workspace_bytes(512, 26, 620, 2400)
    pairs = 512 * 26
    assert real >= pairs * (9 * 2400 + 620) * 4 and real < pairs * (9 * 2400 + 620) * 4 + (16 << 20)
    buf = (ctypes.c_float * 1024)()                              # never dereferenced: every call below is refused before a launch
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    assert L.ncx_gru_pack_t(None, p, 22, 100, p, None) == -1 and L.ncx_gru_pack_t(p, p, 22, 0, p, None) == -1
    fwd = lambda **k: L.ncx_gru_train_forward(*[k.get(a, d) for a, d in (("wids", p), ("B", 4), ("T", 7), ("E", p), ("V1", 31), ("de", 22), ("dq", 100),
                                                                          ("packed", p), ("ws", p), ("n", n), ("q", p), ("flag", p), ("s", None))])
    bwd = lambda **k: L.ncx_gru_train_backward(*[k.get(a, d) for a, d in (("wids", p), ("B", 4), ("T", 7), ("E", p), ("V1", 31), ("de", 22), ("dq", 100),
                                                                           ("packed_t", p), ("ws", p), ("n", n), ("dq_out", p), ("dW_ih", p), ("dW_hh", p),
                                                                           ("db_ih", p), ("db_hh", p), ("dE", None), ("s", None))])
    mis = ctypes.c_void_p(p.value + 16)
    for f in (fwd, bwd):
        assert f(T=65) == -1 and f(B=0) == -1 and f(V1=0) == -1 and f(wids=None) == -1 and f(ws=None) == -1
        assert f(n=n - 1) == -1 and f(ws=mis) == -1              # short / misaligned workspace
    assert fwd(flag=None) == -1 and fwd(q=None) == -1
    assert bwd(dq_out=None) == -1 and bwd(dW_hh=None) == -1 and bwd(packed_t=None) == -1


def test_module_switch_defaults_off_and_a_cpu_call_ignores_it():
    """With the switch set, a CPU call is bit for bit the call without it (same process, same torch kernels), and both sit on the fixture
    within the bounds of the restatement test above (the fixture may come from another CPU)."""
    from vqa.models.seq2vec import GRUEncoder
    assert GRUEncoder.use_hip_train is False
    c = load_case("c0")
    wids, d = torch.from_numpy(c["wids"]), torch.from_numpy(c["dq_out"])
    got = []
    for on in (True, False):
        enc = GRUEncoder(["w"] * 50, dim_q=100, dim_emb=22, dropout=0.25).eval()
        sd = {"embedding.weight": torch.from_numpy(c["E"])}
        sd.update({"gru." + k: torch.from_numpy(c[k]) for k in WKEYS})
        enc.load_state_dict(sd)
        if on:
            enc.use_hip_train = True
        assert not enc._hip_train_ok(wids)
        q = enc(wids)
        assert q.requires_grad
        (q * d).sum().backward()
        got.append((q.detach().numpy(), enc.gru.weight_hh_l0.grad.numpy(), enc.embedding.weight.grad.numpy()))
        assert "use_hip_train" not in enc.state_dict() and len(enc.state_dict()) == 5
    for x, y in zip(*got):
        assert np.array_equal(x, y)
    q, dw, dE = got[0]
    assert float(np.abs(q - c["q"]).max()) <= 2e-6
    assert float(np.abs(dw - c["dweight_hh_l0"]).max()) <= 4e-6 * float(np.abs(c["dweight_hh_l0"]).max())
    assert float(np.abs(dE - c["dE"]).max()) <= 4e-6 * float(np.abs(c["dE"]).max()) and not dE[0].any()


def test_cli_refuses_the_flag_with_no_hip():
    spec = importlib.util.spec_from_file_location("vqa_train_cli_gru", os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.build_parser().parse_args([]).hip_seq2vec_train is False          # a new flag: no default changes
    with pytest.raises(SystemExit) as e:
        cli.main(["--synthetic", "--hip_seq2vec_train", "--no_hip"])
    assert "--hip_seq2vec_train" in str(e.value) and "--no_hip" in str(e.value)
