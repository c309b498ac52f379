"""CPU: training the two-layer LSTM question encoder in HIP, everything around the kernels -- the fp64 restatement against the fixture
(torch autograd through the project's TwoLSTM) and against torch's own fp64 autograd, the padding row, the transposed pack's layout, the
C ABI's declarations and refusals, the module's switch and the CLI flag.  No compute on a device."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT
from lstm_ref import lengths
from lstm_train_ref import GRADS, lstm_train

CASES = ("c0", "c1")
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
GKEY = {"E": "dE"}
GKEY.update({"%s%d" % (s, l): "drnn_%d.%s" % (l, k) for l in (0, 1) for s, k in zip(("w_ih", "w_hh", "b_ih", "b_hh"), WKEYS)})
SYMS = ("ncx_lstm2_train_workspace_bytes", "ncx_lstm2_packed_t_bytes", "ncx_lstm2_pack_t", "ncx_lstm2_train_forward", "ncx_lstm2_train_backward")
YAML_2LSTM = os.path.join(PKG, "options", "vqa2", "mutan_noatt_train_2lstm.yaml")


def load_case(name):
    g = np.load(os.path.join(GOLDEN, "g20_lstm_train.npz"))
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}


def layers_of(c):
    return tuple(tuple(c["rnn_%d.%s" % (l, k)] for k in WKEYS) for l in (0, 1))


def ref_of(c, dq_out=None, wids=None):
    l0, l1 = layers_of(c)
    return lstm_train(c["wids"] if wids is None else wids, c["E"], l0, l1, c["dq_out"] if dq_out is None else dq_out)


def encoder_of(c, dtype=torch.float32):
    from vqa.models.seq2vec import TwoLSTM
    H, emb = c["rnn_0.weight_hh_l0"].shape[1], c["E"].shape[1]
    enc = TwoLSTM(["w"] * (c["E"].shape[0] - 1), emb, H).eval()
    sd = {"embedding.weight": torch.from_numpy(c["E"])}
    sd.update({"rnn_%d.%s" % (l, k): torch.from_numpy(c["rnn_%d.%s" % (l, k)]) for l in (0, 1) for k in WKEYS})
    enc.load_state_dict(sd, strict=True)
    return enc.to(dtype)


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_reproduces_the_fixture(name):
    """torch's fp32 CPU autograd against fp64: 1e-6 on q (as g19), and 4e-6 of each gradient's max -- a few fp32 roundings through at most
    7 steps of two layers; the GPU bound is 1e-4 of the max."""
    c = load_case(name)
    ref = ref_of(c)
    assert float(np.abs(ref["q"] - c["q"]).max()) <= 1e-6
    for k in GRADS:
        err, m = float(np.abs(ref[k] - c[GKEY[k]]).max()), float(np.abs(ref[k]).max())
        print(name, k, "max|torch fp32 autograd - fp64| = %.3e of max %.3e" % (err, m))
        assert ref[k].shape == c[GKEY[k]].shape and m > 0
        assert err <= 4e-6 * m, k


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_equals_torch_fp64_autograd(name):
    c = load_case(name)
    ref = ref_of(c)
    enc = encoder_of(c, torch.float64)
    q = enc(torch.from_numpy(c["wids"]))
    (q * torch.from_numpy(c["dq_out"]).double()).sum().backward()
    assert float(np.abs(q.detach().numpy() - ref["q"]).max()) <= 1e-9
    got = {"E": enc.embedding.weight.grad}
    got.update({"%s%d" % (s, l): getattr(getattr(enc, "rnn_%d" % l), k).grad for l in (0, 1) for s, k in zip(("w_ih", "w_hh", "b_ih", "b_hh"), WKEYS)})
    for k in GRADS:
        err, m = float(np.abs(got[k].numpy() - ref[k]).max()), float(np.abs(ref[k]).max())
        print(name, k, "max|torch fp64 autograd - restatement| = %.3e of max %.3e" % (err, m))
        assert err <= 1e-9 * max(m, 1.0), k


def test_fixture_has_the_planted_rows_and_the_padding_row_gets_no_embedding_gradient():
    c = load_case("c0")
    w = c["wids"]
    assert c["E"].shape == (51, 10) and w.shape == (5, 7) and c["rnn_1.weight_ih_l0"].shape == (96, 24)
    assert os.path.getsize(os.path.join(GOLDEN, "g20_lstm_train.npz")) < 300 * 1024
    assert c["E"][0].any()                                       # row 0 is nonzero and READ by the all-padding row and the inner zero ...
    assert not w[0].any() and lengths(w)[0] == 7                 # ... over all T steps (select_last's index -1)
    assert w[3, 4] == 0 and w[3, 5] != 0 and lengths(w)[3] == 6
    for name in CASES:                                           # ... and still gets no gradient, from torch or from the restatement
        cc = load_case(name)
        assert not cc["dE"][0].any() and not ref_of(cc)["E"][0].any()
    # the all-padding row's weight gradients count, its dE does not: a one-hot dq_out on it moves the weights and nothing of E
    d = np.zeros_like(c["dq_out"])
    d[0] = c["dq_out"][0]
    g = ref_of(c, dq_out=d)
    assert all(np.abs(g[k]).max() > 0 for k in GRADS if k != "E") and not g["E"].any()


def test_all_lengths_one_leave_both_dw_hh_exactly_zero_and_dw_ih1_not():
    c = load_case("c1")
    w = np.zeros_like(c["wids"])
    w[:, 0] = np.maximum(c["wids"][:, 0], 1)
    assert (lengths(w) == 1).all()
    g = ref_of(c, wids=w)
    assert not g["w_hh0"].any() and not g["w_hh1"].any() and g["w_ih0"].any() and g["w_ih1"].any()
    g = ref_of(c, wids=w[:, :1])                                 # T = 1
    assert not g["w_hh0"].any() and not g["w_hh1"].any() and g["w_ih1"].any()


@pytest.mark.parametrize("name", CASES)
def test_transposed_pack_layout_round_trips(name):
    from neuralcx import _lib, ops
    c = load_case(name)
    (w_ih0, w_hh0, _, _), (w_ih1, w_hh1, _, _) = [[torch.from_numpy(a) for a in l] for l in layers_of(c)]
    H, emb = w_hh0.shape[1], w_ih0.shape[1]
    packed_t = ops.lstm_pack_t_layout(w_ih0, w_hh0, w_ih1, w_hh1)
    assert packed_t.numel() * 4 == _lib.lib().ncx_lstm2_packed_t_bytes(emb, H)
    for got, want in zip(ops.lstm_unpack_t_layout(packed_t, emb, H), (w_ih0, w_hh0, w_ih1, w_hh1)):
        assert torch.equal(got, want)
    Hp, rows_h = (H + 31) // 32 * 32, (H + 63) // 64 * 64
    P0 = packed_t[:rows_h * 8 * Hp].view(rows_h, 8, Hp).numpy()
    assert P0[5, 2, 7] == w_hh0.numpy()[2 * H + 7, 5]           # P0[j][g Hp + u] = w_hh0[g H + u][j]
    assert P0[5, 4 + 3, 9] == w_ih1.numpy()[3 * H + 9, 5]       # P0[j][4 Hp + g Hp + u] = w_ih1[g H + u][j]
    assert not P0[:, :, H:].any() and not P0[H:].any()
    P1 = packed_t[rows_h * 8 * Hp:rows_h * 12 * Hp].view(rows_h, 4, Hp).numpy()
    assert P1[11, 1, 2] == w_hh1.numpy()[H + 2, 11] and not P1[H:].any()
    X = packed_t[rows_h * 12 * Hp:].view(64, 4, Hp).numpy()
    assert X[9, 1, 3] == w_ih0.numpy()[H + 3, 9] and not X[emb:].any()


def test_symbols_declared_exported_and_cited():
    from neuralcx import _lib
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = _lib.lib()
    for s in SYMS:
        assert s in _lib.EXPORTS and s + "(" in hdr
        assert getattr(L, s).argtypes is not None
    assert "ncx_lstm_train" in open(os.path.join(PKG, "Makefile")).read()
    at = hdr.index("csrc/ncx_lstm_train.hip")
    assert "seq2vec.py:48-76" in hdr[at:at + 600]               # the reference lines the entries replace


def test_invalid_arguments_are_refused():
    from neuralcx import _lib
    L = _lib.lib()
    n = L.ncx_lstm2_train_workspace_bytes(4, 7, 22, 100)
    assert n > L.ncx_lstm2_workspace_bytes(4, 7, 22, 100)
    for bad in ((0, 7, 22, 100), (4, 0, 22, 100), (4, 65, 22, 100), (4, 7, 0, 100), (4, 7, 22, 0)):
        assert L.ncx_lstm2_train_workspace_bytes(*bad) == 0
    assert L.ncx_lstm2_train_workspace_bytes(1, 1, 1, 1) > 0 and L.ncx_lstm2_train_workspace_bytes(1, 64, 1, 1) > 0
    assert L.ncx_lstm2_packed_t_bytes(22, 100) == (128 * 8 + 128 * 4 + 64 * 4) * 128 * 4
    assert L.ncx_lstm2_packed_t_bytes(0, 100) == 0 and L.ncx_lstm2_packed_t_bytes(22, -1) == 0
    # the stash at the real shape: per layer h + c + 4 gate blocks + 4 gate-gradient blocks, + dX + the plan
    real = L.ncx_lstm2_train_workspace_bytes(512, 26, 620, 1200)
    per_pair = 2 * (2 * 1200 + 8 * 1216) + 620
    assert real >= 512 * 26 * per_pair * 4 and real < 512 * 26 * per_pair * 4 + (16 << 20)
    buf = (ctypes.c_float * 1024)()                              # never dereferenced: every call below is refused before a launch
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    assert L.ncx_lstm2_pack_t(None, p, p, p, 22, 100, p, None) == -1 and L.ncx_lstm2_pack_t(p, p, p, None, 22, 100, p, None) == -1
    assert L.ncx_lstm2_pack_t(p, p, p, p, 22, 0, p, None) == -1 and L.ncx_lstm2_pack_t(p, p, p, p, 22, 100, None, None) == -1
    fwd = lambda **k: L.ncx_lstm2_train_forward(*[k.get(a, d) for a, d in (("wids", p), ("B", 4), ("T", 7), ("E", p), ("V1", 31), ("emb", 22), ("H", 100),
                                                                            ("packed", p), ("ws", p), ("n", n), ("q", p), ("flag", p), ("s", None))])
    outs = ("dW_ih0", "dW_hh0", "db_ih0", "db_hh0", "dW_ih1", "dW_hh1", "db_ih1", "db_hh1")
    bwd = lambda **k: L.ncx_lstm2_train_backward(*[k.get(a, d) for a, d in (("wids", p), ("B", 4), ("T", 7), ("E", p), ("V1", 31), ("emb", 22), ("H", 100),
                                                                             ("packed_t", p), ("ws", p), ("n", n), ("dq_out", p)) + tuple((o, p) for o in outs)
                                                   + (("dE", None), ("s", None))])
    mis = ctypes.c_void_p(p.value + 16)
    for f in (fwd, bwd):
        assert f(T=65) == -1 and f(T=0) == -1 and f(B=0) == -1 and f(V1=0) == -1 and f(emb=0) == -1 and f(H=0) == -1
        assert f(wids=None) == -1 and f(E=None) == -1 and f(ws=None) == -1
        assert f(n=n - 1) == -1 and f(ws=mis) == -1              # short / misaligned workspace
    assert fwd(flag=None) == -1 and fwd(q=None) == -1 and fwd(packed=None) == -1
    assert bwd(dq_out=None) == -1 and bwd(packed_t=None) == -1
    for o in outs:
        assert bwd(**{o: None}) == -1, o


def test_ops_wrappers_check_their_arguments():
    from neuralcx import ops
    c = load_case("c0")
    l0, l1 = [[torch.from_numpy(a) for a in l] for l in layers_of(c)]
    E = torch.from_numpy(c["E"])
    with pytest.raises(ValueError):
        ops.lstm_train_weights(E, *l0)                           # four tensors, not eight
    with pytest.raises(ValueError):
        ops.lstm_train_weights(E, *(l0 + [l1[0].t().contiguous()] + l1[1:]))
    with pytest.raises(Exception):
        ops.lstm_train_weights(E.double(), *(l0 + l1))


def test_module_switch_defaults_off_and_a_cpu_call_ignores_it():
    """With the switch set, a CPU call is bit for bit the call without it (same process, same torch kernels), and both sit on the fixture
    within the bounds of the restatement test above (the fixture may come from another CPU)."""
    from vqa.models.seq2vec import TwoLSTM
    assert TwoLSTM.use_hip_bptt is False
    assert not hasattr(TwoLSTM, "use_hip_train")                 # train.py --hip_seq2vec_train tells the encoders apart by that name
    c = load_case("c0")
    wids, d = torch.from_numpy(c["wids"]), torch.from_numpy(c["dq_out"])
    got = []
    for on in (True, False):
        enc = encoder_of(c)
        if on:
            enc.use_hip_bptt = True
        assert not enc._hip_bptt_ok(wids)
        q = enc(wids)
        assert q.requires_grad
        (q * d).sum().backward()
        got.append((q.detach().numpy(), enc.rnn_1.weight_hh_l0.grad.numpy(), enc.embedding.weight.grad.numpy()))
        assert "use_hip_bptt" not in enc.state_dict() and len(enc.state_dict()) == 9
    for x, y in zip(*got):
        assert np.array_equal(x, y)
    q, dw, dE = got[0]
    assert float(np.abs(q - c["q"]).max()) <= 2e-6
    assert float(np.abs(dw - c["drnn_1.weight_hh_l0"]).max()) <= 8e-6 * float(np.abs(c["drnn_1.weight_hh_l0"]).max())
    assert float(np.abs(dE - c["dE"]).max()) <= 8e-6 * float(np.abs(c["dE"]).max()) and not dE[0].any()


def _cli():
    spec = importlib.util.spec_from_file_location("vqa_train_cli_lstm", os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    return cli


def test_cli_flag_defaults_off_and_is_refused_three_ways():
    cli = _cli()
    args = cli.build_parser().parse_args([])
    assert args.hip_2lstm_train is False and args.hip_seq2vec_train is False      # a new flag: no default changes
    with pytest.raises(SystemExit) as e:
        cli.main(["--synthetic", "--path_opt", YAML_2LSTM, "--hip_2lstm_train", "--no_hip"])
    assert "--hip_2lstm_train" in str(e.value) and "--no_hip" in str(e.value)
    with pytest.raises(SystemExit) as e:
        cli.main(["--synthetic", "--path_opt", YAML_2LSTM, "--hip_2lstm_train", "--freeze_seq2vec"])
    assert "--hip_2lstm_train" in str(e.value) and "--freeze_seq2vec" in str(e.value)
    with pytest.raises(SystemExit) as e:                         # the default YAML builds the GRU stand-in
        cli.main(["--synthetic", "--hip_2lstm_train"])
    assert "--hip_2lstm_train" in str(e.value) and "2-lstm" in str(e.value)
