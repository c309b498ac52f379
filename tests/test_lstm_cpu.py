"""CPU: the two-layer LSTM question encoder (seq2vec arch 2-lstm) around its kernels -- the reference's names, shapes, length and
selection rules (recorded in g19_lstm.npz), TwoLSTM's CPU path against the fixture and the fp64 restatement, the factory, the C ABI's
refusals and the packed layout.  No compute on a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lstm_ref
from conftest import GOLDEN, ROOT

CASES = ("c0", "c1")
SYMS = ("ncx_lstm2_packed_bytes", "ncx_lstm2_pack", "ncx_lstm2_workspace_bytes", "ncx_lstm2_encode")
KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
V, EMB, H = 30, 22, 50


def golden():
    return np.load(os.path.join(GOLDEN, "g19_lstm.npz"))


def load_case(name):
    g = golden()
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}


def layers_of(c):
    return tuple(tuple(c["%s.%s" % (r, k)] for k in KEYS) for r in ("rnn_0", "rnn_1"))


def encoder_of(c):
    from vqa.models.seq2vec import TwoLSTM
    V1, emb = c["E"].shape
    enc = TwoLSTM(["w"] * (V1 - 1), emb, c["rnn_0.weight_hh_l0"].shape[1])
    sd = {"embedding.weight": torch.from_numpy(c["E"])}
    sd.update({"%s.%s" % (r, k): torch.from_numpy(c["%s.%s" % (r, k)]) for r in ("rnn_0", "rnn_1") for k in KEYS})
    enc.load_state_dict(sd)
    return enc.eval()


def test_state_dict_is_the_references():
    from vqa.models.seq2vec import TwoLSTM
    g = golden()
    enc = TwoLSTM(["w"] * V, EMB, H)
    sd = enc.state_dict()
    assert list(sd.keys()) == [str(n) for n in g["ref/sd_names"]]
    for v, shape in zip(sd.values(), g["ref/sd_shapes"]):
        assert list(v.shape) == [int(s) for s in shape[:v.dim()]]
    # a reference-shaped state_dict loads (strict)
    ref_sd = {str(n): torch.full([int(s) for s in shape if s], 0.25) for n, shape in zip(g["ref/sd_names"], g["ref/sd_shapes"])}
    enc.load_state_dict(ref_sd)
    assert float(enc.rnn_1.weight_hh_l0.detach()[3, 3]) == 0.25
    assert enc.rnn_0.batch_first and enc.rnn_1.batch_first and "use_hip" not in sd


def test_length_and_selection_rules_are_the_references():
    g = golden()
    wids, ref_len = g["ref/wids"], g["ref/lengths"]
    T = wids.shape[1]
    assert not wids[0].any() and ref_len[0] == 0                  # all padding: process_lengths says 0 ...
    assert wids[1, 2] == 0 and wids[1, 3] != 0 and ref_len[1] == 4  # a zero inside a question shortens it
    assert ref_len[2] == T and ref_len[3] == 1
    mine = lstm_ref.lengths(wids)
    assert np.array_equal(np.where(ref_len > 0, ref_len, T), mine) and mine[0] == T
    x = g["ref/sel_x"]
    assert np.array_equal(g["ref/sel_out"][0], x[0, T - 1])      # ... and select_last's index -1 is step T - 1
    assert np.array_equal(lstm_ref.select_last(x, ref_len), g["ref/sel_out"])
    assert np.array_equal(lstm_ref.select_last(x, mine), g["ref/sel_out"])


def test_as_written_the_reference_depends_on_the_batch_position():
    """The deliberate difference: without batch_first the reference's recurrence runs over the batch axis."""
    g = golden()
    a, b, swap = g["ref/fwd"], g["ref/fwd_swapped"], g["ref/swap"]
    assert list(swap) == [0, 2, 1, 3] and np.array_equal(g["ref/fwd_wids"][swap][2], g["ref/fwd_wids"][1])
    d = float(np.abs(a[1] - b[2]).max())
    print("the same question at batch positions 1 and 2, as written: max|diff| = %.3f" % d)
    assert d > 1e-2


def test_fixture_has_the_planted_rows():
    c = load_case("c0")
    w = c["wids"]
    assert c["E"].shape == (V + 1, EMB) and w.shape == (9, 7) and c["q"].shape == (9, 2 * H)
    assert c["E"][0].any()
    assert not w[2].any() and lstm_ref.lengths(w)[2] == 7
    assert w[3, 2] == 0 and w[3, 3] != 0 and lstm_ref.lengths(w)[3] == 4
    assert lstm_ref.lengths(w)[0] == 7 and lstm_ref.lengths(w)[1] == 1
    assert np.array_equal(np.concatenate([c["x0"], c["x1"]], 1), c["q"])
    c1 = load_case("c1")
    assert np.abs(c1["q"]).max() > 0.7                           # weights x 3: gates outside the linear range


@pytest.mark.parametrize("name", CASES)
def test_cpu_module_equals_the_fixture(name):
    c = load_case(name)
    enc = encoder_of(c)
    assert enc.use_hip is True                                   # on by default; a CPU tensor never takes the HIP path
    with torch.no_grad():
        q = enc(torch.from_numpy(c["wids"])).numpy()
    err = float(np.abs(q - c["q"]).max())
    print(name, "max|module - fixture| = %.3e" % err)
    assert err <= 1e-6


@pytest.mark.parametrize("name", CASES)
def test_cpu_module_against_fp64(name):
    c = load_case(name)
    ref = lstm_ref.lstm_encode(c["wids"], c["E"], *layers_of(c))
    with torch.no_grad():
        q = encoder_of(c)(torch.from_numpy(c["wids"])).numpy()
    err = float(np.abs(q - ref).max())
    print(name, "max|torch fp32 nn.LSTM - fp64 restatement| = %.3e" % err)
    assert ref.shape == (9, 2 * H) and err <= 1e-5
    assert np.abs(ref).max() < 1.0


def test_a_row_alone_gives_the_same_vector():
    c = load_case("c1")
    enc = encoder_of(c)
    w = torch.from_numpy(c["wids"])
    with torch.no_grad():
        q = enc(w)
        for b in range(w.shape[0]):
            assert float((enc(w[b:b + 1])[0] - q[b]).abs().max()) <= 1e-6, b


def test_factory():
    from vqa.models import seq2vec
    vw = ["w"] * V
    enc = seq2vec.factory(vw, {"arch": "2-lstm", "emb_size": EMB, "hidden_size": H}, dim_q=2 * H)
    assert type(enc) is seq2vec.TwoLSTM and enc.rnn_0.input_size == EMB and enc.rnn_1.hidden_size == H
    assert type(seq2vec.factory(vw, {"arch": "2-lstm", "emb_size": EMB}, dim_q=2 * H)) is seq2vec.GRUEncoder
    assert type(seq2vec.factory(vw, {"arch": "gru", "emb_size": EMB, "hidden_size": H}, dim_q=2 * H)) is seq2vec.GRUEncoder
    with pytest.raises(ValueError):
        seq2vec.factory(vw, {"arch": "2-lstm", "emb_size": EMB, "hidden_size": H}, dim_q=2 * H + 2)
    with pytest.raises(KeyError):                                 # the reference reads both keys
        seq2vec.factory(vw, {"arch": "2-lstm", "hidden_size": H}, dim_q=2 * H)


def test_dropout_in_training_only():
    c = load_case("c0")
    enc = encoder_of(c)
    w = torch.from_numpy(c["wids"])
    with torch.no_grad():
        assert torch.equal(enc(w), enc(w))
        enc.train()
        torch.manual_seed(3)
        q = enc(w)
    zeros = float((q == 0).float().mean())
    assert 0.15 < zeros < 0.45                                   # p = 0.3 over 900 elements
    kept = q != 0
    assert np.allclose(q[kept].numpy() * 0.7, c["q"][kept.numpy()], atol=1e-6)


def test_selection_rule():
    class Cuda:
        is_cuda, shape = True, (3, 7)
        device = torch.device("cpu")

        def dim(self):
            return 2
    fake = Cuda()
    enc = encoder_of(load_case("c0"))
    assert not enc._hip_ok(fake)                                 # a parameter requires grad under enabled grad mode
    with torch.no_grad():
        assert enc._hip_ok(fake) and not enc._hip_ok(torch.zeros(3, 7, dtype=torch.long))
        enc.train()
        assert not enc._hip_ok(fake)                             # p = 0.3 is live
        enc.eval()
        enc.use_hip = False
        assert not enc._hip_ok(fake)


def test_symbols_declared_and_exported():
    from neuralcx import _lib
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = _lib.lib()
    for s in SYMS:
        assert s in _lib.EXPORTS and s + "(" in hdr
        assert getattr(L, s).argtypes is not None
    assert "seq2vec.py:48-76" in hdr and "seq2vec.py:86-89" in hdr and "seq2vec.py:11-25, 61-76" in hdr


def test_invalid_dims_are_refused():
    from neuralcx import _lib
    L = _lib.lib()
    assert L.ncx_lstm2_workspace_bytes(4, 7, 22, 50) > 0
    for bad in ((0, 7, 22, 50), (4, 0, 22, 50), (4, 65, 22, 50), (4, 7, 0, 50), (4, 7, 22, 0)):
        assert L.ncx_lstm2_workspace_bytes(*bad) == 0
    # H 50: 2 unit blocks of 128 weight rows; kp = 32 + 64 and 64 + 64; 256 bias floats per layer
    assert L.ncx_lstm2_packed_bytes(22, 50) == (256 * 96 + 256 + 256 * 128 + 256) * 4
    assert L.ncx_lstm2_packed_bytes(0, 50) == 0 and L.ncx_lstm2_packed_bytes(22, -1) == 0
    buf = (ctypes.c_float * 64)()                                # never dereferenced: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ncx_lstm2_pack(p, p, p, p, p, p, p, p, 0, 50, p, None) == -1
    assert L.ncx_lstm2_pack(p, p, p, p, None, p, p, p, 22, 50, p, None) == -1
    n = L.ncx_lstm2_workspace_bytes(4, 7, 22, 50)
    assert L.ncx_lstm2_encode(p, 4, 65, p, 31, 22, 50, p, p, n, p, p, None) == -1        # T > 64
    assert L.ncx_lstm2_encode(p, 0, 7, p, 31, 22, 50, p, p, n, p, p, None) == -1         # B < 1
    assert L.ncx_lstm2_encode(p, 4, 7, p, 0, 22, 50, p, p, n, p, p, None) == -1          # empty table
    assert L.ncx_lstm2_encode(p, 4, 7, p, 31, 22, 50, p, p, n, p, None, None) == -1      # no flag
    assert L.ncx_lstm2_encode(p, 4, 7, p, 31, 22, 50, p, p, n - 1, p, p, None) == -1     # short workspace


@pytest.mark.parametrize("name", CASES)
def test_pack_layout_round_trips(name):
    from neuralcx import _lib, ops
    c = load_case(name)
    lw = ops.lstm_weights(encoder_of(c))
    assert isinstance(lw, ops.LstmWeights) and (lw.V1, lw.emb, lw.H) == (V + 1, EMB, H)
    assert lw.packed.numel() * 4 == _lib.lib().ncx_lstm2_packed_bytes(EMB, H)
    for l, (w_ih, w_hh, b) in enumerate(lw.unpack()):
        r = "rnn_%d." % l
        assert np.array_equal(w_ih.numpy(), c[r + "weight_ih_l0"]) and np.array_equal(w_hh.numpy(), c[r + "weight_hh_l0"])
        assert np.array_equal(b.numpy(), c[r + "bias_ih_l0"] + c[r + "bias_hh_l0"])
    # the layout itself: unit 37 = block 1, slot 5; its i, f, g, o rows sit 32 rows apart in one block, x columns then h columns
    kp0, kp1 = 32 + 64, 64 + 64
    W0 = lw.packed[:256 * kp0].view(2, 4, 32, kp0).numpy()
    off1 = 256 * kp0 + 256
    W1 = lw.packed[off1:off1 + 256 * kp1].view(2, 4, 32, kp1).numpy()
    for g in range(4):
        assert np.array_equal(W0[1, g, 5, :22], c["rnn_0.weight_ih_l0"][g * H + 37])
        assert np.array_equal(W0[1, g, 5, 32:32 + H], c["rnn_0.weight_hh_l0"][g * H + 37])
        assert not W0[1, g, 5, 22:32].any() and not W0[1, g, 5, 32 + H:].any()
        assert np.array_equal(W1[1, g, 5, :H], c["rnn_1.weight_ih_l0"][g * H + 37])
        assert np.array_equal(W1[1, g, 5, 64:64 + H], c["rnn_1.weight_hh_l0"][g * H + 37])
    assert not W0[1, :, 18:].any() and not W1[1, :, 18:].any()   # units 50..63 do not exist
    b1 = lw.packed[off1 + 256 * kp1:].view(2, 4, 32).numpy()
    assert b1[1, 2, 5] == c["rnn_1.bias_ih_l0"][2 * H + 37] + c["rnn_1.bias_hh_l0"][2 * H + 37]
