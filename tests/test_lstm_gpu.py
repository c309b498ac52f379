"""GPU: the HIP two-layer LSTM question encoder (ops.lstm_encode, TwoLSTM's device path) against the fp64 restatement tests/lstm_ref.py.

Tolerance: 1e-4 absolute, the project's bound for forward outputs; every element of q lies in (-1, 1).  torch's own fp32 path stays
within 2.5e-6 of fp64 at the real dims with the weights x 3, 40 times inside the bound.
Shapes: the smallest at which 64-row x 32-unit tiles, 32-deep k-steps, the two input widths and the wavefront over the layers can go
wrong.  The LSTM weights of every case are nn.LSTM's init x 3, so that gates leave the linear range."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import lstm_ref
from conftest import PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

#         name       emb    H     B   T
SHAPES = {"unit":     (1,    1,    2,  2),     # smallest legal dims
          "one":      (22,   48,   1,  1),     # one row, one launch pair
          "ragged":   (22,  100,   5,  7),     # lengths {0, 1, 3, 7, 7}, a zero inside a question, E[0] nonzero
          "odd":      (7,    37,   5,  7),     # H % 4 != 0: q[:, H:] and the rows of h are unaligned
          "over32":   (33,   33,   9,  3),     # one past the 32-deep k-step
          "over64":   (65,   65,  65,  4),     # one past the 64-row tile
          "wide_e":   (1030, 12,   4,  3),     # emb >> H
          "wide_h":   (5,   136,   4,  3),     # emb << H
          "all1":     (40,  100,  70, 26),     # every length 1: layer 1 runs exactly its step 0
          "all26":    (40,  136,  70, 26),     # every length 26
          "fall":     (40,  136, 200, 26),     # one row of length 26: n_t falls to 1
          "long":     (6,    24, 300, 64),     # T = 64, B > 256, every length 0..64 planted
          "real":     (620, 1200,  40, 26)}    # the real dims, lengths 3..26
V = 50


def make_wids(name, B, T, rng):
    if name == "ragged":
        lens = [0, 1, 3, 7, 7]
    elif name == "odd":
        lens = [7, 0, 2, 5, 1]
    elif name == "all1":
        lens = [1] * B
    elif name == "all26":
        lens = [T] * B
    elif name == "long":
        lens = list(range(T + 1)) + list(rng.integers(0, T + 1, size=B - T - 1))
    elif name in ("fall", "real"):
        lens = list(rng.integers(3, T, size=B))                # 3..25
        if name == "fall":
            lens[B // 3] = T                                   # exactly one row of 26
        else:
            lens[: 24] = range(3, 27)                          # 3..26, each at least once
    else:
        lens = list(rng.integers(1, T + 1, size=B))
        lens[0] = T
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
        enc.embedding.weight[0] = torch.randn(emb) * 0.5       # the padding row is READ, never assumed zero
        for p in list(enc.rnn_0.parameters()) + list(enc.rnn_1.parameters()):
            p.mul_(3.0)
    return enc


def weights_of(enc):
    """(E, layer 0, layer 1) as numpy, the arguments of lstm_ref.lstm_encode after wids"""
    return (enc.embedding.weight.detach().cpu().numpy(),) + tuple(tuple(getattr(r, k).detach().cpu().numpy() for k in KEYS) for r in (enc.rnn_0, enc.rnn_1))


_CASES = {}


def case(name):
    """(encoder on the device, wids, fp64 reference, q of the HIP path) -- computed once, shared, never modified."""
    if name not in _CASES:
        from neuralcx import ops
        emb, H, B, T = SHAPES[name]
        enc = make_encoder(emb, H, seed=sorted(SHAPES).index(name))
        wids = make_wids(name, B, T, np.random.default_rng(7))
        ref = lstm_ref.lstm_encode(wids, *weights_of(enc))
        enc = enc.to(DEV)
        q = ops.lstm_encode(torch.from_numpy(wids).to(DEV), ops.lstm_weights(enc))
        ops.check_gru_ids(device=DEV)
        _CASES[name] = (enc, wids, ref, q.cpu().numpy())
    return _CASES[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_encode_matches_fp64(name):
    enc, wids, ref, q = case(name)
    emb, H, B, T = SHAPES[name]
    err = float(np.abs(q - ref).max())
    print("%s dims %s: max|hip - fp64| = %.3e, max|q| = %.3f" % (name, SHAPES[name], err, float(np.abs(ref).max())))
    assert q.shape == ref.shape == (B, 2 * H) and q.dtype == np.float32
    assert np.isfinite(q).all() and float(np.abs(q).max()) < 1.0
    assert err <= TOL


def test_planted_lengths():
    assert sorted(set(lstm_ref.lengths(case("long")[1]))) == list(range(1, 65))         # 0 counts as 64
    assert (case("long")[1] != 0).sum(1).min() == 0
    assert set(lstm_ref.lengths(case("all1")[1])) == {1}
    assert (lstm_ref.lengths(case("fall")[1]) == 26).sum() == 1
    assert set(lstm_ref.lengths(case("real")[1])) == set(range(3, 27))


def test_all_padding_row_of_the_ragged_case():
    enc, wids, ref, q = case("ragged")
    E, l0, l1 = weights_of(enc)
    T = wids.shape[1]
    assert E[0].any() and not wids[0].any() and wids[3, 4] == 0 and wids[3, 5] != 0
    # the row's value is T steps on E[0], selected at T - 1
    want = lstm_ref.lstm_encode(np.zeros((1, T), np.int64), E, l0, l1, lens=np.array([T]))
    assert float(np.abs(want[0] - ref[0]).max()) <= 1e-12      # (fp64; BLAS sums a one-row product in another order)
    assert float(np.abs(q[0] - want[0]).max()) <= TOL
    # a clamp to one step (the GRU stand-in's rule), or a padding row taken as zero, would miss it by far
    clamp = lstm_ref.lstm_encode(wids[:1], E, l0, l1, lens=np.array([1]))
    zero_row = lstm_ref.lstm_encode(wids[:1], np.zeros_like(E), l0, l1)
    assert float(np.abs(clamp - want).max()) > 100 * TOL
    assert float(np.abs(zero_row - want).max()) > 100 * TOL


def test_device_pack_equals_the_layout_restatement():
    from neuralcx import ops
    for name in ("ragged", "odd", "over32", "wide_e"):
        enc = case(name)[0]
        lw = ops.lstm_weights(enc)
        want = ops.lstm_pack_layout([getattr(enc.rnn_0, k) for k in KEYS], [getattr(enc.rnn_1, k) for k in KEYS])
        assert lw.packed.shape == want.shape and torch.equal(lw.packed, want), name
        for r, (w_ih, w_hh, b) in zip((enc.rnn_0, enc.rnn_1), lw.unpack()):
            assert torch.equal(w_ih, r.weight_ih_l0.detach()) and torch.equal(w_hh, r.weight_hh_l0.detach())
            assert torch.equal(b, (r.bias_ih_l0 + r.bias_hh_l0).detach())


def test_bit_identical_from_run_to_run():
    from neuralcx import ops
    for name in ("fall", "ragged", "long"):
        enc, wids, _, q = case(name)
        again = ops.lstm_encode(torch.from_numpy(wids).to(DEV), ops.lstm_weights(enc)).cpu().numpy()
        assert np.array_equal(again, q), name


@pytest.mark.parametrize("name", ["odd", "over64", "long"])
def test_q_does_not_depend_on_the_workspace(name):
    """Through the C ABI: a zeroed workspace and one filled with 0xFF (NaN as floats, -1 as ints) give the same bits."""
    from neuralcx import _lib, ops
    enc, wids, _, q = case(name)
    emb, H, B, T = SHAPES[name]
    lw = ops.lstm_weights(enc)
    L = _lib.lib()
    n = L.ncx_lstm2_workspace_bytes(B, T, emb, H)
    assert n > 0 and n % 256 == 0
    w = torch.from_numpy(wids).to(DEV).to(torch.int32).contiguous()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    stream = C.c_void_p(torch.cuda.current_stream().cuda_stream)
    outs = []
    for fill in (0, 0xFF):
        ws = torch.full((n + 256,), fill, dtype=torch.uint8, device=DEV)
        base = (ws.data_ptr() + 255) // 256 * 256
        out = torch.full((B, 2 * H), float("nan"), dtype=torch.float32, device=DEV)
        rc = L.ncx_lstm2_encode(C.c_void_p(w.data_ptr()), B, T, C.c_void_p(lw.E.data_ptr()), lw.V1, emb, H, C.c_void_p(lw.packed.data_ptr()),
                                C.c_void_p(base), n, C.c_void_p(out.data_ptr()), C.c_void_p(flag.data_ptr()), stream)
        assert rc == 0
        outs.append(out.cpu().numpy())
    assert int(flag.item()) == 0
    assert np.array_equal(outs[0], outs[1]) and np.array_equal(outs[0], q)


def test_row_order_is_the_input_order():
    from neuralcx import ops
    enc, wids, ref, q = case("fall")
    perm = np.random.default_rng(3).permutation(wids.shape[0])
    qp = ops.lstm_encode(torch.from_numpy(wids[perm]).to(DEV), ops.lstm_weights(enc)).cpu().numpy()
    assert float(np.abs(qp - ref[perm]).max()) <= TOL


def test_module_takes_the_hip_path_and_trains_under_autograd(monkeypatch):
    from neuralcx import ops
    enc, wids, ref, q = case("ragged")
    w = torch.from_numpy(wids).to(DEV)
    calls = []
    real = ops.lstm_encode
    monkeypatch.setattr(ops, "lstm_encode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        got = enc(w)
        first = enc.__dict__["_hip_lstm"][1]
        assert enc(w) is not None and enc.__dict__["_hip_lstm"][1] is first        # packed once while nothing changes
    assert calls == [1, 1] and got.is_cuda and got.dtype == torch.float32 and not got.requires_grad
    assert np.array_equal(got.cpu().numpy(), q)
    out = enc(w)                                               # grad mode on, parameters require grad: torch, with a graph
    assert calls == [1, 1] and out.requires_grad
    assert float((out.detach() - got).abs().max()) <= TOL
    enc.train()                                                # training (the device's RNN backward exists in training mode only)
    try:
        out = enc(w)
        assert calls == [1, 1] and out.requires_grad
        out.square().sum().backward()
        g = enc.rnn_1.weight_hh_l0.grad
        assert g is not None and float(g.abs().max()) > 0 and float(enc.embedding.weight.grad.abs().max()) > 0
    finally:
        enc.eval()
        enc.zero_grad(set_to_none=True)
    enc.use_hip = False
    try:
        with torch.no_grad():
            assert float((enc(w) - got).abs().max()) <= TOL and calls == [1, 1]
    finally:
        del enc.use_hip                                        # back to the class default
    enc.drop_hip_weights()
    assert "_hip_lstm" not in enc.__dict__


def test_out_of_range_word_id_is_clamped_and_reported():
    from neuralcx import ops
    enc, wids, _, q = case("ragged")
    lw = ops.lstm_weights(enc)
    for bad in (V + 1, -3, 2 ** 30):
        w = wids.copy()
        w[2, 0] = bad
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.lstm_encode(torch.from_numpy(w).to(DEV), lw, bad_flag=flag)
        with pytest.raises(IndexError):
            ops.check_gru_ids(flag)
        assert int(flag.item()) == 0                           # cleared by the check
        keep = [0, 1, 3, 4]                                    # the other rows are untouched by the bad one
        assert np.array_equal(got.cpu().numpy()[keep], q[keep])
    ops.lstm_encode(torch.from_numpy(w).to(DEV), lw)           # the default per-device flag: the one check_gru_ids reads
    with pytest.raises(IndexError):
        ops.check_gru_ids(device=DEV)
    ops.check_gru_ids(device=DEV)                              # cleared


def test_load_state_dict_invalidates_the_packed_weights():
    enc, wids, ref, q = case("ragged")
    emb, H, _, _ = SHAPES["ragged"]
    mine = make_encoder(emb, H, seed=sorted(SHAPES).index("ragged")).to(DEV)
    w = torch.from_numpy(wids).to(DEV)
    with torch.no_grad():
        assert np.array_equal(mine(w).cpu().numpy(), q)
        first = mine.__dict__["_hip_lstm"][1]
        other = make_encoder(emb, H, seed=99)
        mine.load_state_dict(other.state_dict())
        got = mine(w).cpu().numpy()
    assert mine.__dict__["_hip_lstm"][1] is not first
    assert float(np.abs(got - q).max()) > 100 * TOL
    assert float(np.abs(got - lstm_ref.lstm_encode(wids, *weights_of(other))).max()) <= TOL


YAML_2LSTM = os.path.join(PKG, "options", "vqa2", "mutan_noatt_train_2lstm.yaml")


def _counting(monkeypatch):
    from neuralcx import ops
    calls = []
    real = ops.lstm_encode
    monkeypatch.setattr(ops, "lstm_encode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    return calls


def test_vqa_forward_on_the_2lstm_yaml(monkeypatch):
    import yaml
    import vqa.models as M
    from vqa.models import seq2vec
    from vqa.models.cx import CXModelBase
    with open(YAML_2LSTM) as f:
        opt = yaml.safe_load(f)["model"]
    torch.manual_seed(0)
    vqa = M.factory(opt, ["w%d" % i for i in range(V)], ["a%d" % i for i in range(40)], cuda=True, data_parallel=False)
    assert type(vqa.seq2vec) is seq2vec.TwoLSTM and vqa.seq2vec.use_hip is True
    m = CXModelBase(vqa, knn_size=2).cuda().eval()
    B = 6
    torch.manual_seed(1)
    feats = (torch.randn(B, 3, opt["fusion"]["dim_v"]).abs() * 0.45).to(DEV)
    wids = torch.from_numpy(make_wids("fall", B, 26, np.random.default_rng(5))).to(DEV)
    calls = _counting(monkeypatch)
    on = m.vqa_forward(feats, wids)
    assert calls == [1] and on[4].shape == (B, 2400)
    vqa.seq2vec.use_hip = False
    off = m.vqa_forward(feats, wids)
    assert calls == [1]
    err = float((on[4] - off[4]).abs().max())
    print("vqa_forward q_emb: max|hip - torch| = %.3e" % err)
    assert err <= TOL
    for a, b in zip(on[:4], off[:4]):
        assert a.shape == b.shape and torch.isfinite(a).all()


def test_train_cli_freezes_the_2lstm_encoder(tmp_path, monkeypatch):
    import importlib.util
    spec = importlib.util.spec_from_file_location("vqa_train_cli_lstm", os.path.join(PKG, "train.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    from vqa.models import seq2vec
    calls = _counting(monkeypatch)
    args = ["--path_opt", YAML_2LSTM, "--dir_logs", str(tmp_path / "logs"), "--synthetic", "--syn_examples", "256", "--syn_images", "32",
            "--syn_vocab", "30", "--print_freq", "0", "--freeze_seq2vec", "--epochs", "1", "-b", "128", "--save_model", "false"]
    run = cli.main(args)
    tr = run["trainer"]
    enc = tr.model.seq2vec
    assert type(enc) is seq2vec.TwoLSTM and tr.engine is not None and len(calls) >= 2      # one call per split
    assert [h["epoch"] for h in run["history"]] == [1] and np.isfinite(run["history"][0]["train"]["loss"])
    q = tr.q_emb_of(tr.val)
    assert q.shape == (tr.val.N, 2400)
    enc.use_hip = False
    with torch.no_grad():
        off = enc(tr.val.wids)
    err = float((q - off).abs().max())
    print("train.py --freeze_seq2vec q_emb: max|hip - torch| = %.3e" % err)
    assert err <= TOL
    with pytest.raises(SystemExit):                            # the encoder trains under autograd only
        cli.main([a for a in args if a != "--freeze_seq2vec"] + ["--hip_seq2vec_train"])
