"""GPU: the HIP question encoder (ops.gru_encode, GRUEncoder's device path) against the fp64 restatement tests/gru_ref.py.

Tolerance: 1e-4 absolute, the project's bound for forward outputs; every element of q lies in (-1, 1).
Shapes: the smallest at which the step kernel (64 rows x 32 hidden units per workgroup, 32-deep k-steps) can go wrong."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG
from gru_ref import gru_encode as ref_encode

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL = 1e-4
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")

#         name       dim_emb dim_q  B   T
SHAPES = {"one":      (22,   48,    1,  1),     # one row, one step, below one unit tile, dim_emb no multiple of the MFMA k-step
          "ragged":   (22,  100,    5,  7),     # ragged unit tail; lengths {0, 1, 3, 7, 7}, a zero inside a question, E[0] nonzero
          "all1":     (40,  100,   70, 26),     # every length 1: no recurrent product runs; more than one row tile, ragged
          "all26":    (40,  136,   70, 26),     # every length 26: n_t constant
          "fall":     (40,  136,  200, 26),     # uniform 3..26 with exactly one row of 26: n_t falls to 1
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


def make_encoder(de, dq, seed):
    from vqa.models.seq2vec import GRUEncoder
    torch.manual_seed(seed)
    enc = GRUEncoder(["w%d" % i for i in range(V)], dim_q=dq, dim_emb=de, dropout=0.25).eval()
    with torch.no_grad():
        enc.embedding.weight[0] = torch.randn(de) * 0.5       # the padding row is READ, never assumed zero
    return enc


def weights_of(enc):
    return [enc.embedding.weight.detach().cpu().numpy()] + [getattr(enc.gru, k).detach().cpu().numpy() for k in WKEYS]


_CASES = {}


def case(name):
    """(encoder on the device, wids, fp64 reference, q of the HIP path) -- computed once, shared, never modified."""
    if name not in _CASES:
        from neuralcx import ops
        de, dq, B, T = SHAPES[name]
        enc = make_encoder(de, dq, seed=sorted(SHAPES).index(name))
        wids = make_wids(name, B, T, np.random.default_rng(7))
        ref = ref_encode(wids, *weights_of(enc))
        enc = enc.to(DEV)
        q = ops.gru_encode(torch.from_numpy(wids).to(DEV), ops.gru_weights(enc))
        ops.check_gru_ids(device=DEV)
        _CASES[name] = (enc, wids, ref, q.cpu().numpy())
    return _CASES[name]


@pytest.mark.parametrize("name", list(SHAPES))
def test_encode_matches_fp64(name):
    enc, wids, ref, q = case(name)
    err = float(np.abs(q - ref).max())
    print("%s dims %s: max|hip - fp64| = %.3e, max|q| = %.3f" % (name, SHAPES[name], err, float(np.abs(ref).max())))
    assert q.shape == ref.shape and q.dtype == np.float32
    assert np.isfinite(q).all() and float(np.abs(q).max()) < 1.0
    assert err <= TOL


def test_planted_rows_of_the_ragged_case():
    enc, wids, ref, q = case("ragged")
    E = enc.embedding.weight.detach().cpu().numpy()
    assert E[0].any() and not wids[0].any() and wids[3, 4] == 0 and wids[3, 5] != 0
    # the all-padding row is one step on E[0]: a kernel that assumed a zero padding row would return the bias-only state
    zero_row = ref_encode(wids[:1], np.zeros_like(E), *weights_of(enc)[1:])
    assert float(np.abs(zero_row - ref[:1]).max()) > 100 * TOL
    assert float(np.abs(q[0] - ref[0]).max()) <= TOL


def test_device_pack_equals_the_layout_restatement():
    from neuralcx import ops
    for name in ("ragged", "all26"):
        enc = case(name)[0]
        gw = ops.gru_weights(enc)
        want = ops.gru_pack_layout(*[getattr(enc.gru, k) for k in WKEYS])
        assert torch.equal(gw.packed, want)
        for got, k in zip(gw.unpack(), WKEYS):
            assert torch.equal(got, getattr(enc.gru, k).detach()), k


def test_bit_identical_from_run_to_run():
    from neuralcx import ops
    for name in ("fall", "ragged"):
        enc, wids, _, q = case(name)
        again = ops.gru_encode(torch.from_numpy(wids).to(DEV), ops.gru_weights(enc)).cpu().numpy()
        assert np.array_equal(again, q)


def test_row_order_is_the_input_order():
    from neuralcx import ops
    enc, wids, ref, q = case("fall")
    perm = np.random.default_rng(3).permutation(wids.shape[0])
    qp = ops.gru_encode(torch.from_numpy(wids[perm]).to(DEV), ops.gru_weights(enc)).cpu().numpy()
    assert float(np.abs(qp - ref[perm]).max()) <= TOL
    assert float(np.abs(qp - q[perm]).max()) <= TOL


def test_module_takes_the_hip_path_and_agrees_with_torch(monkeypatch):
    from neuralcx import ops
    enc, wids, ref, q = case("ragged")
    w = torch.from_numpy(wids).to(DEV)
    calls = []
    real = ops.gru_encode
    monkeypatch.setattr(ops, "gru_encode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        got = enc(w)
    assert calls == [1] and got.is_cuda and got.dtype == torch.float32 and not got.requires_grad
    assert np.array_equal(got.cpu().numpy(), q)
    out = enc(w)                                               # grad mode on, parameters require grad: torch, with a graph
    assert calls == [1] and out.requires_grad
    assert float((out.detach() - got).abs().max()) <= TOL
    enc.use_hip = False
    try:
        with torch.no_grad():
            assert float((enc(w) - got).abs().max()) <= TOL and calls == [1]
    finally:
        del enc.use_hip                                        # back to the class default


def test_out_of_range_word_id_raises_indexerror():
    from neuralcx import ops
    enc, wids, _, q = case("ragged")
    gw = ops.gru_weights(enc)
    for bad in (V + 1, -3, 2 ** 30):
        w = wids.copy()
        w[2, 0] = bad
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        got = ops.gru_encode(torch.from_numpy(w).to(DEV), gw, bad_flag=flag)
        with pytest.raises(IndexError):
            ops.check_gru_ids(flag)
        assert int(flag.item()) == 0                           # cleared by the check
        keep = [0, 1, 3, 4]                                    # the other rows are untouched by the bad one
        assert np.array_equal(got.cpu().numpy()[keep], q[keep])
    ops.gru_encode(torch.from_numpy(w).to(DEV), gw)            # the default per-device flag
    with pytest.raises(IndexError):
        ops.check_gru_ids(device=DEV)
    ops.check_gru_ids(device=DEV)                              # cleared


def test_load_state_dict_invalidates_the_packed_weights():
    enc, wids, ref, q = case("ragged")
    de, dq, _, _ = SHAPES["ragged"]
    mine = make_encoder(de, dq, seed=sorted(SHAPES).index("ragged")).to(DEV)
    w = torch.from_numpy(wids).to(DEV)
    with torch.no_grad():
        assert np.array_equal(mine(w).cpu().numpy(), q)
        first = mine.__dict__["_hip_gru"][1]
        assert mine(w) is not None and mine.__dict__["_hip_gru"][1] is first       # cached while nothing changes
        other = make_encoder(de, dq, seed=99)
        mine.load_state_dict(other.state_dict())
        got = mine(w).cpu().numpy()
    assert mine.__dict__["_hip_gru"][1] is not first
    want = ref_encode(wids, *weights_of(other))
    assert float(np.abs(got - q).max()) > 100 * TOL
    assert float(np.abs(got - want).max()) <= TOL


def _tiny_vqa(A):
    import vqa.models as M
    opt = dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
               fusion=dict(dim_v=64, dim_q=48, dim_hv=16, dim_hq=16, dim_mm=16, R=3, dropout_v=0.5, dropout_q=0.5,
                           activation_v="tanh", activation_q="tanh", dropout_hv=0, dropout_hq=0),
               classif=dict(dropout=0.5))
    torch.manual_seed(0)
    return M.factory(opt, ["w%d" % i for i in range(30)], ["a%d" % i for i in range(A)], cuda=True, data_parallel=False)


@pytest.mark.parametrize("which", ["NeuralModel", "SimilarityModel"])
def test_scorers_agree_with_the_encoder_on_and_off(which, monkeypatch):
    from neuralcx import ops
    from vqa.models.cx import NeuralModel, SimilarityModel
    A, B = 20, 6
    vqa = _tiny_vqa(A)
    if which == "NeuralModel":
        spec = dict(v_emb=True, v_mult=True, v_dist=True, v_rank=True, q_emb=True, a_emb=True, z_emb=True)
        m = NeuralModel(model_spec=spec, dim_h=16, n_layers=2, emb=None, drop_p=0.25, vqa_model=vqa, knn_size=24, trainable_vqa=False)
    else:
        m = SimilarityModel(vqa, knn_size=24, trainable_vqa=False)
    m = m.cuda().eval()
    torch.manual_seed(1)
    feats = (torch.randn(B, 25, 64).abs() * 0.45).to(DEV)
    wids = torch.zeros(B, 26, dtype=torch.long)
    for b in range(B):
        wids[b, :3 + 4 * b] = torch.randint(1, 31, (3 + 4 * b,))
    wids, aids = wids.to(DEV), torch.randint(0, A, (B,)).to(DEV)
    calls = []
    real = ops.gru_encode
    monkeypatch.setattr(ops, "gru_encode", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    assert vqa.seq2vec.use_hip is True
    with torch.no_grad():
        on = m(feats, wids, aids)
        assert len(calls) == 1                                 # vqa_forward reached the HIP encoder
        vqa.seq2vec.use_hip = False
        off = m(feats, wids, aids)
    assert len(calls) == 1
    err = float((on - off).abs().max())
    print(which, "max|scores(use_hip) - scores(torch encoder)| = %.3e" % err)
    assert err <= TOL


def test_cli_synthetic_has_no_encoder(tmp_path):
    import importlib.util
    spec = importlib.util.spec_from_file_location("cx_cli_gru_gpu", os.path.join(PKG, "counterexamples.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    base = ["--synthetic", "-cx", "DistanceBaseline", "-b", "64", "--syn_val", "128", "--syn_train", "64", "--syn_images", "512"]
    a = cli.main(base + ["--project_dir", str(tmp_path / "a")])
    b = cli.main(base + ["--no_hip_seq2vec", "--project_dir", str(tmp_path / "b")])
    assert a == b and a["recall_5"] >= 0.0
