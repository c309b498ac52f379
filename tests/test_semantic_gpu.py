"""GPU: the semantic baseline scorer (reference vqa/models/cx.py:159-210) -- the cosine Gram against sklearn, the fused
scorer against the reference-pinned fixture and the fp64 restatement, its sweeps and edge cases, the drop-in module and
the CLI."""
import json
import os
import re

import numpy as np
import pytest
import torch

import semantic_ref as R
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _ops():
    from neuralcx import ops
    return ops


def _gaps_ok(scores, gt, min_gap=1e-4):
    """Recall@k is only pinned where no other candidate sits within min_gap of the ground truth's score."""
    sg = scores[np.arange(len(gt)), gt][:, None]
    d = np.abs(scores - sg)
    d[np.arange(len(gt)), gt] = np.inf
    return d.min(1) > min_gap


def _recall(scores, gt, k):
    top = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return (top == gt[:, None]).any(1)


def _case(seed, B, K, A, da=48, scale=3.0):
    rng = np.random.default_rng(seed)
    a = (rng.standard_normal((B, K, A)) * scale).astype(np.float32)
    aids = rng.integers(0, A, size=B).astype(np.int32)
    emb = rng.standard_normal((A, da)).astype(np.float32)
    return a, aids, emb


def _run(a, aids, gram_t, lam, want_raw=True):
    ops = _ops()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    out = ops.semantic_scores(torch.from_numpy(a).to(DEV), torch.from_numpy(aids).to(DEV), gram_t, lam, want_raw=want_raw, bad_flag=flag)
    ops.check_semantic_ids(flag)
    return [t.cpu().numpy() for t in out] if want_raw else out.cpu().numpy()


@pytest.mark.parametrize("A,da", [(2000, 2400), (1, 3), (7, 3), (7, 2401), (1999, 3), (1999, 2401)])
def test_cosine_gram_vs_sklearn(A, da):
    from sklearn.metrics.pairwise import cosine_similarity
    rng = np.random.default_rng(A + da)
    emb = rng.standard_normal((A, da)).astype(np.float32)
    if A >= 7:
        emb[A // 2] = 0                                     # zero row: all its similarities 0, the diagonal included
        emb[A - 1] = emb[1]                                  # duplicated row
    got = _ops().cosine_gram(torch.from_numpy(emb).to(DEV)).cpu().numpy()
    ref = cosine_similarity(emb.astype(np.float64))
    assert got.shape == (A, A)
    assert np.abs(got - ref).max() <= 2e-6, np.abs(got - ref).max()
    if A >= 7:
        assert not got[A // 2].any() and not got[:, A // 2].any()


def test_scores_match_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "g10_semantic.npz"))
    for c in ("c0", "c1", "c2"):
        gram = _ops().cosine_gram(torch.from_numpy(g[c + "/emb"]).to(DEV))
        for i, lam in enumerate(g[c + "/lams"]):
            sc, raw = _run(g[c + "/a_knns"], g[c + "/aids"], gram, float(lam))
            assert np.abs(sc - g[c + "/scores"][i]).max() <= 1e-5, (c, lam, np.abs(sc - g[c + "/scores"][i]).max())
            assert np.isfinite(raw).all()


def _check_vs_restatement(a, aids, emb, lam, gram=None):
    if gram is None:
        gram = _ops().cosine_gram(torch.from_numpy(emb).to(DEV))
    sc, raw = _run(a, aids, gram, lam)
    ref_sc, ref_raw = R.semantic_scores(a, aids, R.cosine_similarity(emb), lam)
    assert np.abs(raw - ref_raw).max() <= 1e-5, np.abs(raw - ref_raw).max()
    assert (np.abs(sc - ref_sc).max(1) <= 1e-5 * ref_sc.max(1)).all()
    return sc, ref_sc


def test_full_size_vs_restatement():
    B, K, A, da = 512, 24, 2000, 2400
    a, aids, emb = _case(7, B, K, A, da, scale=2.0)
    sc, ref_sc = _check_vs_restatement(a, aids, emb, 0.5)
    gt = np.random.default_rng(8).integers(0, K, size=B)
    ok = _gaps_ok(ref_sc, gt)
    assert ok.mean() > 0.5
    for k in (1, 5):
        assert (_recall(sc, gt, k)[ok] == _recall(ref_sc, gt, k)[ok]).all()


@pytest.mark.parametrize("K", [1, 2, 23, 24, 48, 64])
def test_sweep_K(K):
    a, aids, emb = _case(100 + K, 9, K, 300)
    _check_vs_restatement(a, aids, emb, 0.5)


@pytest.mark.parametrize("B", [1, 7, 513])
@pytest.mark.parametrize("lam", [0.0, 0.5, 1.0])
def test_sweep_B_lambda(B, lam):
    a, aids, emb = _case(200 + B, B, 24, 37 if B == 513 else 2000)
    _check_vs_restatement(a, aids, emb, lam)


@pytest.mark.parametrize("A", [1, 3, 5, 255, 257, 1023, 2049, 4096])
def test_widths(A):
    a, aids, emb = _case(300 + A, 5, 24, A)
    _check_vs_restatement(a, aids, emb, 0.3)


def test_large_logits_stay_finite():
    a, aids, emb = _case(11, 6, 24, 2000)
    a[:, :, :5] = 100.0                                      # NaN in the reference's softmax (exp overflow)
    a[0, 3, aids[0]] = 100.0
    gram = _ops().cosine_gram(torch.from_numpy(emb).to(DEV))
    sc, raw = _run(a, aids, gram, 0.5)
    assert np.isfinite(sc).all() and np.isfinite(raw).all()
    assert np.allclose(sc.sum(1), 1.0, atol=1e-5)
    _check_vs_restatement(a, aids, emb, 0.5, gram)


def test_bit_identical_repeats():
    a, aids, emb = _case(12, 64, 24, 2000)
    gram = _ops().cosine_gram(torch.from_numpy(emb).to(DEV))
    gram2 = _ops().cosine_gram(torch.from_numpy(emb).to(DEV))
    assert torch.equal(gram, gram2)
    s1, r1 = _run(a, aids, gram, 0.5)
    s2, r2 = _run(a, aids, gram, 0.5)
    assert (s1 == s2).all() and (r1 == r2).all()


def test_out_of_range_id_raises():
    ops = _ops()
    a, aids, emb = _case(13, 4, 24, 20)
    gram = ops.cosine_gram(torch.from_numpy(emb).to(DEV))
    for bad in (20, -1):
        ids = aids.copy(); ids[2] = bad
        flag = torch.zeros(1, dtype=torch.int32, device=DEV)
        sc = ops.semantic_scores(torch.from_numpy(a).to(DEV), torch.from_numpy(ids).to(DEV), gram, 0.5, bad_flag=flag)
        assert int(flag.item()) == 1
        assert torch.isnan(sc[2]).all() and torch.isfinite(sc[[0, 1, 3]]).all()
        with pytest.raises(IndexError):
            ops.check_semantic_ids(flag)
        ops.check_semantic_ids(flag)                          # cleared once reported
    ops.semantic_scores(torch.from_numpy(a).to(DEV), torch.full((4,), 99, dtype=torch.int32, device=DEV), gram, 0.5)
    with pytest.raises(IndexError):                           # the default per-device flag
        ops.check_semantic_ids(device=DEV)


def _tiny_vqa(A):
    import vqa.models as M
    opt = dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
               fusion=dict(dim_v=64, dim_q=48, dim_hv=16, dim_hq=16, dim_mm=16, R=3, dropout_v=0.5, dropout_q=0.5,
                           activation_v="tanh", activation_q="tanh", dropout_hv=0, dropout_hq=0),
               classif=dict(dropout=0.5))
    torch.manual_seed(0)
    return M.factory(opt, ["w%d" % i for i in range(30)], ["a%d" % i for i in range(A)], cuda=True, data_parallel=False)


def test_module_forward_on_mutan():
    from vqa.models.cx import SemanticBaseline
    A, B = 40, 6
    vqa = _tiny_vqa(A)
    m = SemanticBaseline(vqa, knn_size=24, trainable_vqa=False).cuda()
    feats = (torch.randn(B, 25, 64).abs() * 0.45).to(DEV)
    wids = torch.randint(1, 31, (B, 26)).to(DEV)
    aids = torch.randint(0, A, (B,)).to(DEV)
    s0 = m(feats, wids, aids)                                 # before set_answer_embedding: a zero Gram of the logits' width
    emb = np.random.default_rng(3).standard_normal((A, 2400)).astype(np.float32)
    emb[aids[0].item()] = 0
    m.set_answer_embedding(emb)
    m.set_lambda(0.25)
    s = m(feats, wids, aids)
    assert s.shape == (B, 24) and s.dtype == torch.float32 and s.requires_grad and s.is_cuda
    _, _, a_k, _, _ = m.vqa_forward(feats, wids)
    a_k = a_k.cpu().numpy()
    ref, _ = R.semantic_scores(a_k, aids.cpu().numpy(), R.cosine_similarity(emb), 0.25)
    assert np.abs(s.detach().cpu().numpy() - ref).max() <= 1e-5
    ref0, _ = R.semantic_scores(a_k, aids.cpu().numpy(), np.zeros((A, A)), 0.5)
    assert np.abs(s0.detach().cpu().numpy() - ref0).max() <= 1e-5
    assert np.abs(m.emb_pairs - R.cosine_similarity(emb)).max() <= 2e-6
    loss = torch.nn.CrossEntropyLoss()(s, torch.zeros(B, dtype=torch.long, device=DEV))
    loss.backward()                                           # the reference's train loop can call it; nothing trains
    assert all(k.startswith("vqa_model.") for k in m.state_dict())
    with pytest.raises(IndexError):
        m(feats, wids, torch.full((B,), A, dtype=torch.long, device=DEV))


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cx_cli_sem_gpu", os.path.join(PKG, "counterexamples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_synthetic_matches_restatement(tmp_path, capsys):
    cli = _cli()
    argv = ["--synthetic", "-cx", "SemanticBaseline", "-lb", "0.5", "-t", "-b", "64", "--syn_val", "160", "--syn_train", "64",
            "--syn_images", "512", "--project_dir", str(tmp_path)]
    res = cli.main(argv)
    out = capsys.readouterr().out
    assert re.search(r"Epoch 1 test: loss: [0-9.]+, recall: [0-9.]+", out) and "SemanticBaseline: 160 triplets" in out
    # the same triplets through the restatement
    from neuralcx.synth import SyntheticCX
    kw = dict(K=24, dv=2048, dq=2400, dz=360, A=2000, n_img=512, device=DEV)          # (load_synthetic with the default YAML)
    train = SyntheticCX(n_triplets=64, seed=1234, **kw)
    val = SyntheticCX(n_triplets=160, seed=4321, feats=train.feats, **kw)
    G = R.cosine_similarity(cli.synthetic_answer_embedding(2000))
    sc, gt = [], []
    for lo in range(0, 160, 64):
        sel = torch.arange(lo, min(lo + 64, 160), device=DEV)
        b, g = val.batch(sel, first_id=lo)
        sc.append(R.semantic_scores(b.a_knns.cpu().numpy(), b.answer_aids.cpu().numpy(), G, 0.5)[0]); gt.append(g.cpu().numpy())
    sc, gt = np.concatenate(sc), np.concatenate(gt)
    ok = _gaps_ok(sc, gt)
    assert ok.mean() > 0.8
    slack = (~ok).sum() / 160.0                              # a triplet with a near tie may rank either way
    for k in (1, 5):
        assert abs(res["recall_%d" % k] - _recall(sc, gt, k).mean()) <= slack + 1e-9, (k, slack)
    ce = np.mean(np.log(np.exp(sc).sum(1)) - sc[np.arange(160), gt])          # CrossEntropyLoss on the probabilities
    assert abs(res["loss"] - ce) < 1e-4
    runs = os.listdir(os.path.join(str(tmp_path), "logs", "cx"))
    with open(os.path.join(str(tmp_path), "logs", "cx", runs[0], "final_results.txt")) as f:
        assert json.load(f)["recall_5"] == res["recall_5"]


def test_cli_real_data_mode(tmp_path):
    from neuralcx import formats
    cli = _cli()
    paths = formats.write_synthetic_cx_files(os.path.join(str(tmp_path), "data"), n_train=64, n_val=96, n_img=200, seed=9)
    common = ["--path_opt", os.path.join(PKG, "options", "cx", "neuralcx_256_1_all.yaml"), "-b", "64", "--untrained_vqa",
              "--path_trainset", paths["path_trainset"], "--path_features", paths["path_features"], "--project_dir", str(tmp_path),
              "-cx", "SemanticBaseline", "-lb", "0.5"]
    res = cli.main(common)
    assert 0.0 <= res["recall_5"] <= 1.0 and np.isfinite(res["loss"])
    paths2 = formats.write_synthetic_cx_files(os.path.join(str(tmp_path), "data2"), n_train=64, n_val=96, n_img=200, seed=9,
                                              with_embedding=False)
    swap = {paths["path_trainset"]: paths2["path_trainset"], paths["path_features"]: paths2["path_features"]}
    common2 = [swap.get(x, x) for x in common]
    with pytest.raises(SystemExit, match=re.escape(os.path.join(paths2["path_trainset"], "answer_embedding.pickle"))):
        cli.main(common2)
