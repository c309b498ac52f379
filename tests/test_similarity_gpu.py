"""GPU: the similarity scorer (reference vqa/models/cx.py:490-518) -- the fused kernel against the reference-pinned fixture and
the fp64 restatement at full size, its sweeps and edge cases, the drop-in module and the CLI."""
import json
import os
import re

import numpy as np
import pytest
import torch

import similarity_ref as R
from conftest import GOLDEN, PKG

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
TOL_SUM = 1e-4         # the project's logit tolerance: the sum and the cross-entropy term
TOL_COS = 1e-5         # values bounded by 1 (as tests/test_semantic_gpu.py)


def _ops():
    from neuralcx import ops
    return ops


def _gaps_ok(scores, gt, min_gap):
    """Recall@k is only pinned where no other candidate sits within min_gap of the ground truth's score."""
    sg = scores[np.arange(len(gt)), gt][:, None]
    d = np.abs(scores - sg)
    d[np.arange(len(gt)), gt] = np.inf
    return d.min(1) > min_gap


def _recall(scores, gt, k):
    top = np.argsort(-scores, axis=1, kind="stable")[:, :k]
    return (top == gt[:, None]).any(1)


def _case(seed, B, K, dv, dz, A, n_img=50):
    """Features |N(0, 1)| 0.45, z ~ N(0, 1), logits N(0, 2^2); row ids drawn from an n_img-row table (n_img small: duplicates)."""
    rng = np.random.default_rng(seed)
    feats = (np.abs(rng.standard_normal((n_img, dv), dtype=np.float32)) * np.float32(0.45))
    idx = rng.integers(0, n_img, size=(B, K + 1)).astype(np.int32)
    zo = rng.standard_normal((B, dz), dtype=np.float32)
    zk = rng.standard_normal((B, K, dz), dtype=np.float32)
    a = rng.standard_normal((B, K, A), dtype=np.float32) * np.float32(2.0)
    aids = rng.integers(0, A, size=B).astype(np.int32)
    return feats, idx, zo, zk, a, aids


def _run(feats, idx, zo, zk, a, aids, want_parts=True, check=True):
    ops = _ops()
    flag = torch.zeros(1, dtype=torch.int32, device=DEV)
    t = lambda x: x.to(DEV) if isinstance(x, torch.Tensor) else torch.from_numpy(x).to(DEV)
    out = ops.similarity_scores(t(feats), t(idx), t(zo), t(zk), t(a), t(aids), bad_flag=flag, want_parts=want_parts)
    if check:
        ops.check_similarity_ids(flag)
    return ([x.cpu().numpy() for x in out] if want_parts else out.cpu().numpy()), flag


def _assert_close(sc, parts, ref_sc, ref_parts, what):
    err = np.abs(parts - ref_parts).reshape(-1, 3).max(0)
    e_sum = np.abs(sc - ref_sc).max()
    print(what, "sum %.3g  v_cos %.3g  z_cos %.3g  xent %.3g" % (e_sum, err[0], err[1], err[2]))
    assert e_sum <= TOL_SUM and err[2] <= TOL_SUM, (what, e_sum, err)
    assert err[0] <= TOL_COS and err[1] <= TOL_COS, (what, err)


def _check_vs_restatement(case, what):
    (sc, parts), _ = _run(*case)
    ref_sc, ref_parts = R.similarity_scores_table(*case)
    _assert_close(sc, parts, ref_sc, ref_parts, what)
    (sc2), _ = _run(*case, want_parts=False)
    assert (sc2 == sc).all()                                  # the parts output does not change the scores
    return sc, ref_sc


def test_scores_match_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "g13_similarity.npz"))
    for c in ("c0", "c1", "c2"):
        v = g[c + "/v"]
        B, K1, dv = v.shape
        idx = np.arange(B * K1, dtype=np.int32).reshape(B, K1)
        (sc, parts), _ = _run(v.reshape(B * K1, dv), idx, g[c + "/z_orig"], g[c + "/z_knns"], g[c + "/a_knns"], g[c + "/aids"])
        _assert_close(sc, parts, g[c + "/scores"], g[c + "/parts"], c)


def test_fixture_planted_rows():
    g = np.load(os.path.join(GOLDEN, "g13_similarity.npz"))
    v = g["c0/v"]
    B, K1, dv = v.shape
    idx = np.arange(B * K1, dtype=np.int32).reshape(B, K1)
    (sc, parts), _ = _run(v.reshape(B * K1, dv), idx, g["c0/z_orig"], g["c0/z_knns"], g["c0/a_knns"], g["c0/aids"])
    assert parts[1, 3, 0] == 0 and not parts[2, :, 1].any()                 # an all-zero candidate row, an all-zero z_orig
    assert abs(parts[3, 2, 0] - 1) <= 1e-6 and abs(parts[3, 2, 1] - 1) <= 1e-6
    assert abs(parts[0, 5, 0] - 0.01) <= 1e-6                                # each norm clamped on its own
    assert np.isfinite(sc).all()


def test_full_size_vs_restatement():
    """B = 512, K = 24 at the real widths on an 82 783-row table.  With seeds 21 / 22 the fp64 scores leave 2 of the 512 rows
    (0.39 %) with another candidate within 2e-4 of the ground truth's score (restatement alone, on the CPU); the bound is 1 %."""
    B, K = 512, 24
    case = _case(21, B, K, 2048, 360, 2000, n_img=82783)
    sc, ref_sc = _check_vs_restatement(case, "full size")
    gt = np.random.default_rng(22).integers(0, K, size=B)
    ok = _gaps_ok(ref_sc, gt, 2e-4)                           # twice the score tolerance
    print("rows left out: %d of %d" % ((~ok).sum(), B))
    assert (~ok).mean() <= 0.01
    for k in (1, 5):
        assert (_recall(sc, gt, k)[ok] == _recall(ref_sc, gt, k)[ok]).all()


@pytest.mark.parametrize("K", [1, 2, 23, 24, 48, 64])
def test_sweep_K(K):
    _check_vs_restatement(_case(100 + K, 9, K, 256, 40, 300), "K=%d" % K)


@pytest.mark.parametrize("B", [1, 7, 513])
def test_sweep_B(B):
    _check_vs_restatement(_case(200 + B, B, 24, 2048 if B < 513 else 132, 360 if B < 513 else 24, 2000 if B < 513 else 37), "B=%d" % B)


@pytest.mark.parametrize("A", [1, 3, 255, 257, 2049, 4096])
def test_sweep_A(A):
    _check_vs_restatement(_case(300 + A, 5, 24, 64, 16, A), "A=%d" % A)


@pytest.mark.parametrize("dv", [1, 3, 5, 2047, 2048])
def test_sweep_dv(dv):
    _check_vs_restatement(_case(400 + dv, 5, 24, dv, 16, 100), "dv=%d" % dv)


@pytest.mark.parametrize("dz", [1, 359, 360])
def test_sweep_dz(dz):
    _check_vs_restatement(_case(500 + dz, 5, 24, 64, dz, 100), "dz=%d" % dz)


def test_wide_rows_take_the_global_path():
    """dv + dz beyond the kernel's LDS staging area (8192 floats): the originals are read from global memory instead."""
    _check_vs_restatement(_case(600, 3, 5, 8192, 360, 100, n_img=9), "dv=8192")
    _check_vs_restatement(_case(601, 3, 5, 8191, 7, 100, n_img=9), "dv=8191")


def test_table_ids_with_duplicates():
    """Real row ids into a table, not arange: ids repeated inside one question (the original among its own candidates too)."""
    feats, idx, zo, zk, a, aids = _case(31, 6, 24, 2048, 360, 2000, n_img=300)
    idx[0, 5] = idx[0, 9] = idx[0, 17]                        # one candidate three times
    idx[1, 4] = idx[1, 0]                                     # the original as its own candidate: v_cos = 1
    idx[2, :] = idx[2, 0]                                     # every row the same
    idx[3, 1:] = np.arange(299, 299 - 24, -1)                 # descending, the table's last row included
    case = (feats, idx, zo, zk, a, aids)
    _check_vs_restatement(case, "table ids")
    (sc, parts), _ = _run(*case)
    assert parts[0, 4, 0] == parts[0, 8, 0] == parts[0, 16, 0]
    assert abs(parts[1, 3, 0] - 1) <= 1e-6 and np.abs(parts[2, :, 0] - 1).max() <= 1e-6


def test_bit_identical_repeats():
    case = _case(12, 64, 24, 2048, 360, 2000, n_img=500)
    (s1, p1), _ = _run(*case)
    (s2, p2), _ = _run(*case)
    assert (s1 == s2).all() and (p1 == p2).all()


def test_out_of_range_ids_set_the_flag():
    ops = _ops()
    feats, idx, zo, zk, a, aids = _case(13, 4, 24, 64, 16, 20, n_img=30)
    (clean, clean_parts), _ = _run(feats, idx, zo, zk, a, aids)
    for col, bad in ((3, 30), (0, 30), (24, -1), (7, 2 ** 31 - 1)):          # a bad feature row id: candidate, original, last
        ids = idx.copy(); ids[2, col] = bad
        (sc, parts), flag = _run(feats, ids, zo, zk, a, aids, check=False)
        assert int(flag.item()) == 1
        assert np.isnan(sc[2]).all() and np.isnan(parts[2]).all()
        assert (sc[[0, 1, 3]] == clean[[0, 1, 3]]).all() and (parts[[0, 1, 3]] == clean_parts[[0, 1, 3]]).all()
        with pytest.raises(IndexError):
            ops.check_similarity_ids(flag)
        ops.check_similarity_ids(flag)                        # cleared once reported
    for bad in (20, -1):                                      # a bad answer id
        ans = aids.copy(); ans[1] = bad
        sc, flag = _run(feats, idx, zo, zk, a, ans, want_parts=False, check=False)
        assert int(flag.item()) == 1
        assert np.isnan(sc[1]).all() and (sc[[0, 2, 3]] == clean[[0, 2, 3]]).all()
        with pytest.raises(IndexError):
            ops.check_similarity_ids(flag)
    t = lambda x: torch.from_numpy(x).to(DEV)
    ops.similarity_scores(t(feats), t(idx), t(zo), t(zk), t(a), torch.full((4,), 99, dtype=torch.int32, device=DEV))
    with pytest.raises(IndexError):                           # the default per-device flag
        ops.check_similarity_ids(device=DEV)


def test_unsupported_dims():
    from neuralcx import _lib
    for K, A in ((65, 20), (3, 4097)):
        case = _case(14, 2, K, 8, 4, A)
        with pytest.raises(_lib.NcxError, match="NCX_E_DIMS"):
            _run(*case)


def _tiny_vqa(A):
    import vqa.models as M
    opt = dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
               fusion=dict(dim_v=64, dim_q=48, dim_hv=16, dim_hq=16, dim_mm=16, R=3, dropout_v=0.5, dropout_q=0.5,
                           activation_v="tanh", activation_q="tanh", dropout_hv=0, dropout_hq=0),
               classif=dict(dropout=0.5))
    torch.manual_seed(0)
    return M.factory(opt, ["w%d" % i for i in range(30)], ["a%d" % i for i in range(A)], cuda=True, data_parallel=False)


def test_module_forward_on_mutan():
    from vqa.models.cx import SimilarityModel
    A, B = 40, 6
    vqa = _tiny_vqa(A)
    m = SimilarityModel(vqa, knn_size=24, trainable_vqa=False).cuda()
    feats = (torch.randn(B, 25, 64).abs() * 0.45).to(DEV)
    wids = torch.randint(1, 31, (B, 26)).to(DEV)
    aids = torch.randint(0, A, (B,)).to(DEV)
    s = m(feats, wids, aids)
    assert s.shape == (B, 24) and s.dtype == torch.float32 and not s.requires_grad and s.is_cuda
    m.use_hip_vqa = False                                     # the restatement is fed by the torch vqa_forward
    _, z_o, a_k, z_k, _ = m.vqa_forward(feats, wids)
    m.use_hip_vqa = True
    ref, _ = R.similarity_scores(feats.cpu().numpy(), z_o.cpu().numpy(), z_k.cpu().numpy(), a_k.cpu().numpy(), aids.cpu().numpy())
    err = np.abs(s.cpu().numpy() - ref).max()
    print("module vs restatement", err)
    assert err <= TOL_SUM
    m.knn_size = 5                                            # mutable, as eval_model sets it
    s5 = m(feats[:, :6].contiguous(), wids, aids)
    assert s5.shape == (B, 5) and np.abs(s5.cpu().numpy() - ref[:, :5]).max() <= TOL_SUM
    assert all(k.startswith("vqa_model.") for k in m.state_dict())
    with pytest.raises(IndexError):
        m(feats[:, :6].contiguous(), wids, torch.full((B,), A, dtype=torch.long, device=DEV))


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cx_cli_sim_gpu", os.path.join(PKG, "counterexamples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_synthetic_matches_restatement(tmp_path, capsys):
    cli = _cli()
    argv = ["--synthetic", "-cx", "SimilarityModel", "-t", "-b", "64", "--syn_val", "160", "--syn_train", "64",
            "--syn_images", "512", "--project_dir", str(tmp_path)]
    res = cli.main(argv)
    out = capsys.readouterr().out
    assert re.search(r"Epoch 1 test: loss: [0-9.]+, recall: [0-9.]+", out) and "SimilarityModel: 160 triplets" in out
    # the same triplets through the restatement
    from neuralcx.synth import SyntheticCX
    kw = dict(K=24, dv=2048, dq=2400, dz=360, A=2000, n_img=512, device=DEV)          # (load_synthetic with the default YAML)
    train = SyntheticCX(n_triplets=64, seed=1234, **kw)
    val = SyntheticCX(n_triplets=160, seed=4321, feats=train.feats, **kw)
    feats = val.feats.cpu().numpy()
    sc, gt = [], []
    for lo in range(0, 160, 64):
        sel = torch.arange(lo, min(lo + 64, 160), device=DEV)
        b, g = val.batch(sel, first_id=lo)
        sc.append(R.similarity_scores_table(feats, b.img_idx.cpu().numpy(), b.z_orig.cpu().numpy(), b.z_knns.cpu().numpy(),
                                            b.a_knns.cpu().numpy(), b.answer_aids.cpu().numpy())[0])
        gt.append(g.cpu().numpy())
    sc, gt = np.concatenate(sc), np.concatenate(gt)
    ok = _gaps_ok(sc, gt, 1e-4)
    assert ok.mean() > 0.8
    slack = (~ok).sum() / 160.0                              # a triplet with a near tie may rank either way
    for k in (1, 5):
        assert abs(res["recall_%d" % k] - _recall(sc, gt, k).mean()) <= slack + 1e-9, (k, slack)
    m = sc.max(1)
    ce = np.mean(m + np.log(np.exp(sc - m[:, None]).sum(1)) - sc[np.arange(160), gt])          # CrossEntropyLoss on the scores
    assert abs(res["loss"] - ce) < 1e-4
    runs = os.listdir(os.path.join(str(tmp_path), "logs", "cx"))
    with open(os.path.join(str(tmp_path), "logs", "cx", runs[0], "final_results.txt")) as f:
        assert json.load(f)["recall_5"] == res["recall_5"]
