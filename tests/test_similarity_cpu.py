"""CPU: the similarity scorer's host surface -- the fp64 restatement against the reference-pinned fixture, the completeness of
the drop-in's exports against the reference's import line, the refusals, the C ABI's symbol and argument validation, and the
CLI's model gate (no GPU compute)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import similarity_ref as R
from conftest import GOLDEN, PKG, ROOT

# the reference's `from vqa.models.cx import ...` (counterexamples.py:30-32), as a literal
REFERENCE_IMPORT_LINE = ("RandomBaseline", "DistanceBaseline", "BlackBox", "LinearContext", "PairwiseModel", "PairwiseLinearModel",
                         "SemanticBaseline", "SimilarityModel", "NeuralModel")
TOL_SUM = 1e-4         # the project's logit tolerance: the sum and the cross-entropy term
TOL_COS = 1e-5         # values bounded by 1 (as tests/test_semantic_gpu.py)


def _tiny_opt():
    return dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
                fusion=dict(dim_v=64, dim_q=48, dim_hv=16, dim_hq=16, dim_mm=16, R=3, dropout_v=0.5, dropout_q=0.5,
                            activation_v="tanh", activation_q="tanh", dropout_hv=0, dropout_hq=0),
                classif=dict(dropout=0.5))


def _tiny_vqa():
    import vqa.models as M
    return M.factory(_tiny_opt(), ["w%d" % i for i in range(10)], ["a%d" % i for i in range(20)], cuda=False, data_parallel=False)


def test_restatement_reproduces_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "g13_similarity.npz"))
    for c in ("c0", "c1", "c2"):
        sc, parts = R.similarity_scores(g[c + "/v"], g[c + "/z_orig"], g[c + "/z_knns"], g[c + "/a_knns"], g[c + "/aids"])
        err = np.abs(parts - g[c + "/parts"]).reshape(-1, 3).max(0)
        print(c, "sum", np.abs(sc - g[c + "/scores"]).max(), "v_cos | z_cos | xent", err)
        assert np.abs(sc - g[c + "/scores"]).max() <= TOL_SUM, c
        assert err[0] <= TOL_COS and err[1] <= TOL_COS and err[2] <= TOL_SUM, (c, err)


def test_fixture_covers_the_cases():
    g = np.load(os.path.join(GOLDEN, "g13_similarity.npz"))
    v, zo, a, aids, parts = g["c0/v"], g["c0/z_orig"], g["c0/a_knns"], g["c0/aids"], g["c0/parts"]
    zero_v = np.argwhere(~v[:, 1:].any(2))
    assert len(zero_v) and all(parts[b, k, 0] == 0 for b, k in zero_v)            # an all-zero candidate row: cos = 0
    zero_z = np.where(~zo.any(1))[0]
    assert len(zero_z) and not parts[zero_z, :, 1].any()                           # an all-zero z_orig
    same = np.argwhere((v[:, 1:] == v[:, :1]).all(2))
    assert len(same) and all(abs(parts[b, k, 0] - 1) < 1e-6 and abs(parts[b, k, 1] - 1) < 1e-6 for b, k in same)
    rest = np.stack([np.delete(a[b], aids[b], axis=1) for b in range(len(aids))])
    margin = a[np.arange(len(aids)), :, aids] - rest.max(2), rest.min(2) - a[np.arange(len(aids)), :, aids]
    assert margin[0].max() >= 29.99 and margin[1].max() >= 29.99                         # a[aid] 30 above / 30 below the rest
    # the clamp rule: a candidate of norm < eps against an original of norm ~100 scores |v| / eps, not 1
    n = np.sqrt((v[0].astype(np.float64) ** 2).sum(1))
    assert n[0] > 99 and n[6] < 1e-8 and abs(parts[0, 5, 0] - n[6] / 1e-8) < 1e-6 and parts[0, 5, 0] < 0.02
    assert g["c1/v"].shape[2] == 37 and g["c1/z_orig"].shape[1] == 5 and g["c1/a_knns"].shape[2] == 37
    assert g["c2/v"].shape == (2, 25, 2048) and g["c2/z_knns"].shape == (2, 24, 360) and g["c2/a_knns"].shape == (2, 24, 2000)
    assert os.path.getsize(os.path.join(GOLDEN, "g13_similarity.npz")) < 1000000


def test_every_reference_import_resolves():
    import vqa.models.cx as cx
    missing = [n for n in REFERENCE_IMPORT_LINE if not isinstance(getattr(cx, n, None), type)]
    assert not missing, missing


def test_refusals():
    from vqa.models.cx import CXModelBase, PairwiseModel, SimilarityModel
    vqa = _tiny_vqa()
    with pytest.raises(NotImplementedError, match="--pairwise"):
        PairwiseModel(vqa, knn_size=2, trainable_vqa=False)
    with pytest.raises(NotImplementedError, match="trainable_vqa=True is not supported by the HIP path"):
        SimilarityModel(vqa, knn_size=24, trainable_vqa=True)
    assert issubclass(PairwiseModel, CXModelBase)


def test_module_surface_matches_reference():
    from vqa.models.cx import CXModelBase, SimilarityModel
    vqa = _tiny_vqa()
    m = SimilarityModel(vqa, 24, False)                                    # cx.py:490-494 (CXModelBase's arguments)
    m2 = SimilarityModel(vqa_model=vqa, knn_size=24)
    assert isinstance(m, CXModelBase) and m.knn_size == 24 and m.dim_z == 16 == m2.dim_z
    m.knn_size = 2                                                          # mutable, as eval_model sets it
    assert m.knn_size == 2
    assert sorted(m.state_dict()) == sorted("vqa_model." + k for k in vqa.state_dict())
    assert not [p for n, p in m.named_parameters() if not n.startswith("vqa_model.")]


def test_module_forward_has_no_cpu_fallback():
    from neuralcx import _lib
    from vqa.models.cx import SimilarityModel
    m = SimilarityModel(_tiny_vqa(), knn_size=24)
    with pytest.raises(_lib.NcxError, match="no CPU fallback"):
        m(torch.rand(2, 25, 64), torch.ones(2, 5, dtype=torch.long), torch.zeros(2, dtype=torch.long))


def test_ops_refuse_cpu_tensors():
    from neuralcx import _lib, ops
    with pytest.raises(_lib.NcxError):
        ops.similarity_scores(torch.rand(30, 8), torch.zeros(2, 4, dtype=torch.int32), torch.rand(2, 5), torch.rand(2, 3, 5),
                              torch.rand(2, 3, 7), torch.zeros(2, dtype=torch.int32), bad_flag=torch.zeros(1, dtype=torch.int32))
    with pytest.raises(ValueError):                                         # img_idx must be [B, K + 1]
        ops.similarity_scores(torch.rand(30, 8), torch.zeros(2, 3, dtype=torch.int32), torch.rand(2, 5), torch.rand(2, 3, 5),
                              torch.rand(2, 3, 7), torch.zeros(2, dtype=torch.int32))


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cx_cli_sim", os.path.join(PKG, "counterexamples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_gets_past_the_model_gate(monkeypatch):
    cli = _cli()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    with pytest.raises(SystemExit, match="an MI355X is required"):
        cli.main(["-cx", "SimilarityModel", "--synthetic"])
    assert "SimilarityModel" in cli.SCORERS and "SimilarityModel" in cli.build_parser().format_help()
    with pytest.raises(SystemExit, match="PairwiseModel needs --pairwise"):        # that gate stays
        cli.main(["-cx", "PairwiseModel", "--synthetic"])


def test_symbol_declared_and_exported():
    from neuralcx import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuralcx.h")).read(), flags=re.S)
    assert re.search(r"\bncx_similarity_scores\s*\(", src)
    assert "ncx_similarity_scores" in _lib.EXPORTS
    if os.path.exists(_lib.LIB_PATH):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "ncx_similarity_scores")


def test_abi_validation_without_gpu():
    from neuralcx import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1024)
    x = ctypes.cast(buf, ctypes.c_void_p)                        # non-NULL (never dereferenced: validation comes first)

    def call(feats=x, idx=x, n_img=100, dv=2048, zo=x, zk=x, dz=360, a=x, aid=x, A=2000, B=4, K=24, sc=x, parts=None, flag=x):
        return L.ncx_similarity_scores(feats, idx, n_img, dv, zo, zk, dz, a, aid, A, B, K, sc, parts, flag, None)

    for name in ("feats", "idx", "zo", "zk", "a", "aid", "sc", "flag"):
        assert call(**{name: None}) == -1, name                  # NCX_E_NULL (parts alone is nullable)
    for kw in (dict(K=0), dict(K=65), dict(A=0), dict(A=4097), dict(dv=0), dict(dz=0), dict(B=0), dict(B=-1), dict(n_img=0)):
        assert call(**kw) == -2, kw                              # NCX_E_DIMS
