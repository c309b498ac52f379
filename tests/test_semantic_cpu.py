"""CPU: the semantic baseline scorer's host surface -- the fp64 restatement against the reference-pinned fixture, the C ABI's
symbols and argument validation, the drop-in module's reference surface, and the CLI's model gate (no GPU compute)."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import semantic_ref as R
from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ("ncx_cosine_gram_workspace_bytes", "ncx_cosine_gram", "ncx_semantic_scores")
REF_LB_ERROR = "If semantic baseline is selected then --sb_lambda must also be provided."       # counterexamples.py:240-242


def _tiny_opt():
    return dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
                fusion=dict(dim_v=64, dim_q=48, dim_hv=16, dim_hq=16, dim_mm=16, R=3, dropout_v=0.5, dropout_q=0.5,
                            activation_v="tanh", activation_q="tanh", dropout_hv=0, dropout_hq=0),
                classif=dict(dropout=0.5))


def test_restatement_reproduces_reference_fixture():
    g = np.load(os.path.join(GOLDEN, "g10_semantic.npz"))
    n = 0
    for c in ("c0", "c1", "c2"):
        G = R.cosine_similarity(g[c + "/emb"])
        for i, lam in enumerate(g[c + "/lams"]):
            sc, raw = R.semantic_scores(g[c + "/a_knns"], g[c + "/aids"], G, float(lam))
            assert np.abs(sc - g[c + "/scores"][i]).max() <= 1e-6, (c, lam)
            assert np.isfinite(raw).all()
            n += 1
    assert n == 6


def test_fixture_covers_the_edge_cases():
    g = np.load(os.path.join(GOLDEN, "g10_semantic.npz"))
    assert {0.0, 1.0} <= set(g["c0/lams"].tolist())
    emb, aids, a = g["c0/emb"], g["c0/aids"], g["c0/a_knns"]
    zero_rows = np.where(~emb.any(1))[0]
    assert len(zero_rows) and np.isin(aids, zero_rows).any()                      # an aid at a zero embedding row
    assert any((emb[i] == emb[j]).all() for i in range(len(emb)) for j in range(i + 1, len(emb)))
    p = np.exp(a - a.max(2, keepdims=True)); p /= p.sum(2, keepdims=True)
    pa = p[np.arange(len(aids)), :, aids]
    assert pa.max() > 0.999 and pa.min() < 1e-8
    assert R.cosine_similarity(emb)[zero_rows[0]].tolist() == [0.0] * len(emb)     # sklearn's rule: the diagonal too


def test_symbols_declared_and_exported():
    from neuralcx import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuralcx.h")).read(), flags=re.S)
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in NEW_SYMBOLS:
        assert re.search(r"\b%s\s*\(" % n, src), n
        assert n in _lib.EXPORTS and hasattr(L, n), n


def test_abi_validation_without_gpu():
    from neuralcx import _lib
    L = _lib.lib()
    buf = ctypes.create_string_buffer(1024)
    x = ctypes.cast(buf, ctypes.c_void_p)                        # non-NULL (never dereferenced: validation comes first)
    # NULL pointers -> -1
    assert L.ncx_semantic_scores(None, x, 4, 24, 2000, x, 0.5, x, None, x, None) == -1
    assert L.ncx_semantic_scores(x, x, 4, 24, 2000, x, 0.5, x, None, None, None) == -1
    assert L.ncx_semantic_scores(x, x, 4, 24, 2000, None, 0.5, x, None, x, None) == -1
    assert L.ncx_cosine_gram(None, 20, 12, x, 1 << 20, x, None) == -1
    assert L.ncx_cosine_gram(x, 20, 12, x, 1 << 20, None, None) == -1
    # bad dimensions -> -2
    for B, K, A in ((0, 24, 2000), (4, 0, 2000), (4, 65, 2000), (4, 24, 0), (4, 24, 4097), (-1, 24, 20)):
        assert L.ncx_semantic_scores(x, x, B, K, A, x, 0.5, x, None, x, None) == -2, (B, K, A)
    for A, da in ((0, 12), (20, 0), (8193, 4), (-3, 4)):
        assert L.ncx_cosine_gram(x, A, da, x, 1 << 20, x, None) == -2, (A, da)
        assert L.ncx_cosine_gram_workspace_bytes(A, da) == 0
    assert L.ncx_cosine_gram_workspace_bytes(2000, 2400) == 2000 * 2400 * 4 + 2000 * 2000 * 8
    assert L.ncx_cosine_gram_workspace_bytes(7, 3) == 256 + 7 * 7 * 8      # (rows padded to 4 columns, 256-byte rounding)
    assert L.ncx_cosine_gram(x, 20, 12, x, 16, x, None) == -3              # workspace too small


def test_module_surface_matches_reference():
    import vqa.models as M
    from vqa.models.cx import CXModelBase, SemanticBaseline
    vqa = M.factory(_tiny_opt(), ["w%d" % i for i in range(10)], ["a%d" % i for i in range(20)], cuda=False, data_parallel=False)
    m = SemanticBaseline(vqa, knn_size=24, trainable_vqa=False)          # cx.py:159-163 (CXModelBase's arguments)
    m2 = SemanticBaseline(vqa_model=vqa, knn_size=24)
    assert isinstance(m, CXModelBase) and m.knn_size == 24 and m2.lam == 0.5 and m.dim_z == 16
    m.knn_size = 2                                                        # mutable, as eval_model sets it (counterexamples.py:458)
    assert m.knn_size == 2
    m.set_lambda(0.3)
    assert m.lam == 0.3
    assert sorted(m.state_dict()) == sorted("vqa_model." + k for k in vqa.state_dict())     # checkpoints interchange
    assert m.emb_pairs.shape == (2000, 2000) and not m.emb_pairs.any()                       # cx.py:168
    m.set_answer_embedding(np.ones((20, 6), np.float32))
    m.set_answer_embedding(torch.ones(20, 6))
    assert sorted(m.state_dict()) == sorted("vqa_model." + k for k in vqa.state_dict())
    assert np.allclose(m.softmax([1.0, 2.0, 3.0]), R.softmax([1.0, 2.0, 3.0]))
    assert np.isfinite(m.softmax([100.0, 0.0])).all()


def test_module_forward_has_no_cpu_fallback():
    import vqa.models as M
    from neuralcx import _lib
    from vqa.models.cx import SemanticBaseline
    vqa = M.factory(_tiny_opt(), ["w%d" % i for i in range(10)], ["a%d" % i for i in range(20)], cuda=False, data_parallel=False)
    m = SemanticBaseline(vqa, knn_size=24)
    with pytest.raises(_lib.NcxError):
        m(torch.rand(2, 25, 64), torch.ones(2, 5, dtype=torch.long), torch.zeros(2, dtype=torch.long))


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cx_cli_sem", os.path.join(PKG, "counterexamples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_requires_lambda():
    cli = _cli()
    with pytest.raises(ValueError, match=re.escape(REF_LB_ERROR)):
        cli.main(["-cx", "SemanticBaseline", "--synthetic"])


def test_cli_gets_past_the_model_gate(monkeypatch):
    cli = _cli()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    with pytest.raises(SystemExit, match="an MI355X is required"):
        cli.main(["-cx", "SemanticBaseline", "-lb", "0.5", "--synthetic"])


def test_cli_synthetic_embedding_is_seeded():
    cli = _cli()
    a, b = cli.synthetic_answer_embedding(30), cli.synthetic_answer_embedding(30)
    assert a.shape == (30, 2400) and a.dtype == np.float32 and (a == b).all()
