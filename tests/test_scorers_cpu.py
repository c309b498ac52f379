"""CPU: the trainable scorers LinearContext and PairwiseLinearModel -- the fp64 restatement against the reference-produced
fixture, the C ABI's symbols and argument validation, the drop-in modules' reference surface and the CLI's model gate."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import scorers_ref as R
from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ("ncx_pairlin_workspace_bytes", "ncx_pairlin_forward", "ncx_pairlin_backward",
               "ncx_linctx_workspace_bytes", "ncx_linctx_forward", "ncx_linctx_backward")


def _g(name="g11_scorers.npz"):
    return np.load(os.path.join(GOLDEN, name))


def _state(g, prefix, tag="init/"):
    return {str(n): g[prefix + tag + str(n)] for n in g[prefix + "init/names"]}


def _close(a, b, rel=1e-4):
    a, b = np.asarray(a, np.float64), np.asarray(b, np.float64)
    tol = rel * max(np.abs(b).max(), 1e-30)
    assert np.abs(a - b).max() <= tol, (np.abs(a - b).max(), tol)


def test_restatement_reproduces_reference_linear_context():
    g = _g()
    s, loss, grads = R.linctx(g["lc/z_knns"], _state(g, "lc/"), g["lc/gt"])
    assert np.abs(s - g["lc/scores"]).max() < 1e-5 and abs(loss - g["lc/loss"]) < 1e-5
    for n, v in grads.items():
        _close(v, g["lc/grad/" + n])


def test_restatement_reproduces_reference_pairwise_linear():
    g = _g()
    p = _state(g, "pl/")
    s, loss, grads, pre_h, pre_s = R.pairlin(g["pl/feats"], g["pl/q_emb"], g["pl/z_orig"], g["pl/z_knns"], g["pl/aids"], p, g["pl/gt"])
    assert np.abs(s - g["pl/scores"]).max() < 1e-5 and abs(loss - g["pl/loss"]) < 1e-5
    assert (s[0] == 0).all() and (g["pl/scores"][0] == 0).all()                  # the whole-zero triplet
    for n, v in grads.items():
        _close(v, g["pl/grad/" + n])
    gE = g["pl/grad/answer_embedding.weight"]
    assert np.abs(gE[2]).max() > 0 and not gE[[1, 3, 4, 6, 8, 9]].any()            # duplicated id 2 summed, untouched rows 0


def test_restatement_adam_reproduces_reference_first_step():
    g, ga = _g(), _g("g11_scorers_adam.npz")
    for prefix in ("lc/", "pl/"):
        p0 = _state(g, prefix)
        grads = {n: g[prefix + "grad/" + n] for n in p0}
        p1 = R.adam(p0, [grads], lr=1e-3)
        for n in p0:
            assert np.abs(p1[n] - ga[prefix + "step1/" + n]).max() < 2e-6, n


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
    d = _lib.NcxScorerDims(B=4, K=24, dv=8, dq=8, dz=8, A=10, n_img=100)
    ins = _lib.NcxInputs(*([x] * 10))
    pp = _lib.NcxPairlinParams(*([x] * 5))
    gg = _lib.NcxPairlinGrads(*([x] * 5))
    by = ctypes.byref
    assert L.ncx_pairlin_workspace_bytes(by(d)) > 0 and L.ncx_linctx_workspace_bytes(by(d)) > 0
    # NULL pointers -> -1
    assert L.ncx_pairlin_forward(None, by(ins), by(pp), x, 1 << 30, x, x, None) == -1
    assert L.ncx_pairlin_forward(by(d), by(ins), by(pp), x, 1 << 30, None, x, None) == -1
    assert L.ncx_pairlin_forward(by(d), by(ins), by(pp), x, 1 << 30, x, None, None) == -1
    assert L.ncx_pairlin_forward(by(d), by(_lib.NcxInputs(x, None, *([x] * 8))), by(pp), x, 1 << 30, x, x, None) == -1
    assert L.ncx_pairlin_forward(by(d), by(ins), by(_lib.NcxPairlinParams(x, None, x, x, x)), x, 1 << 30, x, x, None) == -1
    assert L.ncx_pairlin_backward(by(d), by(ins), by(pp), x, 1 << 30, None, by(gg), None) == -1
    assert L.ncx_pairlin_backward(by(d), by(ins), by(pp), x, 1 << 30, x, by(_lib.NcxPairlinGrads(x, x, x, None, x)), None) == -1
    assert L.ncx_linctx_forward(by(d), None, x, x, x, 1 << 30, x, None) == -1
    assert L.ncx_linctx_forward(by(d), x, x, None, x, 1 << 30, x, None) == -1
    assert L.ncx_linctx_backward(by(d), x, x, x, 1 << 30, None, x, None) == -1
    # bad dimensions -> -2 (and a zero workspace size)
    for kw in (dict(B=0), dict(K=0), dict(K=65), dict(dv=3), dict(dq=2), dict(dz=3), dict(A=0), dict(n_img=0), dict(B=-1)):
        bad = _lib.NcxScorerDims(**dict(dict(B=4, K=24, dv=8, dq=8, dz=8, A=10, n_img=100), **kw))
        assert L.ncx_pairlin_workspace_bytes(by(bad)) == 0, kw
        assert L.ncx_pairlin_forward(by(bad), by(ins), by(pp), x, 1 << 30, x, x, None) == -2, kw
        assert L.ncx_pairlin_backward(by(bad), by(ins), by(pp), x, 1 << 30, x, by(gg), None) == -2, kw
    for kw in (dict(B=0), dict(K=0), dict(K=65), dict(K=1, dz=3), dict(dz=0)):
        bad = _lib.NcxScorerDims(**dict(dict(B=4, K=24, dv=8, dq=8, dz=8, A=10, n_img=100), **kw))
        assert L.ncx_linctx_workspace_bytes(by(bad)) == 0, kw
        assert L.ncx_linctx_forward(by(bad), x, x, x, x, 1 << 30, x, None) == -2, kw
        assert L.ncx_linctx_backward(by(bad), x, x, x, 1 << 30, x, x, None) == -2, kw
    # a short or misaligned workspace -> -3
    assert L.ncx_linctx_forward(by(d), x, x, x, x, 16, x, None) == -3
    assert L.ncx_pairlin_forward(by(d), by(ins), by(pp), x, 16, x, x, None) == -3


class _StubVQA(torch.nn.Module):
    def __init__(self, dv, dq, dz, A):
        super().__init__()
        self.opt = {"fusion": {"dim_v": dv, "dim_q": dq, "dim_mm": dz}}
        self.vocab_answers = ["a%d" % i for i in range(A)]
        self.lin = torch.nn.Linear(2, 2)                 # a parameter: the state_dict carries vqa_model.*


def test_module_state_dict_matches_reference():
    from vqa.models.cx import CXModelBase, LinearContext, PairwiseLinearModel
    g = _g()
    m = LinearContext(_StubVQA(4, 4, 8, 3), knn_size=24, trainable_vqa=False)
    ref = {str(n): g["lc/init/" + str(n)].shape for n in g["lc/init/names"]}
    own = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("vqa_model.")}
    assert own == ref and isinstance(m, CXModelBase)
    assert sorted(k for k in m.state_dict() if k.startswith("vqa_model.")) == ["vqa_model.lin.bias", "vqa_model.lin.weight"]
    m = PairwiseLinearModel(_StubVQA(4, 4, 4, 10), 24)
    ref = {str(n): g["pl/init/" + str(n)].shape for n in g["pl/init/names"]}
    own = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("vqa_model.")}
    assert own == ref
    assert [n for n, _ in m.named_parameters() if not n.startswith("vqa_model.")] == [str(n) for n in g["pl/init/names"]]
    with pytest.raises(NotImplementedError):
        LinearContext(_StubVQA(4, 4, 8, 3), knn_size=24, trainable_vqa=True)
    with pytest.raises(NotImplementedError):
        PairwiseLinearModel(_StubVQA(4, 4, 4, 10), knn_size=24, trainable_vqa=True)


def test_module_forward_has_no_cpu_fallback():
    from neuralcx import _lib
    from vqa.models.cx import LinearContext, PairwiseLinearModel
    for m in (LinearContext(_StubVQA(4, 4, 8, 3), 24), PairwiseLinearModel(_StubVQA(4, 4, 4, 10), 24)):
        with pytest.raises(_lib.NcxError, match="no CPU fallback"):
            m(torch.zeros(2, 25, 4), torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, dtype=torch.long))


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cx_cli_scorers", os.path.join(PKG, "counterexamples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("model", ["LinearContext", "PairwiseLinearModel"])
def test_cli_gets_past_the_model_gate(monkeypatch, model):
    cli = _cli()
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    with pytest.raises(SystemExit, match="an MI355X is required"):
        cli.main(["-cx", model, "--synthetic"])
    for flag in ("--bf16", "--x6"):
        with pytest.raises(SystemExit, match="NeuralModel"):
            cli.main(["-cx", model, "--synthetic", flag])


def test_cli_still_refuses_pairwise_model():
    cli = _cli()
    with pytest.raises(SystemExit, match="--pairwise"):
        cli.main(["-cx", "PairwiseModel", "--synthetic"])
    with pytest.raises(SystemExit, match="PairwiseModel"):
        cli.main(["-cx", "NeuralModel", "--synthetic", "--pairwise"])
