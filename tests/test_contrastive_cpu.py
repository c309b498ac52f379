"""CPU: the contrastive path (ContrastiveModel + ContrastiveLoss, the reference's contrastive.py) -- the fp64 restatement against
the reference-produced fixture, the C ABI's symbols and argument validation, the drop-in module's reference surface, the CLI's
flags and resume rule, and the host-side properties of the triple sampler's contract."""
import ctypes
import os
import re

import numpy as np
import pytest
import torch

import contrastive_ref as R
import scorers_ref
from conftest import GOLDEN, PKG, ROOT

NEW_SYMBOLS = ("ncx_contrastive_workspace_bytes", "ncx_contrastive_forward", "ncx_contrastive_distances", "ncx_contrastive_loss",
               "ncx_contrastive_backward")


def _g(name="g12_contrastive.npz"):
    return np.load(os.path.join(GOLDEN, name))


def _state(g):
    return {str(n): g["init/" + str(n)] for n in g["init/names"]}


def test_fixture_holds_the_conditions_it_was_drawn_for():
    g = _g()
    p = _state(g)
    assert np.abs(R.pre(g["t/feats"], g["t/z_orig"], g["t/z_knns"], p)[0]).min() > 2e-5
    assert np.abs(R.pre(g["e/feats"], g["e/z_orig"], g["e/z_knns"], p)[0]).min() > 2e-5
    d = g["t/dist_comp"]
    assert np.abs(d - 2.0).min() > 1e-3 and (d < 2).sum() >= len(d) // 4 and (d > 2).sum() >= len(d) // 4
    assert not g["t/h"][0].any() and g["t/h"][1:].any(axis=(1, 2)).all()          # example 0: three all-zero rows
    assert abs(float(g["t/dist_comp"][0]) - 1e-6 * np.sqrt(300)) < 1e-9
    s = np.sort(g["e/dist"], 1)[:, ::-1]
    assert (s[:, 0] - s[:, 1]).min() > 1e-3 and (s[:, 4] - s[:, 5]).min() > 1e-3
    for name in ("g12_contrastive.npz", "g12_contrastive_adam.npz"):
        assert os.path.getsize(os.path.join(GOLDEN, name)) < 1 << 20


def test_restatement_reproduces_reference_training_step():
    g = _g()
    r = R.loss_and_grads(g["t/feats"], g["t/z_orig"], g["t/z_knns"], _state(g))
    assert np.abs(r["h"] - g["t/h"]).max() < 1e-5
    assert abs(r["loss_comp"] - g["t/loss_comp"]) < 1e-5 and abs(r["loss_other"] - g["t/loss_other"]) < 1e-5 * max(1, g["t/loss_other"])
    assert np.abs(r["dist"][:, 0] - g["t/dist_comp"]).max() < 1e-5 and np.abs(r["dist"][:, 1] - g["t/dist_other"]).max() < 1e-4
    for n, v in r["grads"].items():
        ref = g["t/grad/" + n]
        assert np.abs(v - ref).max() <= 1e-4 * np.abs(ref).max(), n
    assert not r["dpre"][0].any()                                                  # the all-zero example passes no gradient


def test_restatement_reproduces_reference_evaluation():
    g = _g()
    h = R.forward(g["e/feats"], g["e/z_orig"], g["e/z_knns"], _state(g))
    assert np.abs(h - g["e/h"]).max() < 1e-5
    d = R.distances(h)
    assert d.shape == (8, 24) and np.abs(d - g["e/dist"]).max() < 1e-4
    assert ((R.rank_farthest(d, g["e/comp"]) < 5).astype(np.int32) == g["e/recall5"]).all()


def test_restatement_adam_reproduces_reference_first_step():
    g, ga = _g(), _g("g12_contrastive_adam.npz")
    p0 = {n: v for n, v in _state(g).items() if n != "answer_embedding.weight"}
    p1 = scorers_ref.adam(p0, [{n: g["t/grad/" + n] for n in p0}], lr=1e-3)
    for n in p0:
        assert np.abs(p1[n] - ga["t/step1/" + n]).max() < 2e-6, n
    for step in ("step1", "step3"):                                                 # never trained (cx.py:440-441, 458)
        assert np.array_equal(ga["t/%s/answer_embedding.weight" % step], g["init/answer_embedding.weight"])


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
    good = dict(B=4, P=3, dv=8, dz=8, n_img=100)
    d = _lib.NcxContrastiveDims(**good)
    ins = _lib.NcxInputs(*([x] * 10))
    by = ctypes.byref
    assert L.ncx_contrastive_workspace_bytes(by(d)) > 0
    assert ctypes.sizeof(_lib.NcxContrastiveDims) == 20
    big = 1 << 30
    # NULL pointers -> -1
    assert L.ncx_contrastive_forward(None, by(ins), x, x, x, big, x, x, None) == -1
    assert L.ncx_contrastive_forward(by(d), by(ins), None, x, x, big, x, x, None) == -1
    assert L.ncx_contrastive_forward(by(d), by(ins), x, x, x, big, x, None, None) == -1
    assert L.ncx_contrastive_forward(by(d), by(_lib.NcxInputs(x, None, *([x] * 8))), x, x, x, big, x, x, None) == -1
    assert L.ncx_contrastive_distances(by(d), None, None, 0, x, None) == -1
    assert L.ncx_contrastive_distances(by(d), x, x, big, None, None) == -1
    assert L.ncx_contrastive_loss(by(d), x, big, 2.0, 0.25, None, x, None) == -1
    assert L.ncx_contrastive_backward(by(d), by(ins), x, big, None, None, x, None) == -1
    # bad dimensions -> -2 (and a zero workspace size); the loss is the P = 3 step only
    for kw in (dict(B=0), dict(P=1), dict(P=66), dict(dv=3), dict(dz=3), dict(n_img=0), dict(B=-1)):
        bad = _lib.NcxContrastiveDims(**dict(good, **kw))
        assert L.ncx_contrastive_workspace_bytes(by(bad)) == 0, kw
        assert L.ncx_contrastive_forward(by(bad), by(ins), x, x, x, big, x, x, None) == -2, kw
        assert L.ncx_contrastive_distances(by(bad), None, x, big, x, None) == -2, kw
        assert L.ncx_contrastive_backward(by(bad), by(ins), x, big, None, x, x, None) == -2, kw
    assert L.ncx_contrastive_loss(by(_lib.NcxContrastiveDims(**dict(good, P=25))), x, big, 2.0, 0.25, x, x, None) == -2
    assert L.ncx_contrastive_workspace_bytes(by(_lib.NcxContrastiveDims(**dict(good, P=65)))) > 0
    # a short workspace -> -3
    assert L.ncx_contrastive_forward(by(d), by(ins), x, x, x, 16, x, x, None) == -3
    assert L.ncx_contrastive_loss(by(d), x, 16, 2.0, 0.25, x, x, None) == -3


class _StubVQA(torch.nn.Module):
    def __init__(self, dv, dq, dz, A):
        super().__init__()
        self.opt = {"fusion": {"dim_v": dv, "dim_q": dq, "dim_mm": dz}}
        self.vocab_answers = ["a%d" % i for i in range(A)]
        self.lin = torch.nn.Linear(2, 2)                 # a parameter: the state_dict carries vqa_model.*


def test_module_state_dict_matches_reference():
    from vqa.models.cx import CXModelBase, ContrastiveModel
    g = _g()
    m = ContrastiveModel(_StubVQA(12, 4, 8, 6), knn_size=2, trainable_vqa=False)
    ref = {str(n): g["init/" + str(n)].shape for n in g["init/names"]}
    own = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("vqa_model.")}
    assert own == ref and isinstance(m, CXModelBase)
    assert [n for n, _ in m.named_parameters() if not n.startswith("vqa_model.")] == [str(n) for n in g["init/names"]]
    assert sorted(k for k in m.state_dict() if k.startswith("vqa_model.")) == ["vqa_model.lin.bias", "vqa_model.lin.weight"]
    assert (m.dim_h, m.dim_a, m.knn_size) == (300, 300, 2)
    m.knn_size = 24                                               # mutable, as contrastive.py:270, 287 use it
    with pytest.raises(NotImplementedError):
        ContrastiveModel(_StubVQA(12, 4, 8, 6), knn_size=2, trainable_vqa=True)


def test_module_forward_has_no_cpu_fallback():
    from neuralcx import _lib
    from vqa.models.cx import ContrastiveModel
    m = ContrastiveModel(_StubVQA(12, 4, 8, 6), 2)
    m.vqa_forward = lambda image_features, wids: (None, torch.zeros(2, 8), None, torch.zeros(2, 2, 8), None)
    with pytest.raises(_lib.NcxError, match="no CPU fallback"):
        m(torch.zeros(2, 3, 12), torch.zeros(2, 3, dtype=torch.long), torch.zeros(2, dtype=torch.long))


def test_engine_state_layout_and_single_gpu_rule():
    from neuralcx import ops
    from neuralcx.contrastive import ContrastiveEngine
    shapes = ops.contrastive_shapes(2048, 360, 2000)
    assert shapes == {"linear.weight": (300, 2408), "linear.bias": (300,), "answer_embedding.weight": (2000, 300)}
    assert set(ops.CONTRASTIVE_STATE_TO_FIELD) == {"linear.weight", "linear.bias"}
    with pytest.raises(NotImplementedError, match="one GPU"):
        ContrastiveEngine(world_size=2)


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("contrastive_cli", os.path.join(PKG, "contrastive.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_accepts_the_reference_flags(monkeypatch):
    cli = _cli()
    a = cli.build_parser().parse_args(["--path_opt", "x.yaml", "-lr", "1e-3", "-b", "64", "--epochs", "3", "--resume", "run", "--best",
                                       "-c", "note", "-p", "10", "-v", "50", "--pairwise", "--pretrained_vqa", "-dev"])
    assert (a.learning_rate, a.batch_size, a.epochs, a.resume, a.best, a.comment, a.print_freq, a.eval_freq) == \
        (1e-3, 64, 3, "run", True, "note", 10, 50)
    assert a.pairwise and a.pretrained_vqa and a.dev_mode and not a.trainable_vqa
    d = cli.build_parser().parse_args([])
    assert d.pairwise and d.resume == "" and d.print_freq == 100 and d.eval_freq == -1          # contrastive.py:49-60
    assert os.path.samefile(d.path_opt, os.path.join(PKG, "options", "cx", "neuralcx_256_1_all.yaml"))
    assert cli.build_parser().parse_args(["--untrained_vqa"]).pretrained_vqa is False
    with pytest.raises(SystemExit):
        cli.build_parser().parse_args(["--pretrained_vqa", "--untrained_vqa"])
    with pytest.raises(SystemExit, match="trainable_vqa"):
        cli.main(["--synthetic", "--trainable_vqa"])
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    with pytest.raises(SystemExit, match="an MI355X is required"):
        cli.main(["--synthetic"])
    monkeypatch.setenv("WORLD_SIZE", "2")
    with pytest.raises(SystemExit, match="one GPU"):
        cli.main(["--synthetic"])


def test_resume_accepts_both_recall_keys():
    cli = _cli()
    assert cli.last_recall([{"contrastive/recall": 0.1}, {"contrastive/recall": 0.25}]) == 0.25
    assert cli.last_recall([{"recall": 0.5}]) == 0.5                                  # the key contrastive.py:396 reads
    with pytest.raises(KeyError):
        cli.last_recall([{"loss": 1.0}])


def test_counterexamples_cli_keeps_its_refusals():
    import importlib.util
    spec = importlib.util.spec_from_file_location("cx_cli_for_contrastive", os.path.join(PKG, "counterexamples.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    with pytest.raises(SystemExit, match="--pairwise"):
        mod.main(["-cx", "PairwiseModel", "--synthetic"])
    with pytest.raises(SystemExit):
        mod.main(["-cx", "ContrastiveModel", "--synthetic"])


def test_sampler_contract_on_the_host():
    """sample_positions: `other` never the counterexample's position, always in 0..K-1, every allowed position occurs, same seed
    same draws; triple_img_idx / triple_z pick [orig, comp, other] and the two neighbours' z (from a batch block or a split cache)."""
    from neuralcx.contrastive import sample_positions, triple_img_idx, triple_z
    K, B = 24, 24 * 1024
    gen = torch.Generator().manual_seed(7)
    gt = torch.arange(B, dtype=torch.int32) % K
    pos = sample_positions(gt, K, gen)
    assert pos.shape == (B, 2) and pos.dtype == torch.int64
    assert torch.equal(pos[:, 0], gt.long()) and (pos[:, 1] != pos[:, 0]).all() and pos[:, 1].min() >= 0 and pos[:, 1].max() <= K - 1
    for c in range(K):
        seen = set(pos[gt == c, 1].tolist())
        assert seen == set(range(K)) - {c}, c                       # 1024 draws per c: P(any position missed) <= 24 . 23 . (22/23)^1024 ~ 1e-17
    again = sample_positions(gt, K, torch.Generator().manual_seed(7))
    assert torch.equal(pos, again) and not torch.equal(pos, sample_positions(gt, K, gen))
    assert torch.equal(sample_positions(torch.tensor([0, 1]), 2, gen), torch.tensor([[0, 1], [1, 0]]))     # K = 2: no choice
    with pytest.raises(ValueError):
        sample_positions(gt, 1, gen)
    img = torch.arange(B * (K + 1), dtype=torch.int32).view(B, K + 1)
    i3 = triple_img_idx(img, pos)
    assert i3.dtype == torch.int32 and torch.equal(i3[:, 0], img[:, 0])
    assert torch.equal(i3[:, 1].long(), img[:, 0].long() + 1 + pos[:, 0]) and torch.equal(i3[:, 2].long(), img[:, 0].long() + 1 + pos[:, 1])
    z = torch.randn(B, K, 5)
    z3 = triple_z(z, pos)
    assert torch.equal(z3[:, 0], z[torch.arange(B), pos[:, 0]]) and torch.equal(z3[:, 1], z[torch.arange(B), pos[:, 1]])
    sel = torch.randperm(B)[:100]
    assert torch.equal(triple_z(z, pos[:100], sel), torch.stack([z[sel, pos[:100, 0]], z[sel, pos[:100, 1]]], 1))
