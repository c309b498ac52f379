"""CPU: the MLB no-attention producer (MLBNoAtt behind the cx drop-in surface) -- fixture vs the fp64 restatement, the factory,
the width helper, refusals, the C ABI and the CLI gates.  No compute on a device."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT
from mlb_ref import mlb_vqa_forward

CASES = ("c0", "c1")
OUTS = ("a_orig", "z_orig", "a_knns", "z_knns")


def load_case(name):
    g = np.load(os.path.join(GOLDEN, "g14_mlb.npz"))
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    c["state"] = {k[len("state/"):]: v for k, v in c.items() if k.startswith("state/")}
    c["act_c"] = str(c["classif_activation"]) or None
    return c


def mlb_opt(dv, dq, dh, act_c="tanh", **fusion_over):
    fusion = dict(dim_v=dv, dim_q=dq, dim_h=dh, dropout_v=0.5, dropout_q=0.5, activation_v="tanh", activation_q="tanh")
    fusion.update(fusion_over)
    classif = dict(dropout=0.5)
    if act_c:
        classif["activation"] = act_c
    return dict(arch="MLBNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0), fusion=fusion, classif=classif)


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_reproduces_the_reference_fixture(name):
    """... and the reference's own fp32 outputs lie inside the GPU tolerance (1e-4 max|ref|, tests/test_mlb_gpu.py) measured
    against the restatement: the tolerance is one the reference alone meets."""
    c = load_case(name)
    ref = mlb_vqa_forward(c["state"], c["feats"], c["img_idx"], c["q_emb"], act_c=c["act_c"])
    for r, key in zip(ref, OUTS):
        assert r.shape == c[key].shape, key
        err, mx = float(np.abs(c[key] - r).max()), float(np.abs(r).max())
        print(name, key, "max|reference fp32 - fp64 restatement| = %.3e, max|ref| = %.3e" % (err, mx))
        assert err <= 1e-4 * mx, (key, err, mx)


@pytest.mark.parametrize("name", CASES)
def test_fixture_has_the_planted_rows(name):
    c = load_case(name)
    idx, st = c["img_idx"], c["state"]
    assert not c["feats"][3].any() and idx[0, 3] == 3 and idx[2, 0] == 3          # the all-zero feature row, as candidate and as original
    assert idx[0, 10] == idx[0, 5]                                                # the same image twice in one list
    assert np.array_equal(c["z_knns"][0, 9], c["z_knns"][0, 4]) and np.array_equal(c["a_knns"][0, 9], c["a_knns"][0, 4])
    xq = np.tanh(c["q_emb"].astype(np.float64) @ st["fusion.linear_q.weight"].T.astype(np.float64) + st["fusion.linear_q.bias"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5                                   # the saturating question
    dh = int(c["dims"][2])
    assert (dh % 32 != 0) == (name == "c1") and (c["act_c"] is None) == (name == "c1")


@pytest.mark.parametrize("name", CASES)
def test_factory_builds_mlbnoatt_with_the_reference_keys_and_shapes(name):
    """Key names and shapes of the reference model's state_dict, seq2vec.* aside: the fixture's encoder is the oracle's stand-in for the
    un-vendored skipthoughts package, an input producer with its own parameter names."""
    import vqa.models as M
    c = load_case(name)
    dv, dq, dh, A, B, K = (int(x) for x in c["dims"])
    assert "MLBNoAtt" in M.model_names and "MutanNoAtt" in M.model_names
    vqa = M.factory(mlb_opt(dv, dq, dh, c["act_c"]), ["w%d" % i for i in range(40)], ["a%d" % i for i in range(A)], cuda=False)
    assert isinstance(vqa, M.MLBNoAtt) and isinstance(vqa.fusion, M.MLBFusion) and not isinstance(vqa, M.MutanNoAtt)
    own = {k: tuple(v.shape) for k, v in vqa.state_dict().items() if not k.startswith("seq2vec.")}
    ref = {k: tuple(v.shape) for k, v in c["state"].items() if not k.startswith("seq2vec.")}
    assert own == ref and set(ref) == {"fusion.linear_v.weight", "fusion.linear_v.bias", "fusion.linear_q.weight", "fusion.linear_q.bias",
                                       "linear_classif.weight", "linear_classif.bias"}
    assert any(k.startswith("seq2vec.") for k in vqa.state_dict()) and any(k.startswith("seq2vec.") for k in c["state_keys"])
    # the module's torch path computes the fixture (the yardstick of the GPU tests)
    vqa.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items() if not k.startswith("seq2vec.")}, strict=False)
    vqa.eval()
    v = torch.from_numpy(c["feats"][c["img_idx"].reshape(-1)])
    q = torch.from_numpy(c["q_emb"]).repeat_interleave(K + 1, 0)
    with torch.no_grad():
        z = vqa._fusion(v, q)
        a = vqa._classif(z)
    assert float((z.view(B, K + 1, -1)[:, 1:] - torch.from_numpy(c["z_knns"])).abs().max()) <= 1e-5
    assert float((a.view(B, K + 1, -1)[:, 1:] - torch.from_numpy(c["a_knns"])).abs().max()) <= 1e-4


def test_width_helper():
    from vqa.models.fusion import out_dim
    assert out_dim(dict(dim_mm=360, dim_h=99)) == 360 and out_dim(dict(dim_h=1200)) == 1200
    with pytest.raises(KeyError):
        out_dim(dict(dim_v=2048))
    import yaml
    with open(os.path.join(PKG, "options", "cx", "neuralcx_256_1_all_mlb.yaml")) as f:
        opt = yaml.safe_load(f)
    assert opt["model"]["arch"] == "MLBNoAtt" and out_dim(opt["model"]["fusion"]) == 1200 and opt["model"]["classif"]["activation"] == "tanh"
    assert "dim_mm" not in opt["model"]["fusion"]


def test_scorers_take_their_z_width_from_an_mlb_model():
    import vqa.models as M
    from vqa.models.cx import LinearContext, NeuralModel
    vqa = M.factory(mlb_opt(64, 48, 28), ["w%d" % i for i in range(10)], ["a%d" % i for i in range(20)], cuda=False)
    spec = dict(v_emb=True, v_mult=True, v_dist=True, v_rank=True, q_emb=True, a_emb=True, z_emb=True)
    m = NeuralModel(model_spec=spec, dim_h=16, n_layers=1, emb=None, drop_p=0.25, vqa_model=vqa, knn_size=24, trainable_vqa=False)
    assert m.dim_z == 28 and m.linear_1.weight.shape[1] == 3 * 64 + 1 + 24 + 48 + 2 * 28 + 2 * 2400
    assert LinearContext(vqa, 24).dim_z == 28


def test_weights_object_and_refusals():
    import vqa.models as M
    from neuralcx import _lib, ops
    words, answers = ["w%d" % i for i in range(10)], ["a%d" % i for i in range(20)]
    vqa = M.factory(mlb_opt(64, 48, 28), words, answers, cuda=False)
    mw = ops.vqa_weights(vqa)
    assert isinstance(mw, ops.MlbWeights) and (mw.dz, mw.A, mw.act_v, mw.act_q, mw.act_c) == (28, 20, 2, 2, 2)
    assert all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in mw.t.values())
    assert ops.MlbWeights(M.factory(mlb_opt(64, 48, 28, act_c=None), words, answers, cuda=False)).act_c == 0
    for bad in (dict(activation_v="relu"), dict(activation_q="sigmoid")):
        with pytest.raises(_lib.NcxError, match="none, tanh"):
            ops.MlbWeights(M.factory(mlb_opt(64, 48, 28, **bad), words, answers, cuda=False))
    with pytest.raises(_lib.NcxError, match="classif.activation"):
        ops.MlbWeights(M.factory(mlb_opt(64, 48, 28, act_c="relu"), words, answers, cuda=False))
    no_v = mlb_opt(64, 48, 28)
    del no_v["fusion"]["dim_v"]
    with pytest.raises(_lib.NcxError, match="dim_v"):
        ops.MlbWeights(M.factory(no_v, words, answers, cuda=False))
    # MutanWeights is unchanged: it still refuses classif.activation, and the dispatcher still picks it for a MUTAN model
    mopt = dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
                fusion=dict(dim_v=64, dim_q=48, dim_hv=16, dim_hq=16, dim_mm=16, R=2, dropout_v=0.5, dropout_q=0.5, activation_v="tanh",
                            activation_q="tanh", dropout_hv=0, dropout_hq=0), classif=dict(dropout=0.5))
    mut = M.factory(mopt, words, answers, cuda=False)
    assert isinstance(ops.vqa_weights(mut), ops.MutanWeights)
    mut.opt["classif"]["activation"] = "tanh"
    with pytest.raises(_lib.NcxError, match="classif.activation is not supported"):
        ops.MutanWeights(mut)
    # the ops refuse CPU tensors (the HIP path has no CPU fallback)
    with pytest.raises(_lib.NcxError, match="device tensor"):
        ops.vqa_forward(torch.zeros(50, 64), torch.zeros(2, 25, dtype=torch.int32), torch.zeros(2, 48), mw)


def test_symbols_declared_exported_and_validated_on_the_host():
    from neuralcx import _lib
    from neuralcx._lib import NcxDims, NcxMlbParams
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("ncx_mlb_workspace_bytes", "ncx_mlb_forward"):
        assert n + "(" in hdr and n in _lib.EXPORTS and hasattr(L, n), n
    assert "typedef struct ncx_mlb_params" in hdr and ctypes.sizeof(NcxMlbParams) == 6 * 8 + 4 * 4
    lib = _lib.lib()
    d = NcxDims(B=512, K=24, dv=2048, dq=2400, dz=1200, da=4, A=2000, H=4, L=1, n_img=82783)
    one = ctypes.c_void_p(256)                      # never dereferenced: validation only
    m = NcxMlbParams(wv=one, bv=one, wq=one, bq=one, wc=one, bc=one, dh=1200, act_v=2, act_q=2, act_c=2)
    need = lib.ncx_mlb_workspace_bytes(ctypes.byref(d), ctypes.byref(m))
    t_bytes = 512 * 24 * 1200 * 4
    assert t_bytes < need < 4 * t_bytes             # x_q, t = tanh(z) of the B K + B rows, padded classifier weights; no dense x_v
    m.act_c = 0
    assert 0 < lib.ncx_mlb_workspace_bytes(ctypes.byref(d), ctypes.byref(m)) < t_bytes         # no t without classif.activation
    for field, val in (("act_c", 1), ("act_v", 3), ("dh", 360), ("wq", None)):
        bad = NcxMlbParams(wv=one, bv=one, wq=one, bq=one, wc=one, bc=one, dh=1200, act_v=2, act_q=2, act_c=2)
        setattr(bad, field, val)
        assert lib.ncx_mlb_workspace_bytes(ctypes.byref(d), ctypes.byref(bad)) == 0, field
    args = (None, None, None, ctypes.byref(m), None, 0, None, None, None, None, None)
    assert lib.ncx_mlb_forward(ctypes.byref(d), *args) == -1                                    # NCX_E_NULL before any launch
    m.act_c = 7
    assert lib.ncx_mlb_forward(ctypes.byref(d), *args) == -4                                    # NCX_E_FLAGS


def _cli(name):
    spec = importlib.util.spec_from_file_location("cx_cli_mlb_" + name.split(".")[0], os.path.join(PKG, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


@pytest.mark.parametrize("script,extra", [("counterexamples.py", []), ("counterexamples.py", ["-cx", "LinearContext"]),
                                          ("counterexamples.py", ["-cx", "BlackBox"]), ("contrastive.py", [])])
def test_cli_with_the_mlb_yaml_gets_past_every_gate(monkeypatch, script, extra):
    cli = _cli(script)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    with pytest.raises(SystemExit, match="an MI355X is required"):
        cli.main(["--synthetic", "--path_opt", os.path.join(PKG, "options", "cx", "neuralcx_256_1_all_mlb.yaml")] + extra)
