"""CPU: the MLB attention model (MLBAtt) -- the reference fixture against the fp64 restatement and against the module's torch path,
the peakedness condition, the factory, the state_dict, training under autograd, the C ABI's host-side checks and train.py --no_hip.
No compute on a device."""
import ctypes
import importlib.util
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, PKG, ROOT
import mlb_att_ref

CASES = ("c0", "c1")
WORDS = ["w%d" % i for i in range(40)]


def load_case(name):
    g = np.load(os.path.join(GOLDEN, "g21_mlb_att.npz"))
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    c["state"] = {k[len("state/"):]: v for k, v in c.items() if k.startswith("state/")}
    c["acts"] = dict(att_mm=str(c["activation_mm"]) or None, c=str(c["classif_activation"]) or None)
    c["maps"] = c["table"][c["img_idx"]]
    return c


def att_opt(dv, dq, dh_att, G, dh_f, att_mm="tanh", act_c="tanh", **att_over):
    attention = dict(nb_glimpses=G, dim_h=dh_att, dropout_v=0.5, dropout_q=0.5, dropout_mm=0.5, activation_v="tanh", activation_q="tanh")
    if att_mm:
        attention["activation_mm"] = att_mm
    attention.update(att_over)
    classif = dict(dropout=0.5)
    if act_c:
        classif["activation"] = act_c
    return dict(arch="MLBAtt", dim_v=dv, dim_q=dq, seq2vec=dict(arch="gru", emb_size=8, dropout=0.0), attention=attention,
                fusion=dict(dim_h=dh_f, dropout_v=0.5, dropout_q=0.5, activation_v="tanh", activation_q="tanh"), classif=classif)


def build(c):
    import vqa.models as M
    dv, dq, dh_att, G, dh_f, A = (int(x) for x in c["dims"][:6])
    m = M.factory(att_opt(dv, dq, dh_att, G, dh_f, c["acts"]["att_mm"], c["acts"]["c"]), WORDS, ["a%d" % i for i in range(A)], cuda=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items()}, strict=False)
    return m


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_reproduces_the_reference_fixture(name):
    c = load_case(name)
    logits, att, pos = mlb_att_ref.mlb_att_forward(c["state"], c["maps"], c["q_emb"], c["acts"], want_logits=True)
    assert mlb_att_ref.peaked(pos, att), "every parity input must have peaked attention"
    for key, r in (("logits", logits), ("att", att)):
        assert r.shape == c[key].shape, key
        err, mx = float(np.abs(c[key] - r).max()), float(np.abs(r).max())
        print(name, key, "max|reference fp32 - fp64 restatement| = %.3e, max|ref| = %.3e" % (err, mx))
        assert err <= 1e-5 * max(1.0, mx), (key, err, mx)


@pytest.mark.parametrize("name", CASES)
def test_fixture_has_the_planted_rows_and_peaked_attention(name):
    c = load_case(name)
    idx = c["img_idx"]
    assert not c["table"][3].any() and idx[2] == 3                                     # the all-zero image
    assert np.array_equal(c["att"][2], np.full_like(c["att"][2], c["att"][2, 0, 0]))  # ... whose attention is exactly uniform
    assert idx[0] == idx[3] and not np.array_equal(idx, np.arange(len(idx)))          # one image for two questions; not the identity
    xq = np.tanh(c["q_emb"].astype(np.float64) @ c["state"]["linear_q_att.weight"].T.astype(np.float64) + c["state"]["linear_q_att.bias"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5                                        # the saturating question
    W, H = int(c["dims"][7]), int(c["dims"][8])
    assert ((W * H) % 4 != 0 and W != H) == (name == "c0")
    assert (c["acts"]["att_mm"] is None and c["acts"]["c"] is None) == (name == "c1")
    assert c["att"].max() >= 0.3


@pytest.mark.parametrize("name", CASES)
def test_module_torch_path_computes_the_fixture(name):
    """Key names and shapes of the reference model's state_dict (seq2vec.* aside: the fixture's encoder is the oracle's stand-in), and
    the module's torch path on the fixture's inputs, with the tolerance of test_mlb_gpu._check."""
    import vqa.models as M
    c = load_case(name)
    m = build(c)
    assert isinstance(m, M.MLBAtt) and M.MLBAtt.use_hip is True
    own = {k: tuple(v.shape) for k, v in m.state_dict().items() if not k.startswith("seq2vec.")}
    ref = {k: tuple(v.shape) for k, v in c["state"].items()}
    assert own == ref and set(ref) == set(str(k) for k in c["state_keys"])
    dv, dq, dh_att, G, dh_f, A = (int(x) for x in c["dims"][:6])
    want = {"conv_v_att.weight": (dh_att, dv, 1, 1), "linear_q_att.weight": (dh_att, dq), "conv_att.weight": (G, dh_att, 1, 1),
            "linear_q_fusion.weight": (G * dh_f, dq), "linear_classif.weight": (A, G * dh_f), "list_linear_v_fusion.%d.weight" % (G - 1): (dh_f, dv)}
    assert all(ref[k] == v for k, v in want.items())
    assert any(k.startswith("seq2vec.") for k in m.state_dict())
    m.eval()
    with torch.no_grad():
        logits = m.forward_from_q(torch.from_numpy(c["maps"]), torch.from_numpy(c["q_emb"]))
    att = torch.stack(m.list_att, 1).numpy()
    for key, got in (("logits", logits.numpy()), ("att", att)):
        err, mx = float(np.abs(got - c[key]).max()), float(np.abs(c[key]).max())
        assert err <= 1e-4 * max(1.0, mx), (key, err, mx)
    assert len(m.list_att) == G and all(a.shape == (len(c["img_idx"]), att.shape[2]) for a in m.list_att)
    assert np.allclose(att.sum(2), 1.0, atol=1e-5)


def test_factory_registers_mlbatt_and_still_refuses_mutanatt():
    import vqa.models as M
    assert "MLBAtt" in M.model_names and "MutanAtt" not in M.model_names and set(M.model_names) == {"MLBAtt", "MLBNoAtt", "MutanNoAtt"}
    with pytest.raises(ValueError, match="unknown VQA arch"):
        M.factory(dict(att_opt(64, 48, 32, 2, 24), arch="MutanAtt"), WORDS, ["a%d" % i for i in range(20)], cuda=False)


def test_training_mode_backward_reaches_every_parameter():
    import vqa.models as M
    torch.manual_seed(0)
    m = M.factory(att_opt(16, 12, 8, 2, 6), WORDS, ["a%d" % i for i in range(10)], cuda=False)
    m.train()
    v = torch.rand(3, 16, 3, 2)
    wids = torch.tensor([[1, 2, 3, 0], [4, 5, 0, 0], [6, 7, 8, 9]])
    loss = torch.nn.functional.cross_entropy(m(v, wids), torch.tensor([1, 2, 3]))
    loss.backward()
    missing = [n for n, p in m.named_parameters() if p.grad is None or not torch.isfinite(p.grad).all()]
    assert not missing, missing
    assert all(float(p.grad.abs().max()) > 0 for n, p in m.named_parameters() if n.endswith("weight") and not n.startswith("seq2vec.embedding"))
    assert len(m.list_att) == 2 and all(not a.requires_grad and torch.allclose(a.sum(1), torch.ones(3), atol=1e-5) for a in m.list_att)
    # a CPU module never takes the HIP route, in any mode
    m.eval()
    with torch.no_grad():
        assert not m._hip_ok(v, torch.zeros(3, 12))


def test_weights_object_layout():
    import vqa.models as M
    from neuralcx import _lib, ops
    c = load_case("c1")
    m = build(c)
    mw = ops.mlb_att_weights(m)
    dv, dq, dh_att, G, dh_f, A = (int(x) for x in c["dims"][:6])
    assert (mw.dv, mw.dq, mw.dh_att, mw.G, mw.dh_f, mw.A) == (dv, dq, dh_att, G, dh_f, A)
    assert mw.acts == dict(act_v_att=2, act_q_att=2, act_mm=0, act_v=2, act_q=2, act_c=0)
    assert all(t.dtype == torch.float32 and t.is_contiguous() and not t.requires_grad for t in mw.t.values())
    assert torch.equal(mw.t["wg"][1], m.list_linear_v_fusion[1].weight.detach()) and mw.t["wv_att"].shape == (dh_att, dv)
    bad = M.factory(att_opt(64, 48, 32, 2, 24, activation_v="relu"), WORDS, ["a%d" % i for i in range(20)], cuda=False)
    assert ops.mlb_att_acts(bad.opt) is None
    with pytest.raises(_lib.NcxError, match="none, tanh"):
        ops.MlbAttWeights(bad)
    with pytest.raises(_lib.NcxError, match="device tensor"):              # the HIP path has no CPU fallback
        ops.mlb_att_forward(torch.from_numpy(c["maps"]), None, torch.from_numpy(c["q_emb"]), mw)


def test_symbols_declared_exported_and_validated_on_the_host():
    from neuralcx import _lib
    from neuralcx._lib import NcxMlbAttDims, NcxMlbAttParams
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("ncx_mlb_att_workspace_bytes", "ncx_mlb_att_forward"):
        assert n + "(" in hdr and n in _lib.EXPORTS and hasattr(L, n), n
    assert "typedef struct ncx_mlb_att_dims" in hdr and ctypes.sizeof(NcxMlbAttDims) == 9 * 4
    assert "typedef struct ncx_mlb_att_params" in hdr and ctypes.sizeof(NcxMlbAttParams) == 12 * 8 + 6 * 4
    lib = _lib.lib()
    one = ctypes.c_void_p(256)                      # never dereferenced: validation only
    ptrs = {n: one for n, _ in NcxMlbAttParams._fields_[:12]}
    acts = {n: 2 for n, _ in NcxMlbAttParams._fields_[12:]}
    good = dict(B=128, P=196, dv=2048, dq=2400, dh_att=1200, G=4, dh_f=1200, A=2000, n_img=82783)
    m = NcxMlbAttParams(**ptrs, **acts)
    d = NcxMlbAttDims(**good)
    need = lib.ncx_mlb_att_workspace_bytes(ctypes.byref(d), ctypes.byref(m))
    slab = 128 * 19 * 4 * 196 * 4                   # [B, h-tiles, G, P]: the partial position logits; x_att [B, P, dh_att] is never stored
    x_att = 128 * 196 * 1200 * 4
    assert slab < need < x_att // 2 and need % 256 == 0
    for field, val in (("B", 0), ("P", 0), ("G", 0), ("G", 9), ("dv", 3), ("dq", 2), ("dh_att", 0), ("dh_f", 3), ("A", 1), ("n_img", 0),
                       ("P", 1 << 20)):
        bad = NcxMlbAttDims(**dict(good, **{field: val}))
        assert lib.ncx_mlb_att_workspace_bytes(ctypes.byref(bad), ctypes.byref(m)) == 0, (field, val)
    for field, val in (("act_mm", 1), ("act_c", 3), ("wa", None), ("bg", None)):
        bm = NcxMlbAttParams(**ptrs, **acts)
        setattr(bm, field, val)
        assert lib.ncx_mlb_att_workspace_bytes(ctypes.byref(d), ctypes.byref(bm)) == 0, field
    assert lib.ncx_mlb_att_workspace_bytes(None, ctypes.byref(m)) == 0 and lib.ncx_mlb_att_workspace_bytes(ctypes.byref(d), None) == 0
    # P = 1 .. 3 (no 16-byte window in a row of the map) and every G up to 8 are valid shapes
    for over in (dict(P=1), dict(P=3), dict(G=8), dict(G=1)):
        ok = NcxMlbAttDims(**dict(good, **over))
        assert lib.ncx_mlb_att_workspace_bytes(ctypes.byref(ok), ctypes.byref(m)) > 0, over
    # NULLs and dims are rejected before any launch
    null_args = (None, None, None, ctypes.byref(m), None, 0, None, None, None)
    assert lib.ncx_mlb_att_forward(ctypes.byref(d), *null_args) == -1                             # NCX_E_NULL
    assert lib.ncx_mlb_att_forward(None, *null_args) == -1
    assert lib.ncx_mlb_att_forward(ctypes.byref(d), one, one, one, None, one, 1 << 40, one, one, None) == -1
    bad = NcxMlbAttDims(**dict(good, G=9))
    assert lib.ncx_mlb_att_forward(ctypes.byref(bad), one, one, one, ctypes.byref(m), one, 1 << 40, one, one, None) == -2     # NCX_E_DIMS
    m.act_q = 7
    assert lib.ncx_mlb_att_forward(ctypes.byref(d), *null_args) == -4                             # NCX_E_FLAGS
    m.act_q = 2
    # a short or misaligned workspace is refused before any launch
    assert lib.ncx_mlb_att_forward(ctypes.byref(d), one, one, one, ctypes.byref(m), one, need - 1, one, one, None) == -3
    assert lib.ncx_mlb_att_forward(ctypes.byref(d), one, one, one, ctypes.byref(m), ctypes.c_void_p(264), 1 << 40, one, one, None) == -3


def _cli(name):
    spec = importlib.util.spec_from_file_location("cx_cli_mlb_att_" + name.split(".")[0], os.path.join(PKG, name))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


YAML = os.path.join(PKG, "options", "vqa2", "mlb_att_train.yaml")


def test_yaml_carries_the_reference_keys():
    import yaml
    with open(YAML) as f:
        opt = yaml.safe_load(f)
    m = opt["model"]
    assert m["arch"] == "MLBAtt" and (m["dim_v"], m["dim_q"]) == (2048, 2400) and opt["vqa"]["nans"] == 2000
    assert m["attention"]["nb_glimpses"] == 4 and m["attention"]["dim_h"] == 1200 and m["fusion"]["dim_h"] == 1200
    assert all(m["attention"]["activation_" + k] == "tanh" for k in ("v", "q", "mm")) and m["classif"]["activation"] == "tanh"
    assert m["seq2vec"]["arch"] == "gru" and opt["optim"]["batch_size"] == 128


def test_train_cli_no_hip_runs_a_tiny_epoch_on_the_cpu(tmp_path, monkeypatch, capsys):
    import yaml
    with open(YAML) as f:
        opt = yaml.safe_load(f)
    m = opt["model"]
    m["dim_v"], m["dim_q"], m["seq2vec"]["emb_size"] = 16, 12, 8
    m["attention"].update(dim_h=8, nb_glimpses=2)
    m["fusion"]["dim_h"] = 6
    opt["vqa"].update(nans=10, maxlength=5)
    opt["optim"].update(batch_size=8, epochs=1)
    opt["logs"]["dir_logs"] = str(tmp_path / "logs")
    path = tmp_path / "tiny.yaml"
    path.write_text(yaml.safe_dump(opt))
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    cli = _cli("train.py")
    out = cli.main(["--path_opt", str(path), "--synthetic", "--no_hip", "--syn_examples", "32", "--syn_images", "6", "--syn_vocab", "20",
                    "--syn_grid", "3", "--print_freq", "0"])
    text = capsys.readouterr().out
    assert "=> route: torch path: --no_hip" in text
    t = out["trainer"]
    assert t.train.feats.shape == (6, 16, 3, 3) and t.model.use_hip is False
    assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["val"]["loss"]) and np.isfinite(out["history"][0]["train"]["loss"])
    assert os.path.isfile(os.path.join(str(tmp_path / "logs"), "best_model.pth.tar"))
    # --freeze_seq2vec freezes the encoder and keeps q_emb per split; the model still trains under autograd
    frozen = cli.main(["--path_opt", str(path), "--synthetic", "--no_hip", "--freeze_seq2vec", "--syn_examples", "32", "--syn_images", "6",
                       "--syn_vocab", "20", "--syn_grid", "3", "--print_freq", "0"])
    assert all(not p.requires_grad for p in frozen["trainer"].model.seq2vec.parameters()) and frozen["trainer"].engine is None
    assert np.isfinite(frozen["history"][0]["val"]["loss"]) and frozen["trainer"].train.q_emb.shape == (28, 12)
    # real-data attention tables are out of scope: a clear message, not a traceback
    with pytest.raises(SystemExit, match="attention tables"):
        cli.main(["--path_opt", str(path), "--no_hip"])
    # without --no_hip a CPU box is refused as for every other model
    with pytest.raises(SystemExit, match="MI355X"):
        cli.main(["--path_opt", str(path), "--synthetic"])
