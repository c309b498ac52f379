"""CPU: the MLBNoAtt trainer without a GPU -- the fp64 restatement against the reference-produced fixture, the C ABI's symbols and
argument checks, the option routes, the engine's state_dict against models.factory's MLBNoAtt, the module's default route and the
CLI's torch path end to end on an MLB YAML."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import mlb_train_ref as R
from conftest import GOLDEN, PKG, ROOT
from helpers import grad_tol

NEW = ("ncx_mlb_train_workspace_bytes", "ncx_mlb_train_forward", "ncx_mlb_train_backward", "ncx_mlb_train_ws_region")
CASES = {"c0": dict(act_v=True, act_c=True), "c1": dict(act_v=False, act_c=False)}


def _opt(classif_act="tanh", **fusion_kw):
    fus = dict(dim_v=64, dim_q=48, dim_h=24, activation_v="tanh", activation_q="tanh", dropout_v=0.5, dropout_q=0.5)
    fus.update(fusion_kw)
    classif = dict(dropout=0.5)
    if classif_act is not None:
        classif["activation"] = classif_act
    return dict(arch="MLBNoAtt", seq2vec=dict(arch="gru", emb_size=16, dropout=0.0, fixed_emb=False), fusion=fus, classif=classif)


@pytest.mark.parametrize("case", ["c0", "c1"])
def test_restatement_reproduces_fixture(case):
    g, c = np.load(os.path.join(GOLDEN, "g17_mlb_train.npz")), case + "/"
    names = [str(n) for n in g[c + "names"]]
    assert sorted(names) == sorted(R.STATE_KEYS.values())
    P = R.state_to_fields({n: g[c + "init/" + n] for n in names})
    ref = R.step(P, g[c + "feats"][g[c + "img_idx"]], g[c + "q_emb"], g[c + "target"], **CASES[case])
    lg = g[c + "logits"]
    assert np.abs(ref["logits"] - lg).max() <= 1e-4 * max(1.0, np.abs(lg).max())
    assert abs(ref["loss"] - float(g[c + "loss"])) <= 1e-5 * max(1.0, abs(float(g[c + "loss"])))
    gsd = R.state_to_fields({n: g[c + "grad/" + n] for n in names})
    for k, want in gsd.items():
        assert np.abs(ref["grads"][k] - want).max() <= grad_tol(k, want), k
    assert np.abs(ref["dq"] - g[c + "grad_q_emb"]).max() <= grad_tol("dq_emb", g[c + "grad_q_emb"])
    B = lg.shape[0]
    if R.rank_safe(lg.astype(np.float64), g[c + "target"]).all():
        assert abs(100.0 * (ref["rank"] < 1).sum() / B - float(g[c + "acc1"])) < 1e-3
        assert abs(100.0 * (ref["rank"] < 5).sum() / B - float(g[c + "acc5"])) < 1e-3
    P64 = {k: v.astype(np.float64) for k, v in P.items()}
    zeros = lambda: {k: np.zeros_like(v) for k, v in P64.items()}
    after = R.adam(P64, ref["grads"], zeros(), zeros(), 1, lr=1e-4)
    want = R.state_to_fields({n: g[c + "after/" + n] for n in names})
    for k in want:
        assert np.abs(after[k] - want[k]).max() <= 2e-6, k
    # the planted rows are what the generator says they are
    assert not g[c + "feats"][3].any() and g[c + "img_idx"][2] == 3 and g[c + "img_idx"][0] == g[c + "img_idx"][1]
    assert g[c + "target"][0] == g[c + "target"][3]
    xq = np.tanh(g[c + "q_emb"].astype(np.float64) @ P["wq"].astype(np.float64).T + P["bq"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5                  # question 1 saturates linear_q
    assert os.path.getsize(os.path.join(GOLDEN, "g17_mlb_train.npz")) < os.path.getsize(os.path.join(GOLDEN, "g16_vqa_train.npz"))


def test_symbols_in_header_exports_and_library():
    from neuralcx import _lib, ops
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuralcx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ncx_[a-z_0-9]+)\s*\(", src))
    L = _lib.lib()
    for n in NEW:
        assert n in declared and n in _lib.EXPORTS, n
        getattr(L, n)
    assert "ncx_mlb_grads" in src and C.sizeof(ops.MlbGrads) == 6 * C.sizeof(C.c_void_p)
    assert "ncx_mlb_train" in open(os.path.join(PKG, "Makefile")).read()
    for n in ("mlb_train_workspace", "mlb_train_forward", "mlb_train_backward", "mlb_train_ws_region"):
        assert callable(getattr(ops, n)), n


def _dims(**kw):
    from neuralcx import _lib
    d = _lib.NcxVqaTrainDims()
    d.B, d.dv, d.dq, d.dz, d.A, d.n_img = 8, 64, 48, 24, 40, 10
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _mp(fill=1, **kw):
    from neuralcx import _lib
    m = _lib.NcxMlbParams()
    for n in ("wv", "bv", "wq", "bq", "wc", "bc"):
        setattr(m, n, 4096 * fill or None)          # never dereferenced: every call below is refused before a launch
    m.dh, m.act_v, m.act_q, m.act_c = 24, 2, 2, 2
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_abi_argument_checks():
    from neuralcx import _lib
    L = _lib.lib()
    ws_bytes = L.ncx_mlb_train_workspace_bytes
    d, m = _dims(), _mp()
    assert ws_bytes(C.byref(d), C.byref(m)) > 0
    assert ws_bytes(C.byref(d), C.byref(_mp(act_v=0, act_q=0, act_c=0))) > 0
    assert ws_bytes(None, C.byref(m)) == 0 and ws_bytes(C.byref(d), None) == 0
    for bad in (dict(B=0), dict(dv=3), dict(dq=2), dict(dz=0), dict(A=2), dict(n_img=0), dict(dropout_mode=3), dict(p_v=1.0), dict(p_c=-0.1),
                dict(dz=28)):                                    # the last: dz != dh
        assert ws_bytes(C.byref(_dims(**bad)), C.byref(m)) == 0, bad
    for bad in (dict(dh=20), dict(act_v=1), dict(act_q=3), dict(act_c=1)):
        assert ws_bytes(C.byref(d), C.byref(_mp(**bad))) == 0, bad
    p = C.c_void_p(4096)
    fwd = lambda d_, m_, feats=p, ws=p, n=1 << 30: L.ncx_mlb_train_forward(C.byref(d_), feats, p, p, C.byref(m_), None, ws, n, p, p, None)
    assert fwd(d, m, feats=None) == -1
    assert fwd(d, _mp(fill=0)) == -1
    assert fwd(_dims(B=0), m) == -2
    assert fwd(_dims(dz=28), m) == -2                          # dz != dh
    assert fwd(d, _mp(dh=28)) == -2
    assert fwd(d, _mp(act_v=1)) == -4 and fwd(d, _mp(act_c=1)) == -4
    assert fwd(d, m, n=64) == -3                               # short workspace
    assert fwd(d, m, ws=C.c_void_p(4096 + 16)) == -3           # misaligned workspace
    assert fwd(_dims(dropout_mode=2), m) == -1                 # explicit masks wanted, none given
    g = _lib.NcxMlbGrads()
    bwd = lambda g_, d_=d, n=1 << 30: L.ncx_mlb_train_backward(C.byref(d_), C.byref(m), None, p, n, p, C.byref(g_), None, None)
    assert bwd(g) == -1
    for n, _ in g._fields_:
        setattr(g, n, 4096)
    assert bwd(g, _dims(want_dq=1)) == -1                      # dq_emb wanted, none given
    assert bwd(g, n=64) == -3
    assert bwd(g, _dims(dz=28)) == -2
    assert L.ncx_mlb_train_backward(C.byref(d), C.byref(_mp(act_q=1)), None, p, 1 << 30, p, C.byref(g), None, None) == -4
    off, nb = C.c_size_t(), C.c_size_t()
    reg = lambda which, d_=d: L.ncx_mlb_train_ws_region(C.byref(d_), C.byref(m), which, C.byref(off), C.byref(nb))
    assert reg(1) == 0 and nb.value == 8 * 64 * 4 and off.value % 256 == 0
    assert reg(2) == 0 and nb.value == 8 * 48 * 4 and off.value % 256 == 0
    assert reg(3) == 0 and nb.value == 8 * 24 * 4 and off.value % 256 == 0
    assert reg(9) == -4 and reg(1, _dims(dz=28)) == -2


def test_routes():
    from neuralcx import vqa_train
    assert vqa_train.mlb_route_for(_opt()) == "hip"
    assert vqa_train.mlb_route_for(_opt(classif_act=None)) == "hip"
    o = _opt(); del o["fusion"]["activation_v"]
    assert vqa_train.mlb_route_for(o) == "hip"
    for bad in (dict(activation_v="relu"), dict(activation_q="sigmoid")):
        assert vqa_train.mlb_route_for(_opt(**bad)).startswith("torch path"), bad
    assert vqa_train.mlb_route_for(_opt(classif_act="relu")).startswith("torch path")
    for k in ("dim_v", "dim_q", "dim_h"):
        o = _opt(); del o["fusion"][k]
        assert vqa_train.mlb_route_for(o) == "torch path: fusion.%s is missing" % k
    with pytest.raises(Exception):
        vqa_train.MlbTrainEngine.from_options(_opt(classif_act="relu"), 40, device="cpu")
    # the Mutan route is what it was
    mutan = dict(arch="MutanNoAtt", fusion=dict(dim_v=64, dim_q=48, dim_hv=32, dim_hq=36, dim_mm=24, R=3, activation_v="tanh", activation_q="tanh",
                                                dropout_v=0.5, dropout_q=0.5, dropout_hv=0, dropout_hq=0), classif=dict(dropout=0.5))
    assert vqa_train.route_for(mutan) == "hip"
    assert vqa_train.route_for(_opt(classif_act=None)) == "torch path: fusion.dim_hv is missing"


def test_module_default_route():
    from vqa import models
    from vqa.models.noatt import MLBNoAtt
    assert MLBNoAtt.use_hip_train is False
    # on the CPU the module never takes the HIP route, whatever the attribute says
    m = models.factory(_opt(), ["w%d" % i for i in range(20)], ["a%d" % i for i in range(40)], cuda=False).eval()
    assert type(m) is MLBNoAtt
    v, w = torch.rand(3, 64), torch.randint(1, 20, (3, 5))
    ref = m(v, w)
    m.use_hip_train = True
    assert torch.equal(m(v, w), ref)
    del m.use_hip_train
    assert m.use_hip_train is False


def test_engine_state_dict_matches_factory_model():
    from neuralcx import ops
    from neuralcx.vqa_train import MlbTrainEngine
    from vqa import models
    opt = _opt()
    A = 40
    model = models.factory(opt, ["w%d" % i for i in range(20)], ["a%d" % i for i in range(A)], cuda=False)
    e = MlbTrainEngine.from_options(opt, A, device="cpu")
    e.init_parameters(seed=5)
    sd = e.state_dict()
    want = {k: v for k, v in model.state_dict().items() if not k.startswith("seq2vec.")}
    assert set(sd) == set(want) == set(R.STATE_KEYS.values())
    for k, v in want.items():
        assert tuple(sd[k].shape) == tuple(v.shape), k
        bound = 1.0 / np.sqrt(v.shape[1] if v.dim() == 2 else want[k.replace("bias", "weight")].shape[1])
        assert sd[k].abs().max() <= bound and sd[k].abs().max() > 0.5 * bound, k            # nn.Linear's U(+-1/sqrt(fan_in))
    e.load_state_dict(model.state_dict())                       # with seq2vec.*: carried through
    full = e.state_dict()
    assert set(full) == set(model.state_dict())
    model2 = models.factory(opt, ["w%d" % i for i in range(20)], ["a%d" % i for i in range(A)], cuda=False)
    model2.load_state_dict(full, strict=True)
    for k, v in model.state_dict().items():
        assert torch.equal(model2.state_dict()[k], v), k
    with pytest.raises(KeyError):
        e.load_state_dict({"fusion.linear_v.weight": sd["fusion.linear_v.weight"]})
    with pytest.raises(KeyError):
        e.load_state_dict(dict(full, **{"fusion.list_linear_hv.0.weight": torch.zeros(2, 2)}))
    # the frozen producer's weights object holds the SAME buffers
    mw = e.mlb_weights()
    assert isinstance(mw, ops.MlbWeights) and (mw.dz, mw.A, mw.act_v, mw.act_q, mw.act_c) == (24, 40, 2, 2, 2)
    for k in ops.MLB_FIELDS:
        assert mw.t[k].data_ptr() == e.params.views[k].data_ptr(), k
    assert MlbTrainEngine.from_options(_opt(classif_act=None), A, device="cpu").mlb_weights().act_c == 0
    st = e.optimizer_state()
    assert st["numel"] == e.params.numel and st["step"] == 0
    e.load_optimizer_state(st)
    with pytest.raises(ValueError):
        e.load_optimizer_state(dict(st, numel=3))


TINY_YAML = """
logs: {dir_logs: %s}
vqa: {nans: 40, maxlength: 8}
coco: {}
model:
  arch: MLBNoAtt
  seq2vec: {arch: gru, emb_size: 16, dropout: 0.0, fixed_emb: False}
  fusion: {dim_v: 64, dim_q: 48, dim_h: 24, activation_v: tanh, activation_q: tanh, dropout_v: 0.1, dropout_q: 0.1}
  classif: {activation: tanh, dropout: 0.1}
optim: {lr: 0.003, batch_size: 64, epochs: 3}
"""
TINY_ARGS = ["--synthetic", "--syn_examples", "384", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0"]


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("vqa_train_cli", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_shipped_yaml_is_the_supported_model():
    from neuralcx import vqa_train
    cli = _cli()
    path = os.path.join(PKG, "options", "vqa2", "mlb_noatt_train.yaml")
    opt = cli.load_options(cli.build_parser().parse_args(["--path_opt", path]))
    m = opt["model"]
    assert m["arch"] == "MLBNoAtt" and vqa_train.mlb_route_for(m) == "hip"
    assert (m["fusion"]["dim_v"], m["fusion"]["dim_q"], m["fusion"]["dim_h"], opt["vqa"]["nans"]) == (2048, 2400, 1200, 2000)
    assert vqa_train.mlb_acts(m) == (2, 2, 2) and vqa_train.dropouts(m) == (0.5, 0.5, 0.5)
    assert opt["optim"]["lr"] == 1e-4 and opt["optim"]["batch_size"] == 512


def test_cli_torch_path_on_cpu_writes_checkpoints(tmp_path):
    cli = _cli()
    logs = str(tmp_path / "logs")
    y = tmp_path / "tiny.yaml"
    y.write_text(TINY_YAML % logs)
    out = cli.main(["--path_opt", str(y), "--no_hip", "--epochs", "1", "-b", "128"] + TINY_ARGS)
    assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["train"]["loss"])
    assert type(out["trainer"].model).__name__ == "MLBNoAtt" and out["trainer"].engine is None
    for tag in ("ckpt", "best"):
        for part in ("info", "model", "optim"):
            assert os.path.isfile(os.path.join(logs, "%s_%s.pth.tar" % (tag, part))), (tag, part)
    from vqa import models
    opt = cli.load_options(cli.build_parser().parse_args(["--path_opt", str(y)]))
    m = models.factory(opt["model"], ["w%d" % i for i in range(30)], ["a%d" % i for i in range(40)], cuda=False)
    m.load_state_dict(torch.load(os.path.join(logs, "best_model.pth.tar")), strict=True)
