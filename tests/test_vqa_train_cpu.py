"""CPU: the VQA trainer without a GPU -- the fp64 restatement against the reference-produced fixture, the C ABI's argument checks
and struct sizes, the engine's state_dict against models.factory's MutanNoAtt, the module's default route, the CLI's parser,
checkpoint names and its torch path end to end."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import vqa_train_ref as R
from conftest import GOLDEN, PKG, ROOT
from helpers import grad_tol

NEW = ("ncx_vqa_train_workspace_bytes", "ncx_vqa_train_forward", "ncx_ce_loss", "ncx_vqa_train_backward", "ncx_vqa_train_ws_region")
CASES = {"c0": dict(R=10, act_v=True), "c1": dict(R=3, act_v=False)}


def _opt(**fusion_kw):
    fus = dict(dim_v=64, dim_q=48, dim_hv=32, dim_hq=36, dim_mm=24, R=3, activation_v="tanh", activation_q="tanh", dropout_v=0.5, dropout_q=0.5,
               dropout_hv=0, dropout_hq=0)
    fus.update(fusion_kw)
    return dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=16, dropout=0.0, fixed_emb=False), fusion=fus, classif=dict(dropout=0.5))


@pytest.mark.parametrize("case", ["c0", "c1"])
def test_restatement_reproduces_fixture(case):
    g, c = np.load(os.path.join(GOLDEN, "g16_vqa_train.npz")), case + "/"
    names = [str(n) for n in g[c + "names"]]
    Rk, act_v = CASES[case]["R"], CASES[case]["act_v"]
    P = R.state_to_fields({n: g[c + "init/" + n] for n in names}, Rk)
    ref = R.step(P, g[c + "feats"][g[c + "img_idx"]], g[c + "q_emb"], g[c + "target"], act_v=act_v)
    lg = g[c + "logits"]
    assert np.abs(ref["logits"] - lg).max() <= 1e-5 * max(1.0, np.abs(lg).max())
    assert abs(ref["loss"] - float(g[c + "loss"])) <= 1e-5 * max(1.0, abs(float(g[c + "loss"])))
    gsd = R.state_to_fields({n: g[c + "grad/" + n] for n in names}, Rk)
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
    want = R.state_to_fields({n: g[c + "after/" + n] for n in names}, Rk)
    for k in want:
        assert np.abs(after[k] - want[k]).max() <= 2e-6, k
    # the planted rows are what the generator says they are
    assert not g[c + "feats"][3].any() and g[c + "img_idx"][2] == 3 and g[c + "img_idx"][0] == g[c + "img_idx"][1]
    assert g[c + "target"][0] == g[c + "target"][3]


def test_symbols_in_header_exports_and_library():
    from neuralcx import _lib
    src = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "neuralcx.h")).read(), flags=re.S)
    declared = set(re.findall(r"\b(ncx_[a-z_0-9]+)\s*\(", src))
    L = _lib.lib()
    for n in NEW:
        assert n in declared and n in _lib.EXPORTS, n
        getattr(L, n)
    assert "ncx_vqa_train" in open(os.path.join(PKG, "Makefile")).read()


def _dims(**kw):
    from neuralcx import _lib
    d = _lib.NcxVqaTrainDims()
    d.B, d.dv, d.dq, d.dz, d.A, d.n_img = 8, 64, 48, 24, 40, 10
    for k, v in kw.items():
        setattr(d, k, v)
    return d


def _mp(fill=1, **kw):
    from neuralcx import _lib
    m = _lib.NcxMutanParams()
    for n in ("wv", "bv", "wq", "bq", "whv", "bhv", "whq", "bhq", "wc", "bc"):
        setattr(m, n, 4096 * fill or None)          # never dereferenced: every call below is refused before a launch
    m.dhv, m.dhq, m.R, m.act_v, m.act_q = 32, 36, 3, 2, 2
    for k, v in kw.items():
        setattr(m, k, v)
    return m


def test_abi_argument_checks_and_struct_sizes():
    from neuralcx import _lib
    L = _lib.lib()
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    body = re.search(r"typedef struct ncx_vqa_train_dims \{(.*?)\} ncx_vqa_train_dims;", hdr, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    n32 = sum(len(x.split(",")) for x in re.findall(r"(?:int32_t|float)\s+([^;]+);", body))
    n64 = len(re.findall(r"uint64_t\s+\w+;", body))
    assert C.sizeof(_lib.NcxVqaTrainDims) == 4 * n32 + 8 * n64 == 56
    assert C.sizeof(_lib.NcxMutanGrads) == 10 * C.sizeof(C.c_void_p)
    ws_bytes = L.ncx_vqa_train_workspace_bytes
    d, m = _dims(), _mp()
    assert ws_bytes(C.byref(d), C.byref(m)) > 0
    assert ws_bytes(None, C.byref(m)) == 0 and ws_bytes(C.byref(d), None) == 0
    for bad in (dict(B=0), dict(dv=3), dict(dz=0), dict(A=2), dict(n_img=0), dict(dropout_mode=3), dict(p_v=1.0), dict(p_c=-0.1)):
        assert ws_bytes(C.byref(_dims(**bad)), C.byref(m)) == 0, bad
    for bad in (dict(R=0), dict(R=11), dict(dhv=2), dict(act_v=1), dict(act_q=3)):
        assert ws_bytes(C.byref(d), C.byref(_mp(**bad))) == 0, bad
    p = C.c_void_p(4096)
    fwd = lambda d_, m_, feats=p, ws=p, n=1 << 30: L.ncx_vqa_train_forward(C.byref(d_), feats, p, p, C.byref(m_), None, ws, n, p, p, None)
    assert fwd(d, m, feats=None) == -1
    assert fwd(d, _mp(fill=0)) == -1
    assert fwd(_dims(B=0), m) == -2
    assert fwd(_dims(dq=2), m) == -2
    assert fwd(d, _mp(act_v=1)) == -4
    assert fwd(d, m, n=64) == -3                               # short workspace
    assert fwd(d, m, ws=C.c_void_p(4096 + 16)) == -3           # misaligned workspace
    assert fwd(_dims(dropout_mode=2), m) == -1                 # explicit masks wanted, none given
    g = _lib.NcxMutanGrads()
    bwd = lambda g_: L.ncx_vqa_train_backward(C.byref(d), C.byref(m), None, p, 1 << 30, p, C.byref(g_), None, None)
    assert bwd(g) == -1
    for n, _ in g._fields_:
        setattr(g, n, 4096)
    assert L.ncx_vqa_train_backward(C.byref(_dims(want_dq=1)), C.byref(m), None, p, 1 << 30, p, C.byref(g), None, None) == -1
    assert L.ncx_vqa_train_backward(C.byref(d), C.byref(m), None, p, 64, p, C.byref(g), None, None) == -3
    ce = lambda logits, B, A, rows=p: L.ncx_ce_loss(logits, p, B, A, 0.0, p, p, p, p, p, rows, None)
    assert ce(None, 4, 8) == -1 and ce(p, 4, 8, rows=None) == -1 and ce(p, 0, 8) == -2 and ce(p, 4, 0) == -2
    off, nb = C.c_size_t(), C.c_size_t()
    assert L.ncx_vqa_train_ws_region(C.byref(d), C.byref(m), 1, C.byref(off), C.byref(nb)) == 0 and nb.value == 8 * 64 * 4 and off.value % 256 == 0
    assert L.ncx_vqa_train_ws_region(C.byref(d), C.byref(m), 9, C.byref(off), C.byref(nb)) == -4


def test_engine_state_dict_matches_factory_model():
    from neuralcx.vqa_train import VqaTrainEngine
    from vqa import models
    opt = _opt()
    A = 40
    model = models.factory(opt, ["w%d" % i for i in range(20)], ["a%d" % i for i in range(A)], cuda=False)
    e = VqaTrainEngine.from_options(opt, A, device="cpu")
    e.init_parameters(seed=5)
    sd = e.state_dict()
    want = {k: v for k, v in model.state_dict().items() if not k.startswith("seq2vec.")}
    assert set(sd) == set(want)
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
    # list_linear_hv.{i} are row views of ONE stacked block, which is what the frozen producer's weights object holds
    views = e.state_dict(views=True)
    whv = e.params.views["whv"]
    dz = opt["fusion"]["dim_mm"]
    for i in range(opt["fusion"]["R"]):
        v = views["fusion.list_linear_hv.%d.weight" % i]
        assert v.data_ptr() == whv[i * dz].data_ptr() and v.is_contiguous()
    mw = e.mutan_weights()
    assert mw.t["whv"].data_ptr() == whv.data_ptr() and (mw.dhv, mw.dhq, mw.R, mw.dz, mw.A) == (32, 36, 3, 24, 40)
    e2 = VqaTrainEngine.from_options(opt, A, device="cpu")
    e2.init_parameters(seed=5)
    assert torch.equal(e2.params.flat, VqaTrainEngine.from_options(opt, A, device="cpu").params.flat) is False
    e3 = VqaTrainEngine.from_options(opt, A, device="cpu"); e3.init_parameters(seed=5)
    assert torch.equal(e2.params.flat, e3.params.flat)


def test_default_route_and_unsupported_options():
    from neuralcx import vqa_train
    from vqa.models.noatt import MutanNoAtt
    assert MutanNoAtt.use_hip_train is False
    assert vqa_train.route_for(_opt()) == "hip"
    o = _opt(); del o["fusion"]["activation_v"]
    assert vqa_train.route_for(o) == "hip"
    for bad in (dict(activation_hv="tanh"), dict(activation_mm="tanh"), dict(dropout_hv=0.1), dict(activation_q="relu")):
        assert vqa_train.route_for(_opt(**bad)).startswith("torch path"), bad
    o = _opt(); o["classif"]["activation"] = "tanh"
    assert vqa_train.route_for(o).startswith("torch path")
    with pytest.raises(Exception):
        vqa_train.VqaTrainEngine.from_options(o, 40, device="cpu")
    # on the CPU the module never takes the HIP route, whatever the attribute says
    from vqa import models
    m = models.factory(_opt(), ["w%d" % i for i in range(20)], ["a%d" % i for i in range(40)], cuda=False).eval()
    v, w = torch.rand(3, 64), torch.randint(1, 20, (3, 5))
    ref = m(v, w)
    m.use_hip_train = True
    assert torch.equal(m(v, w), ref)


TINY_YAML = """
logs: {dir_logs: %s}
vqa: {nans: 40, maxlength: 8}
coco: {}
model:
  arch: MutanNoAtt
  seq2vec: {arch: gru, emb_size: 16, dropout: 0.0, fixed_emb: False}
  fusion: {dim_v: 64, dim_q: 48, dim_hv: 32, dim_hq: 32, dim_mm: 24, R: 3, activation_v: tanh, activation_q: tanh, dropout_v: 0.1, dropout_q: 0.1, dropout_hv: 0, dropout_hq: 0}
  classif: {dropout: 0.1}
optim: {lr: 0.003, batch_size: 64, epochs: 3}
"""
TINY_ARGS = ["--synthetic", "--syn_examples", "384", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0"]


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("vqa_train_cli", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_parser_and_checkpoint_names():
    cli = _cli()
    a = cli.build_parser().parse_args([])
    assert a.path_opt.endswith(os.path.join("options", "vqa2", "mutan_noatt_train.yaml")) and os.path.isfile(a.path_opt)
    assert (a.synthetic, a.freeze_seq2vec, a.no_hip, a.evaluate, a.resume, a.start_epoch, a.save_model, a.print_freq) == \
        (False, False, False, False, "", 0, True, 10)
    assert (a.syn_examples, a.syn_images, a.syn_vocab) == (8192, 1024, 1000)
    a = cli.build_parser().parse_args(["-lr", "0.01", "-b", "32", "--epochs", "2", "--dir_logs", "x", "--resume", "best", "-e", "--st_dropout", "0.1",
                                       "--st_fixed_emb", "true", "--synthetic", "--freeze_seq2vec", "--no_hip", "--seed", "3", "--save_model", "false",
                                       "--path_trainset", "t", "--path_features", "f", "--start_epoch", "1", "--print_freq", "5"])
    opt = cli.load_options(a)
    assert opt["optim"] == dict(lr=0.01, batch_size=32, epochs=2) and opt["logs"]["dir_logs"] == "x"
    assert opt["model"]["seq2vec"]["dropout"] == 0.1 and opt["model"]["seq2vec"]["fixed_emb"] is True and a.save_model is False
    assert opt["model"]["fusion"]["R"] == 10 and opt["vqa"]["nans"] == 2000          # the YAML's values where no flag overrides
    from neuralcx import vqa_train
    assert vqa_train.route_for(opt["model"]) == "hip"
    p = cli.ckpt_paths("logs/d", "best")
    assert p == {k: os.path.join("logs/d", "best_%s.pth.tar" % k) for k in ("info", "model", "optim")}


def test_cli_torch_path_on_cpu_writes_checkpoints(tmp_path):
    cli = _cli()
    logs = str(tmp_path / "logs")
    y = tmp_path / "tiny.yaml"
    y.write_text(TINY_YAML % logs)
    out = cli.main(["--path_opt", str(y), "--no_hip", "--epochs", "1", "-b", "128"] + TINY_ARGS)
    assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["train"]["loss"])
    for tag in ("ckpt", "best"):
        for part in ("info", "model", "optim"):
            assert os.path.isfile(os.path.join(logs, "%s_%s.pth.tar" % (tag, part))), (tag, part)
    from vqa import models
    opt = cli.load_options(cli.build_parser().parse_args(["--path_opt", str(y)]))
    m = models.factory(opt["model"], ["w%d" % i for i in range(30)], ["a%d" % i for i in range(40)], cuda=False)
    m.load_state_dict(torch.load(os.path.join(logs, "best_model.pth.tar")), strict=True)
