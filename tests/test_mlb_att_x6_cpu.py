"""No GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the MLB attention model's conv_v_att kernel from the C ABI up to train.py --x6:
the host-only form query, flag validation before any launch, the unchanged workspace, the binding's three-valued x6 argument, the
module attribute and the command line."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT
from test_mlb_att_cpu import WORDS, YAML, _cli, att_opt

SHAPE = dict(B=3, dv=100, dq=48, dh_att=130, G=4, dh_f=20, A=40, P=196, n_img=3)
FORMS = {0: "small", 1: "fp32_64", 2: "fp32_208", 3: "x6_64", 4: "x6_208"}


def _params():
    from neuralcx._lib import NcxMlbAttParams
    one = ctypes.c_void_p(256)                      # never dereferenced: validation only
    return NcxMlbAttParams(**{n: one for n, _ in NcxMlbAttParams._fields_[:12]}, **{n: 2 for n, _ in NcxMlbAttParams._fields_[12:]})


def _dims(**over):
    from neuralcx._lib import NcxMlbAttDims
    return NcxMlbAttDims(**dict(SHAPE, **over))


def _weights(dv=100, dq=48, dh_att=130, G=4, dh_f=20, A=40):
    import vqa.models as M
    from neuralcx import ops
    m = M.factory(att_opt(dv, dq, dh_att, G, dh_f), WORDS, ["a%d" % i for i in range(A)], cuda=False)
    return ops.mlb_att_weights(m), m


def test_logits_form_through_the_c_call():
    from neuralcx import _lib
    lib = _lib.lib()
    form = lambda flags, **over: lib.ncx_mlb_att_logits_form(ctypes.byref(_dims(**over)), flags)
    assert FORMS[form(0)] == "fp32_208" and FORMS[form(_lib.NCX_F_X6)] == "x6_208"
    assert FORMS[form(0, P=135)] == "fp32_64" and FORMS[form(_lib.NCX_F_X6, P=135)] == "x6_64"
    for P in (1, 3):                                # no 16-byte window in a row of the map: the small kernel under both flags
        assert FORMS[form(0, P=P)] == "small" and FORMS[form(_lib.NCX_F_X6, P=P)] == "small"
    assert FORMS[form(_lib.NCX_F_X6, P=4)] == "x6_64"
    for over in (dict(G=9), dict(dv=3)):
        assert form(0, **over) < 0 and form(_lib.NCX_F_X6, **over) < 0, over
    assert form(_lib.NCX_F_BF16) < 0 and form(0x100) < 0 and lib.ncx_mlb_att_logits_form(None, 0) < 0


def test_workspace_is_what_it_was():
    """att_layout restated: five 256-byte aligned regions, then the GEMM engine's slab.  The X6 form writes one slab slot per 64-column
    group into the same [B][ceil(dh_att / 64)][G][P] region, so the flag needs no byte more."""
    from neuralcx import _lib
    lib = _lib.lib()
    s = SHAPE
    up = lambda n: (n + 255) // 256 * 256
    HT, GF = -(-s["dh_att"] // 64), s["G"] * s["dh_f"]
    regions = up(s["B"] * s["dh_att"] * 4) + up(s["B"] * HT * s["G"] * s["P"] * 4) + up(s["B"] * s["G"] * s["dv"] * 4) + 2 * up(s["B"] * GF * 4)
    need = lib.ncx_mlb_att_workspace_bytes(ctypes.byref(_dims()), ctypes.byref(_params()))
    engine_slab = need - regions                    # the largest split-k slab of the four engine launches: none splits at this size
    assert regions == 1792 + 28416 + 4864 + 2 * 1024 and need % 256 == 0
    assert engine_slab == 0, (need, regions)


def test_flags_are_checked_before_any_launch():
    from neuralcx import _lib
    lib = _lib.lib()
    d, m = _dims(), _params()
    null_args = (None, None, None, ctypes.byref(m))
    for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
        assert lib.ncx_mlb_att_forward_flags(ctypes.byref(d), *null_args, flags, None, 0, None, None, None) == -2, flags       # NCX_E_DIMS
    for flags in (0, _lib.NCX_F_X6):                # an accepted flag: the NULL pointers are what is refused
        assert lib.ncx_mlb_att_forward_flags(ctypes.byref(d), *null_args, flags, None, 0, None, None, None) == -1, flags
    t = _lib.NcxMlbAttTrain()
    for flags, rc in ((_lib.NCX_F_BF16, -2), (0x100, -2), (0, -1), (_lib.NCX_F_X6, -1)):
        got = lib.ncx_mlb_att_train_forward_flags(ctypes.byref(d), ctypes.byref(t), None, None, None, ctypes.byref(m), None, flags, None, 0,
                                                  None, None, None)
        assert got == rc, (flags, got)
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    for n in ("ncx_mlb_att_forward_flags", "ncx_mlb_att_train_forward_flags", "ncx_mlb_att_logits_form"):
        assert n + "(" in hdr and n in _lib.EXPORTS, n


def test_binding_reads_the_process_flag_at_call_time(monkeypatch):
    from neuralcx import _lib, ops
    mw, m = _weights()
    form = lambda P, **k: ops.mlb_att_logits_form(mw, 3, P, 3, **k)
    monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    assert form(196) == "fp32_208" and form(196, x6=None) == "fp32_208" and form(196, x6=True) == "x6_208" and form(135, x6=True) == "x6_64"
    monkeypatch.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6)
    assert form(196, x6=None) == "x6_208" and form(135) == "x6_64"
    assert form(196, x6=False) == "fp32_208"        # an explicit choice wins over the process-wide one
    assert form(1) == "small" and form(3, x6=True) == "small"
    assert ops.mlb_att_flags(None) == _lib.NCX_F_X6 and ops.mlb_att_flags(False) == 0
    with pytest.raises(_lib.NcxError):
        ops.mlb_att_logits_form(mw, 0, 196, 3)
    import vqa.models as M
    assert M.att.MLBAtt.hip_x6 is None and m.hip_x6 is None and "hip_x6" not in m.__dict__
    with pytest.raises(_lib.NcxError, match="device tensor"):              # x6 or not, the HIP path has no CPU fallback
        ops.mlb_att_forward(torch.zeros(3, 100, 14, 14), None, torch.zeros(3, 48), mw, x6=True)


def _tiny_yaml(tmp_path, arch=None):
    import yaml
    with open(YAML) as f:
        opt = yaml.safe_load(f)
    m = opt["model"]
    m["dim_v"], m["dim_q"], m["seq2vec"]["emb_size"] = 16, 12, 8
    m["attention"].update(dim_h=8, nb_glimpses=2)
    m["fusion"]["dim_h"] = 6
    if arch:
        m["arch"] = arch
    opt["vqa"].update(nans=10, maxlength=5)
    opt["optim"].update(batch_size=8, epochs=1)
    opt["logs"]["dir_logs"] = str(tmp_path / "logs")
    path = tmp_path / ("tiny_%s.yaml" % (arch or "att"))
    path.write_text(yaml.safe_dump(opt))
    return str(path)


def test_train_cli_x6(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    cli = _cli("train.py")
    path = _tiny_yaml(tmp_path)
    syn = ["--synthetic", "--syn_examples", "32", "--syn_images", "6", "--syn_vocab", "20", "--syn_grid", "3", "--print_freq", "0"]
    assert cli.build_parser().parse_args(["--path_opt", path, "--x6"]).x6 is True and cli.build_parser().parse_args(["--path_opt", path]).x6 is False
    with pytest.raises(SystemExit, match="--x6 .* cannot be combined with --no_hip"):
        cli.main(["--path_opt", path, "--x6", "--no_hip"] + syn)
    with pytest.raises(SystemExit, match="--x6 needs an attention arch"):
        cli.main(["--path_opt", _tiny_yaml(tmp_path, "MLBNoAtt"), "--x6"] + syn)
    with pytest.raises(SystemExit, match="MI355X"):                      # parsed and accepted; a CPU box is refused as for every HIP route
        cli.main(["--path_opt", path, "--x6"] + syn)
    out = cli.main(["--path_opt", path, "--no_hip"] + syn)
    text = capsys.readouterr().out
    assert "=> route: torch path: --no_hip" in text and "bf16 x 6" not in text
    assert out["trainer"].model.hip_x6 is None
