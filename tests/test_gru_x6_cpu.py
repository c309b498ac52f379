"""No GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the GRU encoder's step kernel from the C ABI up to train.py / counterexamples.py
--x6_seq2vec: the three new symbols, the host-only form query, flag validation before any launch or pointer use, the binding's
three-valued x6 argument, the module attribute and the two command lines."""
import ctypes
import os

import pytest
import torch

from conftest import ROOT
from test_mlb_att_cpu import _cli
from test_mlb_att_x6_cpu import _tiny_yaml as att_yaml

SYMS = ("ncx_gru_encode_flags", "ncx_gru_train_forward_flags", "ncx_gru_step_form")
DIMS = ((512, 26, 620, 2400), (2, 2, 1, 1), (5, 7, 7, 37))          # (B, T, dim_emb, dim_q)

GRU_YAML = """
logs: {dir_logs: %s}
vqa: {nans: 10, maxlength: 5}
coco: {}
model:
  arch: MutanNoAtt
  seq2vec: {%s, dropout: 0.25, fixed_emb: False}
  fusion: {dim_v: 16, dim_q: 12, dim_hv: 8, dim_hq: 8, dim_mm: 6, R: 2, activation_v: tanh, activation_q: tanh, dropout_v: 0.1, dropout_q: 0.1, dropout_hv: 0, dropout_hq: 0}
  classif: {dropout: 0.1}
optim: {lr: 0.01, batch_size: 8, epochs: 1}
"""
SYN = ["--synthetic", "--syn_examples", "32", "--syn_images", "6", "--syn_vocab", "20", "--print_freq", "0"]


def _yaml(tmp_path, seq2vec):
    path = tmp_path / ("gru_x6_%d.yaml" % len(seq2vec))
    path.write_text(GRU_YAML % (str(tmp_path / "logs"), seq2vec))
    return str(path)


def test_symbols_declared_exported_and_bound():
    from neuralcx import _lib
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = _lib.lib()
    for s in SYMS:
        assert s + "(" in hdr and s in _lib.EXPORTS, s
        assert getattr(L, s).argtypes is not None, s
    # `uint32_t flags` sits before `workspace`, after the eight arguments up to `packed`
    assert L.ncx_gru_encode_flags.argtypes[8] is ctypes.c_uint32 and len(L.ncx_gru_encode_flags.argtypes) == len(L.ncx_gru_encode.argtypes) + 1
    assert list(L.ncx_gru_train_forward_flags.argtypes) == list(L.ncx_gru_encode_flags.argtypes)
    covered = hdr[hdr.index("Covered:"):hdr.index("#define NCX_F_X6")]
    assert "ncx_gru_encode_flags" in covered and "ncx_gru_train_forward_flags" in covered


def test_step_form_through_the_c_call():
    from neuralcx import _lib
    form = _lib.lib().ncx_gru_step_form
    for B, T, de, dq in DIMS:
        assert form(B, T, de, dq, 0) == 0 and form(B, T, de, dq, _lib.NCX_F_X6) == 1, (B, T, de, dq)
        for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
            assert form(B, T, de, dq, flags) == -1, flags
    for flags in (0, _lib.NCX_F_X6):
        for bad in ((0, 7, 7, 37), (5, 65, 7, 37), (5, 7, 0, 37), (5, 7, 7, 0)):       # B = 0, T = 65, a zero width
            assert form(*bad, flags) == -1, (bad, flags)


def test_flags_are_checked_before_any_launch_or_pointer_use():
    from neuralcx import _lib
    L = _lib.lib()
    for entry in (L.ncx_gru_encode_flags, L.ncx_gru_train_forward_flags):
        call = lambda flags: entry(None, 5, 7, None, 31, 7, 37, None, flags, None, 0, None, None, None)
        for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
            assert call(flags) == -1, flags
        for flags in (0, _lib.NCX_F_X6):            # an accepted flag: the NULL pointers are what is refused
            assert call(flags) == -1, flags
    # a refused flag beside arguments that are otherwise complete (never dereferenced: refused before any launch)
    buf = (ctypes.c_float * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    n = L.ncx_gru_workspace_bytes(5, 7, 7, 37)
    assert L.ncx_gru_encode_flags(p, 5, 7, p, 31, 7, 37, p, 0x100, p, n, p, p, None) == -1
    assert L.ncx_gru_encode_flags(p, 5, 7, p, 31, 7, 37, p, _lib.NCX_F_X6, p, n - 1, p, p, None) == -1      # short workspace, X6 as fp32
    # the sizes do not know the flag: the X6 form reads the existing pack and the existing workspaces
    assert L.ncx_gru_packed_bytes(22, 100) == (4 * 96 * (32 + 128) + 4 * 192) * 4


def test_binding_reads_the_process_flag_at_call_time(monkeypatch):
    from neuralcx import _lib, ops
    monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    for B, T, de, dq in DIMS:
        form = lambda **k: ops.gru_step_form(de, dq, B, T, **k)
        assert form() == "fp32" and form(x6=None) == "fp32" and form(x6=True) == "x6" and form(x6=False) == "fp32"
    monkeypatch.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6)
    assert ops.gru_step_form(620, 2400, 512, 26) == "x6" and ops.gru_step_form(620, 2400, 512, 26, x6=None) == "x6"
    assert ops.gru_step_form(620, 2400, 512, 26, x6=False) == "fp32"        # an explicit choice wins over the process-wide one
    with pytest.raises(_lib.NcxError):
        ops.gru_step_form(620, 2400, 0, 26)
    with pytest.raises(_lib.NcxError):
        ops.gru_step_form(620, 2400, 4, 65, x6=True)


def test_module_attribute_and_no_cpu_fallback():
    from neuralcx import _lib, ops
    from vqa.models.seq2vec import GRUEncoder
    enc = GRUEncoder(["w%d" % i for i in range(20)], dim_q=12, dim_emb=8).eval()
    assert GRUEncoder.hip_x6 is None and enc.hip_x6 is None and "hip_x6" not in enc.__dict__
    assert "hip_x6" not in enc.state_dict() and len(enc.state_dict()) == 5
    wids = torch.tensor([[3, 4, 0], [5, 0, 0]])
    gw = ops.gru_weights(enc)
    raised = []
    for x6 in (None, True):                         # x6 or not, the HIP path has no CPU fallback: the same refusal
        with pytest.raises(_lib.NcxError) as e:
            ops.gru_encode(wids, gw, x6=x6)
        raised.append(str(e.value))
    assert raised[0] == raised[1]
    enc.hip_x6 = True                               # changes no routing decision: a CPU tensor stays on the torch path
    with torch.no_grad():
        want = GRUEncoder.forward(enc, wids)
        assert not enc._hip_ok(wids) and torch.equal(enc(wids), want)


def test_parsers_accept_the_switch(tmp_path):
    train, cx = _cli("train.py"), _cli("counterexamples.py")
    path = _yaml(tmp_path, "arch: gru, emb_size: 8")
    assert train.build_parser().parse_args(["--path_opt", path, "--x6_seq2vec"]).x6_seq2vec is True
    a = train.build_parser().parse_args(["--path_opt", path])
    assert a.x6_seq2vec is False and a.x6 is False                          # a new flag: no default changes
    assert cx.build_parser().parse_args(["--x6_seq2vec"]).x6_seq2vec is True
    a = cx.build_parser().parse_args([])
    assert a.x6_seq2vec is False and a.x6 is False and a.no_hip_seq2vec is False
    assert cx.build_parser().parse_args(["--x6"]).x6_seq2vec is False        # --x6 keeps its meaning: NeuralModel's kernels only


def test_train_cli_refusals(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    cli = _cli("train.py")
    gru = _yaml(tmp_path, "arch: gru, emb_size: 8")
    with pytest.raises(SystemExit, match="--x6_seq2vec .* cannot be combined with --no_hip"):
        cli.main(["--path_opt", gru, "--x6_seq2vec", "--no_hip"] + SYN)
    with pytest.raises(SystemExit, match="--x6_seq2vec needs the GRU encoder"):
        cli.main(["--path_opt", _yaml(tmp_path, "arch: 2-lstm, emb_size: 8, hidden_size: 6"), "--x6_seq2vec"] + SYN)
    with pytest.raises(SystemExit, match="MI355X"):                      # parsed and accepted; a CPU box is refused as for every HIP route
        cli.main(["--path_opt", gru, "--x6_seq2vec"] + SYN)
    with pytest.raises(SystemExit, match="--x6 needs an attention arch"):  # --x6 keeps its meaning on a no-attention arch
        cli.main(["--path_opt", att_yaml(tmp_path, "MLBNoAtt"), "--x6"] + SYN + ["--syn_grid", "3"])
    out = cli.main(["--path_opt", gru, "--no_hip"] + SYN)
    text = capsys.readouterr().out
    assert "=> route: torch path: --no_hip" in text and "bf16 x 6" not in text
    assert out["trainer"].model.seq2vec.hip_x6 is None


def test_counterexamples_cli_refusal():
    cli = _cli("counterexamples.py")
    with pytest.raises(SystemExit, match="--x6_seq2vec .* cannot be combined with --no_hip_seq2vec"):
        cli.main(["--synthetic", "-cx", "DistanceBaseline", "--x6_seq2vec", "--no_hip_seq2vec"])
