"""No GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the 2-lstm encoder's step kernel from the C ABI up to train.py --x6_2lstm: the three new
symbols, the host-only form query, flag validation before any launch or pointer use, the binding's three-valued x6 argument, the module
attribute, the command line -- and the emulation that gives the GPU suite's fp32-grade bound its meaning.

The emulation restates the cut (x = x1 + x2 + x3, three bf16 values by truncation) and the recurrence without the wavefront (tanh(E),
two layers, every row at every step, the step's product [x_t | h_{t-1}] . [W_ih | W_hh]^T as fp32 matmuls over the planes, small terms
first) in torch on the CPU, on `real`, `fall` and `all26` of test_lstm_gpu.SHAPES.  With e32 the error of a plain fp32 forward against
tests/lstm_ref.py, six products must stay within 1.5 e32 + 1e-7 max(1, max|ref|); three products, and each five-product form that drops
one of a1 b3, a2 b2, a3 b1, must exceed that bound at least fivefold.  Those errors (1.5e-5 .. 6.6e-5) are below the suites' 1e-4: only
this bound tells a dropped plane product from a correct kernel."""
import ctypes
import os

import numpy as np
import pytest
import torch

import lstm_ref
import test_lstm_gpu as fwd_suite
from conftest import ROOT
from test_gru_x6_cpu import GRU_YAML, SYN
from test_mlb_att_cpu import _cli
from x6_ref import cut

SYMS = ("ncx_lstm2_encode_flags", "ncx_lstm2_train_forward_flags", "ncx_lstm2_step_form")
DIMS = ((512, 26, 620, 1200), (2, 2, 1, 1), (5, 7, 7, 37))          # (B, T, emb, H)
LSTM = "arch: 2-lstm, emb_size: 8, hidden_size: 6"


def _yaml(tmp_path, seq2vec):
    path = tmp_path / ("lstm_x6_%d.yaml" % len(seq2vec))
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
    assert L.ncx_lstm2_encode_flags.argtypes[8] is ctypes.c_uint32 and L.ncx_lstm2_train_forward_flags.argtypes[8] is ctypes.c_uint32
    assert len(L.ncx_lstm2_encode_flags.argtypes) == len(L.ncx_lstm2_encode.argtypes) + 1
    assert list(L.ncx_lstm2_train_forward_flags.argtypes) == list(L.ncx_lstm2_encode_flags.argtypes)
    assert list(L.ncx_lstm2_step_form.argtypes) == [ctypes.c_int32] * 4 + [ctypes.c_uint32]
    covered = hdr[hdr.index("Covered:"):hdr.index("#define NCX_F_X6")]
    assert "ncx_lstm2_encode_flags" in covered and "ncx_lstm2_train_forward_flags" in covered
    assert "ncx_gru_encode_flags" in covered                                 # one MORE bullet: the GRU's stays


def test_step_form_through_the_c_call():
    from neuralcx import _lib
    form = _lib.lib().ncx_lstm2_step_form
    for B, T, emb, H in DIMS:
        assert form(B, T, emb, H, 0) == 0 and form(B, T, emb, H, _lib.NCX_F_X6) == 1, (B, T, emb, H)
        for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
            assert form(B, T, emb, H, flags) == -1, flags
    for flags in (0, _lib.NCX_F_X6):
        for bad in ((0, 7, 7, 37), (5, 65, 7, 37), (5, 7, 0, 37), (5, 7, 7, 0)):       # B = 0, T = 65, a zero width
            assert form(*bad, flags) == -1, (bad, flags)


def test_flags_are_checked_before_any_launch_or_pointer_use():
    from neuralcx import _lib
    L = _lib.lib()
    for entry in (L.ncx_lstm2_encode_flags, L.ncx_lstm2_train_forward_flags):
        call = lambda flags: entry(None, 5, 7, None, 31, 7, 37, None, flags, None, 0, None, None, None)
        for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
            assert call(flags) == -1, flags
        for flags in (0, _lib.NCX_F_X6):            # an accepted flag: the NULL pointers are what is refused
            assert call(flags) == -1, flags
    # a refused flag beside arguments that are otherwise complete (never dereferenced: refused before any launch)
    n, nt = L.ncx_lstm2_workspace_bytes(5, 7, 7, 37), L.ncx_lstm2_train_workspace_bytes(5, 7, 7, 37)
    assert 0 < n < nt
    buf = (ctypes.c_char * (nt + 512))()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    for flags in (0x100, _lib.NCX_F_BF16, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
        assert L.ncx_lstm2_encode_flags(p, 5, 7, p, 31, 7, 37, p, flags, p, n, p, p, None) == -1
        assert L.ncx_lstm2_train_forward_flags(p, 5, 7, p, 31, 7, 37, p, flags, p, nt, p, p, None) == -1
    for flags in (0, _lib.NCX_F_X6):                # a workspace one byte short: refused under X6 as under 0
        assert L.ncx_lstm2_encode_flags(p, 5, 7, p, 31, 7, 37, p, flags, p, n - 1, p, p, None) == -1
        assert L.ncx_lstm2_train_forward_flags(p, 5, 7, p, 31, 7, 37, p, flags, p, nt - 1, p, p, None) == -1


# (B, T, emb, H) -> ncx_lstm2_packed_bytes, ncx_lstm2_workspace_bytes, ncx_lstm2_train_workspace_bytes of the commit before the flag existed
SIZES = {(512, 26, 620, 1200): (83466240, 14752000, 1329572096), (2, 2, 1, 1): (66560, 2560, 11264), (5, 7, 7, 37): (231424, 5632, 168704),
         (70, 26, 40, 136): (1397760, 230656, 22974464)}


def test_sizes_do_not_know_the_flag():
    """The X6 form reads the existing pack and the existing workspaces: the three sizes are what they were."""
    from neuralcx import _lib
    L = _lib.lib()
    pad = lambda n, m: (n + m - 1) // m * m
    for (B, T, emb, H), (packed, ws, train_ws) in SIZES.items():
        rows = pad(H, 32) * 4                                                # weight rows of a layer = floats of its bias block
        assert packed == sum(rows * (pad(i, 32) + pad(H, 32)) + rows for i in (emb, H)) * 4          # (the layout of csrc/ncx_lstm.hip, restated)
        assert L.ncx_lstm2_packed_bytes(emb, H) == packed, (emb, H)
        assert L.ncx_lstm2_workspace_bytes(B, T, emb, H) == ws, (B, T, emb, H)
        assert L.ncx_lstm2_train_workspace_bytes(B, T, emb, H) == train_ws, (B, T, emb, H)


def test_binding_reads_the_process_flag_at_call_time(monkeypatch):
    from neuralcx import _lib, ops
    monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    for B, T, emb, H in DIMS:
        form = lambda **k: ops.lstm_step_form(emb, H, B, T, **k)
        assert form() == "fp32" and form(x6=None) == "fp32" and form(x6=True) == "x6" and form(x6=False) == "fp32"
    monkeypatch.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6)
    assert ops.lstm_step_form(620, 1200, 512, 26) == "x6" and ops.lstm_step_form(620, 1200, 512, 26, x6=None) == "x6"
    assert ops.lstm_step_form(620, 1200, 512, 26, x6=False) == "fp32"        # an explicit choice wins over the process-wide one
    with pytest.raises(_lib.NcxError):
        ops.lstm_step_form(620, 1200, 0, 26)
    with pytest.raises(_lib.NcxError):
        ops.lstm_step_form(620, 1200, 4, 65, x6=True)


def test_module_attribute_and_no_cpu_fallback():
    from neuralcx import _lib, ops
    from vqa.models.seq2vec import TwoLSTM
    enc = TwoLSTM(["w%d" % i for i in range(20)], 8, 6).eval()
    assert TwoLSTM.hip_x6 is None and enc.hip_x6 is None and "hip_x6" not in enc.__dict__
    assert "hip_x6" not in enc.state_dict() and len(enc.state_dict()) == 9
    wids = torch.tensor([[3, 4, 0], [5, 0, 0]])
    lw = ops.lstm_weights(enc)
    raised = []
    for x6 in (None, True, False):                  # x6 or not, the HIP path has no CPU fallback: the same refusal
        with pytest.raises(_lib.NcxError) as e:
            ops.lstm_encode(wids, lw, x6=x6)
        raised.append(str(e.value))
    assert raised[0] == raised[1] == raised[2]
    enc.hip_x6 = True                               # changes no routing decision: a CPU tensor stays on the torch path
    with torch.no_grad():
        want = TwoLSTM.forward(enc, wids)
        assert not enc._hip_ok(wids) and torch.equal(enc(wids), want)
    assert "hip_x6" not in enc.state_dict()


def test_train_cli_parses_and_refuses(tmp_path, monkeypatch, capsys):
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    cli = _cli("train.py")
    lstm, gru = _yaml(tmp_path, LSTM), _yaml(tmp_path, "arch: gru, emb_size: 8")
    assert cli.build_parser().parse_args(["--path_opt", lstm, "--x6_2lstm"]).x6_2lstm is True
    a = cli.build_parser().parse_args(["--path_opt", lstm])
    assert a.x6_2lstm is False and a.x6_seq2vec is False and a.x6 is False      # a new switch: no default changes
    with pytest.raises(SystemExit, match="--x6_2lstm .* cannot be combined with --no_hip"):
        cli.main(["--path_opt", lstm, "--x6_2lstm", "--no_hip"] + SYN)
    with pytest.raises(SystemExit, match="--x6_2lstm needs the 2-lstm encoder"):
        cli.main(["--path_opt", gru, "--x6_2lstm"] + SYN)
    with pytest.raises(SystemExit, match="--x6_seq2vec needs the GRU encoder.*--x6_2lstm"):       # the GRU switch keeps refusing, and points here
        cli.main(["--path_opt", lstm, "--x6_seq2vec"] + SYN)
    with pytest.raises(SystemExit, match="MI355X"):                      # parsed and accepted; a CPU box is refused as for every HIP route
        cli.main(["--path_opt", lstm, "--x6_2lstm"] + SYN)
    with pytest.raises(SystemExit, match="MI355X"):
        cli.main(["--path_opt", lstm, "--x6_2lstm", "--freeze_seq2vec"] + SYN)
    out = cli.main(["--path_opt", lstm, "--no_hip"] + SYN)
    text = capsys.readouterr().out
    assert "=> route: torch path: --no_hip" in text and "bf16 x 6" not in text
    assert out["trainer"].model.seq2vec.hip_x6 is None


def test_counterexamples_help_names_both_encoders():
    cx = _cli("counterexamples.py")
    text = cx.build_parser().format_help()
    assert "TwoLSTM.hip_x6" in " ".join(text.split()) and cx.build_parser().parse_args(["--x6_seq2vec"]).x6_seq2vec is True


# ---- the emulation ------------------------------------------------------------------------------------------------------------------

SIX = ((0, 2), (1, 1), (2, 0), (0, 1), (1, 0), (0, 0))              # (plane of a, plane of b), small terms first: a1 b3 ... a1 b1
THREE = ((0, 1), (1, 0), (0, 0))
FIVES = {"no a1 b3": SIX[1:], "no a2 b2": SIX[:1] + SIX[2:], "no a3 b1": SIX[:2] + SIX[3:]}


def emulate(wids, E, layer0, layer1, products):
    """TwoLSTM's forward in fp32 on the CPU, every row at every step; products None: plain matmuls, else the plane products in order."""
    wids = torch.from_numpy(wids)
    x = torch.tanh(torch.from_numpy(E)[wids])                           # the tanh BEFORE the cut
    B, T = wids.shape
    outs = []
    for layer in (layer0, layer1):
        w_ih, w_hh, b_ih, b_hh = (torch.from_numpy(a) for a in layer)
        H = w_hh.shape[1]
        W = torch.cat([w_ih, w_hh], 1).t().contiguous()
        Wp = cut(W) if products else None
        bias = b_ih + b_hh
        h, c = torch.zeros(B, H), torch.zeros(B, H)
        out = torch.zeros(B, T, H)
        for t in range(T):
            A = torch.cat([x[:, t], h], 1)
            if products:
                Ap = cut(A)
                g = torch.zeros(B, 4 * H)
                for pa, pb in products:
                    g = g + Ap[pa] @ Wp[pb]
            else:
                g = A @ W
            g = g + bias
            c = torch.sigmoid(g[:, H:2 * H]) * c + torch.sigmoid(g[:, :H]) * torch.tanh(g[:, 2 * H:3 * H])
            h = torch.sigmoid(g[:, 3 * H:]) * torch.tanh(c)
            out[:, t] = h
        outs.append(out)
        x = out
    lens = lstm_ref.lengths(wids.numpy())
    return np.concatenate([lstm_ref.select_last(o.numpy(), lens) for o in outs], 1)


def test_the_cut_is_exact_and_each_plane_is_a_bf16():
    torch.manual_seed(0)
    x = torch.cat([torch.randn(4096) * 3, torch.randn(4096) * 1e-3, torch.tensor([0.0, 1.0, -1.0, 2.0 ** -100, 1.0 + 2.0 ** -23])])
    x1, x2, x3 = cut(x)
    assert torch.equal(x1 + x2 + x3, x) and torch.equal((x1 + x2) + x3, x)
    for p in (x1, x2, x3):
        assert torch.equal(p.to(torch.bfloat16).to(torch.float32), p)


@pytest.mark.parametrize("name", ["fall", "all26", "real"])
def test_six_products_are_fp32_grade_and_fewer_are_not(name):
    emb, H, B, T = fwd_suite.SHAPES[name]
    enc = fwd_suite.make_encoder(emb, H, seed=sorted(fwd_suite.SHAPES).index(name))
    wids = fwd_suite.make_wids(name, B, T, np.random.default_rng(7))
    w = fwd_suite.weights_of(enc)
    ref = lstm_ref.lstm_encode(wids, *w)
    torch.set_num_threads(min(torch.get_num_threads(), 16))
    err = lambda products: float(np.abs(emulate(wids, *w, products) - ref).max())
    e32, e6 = err(None), err(SIX)
    bound = 1.5 * e32 + 1e-7 * max(1.0, float(np.abs(ref).max()))
    print("%s: plain fp32 %.3e, six products %.3e, bound %.3e" % (name, e32, e6, bound))
    assert e6 <= bound
    fewer = dict(FIVES, three=THREE)
    for tag, products in fewer.items():
        e = err(products)
        print("%s: %s %.3e (%.1f x the bound)" % (name, tag, e, e / bound))
        assert e >= 5 * bound, tag
        assert e < 1e-4, tag                                                 # ... and the suites' tolerance would not have seen it
