"""No GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the GRU encoder's backward through time from the C ABI up to train.py
--x6_seq2vec --hip_seq2vec_train: the two new symbols, the host-only form query, flag validation before any pointer use, the binding's
three-valued x6 argument, the autograd function handing hip_x6 on, the command line -- and an emulation of the cut (tests/gru_bwd_x6_ref.py)
that pins the accuracy bound of tests/test_gru_bwd_x6_gpu.py:

    err_x6 <= 1.5 err_fp32 + c max|ref|   per gradient tensor,   c = 1e-7 (the floor of the forward's X6 suite)

err_fp32 is the same restatement with plain fp32 matmuls.  The emulation's figures with all four products cut (max|x - fp64| of dW_ih /
dW_hh; fp32 beside it; the c a form would need on those two tensors):
    real    eight products 4.7e-6 / 5.8e-7 (fp32 5.5e-6 / 5.8e-7; c = 0);  five 2.3e-4 / 2.5e-5 (c >= 9.8e-6);  three 6.9e-4 / 7.7e-5 (c >= 3.0e-5)
    fall    eight products 6.7e-6 / 1.4e-6 (fp32 8.2e-6 / 1.2e-6; c = 0);  five 3.7e-4 / 6.1e-5 (c >= 1.1e-5);  three 9.6e-4 / 1.5e-4 (c >= 2.7e-5)
    all26   eight products 6.5e-6 / 1.1e-6 (fp32 7.2e-6 / 1.1e-6; c = 0);  five 2.4e-4 / 2.8e-5 (c >= 9.4e-6);  three 6.1e-4 / 8.4e-5 (c >= 2.6e-5)
db_ih, db_hh (the sweep alone) and dE (the sweep and dX) tell the same story: eight products need c = 0, five c >= 1.8e-6, three c >= 6.1e-6.
So c = 1e-7 separates the shipped form from the truncated ones by more than an order of magnitude on every tensor."""
import ctypes
import os

import numpy as np
import pytest
import torch

import gru_bwd_x6_ref as x6ref
import test_gru_train_gpu as train_suite          # (shapes and recipes only: nothing of it runs here)
from conftest import PKG, ROOT
from gru_train_ref import gru_train
from test_gru_x6_cpu import DIMS, SYN, _yaml
from test_mlb_att_cpu import _cli

SYMS = ("ncx_gru_train_backward_flags", "ncx_gru_bwd_form")
C_FLOOR = 1e-7


def test_symbols_declared_exported_and_bound():
    from neuralcx import _lib
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = _lib.lib()
    for s in SYMS:
        assert s + "(" in hdr and s in _lib.EXPORTS, s
        assert getattr(L, s).argtypes is not None, s
    plain, flags = list(L.ncx_gru_train_backward.argtypes), list(L.ncx_gru_train_backward_flags.argtypes)
    assert flags[8] is ctypes.c_uint32 and flags[:8] + flags[9:] == plain          # `uint32_t flags` after `packed_t`
    assert list(L.ncx_gru_bwd_form.argtypes) == [ctypes.c_int32] * 4 + [ctypes.c_uint32]


def test_bwd_form_through_the_c_call():
    from neuralcx import _lib, ops
    form = _lib.lib().ncx_gru_bwd_form
    assert x6ref.SHIPPED_MASK & (ops.GRU_BWD_DWHH | ops.GRU_BWD_DWIH) == ops.GRU_BWD_DWHH | ops.GRU_BWD_DWIH == 12   # the two walks are required
    assert (ops.GRU_BWD_SWEEP, ops.GRU_BWD_DX) == (x6ref.SWEEP, x6ref.DX) == (1, 2)
    shapes = DIMS + tuple((B, T, de, dq) for de, dq, B, T in train_suite.SHAPES.values())
    for B, T, de, dq in shapes:
        assert form(B, T, de, dq, 0) == 0 and form(B, T, de, dq, _lib.NCX_F_X6) == x6ref.SHIPPED_MASK, (B, T, de, dq)
        for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
            assert form(B, T, de, dq, flags) == -1, flags
    for flags in (0, _lib.NCX_F_X6):
        for bad in ((0, 7, 7, 37), (5, 65, 7, 37), (5, 7, 0, 37), (5, 7, 7, 0)):       # B = 0, T = 65, a zero width
            assert form(*bad, flags) == -1, (bad, flags)


def test_flags_are_checked_before_any_pointer_use():
    from neuralcx import _lib
    L = _lib.lib()
    call = lambda flags: L.ncx_gru_train_backward_flags(None, 5, 7, None, 31, 7, 37, None, flags, None, 0, None, None, None, None, None, None, None)
    for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16, 1):
        assert call(flags) == -1, flags
    for flags in (0, _lib.NCX_F_X6):                # an accepted flag: the NULL pointers are what is refused
        assert call(flags) == -1, flags
    # a refused flag beside arguments that are otherwise complete (never dereferenced: refused before any launch)
    buf = (ctypes.c_float * 1024)()
    p = ctypes.c_void_p((ctypes.addressof(buf) + 255) // 256 * 256)
    n = L.ncx_gru_train_workspace_bytes(5, 7, 7, 37)
    assert n > 0
    assert L.ncx_gru_train_backward_flags(p, 5, 7, p, 31, 7, 37, p, 0x100, p, n, p, p, p, p, p, p, None) == -1
    assert L.ncx_gru_train_backward_flags(p, 5, 7, p, 31, 7, 37, p, _lib.NCX_F_X6, p, n - 1, p, p, p, p, p, p, None) == -1   # short workspace, X6 as fp32
    # the sizes do not know the flag: the X6 form reads the existing pack and the existing workspace
    assert L.ncx_gru_packed_t_bytes(22, 100) == (128 + 64) * 3 * 128 * 4


def test_binding_reads_the_process_flag_at_call_time(monkeypatch):
    from neuralcx import _lib, ops
    monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    for B, T, de, dq in DIMS:
        form = lambda **k: ops.gru_bwd_form(de, dq, B, T, **k)
        assert form() == 0 and form(x6=None) == 0 and form(x6=True) == x6ref.SHIPPED_MASK and form(x6=False) == 0
    monkeypatch.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6)
    assert ops.gru_bwd_form(620, 2400, 512, 26) == x6ref.SHIPPED_MASK and ops.gru_bwd_form(620, 2400, 512, 26, x6=None) == x6ref.SHIPPED_MASK
    assert ops.gru_bwd_form(620, 2400, 512, 26, x6=False) == 0               # an explicit choice wins over the process-wide one
    with pytest.raises(_lib.NcxError):
        ops.gru_bwd_form(620, 2400, 0, 26)
    with pytest.raises(_lib.NcxError):
        ops.gru_bwd_form(620, 2400, 4, 65, x6=True)


def test_backward_binding_resolves_x6_like_the_forward(monkeypatch):
    """ops.gru_train_backward hands mlb_att_flags(x6) to ncx_gru_train_backward_flags: seen through a stand-in library."""
    from neuralcx import _lib, ops
    seen = []

    class Lib:
        def ncx_gru_train_backward_flags(self, *a):
            seen.append(a[8])
            return 0
    monkeypatch.setattr(_lib, "lib", lambda: Lib())
    monkeypatch.setattr(ops, "_ptr", lambda t, *a: None)
    monkeypatch.setattr(ops, "_ws_ptr", lambda ws: (None, 0))
    monkeypatch.setattr(ops, "_stream", lambda: None)
    gw = ops.GruTrainWeights.__new__(ops.GruTrainWeights)
    monkeypatch.setattr(ops, "_gru_train_args", lambda wids, gw_, who: (2, 3, wids))
    for k, v in (("dim_emb", 4), ("dim_q", 5), ("V1", 6), ("E", None), ("packed_t", None)):
        object.__setattr__(gw, k, v)
    wids, d = torch.zeros(2, 3, dtype=torch.int64), torch.zeros(2, 5)
    for process_wide in (0, _lib.NCX_F_X6):
        monkeypatch.setattr(ops, "EXTRA_FLAGS", process_wide)
        for x6, want in ((None, process_wide), (True, _lib.NCX_F_X6), (False, 0)):
            del seen[:]
            ops.gru_train_backward(wids, gw, None, d, x6=x6)
            assert seen == [want], (process_wide, x6)
        del seen[:]
        ops.gru_train_backward(wids, gw, None, d)                                  # the argument's default is None
        assert seen == [process_wide]


def test_autograd_function_hands_hip_x6_to_the_backward(monkeypatch):
    from neuralcx import ops
    from neuralcx.vqa_train import GruTrainFunction
    from vqa.models.seq2vec import GRUEncoder
    enc = GRUEncoder(["w%d" % i for i in range(20)], dim_q=12, dim_emb=8).train()
    g = enc.gru
    wids = torch.tensor([[3, 4, 0], [5, 0, 0]])
    seen = {"fwd": [], "bwd": []}
    monkeypatch.setattr(ops, "gru_train_weights", lambda *t: "gw")
    monkeypatch.setattr(ops, "gru_train_workspace", lambda *a: "ws")
    monkeypatch.setattr(ops, "gru_train_forward", lambda w, gw, ws, x6=None: (seen["fwd"].append(x6), torch.zeros(2, 12))[1])

    def bwd(w, gw, ws, dq, want_dE=True, x6="unset"):
        seen["bwd"].append(x6)
        return {"E": torch.zeros(21, 8), "w_ih": torch.zeros(36, 8), "w_hh": torch.zeros(36, 12), "b_ih": torch.zeros(36), "b_hh": torch.zeros(36)}
    monkeypatch.setattr(ops, "gru_train_backward", bwd)
    for flag in (True, False, None):
        enc.hip_x6 = flag
        out = GruTrainFunction.apply(wids, enc.embedding.weight, g.weight_ih_l0, g.weight_hh_l0, g.bias_ih_l0, g.bias_hh_l0, enc)
        enc.hip_x6 = "changed after the forward"              # the choice is read once, in forward, and kept on ctx
        out.sum().backward()
    assert seen["fwd"] == [True, False, None] and seen["bwd"] == [True, False, None]
    enc.__dict__.pop("hip_x6", None)
    # the module stays on the CPU route otherwise: hip_x6 changes no routing decision
    enc.hip_x6, enc.use_hip_train = True, True
    del seen["fwd"][:]
    assert enc(wids).shape == (2, 12) and seen["fwd"] == []


def test_train_cli_route_line_and_refusals(tmp_path, monkeypatch):
    src = open(os.path.join(PKG, "train.py")).read()
    line = src[src.index('print("=> route:'):]
    line = line[:line.index("flush=True")]
    first, second = '" (question encoder: bf16 x 6 step kernel)"', '" (and the bf16 x 6 products of its backward)"'
    assert first in line and second in line and line.index(first) < line.index(second)
    assert "hip_seq2vec" in line[line.index(second):line.index(second) + 120]      # the backward's note only where the encoder trains in HIP
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)        # (the GPU box runs this test too)
    cli = _cli("train.py")
    gru = _yaml(tmp_path, "arch: gru, emb_size: 8")
    with pytest.raises(SystemExit, match="--x6_seq2vec .* cannot be combined with --no_hip"):
        cli.main(["--path_opt", gru, "--x6_seq2vec", "--no_hip"] + SYN)
    with pytest.raises(SystemExit, match="--hip_seq2vec_train .* cannot be combined with --no_hip"):       # the older refusal still comes first
        cli.main(["--path_opt", gru, "--x6_seq2vec", "--hip_seq2vec_train", "--no_hip"] + SYN)
    with pytest.raises(SystemExit, match="--x6_seq2vec needs the GRU encoder"):
        cli.main(["--path_opt", _yaml(tmp_path, "arch: 2-lstm, emb_size: 8, hidden_size: 6"), "--x6_seq2vec", "--hip_seq2vec_train"] + SYN)
    with pytest.raises(SystemExit, match="MI355X"):                      # parsed and accepted; a CPU box is refused as for every HIP route
        cli.main(["--path_opt", gru, "--x6_seq2vec", "--hip_seq2vec_train"] + SYN)


_EMU = {}


def emulation(name):
    """-> (fp64 reference, err_fp32, {nprod: err}) of a shape of test_gru_train_gpu.py, its recipe restated on the CPU."""
    if name not in _EMU:
        de, dq, B, T = train_suite.SHAPES[name]
        enc = train_suite.make_encoder(de, dq, seed=sorted(train_suite.SHAPES).index(name))
        rng = np.random.default_rng(7)
        wids = train_suite.make_wids(name, B, T, rng)
        dq_out = rng.standard_normal((B, dq)).astype(np.float32)
        E, w_ih, w_hh, b_ih, b_hh = [t.numpy() for t in train_suite.tensors_of(enc)]
        ref = gru_train(wids, E, w_ih, w_hh, b_ih, b_hh, dq_out)
        lens, stash = x6ref.forward_stash(wids, E, w_ih, w_hh, b_ih, b_hh)
        run = lambda mask, n: x6ref.errors(x6ref.backward(wids, E, w_ih, w_hh, dq_out, lens, stash, mask, n), ref)
        _EMU[name] = (ref, run(0, x6ref.SHIPPED_NPROD), {n: run(x6ref.SHIPPED_MASK, n) for n in (x6ref.SHIPPED_NPROD, 5, 3)})
    return _EMU[name]


def test_the_cut_is_exact():
    x = torch.randn(4096) * torch.logspace(-20, 20, 4096)
    x1, x2, x3 = x6ref.cut(x)
    assert torch.equal(x1 + x2 + x3, x) and torch.equal((x1 + x2) + x3, x)
    for p in (x1, x2, x3):
        assert torch.equal(p.bfloat16().float(), p)                 # every plane is a bf16 value
    a, b = torch.randn(8, 64), torch.randn(64, 8)
    exact = a.double() @ b.double()
    assert float((x6ref.plane_matmul(a, b, 8).double() - exact).abs().max()) <= 4 * float((a @ b - exact).abs().max()) + 1e-6
    assert float((x6ref.plane_matmul(a, b, 3).double() - exact).abs().max()) > 1e-5      # three planes products are not fp32 grade


@pytest.mark.parametrize("name", ["real", "fall", "all26"])
def test_emulated_cut_pins_the_bound(name):
    ref, e32, forms = emulation(name)
    bound = x6ref.bound(e32, ref, C_FLOOR)
    for n, err in forms.items():
        for k in x6ref.GRADS:
            print("%s %d products d%s: err %.3e, fp32 %.3e, bound %.3e, max|ref| %.3e" % (name, n, k, err[k], e32[k], bound[k], float(np.abs(ref[k]).max())))
    shipped = forms[x6ref.SHIPPED_NPROD]
    for k in x6ref.GRADS:
        assert shipped[k] <= bound[k], (name, k)
    for n in (5, 3):
        assert any(forms[n][k] > bound[k] for k in x6ref.GRADS), (name, n)
        assert forms[n]["w_hh"] > bound["w_hh"] and forms[n]["w_ih"] > bound["w_ih"], (name, n)      # a truncated walk shows in the tensor it makes
