"""CPU: the HIP question encoder's surroundings -- fixture vs the fp64 restatement, the C ABI's declarations and refusals, the packed
weight layout, GRUEncoder's CPU path and the rule that selects the HIP path.  No compute on a device."""
import ctypes
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN, ROOT
from gru_ref import gru_encode, lengths

CASES = ("c0", "c1")
SYMS = ("ncx_gru_packed_bytes", "ncx_gru_pack", "ncx_gru_workspace_bytes", "ncx_gru_encode")
WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def load_case(name):
    g = np.load(os.path.join(GOLDEN, "g15_gru.npz"))
    return {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}


def encoder_of(c, dropout=0.25):
    from vqa.models.seq2vec import GRUEncoder
    V1, de = c["E"].shape
    enc = GRUEncoder(["w"] * (V1 - 1), dim_q=c["weight_hh_l0"].shape[1], dim_emb=de, dropout=dropout)
    sd = {"embedding.weight": torch.from_numpy(c["E"])}
    sd.update({"gru." + k: torch.from_numpy(c[k]) for k in WKEYS})
    enc.load_state_dict(sd)
    return enc


@pytest.mark.parametrize("name", CASES)
def test_fp64_restatement_matches_the_fixture(name):
    c = load_case(name)
    ref = gru_encode(c["wids"], c["E"], *[c[k] for k in WKEYS])
    err = float(np.abs(ref - c["q"]).max())
    print(name, "max|torch fp32 nn.GRU - fp64 restatement| = %.3e" % err)
    assert ref.shape == c["q"].shape == (9, 100)
    assert err <= 1e-6


def test_fixture_has_the_planted_rows():
    c = load_case("c0")
    w = c["wids"]
    assert c["E"].shape[1] == 22 and w.shape == (9, 7)
    assert c["E"][0].any()                                       # row 0 is nonzero: it must be READ
    assert not w[2].any() and lengths(w)[2] == 1                 # the all-padding row
    assert w[3, 2] == 0 and w[3, 3] != 0 and lengths(w)[3] == 4  # a zero inside the question
    assert lengths(w)[0] == 7 and lengths(w)[1] == 1


def test_symbols_declared_and_exported():
    from neuralcx import _lib
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = _lib.lib()
    for s in SYMS:
        assert s in _lib.EXPORTS and s + "(" in hdr
        assert getattr(L, s).argtypes is not None
    # every entry point cites the lines of the reference's seq2vec.py whose role it takes
    assert "seq2vec.py:11-25" in hdr and "seq2vec.py:79-97" in hdr


def test_invalid_dims_are_refused():
    from neuralcx import _lib
    L = _lib.lib()
    assert L.ncx_gru_workspace_bytes(4, 7, 22, 100) > 0
    for bad in ((0, 7, 22, 100), (4, 0, 22, 100), (4, 65, 22, 100), (4, 7, 0, 100), (4, 7, 22, 0)):
        assert L.ncx_gru_workspace_bytes(*bad) == 0
    assert L.ncx_gru_packed_bytes(22, 100) == (4 * 96 * (32 + 128) + 4 * 192) * 4
    assert L.ncx_gru_packed_bytes(0, 100) == 0 and L.ncx_gru_packed_bytes(22, -1) == 0
    buf = (ctypes.c_float * 64)()                                # never dereferenced: every call below is refused before a launch
    p = ctypes.cast(buf, ctypes.c_void_p)
    assert L.ncx_gru_pack(p, p, p, p, 0, 100, p, None) == -1
    assert L.ncx_gru_pack(None, p, p, p, 22, 100, p, None) == -1
    n = L.ncx_gru_workspace_bytes(4, 7, 22, 100)
    assert L.ncx_gru_encode(p, 4, 65, p, 31, 22, 100, p, p, n, p, p, None) == -1        # T > 64
    assert L.ncx_gru_encode(p, 0, 7, p, 31, 22, 100, p, p, n, p, p, None) == -1         # B < 1
    assert L.ncx_gru_encode(p, 4, 7, p, 0, 22, 100, p, p, n, p, p, None) == -1          # empty table
    assert L.ncx_gru_encode(p, 4, 7, p, 31, 22, 100, p, p, n, p, None, None) == -1      # no flag
    assert L.ncx_gru_encode(p, 4, 7, p, 31, 22, 100, p, p, n - 1, p, p, None) == -1     # short workspace


@pytest.mark.parametrize("name", CASES)
def test_gru_weights_round_trip_the_gate_blocks(name):
    from neuralcx import _lib, ops
    c = load_case(name)
    enc = encoder_of(c)
    gw = ops.gru_weights(enc)
    assert isinstance(gw, ops.GruWeights) and (gw.V1, gw.dim_emb, gw.dim_q) == (31, 22, 100)
    assert gw.packed.numel() * 4 == _lib.lib().ncx_gru_packed_bytes(22, 100)
    for got, k in zip(gw.unpack(), WKEYS):
        assert np.array_equal(got.numpy(), c[k]), k
    # the layout itself: unit 37 = block 1, slot 5; its r, z, n rows sit 32 rows apart in one block, x columns then h columns
    kp = 32 + 128
    W = gw.packed[:4 * 96 * kp].view(4, 3, 32, kp).numpy()
    for g in range(3):
        assert np.array_equal(W[1, g, 5, :22], c["weight_ih_l0"][g * 100 + 37])
        assert np.array_equal(W[1, g, 5, 32:132], c["weight_hh_l0"][g * 100 + 37])
        assert not W[1, g, 5, 22:32].any() and not W[1, g, 5, 132:].any()
    assert not W[3, :, 4:].any()                                 # units 100..127 do not exist
    b = gw.packed[4 * 96 * kp:].view(4, 6, 32).numpy()
    assert b[1, 4, 5] == c["bias_hh_l0"][100 + 37] and b[1, 2, 5] == c["bias_ih_l0"][200 + 37]


@pytest.mark.parametrize("name", CASES)
def test_cpu_encoder_equals_the_fixture_bit_for_bit(name):
    c = load_case(name)
    enc = encoder_of(c).eval()
    assert enc.use_hip is True                                   # on by default; a CPU tensor never takes the HIP path
    with torch.no_grad():
        q = enc(torch.from_numpy(c["wids"]))
    assert np.array_equal(q.numpy(), c["q"])


class _Cuda:
    """A stand-in for a CUDA LongTensor as far as the selection rule looks at it."""
    is_cuda = True
    shape = (3, 7)

    def dim(self):
        return 2

    @property
    def device(self):
        return torch.device("cpu")                               # the parameters' device in this test


def test_selection_rule(monkeypatch):
    from neuralcx import ops

    def boom(*a, **k):
        raise AssertionError("ops.gru_encode called")
    monkeypatch.setattr(ops, "gru_encode", boom)
    c = load_case("c0")
    wids = torch.from_numpy(c["wids"])
    fake = _Cuda()

    enc = encoder_of(c, dropout=0.25)
    enc.train()                                                  # dropout live: torch path
    assert not enc._hip_ok(fake)
    assert enc(wids).shape == (9, 100)
    enc.eval()                                                   # a parameter requires grad under enabled grad mode: torch path
    assert torch.is_grad_enabled() and not enc._hip_ok(fake)
    out = enc(wids)
    assert out.requires_grad and np.array_equal(out.detach().numpy(), c["q"])
    with torch.no_grad():                                        # grad mode off: the HIP path (on a device)
        assert enc._hip_ok(fake) and not enc._hip_ok(wids)
        enc.use_hip = False
        assert not enc._hip_ok(fake)
        enc.use_hip = True
    for p in enc.parameters():
        p.requires_grad_(False)
    assert enc._hip_ok(fake)                                     # frozen: the HIP path with grad mode on as well
    enc.train()
    assert not enc._hip_ok(fake)
    enc0 = encoder_of(c, dropout=0.0).train()                    # training with p == 0: dropout is inert
    with torch.no_grad():
        assert enc0._hip_ok(fake)
    assert "use_hip" not in enc.state_dict() and len(enc.state_dict()) == 5


def test_cli_has_the_switch():
    import importlib.util
    from conftest import PKG
    spec = importlib.util.spec_from_file_location("cx_cli_gru_cpu", os.path.join(PKG, "counterexamples.py"))
    cli = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(cli)
    assert cli.build_parser().parse_args([]).no_hip_seq2vec is False             # a new flag: no default changes
    assert cli.build_parser().parse_args(["--no_hip_seq2vec"]).no_hip_seq2vec is True
