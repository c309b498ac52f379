"""No GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the MLB attention model's weight-gradient kernel (k_att_dwv_x6) from the C ABI up
to the binding: the host-only form query, flag validation before any launch, the unchanged workspace and the binding's three-valued
x6 argument."""
import ctypes
import os

import pytest

from conftest import ROOT
from test_mlb_att_x6_cpu import _dims, _params, _weights

FORMS = {0: "small", 1: "fp32", 2: "x6"}


def test_dwv_form_through_the_c_call():
    from neuralcx import _lib
    lib = _lib.lib()
    form = lambda flags, **over: lib.ncx_mlb_att_dwv_form(ctypes.byref(_dims(**over)), flags)
    assert FORMS[form(0)] == "fp32" and FORMS[form(_lib.NCX_F_X6)] == "x6"                     # P = 196
    assert FORMS[form(0, P=35)] == "fp32" and FORMS[form(_lib.NCX_F_X6, P=35)] == "x6"
    for P in (1, 3):                                # no 16-byte window in a row of the map: the small kernel under both flags
        assert FORMS[form(0, P=P)] == "small" and FORMS[form(_lib.NCX_F_X6, P=P)] == "small"
    assert FORMS[form(_lib.NCX_F_X6, P=4)] == "x6"
    for over in (dict(G=9), dict(dv=3)):
        assert form(0, **over) < 0 and form(_lib.NCX_F_X6, **over) < 0, over
    assert form(_lib.NCX_F_BF16) < 0 and form(0x100) < 0 and lib.ncx_mlb_att_dwv_form(None, 0) < 0


def test_backward_flags_are_checked_before_any_launch():
    from neuralcx import _lib
    lib = _lib.lib()
    d, m, t = _dims(), _params(), _lib.NcxMlbAttTrain()
    call = lambda flags: lib.ncx_mlb_att_train_backward_flags(ctypes.byref(d), ctypes.byref(t), None, None, None, ctypes.byref(m), None, flags,
                                                              None, 0, None, None, None, None, None)
    for flags in (_lib.NCX_F_BF16, 0x100, _lib.NCX_F_X6 | _lib.NCX_F_BF16):
        assert call(flags) == -2, flags                                                        # NCX_E_DIMS
    for flags in (0, _lib.NCX_F_X6):                # an accepted flag: the NULL pointers are what is refused
        assert call(flags) == -1, flags
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    raw = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("ncx_mlb_att_train_backward_flags", "ncx_mlb_att_dwv_form"):
        assert n + "(" in hdr and n in _lib.EXPORTS and hasattr(raw, n), n


def test_the_flag_needs_no_workspace_byte():
    """ncx_mlb_att_train_workspace_bytes has no flags argument: the slab [S][dh_att][dv] the X6 kernel writes is the fp32 kernel's,
    with S computed from the fp32 kernel's 64 x 128 tiles."""
    from neuralcx import _lib
    lib = _lib.lib()
    d, m, t = _dims(B=128, dv=2048, dh_att=1200, n_img=128), _params(), _lib.NcxMlbAttTrain()
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    assert lib.ncx_mlb_att_train_ws_region(ctypes.byref(d), ctypes.byref(t), ctypes.byref(m), 5, ctypes.byref(off), ctypes.byref(nb)) == 0
    tiles = -(-1200 // 64) * (2048 // 128)
    S = min(8, -(-1024 // tiles))
    assert S == 4 and nb.value == S * 1200 * 2048 * 4
    assert len(lib.ncx_mlb_att_train_workspace_bytes.argtypes) == 3


def test_binding_reads_the_process_flag_at_call_time(monkeypatch):
    from neuralcx import _lib, ops
    mw, m = _weights()
    form = lambda P, **k: ops.mlb_att_dwv_form(mw, 3, P, 3, **k)
    monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    assert form(196) == "fp32" and form(196, x6=None) == "fp32" and form(196, x6=True) == "x6" and form(35, x6=True) == "x6"
    monkeypatch.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6)
    assert form(196, x6=None) == "x6" and form(35) == "x6"
    assert form(196, x6=False) == "fp32"            # an explicit choice wins over the process-wide one
    assert form(1) == "small" and form(3, x6=True) == "small"
    with pytest.raises(_lib.NcxError):
        ops.mlb_att_dwv_form(mw, 0, 196, 3)
    import inspect
    assert inspect.signature(ops.mlb_att_train_backward).parameters["x6"].default is None
