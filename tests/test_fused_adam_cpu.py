"""CPU: ncx_backward_adam is exported and rejects a NULL or inconsistent ncx_adam_state before any launch (no GPU needed: every call here
returns from the argument checks; the pointers are made-up addresses that are never dereferenced)."""
import ctypes as C

from conftest import ROOT  # noqa: F401  (puts the package on the path)


def _call(d, p, g, st, in_ok=True):
    from neuralcx import _lib
    ins = _lib.NcxInputs()
    return _lib.lib().ncx_backward_adam(C.byref(d), C.byref(ins) if in_ok else None, C.byref(p) if p is not None else None,
                                        C.c_void_p(1 << 20), 1 << 30, C.c_void_p(1 << 12), C.byref(g) if g is not None else None,
                                        C.byref(st) if st is not None else None, None)


def _consistent():
    """dims and four flat buffers at made-up 16-byte aligned addresses, laid out like the engine's: answer_embedding first."""
    from neuralcx import _lib
    d = _lib.NcxDims(B=4, K=24, dv=16, dq=8, dz=8, da=36, A=68, H=32, L=1, n_img=100, flags=_lib.NCX_F_ALL)
    din = 3 * 16 + 2 * 36 + 2 * 8 + 8 + 24 + 1
    n_emb = 68 * 36
    sizes = (("w1", 32 * din), ("b1", 32), ("w_out", 32), ("b_out", 4))
    n = n_emb + sum(s for _, s in sizes)
    bases = dict(param=0x10000000, grad=0x20000000, exp_avg=0x30000000, exp_avg_sq=0x40000000)
    p, g = _lib.NcxParams(), _lib.NcxGrads()
    for s, base in ((p, bases["param"]), (g, bases["grad"])):
        s.answer_embedding = base
        off = n_emb
        for name, cnt in sizes:
            setattr(s, name, base + 4 * off)
            off += cnt
    st = _lib.NcxAdamState(bases["param"], bases["grad"], bases["exp_avg"], bases["exp_avg_sq"], n, n_emb, 1, 1e-4, 0.9, 0.999, 1e-8, 1.0)
    return d, p, g, st, n, n_emb


def test_symbol_and_struct_layout():
    from neuralcx import _lib
    assert "ncx_backward_adam" in _lib.EXPORTS and hasattr(C.CDLL(_lib.LIB_PATH), "ncx_backward_adam")
    assert C.sizeof(_lib.NcxAdamState) == 72                # 4 pointers, 2 size_t, int32 + 5 floats


def test_null_arguments_are_ncx_e_null():
    d, p, g, st, n, n_emb = _consistent()
    assert _call(d, p, g, None) == -1
    assert _call(d, None, g, st) == -1 and _call(d, p, None, st) == -1 and _call(d, p, g, st, in_ok=False) == -1
    for f in ("param", "grad", "exp_avg", "exp_avg_sq"):
        d, p, g, st, n, n_emb = _consistent()
        setattr(st, f, None)
        assert _call(d, p, g, st) == -1, f


def test_inconsistent_state_is_ncx_e_dims():
    d, p, g, st, n, n_emb = _consistent()
    st.n_emb = n + 4
    assert _call(d, p, g, st) == -2                       # n_emb > n
    d, p, g, st, n, n_emb = _consistent()
    st.n_emb = n_emb - 4
    assert _call(d, p, g, st) == -2                       # the embedding does not fit its slice
    d, p, g, st, n, n_emb = _consistent()
    st.step = 0
    assert _call(d, p, g, st) == -2
    d, p, g, st, n, n_emb = _consistent()
    st.n = 0
    assert _call(d, p, g, st) == -2
    d, p, g, st, n, n_emb = _consistent()
    p.answer_embedding = st.param + 16
    assert _call(d, p, g, st) == -2                       # params->answer_embedding != param
    d, p, g, st, n, n_emb = _consistent()
    g.answer_embedding = st.grad + 16
    assert _call(d, p, g, st) == -2
    d, p, g, st, n, n_emb = _consistent()
    p.b_out = st.param + 4 * n                            # one past the end of the flat buffer
    assert _call(d, p, g, st) == -2
    d, p, g, st, n, n_emb = _consistent()
    g.w1 = st.exp_avg + 4 * n_emb                         # a gradient tensor in another buffer
    assert _call(d, p, g, st) == -2
    d, p, g, st, n, n_emb = _consistent()
    p.w1 = st.param                                       # inside the embedding slice
    assert _call(d, p, g, st) == -2
    bad = type(d)(B=0, K=24, dv=1, dq=1, dz=1, da=1, A=1, H=1, L=1, n_img=1)
    assert _call(bad, p, g, st) == -2


def test_misaligned_buffer_is_ncx_e_workspace():
    d, p, g, st, n, n_emb = _consistent()
    st.exp_avg = st.exp_avg + 4
    assert _call(d, p, g, st) == -3
