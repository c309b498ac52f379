"""GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the MLB attention model's conv_v_att kernel (k_att_logits_x6) against the fp64
restatement and against the fp32 MFMA kernels.  Tolerances are the suite's own: 1e-4 max|ref| per tensor against fp64 (`check` of
tests/test_mlb_att_gpu.py), 1e-5 of each tensor's max between the two forms (tests/test_hip_parity.py::test_x6_*), and
err_x6 <= 1.5 err_fp32 + 1e-7 max(1, max|ref|) for "fp32-grade" (test_x6_logits_are_as_close_to_fp64_as_the_fp32_kernels): the
bound that tells six plane products from three.  Every parity input has PEAKED attention, asserted on its fp64 reference first."""
import numpy as np
import pytest
import torch

import mlb_att_ref as R
import mlb_att_train_ref as TR
from test_mlb_att_cpu import YAML, _cli
from test_mlb_att_gpu import RAGGED, case, check, module_on_gpu, weights_of
from test_mlb_att_train_gpu import EDGE, HALF, compare, ref_of, t_dev, train_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P4 = (2, 36, 48, 70, 2, 24, 40, 2, 2)               # P = 4, dv one past a 32-step, dh_att one past a 64-tile
FULL = (8, 2048, 2400, 1200, 4, 1200, 2000, 14, 14)


def run(st, maps, q, x6, ws=None):
    from neuralcx import ops
    return ops.mlb_att_forward(t_dev(maps), None, t_dev(q), weights_of(st), ws=ws, x6=x6)


def form(shape, x6):
    from neuralcx import ops
    st = case(31, shape)[0] if shape != FULL else case(33, shape)[0]
    return ops.mlb_att_logits_form(weights_of(st), shape[0], shape[7] * shape[8], shape[0], x6=x6)


def rel_to_max(a, b):
    a, b = a.detach().cpu().numpy().astype(np.float64), b.detach().cpu().numpy().astype(np.float64)
    return float(np.abs(a - b).max()), float(np.abs(b).max())


# ---- 1. ragged shapes against fp64 under X6 ----------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", RAGGED + [P4], ids=lambda s: "x".join(map(str, s)))
def test_ragged_shapes_vs_fp64_under_x6(shape):
    st, maps, q, ref = case(31, shape)
    logits, att = run(st, maps, q, True)
    check(logits, att, ref[0], ref[1], 0.0, "x6 ragged %s" % (shape,))
    if shape[-1] * shape[-2] == 1:                  # P = 1: both flags take the small kernel
        assert form(shape, True) == form(shape, False) == "small"
        l0, a0 = run(st, maps, q, False)
        assert torch.equal(logits, l0) and torch.equal(att, a0)
    else:
        assert form(shape, True) in ("x6_64", "x6_208")


# ---- 2. the flag switches kernels and agrees with the fp32 kernels -----------------------------------------------------------------
@pytest.mark.parametrize("shape", RAGGED[1:], ids=lambda s: "x".join(map(str, s)))
def test_flag_switches_kernels_and_agrees_with_fp32(shape):
    st, maps, q, ref = case(31, shape)
    f6, f32 = form(shape, True), form(shape, False)
    assert f6 != f32 and f6.startswith("x6_") and f32.startswith("fp32_") and f6[3:] == f32[5:], (f6, f32)
    l6, a6 = run(st, maps, q, True)
    l32, a32 = run(st, maps, q, False)
    figs = [("logits",) + rel_to_max(l6, l32)] + [("att[%d]" % g,) + rel_to_max(a6[:, g], a32[:, g]) for g in range(shape[4])]
    for key, err, mx in figs:
        print("x6 vs fp32 %s %s: max diff %.3e, max %.3e" % (shape, key, err, mx))
    for key, err, mx in figs:
        assert err <= 1e-5 * mx, (key, err, mx)


# ---- 3. / 4. what "fp32-grade" means -----------------------------------------------------------------------------------------------
def fp32_grade(st, maps, q, ref, what):
    """Both forms within 1e-4 max|ref| of fp64; the X6 form no farther from fp64 than 1.5 x the fp32 form + 1e-7 max(1, max|ref|).
    The fp32 form is asserted first: the case must be fair to it."""
    l32, a32 = run(st, maps, q, False)
    l6, a6 = run(st, maps, q, True)
    check(l32, a32, ref[0], ref[1], 0.0, what + ", fp32 form")
    check(l6, a6, ref[0], ref[1], 0.0, what + ", x6 form")
    figs = []
    for key, g32, g6, r in (("logits", l32, l6, ref[0]), ("maps", a32, a6, ref[1])):
        e32, e6, mx = float(np.abs(g32.cpu().numpy() - r).max()), float(np.abs(g6.cpu().numpy() - r).max()), float(np.abs(r).max())
        print("%s %s: err fp32 %.3e, err x6 %.3e, max|ref| %.3e" % (what, key, e32, e6, mx))
        figs.append((key, e32, e6, mx))
    for key, e32, e6, mx in figs:
        assert e6 <= 1.5 * e32 + 1e-7 * max(1.0, mx), (what, key, e32, e6, mx)


def test_full_widths_are_fp32_grade():
    st, maps, q, ref = case(33, FULL)
    assert form(FULL, True) == "x6_208"
    fp32_grade(st, maps, q, ref, "full widths")


def test_mixed_magnitudes_are_fp32_grade():
    """Channel c of every map scaled by 2^((7 c) % 25 - 12), column c of conv_v_att.weight by the inverse: exact in fp32, so the
    fp64 result is that of the unscaled case, while the planes of the cut hold 25 different exponents side by side.  The pooled map
    v_att = att . V carries the scale on into the glimpse Linears, so their column c takes the inverse as well: only then are the
    logits those of the unscaled case too.  (Without that, the glimpse Linears see channels up to 2^12 too large and the logits turn
    the 7.5e-7 difference of the maps into 6e-6 (fp32 form) and 1.3e-5 (X6 form): a figure about the fusion's conditioning, the
    same engine launches under both forms, and not about the attention kernel.)"""
    shape = RAGGED[3]
    st, maps, q, ref = case(31, shape)
    s = (2.0 ** ((7 * np.arange(shape[1])) % 25 - 12)).astype(np.float32)
    st2 = dict(st)
    st2["conv_v_att.weight"] = (st["conv_v_att.weight"] / s[None, :, None, None]).astype(np.float32)
    for g in range(shape[4]):
        st2["list_linear_v_fusion.%d.weight" % g] = (st["list_linear_v_fusion.%d.weight" % g] / s[None, :]).astype(np.float32)
    maps2 = (maps * s[None, :, None, None]).astype(np.float32)
    assert np.array_equal(st2["conv_v_att.weight"] * s[None, :, None, None], st["conv_v_att.weight"]) and np.array_equal(maps2 / s[None, :, None, None], maps)
    ref2 = R.mlb_att_forward(st2, maps2, q, want_logits=True)
    assert R.peaked(ref2[2], ref2[1])
    for a, b in zip(ref2, ref):                     # logits, maps, position logits: the unscaled case's, to fp64 rounding
        assert np.abs(a - b).max() <= 1e-9 * max(1.0, np.abs(b).max())
    fp32_grade(st2, maps2, q, ref2, "mixed magnitudes")


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [RAGGED[2], RAGGED[3]], ids=["64row", "208row"])
def test_x6_calls_are_bit_identical_and_ignore_a_stale_workspace(shape):
    from neuralcx import ops
    st, maps, q, ref = case(31, shape)
    ws = ops.mlb_att_workspace(weights_of(st), shape[0], shape[7] * shape[8], shape[0], torch.device(DEV))
    l0, a0 = run(st, maps, q, True, ws=ws)
    l1, a1 = run(st, maps, q, True, ws=ws)
    ws.view(torch.float32).fill_(float("nan"))
    l2, a2 = run(st, maps, q, True, ws=ws)
    assert torch.isfinite(l2).all() and torch.isfinite(a2).all()
    assert torch.equal(l0, l1) and torch.equal(a0, a1) and torch.equal(l0, l2) and torch.equal(a0, a2)


# ---- 6. the training forward --------------------------------------------------------------------------------------------------------
def train_step(st, table, q, target, masks, x6, backward):
    from neuralcx import ops
    mw = weights_of(st)
    B, P = q.shape[0], int(np.prod(table.shape[2:]))
    dt = ops.mlb_att_train_dims(mw, B, P, B, p=HALF, dropout_mode=2, want_dq=True)
    ws = ops.mlb_att_train_workspace(dt, mw, torch.device(DEV))
    ws.view(torch.float32).fill_(float("nan"))
    mk = t_dev(TR.concat_masks(masks))
    feats, idx, q_d = t_dev(table), t_dev(np.arange(B, dtype=np.int32)), t_dev(q)
    logits, att = ops.mlb_att_train_forward(dt, feats, idx, q_d, mw, ws, masks=mk, x6=x6)
    out = dict(t_logits=logits, t_att=att, xv=ops.mlb_att_train_ws_region(dt, mw, ws, ops.AT_WS_XV).clone())
    if backward:
        r = ops.ce_loss(logits, t_dev(np.asarray(target, np.int32)))
        grads = {k: torch.full_like(v, float("nan")) for k, v in mw.t.items()}
        dq = ops.mlb_att_train_backward(dt, feats, idx, q_d, mw, ws, att, r["dlogits"], grads, masks=mk)
        torch.cuda.synchronize()
        out.update(logits=logits.cpu().numpy(), att=att.cpu().numpy(), loss=float(r["loss"].cpu()),
                   grads={k: v.cpu().numpy() for k, v in grads.items()}, dq=dq.cpu().numpy())
    return out


@pytest.mark.parametrize("shape", [EDGE[0], EDGE[1]], ids=["64row", "208row"])
def test_training_forward_under_x6_and_the_unchanged_backward(shape):
    from neuralcx import ops
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 2, HALF, None, False)
    mw = weights_of(st)
    assert ops.mlb_att_logits_form(mw, shape[0], shape[7] * shape[8], shape[0], x6=True) == ("x6_208" if shape is EDGE[1] else "x6_64")
    h32 = train_step(st, table, q, target, masks, False, False)
    h6 = train_step(st, table, q, target, masks, True, True)
    figs = [(key,) + rel_to_max(h6[key], h32[key]) for key in ("xv", "t_logits", "t_att")]
    for key, err, mx in figs:
        print("x6 vs fp32 training forward %s %s: max diff %.3e, max %.3e" % (shape, key, err, mx))
    for key, err, mx in figs:
        assert np.isfinite(err) and err <= 1e-5 * mx, (key, err, mx)
    compare(h6, ref_of(r, shape[4]), "x6 forward + backward %s" % (shape,), ba32=ba32)


# ---- 7. the module and the command line ---------------------------------------------------------------------------------------------
def test_module_with_hip_x6_returns_the_ops_tensors(monkeypatch):
    from neuralcx import _lib, ops
    shape = RAGGED[3]
    st, maps, q, ref = case(31, shape)
    m = module_on_gpu(st, shape)
    v, qd = t_dev(maps), t_dev(q)
    want6, want32 = run(st, maps, q, True), run(st, maps, q, False)
    assert not torch.equal(want6[0], want32[0])                            # two kernels, two summation orders
    monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    for flag, want in ((True, want6), (False, want32), (None, want32)):
        m.hip_x6 = flag
        with torch.no_grad():
            logits = m.forward_from_q(v, qd)
        assert torch.equal(logits, want[0]) and torch.equal(torch.stack(m.list_att, 1), want[1]), flag
    monkeypatch.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6)                 # None follows the process-wide flag, read at call time
    with torch.no_grad():
        logits = m.forward_from_q(v, qd)
    assert torch.equal(logits, want6[0])
    m.hip_x6, m.use_hip = True, False                                      # no routing decision changes: the torch path stays the torch path
    calls = []
    real = ops.mlb_att_forward
    monkeypatch.setattr(ops, "mlb_att_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        m.forward_from_q(v, qd)
    assert not calls


def test_train_cli_x6_prints_the_route_and_finishes(tmp_path, capsys):
    import yaml
    with open(YAML) as f:
        opt = yaml.safe_load(f)
    mo = opt["model"]
    mo["dim_v"], mo["dim_q"], mo["seq2vec"]["emb_size"] = 64, 48, 16
    mo["attention"].update(dim_h=32, nb_glimpses=2)
    mo["fusion"]["dim_h"] = 24
    opt["vqa"].update(nans=20, maxlength=6)
    opt["optim"].update(batch_size=16, epochs=1)
    opt["logs"]["dir_logs"] = str(tmp_path / "logs")
    path = tmp_path / "tiny.yaml"
    path.write_text(yaml.safe_dump(opt))
    from neuralcx import ops
    seen = []
    real = ops.mlb_att_forward
    ops.mlb_att_forward = lambda *a, **k: (seen.append(k.get("x6")), real(*a, **k))[1]
    try:
        out = _cli("train.py").main(["--path_opt", str(path), "--synthetic", "--x6", "--epochs", "1", "--syn_examples", "36", "--syn_images", "64",
                                     "--syn_vocab", "30", "--syn_grid", "5", "--print_freq", "0"])
    finally:
        ops.mlb_att_forward = real
    text = capsys.readouterr().out
    assert "eval-mode forward in HIP (ncx_mlb_att_forward) (bf16 x 6 attention kernel)" in text
    assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["val"]["loss"])
    assert seen and all(x is True for x in seen) and out["trainer"].model.hip_x6 is True
