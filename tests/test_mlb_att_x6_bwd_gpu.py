"""GPU: the X6 ("bf16 x 6", NCX_F_X6) form of the MLB attention model's weight-gradient kernel (k_att_dwv_x6, d conv_v_att.weight
= sum over b, p of dXv V) against the fp64 restatement of the step and against the fp32 MFMA kernel.  Tolerances are the suite's
own: `compare` of tests/test_mlb_att_train_gpu.py against fp64 (1e-4 of each gradient's max, the conv_att.bias noise bound), 1e-5
of the tensor's max between the two forms, and err_x6 <= 1.5 err_fp32 + 1e-7 max(1, max|ref|) for "fp32-grade".  Every parity input
has PEAKED attention under its own masks (train_case asserts it on fp64)."""
import numpy as np
import pytest
import torch

import mlb_att_train_ref as TR
from test_mlb_att_cpu import YAML, _cli
from test_mlb_att_gpu import module_on_gpu, weights_of
from test_mlb_att_train_gpu import EDGE, FIELDS, HALF, compare, ref_of, t_dev, train_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
P4 = (2, 36, 48, 70, 2, 24, 40, 2, 2)               # P = 4: a ragged step only
PAST128 = (3, 132, 20, 130, 2, 12, 9, 2, 2)         # dv one 4-element window past 128 channels, dh_att past 128
PAST_TILE = (3, 132, 20, 164, 2, 12, 9, 2, 2)       # the kernel's tile is 160 hidden x 128 channels: dh_att one window past 160
FULL = (8, 2048, 2400, 1200, 4, 1200, 2000, 14, 14)
NO_DROP = (0.0,) * 6


def step(st, table, q, target, mode, p, masks, fwd_x6, bwd_x6, img_idx=None, seed=0, ws=None, poison=False):
    """forward (x6 = fwd_x6) + ncx_ce_loss + backward (x6 = bwd_x6) through the ops -> what hip_step returns."""
    from neuralcx import ops
    mw = weights_of(st)
    B, P = q.shape[0], int(np.prod(table.shape[2:]))
    idx = np.arange(B, dtype=np.int32) if img_idx is None else np.asarray(img_idx, np.int32)
    dt = ops.mlb_att_train_dims(mw, B, P, table.shape[0], p=p, dropout_mode=mode, seed=seed, want_dq=True)
    if ws is None:
        ws = ops.mlb_att_train_workspace(dt, mw, torch.device(DEV))
    if poison:
        ws.view(torch.float32).fill_(float("nan"))
    mk = None if masks is None else t_dev(TR.concat_masks(masks))
    feats, idx_d, q_d = t_dev(table), t_dev(idx), t_dev(q)
    logits, att = ops.mlb_att_train_forward(dt, feats, idx_d, q_d, mw, ws, masks=mk, x6=fwd_x6)
    r = ops.ce_loss(logits, t_dev(np.asarray(target, np.int32)))
    grads = {k: torch.full_like(v, float("nan")) for k, v in mw.t.items()}
    dq = ops.mlb_att_train_backward(dt, feats, idx_d, q_d, mw, ws, att, r["dlogits"], grads, masks=mk, x6=bwd_x6)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu().numpy(), att=att.cpu().numpy(), loss=float(r["loss"].cpu()), grads={k: v.cpu().numpy() for k, v in grads.items()},
                dq=dq.cpu().numpy(), dt=dt, mw=mw, ws=ws, t_grads=grads, t_logits=logits, t_att=att, t_dq=dq)


def dwv_form(st, shape, x6):
    from neuralcx import ops
    return ops.mlb_att_dwv_form(weights_of(st), shape[0], shape[7] * shape[8], shape[0], x6=x6)


# ---- 1. edge shapes against fp64 under X6 ------------------------------------------------------------------------------------------
CASES = [(s, 2) for s in (EDGE[0], EDGE[1], EDGE[2], EDGE[5], P4, PAST128, PAST_TILE)] + [(EDGE[0], 0), (EDGE[1], 0)]


@pytest.mark.parametrize("shape,mode", CASES, ids=lambda v: "x".join(map(str, v)) if isinstance(v, tuple) else "mode%d" % v)
def test_edge_shapes_vs_fp64_under_x6(shape, mode):
    from neuralcx import ops
    p = HALF if mode == 2 else NO_DROP
    gather = shape[0] == 13
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), mode, p, None, gather)
    assert dwv_form(st, shape, True) == "x6" and dwv_form(st, shape, False) == "fp32"
    h = step(st, table, q, target, mode, p, masks, True, True, img_idx=idx)
    compare(h, ref_of(r, shape[4]), "x6 step %s mode %d" % (shape, mode), ba32=ba32)
    vd = ops.mlb_att_train_ws_region(h["dt"], h["mw"], h["ws"], ops.AT_WS_VD)
    assert vd.numel() == (shape[0] * shape[1] * shape[7] * shape[8] if mode == 2 else 0)       # mode 0: the table is read in place
    if gather:
        slab = ops.mlb_att_train_ws_region(h["dt"], h["mw"], h["ws"], ops.AT_WS_DWV)
        S = slab.numel() // (shape[3] * shape[1])
        ipg = -(-shape[0] // S)
        assert S > 1 and slab.numel() == S * shape[3] * shape[1] and shape[0] % ipg != 0, (S, ipg)      # the last group is shorter
        assert len(set(idx.tolist())) < shape[0]


@pytest.mark.parametrize("shape", [EDGE[3], EDGE[4]], ids=["P2", "P1"])
def test_small_maps_stay_on_the_small_kernel(shape):
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 2, HALF, None, False)
    assert dwv_form(st, shape, True) == dwv_form(st, shape, False) == "small"
    h6 = step(st, table, q, target, 2, HALF, masks, True, True)
    h32 = step(st, table, q, target, 2, HALF, masks, True, False)
    compare(h6, ref_of(r, shape[4]), "x6 step %s" % (shape,), ba32=ba32)
    assert torch.equal(h6["t_grads"]["wv_att"], h32["t_grads"]["wv_att"])


# ---- 2. the flag switches kernels and agrees with the fp32 kernel ------------------------------------------------------------------
@pytest.mark.parametrize("shape", [EDGE[0], EDGE[1]], ids=["P35", "P196"])
def test_flag_switches_kernels_and_agrees_with_fp32(shape):
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 2, HALF, None, False)
    h32 = step(st, table, q, target, 2, HALF, masks, False, False)
    h6 = step(st, table, q, target, 2, HALF, masks, False, True)
    a, b = h6["grads"]["wv_att"].astype(np.float64), h32["grads"]["wv_att"].astype(np.float64)
    err, mx = float(np.abs(a - b).max()), float(np.abs(b).max())
    print("x6 vs fp32 %s d wv_att: max diff %.3e, max %.3e" % (shape, err, mx))
    assert not torch.equal(h6["t_grads"]["wv_att"], h32["t_grads"]["wv_att"])                   # two kernels, two summation orders
    assert np.isfinite(err) and err <= 1e-5 * mx, (err, mx)
    for k in FIELDS:                                                                            # only this product changes
        if k != "wv_att":
            assert torch.equal(h6["t_grads"][k], h32["t_grads"][k]), k
    assert torch.equal(h6["t_dq"], h32["t_dq"]) and torch.equal(h6["t_logits"], h32["t_logits"])


# ---- 3. / 4. what "fp32-grade" means -----------------------------------------------------------------------------------------------
def fp32_grade(g32, g6, ref, what):
    """The fp32 form within 1e-4 max|ref| of fp64, asserted first (the case must be fair to it); then the X6 form within the same,
    and no farther from fp64 than 1.5 x the fp32 form + 1e-7 max(1, max|ref|)."""
    ref = np.asarray(ref, np.float64)
    e32, e6, mx = float(np.abs(g32 - ref).max()), float(np.abs(g6 - ref).max()), float(np.abs(ref).max())
    print("%s d wv_att: err fp32 %.3e, err x6 %.3e, max|ref| %.3e" % (what, e32, e6, mx))
    assert np.isfinite(g32).all() and e32 <= 1e-4 * mx, (what, "fp32 form", e32, mx)
    assert np.isfinite(g6).all() and e6 <= 1e-4 * mx, (what, "x6 form", e6, mx)
    assert e6 <= 1.5 * e32 + 1e-7 * max(1.0, mx), (what, e32, e6, mx)


def test_full_widths_are_fp32_grade():
    seed = 0x0123456789ABCDEF
    st, table, q, target, idx, masks, r, ba32 = train_case(54, FULL, (), 1, HALF, seed)
    assert dwv_form(st, FULL, True) == "x6"
    h32 = step(st, table, q, target, 1, HALF, None, False, False, seed=seed)
    compare(h32, ref_of(r, 4), "full widths, fp32 backward", ba32=ba32)
    h6 = step(st, table, q, target, 1, HALF, None, False, True, seed=seed, ws=h32["ws"])
    compare(h6, ref_of(r, 4), "full widths, x6 backward", ba32=ba32)
    fp32_grade(h32["grads"]["wv_att"], h6["grads"]["wv_att"], ref_of(r, 4)["grads"]["wv_att"], "full widths")


def test_mixed_magnitudes_are_fp32_grade():
    """Channel c of the table scaled by 2^((7 c) % 25 - 12), column c of conv_v_att.weight and of every glimpse Linear by the inverse:
    exact in fp32, so the step is the unscaled one and the fp64 d conv_v_att.weight[:, c] is the unscaled column times that power of
    two, while the planes of the cut hold 25 different exponents side by side.  Column c divided by its scale (exact) is compared
    with the unscaled fp64 reference."""
    shape = EDGE[1]
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 2, HALF, None, False)
    s = (2.0 ** ((7 * np.arange(shape[1])) % 25 - 12)).astype(np.float32)
    st2 = dict(st)
    st2["conv_v_att.weight"] = (st["conv_v_att.weight"] / s[None, :, None, None]).astype(np.float32)
    for g in range(shape[4]):
        st2["list_linear_v_fusion.%d.weight" % g] = (st["list_linear_v_fusion.%d.weight" % g] / s[None, :]).astype(np.float32)
    table2 = (table * s[None, :, None, None]).astype(np.float32)
    assert np.array_equal(st2["conv_v_att.weight"] * s[None, :, None, None], st["conv_v_att.weight"]) and np.array_equal(table2 / s[None, :, None, None], table)
    for g in range(shape[4]):
        assert np.array_equal(st2["list_linear_v_fusion.%d.weight" % g] * s[None, :], st["list_linear_v_fusion.%d.weight" % g])
    ref = np.asarray(ref_of(r, shape[4])["grads"]["wv_att"], np.float64)
    r2 = TR.step(st2, table2, q, target, {}, masks, HALF)                                   # the scaled step in fp64: the same step
    ref2 = np.asarray(ref_of(r2, shape[4])["grads"]["wv_att"], np.float64) / s[None, :].astype(np.float64)
    assert np.abs(r2["logits"] - r["logits"]).max() <= 1e-9 * max(1.0, np.abs(r["logits"]).max())
    assert np.abs(ref2 - ref).max() <= 1e-9 * np.abs(ref).max()
    h32 = step(st2, table2, q, target, 2, HALF, masks, False, False)
    h6 = step(st2, table2, q, target, 2, HALF, masks, False, True)
    un = lambda h: h["grads"]["wv_att"].astype(np.float64) / s[None, :].astype(np.float64)
    fp32_grade(un(h32), un(h6), ref, "mixed magnitudes")


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------
def test_x6_backwards_are_bit_identical_and_ignore_stale_buffers():
    shape = EDGE[5]
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 2, HALF, None, True)
    a = step(st, table, q, target, 2, HALF, masks, True, True, img_idx=idx)
    b = step(st, table, q, target, 2, HALF, masks, True, True, img_idx=idx)
    c = step(st, table, q, target, 2, HALF, masks, True, True, img_idx=idx, ws=a["ws"], poison=True)    # NaN-filled workspace and gradient buffers
    for other in (b, c):
        assert torch.equal(a["t_logits"], other["t_logits"]) and torch.equal(a["t_dq"], other["t_dq"])
        for k in FIELDS:
            assert torch.isfinite(other["t_grads"][k]).all() and torch.equal(a["t_grads"][k], other["t_grads"][k]), k


# ---- 6. the module and the command line ---------------------------------------------------------------------------------------------
def test_module_hands_hip_x6_to_the_backward(monkeypatch):
    from neuralcx import _lib, ops
    shape = (13, 96, 48, 44, 2, 28, 52, 5, 7)
    import mlb_att_ref as R
    st, maps, q, ref = R.peaked_case(31, *shape)
    v = t_dev(maps)
    target = torch.randint(0, shape[6], (shape[0],), generator=torch.Generator().manual_seed(4)).to(DEV)
    seen = []
    real = ops.mlb_att_train_backward

    def spy(*a, **k):
        out = real(*a, **k)
        seen.append((k.get("x6", "absent"), a[8]))
        return out

    monkeypatch.setattr(ops, "mlb_att_train_backward", spy)
    for flag, extra in ((True, 0), (False, _lib.NCX_F_X6)):
        monkeypatch.setattr(ops, "EXTRA_FLAGS", extra)
        m = module_on_gpu(st, shape).train()
        m.use_hip_train, m.hip_x6 = True, flag
        qd = t_dev(q).requires_grad_(True)
        loss = torch.nn.functional.cross_entropy(m.forward_from_q(v, qd), target.long())
        loss.backward()
        assert len(seen) == 1 and seen[0][0] is flag, seen
        g = seen.pop()[1]
        lin = list(m.list_linear_v_fusion)
        pairs = [("wv_att", m.conv_v_att.weight.grad.flatten(1)), ("bv_att", m.conv_v_att.bias.grad), ("wq_att", m.linear_q_att.weight.grad),
                 ("bq_att", m.linear_q_att.bias.grad), ("wa", m.conv_att.weight.grad.flatten(1)), ("ba", m.conv_att.bias.grad),
                 ("wg", torch.stack([l.weight.grad for l in lin])), ("bg", torch.stack([l.bias.grad for l in lin])),
                 ("wqf", m.linear_q_fusion.weight.grad), ("bqf", m.linear_q_fusion.bias.grad), ("wc", m.linear_classif.weight.grad),
                 ("bc", m.linear_classif.bias.grad)]
        assert [k for k, _ in pairs] == list(FIELDS)
        for k, got in pairs:
            assert torch.isfinite(got).all() and torch.equal(got.reshape(g[k].shape), g[k]), (flag, k)
        assert qd.grad is not None and torch.isfinite(qd.grad).all()


def test_train_cli_x6_with_hip_att_train_finishes(tmp_path, capsys):
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
    real = ops.mlb_att_train_backward
    ops.mlb_att_train_backward = lambda *a, **k: (seen.append(k.get("x6")), real(*a, **k))[1]
    try:
        out = _cli("train.py").main(["--path_opt", str(path), "--synthetic", "--x6", "--hip_att_train", "--epochs", "1", "--syn_examples", "36",
                                     "--syn_images", "64", "--syn_vocab", "30", "--syn_grid", "5", "--print_freq", "0"])
    finally:
        ops.mlb_att_train_backward = real
    text = capsys.readouterr().out
    assert "attention head, glimpse fusion and classifier train in HIP" in text and "(bf16 x 6 attention kernel)" in text
    assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["train"]["loss"]) and np.isfinite(out["history"][0]["val"]["loss"])
    assert seen and all(x is True for x in seen) and out["trainer"].model.hip_x6 is True and out["trainer"].model.use_hip_train is True
