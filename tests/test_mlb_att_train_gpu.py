"""GPU: the HIP training step of the MLB attention model (ncx_mlb_att_train_forward / _backward, MlbAttTrainFunction, the module
route, train.py --hip_att_train) against the reference fixture g22, the fp64 restatement (tests/mlb_att_train_ref.py) and the
module's torch path.  Tolerances are the project's: logits and maps 1e-4 max|ref| against fp64 (1e-4 max(1, max|ref|) against the
fixture and torch), loss 1e-5 max(1, |ref|), every gradient and dq_emb helpers.grad_tol (1e-4 of the tensor's max).  One tensor has
no scale of its own: d conv_att.bias = sum_p ds is zero in mathematics (the softmax is shift-invariant), so every implementation
holds rounding noise there; its bound is twice the error of the fp32 torch path against fp64 on the same input.
Every parity input has PEAKED attention, asserted on the fp64 reference of the step itself before anything is compared."""
import functools

import numpy as np
import pytest
import torch

import mlb_att_ref as R
import mlb_att_train_ref as TR
import trainer_edge_cases as E
from helpers import grad_tol
from test_mlb_att_cpu import YAML, _cli
from test_mlb_att_gpu import ACT_FIELD, module_on_gpu, weights_of
from test_mlb_att_train_cpu import ZERO_IN_MATHS, load_train_case, masks_for_module, module_for, noise_bound, torch_step_with_masks

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
HALF = (0.5,) * 6
FIELDS = ("wv_att", "bv_att", "wq_att", "bq_att", "wa", "ba", "wg", "bg", "wqf", "bqf", "wc", "bc")


def t_dev(a):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV)


def hip_step(st, table, q, target, acts=(), mode=0, p=(0.0,) * 6, masks=None, seed=0, want_dq=True, img_idx=None, ws=None, poison=False):
    """forward + ncx_ce_loss + backward through the ops -> dict(logits, att, loss, grads {field: array}, dq, dt, mw, ws)."""
    from neuralcx import ops
    mw = weights_of(st, dict(acts))
    B = q.shape[0]
    P = int(np.prod(table.shape[2:]))
    idx = np.arange(B, dtype=np.int32) if img_idx is None else np.asarray(img_idx, np.int32)
    dt = ops.mlb_att_train_dims(mw, B, P, table.shape[0], p=p, dropout_mode=mode, seed=seed, want_dq=want_dq)
    if ws is None:
        ws = ops.mlb_att_train_workspace(dt, mw, torch.device(DEV))
    if poison:
        ws.view(torch.float32).fill_(float("nan"))
    mk = None if masks is None else t_dev(TR.concat_masks(masks))
    feats, idx_d, q_d = t_dev(table), t_dev(idx), t_dev(q)
    logits, att = ops.mlb_att_train_forward(dt, feats, idx_d, q_d, mw, ws, masks=mk)
    r = ops.ce_loss(logits, t_dev(np.asarray(target, np.int32)))
    grads = {k: torch.full_like(v, float("nan")) for k, v in mw.t.items()}
    dq = ops.mlb_att_train_backward(dt, feats, idx_d, q_d, mw, ws, att, r["dlogits"], grads, masks=mk)
    torch.cuda.synchronize()
    return dict(logits=logits.cpu().numpy(), att=att.cpu().numpy(), loss=float(r["loss"].cpu()), grads={k: v.cpu().numpy() for k, v in grads.items()},
                dq=None if dq is None else dq.cpu().numpy(), dt=dt, mw=mw, ws=ws, t_grads=grads, t_logits=logits, t_att=att, t_dq=dq)


def compare(h, ref, what, floor=0.0, ba32=None, want_dq=True):
    """h: hip_step's result; ref: dict(logits, att, loss, grads by field, dq_emb).  Prints every figure, then asserts all of them."""
    figs = []
    for key in ("logits", "att"):
        err, mx = float(np.abs(h[key] - ref[key]).max()), float(np.abs(ref[key]).max())
        figs.append((key, err, 1e-4 * max(floor, mx), bool(np.isfinite(h[key]).all())))
    figs.append(("loss", abs(h["loss"] - ref["loss"]), 1e-5 * max(1.0, abs(ref["loss"])), bool(np.isfinite(h["loss"]))))
    assert set(h["grads"]) == set(ref["grads"]) == set(FIELDS)                 # no test may skip a tensor
    for k in FIELDS:
        g, rg = h["grads"][k], np.asarray(ref["grads"][k])
        assert g.shape == rg.shape, (what, k, g.shape, rg.shape)
        tol = noise_bound("conv_att.bias", rg, ba32) if k == "ba" else grad_tol(k, rg)
        figs.append(("d " + k, float(np.abs(g - rg).max()), tol, bool(np.isfinite(g).all())))
    if want_dq:
        figs.append(("dq_emb", float(np.abs(h["dq"] - ref["dq_emb"]).max()), grad_tol("q_emb", ref["dq_emb"]), bool(np.isfinite(h["dq"]).all())))
    else:
        assert h["dq"] is None
    for key, err, tol, fin in figs:
        print("%s %s: max err %.3e, bound %.3e" % (what, key, err, tol))
    for key, err, tol, fin in figs:
        assert fin and err <= tol, (what, key, err, tol)


def ref_of(r, G):
    return dict(logits=r["logits"], att=r["att"], loss=r["loss"], grads=TR.grads_by_field(r["grads"], G), dq_emb=r["dq_emb"])


@functools.lru_cache(maxsize=None)
def train_case(seed, shape, acts=(), mode=0, p=(0.0,) * 6, gen_seed=None, gather=False):
    """A seeded step whose attention is peaked UNDER ITS MASKS: mlb_att_ref.peaked_case, then conv_att.weight doubled until the fp64
    step's own position logits are peaked (dropout rescales them).  Computed once per session, never modified.
    -> (state, table, q, target, img_idx or None, masks or None, fp64 step, d conv_att.bias of the fp32 torch path)"""
    B, dv, dq, dh_att, G, dh_f, A, W, H = shape
    st, maps, q, _ = R.peaked_case(seed, *shape, acts=dict(acts))
    rng = np.random.default_rng(seed + 1000)
    target = rng.integers(0, A, size=B)
    masks = None
    if mode == 2:
        masks = TR.random_masks(rng, p, B, W * H, dv, dq, dh_att, G, dh_f)
    elif mode == 1:
        masks = TR.generator_masks(gen_seed, p, B, W * H, dv, dq, dh_att, G, dh_f)
    table, idx, dense = maps, None, maps
    if gather:                                   # a table with repeated, non-identity indices
        idx = rng.integers(0, B, size=B).astype(np.int32)
        idx[1] = idx[0]
        assert not np.array_equal(idx, np.arange(B)) and len(set(idx.tolist())) < B
        dense = np.ascontiguousarray(maps[idx])
    st = dict(st)
    for _ in range(8):
        r = TR.step(st, dense, q, target, dict(acts), masks, p)
        if W * H == 1 or R.peaked(r["pos"], r["att"]):
            break
        st["conv_att.weight"] = (st["conv_att.weight"] * np.float32(2.0)).astype(np.float32)
    assert W * H == 1 or R.peaked(r["pos"], r["att"]), "every parity input must have peaked attention"
    mm = masks if masks is not None else [np.ones(s, np.float32) for s in TR.mask_shapes(B, W * H, dv, dq, dh_att, G, dh_f)]
    g32 = torch_step_with_masks(module_for(st, shape, acts), dense, q, target, masks_for_module(mm, shape), p, torch.float32)[3]
    return st, table, q, target, idx, masks, r, g32[ZERO_IN_MATHS]


# ---- 1. the reference fixture ------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", ["c0", "c1"])
def test_hip_step_vs_golden(name):
    c = load_train_case(name)
    G = int(c["dims"][3])
    r64 = TR.step(c["state"], c["maps"], c["q_emb"], c["target"], c["acts"])
    assert R.peaked(r64["pos"], r64["att"])
    h = hip_step(c["state"], c["table"], c["q_emb"], c["target"], tuple(c["acts"].items()), img_idx=c["img_idx"])
    ref = dict(logits=c["logits"], att=c["att"], loss=float(c["loss"]), grads=TR.grads_by_field(c["grads"], G), dq_emb=c["grad_q_emb"])
    # d conv_att.bias: the fixture's own value is the fp32 reference's rounding noise around zero, so that tensor is compared with
    # the fp64 restatement, and the fixture's distance from it sets the bound (twice that)
    ref["grads"]["ba"] = r64["grads"][ZERO_IN_MATHS]
    compare(h, ref, "golden " + name, floor=1.0, ba32=c["grads"][ZERO_IN_MATHS])
    assert np.array_equal(h["att"][2], np.full_like(h["att"][2], h["att"][2, 0, 0]))          # the all-zero image: exactly uniform


# ---- 2. fp64 parity on edge shapes -------------------------------------------------------------------------------------------------
EDGE = E.ATT_EDGE


@pytest.mark.parametrize("mode", [0, 2], ids=["mode0", "mode2_p0.5"])
@pytest.mark.parametrize("shape", EDGE, ids=lambda s: "x".join(map(str, s)))
def test_edge_shapes_vs_fp64(shape, mode):
    from neuralcx import ops
    p = HALF if mode == 2 else (0.0,) * 6
    gather = shape[0] == 13
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), mode, p, None, gather)
    G = shape[4]
    h = hip_step(st, table, q, target, (), mode, p, masks, want_dq=True, img_idx=idx)
    compare(h, ref_of(r, G), "edge %s mode %d" % (shape, mode), ba32=ba32)
    h0 = hip_step(st, table, q, target, (), mode, p, masks, want_dq=False, img_idx=idx)
    compare(h0, ref_of(r, G), "edge %s mode %d, no dq" % (shape, mode), ba32=ba32, want_dq=False)
    # the stash regions the library documents
    dtf, mw, wsf = h["dt"], h["mw"], h["ws"]
    mk = None if masks is None else t_dev(TR.concat_masks(masks))            # a fresh forward: the backward overwrote Xv with dXv
    ops.mlb_att_train_forward(dtf, t_dev(table), t_dev(np.arange(shape[0], dtype=np.int32) if idx is None else idx), t_dev(q), mw, wsf, masks=mk)
    for which, key in ((ops.AT_WS_XV, "Xv"), (ops.AT_WS_VATT, "v_att"), (ops.AT_WS_T, "t")):
        got = ops.mlb_att_train_ws_region(dtf, mw, wsf, which).cpu().numpy().reshape(r[key].shape)
        err, mx = float(np.abs(got - r[key]).max()), float(np.abs(r[key]).max())
        print("stash %s: max err %.3e, max|ref| %.3e" % (key, err, mx))
        assert err <= 1e-4 * mx, (key, err, mx)
    vd = ops.mlb_att_train_ws_region(dtf, mw, wsf, ops.AT_WS_VD)
    assert vd.numel() == (shape[0] * shape[1] * shape[7] * shape[8] if mode == 2 else 0)
    if shape[-1] * shape[-2] == 1:
        for k in ("wv_att", "bv_att", "wq_att", "bq_att", "wa"):                            # one position: ds == 0 exactly
            assert not h["grads"][k].any(), k
        assert np.array_equal(h["att"], np.ones_like(h["att"]))
    if gather:
        slab = ops.mlb_att_train_ws_region(dtf, mw, wsf, ops.AT_WS_DWV)
        S = slab.numel() // (shape[3] * shape[1])
        ipg = -(-shape[0] // S)
        assert S > 1 and slab.numel() == S * shape[3] * shape[1] and shape[0] % ipg != 0, (S, ipg)      # the last group is shorter


# ---- 3. generator mode --------------------------------------------------------------------------------------------------------------
def test_generator_mode_with_the_yaml_dropouts():
    import yaml
    with open(YAML) as f:
        mo = yaml.safe_load(f)["model"]
    from neuralcx import ops
    p = ops.mlb_att_dropouts(mo)
    assert p == HALF
    shape, seed = (5, 64, 48, 32, 2, 24, 40, 5, 7), 0x9E3779B97F4A7C15
    st, table, q, target, idx, masks, r, ba32 = train_case(52, shape, (), 1, p, seed)
    assert all(0.3 < m.mean() < 0.7 for m in masks)
    h = hip_step(st, table, q, target, (), 1, p, None, seed=seed)
    compare(h, ref_of(r, shape[4]), "generator mode", ba32=ba32)
    other = hip_step(st, table, q, target, (), 1, p, None, seed=seed + 1)
    assert not np.array_equal(other["logits"], h["logits"])                                 # the seed matters


# ---- 4. one activation off at a time ------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("off", list(R.ACT_KEYS))
def test_one_activation_off(off):
    shape = (5, 64, 48, 32, 2, 24, 40, 5, 7)
    acts = ((off, None),)
    st, table, q, target, idx, masks, r, ba32 = train_case(53, shape, acts, 2, HALF, None, False)
    h = hip_step(st, table, q, target, acts, 2, HALF, masks)
    assert h["mw"].acts[ACT_FIELD[off]] == 0 and sum(h["mw"].acts.values()) == 10
    compare(h, ref_of(r, shape[4]), "activation %s off" % off, ba32=ba32)


# ---- 5. determinism -----------------------------------------------------------------------------------------------------------------
def test_bit_identical_calls_and_nan_filled_buffers():
    shape = (13, 40, 16, 48, 2, 8, 6, 3, 3)
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 2, HALF, None, True)
    a = hip_step(st, table, q, target, (), 2, HALF, masks, img_idx=idx)
    b = hip_step(st, table, q, target, (), 2, HALF, masks, img_idx=idx, ws=a["ws"], poison=True)      # the same buffer, NaN-filled first
    c = hip_step(st, table, q, target, (), 2, HALF, masks, img_idx=idx)
    for other in (b, c):
        assert torch.equal(a["t_logits"], other["t_logits"]) and torch.equal(a["t_att"], other["t_att"]) and torch.equal(a["t_dq"], other["t_dq"])
        for k in FIELDS:
            assert torch.isfinite(other["t_grads"][k]).all() and torch.equal(a["t_grads"][k], other["t_grads"][k]), k
    shape = (3, 36, 20, 70, 3, 12, 9, 14, 14)
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 0, (0.0,) * 6, None, False)
    a = hip_step(st, table, q, target)
    b = hip_step(st, table, q, target, ws=a["ws"], poison=True)
    assert torch.equal(a["t_logits"], b["t_logits"]) and torch.equal(a["t_dq"], b["t_dq"])
    assert all(torch.equal(a["t_grads"][k], b["t_grads"][k]) for k in FIELDS)


# ---- 6. eval agreement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [EDGE[1], EDGE[3]], ids=["P196", "P2"])
def test_training_forward_without_dropout_equals_the_eval_forward(shape):
    from neuralcx import ops
    st, table, q, target, idx, masks, r, ba32 = train_case(51, shape, (), 0, (0.0,) * 6, None, False)
    h = hip_step(st, table, q, target)
    logits, att = ops.mlb_att_forward(t_dev(table), None, t_dev(q), h["mw"])
    el, ea = logits.cpu().numpy(), att.cpu().numpy()
    for key, g, e in (("logits", h["logits"], el), ("att", h["att"], ea)):
        err, mx = float(np.abs(g - e).max()), float(np.abs(e).max())
        print("train vs eval forward %s: %.3e (max %.3e)" % (key, err, mx))
        assert err <= 1e-4 * max(1.0, mx)


# ---- 7. the module route -----------------------------------------------------------------------------------------------------------
def test_module_route(monkeypatch):
    from neuralcx import ops
    shape = (13, 96, 48, 44, 2, 28, 52, 5, 7)
    st, maps, q, ref = R.peaked_case(31, *shape)
    v = torch.from_numpy(maps).to(DEV)
    wids = torch.randint(1, 40, (13, 6), generator=torch.Generator().manual_seed(3)).to(DEV)
    target = torch.randint(0, 52, (13,), generator=torch.Generator().manual_seed(4)).to(DEV)
    calls = []
    real = ops.mlb_att_train_forward
    monkeypatch.setattr(ops, "mlb_att_train_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])

    def build(flag, dtype):
        m = module_on_gpu(st, shape)
        for k in ("attention", "fusion", "classif"):
            for d in [x for x in m.opt[k] if x.startswith("dropout")]:
                m.opt[k][d] = 0.0
        torch.manual_seed(11)
        for p_ in m.seq2vec.parameters():                               # the same encoder on every side
            torch.nn.init.uniform_(p_, -0.3, 0.3)
        m = m.to(dtype)
        m.train()
        m.use_hip_train = flag
        return m

    # the question vectors come from the encoder here: conv_att.weight is doubled until the attention is peaked for THEM
    st = dict(st)
    with torch.no_grad():
        q_enc = build(False, torch.float32).seq2vec(wids).double().cpu().numpy()
    for _ in range(8):
        r = R.mlb_att_forward(st, maps, q_enc, want_logits=True)
        if R.peaked(r[2], r[1]):
            break
        st["conv_att.weight"] = (st["conv_att.weight"] * np.float32(2.0)).astype(np.float32)
    assert R.peaked(r[2], r[1])

    def grads_of(flag, dtype=torch.float32):
        m = build(flag, dtype)
        n = len(calls)
        out = m(v.to(dtype), wids)
        loss = torch.nn.functional.cross_entropy(out, target.long())
        loss.backward()
        g = {k: p_.grad.detach().double().cpu().numpy() for k, p_ in m.named_parameters() if p_.grad is not None}
        return g, len(calls) - n, out.detach().double().cpu().numpy(), torch.stack(m.list_att, 1).double().cpu().numpy(), m

    g_t, n_t, l_t, a_t, m_t = grads_of(False)
    assert n_t == 0                                                      # the flag off: the op is never called
    g_h, n_h, l_h, a_h, m_h = grads_of(True)
    assert n_h == 1                                                      # exactly once per step
    g_64 = grads_of(False, torch.float64)[0]
    assert set(g_h) == set(g_t) and any(k.startswith("seq2vec.") for k in g_h) and len([k for k in g_h if not k.startswith("seq2vec.")]) == 14
    assert np.abs(l_h - l_t).max() <= 1e-4 * max(1.0, np.abs(l_t).max()) and np.abs(a_h - a_t).max() <= 1e-4
    assert len(m_h.list_att) == 2 and m_h.list_att[0].shape == (13, 35) and not m_h.list_att[0].requires_grad
    for k, rg in g_t.items():
        tol = grad_tol(k, rg)
        if k == ZERO_IN_MATHS:
            tol = max(tol, 2.0 * float(np.abs(rg - g_64[k]).max()))
            err = float(np.abs(g_h[k] - g_64[k]).max())
        else:
            err = float(np.abs(g_h[k] - rg).max())
        print("module route d %s: max err %.3e, bound %.3e" % (k, err, tol))
        assert err <= tol, (k, err, tol)
    # eval mode under no_grad keeps the eval-mode HIP forward; a frozen head in eval mode never takes the training route
    m_h.eval()
    with torch.no_grad():
        n = len(calls)
        m_h(v, wids)
        assert len(calls) == n


# ---- 8. the command line -----------------------------------------------------------------------------------------------------------
def test_train_cli_hip_att_train(tmp_path, capsys):
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
    calls = []
    real = ops.mlb_att_train_forward
    ops.mlb_att_train_forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    base = ["--path_opt", str(path), "--synthetic", "--syn_examples", "36", "--syn_images", "64", "--syn_vocab", "30", "--syn_grid", "5", "--print_freq", "0"]
    try:
        out = _cli("train.py").main(base + ["--hip_att_train"])
        text = capsys.readouterr().out
        assert "attention head, glimpse fusion and classifier train in HIP" in text and "there is no HIP engine" not in text
        assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["train"]["loss"]) and np.isfinite(out["history"][0]["val"]["loss"])
        n_train = len(calls)
        assert n_train >= 2 and out["trainer"].model.use_hip_train is True and out["trainer"].engine is None
        assert isinstance(out["trainer"].optim, torch.optim.Adam)
        fr = _cli("train.py").main(base + ["--hip_att_train", "--freeze_seq2vec"])
        text = capsys.readouterr().out
        assert "the encoder is frozen" in text and np.isfinite(fr["history"][0]["train"]["loss"]) and len(calls) > n_train
        assert all(not p.requires_grad for p in fr["trainer"].model.seq2vec.parameters())
        # without the flag nothing changes
        n = len(calls)
        plain = _cli("train.py").main(base)
        assert len(calls) == n and plain["trainer"].model.use_hip_train is False
        assert "module under torch autograd; eval-mode forward in HIP (ncx_mlb_att_forward)" in capsys.readouterr().out
    finally:
        ops.mlb_att_train_forward = real


# ---- 9. the YAML's full widths -----------------------------------------------------------------------------------------------------
def test_full_widths_vs_fp64():
    shape, seed = (8, 2048, 2400, 1200, 4, 1200, 2000, 14, 14), 0x0123456789ABCDEF
    st, table, q, target, idx, masks, r, ba32 = train_case(54, shape, (), 1, HALF, seed)
    h = hip_step(st, table, q, target, (), 1, HALF, None, seed=seed)
    compare(h, ref_of(r, 4), "full widths", ba32=ba32)
