"""GPU: training the MLBNoAtt VQA model in HIP -- the training-mode forward and the backward (with ncx_ce_loss between them) against
the reference-produced fixture and the fp64 restatement (explicit masks, each activation switched off, the counter-based generator,
edge shapes, the real widths), the eval forward against the frozen producer, determinism, the autograd route of the module, the
engine against a torch loop, and the CLI closing the loop into the counterexample pipeline's producer.

Bounds (the project's, tests/test_vqa_train_gpu.py): logits and z 1e-4 max(1, max|ref|); loss 1e-5 max(1, |ref|); every gradient
and dq_emb helpers.grad_tol (1e-4 of the tensor's max)."""
import os

import numpy as np
import pytest
import torch

import mlb_train_ref as R
import trainer_edge_cases as E
from conftest import GOLDEN, PKG
from helpers import grad_tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, dv, dq, dh, A)
EDGE_SHAPES = E.MLB_EDGE + [E.MLB_RAGGED, (48, 2048, 2400, 1200, 2000)]
_case = E.mlb_case
ALL_ON = (True, True, True)
_ids = lambda s: "x".join(map(str, s))


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _weights(P, acts=ALL_ON):
    from neuralcx import ops
    return ops.MlbWeights.from_tensors({k: _t(v) for k, v in P.items()}, *(2 if a else 0 for a in acts))


def _run(shape, P, feats, q, idx, target, masks=None, p=(0.0, 0.0, 0.0), mode=0, seed=0, want_dq=True, acts=ALL_ON):
    """forward + ce_loss + backward through the C ABI -> dict of device results (and the objects a test may want to look into).
    Every gradient buffer is NaN before the call: a missed write shows."""
    from neuralcx import ops
    B, dv, dq, dh, A = shape
    mw = _weights(P, acts)
    d = ops.vqa_train_dims(B, dv, dq, dh, A, feats.shape[0], p=p, dropout_mode=mode, seed=seed, want_dq=want_dq)
    ws = ops.mlb_train_workspace(d, mw, DEV)
    mk = None if masks is None else torch.cat([_t(m).reshape(-1) for m in masks])
    logits, z = ops.mlb_train_forward(d, _t(feats), _t(idx, torch.int32), _t(q), mw, ws, masks=mk)
    ce = ops.ce_loss(logits, _t(target, torch.int32))
    grads = {k: torch.full_like(v, float("nan")) for k, v in mw.t.items()}
    dqe = ops.mlb_train_backward(d, mw, ws, ce["dlogits"], grads, masks=mk)
    torch.cuda.synchronize()
    ops.check_vqa_targets(device=DEV)
    return dict(logits=logits, z=z, ce=ce, grads=grads, dq=dqe, d=d, mw=mw, ws=ws)


def _compare(out, ref, target, want_dq=True):
    lg = out["logits"].cpu().numpy().astype(np.float64)
    e_l = np.abs(lg - ref["logits"]).max()
    e_z = np.abs(out["z"].cpu().numpy() - ref["z"]).max()
    e_loss = abs(float(out["ce"]["loss"].cpu()) - ref["loss"])
    print("logits err %.3e (max %.3e)  z err %.3e  loss err %.3e" % (e_l, np.abs(ref["logits"]).max(), e_z, e_loss))
    assert e_l <= 1e-4 * max(1.0, np.abs(ref["logits"]).max())
    assert e_z <= 1e-4 * max(1.0, np.abs(ref["z"]).max())
    assert e_loss <= 1e-5 * max(1.0, abs(ref["loss"]))
    errs = {}
    for k, g in ref["grads"].items():
        got = out["grads"][k].cpu().numpy().astype(np.float64)
        assert np.isfinite(got).all(), k
        errs[k] = (np.abs(got - g).max(), grad_tol(k, g))
    if want_dq:
        errs["dq_emb"] = (np.abs(out["dq"].cpu().numpy() - ref["dq"]).max(), grad_tol("dq_emb", ref["dq"]))
    print("grad err / tol:", {k: "%.2e/%.2e" % v for k, v in errs.items()})
    for k, (e, tol) in errs.items():
        assert e <= tol, (k, e, tol)
    safe = R.rank_safe(ref["logits"], target)
    rk = ref["rank"][safe]
    # the counts over the rows whose rank cannot depend on rounding bracket the kernel's counts
    n_unsafe = int((~safe).sum())
    h1, h5 = int(out["ce"]["hits1"].cpu()), int(out["ce"]["hits5"].cpu())
    assert int((rk < 1).sum()) <= h1 <= int((rk < 1).sum()) + n_unsafe
    assert int((rk < 5).sum()) <= h5 <= int((rk < 5).sum()) + n_unsafe


GOLDEN_CASES = {"c0": (True, True, True), "c1": (False, True, False)}


@pytest.mark.parametrize("case", ["c0", "c1"])
def test_parity_with_reference_fixture(case):
    """forward, ce_loss, backward and one ncx_adam_step against what the reference's own code produced."""
    from neuralcx import ops
    g, c = np.load(os.path.join(GOLDEN, "g17_mlb_train.npz")), case + "/"
    names = [str(n) for n in g[c + "names"]]
    P = R.state_to_fields({n: g[c + "init/" + n] for n in names})
    feats, idx, q, target = g[c + "feats"], g[c + "img_idx"].astype(np.int32), g[c + "q_emb"], g[c + "target"].astype(np.int32)
    B, dv, dq = idx.shape[0], feats.shape[1], q.shape[1]
    shape = (B, dv, dq, P["wc"].shape[1], P["wc"].shape[0])
    out = _run(shape, P, feats, q, idx, target, acts=GOLDEN_CASES[case])
    lg = g[c + "logits"]
    e_l, e_loss = np.abs(out["logits"].cpu().numpy() - lg).max(), abs(float(out["ce"]["loss"].cpu()) - float(g[c + "loss"]))
    print("logits err %.3e (max %.3e)  loss err %.3e" % (e_l, np.abs(lg).max(), e_loss))
    assert e_l <= 1e-4 * max(1.0, np.abs(lg).max())
    assert e_loss <= 1e-5 * max(1.0, abs(float(g[c + "loss"])))
    gsd = R.state_to_fields({n: g[c + "grad/" + n] for n in names})
    for k, ref in gsd.items():
        got = out["grads"][k].cpu().numpy()
        assert np.isfinite(got).all(), k
        e = np.abs(got - ref).max()
        print("grad %s err %.2e / tol %.2e" % (k, e, grad_tol(k, ref)))
        assert e <= grad_tol(k, ref), (k, e, grad_tol(k, ref))
    e = np.abs(out["dq"].cpu().numpy() - g[c + "grad_q_emb"]).max()
    assert e <= grad_tol("dq_emb", g[c + "grad_q_emb"]), e
    safe = R.rank_safe(lg.astype(np.float64), target)
    if safe.all():
        assert abs(100.0 * int(out["ce"]["hits1"].cpu()) / B - float(g[c + "acc1"])) < 1e-3
        assert abs(100.0 * int(out["ce"]["hits5"].cpu()) / B - float(g[c + "acc5"])) < 1e-3
    # one Adam step (lr 1e-4) on the flat buffer, at the bound the Mutan fixture test uses
    flat_p = torch.cat([out["mw"].t[k].reshape(-1) for k in ops.MLB_FIELDS])
    flat_g = torch.cat([out["grads"][k].reshape(-1) for k in ops.MLB_FIELDS])
    ops.adam_step(flat_p, flat_g, torch.zeros_like(flat_p), torch.zeros_like(flat_p), 1, lr=1e-4)
    after = R.state_to_fields({n: g[c + "after/" + n] for n in names})
    ref_flat = np.concatenate([after[k].reshape(-1) for k in ops.MLB_FIELDS])
    assert np.abs(flat_p.cpu().numpy() - ref_flat).max() <= 2e-6


def _edge_inputs(shape):
    P, feats, q, idx, target, masks = _case(shape)
    if shape[0] == 33:                       # a non-identity index: a repeated image, an all-zero feature row, ids outside the table (clamped)
        idx = E.gathered_33(feats, out_of_table=True)
    return P, feats, q, idx, target, masks


def _edge(shape, want_dq, acts):
    P, feats, q, idx, target, masks = _edge_inputs(shape)
    out = _run(shape, P, feats, q, idx, target, masks=masks, p=(0.5, 0.5, 0.5), mode=2, want_dq=want_dq, acts=acts)
    rows = np.clip(idx, 0, feats.shape[0] - 1)
    ref = R.step(P, feats[rows], q, target, act_v=acts[0], act_q=acts[1], act_c=acts[2], masks=masks, p=(0.5, 0.5, 0.5))
    assert (out["dq"] is None) == (not want_dq)
    _compare(out, ref, target, want_dq)


@pytest.mark.parametrize("want_dq", [True, False])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=_ids)
def test_edge_shapes_explicit_masks(shape, want_dq):
    _edge(shape, want_dq, ALL_ON)


@pytest.mark.parametrize("want_dq", [True, False])
@pytest.mark.parametrize("off", [0, 1, 2], ids=["no_act_v", "no_act_q", "no_act_c"])
@pytest.mark.parametrize("shape", EDGE_SHAPES[:3], ids=_ids)
def test_edge_shapes_one_activation_off(shape, off, want_dq):
    """each activation switched off removes one factor of k_train_dfuse (and act_c the stored t)"""
    _edge(shape, want_dq, tuple(i != off for i in range(3)))


def test_generator_dropout_masks_and_gradients():
    from neuralcx import ops
    from oracle.ncx_oracle import dropout_keep_mask
    shape = (70, 132, 96, 44, 100)
    B, dv, dq, dh, A = shape
    P, feats, q, idx, target, _ = _case(shape, seed=3)
    feats = feats + 0.01                     # strictly positive: a zero in a dropped tensor is a dropped element
    q = np.where(np.abs(q) < 1e-3, 0.01, q).astype(np.float32)
    p, seed = (0.25, 0.25, 0.25), 0x1234567855AA
    out = _run(shape, P, feats, q, idx, target, p=p, mode=1, seed=seed)
    want = [dropout_keep_mask(seed, layer, B, w, 0.25).numpy() for layer, w in ((1, dv), (2, dq), (3, dh))]
    view = lambda o, which: ops.mlb_train_ws_region(o["d"], o["mw"], o["ws"], which)
    got_v = (view(out, ops.VT_WS_VD) != 0).float().cpu().numpy()
    got_q = (view(out, ops.VT_WS_QD) != 0).float().cpu().numpy()
    tc = view(out, ops.VT_WS_ZC).cpu().numpy()
    assert got_v.shape == (B, dv) and got_q.shape == (B, dq) and tc.shape == (B, dh)
    assert np.array_equal(got_v, want[0]) and np.array_equal(got_q, want[1])
    znz = np.abs(out["z"].cpu().numpy()) > 1e-6          # tanh(z) is zero only where z is
    assert znz.mean() > 0.9
    assert np.array_equal((tc != 0)[znz], want[2].astype(bool)[znz])
    for m in want:
        assert 0.6 < m.mean() < 0.9
    ref = R.step(P, feats[idx], q, target, masks=tuple(want), p=p)
    _compare(out, ref, target)
    out2 = _run(shape, P, feats, q, idx, target, p=p, mode=1, seed=seed + 1)
    v2 = (view(out2, ops.VT_WS_VD) != 0).float().cpu().numpy()
    assert not np.array_equal(v2, got_v)
    assert np.array_equal(v2, dropout_keep_mask(seed + 1, 1, B, dv, 0.25).numpy())


@pytest.mark.parametrize("act_c", ["tanh", None])
def test_eval_forward_equals_frozen_producer(act_c):
    """MlbTrainEngine.evaluate against ncx_mlb_forward (ops.vqa_forward on the engine's own buffers), K = 1"""
    from neuralcx import ops
    from neuralcx.vqa_train import MlbTrainEngine
    shape = (70, 132, 96, 44, 100)
    B, dv, dq, dh, A = shape
    P, feats, q, idx, target, _ = _case(shape, seed=4)
    e = MlbTrainEngine(dv=dv, dq=dq, dh=dh, A=A, activation_c=act_c, device=DEV)
    for k, x in P.items():
        e.params.views[k].copy_(_t(x))
    r = e.evaluate(_t(feats), _t(idx, torch.int32), _t(q), _t(target, torch.int32))
    mw = e.mlb_weights()
    assert all(mw.t[k].data_ptr() == e.params.views[k].data_ptr() for k in ops.MLB_FIELDS)
    idx2 = np.stack([idx, idx], 1)           # the frozen producer wants an original and one candidate per question
    a_o, z_o, a_k, z_k = ops.vqa_forward(_t(feats), _t(idx2, torch.int32), _t(q), mw, want_a_orig=True)
    ref = R.step(P, feats[idx], q, target, act_c=act_c is not None)
    assert np.abs(r["logits"].cpu().numpy() - ref["logits"]).max() <= 1e-4 * max(1.0, np.abs(ref["logits"]).max())
    assert abs(float(r["loss"].cpu()) - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
    for got, want in ((r["logits"], a_o), (r["logits"], a_k[:, 0]), (r["z"], z_o), (r["z"], z_k[:, 0])):
        assert (got - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())


def test_deterministic_and_overwrites_at_real_widths():
    shape = EDGE_SHAPES[-1]
    P, feats, q, idx, target, masks = _case(shape)
    a, b = [_run(shape, P, feats, q, idx, target, p=(0.5, 0.5, 0.5), mode=1, seed=11) for _ in range(2)]
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["z"], b["z"]) and torch.equal(a["ce"]["loss"], b["ce"]["loss"])
    assert torch.equal(a["dq"], b["dq"]) and torch.isfinite(a["dq"]).all()
    for k in a["grads"]:
        assert torch.isfinite(a["grads"][k]).all(), k            # pre-filled with NaN: every element was overwritten
        assert torch.equal(a["grads"][k], b["grads"][k]), k


# ---- the module route, the engine, the CLI --------------------------------------------------------------------------------------
def _opt(p=0.0):
    fus = dict(dim_v=64, dim_q=48, dim_h=24, activation_v="tanh", activation_q="tanh", dropout_v=p, dropout_q=p)
    return dict(arch="MLBNoAtt", seq2vec=dict(arch="gru", emb_size=16, dropout=0.0, fixed_emb=False), fusion=fus,
                classif=dict(activation="tanh", dropout=p))


def test_module_route_trains_encoder_through_autograd():
    from vqa import models
    torch.manual_seed(0)
    A, B = 40, 37
    model = models.factory(_opt(), ["w%d" % i for i in range(20)], ["a%d" % i for i in range(A)], cuda=True).train()
    assert type(model).__name__ == "MLBNoAtt"
    v = torch.rand(B, 64, device=DEV)
    w = torch.randint(1, 21, (B, 7), device=DEV); w[:, 5:] = 0
    t = torch.randint(0, A, (B,), device=DEV)
    crit = torch.nn.CrossEntropyLoss()
    grads = {}
    for hip in (False, True):
        model.use_hip_train = hip
        model.zero_grad()
        out = model(v, w)
        assert (type(out.grad_fn).__name__ == "MlbTrainFunctionBackward") == hip
        crit(out, t).backward()
        grads[hip] = {n: p.grad.detach().cpu().numpy().astype(np.float64) for n, p in model.named_parameters()}
        grads[hip]["logits"] = out.detach().cpu().numpy()
    assert np.abs(grads[True]["logits"] - grads[False]["logits"]).max() <= 1e-4 * max(1.0, np.abs(grads[False]["logits"]).max())
    for n, ref in grads[False].items():
        if n == "logits":
            continue
        assert n.startswith(("seq2vec.", "fusion.", "linear_classif.")) and np.abs(ref).max() > 0, n
        e = np.abs(grads[True][n] - ref).max()
        assert e <= grad_tol(n, ref), (n, e, grad_tol(n, ref))
    assert any(n.startswith("seq2vec.gru") for n in grads[True])
    # the attribute left at its default: the module's output is the torch ops', bit for bit
    del model.use_hip_train
    assert model.use_hip_train is False
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(v, w), model._classif(model.fusion(v, model.seq2vec(w))))


def test_engine_equals_torch_adam_loop():
    """Three steps, dropout off, lr 1e-3, against torch autograd + torch.optim.Adam on the same parameters."""
    from neuralcx.vqa_train import MlbTrainEngine
    shape = (64, 132, 96, 44, 100)
    B, dv, dq, dh, A = shape
    rng = np.random.default_rng(8)
    P = R.init_params(9, dv, dq, dh, A, gain=2.0)
    v = (np.abs(rng.standard_normal((B, dv))) * 0.45).astype(np.float32)
    q = (rng.standard_normal((B, dq)) * 0.3).astype(np.float32)
    t = rng.integers(0, A, size=B)
    e = MlbTrainEngine(dv=dv, dq=dq, dh=dh, A=A, dropout=(0, 0, 0), lr=1e-3, device=DEV)
    for k, x in P.items():
        e.params.views[k].copy_(_t(x))
    Pt = {k: _t(x).requires_grad_(True) for k, x in P.items()}
    opt = torch.optim.Adam(list(Pt.values()), lr=1e-3)
    vt, qt, tt = _t(v), _t(q), _t(t, torch.int64)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    for s in range(3):
        xv = torch.tanh(vt @ Pt["wv"].t() + Pt["bv"]); xq = torch.tanh(qt @ Pt["wq"].t() + Pt["bq"])
        loss = torch.nn.functional.cross_entropy(torch.tanh(xq * xv) @ Pt["wc"].t() + Pt["bc"], tt)
        opt.zero_grad(); loss.backward()
        r = e.train_step(vt, idx, qt, tt.to(torch.int32))
        ref_loss = float(loss.detach())
        assert abs(float(r["loss"]) - ref_loss) <= 1e-5 * max(1.0, ref_loss), s
        if s == 0:
            for k in P:
                ref = Pt[k].grad.cpu().numpy()
                err = np.abs(e.grads.views[k].cpu().numpy() - ref).max()
                assert err <= grad_tol(k, ref), (k, err)
        opt.step()
    # the drift bound of tests/test_vqa_train_gpu.py::test_engine_equals_torch_adam_loop, by its expression
    bound = min(4 * 5.17e-07, 0.25 * 3 * 1e-3)
    drift = max(float((e.params.views[k] - Pt[k].detach()).abs().max()) for k in P)
    print("drift %.3e (bound %.3e)" % (drift, bound))
    assert drift <= bound, drift


TINY_YAML = """
logs: {dir_logs: %s}
vqa: {nans: 40, maxlength: 8}
coco: {}
model:
  arch: MLBNoAtt
  seq2vec: {arch: gru, emb_size: 16, dropout: 0.0, fixed_emb: False}
  fusion: {dim_v: 64, dim_q: 48, dim_h: 24, activation_v: tanh, activation_q: tanh, dropout_v: 0.1, dropout_q: 0.1}
  classif: {activation: tanh, dropout: 0.1}
optim: {lr: 0.003, batch_size: 64, epochs: 2}
"""
TINY_ARGS = ["--synthetic", "--syn_examples", "384", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0", "--freeze_seq2vec"]


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("vqa_train_cli", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_trains_resumes_and_feeds_the_frozen_producer(tmp_path):
    """train.py --synthetic --freeze_seq2vec (the whole step in HIP) on an MLB YAML, on the seed whose torch path (--no_hip, on a CPU)
    was checked to lower the train loss from epoch 1 (3.698) to epoch 2 (3.677): 1337, the default."""
    from neuralcx import ops
    from neuralcx.vqa_train import MlbTrainEngine
    from vqa import models
    cli = _cli()
    runs = {}
    for name in ("straight", "resumed"):
        logs = str(tmp_path / name)
        y = tmp_path / (name + ".yaml")
        y.write_text(TINY_YAML % logs)
        if name == "straight":
            runs[name] = cli.main(["--path_opt", str(y)] + TINY_ARGS)
        else:
            cli.main(["--path_opt", str(y), "--epochs", "1"] + TINY_ARGS)
            runs[name] = cli.main(["--path_opt", str(y), "--resume", "ckpt"] + TINY_ARGS)
        for tag in ("ckpt", "best"):
            for part in ("info", "model", "optim"):
                assert os.path.isfile(os.path.join(logs, "%s_%s.pth.tar" % (tag, part))), (name, tag, part)
    tr = runs["straight"]["trainer"]
    assert isinstance(tr.engine, MlbTrainEngine) and tr.route == "hip"
    h = runs["straight"]["history"]
    print("train loss by epoch:", [x["train"]["loss"] for x in h])
    assert [x["epoch"] for x in h] == [1, 2] and h[0]["train"]["loss"] > h[1]["train"]["loss"], h
    assert [x["epoch"] for x in runs["resumed"]["history"]] == [1, 2]
    a = torch.load(str(tmp_path / "straight" / "ckpt_model.pth.tar"))
    b = torch.load(str(tmp_path / "resumed" / "ckpt_model.pth.tar"))
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k                      # --resume ckpt continues bit for bit
    oa, ob = (torch.load(str(tmp_path / n / "ckpt_optim.pth.tar")) for n in ("straight", "resumed"))
    assert oa["step"] == ob["step"] and torch.equal(oa["exp_avg"], ob["exp_avg"]) and torch.equal(oa["exp_avg_sq"], ob["exp_avg_sq"])
    # closing the loop: best_model.pth.tar -> models.factory -> the frozen producer's weights -> the trainer's eval logits
    opt = cli.load_options(cli.build_parser().parse_args(["--path_opt", str(tmp_path / "straight.yaml")]))
    model = models.factory(opt["model"], ["w%d" % i for i in range(30)], ["a%d" % i for i in range(40)], cuda=True)
    best = torch.load(str(tmp_path / "straight" / "best_model.pth.tar"))
    model.load_state_dict(best, strict=True)
    tr.engine.load_state_dict(best)
    sel = torch.arange(0, 48, device=DEV)
    idx, q, aids = tr.val.img_idx[sel], tr.q_emb_of(tr.val)[sel], tr.val.aids[sel]
    want = tr.engine.evaluate(tr.val.feats, idx, q, aids)["logits"]
    mw = ops.vqa_weights(model.eval())
    assert isinstance(mw, ops.MlbWeights)
    a_o, _, _, _ = ops.vqa_forward(tr.val.feats, torch.stack([idx, idx], 1).contiguous(), q.contiguous(), mw, want_a_orig=True)
    assert (a_o - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
