"""GPU: training the MutanNoAtt VQA model in HIP -- the training-mode forward, the cross-entropy head and the backward against the
reference-produced fixture and the fp64 restatement (explicit masks, the counter-based generator, edge shapes, the real widths),
the eval forward against the frozen producer, determinism, the autograd route of the module, the engine against a torch loop, and
the CLI closing the loop into the counterexample pipeline's producer."""
import os

import numpy as np
import pytest
import torch

import trainer_edge_cases as E
import vqa_train_ref as R
from conftest import GOLDEN, PKG
from helpers import grad_tol
from loss_adam_ref import ce_ref as _ce_ref

pytestmark = pytest.mark.gpu
DEV = "cuda:0"
# (B, dv, dq, dhv, dhq, dz, R, A)
EDGE_SHAPES = E.MUTAN_EDGE + [E.MUTAN_RAGGED, (48, 2048, 2400, 360, 360, 360, 10, 2000)]
_case = E.mutan_case


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _weights(P, Rk, act_v=True, act_q=True):
    from neuralcx import ops
    return ops.MutanWeights.from_tensors({k: _t(v) for k, v in P.items()}, Rk, 2 if act_v else 0, 2 if act_q else 0)


def _run(shape, P, feats, q, idx, target, masks=None, p=(0.0, 0.0, 0.0), mode=0, seed=0, want_dq=True, act_v=True, act_q=True, nan_fill=True):
    """forward + ce_loss + backward through the C ABI -> dict of device results (and the objects a test may want to look into)"""
    from neuralcx import ops
    B, dv, dq, dhv, dhq, dz, Rk, A = shape
    mw = _weights(P, Rk, act_v, act_q)
    d = ops.vqa_train_dims(B, dv, dq, dz, A, feats.shape[0], p=p, dropout_mode=mode, seed=seed, want_dq=want_dq)
    ws = ops.vqa_train_workspace(d, mw, DEV)
    mk = None if masks is None else torch.cat([_t(m).reshape(-1) for m in masks])
    logits, z = ops.vqa_train_forward(d, _t(feats), _t(idx, torch.int32), _t(q), mw, ws, masks=mk)
    ce = ops.ce_loss(logits, _t(target, torch.int32))
    grads = {k: torch.full_like(v, float("nan")) if nan_fill else torch.zeros_like(v) for k, v in mw.t.items()}
    dqe = ops.vqa_train_backward(d, mw, ws, ce["dlogits"], grads, masks=mk)
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


def _golden():
    return np.load(os.path.join(GOLDEN, "g16_vqa_train.npz"))


GOLDEN_CASES = {"c0": dict(R=10, act_v=True), "c1": dict(R=3, act_v=False)}


@pytest.mark.parametrize("case", ["c0", "c1"])
def test_parity_with_reference_fixture(case):
    """forward, ce_loss, backward and one ncx_adam_step against what the reference's own code produced."""
    from neuralcx import ops
    g, c = _golden(), case + "/"
    names = [str(n) for n in g[c + "names"]]
    sd = {n: g[c + "init/" + n] for n in names}
    Rk, act_v = GOLDEN_CASES[case]["R"], GOLDEN_CASES[case]["act_v"]
    P = R.state_to_fields(sd, Rk)
    feats, idx, q, target = g[c + "feats"], g[c + "img_idx"].astype(np.int32), g[c + "q_emb"], g[c + "target"].astype(np.int32)
    B, dv, dq = idx.shape[0], feats.shape[1], q.shape[1]
    shape = (B, dv, dq, P["wv"].shape[0], P["wq"].shape[0], P["wc"].shape[1], Rk, P["wc"].shape[0])
    out = _run(shape, P, feats, q, idx, target, act_v=act_v)
    lg = g[c + "logits"]
    assert np.abs(out["logits"].cpu().numpy() - lg).max() <= 1e-4 * max(1.0, np.abs(lg).max())
    assert abs(float(out["ce"]["loss"].cpu()) - float(g[c + "loss"])) <= 1e-5 * max(1.0, abs(float(g[c + "loss"])))
    gsd = R.state_to_fields({n: g[c + "grad/" + n] for n in names}, Rk)
    for k, ref in gsd.items():
        e = np.abs(out["grads"][k].cpu().numpy() - ref).max()
        assert e <= grad_tol(k, ref), (k, e, grad_tol(k, ref))
    e = np.abs(out["dq"].cpu().numpy() - g[c + "grad_q_emb"]).max()
    assert e <= grad_tol("dq_emb", g[c + "grad_q_emb"]), e
    safe = R.rank_safe(lg.astype(np.float64), target)
    if safe.all():
        assert abs(100.0 * int(out["ce"]["hits1"].cpu()) / B - float(g[c + "acc1"])) < 1e-3
        assert abs(100.0 * int(out["ce"]["hits5"].cpu()) / B - float(g[c + "acc5"])) < 1e-3
    # one Adam step (lr 1e-4) on the flat buffer: the pin test_parity_with_reference_fixture of the scorers uses
    flat_p = torch.cat([out["mw"].t[k].reshape(-1) for k in ops.MUTAN_FIELDS])
    flat_g = torch.cat([out["grads"][k].reshape(-1) for k in ops.MUTAN_FIELDS])
    ops.adam_step(flat_p, flat_g, torch.zeros_like(flat_p), torch.zeros_like(flat_p), 1, lr=1e-4)
    after = R.state_to_fields({n: g[c + "after/" + n] for n in names}, Rk)
    ref_flat = np.concatenate([after[k].reshape(-1) for k in ops.MUTAN_FIELDS])
    assert np.abs(flat_p.cpu().numpy() - ref_flat).max() <= 2e-6


@pytest.mark.parametrize("want_dq", [True, False])
@pytest.mark.parametrize("shape", EDGE_SHAPES, ids=lambda s: "x".join(map(str, s)))
def test_edge_shapes_explicit_masks(shape, want_dq):
    P, feats, q, idx, target, masks = _case(shape)
    if shape[0] == 33:                       # a non-identity index: a repeated image and an all-zero feature row
        idx = E.gathered_33(feats, out_of_table=False)
    out = _run(shape, P, feats, q, idx, target, masks=masks, p=(0.5, 0.5, 0.5), mode=2, want_dq=want_dq)
    ref = R.step(P, feats[idx], q, target, masks=masks, p=(0.5, 0.5, 0.5))
    assert (out["dq"] is None) == (not want_dq)
    _compare(out, ref, target, want_dq)


def test_generator_dropout_masks_and_gradients():
    from neuralcx import ops
    from oracle.ncx_oracle import dropout_keep_mask
    shape = (70, 132, 96, 44, 40, 40, 10, 100)
    B, dv, dq, dhv, dhq, dz, Rk, A = shape
    P, feats, q, idx, target, _ = _case(shape, seed=3)
    feats = feats + 0.01                     # strictly positive: a zero in a dropped tensor is a dropped element
    q = np.where(np.abs(q) < 1e-3, 0.01, q).astype(np.float32)
    p, seed = (0.25, 0.25, 0.25), 0x1234567855AA
    out = _run(shape, P, feats, q, idx, target, p=p, mode=1, seed=seed)
    want = [dropout_keep_mask(seed, ops.VT_LAYERS[n], B, w, 0.25).numpy() for n, w in (("v", dv), ("q", dq), ("z", dz))]
    got_v = (ops.vqa_train_ws_view(out["d"], out["mw"], out["ws"], ops.VT_WS_VD) != 0).float().cpu().numpy()
    got_q = (ops.vqa_train_ws_view(out["d"], out["mw"], out["ws"], ops.VT_WS_QD) != 0).float().cpu().numpy()
    zc = ops.vqa_train_ws_view(out["d"], out["mw"], out["ws"], ops.VT_WS_ZC).cpu().numpy()
    assert np.array_equal(got_v, want[0]) and np.array_equal(got_q, want[1])
    znz = np.abs(out["z"].cpu().numpy()) > 1e-6
    assert np.array_equal((zc != 0)[znz], want[2].astype(bool)[znz])
    for m in want:
        assert 0.6 < m.mean() < 0.9
    ref = R.step(P, feats[idx], q, target, masks=tuple(want), p=p)
    _compare(out, ref, target)
    out2 = _run(shape, P, feats, q, idx, target, p=p, mode=1, seed=seed + 1)
    v2 = (ops.vqa_train_ws_view(out2["d"], out2["mw"], out2["ws"], ops.VT_WS_VD) != 0).float().cpu().numpy()
    assert not np.array_equal(v2, got_v)
    assert np.array_equal(v2, dropout_keep_mask(seed + 1, 1, B, dv, 0.25).numpy())


def test_eval_mode_equals_frozen_producer():
    from neuralcx import ops
    shape = (70, 132, 96, 44, 40, 40, 10, 100)
    P, feats, q, idx, target, _ = _case(shape, seed=4)
    out = _run(shape, P, feats, q, idx, target)
    # K = 1: the frozen producer wants an original and one candidate per question
    idx2 = np.stack([idx, idx], 1)
    a_o, z_o, _, _ = ops.vqa_forward(_t(feats), _t(idx2, torch.int32), _t(q), out["mw"], want_a_orig=True)
    assert (out["logits"] - a_o).abs().max().item() <= 1e-4 * max(1.0, a_o.abs().max().item())
    assert (out["z"] - z_o).abs().max().item() <= 1e-4 * max(1.0, z_o.abs().max().item())


def test_deterministic_and_overwrites_at_real_widths():
    shape = EDGE_SHAPES[-1]
    P, feats, q, idx, target, masks = _case(shape)
    runs = [_run(shape, P, feats, q, idx, target, p=(0.5, 0.5, 0.5), mode=1, seed=11) for _ in range(2)]
    a, b = runs
    assert torch.equal(a["logits"], b["logits"]) and torch.equal(a["z"], b["z"]) and torch.equal(a["ce"]["loss"], b["ce"]["loss"])
    assert torch.equal(a["dq"], b["dq"]) and torch.isfinite(a["dq"]).all()
    for k in a["grads"]:
        assert torch.isfinite(a["grads"][k]).all(), k            # pre-filled with NaN: every element was overwritten
        assert torch.equal(a["grads"][k], b["grads"][k]), k


@pytest.mark.parametrize("A", [5, 2000])
def test_ce_loss_alone(A):
    from neuralcx import ops
    rng = np.random.default_rng(A)
    B = 9
    x = (rng.standard_normal((B, A)) * 2).astype(np.float32)
    t = rng.integers(0, A, size=B).astype(np.int32)
    x[0, 0], x[0, 1] = 80.0, -80.0                               # extreme logits: the max is subtracted
    t[0] = 1
    t[1] = int(x[1].argmax()); t[2] = int(x[2].argmin())
    # exact top-5 boundaries, gaps >= 1e-2: row 3's target is fifth (a hit), row 4's sixth (a miss); row 5: a tie ahead of the target
    for r, place in ((3, 4), (4, 5)):
        if A > 5:
            x[r] = -5.0 - 0.01 * np.arange(A)
            x[r, :6] = 3.0 - 0.01 * np.arange(6)
            t[r] = place
    x[5, 0] = x[5, A - 1] = x[5].max() + 1.0
    t[5] = A - 1                                                 # an equal logit at a lower index ranks ahead: rank 1
    ref = _ce_ref(x, t)
    ce = ops.ce_loss(_t(x), _t(t, torch.int32))
    torch.cuda.synchronize()
    ops.check_vqa_targets(device=DEV)
    assert abs(float(ce["loss"].cpu()) - ref["loss"]) <= 1e-5 * max(1.0, abs(ref["loss"]))
    e = np.abs(ce["dlogits"].cpu().numpy() - ref["dl"]).max()
    assert e <= 1e-4 * np.abs(ref["dl"]).max(), e
    assert int(ce["hits1"].cpu()) == int((ref["rank"] < 1).sum())
    assert int(ce["hits5"].cpu()) == int((ref["rank"] < 5).sum())
    if A > 5:
        assert ref["rank"][3] == 4 and ref["rank"][4] == 5
    assert ref["rank"][1] == 0 and ref["rank"][2] == A - 1 and ref["rank"][5] == 1
    # the guard: a target of -1 or A raises the flag, its row contributes nothing, and nothing beyond the outputs is touched
    for bad in (-1, A):
        t2 = t.copy(); t2[6] = bad
        guard = torch.full((B * A + 64,), 7.0, device=DEV)
        ce2 = _ce_into(x, t2, guard, B, A)
        torch.cuda.synchronize()
        assert (guard[B * A:] == 7.0).all()
        assert (guard[6 * A:7 * A] == 0).all()
        keep = np.arange(B) != 6
        ref2 = _ce_ref(x[keep], t[keep], scale=1.0 / B)
        assert abs(float(ce2.cpu()) - ref2["loss"]) <= 1e-5 * max(1.0, abs(ref2["loss"]))
        with pytest.raises(IndexError):
            ops.check_vqa_targets(device=DEV)
        ops.check_vqa_targets(device=DEV)                        # cleared


def _ce_into(x, t, guard, B, A):
    """ncx_ce_loss writing dlogits into the head of `guard` (the tail is the canary)"""
    import ctypes as C
    from neuralcx import _lib, ops
    xs, ts = _t(x), _t(t, torch.int32)
    loss = torch.zeros(1, device=DEV); rows = torch.zeros(2 * B, device=DEV); hits = torch.zeros(2, dtype=torch.int32, device=DEV)
    p = lambda a: C.c_void_p(a.data_ptr())
    rc = _lib.lib().ncx_ce_loss(p(xs), p(ts), B, A, 0.0, p(loss), p(guard), p(hits), C.c_void_p(hits.data_ptr() + 4),
                                p(ops.vqa_bad_flag(DEV)), p(rows), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0
    return loss


# ---- the module route, the engine, the CLI --------------------------------------------------------------------------------------
def _opt(p=0.0):
    fus = dict(dim_v=64, dim_q=48, dim_hv=32, dim_hq=36, dim_mm=24, R=3, activation_v="tanh", activation_q="tanh", dropout_v=p, dropout_q=p,
               dropout_hv=0, dropout_hq=0)
    return dict(arch="MutanNoAtt", seq2vec=dict(arch="gru", emb_size=16, dropout=0.0, fixed_emb=False), fusion=fus, classif=dict(dropout=p))


def test_module_route_trains_encoder_through_autograd():
    from vqa import models
    torch.manual_seed(0)
    A, B = 40, 37
    model = models.factory(_opt(), ["w%d" % i for i in range(20)], ["a%d" % i for i in range(A)], cuda=True).train()
    v = torch.rand(B, 64, device=DEV)
    w = torch.randint(1, 21, (B, 7), device=DEV); w[:, 5:] = 0
    t = torch.randint(0, A, (B,), device=DEV)
    crit = torch.nn.CrossEntropyLoss()
    grads = {}
    for hip in (False, True):
        model.use_hip_train = hip
        model.zero_grad()
        out = model(v, w)
        assert (type(out.grad_fn).__name__ == "MutanTrainFunctionBackward") == hip
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
    # a step of torch.optim.Adam on the HIP route moves the encoder as well as the fusion
    model.use_hip_train = True
    opt = torch.optim.Adam(model.parameters(), 1e-3)
    before = {n: p.detach().clone() for n, p in model.named_parameters()}
    opt.zero_grad(); crit(model(v, w), t).backward(); opt.step()
    assert all(not torch.equal(before[n], p) for n, p in model.named_parameters() if n != "seq2vec.embedding.weight")
    # the attribute left at its default: the module's output is the torch ops', bit for bit
    del model.use_hip_train
    assert model.use_hip_train is False
    model.eval()
    with torch.no_grad():
        assert torch.equal(model(v, w), model._classif(model.fusion(v, model.seq2vec(w))))
    model.train()
    torch.manual_seed(5); a = model(v, w)
    torch.manual_seed(5); b = model._classif(model.fusion(v, model.seq2vec(w)))
    assert torch.equal(a, b)


def test_engine_equals_torch_adam_loop():
    """Three steps, dropout off, lr 1e-3, against torch autograd + torch.optim.Adam on the same parameters."""
    from neuralcx.vqa_train import VqaTrainEngine
    shape = (64, 132, 96, 44, 40, 40, 10, 100)
    B, dv, dq, dhv, dhq, dz, Rk, A = shape
    rng = np.random.default_rng(8)
    P = R.init_params(9, dv, dq, dhv, dhq, dz, Rk, A, gain=2.0)
    v = (np.abs(rng.standard_normal((B, dv))) * 0.45).astype(np.float32)
    q = (rng.standard_normal((B, dq)) * 0.3).astype(np.float32)
    t = rng.integers(0, A, size=B)
    e = VqaTrainEngine(dv=dv, dq=dq, dhv=dhv, dhq=dhq, dz=dz, R=Rk, A=A, dropout=(0, 0, 0), lr=1e-3, device=DEV)
    for k, x in P.items():
        e.params.views[k].copy_(_t(x))
    Pt = {k: _t(x).requires_grad_(True) for k, x in P.items()}
    opt = torch.optim.Adam(list(Pt.values()), lr=1e-3)
    vt, qt, tt = _t(v), _t(q), _t(t, torch.int64)
    idx = torch.arange(B, dtype=torch.int32, device=DEV)
    for s in range(3):
        xv = torch.tanh(vt @ Pt["wv"].t() + Pt["bv"]); xq = torch.tanh(qt @ Pt["wq"].t() + Pt["bq"])
        z = ((xv @ Pt["whv"].t() + Pt["bhv"]) * (xq @ Pt["whq"].t() + Pt["bhq"])).view(B, Rk, dz).sum(1)
        loss = torch.nn.functional.cross_entropy(z @ Pt["wc"].t() + Pt["bc"], tt)
        opt.zero_grad(); loss.backward()
        r = e.train_step(vt, idx, qt, tt.to(torch.int32))
        assert abs(float(r["loss"]) - float(loss)) <= 1e-5 * max(1.0, float(loss)), s
        if s == 0:
            for k in P:
                ref = Pt[k].grad.cpu().numpy()
                err = np.abs(e.grads.views[k].cpu().numpy() - ref).max()
                assert err <= grad_tol(k, ref), (k, err)
        opt.step()
    # Drift bound: on this same case torch's fp32 CPU trajectory is 5.17e-07 (max over all parameters) from the fp64 restatement's
    # after the 3 steps; 4 x that, and never more than a quarter of 3 lr.
    bound = min(4 * 5.17e-07, 0.25 * 3 * 1e-3)
    drift = max(float((e.params.views[k] - Pt[k].detach()).abs().max()) for k in P)
    print("drift %.3e (bound %.3e)" % (drift, bound))
    assert drift <= bound, drift


TINY_YAML = """
logs: {dir_logs: %s}
vqa: {nans: 40, maxlength: 8}
coco: {}
model:
  arch: MutanNoAtt
  seq2vec: {arch: gru, emb_size: 16, dropout: 0.0, fixed_emb: False}
  fusion: {dim_v: 64, dim_q: 48, dim_hv: 32, dim_hq: 32, dim_mm: 24, R: 3, activation_v: tanh, activation_q: tanh, dropout_v: 0.1, dropout_q: 0.1, dropout_hv: 0, dropout_hq: 0}
  classif: {dropout: 0.1}
optim: {lr: 0.003, batch_size: 64, epochs: 3}
"""
TINY_ARGS = ["--synthetic", "--syn_examples", "384", "--syn_images", "32", "--syn_vocab", "30", "--print_freq", "0", "--freeze_seq2vec"]


def _cli():
    import importlib.util
    spec = importlib.util.spec_from_file_location("vqa_train_cli", os.path.join(PKG, "train.py"))
    mod = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(mod)
    return mod


def test_cli_trains_resumes_and_feeds_the_frozen_producer(tmp_path):
    """train.py --synthetic --freeze_seq2vec (the whole step in HIP) on the seed whose torch path (--no_hip, on a CPU) was checked
    to lower the loss from epoch 1 (3.69) to epoch 3 (3.59): 1337, the default."""
    from neuralcx import ops
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
            cli.main(["--path_opt", str(y), "--epochs", "2"] + TINY_ARGS)
            runs[name] = cli.main(["--path_opt", str(y), "--resume", "ckpt"] + TINY_ARGS)
        for tag in ("ckpt", "best"):
            for part in ("info", "model", "optim"):
                assert os.path.isfile(os.path.join(logs, "%s_%s.pth.tar" % (tag, part))), (name, tag, part)
    h = runs["straight"]["history"]
    assert [x["epoch"] for x in h] == [1, 2, 3] and h[0]["train"]["loss"] > h[2]["train"]["loss"], h
    assert [x["epoch"] for x in runs["resumed"]["history"]] == [1, 2, 3]
    a = torch.load(str(tmp_path / "straight" / "ckpt_model.pth.tar"))
    b = torch.load(str(tmp_path / "resumed" / "ckpt_model.pth.tar"))
    assert set(a) == set(b)
    for k in a:
        assert torch.equal(a[k], b[k]), k                      # --resume ckpt continues bit for bit
    oa, ob = (torch.load(str(tmp_path / n / "ckpt_optim.pth.tar")) for n in ("straight", "resumed"))
    assert oa["step"] == ob["step"] and torch.equal(oa["exp_avg"], ob["exp_avg"]) and torch.equal(oa["exp_avg_sq"], ob["exp_avg_sq"])
    # closing the loop: best_model.pth.tar -> models.factory -> the frozen producer's weights -> the trainer's eval logits
    tr = runs["straight"]["trainer"]
    opt = cli.load_options(cli.build_parser().parse_args(["--path_opt", str(tmp_path / "straight.yaml")]))
    model = models.factory(opt["model"], ["w%d" % i for i in range(30)], ["a%d" % i for i in range(40)], cuda=True)
    best = torch.load(str(tmp_path / "straight" / "best_model.pth.tar"))
    model.load_state_dict(best, strict=True)
    tr.engine.load_state_dict(best)
    sel = torch.arange(0, 48, device=DEV)
    idx, q, aids = tr.val.img_idx[sel], tr.q_emb_of(tr.val)[sel], tr.val.aids[sel]
    want = tr.engine.evaluate(tr.val.feats, idx, q, aids)["logits"]
    a_o, _, _, _ = ops.vqa_forward(tr.val.feats, torch.stack([idx, idx], 1).contiguous(), q.contiguous(), ops.vqa_weights(model.eval()), want_a_orig=True)
    assert (a_o - want).abs().max().item() <= 1e-4 * max(1.0, want.abs().max().item())
