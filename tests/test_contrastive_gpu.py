"""GPU: the contrastive path (ContrastiveModel + ContrastiveLoss, the reference's contrastive.py) -- HIP against the
reference-produced fixture, against the fp64 restatement at full widths and at edge shapes, the gather, the id clamp, determinism,
the device sampler, the drop-in module under the reference-style loop, and the CLI.  Tolerances are the scorers' (test_scorers_gpu.py,
helpers.grad_tol)."""
import os

import numpy as np
import pytest
import torch

import contrastive_ref as R
from conftest import GOLDEN, PKG
from helpers import grad_tol

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g(name="g12_contrastive.npz"):
    return np.load(os.path.join(GOLDEN, name))


def _state(g, tag="init/"):
    return {str(n): g[tag + str(n)] for n in g["init/names"]}


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)


def _batch(feats, z_o, z_k):
    """feats [B, P, dv] -> an ops.Batch over a feature table with shuffled rows (the gather is exercised)."""
    from neuralcx import ops
    B, P, dv = feats.shape
    perm = np.random.default_rng(B * P).permutation(B * P)
    table = np.empty((B * P, dv), np.float32)
    table[perm] = feats.reshape(B * P, dv)
    return ops.Batch(_t(table), _t(perm.reshape(B, P), torch.int32), None, _t(z_o), _t(z_k), None)


def _engine(params=None, lr=1e-3, **cfg):
    from neuralcx.contrastive import ContrastiveEngine
    e = ContrastiveEngine(lr=lr, device=DEV, **cfg)
    if params is not None:
        e.load_state({k: torch.from_numpy(np.asarray(v)) for k, v in params.items()})
    else:
        e.init_parameters(seed=3)
    return e


def _check_grads(e, ref):
    for n, v in ref.items():
        got = e.grads.views[n].detach().cpu().numpy().astype(np.float64)
        assert np.abs(got - v).max() <= grad_tol(n, v), (n, np.abs(got - v).max(), grad_tol(n, v))


def test_parity_with_reference_fixture():
    g, ga = _g(), _g("g12_contrastive_adam.npz")
    e = _engine(_state(g), dv=12, dz=8, A=6)
    emb0 = e.params.views["answer_embedding.weight"].clone()
    b = _batch(g["t/feats"], g["t/z_orig"], g["t/z_knns"])
    h = e.forward(b).cpu().numpy()
    assert np.abs(h - g["t/h"]).max() <= 1e-4 * max(1.0, np.abs(g["t/h"]).max())
    assert not h[0].any()                                                       # the example with three all-zero rows
    r = e.train_step(b)
    for k in ("loss_comp", "loss_other"):
        assert abs(float(r[k]) - float(g["t/" + k])) <= 1e-5 * max(1.0, abs(float(g["t/" + k]))), k
    assert abs(float(r["loss"]) - float(g["t/loss_comp"]) - float(g["t/loss_other"])) <= 2e-5 * max(1.0, float(g["t/loss_other"]))
    d = r["dist"].cpu().numpy()
    for j, k in enumerate(("dist_comp", "dist_other")):
        assert np.abs(d[:, j] - g["t/" + k]).max() <= 1e-4 * max(1.0, np.abs(g["t/" + k]).max()), k
        assert abs(float(r[k]) - g["t/" + k].mean()) <= 1e-4 * max(1.0, g["t/" + k].mean()), k
    _check_grads(e, {n: g["t/grad/" + n] for n in ("linear.weight", "linear.bias")})
    for n, v in e.params.views.items():
        assert np.abs(v.cpu().numpy() - ga["t/step1/" + n]).max() <= 2e-6, n
    e.train_step(b); e.train_step(b)
    for n, v in e.params.views.items():
        assert np.abs(v.cpu().numpy() - ga["t/step3/" + n]).max() <= 1e-5, n
    assert torch.equal(e.params.views["answer_embedding.weight"], emb0)         # bit-unchanged: outside Adam's span
    assert torch.equal(e.state_dict()["answer_embedding.weight"], emb0)


def test_evaluation_parity_with_reference_fixture():
    g = _g()
    e = _engine(_state(g), dv=12, dz=8, A=6)
    b = _batch(g["e/feats"], g["e/z_orig"], g["e/z_knns"])
    h = e.forward(b).cpu().numpy()
    assert np.abs(h - g["e/h"]).max() <= 1e-4 * max(1.0, np.abs(g["e/h"]).max())
    r = e.eval_step(b, _t(g["e/comp"], torch.int32))
    d = r["scores"].cpu().numpy()
    assert d.shape == (8, 24) and np.abs(d - g["e/dist"]).max() <= 1e-4 * max(1.0, np.abs(g["e/dist"]).max())
    assert ((r["rank"].cpu().numpy() < 5).astype(np.int32) == g["e/recall5"]).all()          # the reference's recallAtK(k=5)
    assert int(r["hits"][1]) == int(g["e/recall5"].sum())


def _case(seed, B, P, dv, dz, A=7, tau=2e-5, train=True):
    """Inputs + parameters (biases negative, so an all-zero example exists) conditioned as the fixture: no pre-activation within
    tau of 0; training: no counterexample distance within 1e-3 of the margin, the hinge active and inactive for >= 1/4 each (B >= 8);
    evaluation: gaps around ranks 1/2 and 5/6 above 1e-3.  Offending examples are redrawn."""
    rng = np.random.default_rng(seed)
    e = _engine(dv=dv, dz=dz, A=A)
    params = {k: v.cpu().numpy() for k, v in e.state_dict().items()}
    params["linear.bias"] = -np.abs(params["linear.bias"]) - 0.05
    # input scale per example: the weights are U(+-1/sqrt(fan_in)), so the pre-activations' spread is ~0.6 x scale whatever the
    # widths, and the distances (~14 x that) fall on both sides of the margin
    scale = rng.uniform(0.05, 1.0, B).astype(np.float32)
    scale[0] = 1e-4
    draw = lambda shape, sc: (rng.standard_normal(shape) * sc.reshape((-1,) + (1,) * (len(shape) - 1))).astype(np.float32)
    feats, z_o, z_k = draw((B, P, dv), scale), draw((B, dz), scale), draw((B, P - 1, dz), scale)
    for _ in range(60):
        p, _x = R.pre(feats, z_o, z_k, params)
        bad = (np.abs(p) < tau).any((1, 2))
        d = R.distances(np.maximum(p, 0))
        if train:
            bad |= np.abs(d[:, 0] - 2.0) < 1e-3
        elif P > 2:
            sd = np.sort(d, 1)[:, ::-1]
            bad |= (sd[:, 0] - sd[:, 1]) < 1e-3
            if P > 6:
                bad |= (sd[:, 4] - sd[:, 5]) < 1e-3
        bad[0] = False
        if not bad.any():
            break
        bb = np.nonzero(bad)[0]
        feats[bb], z_o[bb], z_k[bb] = draw((len(bb), P, dv), scale[bb]), draw((len(bb), dz), scale[bb]), draw((len(bb), P - 1, dz), scale[bb])
    else:
        raise AssertionError("conditioning did not converge")
    if train and B >= 8:
        assert (d[:, 0] < 2).sum() >= B // 4 and (d[:, 0] > 2).sum() >= B // 4, ((d[:, 0] < 2).sum(), B)
    assert not np.maximum(p, 0)[0].any()
    return feats, z_o, z_k, params


def _train_check(seed, B, dv, dz):
    feats, z_o, z_k, params = _case(seed, B, 3, dv, dz)
    ref = R.loss_and_grads(feats, z_o, z_k, params)
    e = _engine(params, dv=dv, dz=dz, A=7)
    b = _batch(feats, z_o, z_k)
    h = e.forward(b).cpu().numpy()
    assert np.abs(h - ref["h"]).max() <= 1e-4 * max(1.0, np.abs(ref["h"]).max())
    assert ((h == 0) == (ref["h"] == 0)).all()
    r = e.train_step(b)
    for k in ("loss_comp", "loss_other"):
        assert abs(float(r[k]) - ref[k]) <= 1e-5 * max(1.0, abs(ref[k])), (k, float(r[k]), ref[k])
    d = r["dist"].cpu().numpy()
    assert np.abs(d - ref["dist"]).max() <= 1e-4 * max(1.0, np.abs(ref["dist"]).max())
    _check_grads(e, ref["grads"])
    return e, b


def _eval_check(seed, B, P, dv, dz):
    feats, z_o, z_k, params = _case(seed, B, P, dv, dz, train=False)
    h_ref = R.forward(feats, z_o, z_k, params)
    d_ref = R.distances(h_ref)
    comp = np.random.default_rng(seed + 1).integers(0, P - 1, B).astype(np.int32)
    e = _engine(params, dv=dv, dz=dz, A=7)
    r = e.eval_step(_batch(feats, z_o, z_k), _t(comp, torch.int32))
    d = r["scores"].cpu().numpy()
    assert np.abs(d - d_ref).max() <= 1e-4 * max(1.0, np.abs(d_ref).max())
    rk, rk_ref = r["rank"].cpu().numpy(), R.rank_farthest(d_ref, comp)
    assert ((rk < 1) == (rk_ref < 1)).all() and ((rk < 5) == (rk_ref < 5)).all()          # Recall@1 / @5 indicator vectors
    assert int(r["hits"][0]) == int((rk_ref < 1).sum()) and int(r["hits"][1]) == int((rk_ref < 5).sum())


def test_full_widths_training_step_vs_restatement():
    _train_check(1, 512, 2048, 360)


def test_full_widths_evaluation_vs_restatement():
    _eval_check(2, 512, 25, 2048, 360)


@pytest.mark.parametrize("B", [1, 33, 513])
@pytest.mark.parametrize("dv,dz", [(4, 4), (37, 13), (70, 33)])
def test_training_edge_shapes(B, dv, dz):
    _train_check(B * 7 + dv, B, dv, dz)


@pytest.mark.parametrize("B", [1, 33])
@pytest.mark.parametrize("K", [1, 2, 24, 64])
@pytest.mark.parametrize("dv,dz", [(4, 4), (37, 13)])
def test_evaluation_edge_shapes(B, K, dv, dz):
    _eval_check(B * 11 + K + dv, B, K + 1, dv, dz)


def test_out_of_range_row_id_sets_flag_and_is_clamped():
    from neuralcx import ops
    feats, z_o, z_k, params = _case(4, 16, 3, 36, 12)
    e = _engine(params, dv=36, dz=12, A=7)
    b = _batch(feats, z_o, z_k)
    e.forward(b)
    assert int(e.bad_flag.item()) == 0
    n = b.feats.shape[0]
    idx = b.img_idx.clone()
    lo_row, hi_row = int(idx[2, 1]), int(idx[5, 0])
    idx[2, 1], idx[5, 0] = -7, n + 1000
    bad = ops.Batch(b.feats, idx, None, b.z_orig, b.z_knns, None)
    h_bad = e.forward(bad)
    torch.cuda.synchronize()
    assert int(e.bad_flag.item()) == 1
    clamped = b.img_idx.clone(); clamped[2, 1], clamped[5, 0] = 0, n - 1
    e2 = _engine(params, dv=36, dz=12, A=7)
    h_clamped = e2.forward(ops.Batch(b.feats, clamped, None, b.z_orig, b.z_knns, None))
    assert torch.equal(h_bad, h_clamped) and int(e2.bad_flag.item()) == 0
    e.train_step(bad)                                            # the backward gathers through the clamped ids too
    torch.cuda.synchronize()
    assert torch.isfinite(e.grads.flat).all()
    with pytest.raises(IndexError):
        e.check_ids()
    e.check_ids()                                                # cleared
    assert (lo_row, hi_row) != (0, n - 1)


def test_bit_identical_runs():
    feats, z_o, z_k, params = _case(5, 512, 3, 2048, 360)
    b = _batch(feats, z_o, z_k)
    out = []
    for _ in range(2):
        e = _engine(params, dv=2048, dz=360, A=7)
        r = e.train_step(b)
        g1 = e.grads.flat.cpu().clone()
        e.train_step(b)
        out.append((r["loss_comp"].cpu().clone(), r["loss_other"].cpu().clone(), r["dist"].cpu().clone(), g1, e.params.flat.cpu().clone()))
    for x, y in zip(*out):
        assert torch.equal(x, y)


def test_device_sampler():
    from neuralcx.contrastive import sample_positions, triple_batch
    K, B = 24, 24 * 1024
    gt = (torch.arange(B, device=DEV) % K).to(torch.int32)
    gen = torch.Generator(device=DEV); gen.manual_seed(42)
    pos = sample_positions(gt, K, gen)
    assert pos.is_cuda and torch.equal(pos[:, 0], gt.long())
    other = pos[:, 1]
    assert bool((other != gt.long()).all()) and int(other.min()) >= 0 and int(other.max()) <= K - 1
    for c in range(K):          # 1024 draws per c: P(any position missed) <= 24 . 23 . (22/23)^1024 ~ 1e-17
        assert set(other[gt == c].tolist()) == set(range(K)) - {c}, c
    gen2 = torch.Generator(device=DEV); gen2.manual_seed(42)
    assert torch.equal(pos, sample_positions(gt, K, gen2))
    assert not torch.equal(pos, sample_positions(gt, K, gen2))                  # the next step draws afresh
    # the P = 3 batch: [orig, comp, other] rows and the two neighbours' z
    n = 512
    img = torch.randint(0, 1000, (n, K + 1), device=DEV, dtype=torch.int32)
    z_o, z_k = torch.randn(n, 8, device=DEV), torch.randn(n, K, 8, device=DEV)
    gen3 = torch.Generator(device=DEV); gen3.manual_seed(1)
    gen4 = torch.Generator(device=DEV); gen4.manual_seed(1)
    b3 = triple_batch(torch.zeros(1000, 4, device=DEV), img, z_o, z_k, gt[:n], gen3)
    p = sample_positions(gt[:n], K, gen4)
    ar = torch.arange(n, device=DEV)
    assert b3.img_idx.shape == (n, 3) and b3.img_idx.dtype == torch.int32
    assert torch.equal(b3.img_idx[:, 0], img[:, 0]) and torch.equal(b3.img_idx[:, 1], img[ar, p[:, 0] + 1]) and \
        torch.equal(b3.img_idx[:, 2], img[ar, p[:, 1] + 1])
    assert torch.equal(b3.z_knns, torch.stack([z_k[ar, p[:, 0]], z_k[ar, p[:, 1]]], 1)) and torch.equal(b3.z_orig, z_o)


class _StubVQA(torch.nn.Module):
    def __init__(self, dv, dq, dz, A):
        super().__init__()
        self.opt = {"fusion": {"dim_v": dv, "dim_q": dq, "dim_mm": dz}}
        self.vocab_answers = ["a%d" % i for i in range(A)]


class _ContrastiveLoss(torch.nn.Module):
    """ContrastiveLoss of contrastive.py:293-309, restated ([B] distances: the same mean and gradient as the reference's [B, 1]
    against a constant label vector)."""

    def __init__(self, margin=2.0):
        super().__init__()
        self.margin = margin

    def forward(self, output1, output2, label):
        d = torch.nn.functional.pairwise_distance(output1, output2)
        return torch.mean((1 - label) * torch.pow(d, 2) + label * torch.pow(torch.clamp(self.margin - d, min=0.0), 2))


def test_dropin_module_reference_loop_against_fixture():
    from vqa.models.cx import ContrastiveModel
    g, ga = _g(), _g("g12_contrastive_adam.npz")
    m = ContrastiveModel(_StubVQA(12, 4, 8, 6), knn_size=2).to(DEV)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state(g).items()}, strict=False)
    m.vqa_forward = lambda image_features, wids: (None, _t(g["t/z_orig"]), None, _t(g["t/z_knns"]), None)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    crit = _ContrastiveLoss().to(DEV)
    B = g["t/feats"].shape[0]
    feats = _t(g["t/feats"])
    for step in range(1, 4):                                       # the reference's loop (contrastive.py:215-224)
        h_out = m(feats, None, None)
        loss_comp = crit(h_out[:, 0], h_out[:, 1], label=torch.ones([B], device=DEV))
        loss_other = crit(h_out[:, 0], h_out[:, 2], label=torch.zeros([B], device=DEV))
        loss = loss_comp + loss_other
        opt.zero_grad()
        loss.backward()
        if step == 1:
            assert h_out.shape == (B, 3, 300)
            assert np.abs(h_out.detach().cpu().numpy() - g["t/h"]).max() <= 1e-4 * max(1.0, np.abs(g["t/h"]).max())
            assert abs(loss_comp.item() - float(g["t/loss_comp"])) <= 1e-5 and \
                abs(loss_other.item() - float(g["t/loss_other"])) <= 1e-5 * max(1.0, float(g["t/loss_other"]))
            assert m.answer_embedding.weight.grad is None
            for n in ("linear.weight", "linear.bias"):
                ref = g["t/grad/" + n]
                got = dict(m.named_parameters())[n].grad.cpu().numpy()
                assert np.abs(got - ref).max() <= grad_tol(n, ref), n
            dists = m.get_scores(h_out[:, 0], h_out[:, 1:])
            assert dists.is_cuda and dists.shape == (B, 2)
            assert np.abs(dists.cpu().numpy()[:, 0] - g["t/dist_comp"]).max() <= 1e-4 * max(1.0, g["t/dist_comp"].max())
        opt.step()
        if step in (1, 3):
            for n, v in m.state_dict().items():
                assert np.abs(v.cpu().numpy() - ga["t/step%d/" % step + n]).max() <= (2e-6 if step == 1 else 1e-5), (step, n)
    # knn_size flips to 24 for evaluation (contrastive.py:270) on the same module
    m.knn_size = 24
    m.load_state_dict({k: torch.from_numpy(v) for k, v in _state(g).items()}, strict=False)
    m.vqa_forward = lambda image_features, wids: (None, _t(g["e/z_orig"]), None, _t(g["e/z_knns"]), None)
    with torch.no_grad():
        h = m(_t(g["e/feats"]), None, None)
    s = m.get_scores(h[:, 0], h[:, 1:]).cpu().numpy()
    assert np.abs(s - g["e/dist"]).max() <= 1e-4 * max(1.0, np.abs(g["e/dist"]).max())
    assert ((R.rank_farthest(s, g["e/comp"]) < 5).astype(np.int32) == g["e/recall5"]).all()
    hid = m.get_hidden(_t(g["e/feats"][:, 3]), _t(g["e/z_knns"][:, 2]))
    assert np.abs(hid.detach().cpu().numpy() - g["e/h"][:, 3]).max() <= 1e-4 * max(1.0, np.abs(g["e/h"]).max())


def test_cli_trains_checkpoints_and_resumes(tmp_path, capsys):
    import contrastive as cli
    common = ["--synthetic", "-b", "64", "--syn_train", "256", "--syn_val", "128", "--syn_images", "1024", "-p", "2", "--max_steps", "3"]
    d = str(tmp_path)
    res = cli.main(common + ["--epochs", "1", "--project_dir", d])
    out = capsys.readouterr().out
    for name in cli.TRAIN_METRICS + (cli.RECALL_KEY,):
        assert name + ":" in out, name
    assert "Epoch 1 train:" in out and "Epoch 1 val:" in out and "Epoch 0 test:" in out
    assert 0.0 <= res[cli.RECALL_KEY] <= 1.0
    run = os.listdir(os.path.join(d, "logs", "cx"))[0]
    for sub in ("ckpt", "best"):
        assert os.path.isfile(os.path.join(d, "logs", "cx", run, sub, "info.ckpt")) or sub == "best"
    s1 = torch.load(os.path.join(d, "logs", "cx", run, "ckpt", "model.ckpt"))
    assert {k: tuple(v.shape) for k, v in s1.items()} == {"answer_embedding.weight": (2000, 300), "linear.weight": (300, 2048 + 360),
                                                          "linear.bias": (300,)}
    info = torch.load(os.path.join(d, "logs", "cx", run, "ckpt", "info.ckpt"))
    assert len(info) == 1 and 0.0 <= info[0][cli.RECALL_KEY] <= 1.0
    assert os.path.isfile(os.path.join(d, "runs", run, "train.jsonl")) and os.path.isfile(os.path.join(d, "runs", run, "val.jsonl"))
    cli.main(common + ["--epochs", "2", "--project_dir", d, "--resume", run])
    out = capsys.readouterr().out
    assert "Epoch 2 val:" in out and "Epoch 1 val" not in out
    s2 = torch.load(os.path.join(d, "logs", "cx", run, "ckpt", "model.ckpt"))
    assert len(torch.load(os.path.join(d, "logs", "cx", run, "ckpt", "info.ckpt"))) == 2
    assert not torch.equal(s1["linear.weight"], s2["linear.weight"])              # it trained
    assert torch.equal(s1["answer_embedding.weight"], s2["answer_embedding.weight"])
    # a checkpoint whose info carries the key the reference READS ('recall') resumes too
    torch.save([{"recall": 0.5}], os.path.join(d, "logs", "cx", run, "ckpt", "info.ckpt"))
    cli.main(common + ["--epochs", "2", "--project_dir", d, "--resume", run])
    assert "Epoch 2 val:" in capsys.readouterr().out
