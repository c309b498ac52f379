"""GPU: the trainable scorers LinearContext and PairwiseLinearModel -- HIP against the reference-produced fixture, against the
fp64 restatement at full widths and at edge shapes, determinism, the drop-in modules under torch.optim.Adam, and the CLI."""
import os

import numpy as np
import pytest
import torch

import scorers_ref as R
from conftest import GOLDEN, PKG
from helpers import grad_tol
from oracle.ncx_oracle import rank_of_gt

pytestmark = pytest.mark.gpu
DEV = "cuda:0"


def _g(name="g11_scorers.npz"):
    return np.load(os.path.join(GOLDEN, name))


def _state(g, prefix, tag="init/"):
    return {str(n): g[prefix + tag + str(n)] for n in g[prefix + "init/names"]}


def _batch(feats, q, z_o, z_k, aids):
    """feats [B, K+1, dv] -> an ops.Batch over a feature table with shuffled rows (the gather is exercised)."""
    from neuralcx import ops
    B, K1, dv = feats.shape
    perm = np.random.default_rng(B * K1).permutation(B * K1)
    table = np.empty((B * K1, dv), np.float32)
    table[perm] = feats.reshape(B * K1, dv)
    t = lambda a, dt=torch.float32: torch.from_numpy(np.ascontiguousarray(a)).to(DEV, dt)
    return ops.Batch(t(table), t(perm.reshape(B, K1), torch.int32), t(q), t(z_o), t(z_k), t(z_k), t(aids, torch.int32))


def _engine(kind, g=None, prefix=None, lr=1e-3, **cfg):
    from neuralcx.scorers import LinearContextEngine, PairwiseLinearEngine
    e = PairwiseLinearEngine(lr=lr, device=DEV, **cfg) if kind == "pl" else LinearContextEngine(lr=lr, device=DEV, **cfg)
    if g is not None:
        e.load_state({k: torch.from_numpy(v) for k, v in _state(g, prefix).items()})
    else:
        e.init_parameters(seed=3)
    return e


def _check_grads(grads, ref):
    for n, v in ref.items():
        got = grads[n].detach().cpu().numpy().astype(np.float64)
        assert np.abs(got - v).max() <= grad_tol(n, v), (n, np.abs(got - v).max(), grad_tol(n, v))


@pytest.mark.parametrize("kind", ["lc", "pl"])
def test_parity_with_reference_fixture(kind):
    g, ga = _g(), _g("g11_scorers_adam.npz")
    p = kind + "/"
    if kind == "pl":
        b = _batch(g[p + "feats"], g[p + "q_emb"], g[p + "z_orig"], g[p + "z_knns"], g[p + "aids"])
        e = _engine("pl", g, p, K=24, dv=4, dq=4, dz=4, A=10)
    else:
        B, K, dz = g[p + "z_knns"].shape
        b = _batch(np.zeros((B, K + 1, 4), np.float32), np.zeros((B, 4), np.float32), np.zeros((B, dz), np.float32),
                   g[p + "z_knns"], np.zeros(B, np.int32))
        e = _engine("lc", g, p, K=K, dz=dz)
    gt = torch.from_numpy(g[p + "gt"]).to(DEV)
    r = e.train_step(b, gt)
    s = r["scores"].cpu().numpy()
    assert np.abs(s - g[p + "scores"]).max() <= 1e-4
    assert abs(float(r["loss"][0]) - float(g[p + "loss"])) <= 1e-5
    _check_grads({n: v for n, v in e.grads.views.items()}, {n: g[p + "grad/" + n] for n in e.grads.views})
    if kind == "pl":
        assert (s[0] == 0).all() and (s[4] == 0).all()
        ge = e.grads.views["answer_embedding.weight"].cpu().numpy()
        assert not ge[[1, 3, 4, 6, 8, 9]].any()
    rank = r["rank"].cpu().numpy()
    assert (rank == rank_of_gt(g[p + "scores"], g[p + "gt"])).all()
    for n, v in e.params.views.items():
        assert np.abs(v.cpu().numpy() - ga[p + "step1/" + n]).max() <= 2e-6, n
    e.train_step(b, gt); e.train_step(b, gt)
    for n, v in e.params.views.items():
        assert np.abs(v.cpu().numpy() - ga[p + "step3/" + n]).max() <= 1e-5, n


def _pl_case(seed, B, K, dv, dq, dz, A, tau=2e-5, params=None):
    """Inputs + parameters with no hidden or score pre-activation within tau of 0 (candidate rows re-drawn until so)."""
    rng = np.random.default_rng(seed)
    feats = (rng.standard_normal((B, K + 1, dv)) * 0.45).astype(np.float32)
    q = (rng.standard_normal((B, dq)) * 0.45).astype(np.float32)
    z_o = (rng.standard_normal((B, dz)) * 0.45).astype(np.float32)
    z_k = (rng.standard_normal((B, K, dz)) * 0.45).astype(np.float32)
    aids = rng.integers(0, A, B).astype(np.int32)
    if B > 2:
        aids[1] = aids[2]
    if params is None:
        e = _engine("pl", K=K, dv=dv, dq=dq, dz=dz, A=A)
        params = {k: v.cpu().numpy() for k, v in e.state_dict().items()}
    for _ in range(40):
        pre_h, pre_s = R.pairlin_pre(feats, q, z_o, z_k, aids, params)
        bad = (np.abs(pre_h) < tau).any(2) | (np.abs(pre_s) < tau)
        if not bad.any():
            break
        bb, kk = np.nonzero(bad)
        feats[bb, kk + 1] = (rng.standard_normal((len(bb), dv)) * 0.45).astype(np.float32)
        z_k[bb, kk] = (rng.standard_normal((len(bb), dz)) * 0.45).astype(np.float32)
    else:
        raise AssertionError("conditioning did not converge")
    gt = rng.integers(0, K, B).astype(np.int32)
    return feats, q, z_o, z_k, aids, gt, params


def _pl_check(seed, B, K, dv, dq, dz, A):
    feats, q, z_o, z_k, aids, gt, params = _pl_case(seed, B, K, dv, dq, dz, A)
    s_ref, loss_ref, g_ref, _, _ = R.pairlin(feats, q, z_o, z_k, aids, params, gt)
    e = _engine("pl", K=K, dv=dv, dq=dq, dz=dz, A=A)
    e.load_state({k: torch.from_numpy(v) for k, v in params.items()})
    r = e.train_step(_batch(feats, q, z_o, z_k, aids), torch.from_numpy(gt).to(DEV))
    s = r["scores"].cpu().numpy()
    assert np.abs(s - s_ref).max() <= 1e-4 * max(1.0, np.abs(s_ref).max())
    assert ((s == 0) == (s_ref == 0)).all()
    assert abs(float(r["loss"][0]) - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    _check_grads(e.grads.views, g_ref)
    rk = r["rank"].cpu().numpy()
    rk_ref = rank_of_gt(s_ref, gt)
    assert ((rk < 1) == (rk_ref < 1)).all() and ((rk < 5) == (rk_ref < 5)).all()
    return e


def test_pairwise_linear_full_widths_vs_restatement():
    _pl_check(1, 512, 24, 2048, 2400, 360, 2000)


@pytest.mark.parametrize("B", [1, 33, 513])
@pytest.mark.parametrize("K,dv,dq,dz", [(3, 36, 20, 12), (64, 37, 21, 13)])
def test_pairwise_linear_edge_shapes(B, K, dv, dq, dz):
    _pl_check(B * 7 + K, B, K, dv, dq, dz, 17)


@pytest.mark.parametrize("B", [1, 33, 513])
@pytest.mark.parametrize("K,dz", [(3, 13), (24, 360), (64, 12)])
def test_linear_context_vs_restatement(B, K, dz):
    rng = np.random.default_rng(B + K + dz)
    z = rng.standard_normal((B, K, dz)).astype(np.float32)
    gt = rng.integers(0, K, B).astype(np.int32)
    e = _engine("lc", K=K, dz=dz)
    params = {k: v.cpu().numpy() for k, v in e.state_dict().items()}
    s_ref, loss_ref, g_ref = R.linctx(z, params, gt)
    b = _batch(np.zeros((B, K + 1, 4), np.float32), np.zeros((B, 4), np.float32), np.zeros((B, dz), np.float32), z, np.zeros(B, np.int32))
    r = e.train_step(b, torch.from_numpy(gt).to(DEV))
    assert np.abs(r["scores"].cpu().numpy() - s_ref).max() <= 1e-4 * max(1.0, np.abs(s_ref).max())
    assert abs(float(r["loss"][0]) - loss_ref) <= 1e-5 * max(1.0, abs(loss_ref))
    _check_grads(e.grads.views, g_ref)


def test_bit_identical_runs():
    feats, q, z_o, z_k, aids, gt, params = _pl_case(5, 512, 24, 2048, 2400, 360, 2000)
    b = _batch(feats, q, z_o, z_k, aids)
    out = []
    for _ in range(2):
        for kind in ("pl", "lc"):
            e = _engine(kind, K=24, dz=360, **(dict(dv=2048, dq=2400, A=2000) if kind == "pl" else {}))
            r = e.train_step(b, torch.from_numpy(gt).to(DEV))
            e.train_step(b, torch.from_numpy(gt).to(DEV))
            out.append((r["scores"].cpu().clone(), e.grads.flat.cpu().clone(), e.params.flat.cpu().clone()))
    for a, c in zip(out[:2], out[2:]):
        for x, y in zip(a, c):
            assert torch.equal(x, y)


class _StubVQA(torch.nn.Module):
    def __init__(self, dv, dq, dz, A):
        super().__init__()
        self.opt = {"fusion": {"dim_v": dv, "dim_q": dq, "dim_mm": dz}}
        self.vocab_answers = ["a%d" % i for i in range(A)]


@pytest.mark.parametrize("kind", ["pl", "lc"])
def test_dropin_adam_loop_equals_engine(kind):
    from vqa.models.cx import LinearContext, PairwiseLinearModel
    K, dv, dq, dz, A = 24, 64, 48, 40, 50
    feats, q, z_o, z_k, aids, gt, params = _pl_case(9, 64, K, dv, dq, dz, A)
    vqa = _StubVQA(dv, dq, dz, A)
    m = (PairwiseLinearModel(vqa, knn_size=K) if kind == "pl" else LinearContext(vqa, knn_size=K)).to(DEV)
    t = lambda a: torch.from_numpy(a).to(DEV)
    m.vqa_forward = lambda image_features, wids: (None, t(z_o), None, t(z_k), t(q))
    e = _engine(kind, K=K, dz=dz, **(dict(dv=dv, dq=dq, A=A) if kind == "pl" else {}))
    m.load_state_dict({k: v for k, v in e.state_dict().items()}, strict=False)
    opt = torch.optim.Adam(m.parameters(), lr=1e-3)
    crit = torch.nn.CrossEntropyLoss(reduction="sum")
    b = _batch(feats, q, z_o, z_k, aids)
    names = dict(m.named_parameters())
    for step in range(3):                                           # the reference's loop (counterexamples.py:330-339)
        scores = m(t(feats), None, t(aids.astype(np.int64)))
        loss = crit(scores, t(gt.astype(np.int64))) / len(gt)
        opt.zero_grad()
        loss.backward()
        opt.step()
        r = e.train_step(b, t(gt))
        assert abs(loss.item() - float(r["loss"][0])) <= 1e-5 * max(1.0, loss.item()), step
        if step == 0:
            # same parameters on both sides: the autograd wiring hands the HIP gradients to torch unchanged (up to the fp32
            # rounding of CrossEntropyLoss vs ncx_loss_rank in dscores).  (The two Adams themselves agree on equal gradients:
            # test_parity_with_reference_fixture pins ncx_adam_step to torch.optim.Adam's first step at 2e-6.)
            assert torch.equal(scores.detach(), r["scores"])
            for n, v in e.grads.views.items():
                ref = v.cpu().numpy()
                # (the suite's gradient bound: out.bias is a sum of 1536 dscores with cancellation, so the last-bit
                # differences of the two dscores reach ~3e-5 of it)
                assert np.abs(names[n].grad.cpu().numpy() - ref).max() <= grad_tol(n, ref), n
        else:
            # (the two Adams round differently in fp32; m / sqrt(v) carries that into the next forward)
            d = (scores.detach() - r["scores"]).abs().max().item()
            assert d <= 1e-4 * max(1.0, r["scores"].abs().max().item()), (step, d)
    sd = m.state_dict()
    for n, v in e.state_dict().items():
        # The two sides' gradients differ in the last bits (dscores from two loss implementations; from step 2 on, parameters
        # too).  Adam's m / (sqrt(v) + eps) turns a last-bit difference of a gradient entry whose magnitude is near eps (1e-8)
        # into a fraction of a step (lr = 1e-3) on that entry: measured 3.3e-5 after one step and up to 1.4e-4
        # (PairwiseLinearModel, linear.weight) after 3 steps
        dd = (sd[n] - v).abs()
        assert dd.max().item() <= ADAM_DRIFT, (n, dd.max().item())


ADAM_DRIFT = 2.5e-4     # parameter bound after 3 steps of two fp32 trajectories whose gradients differ only in rounding (above)


def _dp_case():
    K, dv, dq, dz, A, Bg = 24, 32, 16, 8, 20, 12
    feats, q, z_o, z_k, aids, gt, params = _pl_case(21, Bg, K, dv, dq, dz, A)
    return dict(K=K, dv=dv, dq=dq, dz=dz, A=A), (feats, q, z_o, z_k, aids, gt), params


def _dp_run(kind, rank, world):
    """Three engine steps: two on the global batch of 12 triplets (sharded over the ranks), then a short global batch of 5
    that rank 0 holds alone while rank 1 runs a zero-weight padding triplet (active = False, dp.epoch_plan)."""
    import torch.distributed as dist
    from neuralcx import dp
    cfg, (feats, q, z_o, z_k, aids, gt), params = _dp_case()
    if kind == "pl":
        e = _engine("pl", world_size=world, **cfg)
        e.load_state({k: torch.from_numpy(v) for k, v in params.items()})
    else:
        e = _engine("lc", world_size=world, K=cfg["K"], dz=cfg["dz"])
    e.rank = rank
    out = dict(losses=[], grads=[])
    for ids, gb, pad in ((list(range(12)), 12, False), (list(range(12)), 12, False), (list(range(5)), 5, True)):
        if world == 1:
            mine, active = ids, True
        elif pad:
            mine, active = (ids, True) if rank == 0 else ([0], False)
        else:
            mine, active = dp.shard(ids, rank, world), True
        sl = np.asarray(mine)
        b = _batch(feats[sl], q[sl], z_o[sl], z_k[sl], aids[sl])
        r = e.train_step(b, torch.from_numpy(gt[sl]).to(DEV), global_batch=gb, active=active)
        e.flush()
        loss = torch.tensor([float(r["loss"][0])], dtype=torch.float64)
        if world > 1:
            dist.all_reduce(loss)                       # sum of the 1 / B_global-scaled local losses
        out["losses"].append(float(loss))
        out["grads"].append({k: v.cpu().numpy().copy() for k, v in e.grads.views.items()})
    out["params"] = {k: v.cpu().numpy() for k, v in e.state_dict().items()}
    return out


def _dp_scorer_worker(rank, world, port, q, kind):
    import os, sys
    os.environ.update(MASTER_ADDR="127.0.0.1", MASTER_PORT=str(port), RANK=str(rank), WORLD_SIZE=str(world), LOCAL_RANK="0")
    from conftest import PKG, ROOT
    sys.path[:0] = [ROOT, PKG, os.path.join(ROOT, "tests")]
    import torch.distributed as dist
    from neuralcx import dp
    dp.init_distributed(backend="gloo")
    out = _dp_run(kind, rank, world)
    if rank == 0:
        q.put(out)
    dist.barrier(); dist.destroy_process_group()


@pytest.mark.parametrize("kind", ["pl", "lc"])
def test_dp2_engine_equals_dp1(kind):
    """Two gloo ranks on one card (pattern of test_dropin_gpu.py::test_dp2_hip_engine_equals_dp1) == one rank on the joined
    batch: loss scale 1 / B_global, the all_reduce of the flat gradient before Adam, and a step where rank 1 holds only a
    padding triplet."""
    import torch.multiprocessing as mp
    ctx = mp.get_context("spawn")
    q = ctx.Queue()
    port = 29900 + os.getpid() % 80 + (kind == "lc") * 90
    procs = [ctx.Process(target=_dp_scorer_worker, args=(r, 2, port, q, kind)) for r in range(2)]
    [p.start() for p in procs]
    dp2 = q.get(timeout=240)
    [p.join(120) for p in procs]
    assert all(p.exitcode == 0 for p in procs)
    dp1 = _dp_run(kind, 0, 1)
    for step in range(3):
        assert abs(dp2["losses"][step] - dp1["losses"][step]) <= 1e-5, step
        for k, ref in dp1["grads"][step].items():
            # step 1: summation order only; later steps also see the last-bit parameter drift of ADAM_DRIFT's comment
            assert np.abs(dp2["grads"][step][k] - ref).max() <= grad_tol(k, ref, 1e-5 if step == 0 else 1e-4), (step, k)
    for k, ref in dp1["params"].items():
        assert np.abs(dp2["params"][k] - ref).max() <= ADAM_DRIFT, k


@pytest.mark.parametrize("model", ["LinearContext", "PairwiseLinearModel"])
def test_cli_trains_checkpoints_and_resumes(tmp_path, capsys, model):
    import counterexamples as cli
    common = ["--synthetic", "-cx", model, "--path_opt", os.path.join(PKG, "options", "cx", "neuralcx_256_1_all.yaml"), "-b", "64",
              "--syn_train", "192", "--syn_val", "64", "--syn_images", "1024", "-p", "100"]
    d_full, d_res = os.path.join(str(tmp_path), "full"), os.path.join(str(tmp_path), "res")
    cli.main(common + ["--epochs", "2", "--project_dir", d_full])
    cli.main(common + ["--epochs", "1", "--project_dir", d_res])
    run = os.listdir(os.path.join(d_res, "logs", "cx"))[0]
    s1 = torch.load(os.path.join(d_res, "logs", "cx", run, "ckpt", "model.ckpt"))
    keys = {"LinearContext": {"linear.weight": (24, 24 * 360), "linear.bias": (24,)},
            "PairwiseLinearModel": {"answer_embedding.weight": (2000, 300), "linear.weight": (300, 2 * 2048 + 2400 + 2 * 360 + 300),
                                    "linear.bias": (300,), "out.weight": (1, 300), "out.bias": (1,)}}[model]
    assert {k: tuple(v.shape) for k, v in s1.items()} == keys
    capsys.readouterr()
    cli.main(common + ["--epochs", "2", "--project_dir", d_res, "--resume", run])
    out = capsys.readouterr().out
    assert "Epoch 2 val: loss:" in out and "Epoch 1 val" not in out
    run_full = os.listdir(os.path.join(d_full, "logs", "cx"))[0]
    s_full = torch.load(os.path.join(d_full, "logs", "cx", run_full, "ckpt", "model.ckpt"))
    s_res = torch.load(os.path.join(d_res, "logs", "cx", run, "ckpt", "model.ckpt"))
    for k in s_full:
        assert torch.equal(s_full[k], s_res[k]), k
    assert not torch.equal(s1["linear.weight"], s_res["linear.weight"])       # it trained
