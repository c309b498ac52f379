"""GPU: the MLB no-attention producer in HIP (ncx_mlb_forward) against the reference's fixture, the module's torch path and the fp64
restatement (tests/mlb_ref.py).  Tolerances are the MUTAN producer's own (tests/test_dropin_gpu.py): 1e-4 max(1, max|ref|) against the
golden fixture (and against the module's fp32 torch path), 1e-4 max|ref| against the restatement."""
import os

import numpy as np
import pytest
import torch

from conftest import PKG
from mlb_ref import mlb_vqa_forward
from test_mlb_cpu import OUTS, load_case, mlb_opt

pytestmark = pytest.mark.gpu
DEV = torch.device("cuda:0")
MLB_YAML = os.path.join(PKG, "options", "cx", "neuralcx_256_1_all_mlb.yaml")


def _factory(dv, dq, dh, A, act_c="tanh", n_words=10, **fusion_over):
    import vqa.models as M
    return M.factory(mlb_opt(dv, dq, dh, act_c, **fusion_over), ["w%d" % i for i in range(n_words)], ["a%d" % i for i in range(A)],
                     cuda=True, data_parallel=False).eval()


def _state(vqa):
    return {k: v.detach().cpu().numpy() for k, v in vqa.state_dict().items() if not k.startswith("seq2vec.")}


def _check(got, ref, tol_floor, what):
    """max|got - ref| <= 1e-4 max(tol_floor, max|ref|); prints the figure before it asserts."""
    for g, r, key in zip(got, ref, OUTS):
        g = g.detach().cpu().numpy() if isinstance(g, torch.Tensor) else g
        r = r.detach().cpu().numpy() if isinstance(r, torch.Tensor) else r
        assert g.shape == r.shape, (what, key, g.shape, r.shape)
        err, mx = float(np.abs(g - r).max()), float(np.abs(r).max())
        print("%s %s: max err %.3e, max|ref| %.3e" % (what, key, err, mx))
        assert np.isfinite(g).all() and err <= 1e-4 * max(tol_floor, mx), (what, key, err, mx)


@pytest.mark.parametrize("name", ["c0", "c1"])
def test_hip_mlb_forward_vs_golden(name):
    """The outputs the reference's own MLBNoAtt produced through its vqa_forward, from the feature table + image ids."""
    from neuralcx import ops
    c = load_case(name)
    dv, dq, dh, A, B, K = (int(x) for x in c["dims"])
    vqa = _factory(dv, dq, dh, A, c["act_c"])
    vqa.load_state_dict({k: torch.from_numpy(v) for k, v in c["state"].items() if not k.startswith("seq2vec.")}, strict=False)
    mw = ops.vqa_weights(vqa)
    assert isinstance(mw, ops.MlbWeights)
    t = lambda k: torch.from_numpy(c[k]).to(DEV)
    got = ops.vqa_forward(t("feats"), t("img_idx"), t("q_emb"), mw, want_a_orig=True)
    _check(got, [c[k] for k in OUTS], 1.0, "golden " + name)


def _torch_and_hip(m, feats, wids):
    m.use_hip_vqa = True
    hip = m.vqa_forward(feats, wids)
    m.use_hip_vqa = False
    ref = m.vqa_forward(feats, wids)
    m.use_hip_vqa = True
    return hip, ref


def test_hip_mlb_forward_full_widths_vs_torch_module_and_restatement():
    """dv 2048, dq 2400, dh 1200, 2000 answers, B = 64: against the same module's torch path (use_hip_vqa = False), against the fp64
    restatement fed the module's weights and the q_emb its encoder produced, and NeuralModel scores through both producers."""
    from vqa.models.cx import NeuralModel
    torch.manual_seed(2)
    vqa = _factory(2048, 2400, 1200, 2000, n_words=50)
    spec = dict(v_emb=True, v_mult=True, v_dist=True, v_rank=True, q_emb=True, a_emb=True, z_emb=True)
    m = NeuralModel(model_spec=spec, dim_h=256, n_layers=1, emb=None, drop_p=0.25, vqa_model=vqa, knn_size=24, trainable_vqa=False).cuda().eval()
    assert m.dim_z == 1200
    B = 64
    feats = torch.randn(B, 25, 2048, device=DEV).abs() * 0.45
    wids = torch.randint(1, 51, (B, 26), device=DEV)
    aids = torch.randint(0, 2000, (B,), device=DEV)
    hip, ref = _torch_and_hip(m, feats, wids)
    assert torch.equal(hip[4], ref[4])
    _check(hip[:4], ref[:4], 1.0, "full widths vs torch path")
    idx = np.arange(B * 25).reshape(B, 25)
    o_ref = mlb_vqa_forward(_state(vqa), feats.reshape(B * 25, -1).cpu().numpy(), idx, hip[4].detach().cpu().numpy(), act_c="tanh")
    _check(hip[:4], o_ref, 0.0, "full widths vs fp64 restatement")
    s_hip = m(feats, wids, aids)
    m.use_hip_vqa = False
    s_ref = m(feats, wids, aids)
    err = float((s_hip - s_ref).detach().abs().max())
    print("NeuralModel scores through both producers: max diff %.3e" % err)
    assert err <= 1e-4


def test_hip_mlb_forward_full_batch_rows_of_32_questions():
    """B = 512 at full widths from a shared feature table: every row (original + 24 candidates, z and logits) of 32 questions spread over
    the batch, first and last included, against the fp64 restatement."""
    from neuralcx import ops
    torch.manual_seed(3)
    B, K1, n_img = 512, 25, 9000
    vqa = _factory(2048, 2400, 1200, 2000)
    mw = ops.vqa_weights(vqa)
    feats = torch.randn(n_img, 2048, device=DEV).abs() * 0.45
    idx = torch.randint(0, n_img, (B, K1), device=DEV, dtype=torch.int32)
    q = torch.randn(B, 2400, device=DEV) * 0.3
    got = ops.vqa_forward(feats, idx, q, mw, want_a_orig=True)
    sel = np.linspace(0, B - 1, 32).round().astype(np.int64)
    assert len(set(sel.tolist())) == 32 and sel[0] == 0 and sel[-1] == B - 1
    ref = mlb_vqa_forward(_state(vqa), feats.cpu().numpy(), idx.cpu().numpy()[sel], q.cpu().numpy()[sel], act_c="tanh")
    _check([g[torch.from_numpy(sel).to(DEV)] for g in got], ref, 0.0, "B = 512, 32 questions")


@pytest.mark.parametrize("B,dv,dh,A,act_c,want_a_orig", [
    (13, 96, 28, 52, "tanh", True),       # fused kernel, dh below one tile, partial row tile
    (70, 96, 44, 40, None, False),        # no classif.activation: the classifier reads z itself; a_orig not requested
    (13, 72, 44, 40, "tanh", False),      # dv not a multiple of 32: x_v on the generic engine + k_mlb_mul
    (70, 100, 28, 42, None, True),        # generic engine for x_v AND the classifier (A not a multiple of 4)
    (13, 96, 44, 42, "tanh", True),       # fused x_v, generic classifier
])
def test_hip_mlb_forward_ragged_shapes(B, dv, dh, A, act_c, want_a_orig):
    from neuralcx import ops
    torch.manual_seed(11 + B + dv)
    vqa = _factory(dv, 48, dh, A, act_c)
    mw = ops.vqa_weights(vqa)
    K1 = 25
    feats = torch.randn(B * K1 + 3, dv, device=DEV).abs() * 0.45
    idx = torch.randperm(B * K1 + 3, device=DEV)[:B * K1].to(torch.int32).view(B, K1)
    q = torch.randn(B, 48, device=DEV) * 0.5
    got = ops.vqa_forward(feats, idx, q, mw, want_a_orig=want_a_orig)
    ref = mlb_vqa_forward(_state(vqa), feats.cpu().numpy(), idx.cpu().numpy(), q.cpu().numpy(), act_c=act_c)
    assert (got[0] is not None) == want_a_orig
    if want_a_orig:
        _check(got, ref, 0.0, "ragged")
    else:
        _check(got[1:], ref[1:], 0.0, "ragged")


def test_cli_real_data_mode_with_the_mlb_model(tmp_path, capsys):
    """A tiny on-disk dataset in the reference's formats with arch: MLBNoAtt: load_real, the per-split cache and a few training steps run;
    the cached z / a equal the module's torch path."""
    import counterexamples as cli
    from neuralcx import formats, ops
    from vqa.models.cx import CXModelBase
    paths = formats.write_synthetic_cx_files(os.path.join(str(tmp_path), "data"), n_train=192, n_val=96, n_img=300, seed=6)
    argv = ["--path_opt", MLB_YAML, "-b", "64", "--epochs", "1", "-p", "1", "--untrained_vqa", "--project_dir", str(tmp_path),
            "--path_trainset", paths["path_trainset"], "--path_features", paths["path_features"]]
    cli.main(argv)
    out = capsys.readouterr().out
    assert "Epoch 1 train: loss:" in out and "Epoch 1 val: loss:" in out and "cached VQA outputs of the train split" in out
    args = cli.build_parser().parse_args(argv)
    r = cli.Runner(args, cli.load_options(args))
    r.load_real()
    assert isinstance(r.mutan, ops.MlbWeights) and r.val.vqa_cache is not None
    ids = list(range(40))
    sel = torch.tensor(ids, device=DEV)
    b_cached, _ = r.get_batch(r.val, sel, ids[0])
    r.val.vqa_cache = None
    b, gt = r.get_batch(r.val, sel, ids[0])                    # produced per batch (--no_vqa_cache)
    assert b.z_orig.shape == (40, 1200) and b.a_knns.shape[:2] == (40, 24)
    for name in ("q_emb", "z_orig", "z_knns", "a_knns"):
        assert float((getattr(b, name) - getattr(b_cached, name)).abs().max()) <= 1e-5, name
    img_idx, wids, aids, gt2 = r.val.batch_indices(torch.tensor(ids))
    base = CXModelBase(r.vqa, 24)
    base.use_hip_vqa = False
    _, z_o, a_k, z_k, q = base.vqa_forward(r.val.dense_features(img_idx), wids)
    _check([b_cached.z_orig, b_cached.a_knns, b_cached.z_knns], [z_o, a_k, z_k], 1.0, "cache vs torch path")
    ev = r.engine.eval_step(b, gt)
    assert torch.isfinite(ev["scores"]).all()


def test_cli_synthetic_with_the_mlb_yaml(tmp_path, capsys):
    import counterexamples as cli
    cli.main(["--synthetic", "--path_opt", MLB_YAML, "-b", "64", "--epochs", "1", "--syn_train", "256", "--syn_val", "128", "--syn_images", "2048",
              "-p", "1", "--max_steps", "3", "--project_dir", str(tmp_path)])
    out = capsys.readouterr().out
    assert "Epoch 1 val: loss:" in out
    base = os.path.join(str(tmp_path), "logs", "cx")
    state = torch.load(os.path.join(base, os.listdir(base)[0], "ckpt", "model.ckpt"))
    assert state["linear_1.weight"].shape == (256, 3 * 2048 + 1 + 24 + 2400 + 2 * 1200 + 2 * 2400)
