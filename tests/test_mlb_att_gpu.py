"""GPU: the HIP eval-mode forward of the MLB attention model (ncx_mlb_att_forward) against the reference fixture, the fp64
restatement and the module's torch path.  Tolerances are the project's (tests/test_mlb_gpu.py): 1e-4 max|ref| per tensor against
fp64, 1e-4 max(1, max|ref|) against the fixture and the torch path.  Every parity input has PEAKED attention (asserted on its
reference before anything is compared): against uniform attention a wrong softmax or position order passes every tolerance."""
import functools

import numpy as np
import pytest
import torch

import mlb_att_ref as R
from trainer_edge_cases import ACT_CODE, ACT_FIELD
from trainer_edge_cases import att_weights as weights_of
from test_mlb_att_cpu import WORDS, YAML, _cli, att_opt, load_case

pytestmark = pytest.mark.gpu
DEV = "cuda:0"

def check(got_logits, got_att, ref_logits, ref_att, floor, what):
    """max|got - ref| <= 1e-4 max(floor, max|ref|) for the logits and for each glimpse's map; prints every figure before it asserts."""
    gl, ga = got_logits.detach().cpu().numpy(), got_att.detach().cpu().numpy()
    rl, ra = np.asarray(ref_logits), np.asarray(ref_att)
    assert gl.shape == rl.shape and ga.shape == ra.shape, (what, gl.shape, rl.shape, ga.shape, ra.shape)
    pairs = [("logits", gl, rl)] + [("att[%d]" % g, ga[:, g], ra[:, g]) for g in range(ra.shape[1])]
    figs = []
    for key, g, r in pairs:
        err, mx = float(np.abs(g - r).max()), float(np.abs(r).max())
        print("%s %s: max err %.3e, max|ref| %.3e" % (what, key, err, mx))
        figs.append((key, err, mx, bool(np.isfinite(g).all())))
    for key, err, mx, fin in figs:
        assert fin and err <= 1e-4 * max(floor, mx), (what, key, err, mx)


@functools.lru_cache(maxsize=None)
def case(seed, shape, acts=()):
    """(state, maps, q, (logits, att, pos)) of mlb_att_ref.peaked_case, computed once per test session and never modified."""
    st, maps, q, ref = R.peaked_case(seed, *shape, acts=dict(acts))
    assert shape[-1] * shape[-2] == 1 or R.peaked(ref[2], ref[1])
    return st, maps, q, ref


def run(st, maps, q, acts=(), img_idx=None, ws=None):
    from neuralcx import ops
    mw = weights_of(st, dict(acts))
    t = lambda a: torch.from_numpy(a).to(DEV)
    return ops.mlb_att_forward(t(maps), None if img_idx is None else t(img_idx), t(q), mw, ws=ws)


@pytest.mark.parametrize("name", ["c0", "c1"])
def test_hip_forward_vs_golden(name):
    c = load_case(name)
    ref = R.mlb_att_forward(c["state"], c["maps"], c["q_emb"], c["acts"], want_logits=True)
    assert R.peaked(ref[2], ref[1])
    logits, att = run(c["state"], c["table"], c["q_emb"], tuple(c["acts"].items()), img_idx=c["img_idx"])
    check(logits, att, c["logits"], c["att"], 1.0, "golden " + name)
    assert torch.equal(att[2], torch.full_like(att[2], float(att[2, 0, 0])))        # the all-zero image: exactly uniform
    assert not torch.equal(att[0], att[3])                                          # one image, two questions: two different maps
    assert np.allclose(att.sum(2).cpu().numpy(), 1.0, atol=1e-5)


RAGGED = [(1, 64, 48, 32, 1, 24, 40, 1, 1),          # P = 1: attention == 1
          (13, 96, 48, 44, 2, 28, 52, 5, 7),         # P % 4 != 0
          (70, 72, 40, 28, 3, 44, 42, 7, 7),         # dv not a multiple of 32, A not a multiple of 4, B beyond one tile
          (3, 100, 48, 130, 4, 20, 40, 14, 14),      # dh_att one past two 64-tiles, P = 196: the 208-row tile
          (5, 96, 48, 64, 8, 12, 40, 9, 15)]         # G = 8, P = 135: one past 128, three 64-row tiles


@pytest.mark.parametrize("shape", RAGGED, ids=lambda s: "x".join(map(str, s)))
def test_ragged_shapes_vs_fp64(shape):
    st, maps, q, ref = case(31, shape)
    logits, att = run(st, maps, q)
    check(logits, att, ref[0], ref[1], 0.0, "ragged %s" % (shape,))
    if shape[-1] * shape[-2] == 1:
        assert torch.equal(att, torch.ones_like(att))


@pytest.mark.parametrize("acts", [(("att_mm", None),), (("c", None),), (("att_mm", None), ("c", None))], ids=["no_mm", "no_classif", "neither"])
def test_optional_activations_vs_fp64(acts):
    shape = (13, 96, 48, 44, 2, 28, 52, 5, 7)
    st, maps, q, ref = case(32, shape, acts)
    logits, att = run(st, maps, q, acts)
    check(logits, att, ref[0], ref[1], 0.0, "acts %s" % (acts,))


def module_on_gpu(st, shape, acts=()):
    import vqa.models as M
    B, dv, dq, dh_att, G, dh_f, A = shape[:7]
    a = dict(acts)
    m = M.factory(att_opt(dv, dq, dh_att, G, dh_f, a.get("att_mm", "tanh"), a.get("c", "tanh")), WORDS, ["a%d" % i for i in range(A)], cuda=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    return m.to(DEV).eval()


def test_full_widths_vs_fp64_and_torch_path():
    shape = (8, 2048, 2400, 1200, 4, 1200, 2000, 14, 14)
    st, maps, q, ref = case(33, shape)
    logits, att = run(st, maps, q)
    m = module_on_gpu(st, shape)
    m.use_hip = False
    with torch.no_grad():
        t_logits = m.forward_from_q(torch.from_numpy(maps).to(DEV), torch.from_numpy(q).to(DEV))
    t_att = torch.stack(m.list_att, 1)
    for what, l, a in (("torch path", t_logits, t_att), ("hip", logits, att)):
        print("%s vs fp64: logits %.3e (max|ref| %.3e), att %.3e (max|ref| %.3e)" % (
            what, np.abs(l.cpu().numpy() - ref[0]).max(), np.abs(ref[0]).max(), np.abs(a.cpu().numpy() - ref[1]).max(), ref[1].max()))
    check(logits, att, ref[0], ref[1], 0.0, "full widths vs fp64")
    check(logits, att, t_logits.cpu().numpy(), t_att.cpu().numpy(), 1.0, "full widths vs torch path")


def test_spatial_equivariance():
    """One random permutation of the P positions of every map: the logits stay, each attention map is permuted the same way."""
    shape = (3, 100, 48, 130, 4, 20, 40, 14, 14)
    st, maps, q, ref = case(31, shape)
    perm = np.random.default_rng(5).permutation(196)
    pmaps = np.ascontiguousarray(maps.reshape(3, 100, 196)[:, :, perm]).reshape(maps.shape)
    logits, att = run(st, maps, q)
    p_logits, p_att = run(st, pmaps, q)
    check(p_logits, p_att, ref[0], ref[1][:, :, perm], 0.0, "permuted vs permuted fp64")
    check(p_logits, p_att, logits.cpu().numpy(), att.cpu().numpy()[:, :, perm], 0.0, "permuted vs unpermuted hip")
    assert not np.allclose(att.cpu().numpy(), p_att.cpu().numpy(), atol=1e-3)         # peaked: the permutation is visible


def test_img_idx_with_repeats_equals_the_dense_route():
    shape = (13, 96, 48, 44, 2, 28, 52, 5, 7)
    st, maps, q, ref = case(31, shape)
    logits, att = run(st, maps, q)
    rng = np.random.default_rng(6)
    idx = rng.integers(0, 13, size=13).astype(np.int32)
    idx[1] = idx[0]
    assert not np.array_equal(idx, np.arange(13))
    g_logits, g_att = run(st, maps, q, img_idx=idx)                        # the table route: question b reads maps[idx[b]]
    d_logits, d_att = run(st, np.ascontiguousarray(maps[idx]), q)          # the same maps, gathered on the host
    assert torch.equal(g_logits, d_logits) and torch.equal(g_att, d_att)
    ref_g = R.mlb_att_forward(st, maps[idx], q)
    check(g_logits, g_att, ref_g[0], ref_g[1], 0.0, "img_idx with repeats")


def test_table_beyond_4_gib():
    """86 000 images x 64 x 14 x 14 fp32 = 4.3 GB: the image base address is 64-bit.  Only the rows used are filled, the last included."""
    from neuralcx import ops
    shape = (4, 64, 48, 32, 2, 24, 40, 14, 14)
    st, maps, q, ref = case(34, shape)
    n_img = 86000
    assert n_img * 64 * 196 * 4 > 2 ** 32
    table = torch.empty(n_img, 64, 14, 14, device=DEV)
    idx = np.array([n_img - 1, 21914, 70001, 3], np.int32)                 # byte offsets past 2^30, past 2^31 and (the last image) past 2^32
    table[torch.from_numpy(idx).long().to(DEV)] = torch.from_numpy(maps).to(DEV)
    logits, att = ops.mlb_att_forward(table, torch.from_numpy(idx).to(DEV), torch.from_numpy(q).to(DEV), weights_of(st))
    check(logits, att, ref[0], ref[1], 0.0, "table beyond 4 GiB")
    del table
    torch.cuda.empty_cache()


def test_stale_workspace_and_bit_identical_calls():
    from neuralcx import ops
    shape = (70, 72, 40, 28, 3, 44, 42, 7, 7)
    st, maps, q, ref = case(31, shape)
    mw = weights_of(st)
    ws = ops.mlb_att_workspace(mw, 70, 49, 70, torch.device(DEV))
    l0, a0 = run(st, maps, q, ws=ws)
    ws.view(torch.float32).fill_(float("nan"))
    l1, a1 = run(st, maps, q, ws=ws)
    assert torch.isfinite(l1).all() and torch.isfinite(a1).all()
    assert torch.equal(l0, l1) and torch.equal(a0, a1)
    l2, a2 = run(st, maps, q)                                              # the cached workspace: the same buffer again
    assert torch.equal(l0, l2) and torch.equal(a0, a2)
    check(l1, a1, ref[0], ref[1], 0.0, "stale workspace")


def test_module_routing(monkeypatch):
    from neuralcx import ops
    shape = (13, 96, 48, 44, 2, 28, 52, 5, 7)
    st, maps, q, ref = case(31, shape)
    m = module_on_gpu(st, shape)
    v, qd = torch.from_numpy(maps).to(DEV), torch.from_numpy(q).to(DEV)
    calls = []
    real = ops.mlb_att_forward
    monkeypatch.setattr(ops, "mlb_att_forward", lambda *a, **k: (calls.append(1), real(*a, **k))[1])
    with torch.no_grad():
        logits = m.forward_from_q(v, qd)
    assert len(calls) == 1                                                  # eval + no_grad on CUDA: HIP
    hip_att = torch.stack(m.list_att, 1).clone()
    check(logits, hip_att, ref[0], ref[1], 0.0, "module, hip route")
    wids = torch.randint(1, 40, (13, 6), device=DEV)
    with torch.no_grad():
        full = m(v, wids)                                                   # through the encoder as well
    assert len(calls) == 2 and full.shape == (13, 52) and len(m.list_att) == 2 and m.list_att[0].shape == (13, 35)

    def torch_route(mod, grad=False):
        n = len(calls)
        with torch.set_grad_enabled(grad):
            out = mod.forward_from_q(v, qd)
        assert len(calls) == n, "took the HIP route"
        return out.detach(), torch.stack(mod.list_att, 1)

    l_g, a_g = torch_route(m, grad=True)                                    # grad mode, parameters require grad
    check(logits, hip_att, l_g.cpu().numpy(), a_g.cpu().numpy(), 1.0, "hip vs torch path (grad mode)")
    m.use_hip = False
    l_t, a_t = torch_route(m)                                               # use_hip = False
    check(logits, hip_att, l_t.cpu().numpy(), a_t.cpu().numpy(), 1.0, "hip vs torch path (use_hip = False)")
    m.use_hip = True
    m.train()
    for k in ("attention", "fusion", "classif"):                           # dropout off, so that training mode can be compared
        for d in [x for x in m.opt[k] if x.startswith("dropout")]:
            m.opt[k][d] = 0.0
    with torch.no_grad():
        n = len(calls)
        l_tr = m.forward_from_q(v, qd)
        assert len(calls) == n                                              # training mode
    check(logits, hip_att, l_tr.cpu().numpy(), torch.stack(m.list_att, 1).cpu().numpy(), 1.0, "hip vs torch path (training mode)")
    m.eval()
    m.opt["fusion"]["activation_v"] = "relu"                                # an unsupported activation: the torch path, silently
    l_r, _ = torch_route(m)
    assert torch.isfinite(l_r).all()
    m.opt["fusion"]["activation_v"] = "tanh"

    # the packed weights follow the parameters
    with torch.no_grad():
        m.forward_from_q(v, qd)
        w0 = m._hip_weights()
        assert m._hip_weights() is w0
        m.linear_classif.bias.add_(1.0)                                     # an in-place update (an optimizer step)
        after = m.forward_from_q(v, qd)
        assert m._hip_weights() is not w0
        check(after, torch.stack(m.list_att, 1), ref[0] + 1.0, ref[1], 0.0, "after an in-place update")
        m.load_state_dict({k: torch.from_numpy(x) for k, x in st.items()}, strict=False)
        w1 = m._hip_weights()
        back = m.forward_from_q(v, qd)
        assert torch.equal(back, logits) and w1 is not w0


def test_train_cli_evaluates_in_hip(tmp_path, capsys):
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
    real = ops.mlb_att_forward
    ops.mlb_att_forward = lambda *a, **k: (calls.append(1), real(*a, **k))[1]
    try:
        out = _cli("train.py").main(["--path_opt", str(path), "--synthetic", "--syn_examples", "36", "--syn_images", "64", "--syn_vocab", "30",
                                     "--syn_grid", "5", "--print_freq", "0"])
    finally:
        ops.mlb_att_forward = real
    text = capsys.readouterr().out
    assert "eval-mode forward in HIP (ncx_mlb_att_forward)" in text
    assert len(out["history"]) == 1 and np.isfinite(out["history"][0]["val"]["loss"])
    assert len(calls) >= 1                                                  # validation ran the HIP forward; training did not
    assert out["trainer"].train.feats.shape == (64, 64, 5, 5)
    # --freeze_seq2vec: no HIP engine for this model; the route line says so instead of failing, and evaluation still runs in HIP
    ev = _cli("train.py").main(["--path_opt", str(path), "--synthetic", "--syn_examples", "36", "--syn_images", "64", "--syn_vocab", "30",
                                "--syn_grid", "5", "--print_freq", "0", "--freeze_seq2vec", "--evaluate"])
    assert "there is no HIP engine for this model" in capsys.readouterr().out
    assert ev["trainer"].engine is None and np.isfinite(ev["val"]["loss"])
