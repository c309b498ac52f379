"""CPU: the training step of the MLB attention model -- the fp64 restatement (tests/mlb_att_train_ref.py) against the reference
fixture g22 and against torch autograd in float64 on the module's torch path with injected masks; the generator masks; the C ABI's
host-side checks; train.py's flag.  No compute on a device."""
import ctypes
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

from conftest import GOLDEN, ROOT
import mlb_att_ref
import mlb_att_train_ref as TR
from helpers import grad_tol
from test_mlb_att_cpu import WORDS, YAML, _cli, att_opt

CASES = ("c0", "c1")
YAML_P = (0.5, 0.5, 0.5, 0.5, 0.5, 0.5)
ZERO_IN_MATHS = "conv_att.bias"      # sum_p ds = 0 under the softmax: the gradient is rounding noise in every implementation


def load_train_case(name):
    g = np.load(os.path.join(GOLDEN, "g22_mlb_att_train.npz"))
    c = {k[len(name) + 1:]: g[k] for k in g.files if k.startswith(name + "/")}
    c["state"] = {k[len("state/"):]: v for k, v in c.items() if k.startswith("state/")}
    c["grads"] = {k[len("grad/"):]: v for k, v in c.items() if k.startswith("grad/")}
    c["acts"] = dict(att_mm=str(c["activation_mm"]) or None, c=str(c["classif_activation"]) or None)
    c["maps"] = c["table"][c["img_idx"]]
    return c


def noise_bound(name, ref64, ref32):
    """Tolerance of a gradient tensor: helpers.grad_tol; for conv_att.bias (zero in mathematics) twice the error of the fp32
    reference `ref32` against fp64 on the same input, when that is larger."""
    tol = grad_tol(name, ref64)
    if name == ZERO_IN_MATHS and ref32 is not None:
        tol = max(tol, 2.0 * float(np.abs(np.asarray(ref32, np.float64) - ref64).max()))
    return tol


@pytest.mark.parametrize("name", CASES)
def test_restatement_reproduces_the_reference_fixture(name):
    c = load_train_case(name)
    r = TR.step(c["state"], c["maps"], c["q_emb"], c["target"], c["acts"])
    assert mlb_att_ref.peaked(r["pos"], r["att"]), "every parity input must have peaked attention"
    for key in ("logits", "att"):
        err, mx = float(np.abs(c[key] - r[key]).max()), float(np.abs(r[key]).max())
        print(name, key, "max|reference fp32 - fp64| = %.3e, max|ref| = %.3e" % (err, mx))
        assert err <= 1e-5 * max(1.0, mx), (key, err, mx)
    assert abs(float(c["loss"]) - r["loss"]) <= 1e-5 * max(1.0, abs(r["loss"]))
    assert set(c["grads"]) == set(r["grads"]) == set(c["state"]) and len(c["grads"]) == 10 + 2 * int(c["dims"][3])
    for k, ref in r["grads"].items():
        got = c["grads"][k]
        assert got.shape == ref.shape, k
        err = float(np.abs(got - ref).max())
        print(name, k, "max err %.3e, max|ref| %.3e" % (err, float(np.abs(ref).max())))
        if k == ZERO_IN_MATHS:
            assert err <= 1e-6, (k, err)            # both are rounding noise around zero
        else:
            assert err <= grad_tol(k, ref), (k, err)
    err = float(np.abs(c["grad_q_emb"] - r["dq_emb"]).max())
    assert err <= grad_tol("q_emb", r["dq_emb"]), err


@pytest.mark.parametrize("name", CASES)
def test_fixture_has_the_planted_rows(name):
    c = load_train_case(name)
    idx = c["img_idx"]
    assert not c["table"][3].any() and idx[2] == 3
    assert np.array_equal(c["att"][2], np.full_like(c["att"][2], c["att"][2, 0, 0]))
    assert idx[0] == idx[3] and not np.array_equal(idx, np.arange(len(idx)))
    xq = np.tanh(c["q_emb"].astype(np.float64) @ c["state"]["linear_q_att.weight"].T.astype(np.float64) + c["state"]["linear_q_att.bias"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5
    assert c["att"].max() >= 0.3
    g21 = np.load(os.path.join(GOLDEN, "g21_mlb_att.npz"))
    assert np.array_equal(c["dims"], g21[name + "/dims"])                   # g21's two reduced shapes
    assert os.path.getsize(os.path.join(GOLDEN, "g22_mlb_att_train.npz")) <= os.path.getsize(os.path.join(GOLDEN, "g21_mlb_att.npz"))


def torch_step_with_masks(model, maps, q, target, masks, p, dtype):
    """The module's torch path (vqa/models/att.py) with F.dropout replaced by the given keep masks, under autograd in `dtype`.
    -> (logits, att, loss, {state_dict key: grad}, dq)"""
    m = model.to(dtype)
    m.train()
    G = m.opt["attention"]["nb_glimpses"]
    K = [torch.from_numpy(np.asarray(k)).to(dtype) / (1.0 - pr) for k, pr in zip(masks, p)]
    # the module calls F.dropout for the layers 1, 2, 3, then layer 4 once per glimpse, then 5 and 6
    it = iter([K[0], K[1], K[2]] + [K[3][:, g] for g in range(G)] + [K[4], K[5]])
    order = []

    def fake_dropout(x, p=0.5, training=True, inplace=False):
        k = next(it)
        order.append(tuple(x.shape))
        return x * k.reshape(x.shape)

    v = torch.from_numpy(maps).to(dtype)
    qt = torch.from_numpy(q).to(dtype).requires_grad_(True)
    real = F.dropout
    F.dropout = fake_dropout
    try:
        logits = m.forward_from_q(v, qt)
    finally:
        F.dropout = real
    assert order[0] == tuple(v.shape) and order[1] == tuple(qt.shape) and len(order) == 5 + G
    loss = F.cross_entropy(logits, torch.from_numpy(np.asarray(target)).long())
    m.zero_grad()
    loss.backward()
    grads = {n: p_.grad.detach().numpy().astype(np.float64) for n, p_ in m.named_parameters() if not n.startswith("seq2vec.")}
    return logits.detach().numpy(), torch.stack(m.list_att, 1).numpy(), float(loss.detach()), grads, qt.grad.numpy()


def module_for(st, shape, acts):
    import vqa.models as M
    B, dv, dq, dh_att, G, dh_f, A = shape[:7]
    a = dict(acts)
    opt = att_opt(dv, dq, dh_att, G, dh_f, a.get("att_mm", "tanh"), a.get("c", "tanh"))
    for key, (sect, name) in dict(att_v=("attention", "activation_v"), att_q=("attention", "activation_q"), v=("fusion", "activation_v"),
                                  q=("fusion", "activation_q")).items():
        if key in a and not a[key]:
            del opt[sect][name]
    m = M.factory(opt, WORDS, ["a%d" % i for i in range(A)], cuda=False)
    m.load_state_dict({k: torch.from_numpy(v) for k, v in st.items()}, strict=False)
    return m


def masks_for_module(masks, shape):
    """The library's mask of layer 3 is [B, P, dh_att]; the module's x_att is [B, dh_att, W, H]."""
    W, H = shape[7], shape[8]
    out = list(masks)
    out[2] = np.ascontiguousarray(np.asarray(masks[2]).transpose(0, 2, 1)).reshape(masks[2].shape[0], masks[2].shape[2], W, H)
    out[0] = np.asarray(masks[0]).reshape(masks[0].shape[0], masks[0].shape[1], W, H)
    return out


@pytest.mark.parametrize("acts", [(), (("att_mm", None), ("c", None))], ids=["tanh", "no_mm_no_classif"])
def test_restatement_equals_torch_autograd_in_float64_with_masks(acts):
    shape = (5, 24, 12, 20, 3, 8, 9, 3, 5)
    B, dv, dq, dh_att, G, dh_f, A, W, H = shape
    st, maps, q, ref = mlb_att_ref.peaked_case(41, *shape, acts=dict(acts))
    rng = np.random.default_rng(7)
    p = (0.5, 0.25, 0.5, 0.3, 0.5, 0.4)
    masks = TR.random_masks(rng, p, B, W * H, dv, dq, dh_att, G, dh_f)
    target = rng.integers(0, A, size=B)
    r = TR.step(st, maps, q, target, dict(acts), masks, p)
    logits, att, loss, grads, dq_t = torch_step_with_masks(module_for(st, shape, acts), maps, q, target, masks_for_module(masks, shape), p, torch.float64)
    assert np.abs(logits - r["logits"]).max() <= 1e-10 and np.abs(att - r["att"]).max() <= 1e-10 and abs(loss - r["loss"]) <= 1e-10
    assert set(grads) == set(r["grads"])
    for k, ref_g in r["grads"].items():
        assert np.abs(grads[k] - ref_g).max() <= 1e-10 * max(1.0, np.abs(ref_g).max()), k
    assert np.abs(dq_t - r["dq_emb"]).max() <= 1e-10
    assert float(np.abs(r["dq_emb"]).max()) > 0 and all(float(np.abs(v).max()) > 0 for k, v in r["grads"].items() if k != ZERO_IN_MATHS)


def test_generator_masks_follow_the_documented_ids_and_indices():
    from oracle.ncx_oracle import dropout_keep_mask
    B, P, dv, dq, dh_att, G, dh_f = 6, 35, 40, 24, 32, 2, 16
    seed = 0x1234567890ABCDEF
    p = (0.5, 0.3, 0.5, 0.25, 0.6, 0.5)
    masks = TR.generator_masks(seed, p, B, P, dv, dq, dh_att, G, dh_f)
    shapes = TR.mask_shapes(B, P, dv, dq, dh_att, G, dh_f)
    assert shapes == ((B, dv, P), (B, dq), (B, P, dh_att), (B, G, dv), (B, dq), (B, G * dh_f))
    for layer, (m, shp, pr) in enumerate(zip(masks, shapes, p), start=1):
        assert m.shape == shp and set(np.unique(m)) <= {0.0, 1.0}
        n = m.size
        flat = dropout_keep_mask(seed, layer, 1, n, pr).numpy().reshape(-1)            # element index = linear index in the tensor
        assert np.array_equal(m.reshape(-1), flat), layer
        kept, sd = m.mean(), np.sqrt(pr * (1 - pr) / n)
        assert abs(kept - (1 - pr)) <= 5 * sd, (layer, kept, pr)
    assert not np.array_equal(masks[1], masks[4])                                       # layers 2 and 5: the same shape, different ids
    assert all(np.array_equal(m, np.ones_like(m)) for m in TR.generator_masks(seed, (0.0,) * 6, B, P, dv, dq, dh_att, G, dh_f))
    from neuralcx import ops
    assert ops.mlb_att_mask_sizes(B, P, dv, dq, dh_att, G, dh_f) == tuple(int(np.prod(s)) for s in shapes)
    assert ops.AT_LAYERS == dict(att_v=1, att_q=2, att_mm=3, v=4, q=5, c=6)


def test_symbols_declared_exported_and_validated_on_the_host():
    from neuralcx import _lib
    from neuralcx._lib import NcxMlbAttDims, NcxMlbAttGrads, NcxMlbAttParams, NcxMlbAttTrain
    hdr = open(os.path.join(ROOT, "include", "neuralcx.h")).read()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for n in ("ncx_mlb_att_train_workspace_bytes", "ncx_mlb_att_train_forward", "ncx_mlb_att_train_backward", "ncx_mlb_att_train_ws_region"):
        assert n + "(" in hdr and n in _lib.EXPORTS and hasattr(L, n), n
    assert "typedef struct ncx_mlb_att_train" in hdr and ctypes.sizeof(NcxMlbAttTrain) == 6 * 4 + 2 * 4 + 8
    assert "typedef struct ncx_mlb_att_grads" in hdr and ctypes.sizeof(NcxMlbAttGrads) == 12 * 8
    assert [n for n, _ in NcxMlbAttGrads._fields_] == [n for n, _ in NcxMlbAttParams._fields_[:12]]
    lib = _lib.lib()
    one = ctypes.c_void_p(256)                      # never dereferenced: validation only
    ptrs = {n: one for n, _ in NcxMlbAttParams._fields_[:12]}
    acts = {n: 2 for n, _ in NcxMlbAttParams._fields_[12:]}
    good = dict(B=128, P=196, dv=2048, dq=2400, dh_att=1200, G=4, dh_f=1200, A=2000, n_img=82783)
    m = NcxMlbAttParams(**ptrs, **acts)
    d = NcxMlbAttDims(**good)
    tgood = dict(p_att_v=0.5, p_att_q=0.5, p_att_mm=0.5, p_v=0.5, p_q=0.5, p_c=0.5, dropout_mode=1, want_dq=1, seed=7)
    t = NcxMlbAttTrain(**tgood)
    R = lambda *a: lib.ncx_mlb_att_train_workspace_bytes(*[None if x is None else ctypes.byref(x) for x in a])
    need = R(d, t, m)
    stash, vd = 128 * 196 * 1200 * 4, 128 * 2048 * 196 * 4
    assert need % 256 == 0 and stash + vd < need < 2 * (stash + vd)
    t0 = NcxMlbAttTrain(**dict(tgood, dropout_mode=0))
    assert stash < R(d, t0, m) < need - vd + 4096                    # layer 1 off: no dropped copy of the map
    off, nb = ctypes.c_size_t(), ctypes.c_size_t()
    reg = lambda which, tt=t, dd=d: lib.ncx_mlb_att_train_ws_region(ctypes.byref(dd), ctypes.byref(tt), ctypes.byref(m), which, ctypes.byref(off), ctypes.byref(nb))
    assert reg(1) == 0 and nb.value == stash and off.value % 256 == 0
    assert reg(2) == 0 and nb.value == 128 * 4 * 2048 * 4
    assert reg(3) == 0 and nb.value == 128 * 4 * 1200 * 4
    assert reg(4) == 0 and nb.value == vd
    assert reg(4, t0) == 0 and nb.value == 0
    assert reg(5) == 0 and nb.value % (1200 * 2048 * 4) == 0 and 1 <= nb.value // (1200 * 2048 * 4) <= 8
    assert reg(99) == -4 and lib.ncx_mlb_att_train_ws_region(ctypes.byref(d), ctypes.byref(t), ctypes.byref(m), 1, None, None) == -1
    # bad dims, modes and p's
    for field, val in (("B", 0), ("P", 0), ("G", 9), ("dv", 3), ("dq", 2), ("dh_att", 0), ("dh_f", 3), ("A", 1), ("n_img", 0), ("P", 1 << 20)):
        assert R(NcxMlbAttDims(**dict(good, **{field: val})), t, m) == 0, (field, val)
    for field, val in (("dropout_mode", 3), ("dropout_mode", -1), ("p_att_v", 1.0), ("p_att_mm", -0.1), ("p_c", 1.5), ("p_v", float("nan")),
                       ("p_q", 1.0), ("p_att_q", 2.0)):
        assert R(d, NcxMlbAttTrain(**dict(tgood, **{field: val})), m) == 0, (field, val)
    bm = NcxMlbAttParams(**ptrs, **acts)
    bm.act_mm = 1
    assert R(d, t, bm) == 0
    assert R(None, t, m) == 0 and R(d, None, m) == 0 and R(d, t, None) == 0
    for over in (dict(P=1), dict(P=3), dict(G=8), dict(G=1)):
        assert R(NcxMlbAttDims(**dict(good, **over)), t, m) > 0, over
    # NULLs, dims, modes and p's are rejected before any launch (no pointer is dereferenced)
    g = NcxMlbAttGrads(**ptrs)
    B = ctypes.byref
    fwd = lambda dd, tt, mm, feats=one, masks=None, ws=one, n=1 << 40, logits=one: lib.ncx_mlb_att_train_forward(
        dd, tt, feats, one, one, mm, masks, ws, n, logits, one, None)
    bwd = lambda dd, tt, mm, gg, ws=one, n=1 << 40, att=one, dq=one: lib.ncx_mlb_att_train_backward(
        dd, tt, one, one, one, mm, None, ws, n, att, one, gg, dq, None)
    assert fwd(None, B(t), B(m)) == -1 and fwd(B(d), None, B(m)) == -1 and fwd(B(d), B(t), None) == -1
    assert fwd(B(d), B(t), B(m), feats=None) == -1 and fwd(B(d), B(t), B(m), logits=None) == -1
    t2 = NcxMlbAttTrain(**dict(tgood, dropout_mode=2))
    assert fwd(B(d), B(t2), B(m), masks=None) == -1                                   # mode 2 needs the masks
    assert fwd(B(NcxMlbAttDims(**dict(good, G=9))), B(t), B(m)) == -2
    assert fwd(B(d), B(NcxMlbAttTrain(**dict(tgood, p_c=1.0))), B(m)) == -2
    assert fwd(B(d), B(NcxMlbAttTrain(**dict(tgood, dropout_mode=5))), B(m)) == -2
    assert fwd(B(d), B(t), B(bm)) == -4
    assert fwd(B(d), B(t), B(m), n=need - 1) == -3 and fwd(B(d), B(t), B(m), ws=ctypes.c_void_p(264)) == -3
    assert bwd(B(d), B(t), B(m), None) == -1 and bwd(B(d), B(t), B(m), B(g), att=None) == -1
    assert bwd(B(d), B(t), B(m), B(g), dq=None) == -1                                  # want_dq without a buffer
    gn = NcxMlbAttGrads(**dict(ptrs, wa=None))
    assert bwd(B(d), B(t), B(m), B(gn)) == -1
    assert bwd(B(NcxMlbAttDims(**dict(good, dv=3))), B(t), B(m), B(g)) == -2
    assert bwd(B(d), B(t), B(m), B(g), n=need - 1) == -3


def _tiny_yaml(tmp_path):
    import yaml
    with open(YAML) as f:
        opt = yaml.safe_load(f)
    m = opt["model"]
    m["dim_v"], m["dim_q"], m["seq2vec"]["emb_size"] = 16, 12, 8
    m["attention"].update(dim_h=8, nb_glimpses=2)
    m["fusion"]["dim_h"] = 6
    opt["vqa"].update(nans=10, maxlength=5)
    opt["optim"].update(batch_size=8, epochs=1)
    opt["logs"]["dir_logs"] = str(tmp_path / "logs")
    path = tmp_path / "tiny.yaml"
    path.write_text(yaml.safe_dump(opt))
    return path


def test_hip_att_train_flag_is_refused_with_no_hip_and_off_by_default(tmp_path, monkeypatch):
    import vqa.models as M
    assert M.MLBAtt.use_hip_train is False
    m = M.factory(att_opt(16, 12, 8, 2, 6), WORDS, ["a%d" % i for i in range(10)], cuda=False)
    assert m.use_hip_train is False and "use_hip_train" not in m.__dict__
    m.use_hip_train = True                           # a CPU module never takes the HIP route, in any mode
    m.train()
    assert not m._hip_train_ok(torch.rand(3, 16, 3, 2), torch.zeros(3, 12))
    path = _tiny_yaml(tmp_path)
    monkeypatch.setattr(torch.cuda, "is_available", lambda: False)
    cli = _cli("train.py")
    base = ["--path_opt", str(path), "--synthetic", "--syn_examples", "32", "--syn_images", "6", "--syn_vocab", "20", "--syn_grid", "3", "--print_freq", "0"]
    with pytest.raises(SystemExit, match="--hip_att_train .* cannot be combined with --no_hip"):
        cli.main(base + ["--hip_att_train", "--no_hip"])
    with pytest.raises(SystemExit, match="MI355X"):
        cli.main(base + ["--hip_att_train"])
    noatt = os.path.join(os.path.dirname(YAML), "mlb_noatt_train.yaml")
    with pytest.raises(SystemExit, match="needs an attention arch"):
        cli.main(["--path_opt", noatt, "--synthetic", "--hip_att_train"])
    assert cli.build_parser().parse_args([]).hip_att_train is False
