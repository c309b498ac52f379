"""Shared helpers for the test-suite: load a golden fixture into oracle-shaped inputs."""
import os

import numpy as np
import torch

from oracle import ncx_oracle as orc

GOLDEN = os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden")
# Gradient tolerance of SURVEY 8c: rel * max|reference grad| per tensor, NO absolute floor -- except for out.bias, whose
# gradient is mathematically zero under a listwise softmax (sum_k (p_k - y_k) = 0; the reference itself holds ~4e-8 of
# round-off there), so "relative to its own max" is meaningless for that one tensor.
ZERO_GRAD_TENSORS = ("out.bias",)
ZERO_GRAD_FLOOR = 1e-2


def grad_tol(name, ref, rel=1e-4):
    """Absolute element tolerance for the gradient tensor `name` whose reference value is `ref` (array / tensor)."""
    m = float(np.abs(np.asarray(ref)).max()) if np.asarray(ref).size else 0.0
    if name in ZERO_GRAD_TENSORS:
        m = max(m, ZERO_GRAD_FLOOR)
    return rel * m
SPEC_KEYS = ("v_emb", "v_mult", "v_dist", "v_rank", "q_emb", "a_emb", "z_emb")


def golden_names(prefix=""):
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.endswith(".npz") and f.startswith(prefix)
                  and f.startswith(("g1_", "g2_", "g3_")))          # model cases (g4 / g7 / g8: loss, data helpers, kNN)


def load_golden(name):
    g = dict(np.load(os.path.join(GOLDEN, name + ".npz")))
    K, dv, dq, dz, da, A, H, L = [int(x) for x in g["dims"]]
    d = orc.Dims(K=K, dv=dv, dq=dq, dz=dz, da=da, A=A, H=H, L=L)
    spec = {k: bool(v) for k, v in zip(SPEC_KEYS, g["spec"])}
    params = orc.init_params(d, int(g["weight_seed"]), float(g["weight_gain"]))
    batch = dict(image_features=torch.from_numpy(g["image_features"]),
                 q_emb=torch.from_numpy(g["q_emb"]), z_orig=torch.from_numpy(g["z_orig"]),
                 z_knns=torch.from_numpy(g["z_knns"]), a_knns=torch.from_numpy(g["a_knns"]),
                 answer_aids=torch.from_numpy(g["answer_aids"]), gt=torch.from_numpy(g["gt"]))
    return g, d, spec, params, batch


def check_grads_against_golden(g, grads, rel=1e-4):
    """grads: dict name -> np.ndarray.  Tolerance: rel * max|golden grad| per tensor."""
    for key in g:
        if key.startswith("grad/"):
            n = key[5:]
            ref = g[key]
            tol = grad_tol(n, ref, rel)
            err = np.abs(np.asarray(grads[n]).reshape(ref.shape) - ref).max()
            assert err <= tol, (n, err, tol)
        elif key.startswith("gradval/"):
            n = key[8:]
            ref = g[key]
            got = np.asarray(grads[n]).reshape(-1)[g["gradidx/" + n]]
            tol = grad_tol(n, ref, rel)            # (max over the stored sample <= max over the tensor: the stricter bound)
            assert np.abs(got - ref).max() <= tol, (n, np.abs(got - ref).max(), tol)
        elif key.startswith("gradnorm/"):
            n = key[9:]
            nrm = np.linalg.norm(np.asarray(grads[n]).astype(np.float64))
            assert abs(nrm - float(g[key])) <= 1e-4 * max(float(g[key]), ZERO_GRAD_FLOOR if n in ZERO_GRAD_TENSORS else 0.0), (n, nrm, float(g[key]))


def random_case_f32(seed, B, d, scale=0.45):
    """Seeded synthetic inputs of the shapes NeuralModel.forward sees (|N(0,1)|*0.45 features etc.)."""
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    return dict(image_features=t(np.abs(rng.standard_normal((B, d.K + 1, d.dv), dtype=np.float32)) * scale),
                q_emb=t(rng.standard_normal((B, d.dq), dtype=np.float32) * 0.3), z_orig=t(rng.standard_normal((B, d.dz), dtype=np.float32)),
                z_knns=t(rng.standard_normal((B, d.K, d.dz), dtype=np.float32)),
                a_knns=t(rng.standard_normal((B, d.K, d.A), dtype=np.float32) * 2),
                answer_aids=torch.from_numpy(rng.integers(0, d.A, size=B)), gt=torch.from_numpy(rng.integers(0, d.K, size=B)))


def condition_away_from_kinks(params, d, batch, seed, tau=2e-5, bf16=False, max_rounds=40, spec=None):
    """Full-size parity inputs must not sit ON a discontinuity of the network, where the fp32 summation order alone
    decides the outcome (in the reference too: two BLAS builds disagree there).  Triplets with a pre-activation of ANY
    hidden layer (linear_1 .. linear_L) within `tau` of the ReLU kink -- and, for the bf16 variant, a distance feature
    within a few fp32 ulps of a bf16 rounding boundary -- are redrawn until none is left (the same idea as the rank-gap
    guard of the Recall fixtures).  Returns the number of redrawn triplets; `batch` is modified in place.  Under the a_emb lesion (`spec`) the
    noise blocks a_knns and batch["a_emb_gt"] stay; the other inputs of a triplet are redrawn."""
    B = batch["gt"].shape[0]
    lesion = spec is not None and not spec.get("a_emb", True)
    keys = ("image_features", "q_emb", "z_orig", "z_knns", "a_knns", "answer_aids", "gt")
    redraw = tuple(k for k in keys if not (lesion and k == "a_knns"))
    todo = torch.arange(B)
    redrawn = 0
    for rnd in range(max_rounds):
        sub = {k: batch[k][todo] for k in keys}
        taps = {}
        with torch.no_grad():
            args = (params, d, sub["image_features"], sub["q_emb"], sub["z_orig"], sub["z_knns"], sub["a_knns"], sub["answer_aids"])
            if bf16:
                orc.forward_bf16(*args, taps=taps)
            elif lesion:
                orc.forward_faithful(*args, spec=spec, a_emb_gt_override=batch["a_emb_gt"][todo], taps=taps)
            else:
                orc.forward_faithful(*args, taps=taps)
        bad = torch.zeros(todo.numel(), dtype=torch.bool)
        for l in range(1, d.L + 1):
            bad |= taps["pre%d" % l].abs().flatten(1).min(1).values < tau
        if bf16:
            x = taps["dist"]
            bf = lambda t: t.bfloat16().float()
            bad |= ((bf(x * (1 + 2e-6)) != bf(x)) | (bf(x * (1 - 2e-6)) != bf(x))).any(1)
        todo = todo[bad]
        if todo.numel() == 0:
            return redrawn
        redrawn += todo.numel()
        fresh = random_case_f32(seed * 1000 + rnd + 1, todo.numel(), d)
        for k in redraw:
            batch[k][todo] = fresh[k]
    raise AssertionError("could not condition the batch away from the ReLU kinks")


# ---- the HIP path through the C ABI on cuda:0, and its comparison with the oracle (GPU tests) ------------------------------------------------
FIELD = {"answer_embedding.weight": "answer_embedding", "linear_1.weight": "w1", "linear_1.bias": "b1",
         "linear_2.weight": "w2", "linear_2.bias": "b2", "linear_3.weight": "w3", "linear_3.bias": "b3",
         "out.weight": "w_out", "out.bias": "b_out"}


def dev():
    return torch.device("cuda:0")


def to_dev_params(params):
    return {FIELD[k]: v.to(dev()).contiguous() for k, v in params.items()}


def to_dev_batch(batch, spec=None, keep_mask=None, extra=None):
    from neuralcx.ops import Batch
    extra = extra or {}
    g = lambda k: batch[k].to(dev())
    return Batch.from_dense(g("image_features"), g("q_emb"), g("z_orig"), g("z_knns"), g("a_knns"),
                            g("answer_aids"), keep_mask=None if keep_mask is None else keep_mask.to(dev()),
                            **{k: v.to(dev()) for k, v in extra.items()})


def run_hip(d, spec, params, batch, training=False, drop_p=0.0, keep_mask=None, seed=0, extra=None):
    from neuralcx import ops
    b = to_dev_batch(batch, spec, keep_mask, extra)
    p = to_dev_params(params)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A, flags=ops.flags_from_spec(spec), training=training,
                         drop_p=drop_p, seed=seed)
    ws = ops.alloc_workspace(dims, dev())
    scores = ops.forward(dims, b, p, ws)
    gt = batch["gt"].to(dev()).to(torch.int32)
    lr = ops.ranking_loss(scores, gt)
    grads = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    ops.backward(dims, b, p, ws, lr["dscores"], grads)
    torch.cuda.synchronize()
    inv = {v: k for k, v in FIELD.items()}
    return (scores.cpu(), lr, {inv[k]: v.cpu().numpy() for k, v in grads.items()})


def random_case(seed, B, d, scale=0.45):
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(a.astype(np.float32))
    batch = dict(image_features=t(np.abs(rng.standard_normal((B, d.K + 1, d.dv))) * scale),
                 q_emb=t(rng.standard_normal((B, d.dq)) * 0.3), z_orig=t(rng.standard_normal((B, d.dz))),
                 z_knns=t(rng.standard_normal((B, d.K, d.dz))), a_knns=t(rng.standard_normal((B, d.K, d.A)) * 2),
                 answer_aids=torch.from_numpy(rng.integers(0, d.A, size=B)), gt=torch.from_numpy(rng.integers(0, d.K, size=B)))
    return batch


def compare_with_oracle(d, spec, params, batch, training=False, drop_p=0.0, masks=None, seed=0, extra=None, use_rng=False, ref=None):
    """Logits <= 1e-4, loss <= 1e-5, ranks exact away from near-ties, every gradient <= 1e-4 of its tensor's max against the oracle.
    `ref`: the oracle's (scores, loss, grads) for these inputs when the caller already has them (else computed here)."""
    keep = None if masks is None or use_rng else torch.stack(masks)
    scores, lr, grads = run_hip(d, spec, params, batch, training=training, drop_p=drop_p, keep_mask=keep, seed=seed, extra=extra)
    ob = dict(batch)
    if extra:
        ob.update(extra)
    s_ref, l_ref, g_ref = ref if ref is not None else orc.loss_and_grads(params, d, ob, spec=spec, drop_p=drop_p, keep_masks=masks)
    assert np.abs(scores.numpy() - s_ref.numpy()).max() <= 1e-4
    assert abs(float(lr["loss"].cpu()) - float(l_ref)) <= 1e-5
    sr, gtn = s_ref.numpy(), batch["gt"].numpy()
    gap = np.abs(sr - sr[np.arange(len(gtn)), gtn][:, None]); gap[np.arange(len(gtn)), gtn] = np.inf
    safe = gap.min(1) > 2e-4                                  # rows without a near-tie around the ground truth
    assert (lr["rank"].cpu().numpy()[safe] == orc.rank_of_gt(sr, gtn)[safe]).all()
    for k, ref_g in g_ref.items():
        ref_g = ref_g.numpy()
        tol = grad_tol(k, ref_g, 1e-4)
        err = np.abs(grads[k].reshape(ref_g.shape) - ref_g).max()
        assert err <= tol, (k, err, tol)
    return scores, lr, grads


def full_size_case(d, B, seed, bf16=False, a_emb=True, tau=2e-5):
    """Seeded inputs conditioned away from the ReLU kinks.  a_emb=False: the a_emb lesion's inputs (a_knns is the [B, K, da] noise
    block, batch["a_emb_gt"] the [B, da] one: what the reference draws with torch.rand, cx.py:274-277)."""
    params = orc.init_params(d, seed=42)
    batch = random_case_f32(seed, B, d)
    spec = None
    if not a_emb:
        rng = np.random.default_rng(seed + 1)
        batch["a_knns"] = torch.from_numpy(rng.random((B, d.K, d.da), dtype=np.float32))
        batch["a_emb_gt"] = torch.from_numpy(rng.random((B, d.da), dtype=np.float32))
        spec = dict(orc.DEFAULT_SPEC, a_emb=False)
    batch["answer_aids"][1] = batch["answer_aids"][0]            # a duplicated answer id (owner-computes scatter)
    redrawn = condition_away_from_kinks(params, d, batch, seed, tau=tau, bf16=bf16, spec=spec)
    assert redrawn < 4 * B
    return params, batch


def check_phased_backward_bit_identical(d, params, batch):
    """ncx_backward_phase 1 then 2, 3 then 4, and 5 | 2 | 4 == ncx_backward, bit for bit (what the data-parallel engine relies on)."""
    from neuralcx import ops
    b = to_dev_batch(batch)
    p = to_dev_params(params)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A)
    ws = ops.alloc_workspace(dims, dev())
    scores = ops.forward(dims, b, p, ws)
    lr = ops.ranking_loss(scores, batch["gt"].to(dev()).to(torch.int32))
    g0 = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    ops.backward(dims, b, p, ws, lr["dscores"], g0)
    g12 = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    ops.backward(dims, b, p, ws, lr["dscores"], g12, phase=1)
    assert torch.isfinite(g12["answer_embedding"]).all() and torch.equal(g12["answer_embedding"], g0["answer_embedding"])
    ops.backward(dims, b, p, ws, lr["dscores"], g12, phase=2)
    for k in g0:
        assert torch.equal(g0[k], g12[k]), k
    # the other cut (3 | 4): everything but the embedding gradient, then the embedding gradient from dGt | dGgt;
    # scaling that workspace block by 2 in between doubles the embedding gradient exactly (linearity: what DP sums)
    g34 = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    ops.backward(dims, b, p, ws, lr["dscores"], g34, phase=3)
    for k in g0:
        if k != "answer_embedding":
            assert torch.equal(g0[k], g34[k]), k
    blk = ops.ws_dgt_view(dims, ws)
    assert blk.numel() == 2 * d.H * d.A
    ops.backward(dims, b, p, ws, lr["dscores"], g34, phase=4)
    assert torch.equal(g0["answer_embedding"], g34["answer_embedding"])
    blk.mul_(2.0)
    ops.backward(dims, b, p, ws, lr["dscores"], g34, phase=4)
    assert torch.equal(2.0 * g0["answer_embedding"], g34["answer_embedding"])
    # the three-way cut the DP engine uses (5 | 2 | 4): the block first, then linear_1.weight, then the embedding gradient
    g524 = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    ops.backward(dims, b, p, ws, lr["dscores"], g524, phase=5)
    assert torch.isnan(g524["answer_embedding"]).all() and torch.isnan(g524["w1"]).all()
    blk5 = ops.ws_dgt_view(dims, ws).clone()
    ops.backward(dims, b, p, ws, lr["dscores"], g524, phase=2)
    assert torch.equal(blk5, ops.ws_dgt_view(dims, ws))          # phase 2 leaves the exchanged block alone
    ops.backward(dims, b, p, ws, lr["dscores"], g524, phase=4)
    for k in g0:
        assert torch.equal(g0[k], g524[k]), k
