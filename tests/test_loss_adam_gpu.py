"""GPU: the kernels every trainable path ends in -- ncx_loss_rank, ncx_train_tail, ncx_adam_step, ncx_ce_loss -- at their edge shapes
against the fp64 restatements of tests/loss_adam_ref.py.  Exact quantities (ranks, hit counts, canaries, fused against unfused bits) carry
no tolerance; the listwise / cross-entropy bounds are 4 x torch-float32's own error + one ulp (loss_adam_ref.YARDSTICK, measured in
tests/test_loss_adam_cpu.py, recorded with the kernels' errors in profiles/loss_adam_edges.json); the Adam bounds count k_adam's fp32
roundings (loss_adam_ref.adam_bounds)."""
import ctypes as C

import numpy as np
import pytest
import torch

import loss_adam_ref as R
from helpers import dev, grad_tol, random_case, to_dev_batch, to_dev_params, FIELD
from oracle import ncx_oracle as orc

pytestmark = pytest.mark.gpu


def _t(a, dt=torch.float32):
    return torch.from_numpy(np.ascontiguousarray(a)).to(dev(), dt)


def _vp(t, off=0):
    return None if t is None else C.c_void_p(t.data_ptr() + off)


# ---- ncx_loss_rank -------------------------------------------------------------------------------------------------------------------
CANARY = 7.0


def _loss_rank_raw(s, gt, scale, want=("loss_rows", "loss", "dscores", "rank", "hits")):
    """The raw C call with NaN-filled outputs, each followed by a canary tail; outputs not in `want` are passed as NULL and their buffers
    must stay as they were.  -> dict of host arrays (the NaN fill where an output was not asked for)."""
    from neuralcx import _lib
    B, K = s.shape
    sizes = dict(loss_rows=B, loss=1, dscores=B * K, rank=B, hits=2)
    bufs = {}
    for k, n in sizes.items():
        if k in ("rank", "hits"):
            bufs[k] = torch.full((n + 16,), -77, dtype=torch.int32, device=dev())
        else:
            bufs[k] = torch.full((n + 16,), float("nan"), device=dev())
            bufs[k][n:] = CANARY
    arg = lambda k: _vp(bufs[k]) if k in want else None
    sd, gd = _t(s), _t(gt, torch.int32)                                # (named: they must outlive the call)
    rc = _lib.lib().ncx_loss_rank(_vp(sd), _vp(gd), B, K, float(scale), arg("loss_rows"), arg("loss"), arg("dscores"),
                                  arg("rank"), arg("hits"), C.c_void_p(torch.cuda.current_stream().cuda_stream))
    assert rc == 0, rc
    torch.cuda.synchronize()
    out = {}
    for k, n in sizes.items():
        h = bufs[k].cpu().numpy()
        if k in ("rank", "hits"):
            assert (h[n:] == -77).all(), k
            assert (h[:n] != -77).all() if k in want else (h[:n] == -77).all(), k          # fully overwritten / untouched
        else:
            assert (h[n:] == CANARY).all(), k
            assert np.isfinite(h[:n]).all() if k in want else np.isnan(h[:n]).all(), k
        out[k] = h[:n]
    out["dscores"] = out["dscores"].reshape(B, K)
    return out


@pytest.mark.parametrize("family", R.FAMILIES)
@pytest.mark.parametrize("B,K", R.LOSS_RANK_SHAPES)
def test_loss_rank_against_fp64(B, K, family):
    """loss_rows, loss and dscores inside 4 x torch-float32's error + 1 ulp; rank and both hit counts exact; every output overwritten, none
    beyond its end; a second call bit-identical.  The +-1e4 family is what the association of the loss decides: log(sum) - (s_gt - max)
    keeps the row's offset out of the sum (log(sum) + max - s_gt rounds at the offset's magnitude: ~5e-4 there)."""
    s, gt, planted = R.listwise_case(B, K, family, seed=1)           # (the cases the yardstick was measured on)
    worst = dict(loss_rows=0.0, loss=0.0, dscores=0.0)
    for scale in R.SCALES:
        ref = R.listwise_ref(s, gt, scale)
        got = _loss_rank_raw(s, gt, scale)
        assert (got["rank"] == ref["rank"]).all()
        assert (got["hits"] == ref["hits"]).all()
        err = R.listwise_errors(got["loss_rows"], got["loss"][0], got["dscores"], ref, B)
        worst = {k: max(worst[k], err[k]) for k in worst}
        again = _loss_rank_raw(s, gt, scale)
        for k in got:
            assert np.array_equal(got[k], again[k]), k
    print("hip_err loss_rank %s B=%d K=%d %s" % (family, B, K, " ".join("%s=%.3e" % kv for kv in sorted(worst.items()))))
    for scale in R.SCALES:
        ref = R.listwise_ref(s, gt, scale)
        got = _loss_rank_raw(s, gt, scale)
        tol = R.listwise_bounds(ref, family, B)
        assert (np.abs(got["loss_rows"] - ref["loss_rows"]) <= tol["loss_rows"]).all(), (scale, np.abs(got["loss_rows"] - ref["loss_rows"]).max())
        assert abs(float(got["loss"][0]) - ref["loss"]) <= tol["loss"], (scale, float(got["loss"][0]), ref["loss"])
        assert (np.abs(got["dscores"] - ref["dscores"]) <= tol["dscores"]).all(), (scale, np.abs(got["dscores"] - ref["dscores"]).max())


@pytest.mark.parametrize("K", [1, 2, 5, 6, 24, 25, 64])
def test_loss_rank_every_planted_row_at_every_width(K):
    """All seven planted rows (gt first / last, exactly 5th / 6th, a tie ahead / behind, all equal) at once, in each family: rank and hit
    counts exact.  (The sweep above rotates them through its rows; B = 5 holds only five.)"""
    n = len(R.PLANTS)
    for family in R.FAMILIES:
        s, gt, planted = R.listwise_case(n, K, family, seed=3)
        ref = R.listwise_ref(s, gt, 0.0)
        got = _loss_rank_raw(s, gt, 0.0)
        assert (got["rank"] == ref["rank"]).all(), (family, got["rank"], ref["rank"])
        assert (got["hits"] == ref["hits"]).all()


@pytest.mark.parametrize("want", [("loss_rows", "rank"), ("loss_rows", "loss"), ("rank", "hits"), ("rank",), ("dscores",),
                                  ("loss_rows", "loss", "rank", "hits")])
def test_loss_rank_outputs_not_asked_for_stay_untouched(want):
    """want_grad = False (no dscores), loss / hits NULL, and the other nullable combinations the entry point accepts: what is asked for
    equals the full call bit for bit, what is not stays as it was."""
    B, K = 257, 24
    s, gt, _ = R.listwise_case(B, K, "ordinary", seed=4)
    full = _loss_rank_raw(s, gt, 1.0 / 7.0)
    part = _loss_rank_raw(s, gt, 1.0 / 7.0, want=want)
    for k in want:
        assert np.array_equal(full[k], part[k]), k


def test_loss_rank_through_ops_without_the_gradient():
    from neuralcx import ops
    s, gt, _ = R.listwise_case(5, 25, "ordinary", seed=5)
    a = ops.ranking_loss(_t(s), _t(gt, torch.int32), scale=1.0)
    b = ops.ranking_loss(_t(s), _t(gt, torch.int32), scale=1.0, want_grad=False)
    assert b["dscores"] is None
    for k in ("loss", "loss_rows", "rank", "hits"):
        assert torch.equal(a[k], b[k]), k
    ref = R.listwise_ref(s, gt, 1.0)
    assert (a["rank"].cpu().numpy() == ref["rank"]).all()


# ---- ncx_train_tail ------------------------------------------------------------------------------------------------------------------
# (B, K, H, L) and what the case is there for.  dv / dq / dz / A as the existing tail test (96 / 64 / 24 / 40); da = 64 keeps the oracle of
# the two B > 1024 cases inside a second.  A = 41 where the zero buffer's split matters (below).
TAIL_CASES = {
    "B1_K3_H4":        dict(B=1, K=3, H=4, L=1),                       # one live lane, three blocks with an empty run
    "B3_K8_H5":        dict(B=3, K=8, H=5, L=1),                       # KB = 8 full; the edge lane holds 1 of 4 columns
    "B5_K9_H7_L2":     dict(B=5, K=9, H=7, L=2),                       # KB = 16 with 9 rows; edge lane 3 of 4; no dsh
    "B6_K16_H253":     dict(B=6, K=16, H=253, L=1),                    # KB = 16 full; the last lane's three-way put4
    "B7_K17_H255_L3":  dict(B=7, K=17, H=255, L=3),                    # KB = 24 with 17 rows
    "B2_K24_H256_L2":  dict(B=2, K=24, H=256, L=2),                    # FULL without dsh
    "B1025_K12_H36":   dict(B=1025, K=12, H=36, L=1, da=64),           # runs of more than one triplet on the KB = 16 body
    "B1030_K24_H256":  dict(B=1030, K=24, H=256, L=1, da=64),          # FULL, uneven runs (1030 over 1024 waves)
    # the zero buffer (dGgt, which the backward scatters into): three choices in ncx_train_tail.  ncx_plan_query does not report
    # routes().emb_nt; by ncx_plan.hip's rule it is a_emb && !bf16 && !NCX_NO_EMB_NT (an experiment hook), so: the default fp32 call is
    # the emb_nt side (buffer dGgt^T, A * pad4(H) floats), the hook gives the other side (dGgt, H * A floats), the a_emb lesion none.
    # B = 9 -> nblk * 4 = 12 blocks; A = 41, H = 50: A * pad4(H) = 2132 and H * A = 2050, neither a multiple of 4 * 12 * 4 = 192
    "emb_nt_A41":      dict(B=9, K=5, H=50, L=1, A=41),
    "no_emb_nt_A41":   dict(B=9, K=5, H=50, L=1, A=41, hook="NCX_NO_EMB_NT"),
    "lesion_A41":      dict(B=9, K=5, H=50, L=1, A=41, lesion=True),
}


def _tail_case(c, zero_out=False):
    d = orc.Dims(K=c["K"], dv=96, dq=64, dz=24, da=c.get("da", orc.DIM_A), A=c.get("A", 40), H=c["H"], L=c["L"])
    B = c["B"]
    params = orc.init_params(d, seed=12, gain=3.0)
    if zero_out:
        params["out.weight"] = torch.zeros_like(params["out.weight"])
    batch = random_case(41, B, d)
    if B > 1:
        batch["answer_aids"][0] = batch["answer_aids"][B - 1]          # a duplicated answer id
    spec, extra = None, {}
    if c.get("lesion"):
        torch.manual_seed(3)
        batch["a_knns"] = torch.rand(B, d.K, d.da); extra["a_emb_gt"] = torch.rand(B, d.da)
        spec = dict(orc.DEFAULT_SPEC, a_emb=False)
    if B > 1000:      # enough pre-activations for one to sit on the ReLU kink, where summation order alone decides a gradient gate
        from helpers import condition_away_from_kinks
        condition_away_from_kinks(params, d, batch, 41, spec=spec)
    return d, B, params, batch, spec, extra


def _tail_run(d, B, params, batch, spec, extra, fused, seed=77, drop_p=0.25):
    """forward, (train_tail | ranking_loss), backward on a NaN-filled workspace with NaN-filled gradients"""
    from neuralcx import ops, _lib
    b = to_dev_batch(batch, spec, None, extra)
    p = to_dev_params(params)
    gt = batch["gt"].to(dev()).to(torch.int32)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A, flags=ops.flags_from_spec(spec), training=True, drop_p=drop_p,
                         loss_scale=1.0 / B, seed=seed)
    if fused:
        assert ops.fused_tail_ok(dims)
        dims.flags |= _lib.NCX_F_FUSED_TAIL
    ws = ops.alloc_workspace(dims, dev())
    ws.fill_(0xFF)                                                     # every float of the workspace a NaN (every int -1)
    g = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    scores = ops.forward(dims, b, p, ws)
    r = ops.train_tail(dims, p, ws, scores, gt, g, want_dscores=True) if fused else ops.ranking_loss(scores, gt, scale=1.0 / B)
    ops.backward(dims, b, p, ws, None if fused else r["dscores"], g)
    torch.cuda.synchronize()
    return scores, r, g


def _check_tail(c, d, B, params, batch, spec, extra):
    seed, drop_p = 77, 0.25
    s0, r0, g0 = _tail_run(d, B, params, batch, spec, extra, False, seed, drop_p)
    s1, r1, g1 = _tail_run(d, B, params, batch, spec, extra, True, seed, drop_p)
    live = [k for k in g0 if not (d.L < 3 and k in ("w3", "b3") or d.L < 2 and k in ("w2", "b2"))]
    # 3. fused == unfused, bit for bit except d out.bias (zero in mathematics, summed in another order)
    assert torch.equal(s0, s1)
    for k in ("loss", "loss_rows", "dscores", "rank", "hits"):
        assert torch.equal(r0[k], r1[k]), k
    for k in live:
        assert torch.isfinite(g0[k]).all() and torch.isfinite(g1[k]).all(), k
        if k == "b_out":
            assert abs(float(g0[k]) - float(g1[k])) <= 1e-6, k
        else:
            assert torch.equal(g0[k], g1[k]), k
    # 1. the tail's loss / dscores / rank / hits against fp64 on the scores it RETURNED
    sn = s1.cpu().numpy()
    gtn = batch["gt"].numpy()
    ref = R.listwise_ref(sn, gtn, 1.0 / B)
    tol = R.listwise_bounds(ref, "ordinary", B)
    assert (r1["rank"].cpu().numpy() == ref["rank"]).all()
    assert (r1["hits"].cpu().numpy() == ref["hits"]).all()
    rows, dsc = r1["loss_rows"].cpu().numpy(), r1["dscores"].cpu().numpy()
    err = R.listwise_errors(rows, float(r1["loss"]), dsc, ref, B)
    print("hip_err train_tail ordinary B=%d K=%d %s" % (B, d.K, " ".join("%s=%.3e" % kv for kv in sorted(err.items()))))
    assert (np.abs(rows - ref["loss_rows"]) <= tol["loss_rows"]).all(), np.abs(rows - ref["loss_rows"]).max()
    assert abs(float(r1["loss"]) - ref["loss"]) <= tol["loss"]
    assert (np.abs(dsc - ref["dscores"]) <= tol["dscores"]).all(), np.abs(dsc - ref["dscores"]).max()
    # 2. scores and every gradient against the oracle with the same keep masks (the suite's rule: logits 1e-4, gradients 1e-4 of the max)
    masks = [orc.dropout_keep_mask(seed, l, B * d.K, d.H, drop_p) for l in range(1, d.L + 1)]
    ob = dict(batch); ob.update(extra)
    s_ref, l_ref, g_ref = orc.loss_and_grads(params, d, ob, spec=spec, drop_p=drop_p, keep_masks=masks)
    assert np.abs(sn - s_ref.numpy()).max() <= 1e-4
    for name, ref_g in g_ref.items():
        ref_g = ref_g.numpy()
        for which, g in (("unfused", g0), ("fused", g1)):
            e = np.abs(g[FIELD[name]].cpu().numpy().reshape(ref_g.shape) - ref_g).max()
            # 4. answer_embedding is the zero buffer's consumer: right in both runs, after a NaN-filled workspace
            assert e <= grad_tol(name, ref_g, 1e-4), (name, which, e, grad_tol(name, ref_g, 1e-4))
    return r1, g1


@pytest.mark.parametrize("case", sorted(TAIL_CASES))
def test_train_tail_edge_shapes_against_fp64_and_oracle(case, monkeypatch):
    """The four checks of _check_tail per shape.  B3_K8_H5 and B6_K16_H253 are also the only cases of the suite in which the fused forward
    kernel (csrc/ncx_main.h) writes an output with H % 4 == 1 from its unsplit epilogue: there the last, one-column piece of a row takes
    its row-add operand (Sh[b][H - 1]) out of a 16-byte window slid three elements to the left.  That selection once returned element 1
    of the window -- h1[r][H - 1] = relu(pre + Sh[b][H - 3] - Sh[b][H - 1]), scores 0.24 and 0.025 off the oracle here -- and check 2
    is what caught it."""
    from neuralcx import ops
    monkeypatch.setattr(ops, "EXTRA_FLAGS", 0)
    c = TAIL_CASES[case]
    if c.get("hook"):
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        monkeypatch.setenv(c["hook"], "1")
    _check_tail(c, *_tail_case(c))


def test_train_tail_all_scores_tied():
    """out.weight = 0: every score equals the bias, so rank == gt (the tie rule), dscores = (1/K - onehot) / B, and everything dpre feeds
    -- every gradient below the out layer -- is exactly zero."""
    c = dict(B=6, K=16, H=253, L=2)
    d, B, params, batch, spec, extra = _tail_case(c, zero_out=True)
    batch["gt"] = torch.tensor([0, 15, 4, 5, 7, 9])
    s, r, g = _tail_run(d, B, params, batch, spec, extra, True)
    assert (s == params["out.bias"].item()).all()
    assert (r["rank"].cpu().numpy() == batch["gt"].numpy()).all()
    assert r["hits"].cpu().tolist() == [1, 2]
    ref = R.listwise_ref(s.cpu().numpy(), batch["gt"].numpy(), 1.0 / B)
    tol = R.listwise_bounds(ref, "ordinary", B)
    assert (np.abs(r["dscores"].cpu().numpy() - ref["dscores"]) <= tol["dscores"]).all()
    assert abs(float(r["loss"]) - ref["loss"]) <= tol["loss"]
    for k in ("answer_embedding", "w1", "b1", "w2", "b2"):
        assert (g[k] == 0).all(), k
    assert torch.isfinite(g["w_out"]).all() and torch.isfinite(g["b_out"]).all()


# ---- ncx_adam_step -------------------------------------------------------------------------------------------------------------------
def _adam_hip(p, g, m, v, step, hp, gs, margin=0):
    """-> p', m', v' (host) after one ncx_adam_step on device copies; margin: the state sits at [margin : margin + n] of buffers with
    canaries on both sides, which must come back unchanged (g's too)."""
    from neuralcx import ops
    n = p.size
    bufs = []
    for i, a in enumerate((p, g, m, v)):
        t = torch.full((n + 2 * margin,), 1000.0 + i, device=dev())
        t[margin:margin + n] = _t(a)
        bufs.append(t)
    views = [t[margin:margin + n] for t in bufs]
    ops.adam_step(views[0], views[1], views[2], views[3], step, lr=hp["lr"], betas=hp["betas"], eps=hp["eps"], grad_scale=gs)
    torch.cuda.synchronize()
    for i, t in enumerate(bufs):
        h = t.cpu().numpy()
        assert (h[:margin] == np.float32(1000.0 + i)).all() and (h[margin + n:] == np.float32(1000.0 + i)).all(), "margin of buffer %d" % i
    assert np.array_equal(bufs[1][margin:margin + n].cpu().numpy(), g)
    return tuple(bufs[i][margin:margin + n].cpu().numpy() for i in (0, 2, 3))


def _adam_check(n, step, family, hp, gs, margin=0, seed=1):
    p, g, m, v = R.adam_case(n, step, family, seed)
    args = (step, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], gs)
    ref = R.adam_ref_step(p, g, m, v, *args)
    tol = R.adam_bounds(p, g, m, v, *args)
    got = _adam_hip(p, g, m, v, step, hp, gs, margin)
    worst = 0.0
    for name, a, r, t in zip("pmv", got, ref, tol):
        assert np.isfinite(a).all(), name
        err = np.abs(a.astype(np.float64) - r)
        assert (err <= t).all(), (name, n, step, family, hp, gs, margin, float((err - t).max()), int((err > t).sum()))
        worst = max(worst, float((err[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0)
    if family == "zero":
        if step == 1:
            assert np.array_equal(got[0], p)                          # m = 0 and g = 0: p does not move, to the bit
        assert (got[2] <= v).all() and (np.abs(got[1]) <= np.abs(m)).all()
    return got, worst


@pytest.mark.parametrize("n", R.ADAM_SIZES)
def test_adam_one_step_against_fp64(n):
    """Every size around the vector body / scalar tail boundary, every step count, gradient family, hyper-parameter set and grad_scale:
    one step from a given fp32 state inside the rounding-count bound, element by element."""
    worst = 0.0
    for step in R.ADAM_STEPS:
        for family in R.ADAM_FAMILIES:
            for hp in (R.HP_DEFAULT, R.HP_ALT):
                for gs in R.ADAM_GRAD_SCALES:
                    worst = max(worst, _adam_check(n, step, family, hp, gs)[1])
    print("hip_err adam n=%d worst error / bound %.3f" % (n, worst))


def test_adam_zero_gradient_and_zero_momentum_leaves_p_alone_at_any_step():
    for n in (3, 1025):
        for step in (2, 1000):
            p, g, m, v = R.adam_case(n, step, "zero")
            m = np.zeros_like(m)
            got = _adam_hip(p, g, m, v, step, R.HP_DEFAULT, 3.7)
            assert np.array_equal(got[0], p) and (got[1] == 0).all()
            ref = R.adam_ref_step(p, g, m, v, step, 1e-4, 0.9, 0.999, 1e-8, 3.7)
            assert (np.abs(got[2] - ref[2]) <= R.adam_bounds(p, g, m, v, step, 1e-4, 0.9, 0.999, 1e-8, 3.7)[2]).all()


@pytest.mark.parametrize("n", [3, 5, 7, 1023, 1025])
def test_adam_on_a_slice_with_live_neighbours(n):
    """The data-parallel engine's call pattern: [64 : 64 + n] of four larger buffers.  The margins come back bit-identical (a vector store
    past n would land in the next tensor's moments), the body matches the reference.  n = 3, 7, 1023 (n % 4 == 3) are the sizes at which
    a vector body taken one quad too far (`i + 3 <= n`) writes exactly one element past the slice."""
    for step, family, hp, gs in ((1, "normal", R.HP_DEFAULT, 1.0), (10, "mixed", R.HP_ALT, 1.0 / 8.0), (1000, "flip", R.HP_DEFAULT, 3.7)):
        _adam_check(n, step, family, hp, gs, margin=64)


def test_adam_grid_stride_loop_and_its_tail():
    """n = 4096 * 1024 + 1029: more than one pass of the 4096-block grid, then a vector body, then a one-element scalar tail."""
    n = R.ADAM_BIG
    for step, family, hp, gs in ((1, "normal", R.HP_DEFAULT, 1.0), (10, "mixed", R.HP_ALT, 3.7)):
        _adam_check(n, step, family, hp, gs, margin=64)


def test_adam_two_calls_are_bit_identical():
    for n in (7, 1025):
        p, g, m, v = R.adam_case(n, 10, "mixed")
        a = _adam_hip(p, g, m, v, 10, R.HP_ALT, 3.7)
        b = _adam_hip(p, g, m, v, 10, R.HP_ALT, 3.7)
        for x, y in zip(a, b):
            assert np.array_equal(x, y)


# ---- ncx_ce_loss ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A", R.CE_SHAPES)
def test_ce_loss_edge_shapes(B, A):
    """test_ce_loss_alone's reference, rows and assertions (tests/test_vqa_train_gpu.py) at A around the 256-thread block and B past the
    256-thread finish; its bad-target guard at a row of this shape."""
    from neuralcx import ops
    from test_vqa_train_gpu import _ce_into
    x, t, expect = R.ce_case(B, A)
    ref = R.ce_ref(x, t)
    ce = ops.ce_loss(_t(x), _t(t, torch.int32))
    torch.cuda.synchronize()
    ops.check_vqa_targets(device=dev())
    err = abs(float(ce["loss"].cpu()) - ref["loss"])
    e = np.abs(ce["dlogits"].cpu().numpy() - ref["dl"]).max()
    print("hip_err ce_loss B=%d A=%d loss=%.3e dlogits=%.3e" % (B, A, err, e))
    assert err <= 1e-5 * max(1.0, abs(ref["loss"]))
    assert e <= 1e-4 * np.abs(ref["dl"]).max(), e
    assert int(ce["hits1"].cpu()) == int((ref["rank"] < 1).sum())
    assert int(ce["hits5"].cpu()) == int((ref["rank"] < 5).sum())
    for r, rk in expect.items():
        assert ref["rank"][r] == rk
    again = ops.ce_loss(_t(x), _t(t, torch.int32))
    assert torch.equal(ce["loss"], again["loss"]) and torch.equal(ce["dlogits"], again["dlogits"])
    for bad in (-1, A):
        row = B - 1
        t2 = t.copy(); t2[row] = bad
        guard = torch.full((B * A + 64,), 7.0, device=dev())
        ce2 = _ce_into(x, t2, guard, B, A)
        torch.cuda.synchronize()
        assert (guard[B * A:] == 7.0).all()
        assert (guard[row * A:(row + 1) * A] == 0).all()
        keep = np.arange(B) != row
        want = R.ce_ref(x[keep], t[keep], scale=1.0 / B)["loss"] if B > 1 else 0.0
        assert abs(float(ce2.cpu()) - want) <= 1e-5 * max(1.0, abs(want))
        with pytest.raises(IndexError):
            ops.check_vqa_targets(device=dev())
        ops.check_vqa_targets(device=dev())


@pytest.mark.parametrize("B,A", [(3, 257), (300, 7)])
def test_ce_loss_rows_shifted_by_1e4(B, A):
    """The same association as the listwise loss (log(sum) - (x_t - max)): a logit row at +-1e4 keeps the loss of the unshifted row to
    4 x torch-float32's error + 1 ulp (the listwise yardstick's offset family; loss per row, then / B)."""
    from neuralcx import ops
    x, t, _ = R.ce_case(B, A)
    x[0] = np.clip(x[0], -10, 10)                                     # (row 0 holds the +-80 pair: another family)
    sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0).astype(np.float32)
    xs = (x + sign[:, None] * np.float32(1e4)).astype(np.float32)
    ref = R.listwise_ref(xs, t, 0.0)
    ce = ops.ce_loss(_t(xs), _t(t, torch.int32))
    torch.cuda.synchronize()
    ops.check_vqa_targets(device=dev())
    tol = R.listwise_bounds(ref, "offset1e4", B)
    err = abs(float(ce["loss"].cpu()) - ref["loss"])
    print("hip_err ce_loss offset1e4 B=%d A=%d loss=%.3e (per row %.3e)" % (B, A, err, err / (ref["scale"] * B)))
    assert err <= tol["loss"], (err, tol["loss"])
    assert np.abs(ce["dlogits"].cpu().numpy() - ref["dscores"]).max() <= 1e-4 * np.abs(ref["dscores"]).max()      # (test_ce_loss_alone's rule)
    assert int(ce["hits1"].cpu()) == ref["hits"][0] and int(ce["hits5"].cpu()) == ref["hits"][1]
