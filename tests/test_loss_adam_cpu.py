"""CPU: pins the fp64 restatements and case builders of tests/loss_adam_ref.py (what tests/test_loss_adam_gpu.py holds the HIP kernels
to) against torch in float64, measures the float32 yardstick of the listwise / cross-entropy tolerances, checks the Adam rounding bound on
torch's own float32 optimiser, and the host-side argument checks of ncx_loss_rank / ncx_adam_step (no launch)."""
import ctypes as C
import json
import os

import numpy as np
import pytest
import torch
import torch.nn.functional as F

import loss_adam_ref as R
from conftest import ROOT
from oracle import ncx_oracle as orc

PROFILE = os.path.join(ROOT, "profiles", "loss_adam_edges.json")


# ---- listwise_ref ----------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("family", R.FAMILIES)
def test_listwise_ref_is_torch_float64(family):
    for B, K in R.LOSS_RANK_SHAPES:
        s, gt, _ = R.listwise_case(B, K, family, seed=1)
        for scale in R.SCALES:
            ref = R.listwise_ref(s, gt, scale)
            sc = ref["scale"]
            assert sc == (R.f32(scale) if scale > 0 else float(np.float32(1.0) / np.float32(B)))
            t = torch.from_numpy(s).double().requires_grad_(True)
            g = torch.from_numpy(gt.astype(np.int64))
            loss = F.cross_entropy(t, g, reduction="sum") * sc
            loss.backward()
            rows = F.cross_entropy(t.detach(), g, reduction="none") * sc
            assert abs(ref["loss"] - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
            assert np.abs(ref["loss_rows"] - rows.numpy()).max() <= 1e-12 * max(1.0, float(rows.abs().max()))
            assert np.abs(ref["dscores"] - t.grad.numpy()).max() <= 1e-14
            assert abs(ref["dscores"].sum(1)).max() <= 1e-15 * K          # rows of softmax - onehot sum to zero
            assert (ref["rank"] == orc.rank_of_gt(s, gt)).all()
            assert ref["hits"][0] == (ref["rank"] < 1).sum() and ref["hits"][1] == (ref["rank"] < 5).sum()


def test_listwise_rank_is_recall_at_k_where_no_tie_sits_on_the_boundary():
    """oracle.recall_at_k (the reference's topk rule) == (rank < k) on every row whose k-th and (k+1)-th scores differ."""
    for B, K in R.LOSS_RANK_SHAPES:
        if K < 6:
            continue
        for family in R.FAMILIES:
            s, gt, _ = R.listwise_case(B, K, family, seed=2)
            rank = R.listwise_ref(s, gt, 0.0)["rank"]
            srt = -np.sort(-s, axis=1)
            for k in (1, 5):
                clear = srt[:, k - 1] != srt[:, k]
                rec = orc.recall_at_k(torch.from_numpy(s), torch.from_numpy(gt.astype(np.int64)), k)
                assert clear.sum() >= B // 2
                assert ((rank < k).astype(np.int64)[clear] == rec[clear]).all()


@pytest.mark.parametrize("K", [1, 2, 5, 6, 24, 64])
def test_listwise_planted_rows_are_what_the_builder_says(K):
    n = len(R.PLANTS)
    for rot in range(n):
        s, gt, planted = R.listwise_case(n, K, "ordinary", seed=3, rot=rot)
        rank = R.listwise_ref(s, gt, 0.0)["rank"]
        assert sorted(planted.values()) == sorted(name for name, need in R.PLANTS if K >= need)
        for r, name in planted.items():
            greater = int((s[r] > s[r, gt[r]]).sum())
            if name == "gt_first":
                assert gt[r] == 0
            elif name == "gt_last":
                assert gt[r] == K - 1
            elif name == "fifth":
                assert rank[r] == 4 and greater == 4 and np.sort(s[r])[-5] == s[r, gt[r]]
            elif name == "sixth":
                assert rank[r] == 5 and greater == 5 and np.sort(s[r])[-6] == s[r, gt[r]]
            elif name == "tie_ahead":
                ties = np.flatnonzero(s[r] == s[r, gt[r]])
                assert len(ties) == 2 and ties[0] < gt[r] == ties[1] and rank[r] == greater + 1
            elif name == "tie_behind":
                ties = np.flatnonzero(s[r] == s[r, gt[r]])
                assert len(ties) == 2 and ties[1] > gt[r] == ties[0] and rank[r] == greater
            elif name == "all_equal":
                assert (s[r] == s[r, 0]).all() and rank[r] == gt[r]
    # the two other families keep gt valid and do what their names say
    s, gt, _ = R.listwise_case(9, K, "spread80", seed=3)
    if K > 1:
        assert ((s.max(1) - np.sort(s, axis=1)[:, -2] >= 80.0)[0::2]).all() and ((np.sort(s, axis=1)[:, 1] - s.min(1) >= 80.0)[1::2]).all()
    s, gt, _ = R.listwise_case(9, K, "offset1e4", seed=3)
    assert (s[0::2] > 9.9e3).all() and (s[1::2] < -9.9e3).all()


def _yardstick():
    """torch-float32's error against listwise_ref over the sweep, per family and quantity, in YARDSTICK's units."""
    out = {}
    for family in R.FAMILIES:
        worst = dict(loss_rows=0.0, loss=0.0, dscores=0.0)
        for B, K in R.LOSS_RANK_SHAPES:
            s, gt, _ = R.listwise_case(B, K, family, seed=1)
            for scale in R.SCALES:
                ref = R.listwise_ref(s, gt, scale)
                rows, loss, d = R.torch_f32_listwise(s, gt, ref["scale"])
                e = R.listwise_errors(rows, loss, d, ref, B)
                worst = {k: max(worst[k], e[k]) for k in worst}
        out[family] = worst
    return out


def test_listwise_yardstick_constants_are_the_measured_float32_error():
    """YARDSTICK is torch-float32's measured error, rounded up: never below it, and at most twice above it (the profile file holds the
    figures of the machine that wrote them; another CPU's vector exp may move a last digit, not a factor)."""
    got = _yardstick()
    for family in R.FAMILIES:
        for q, c in R.YARDSTICK[family].items():
            print("yardstick %-9s %-9s measured %.3e  constant %.3e" % (family, q, got[family][q], c))
    for family in R.FAMILIES:
        for q, c in R.YARDSTICK[family].items():
            assert got[family][q] <= c <= 2.0 * max(got[family][q], R.U32), (family, q, got[family][q], c)
    prof = json.load(open(PROFILE))
    for family in R.FAMILIES:
        assert prof["listwise"][family]["yardstick_constant"] == R.YARDSTICK[family]


# ---- ce_ref ----------------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("B,A", R.CE_SHAPES + ((9, 5), (9, 2000)))
def test_ce_ref_is_torch_float64_and_its_planted_rows(B, A):
    x, t, expect = R.ce_case(B, A)
    ref = R.ce_ref(x, t)
    xt = torch.from_numpy(x).double().requires_grad_(True)
    loss = F.cross_entropy(xt, torch.from_numpy(t.astype(np.int64)), reduction="sum") / B
    loss.backward()
    assert abs(ref["loss"] - float(loss)) <= 1e-12 * max(1.0, abs(float(loss)))
    assert np.abs(ref["dl"] - xt.grad.numpy()).max() <= 1e-14
    assert (ref["rank"] == orc.rank_of_gt(x, t)).all()
    for r, rk in expect.items():
        assert ref["rank"][r] == rk, (r, rk)
    if A > 5 and B > 4:
        assert expect[3] == 4 and expect[4] == 5


# ---- adam_ref_step ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("hp", [R.HP_DEFAULT, R.HP_ALT])
def test_adam_ref_iterated_is_torch_adam_float64(hp):
    rng = np.random.default_rng(5)
    n = 257
    p = rng.standard_normal(n); m = np.zeros(n); v = np.zeros(n)
    tp = torch.from_numpy(p.copy()).requires_grad_(True)
    opt = torch.optim.Adam([tp], lr=hp["lr"], betas=hp["betas"], eps=hp["eps"])
    for step in range(1, 41):
        g = rng.standard_normal(n) * (0.01 * step)
        p, m, v = R.adam_ref_step(p, g, m, v, step, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], round_scalars=False)
        tp.grad = torch.from_numpy(g.copy()); opt.step()
        assert np.abs(p - tp.detach().numpy()).max() <= 1e-12 * np.abs(p).max()
        st = opt.state[tp]
        assert np.abs(m - st["exp_avg"].numpy()).max() <= 1e-12 * np.abs(m).max()
        assert np.abs(v - st["exp_avg_sq"].numpy()).max() <= 1e-12 * np.abs(v).max()


def test_adam_ref_rounds_the_scalars_as_the_entry_point_does():
    p = np.float32([1.0]); g = np.float32([0.5]); z = np.float32([0.0])
    a = R.adam_ref_step(p, g, z, z, 1, 1e-3, 0.9, 0.999, 1e-8)
    b = R.adam_ref_step(p, g, z, z, 1, 1e-3, 0.9, 0.999, 1e-8, round_scalars=False)
    assert a[1][0] == 0.5 * (1.0 - R.f32(0.9)) and b[1][0] == 0.5 * (1.0 - 0.9) and a[1][0] != b[1][0]
    assert abs(a[0][0] - b[0][0]) <= 4 * R.U32 * 1e-3


def _torch_adam_f32_step(p, g, m, v, step, hp, gs):
    tp = torch.from_numpy(p.copy()).requires_grad_(True)
    # the hyper-parameters as the C call receives them (floats): 1 - beta2^step is ill-conditioned in beta2 at small steps, the double
    # 0.999 and the float 0.999 are 1.3e-5 apart there -- a property of the float ABI, not a rounding of the kernel
    opt = torch.optim.Adam([tp], lr=R.f32(hp["lr"]), betas=(R.f32(hp["betas"][0]), R.f32(hp["betas"][1])), eps=R.f32(hp["eps"]), foreach=False)
    opt.state[tp] = dict(step=torch.tensor(float(step - 1)), exp_avg=torch.from_numpy(m.copy()), exp_avg_sq=torch.from_numpy(v.copy()))
    tp.grad = torch.from_numpy(g) * torch.tensor(gs, dtype=torch.float32)
    opt.step()
    st = opt.state[tp]
    return tp.detach().numpy(), st["exp_avg"].numpy(), st["exp_avg_sq"].numpy()


@pytest.mark.parametrize("family", R.ADAM_FAMILIES)
def test_adam_bound_holds_torch_float32_adam(family):
    """The rounding-count bound is checked on an fp32 Adam nobody here wrote: torch.optim.Adam in float32 from the same states must sit
    inside it (one more rounding than k_adam: torch divides by sqrt(bc2) where the kernel multiplies by the rounded reciprocal -- a
    relative 1.5 u on |dp|, inside the 9 u of the bound at the sizes measured here).  The worst ratio is printed."""
    worst = dict(p=0.0, m=0.0, v=0.0)
    for n in (7, 1025):
        for step in R.ADAM_STEPS:
            for hp in (R.HP_DEFAULT, R.HP_ALT):
                for gs in R.ADAM_GRAD_SCALES:
                    p, g, m, v = R.adam_case(n, step, family, seed=1)
                    args = (step, hp["lr"], hp["betas"][0], hp["betas"][1], hp["eps"], gs)
                    ref = R.adam_ref_step(p, g, m, v, *args)
                    tol = R.adam_bounds(p, g, m, v, *args)
                    got = _torch_adam_f32_step(p, g, m, v, step, hp, gs)
                    for name, a, r, t in zip("pmv", got, ref, tol):
                        err = np.abs(a.astype(np.float64) - r)
                        assert (err <= t).all(), (name, n, step, hp, gs, float((err - t).max()))
                        worst[name] = max(worst[name], float((err[t > 0] / t[t > 0]).max()) if (t > 0).any() else 0.0)
    print("torch float32 Adam, worst error / bound (%s): p %.3f  m %.3f  v %.3f" % (family, worst["p"], worst["m"], worst["v"]))


def test_adam_case_families_are_what_the_builder_says():
    for step in (1, 10):
        p, g, m, v = R.adam_case(1025, step, "zero")
        assert (g == 0).all() and ((m == 0).all() and (v == 0).all()) == (step == 1) and (v >= 0).all()
        for fam, lo, hi in (("tiny20", 0.5e-20, 2e-20), ("tiny25", 0.5e-25, 2e-25), ("mixed", 1e-6, 1e3)):
            g = R.adam_case(1025, step, fam)[1]
            assert (np.abs(g) >= lo * 0.999).all() and (np.abs(g) <= hi * 1.001).all() and (g < 0).any() and (g > 0).any()
        assert (np.float32(R.adam_case(4, step, "tiny20")[1]) ** 2 < R.FLT_MIN).all()          # g * g underflows
        assert (np.float32(R.adam_case(4, step, "tiny25")[1]) ** 2 == 0).all()
    p, g, m, v = R.adam_case(1025, 10, "flip")
    assert (g * m <= 0).all() and (v > 0).all()
    g = R.adam_case(4096, 10, "mixed")[1]
    assert np.abs(g).min() < 1e-5 and np.abs(g).max() > 1e2


# ---- host-side checks of the two entry points: before any launch, so they run where the library loads without a GPU ----------------------
NCX_E_NULL, NCX_E_DIMS, NCX_E_WORKSPACE = -1, -2, -3


def test_loss_rank_and_adam_reject_bad_arguments_before_any_launch():
    from neuralcx import _lib
    L = _lib.lib()
    buf = (C.c_float * 64)()                       # host memory: never dereferenced, the calls return before they launch
    base = C.addressof(buf)
    a16 = (base + 15) // 16 * 16
    ptr = lambda off=0: C.c_void_p(a16 + off)
    lr = lambda B, K, rows, loss, rank, hits: L.ncx_loss_rank(ptr(), ptr(), B, K, C.c_float(0.0), rows, loss, None, rank, hits, None)
    assert lr(4, 0, ptr(), None, None, None) == NCX_E_DIMS
    assert lr(4, 65, ptr(), None, None, None) == NCX_E_DIMS
    assert lr(0, 24, ptr(), None, None, None) == NCX_E_DIMS
    assert lr(4, 24, None, ptr(), None, None) == NCX_E_NULL          # loss without loss_rows
    assert lr(4, 24, None, None, None, ptr()) == NCX_E_NULL          # hits without rank
    adam = lambda p, g, m, v, n, step: L.ncx_adam_step(p, g, m, v, C.c_size_t(n), C.c_float(1e-4), C.c_float(0.9), C.c_float(0.999),
                                                       C.c_float(1e-8), step, C.c_float(1.0), None)
    assert adam(ptr(), ptr(), ptr(), ptr(), 4, 0) == NCX_E_DIMS      # step = 0
    assert adam(ptr(), ptr(), ptr(), ptr(), 0, 1) == NCX_E_DIMS      # n = 0
    for bad in range(4):                                             # any one pointer 4 bytes off 16-byte alignment
        args = [ptr(4) if i == bad else ptr() for i in range(4)]
        assert adam(*args, 4, 1) == NCX_E_WORKSPACE, bad
