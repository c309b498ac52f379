"""GPU: the answer-embedding gradient over permuted rows (row tiles without an answer of the batch skip the dGgt^T segment) against
the full form of the same product, bit for bit, and against the oracle.

dE[a] = dGt^T[a] . W1ak + dGgt^T[a] . W1agt, and dGgt^T[a] is non-zero only for the answers a that occur in the batch's answer_aids.  The
one-call backward (and phase 1) runs the product over rows permuted so that those answers come first (present ids ascending, then absent ids
ascending: a stable partition by presence) and stops the row tiles behind them after the first segment.  The products left out are exact
zeros added to accumulators that are never -0, so every gradient must keep its bits: each case runs the backward with the experiment hook
NCX_NO_DE_SKIP (the full form) and without it, on NaN-filled workspaces and gradients, and compares with torch.equal.  The shapes are the
smallest at which the row map can go wrong (one answer, the last row present, duplicates, everything present, the long / short boundary
inside a row tile) plus one at the flagship's A x da, the only size that takes the 64 x 64 tile form at three workgroups per CU.
"""
import numpy as np
import pytest
import torch

from oracle import ncx_oracle as orc
from helpers import FIELD, dev, grad_tol, random_case_f32, to_dev_batch, to_dev_params

pytestmark = pytest.mark.gpu


def _distinct(A, n, B, seed):
    """B answer ids with exactly n distinct values out of A (seeded): the n values once each, then repeats of them."""
    rng = np.random.default_rng(seed)
    ids = rng.permutation(A)[:n]
    return np.concatenate([ids, rng.choice(ids, size=B - n)])


# id: (B, A, H, da, K, answer_aids)
CASES = {
    "single-answer-last-row": (1, 5, 20, 12, 3, np.array([4])),
    "all-equal-to-0": (7, 64, 20, 12, 24, np.zeros(7, np.int64)),
    "duplicates-last-row-present": (7, 65, 64, 68, 3, np.array([64, 0, 64, 3, 3, 64, 0])),
    "every-answer-present": (70, 64, 20, 68, 24, np.concatenate([np.arange(64)[::-1], np.arange(6)])),
    "boundary-inside-a-row-tile": (40, 130, 64, 68, 24, _distinct(130, 33, 40, 5)),
    "flagship-tile-form": (64, 2000, 256, 2400, 3, _distinct(2000, 50, 64, 6)),
}
_INPUTS = {}     # per case: dims, parameters, batch and the oracle's gradients, built once


def _inputs(name):
    if name not in _INPUTS:
        B, A, H, da, K, aids = CASES[name]
        assert len(aids) == B and 0 <= aids.min() and aids.max() < A
        d = orc.Dims(K=K, dv=16, dq=8, dz=8, da=da, A=A, H=H, L=1)
        params = orc.init_params(d, seed=21, gain=3.0)
        batch = random_case_f32(100 + B + A, B, d)
        batch["answer_aids"] = torch.from_numpy(np.asarray(aids, np.int64))
        _INPUTS[name] = (d, params, batch, orc.loss_and_grads(params, d, batch)[2])
    return _INPUTS[name]


def _poisoned_workspace(dims):
    from neuralcx import ops
    ws = ops.alloc_workspace(dims, dev())
    ws[: ws.numel() // 4 * 4].view(torch.float32).fill_(float("nan"))
    return ws


def _backward(d, params, batch, phases=(0,)):
    """forward, loss and the backward (in the given phases) on a NaN-filled workspace; returns dims, workspace, gradients and the call's pieces."""
    from neuralcx import ops
    b, p = to_dev_batch(batch), to_dev_params(params)
    dims = ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A)
    ws = _poisoned_workspace(dims)
    scores = ops.forward(dims, b, p, ws)
    lr = ops.ranking_loss(scores, batch["gt"].to(dev()).to(torch.int32))
    g = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    for ph in phases:
        ops.backward(dims, b, p, ws, lr["dscores"], g, phase=ph)
    torch.cuda.synchronize()
    return dims, ws, g, (b, p, lr)


def _both_forms(name, monkeypatch):
    d, params, batch, g_ref = _inputs(name)
    monkeypatch.setenv("NCX_EXPERIMENT", "1")
    monkeypatch.setenv("NCX_NO_DE_SKIP", "1")
    full = _backward(d, params, batch)
    monkeypatch.delenv("NCX_NO_DE_SKIP")
    monkeypatch.delenv("NCX_EXPERIMENT")
    skip = _backward(d, params, batch)
    return d, params, batch, g_ref, full, skip


def _expected_perm(aids, A):
    """The rule, restated: a stable partition of 0 .. A-1 by presence in the batch (present ids ascending, then absent ids ascending)."""
    present = np.zeros(A, bool)
    present[np.asarray(aids)] = True
    ids = np.arange(A)
    return np.concatenate([ids[present], ids[~present]]), int(present.sum())


@pytest.mark.parametrize("name", list(CASES))
def test_skip_form_is_bit_identical_to_the_full_form_and_matches_the_oracle(name, monkeypatch):
    from neuralcx import ops
    d, params, batch, g_ref, (dims_f, ws_f, g_full, _), (dims_s, ws_s, g_skip, _) = _both_forms(name, monkeypatch)
    assert ops.ws_de_perm_view(dims_s, ws_s).numel() == d.A + 1              # the permuted form is what ran without the hook
    for k in g_full:
        assert torch.isfinite(g_skip[k]).all() and torch.equal(g_full[k], g_skip[k]), k
    ref = g_ref["answer_embedding.weight"].numpy()
    err = np.abs(g_skip[FIELD["answer_embedding.weight"]].cpu().numpy() - ref).max()
    assert err <= grad_tol("answer_embedding.weight", ref), (err, grad_tol("answer_embedding.weight", ref))
    # the device's presence map against the rule
    perm, n_present = _expected_perm(batch["answer_aids"].numpy(), d.A)
    got = ops.ws_de_perm_view(dims_s, ws_s).cpu().numpy()
    assert got[d.A] == n_present and np.array_equal(got[: d.A], perm), (got, perm, n_present)


def test_hook_selects_the_full_form(monkeypatch):
    """Under the hook the planner reports no permutation region (size 0) and the backward leaves the region untouched."""
    from neuralcx import ops
    d, params, batch, _ = _inputs("duplicates-last-row-present")
    monkeypatch.setenv("NCX_EXPERIMENT", "1")
    monkeypatch.setenv("NCX_NO_DE_SKIP", "1")
    dims, ws, g, _ = _backward(d, params, batch)
    assert ops.ws_de_perm_view(dims, ws).numel() == 0
    monkeypatch.delenv("NCX_NO_DE_SKIP")
    region = ops.ws_de_perm_view(dims, ws)
    assert region.numel() == d.A + 1 and torch.isnan(region.view(torch.float32)).all()            # still the NaN fill
    assert torch.isfinite(g["answer_embedding"]).all()


def test_phases_5_2_4_stay_bit_identical_to_the_one_call_backward():
    """Phases 5 | 2 | 4 keep the full form (a data-parallel job sums the dGt^T | dGgt^T block between them); the one-call backward runs the
    permuted form.  Every gradient equal, bit for bit -- and phases 1 | 2 (phase 1 runs the permuted form too)."""
    d, params, batch, _ = _inputs("boundary-inside-a-row-tile")
    g0 = _backward(d, params, batch)[2]
    g524 = _backward(d, params, batch, phases=(5, 2, 4))[2]
    g12 = _backward(d, params, batch, phases=(1, 2))[2]
    for k in g0:
        assert torch.equal(g0[k], g524[k]) and torch.equal(g0[k], g12[k]), k


def test_rows_of_absent_answers_are_the_first_segment_alone():
    """Rows of the gradient for answers that do not occur in the batch equal dGt^T . W1ak alone: the full-form product (phase 4) with the
    dGgt^T half of its operand block cleared -- the same kernel adding the same products -- gives those rows bit for bit, and in the
    rows of the answers that do occur the two differ."""
    from neuralcx import ops
    d, params, batch, _ = _inputs("boundary-inside-a-row-tile")
    dims, ws, g, (b, p, lr) = _backward(d, params, batch)
    blk = ops.ws_dgt_view(dims, ws)
    assert blk.numel() % 2 == 0
    blk[blk.numel() // 2:].zero_()
    g4 = {k: torch.full_like(v, float("nan")) for k, v in p.items()}
    ops.backward(dims, b, p, ws, lr["dscores"], g4, phase=4)
    torch.cuda.synchronize()
    present = torch.zeros(d.A, dtype=torch.bool)
    present[batch["answer_aids"]] = True
    dE, first = g["answer_embedding"].cpu(), g4["answer_embedding"].cpu()
    assert torch.isfinite(first).all() and torch.equal(dE[~present], first[~present])
    assert (dE[present] != first[present]).any(dim=1).all()
