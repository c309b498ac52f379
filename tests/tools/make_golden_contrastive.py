"""Generate tests/golden/g12_contrastive.npz and g12_contrastive_adam.npz by RUNNING THE REFERENCE's ContrastiveModel
(vqa/models/cx.py:428-487), ContrastiveLoss and recallAtK (contrastive.py:293-309, 320-325) themselves, on CPU.

Uses oracle/make_golden.py's shims (imported, not changed) plus stub modules for what the reference's contrastive.py imports and is
absent or unimportable here (IPython.display, click, h5py, tqdm, tensorboard, vqa.lib.engine, vqa.datasets, train).  A stub VQA
model carries what the constructor reads; the model's `vqa_forward` is replaced by one that returns stored z_orig and z_knns.
The loss calls are the reference's own (contrastive.py:217-219: label ones for the counterexample, zeros for the other neighbour;
under the keepdim=True shim the distance is [B, 1] and broadcasts against the [B] label as on torch 0.3), the optimiser
torch.optim.Adam(model.parameters(), lr) (contrastive.py:170).  `get_scores` writes a [B, 1] distance into a [B] column, which a
current torch refuses: torch's own F.pairwise_distance is restored for that call (same values).

Cases
  t/   training triple, B = 8, P = 3, dv = 12, dz = 8, A = 6: inputs, initial state, h, both losses, both distance vectors, every
       gradient; g12_contrastive_adam.npz: the parameters after 1 and 3 Adam steps (lr 1e-3) on the same triple.
  e/   evaluation, B = 8, P = 25: inputs, h, the [B, 24] distances, the counterexample positions and recallAtK(k=5).
Every bias is negative and example 0's inputs are tiny, so all three of its hidden rows are exactly zero after the ReLU; the other
examples' inputs are scaled per example so that the hinge is active for some and inactive for others.
Asserted on the reference's own numbers (redrawn until they hold): no hidden pre-activation within 2e-5 of 0; no counterexample
distance within 1e-3 of the margin; hinge active (d < 2) for >= 1/4 of the examples and inactive for >= 1/4; example 0 all zero;
in e/ the gaps around ranks 1/2 and 5/6 of every row exceed 1e-3.
Usage:  python tests/tools/make_golden_contrastive.py
"""
import importlib
import os
import sys
import types

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)

import oracle.make_golden as mg  # noqa: E402  (the shims; puts the reference first on sys.path)
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402


def _stub(name, **kw):
    m = types.ModuleType(name)
    m.__dict__.update(kw)
    sys.modules[name] = m
    return m


for mod in ("h5py", "click", "tqdm"):
    try:
        importlib.import_module(mod)
    except ImportError:
        _stub(mod, tqdm=lambda x, **k: x)
_stub("tensorboard", SummaryWriter=object)
_stub("IPython"); _stub("IPython.display", Image=None, display=None)
import vqa  # noqa: E402  (the reference package)
import vqa.lib  # noqa: E402
sys.modules["vqa.lib.engine"] = _stub("vqa.lib.engine"); vqa.lib.engine = sys.modules["vqa.lib.engine"]
sys.modules["vqa.datasets"] = _stub("vqa.datasets"); vqa.datasets = sys.modules["vqa.datasets"]
_stub("train", load_checkpoint=lambda *a, **k: None)
import contrastive as ref_ct  # noqa: E402  (the reference script, imported as a module)
from vqa.models.cx import ContrastiveModel  # noqa: E402

assert ref_ct.__file__.startswith(mg.REF) and vqa.__file__.startswith(mg.REF), (ref_ct.__file__, vqa.__file__)

LR, MARGIN, TAU = 1e-3, 2.0, 2e-5


class _StubVQA(torch.nn.Module):
    def __init__(self, dv, dq, dz, A):
        super().__init__()
        self.opt = {"fusion": {"dim_v": dv, "dim_q": dq, "dim_mm": dz}}
        self.vocab_answers = ["a%d" % i for i in range(A)]


def _stub_forward(z_o, z_k):
    def f(image_features, question_wids):
        return (None, torch.from_numpy(z_o).requires_grad_(True), None, torch.from_numpy(z_k).requires_grad_(True), None)
    return f


def _pre(model, feats, z_o, z_k):
    """fp64 pre-activations [B, P, 300] of the reference's parameters (for the kink condition only)."""
    W, b = model.linear.weight.detach().double().numpy(), model.linear.bias.detach().double().numpy()
    x = np.concatenate([feats.astype(np.float64), np.concatenate([z_o[:, None], z_k], 1).astype(np.float64)], 2)
    return x @ W.T + b


def _scores(model, h):
    shim, F.pairwise_distance = F.pairwise_distance, mg._pd          # (see the module docstring)
    try:
        return model.get_scores(h[:, 0], h[:, 1:])
    finally:
        F.pairwise_distance = shim


def train_case(rng, model, B, dv, dz):
    for attempt in range(200):
        scale = rng.uniform(0.3, 6.0, B).astype(np.float32)
        scale[0] = 1e-3                                                     # example 0: every hidden row exactly zero
        feats = (rng.standard_normal((B, 3, dv)) * scale[:, None, None]).astype(np.float32)
        z_o = (rng.standard_normal((B, dz)) * scale[:, None]).astype(np.float32)
        z_k = (rng.standard_normal((B, 2, dz)) * scale[:, None, None]).astype(np.float32)
        model.vqa_forward = _stub_forward(z_o, z_k)
        model.knn_size = 2
        h = model(torch.from_numpy(feats), None, None)
        d = _scores(model, h.detach()).numpy()
        ok = np.abs(_pre(model, feats, z_o, z_k)).min() > TAU and np.abs(d[:, 0] - MARGIN).min() > 1e-3
        ok = ok and (d[:, 0] < MARGIN).sum() >= B // 4 and (d[:, 0] > MARGIN).sum() >= B // 4
        ok = ok and not h.detach().numpy()[0].any() and h.detach().numpy()[1:].any(axis=(1, 2)).all()
        if ok:
            return feats, z_o, z_k
    raise SystemExit("train_case: the conditions did not hold after 200 draws")


def eval_case(rng, model, B, dv, dz, K=24):
    for attempt in range(200):
        feats = (rng.standard_normal((B, K + 1, dv)) * 1.5).astype(np.float32)
        z_o = (rng.standard_normal((B, dz)) * 1.5).astype(np.float32)
        z_k = (rng.standard_normal((B, K, dz)) * 1.5).astype(np.float32)
        model.vqa_forward = _stub_forward(z_o, z_k)
        model.knn_size = K
        h = model(torch.from_numpy(feats), None, None).detach()
        d = _scores(model, h)
        s = np.sort(d.numpy(), 1)[:, ::-1]
        if np.abs(_pre(model, feats, z_o, z_k)).min() > TAU and (s[:, 0] - s[:, 1]).min() > 1e-3 and (s[:, 4] - s[:, 5]).min() > 1e-3:
            return feats, z_o, z_k, h.numpy(), d.numpy()
    raise SystemExit("eval_case: the conditions did not hold after 200 draws")


def main():
    torch.manual_seed(12)
    rng = np.random.default_rng(12)
    out, adam_out = {}, {}
    B, dv, dz, A = 8, 12, 8, 6
    model = ContrastiveModel(_StubVQA(dv, 4, dz, A), knn_size=2, trainable_vqa=False)
    with torch.no_grad():
        model.linear.bias.copy_(-model.linear.bias.abs() - 0.05)
    names = [n for n, _ in model.named_parameters()]
    assert names == ["answer_embedding.weight", "linear.weight", "linear.bias"], names
    out["init/names"] = np.array(names)
    for n, p in model.named_parameters():
        out["init/" + n] = p.detach().numpy().copy()

    # ---- evaluation case first (the initial parameters) ----
    comp = rng.integers(0, 24, B).astype(np.int64)
    e_feats, e_zo, e_zk, e_h, e_d = eval_case(rng, model, B, dv, dz)
    rec = ref_ct.recallAtK(torch.from_numpy(e_d), torch.from_numpy(comp), k=5)
    for n, v in (("feats", e_feats), ("z_orig", e_zo), ("z_knns", e_zk), ("h", e_h), ("dist", e_d), ("comp", comp.astype(np.int32)),
                 ("recall5", np.asarray(rec).astype(np.int32))):
        out["e/" + n] = v

    # ---- training triple ----
    feats, z_o, z_k = train_case(rng, model, B, dv, dz)
    for n, v in (("feats", feats), ("z_orig", z_o), ("z_knns", z_k)):
        out["t/" + n] = v
    crit = ref_ct.ContrastiveLoss()
    opt = torch.optim.Adam(model.parameters(), lr=LR)
    model.vqa_forward = _stub_forward(z_o, z_k)
    model.knn_size = 2
    for step in range(1, 4):
        h_out = model(torch.from_numpy(feats), None, None)
        loss_comp = crit(h_out[:, 0], h_out[:, 1], label=torch.ones([B]))            # contrastive.py:217-219
        loss_other = crit(h_out[:, 0], h_out[:, 2], label=torch.zeros([B]))
        loss = loss_comp + loss_other
        opt.zero_grad()
        loss.backward()
        if step == 1:
            d = _scores(model, h_out.detach()).numpy()
            out["t/h"] = h_out.detach().numpy().copy()
            out["t/loss_comp"], out["t/loss_other"] = np.float32(loss_comp.item()), np.float32(loss_other.item())
            out["t/dist_comp"], out["t/dist_other"] = d[:, 0].copy(), d[:, 1].copy()
            assert model.answer_embedding.weight.grad is None
            assert out["t/loss_comp"] > 0 and out["t/loss_other"] > 0
            for n in ("linear.weight", "linear.bias"):
                out["t/grad/" + n] = dict(model.named_parameters())[n].grad.numpy().copy()
        opt.step()
        if step in (1, 3):
            for n, p in model.named_parameters():
                adam_out["t/step%d/" % step + n] = p.detach().numpy().copy()
    assert np.array_equal(adam_out["t/step3/answer_embedding.weight"], out["init/answer_embedding.weight"])

    for name, d in (("g12_contrastive.npz", out), ("g12_contrastive_adam.npz", adam_out)):
        path = os.path.join(GOLDEN, name)
        np.savez_compressed(path, **d)
        print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
