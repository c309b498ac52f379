"""Generate tests/golden/g22_mlb_att_train.npz by RUNNING THE REFERENCE's MLBAtt (vqa/models/att.py:11-192) on the CPU in TRAINING
mode with every dropout probability 0 (deterministic): forward, criterions.factory's loss (vqa/lib/criterions.py), loss.backward().

Uses oracle/make_golden.py's shims (imported, not changed) and a stored q_emb in place of the encoder, so that d loss / d q_emb is
the gradient of a leaf.  The two cases are g21's reduced shapes (tests/tools/make_golden_mlb_att.py), with its planted rows: table
image 3 all zero (question 2's image), question 1 with q_emb x 300 (saturating), the same image for questions 0 and 3, a
non-identity img_idx.  conv_att.weight is scaled up until the attention is PEAKED in the fp64 restatement (asserted).

Recorded per case: the table, img_idx, q_emb, target, the state_dict, logits, attention maps, loss, the reference's autograd gradient
of every parameter and of q_emb.  The fixture is data.  This script needs the reference checkout (build container only).
Usage:  python tests/tools/make_golden_mlb_att_train.py
"""
import copy
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
GOLDEN = os.path.join(ROOT, "tests", "golden")
sys.path.insert(0, ROOT)
sys.path.insert(1, os.path.join(ROOT, "tests"))

import oracle.make_golden as mg  # noqa: E402  (the shims; puts the reference first on sys.path)
import torch  # noqa: E402

import vqa.models as ref_models  # noqa: E402  (the reference package)
from vqa.lib import criterions  # noqa: E402
import mlb_att_ref  # noqa: E402

assert ref_models.__file__.startswith(mg.REF), ref_models.__file__


class _Stored(torch.nn.Module):
    def __init__(self, q):
        super().__init__()
        self.q = q

    def forward(self, wids):
        return self.q


def run_case(seed, dv, dq, dh_att, G, dh_f, A, B, W, H, act_mm, classif_act):
    mg._StandInSeq2Vec.hidden = dq
    vocab_words = ["w%d" % i for i in range(40)]
    vocab_answers = ["a%d" % i for i in range(A)]
    attention = dict(nb_glimpses=G, dim_h=dh_att, dropout_v=0.0, dropout_q=0.0, dropout_mm=0.0, activation_v="tanh", activation_q="tanh")
    if act_mm:
        attention["activation_mm"] = act_mm
    classif = dict(dropout=0.0)
    if classif_act:
        classif["activation"] = classif_act
    opt = dict(arch="MLBAtt", dim_v=dv, dim_q=dq,
               seq2vec=dict(arch="skipthoughts", dir_st="", type="BayesianUniSkip", dropout=0.25, fixed_emb=False),
               attention=attention, fusion=dict(dim_h=dh_f, dropout_v=0.0, dropout_q=0.0, activation_v="tanh", activation_q="tanh"),
               classif=classif)
    torch.manual_seed(seed)
    vqa = ref_models.factory(copy.deepcopy(opt), vocab_words, vocab_answers, cuda=False, data_parallel=False)
    assert type(vqa).__name__ == "MLBAtt"
    rng = np.random.default_rng(seed)
    named = {n: p for n, p in vqa.named_parameters() if not n.startswith("seq2vec.")}
    with torch.no_grad():           # numpy-seeded weights (stable across torch builds)
        for name, p in named.items():
            fan_in = named[name.replace("bias", "weight")].shape[1]
            b = (12.0 if name.startswith("conv_att.") else 3.0) / np.sqrt(fan_in)
            p.copy_(torch.from_numpy(rng.uniform(-b, b, size=tuple(p.shape)).astype(np.float32)))

    n_img = B + 4
    table = (np.abs(rng.standard_normal((n_img, dv, W, H))) * 0.45).astype(np.float32)
    table = (np.round(table * 1024.0) / 1024.0).astype(np.float32)     # a 2^-10 grid: exact in fp32, and the low mantissa bits compress
    table[3] = 0.0
    img_idx = np.array([5, 1, 3, 5, 7, 0, 2, 4][:B], np.int32)
    table[np.setdiff1d(np.arange(n_img), img_idx)] = 0.0                # rows no question reads: zeros compress, the file stays below g21's size
    target = rng.integers(0, A, size=B).astype(np.int64)
    q = (rng.standard_normal((B, dq)) * 0.3).astype(np.float32)
    q[1] *= 300.0
    acts = dict(att_mm=act_mm, c=classif_act)
    dense = table[img_idx]
    for _ in range(12):             # scale conv_att.weight until the attention is peaked (fp64 restatement)
        state = {k: v.detach().numpy().copy() for k, v in vqa.state_dict().items() if not k.startswith("seq2vec.")}
        r_logits, r_att, r_pos = mlb_att_ref.mlb_att_forward(state, dense, q, acts, want_logits=True)
        if mlb_att_ref.peaked(r_pos, r_att):
            break
        with torch.no_grad():
            vqa.conv_att.weight.mul_(2.0)
    else:
        raise AssertionError("attention not peaked")
    assert mlb_att_ref.peaked(r_pos, r_att)

    q_t = torch.from_numpy(q.copy()).requires_grad_(True)
    vqa.seq2vec = _Stored(q_t)
    vqa.train()
    criterion = criterions.factory({}, cuda=False)
    logits = vqa(torch.from_numpy(dense), torch.zeros(B, 4, dtype=torch.long))
    loss = criterion(logits, torch.from_numpy(target))
    att = torch.stack([a.detach() for a in vqa.list_att], 1).numpy()
    assert att.shape == (B, G, W * H)
    vqa.zero_grad()
    loss.backward()
    out = dict(table=table, img_idx=img_idx, q_emb=q, target=target.astype(np.int32), logits=logits.detach().numpy(), att=att,
               loss=np.float32(loss.item()), grad_q_emb=q_t.grad.numpy().copy(), state_keys=np.array(sorted(state)),
               dims=np.array([dv, dq, dh_att, G, dh_f, A, B, W, H], np.int32),
               activation_mm=np.array(act_mm or ""), classif_activation=np.array(classif_act or ""))
    for k, v in state.items():
        out["state/" + k] = v
        out["grad/" + k] = named[k].grad.detach().numpy().copy()
    assert all(np.isfinite(v).all() for v in out.values() if v.dtype.kind == "f")
    assert np.array_equal(att[2], np.full_like(att[2], att[2, 0, 0])), "the all-zero image's attention is meant to be exactly uniform"
    xq = np.tanh(q.astype(np.float64) @ state["linear_q_att.weight"].astype(np.float64).T + state["linear_q_att.bias"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5, "question 1 is meant to saturate linear_q_att"
    e_att = np.abs(att - r_att).max() / np.abs(r_att).max()
    e_log = np.abs(out["logits"] - r_logits).max() / np.abs(r_logits).max()
    print("  reference fp32 (training mode, p = 0) against the fp64 eval restatement: att %.2e, logits %.2e; position-logit range %.1f, "
          "max attention %.3f" % (e_att, e_log, (r_pos.max(2) - r_pos.min(2)).max(), r_att.max()))
    assert e_att < 1e-5 and e_log < 1e-5
    return out


def main():
    out = {}
    for name, kw in (("c0", dict(seed=220, dv=64, dq=48, dh_att=32, G=2, dh_f=24, A=40, B=5, W=5, H=7, act_mm="tanh", classif_act="tanh")),
                     ("c1", dict(seed=221, dv=96, dq=40, dh_att=44, G=3, dh_f=28, A=36, B=4, W=7, H=7, act_mm=None, classif_act=None))):
        case = run_case(**kw)
        for k, v in case.items():
            out[name + "/" + k] = v
        print(name, "loss", float(case["loss"]), "max|logits|", float(np.abs(case["logits"]).max()), "max|dq|", float(np.abs(case["grad_q_emb"]).max()),
              "max|d conv_att.bias|", float(np.abs(case["grad/conv_att.bias"]).max()))
    path = os.path.join(GOLDEN, "g22_mlb_att_train.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
