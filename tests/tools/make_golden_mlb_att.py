"""Generate tests/golden/g21_mlb_att.npz by RUNNING THE REFERENCE's MLBAtt (vqa/models/att.py:11-192) on the CPU in eval mode.

Uses oracle/make_golden.py's shims (imported, not changed) and its stand-in question encoder.  The encoder is an input producer: its
output q_emb is stored, and the planted question is written into it before the model sees it.

Cases, at reduced widths (each: the table of NCHW maps [n_img, dv, W, H], img_idx [B], question ids, q_emb, the reference model's
state_dict, and the reference's logits [B, A] and attention maps [B, G, W H]):
  c0  every activation tanh: dv 64, dq 48, dh_att 32, G 2, dh_f 24, A 40, B 5, grid 5 x 7 (P = 35: not a multiple of 4, non-square)
  c1  attention.activation_mm and classif.activation absent: dv 96, dq 40, dh_att 44, G 3, dh_f 28, A 36, B 4, grid 7 x 7
Both with planted rows: table image 3 all zero (question 2's image: its attention is exactly uniform and v_att = 0), question 1
with q_emb x 300 (linear_q_att and linear_q_fusion saturate tanh), the same image for questions 0 and 3.

The attention must be PEAKED, or a wrong softmax or position order passes every tolerance (uniform attention is mean pooling):
conv_att.weight is scaled up (x 2 per try from gain 12; every other parameter has gain 3) until, in the fp64 restatement
tests/mlb_att_ref.py, some (b, g) has position logits spanning >= 8 and some map a maximum >= 0.3.

The fixture is data: inputs and the reference's outputs.  This script needs the reference checkout (build container only).
Usage:  python tests/tools/make_golden_mlb_att.py
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
import mlb_att_ref  # noqa: E402

assert ref_models.__file__.startswith(mg.REF), ref_models.__file__


class _Stored(torch.nn.Module):
    """Hands the stored (planted) q_emb to the model in place of the encoder that produced it."""

    def __init__(self, q):
        super().__init__()
        self.q = q

    def forward(self, wids):
        return self.q


def run_case(seed, dv, dq, dh_att, G, dh_f, A, B, W, H, act_mm, classif_act):
    mg._StandInSeq2Vec.hidden = dq
    vocab_words = ["w%d" % i for i in range(40)]
    vocab_answers = ["a%d" % i for i in range(A)]
    attention = dict(nb_glimpses=G, dim_h=dh_att, dropout_v=0.5, dropout_q=0.5, dropout_mm=0.5, activation_v="tanh", activation_q="tanh")
    if act_mm:
        attention["activation_mm"] = act_mm
    classif = dict(dropout=0.5)
    if classif_act:
        classif["activation"] = classif_act
    opt = dict(arch="MLBAtt", dim_v=dv, dim_q=dq,
               seq2vec=dict(arch="skipthoughts", dir_st="", type="BayesianUniSkip", dropout=0.25, fixed_emb=False),
               attention=attention, fusion=dict(dim_h=dh_f, dropout_v=0.5, dropout_q=0.5, activation_v="tanh", activation_q="tanh"),
               classif=classif)
    torch.manual_seed(seed)
    vqa = ref_models.factory(copy.deepcopy(opt), vocab_words, vocab_answers, cuda=False, data_parallel=False)
    assert type(vqa).__name__ == "MLBAtt"
    vqa.eval()
    rng = np.random.default_rng(seed)
    named = dict(vqa.named_parameters())
    with torch.no_grad():           # numpy-seeded weights (stable across torch builds)
        for name, p in named.items():
            if name.startswith("seq2vec."):
                continue
            fan_in = named[name.replace("bias", "weight")].shape[1]
            b = (12.0 if name.startswith("conv_att.") else 3.0) / np.sqrt(fan_in)
            p.copy_(torch.from_numpy(rng.uniform(-b, b, size=tuple(p.shape)).astype(np.float32)))

    n_img = B + 4
    table = (np.abs(rng.standard_normal((n_img, dv, W, H))) * 0.45).astype(np.float32)
    table[3] = 0.0
    img_idx = np.array([5, 1, 3, 5, 7, 0, 2, 4][:B], np.int32)          # image 5 twice, image 3 (zeros) for question 2; not the identity
    wids = np.zeros((B, 9), np.int64)
    for b in range(B):
        n = int(rng.integers(3, 9))
        wids[b, :n] = rng.integers(1, len(vocab_words) + 1, size=n)
    with torch.no_grad():
        q = vqa.seq2vec(torch.from_numpy(wids)).clone()
    q[1] *= 300.0
    vqa.seq2vec = _Stored(q)
    acts = dict(att_mm=act_mm, c=classif_act)
    dense = table[img_idx]
    for _ in range(12):             # scale conv_att.weight until the attention is peaked (fp64 restatement)
        state = {k: v.detach().numpy().copy() for k, v in vqa.state_dict().items() if not k.startswith("seq2vec.")}
        r_logits, r_att, r_pos = mlb_att_ref.mlb_att_forward(state, dense, q.numpy(), acts, want_logits=True)
        if mlb_att_ref.peaked(r_pos, r_att):
            break
        with torch.no_grad():
            vqa.conv_att.weight.mul_(2.0)
    else:
        raise AssertionError("attention not peaked")
    with torch.no_grad():
        logits = vqa(torch.from_numpy(dense), torch.from_numpy(wids))
    att = torch.stack(list(vqa.list_att), 1).numpy()                     # [B, G, P]
    assert att.shape == (B, G, W * H)
    out = dict(table=table, img_idx=img_idx, question_wids=wids.astype(np.int32), q_emb=q.numpy().copy(), logits=logits.numpy(), att=att,
               state_keys=np.array(sorted(state)), dims=np.array([dv, dq, dh_att, G, dh_f, A, B, W, H], np.int32),
               activation_mm=np.array(act_mm or ""), classif_activation=np.array(classif_act or ""))
    for k, v in state.items():
        out["state/" + k] = v
    for k in ("logits", "att"):
        assert out[k].dtype == np.float32 and np.isfinite(out[k]).all()
    assert np.array_equal(att[2], np.full_like(att[2], att[2, 0, 0])), "the all-zero image's attention is meant to be exactly uniform"
    xq = np.tanh(q.numpy().astype(np.float64) @ state["linear_q_att.weight"].astype(np.float64).T + state["linear_q_att.bias"])
    assert (np.abs(xq[1]) > 0.999).mean() > 0.5, "question 1 is meant to saturate linear_q_att"
    e_att = np.abs(att - r_att).max() / np.abs(r_att).max()
    e_log = np.abs(logits.numpy() - r_logits).max() / np.abs(r_logits).max()
    print("  reference fp32 against the fp64 restatement: att %.2e, logits %.2e (relative to max|ref|); position-logit range %.1f, "
          "max attention %.3f" % (e_att, e_log, (r_pos.max(2) - r_pos.min(2)).max(), r_att.max()))
    assert e_att < 1e-5 and e_log < 1e-5
    return out


def main():
    out = {}
    for name, kw in (("c0", dict(seed=210, dv=64, dq=48, dh_att=32, G=2, dh_f=24, A=40, B=5, W=5, H=7, act_mm="tanh", classif_act="tanh")),
                     ("c1", dict(seed=211, dv=96, dq=40, dh_att=44, G=3, dh_f=28, A=36, B=4, W=7, H=7, act_mm=None, classif_act=None))):
        case = run_case(**kw)
        for k, v in case.items():
            out[name + "/" + k] = v
        print(name, {k: case[k].shape for k in ("table", "img_idx", "q_emb", "logits", "att")}, "max|logits|", float(np.abs(case["logits"]).max()))
    path = os.path.join(GOLDEN, "g21_mlb_att.npz")
    np.savez_compressed(path, **out)
    print("written", path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
