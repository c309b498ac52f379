"""One training step of the MLBNoAtt VQA model at B = 512 and the real widths (dv 2048, dq 2400, dh 1200, A 2000, tanh x 3),
dropout 0.5 / 0.5 / 0.5, frozen encoder (q_emb resident): MlbTrainEngine.train_step (forward, cross-entropy, backward and Adam in HIP)
against the same step on the module's torch path (MLBNoAtt fusion + _classif + CrossEntropyLoss + torch.optim.Adam) in the same
process.  HIP events around --steps steps after --warmup steps; --repeats windows per path, the two paths alternating; reported: the
median window and the spread (max - min) / median of each path, and the HIP step's split by entry point (events around forward,
ncx_ce_loss, backward, ncx_adam_step; tools/kstats.sh gives the per-kernel trace).  The frozen encoder takes no d loss / d q_emb, so the
step's arithmetic is 18.3 GFLOP (21.1 with that product).  Prints one JSON line; --out writes it."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neuralcx import ops  # noqa: E402
from neuralcx.vqa_train import MlbTrainEngine  # noqa: E402
from vqa import models  # noqa: E402

PEAK_FP32_MFMA = 157.3e12      # MI355X matrix fp32, FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps-only", type=int, default=0, help="N HIP steps and nothing else (for a kernel trace)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mlb_train.py needs the MI355X"
    dev = "cuda:0"
    B, dv, dq, dh, A, n_img = a.batch, 2048, 2400, 1200, 2000, 8192
    opt = dict(arch="MLBNoAtt", seq2vec=dict(arch="gru", emb_size=16, dropout=0.0, fixed_emb=False),
               fusion=dict(dim_v=dv, dim_q=dq, dim_h=dh, activation_v="tanh", activation_q="tanh", dropout_v=0.5, dropout_q=0.5),
               classif=dict(activation="tanh", dropout=0.5))
    torch.manual_seed(1)
    model = models.factory(opt, ["w"] * 10, ["a%d" % i for i in range(A)], cuda=True).train()
    for p in model.seq2vec.parameters():
        p.requires_grad_(False)
    eng = MlbTrainEngine.from_options(opt, A, lr=1e-4, device=dev, seed=1)
    eng.load_state_dict(model.state_dict())
    feats = torch.randn(n_img, dv, device=dev).abs_() * 0.45
    idx = torch.randint(0, n_img, (B,), device=dev, dtype=torch.int32)
    q = torch.randn(B, dq, device=dev) * 0.3
    tgt = torch.randint(0, A, (B,), device=dev, dtype=torch.int32)
    tgt64, idx64 = tgt.long(), idx.long()
    optim = torch.optim.Adam([p for p in model.parameters() if p.requires_grad], 1e-4)
    crit = torch.nn.CrossEntropyLoss()

    def hip_step():
        return eng.train_step(feats, idx, q, tgt)

    def torch_step():
        loss = crit(model._classif(model._fusion(feats.index_select(0, idx64), q)), tgt64)
        optim.zero_grad()
        loss.backward()
        optim.step()
        return loss

    if a.steps_only:
        for _ in range(a.steps_only):
            hip_step()
        torch.cuda.synchronize()
        return

    def window(fn):
        for _ in range(a.warmup):
            fn()
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record()
        torch.cuda.synchronize()
        return e0.elapsed_time(e1) / a.steps

    t_hip, t_torch = [], []
    for _ in range(a.repeats):
        t_hip.append(window(hip_step))
        t_torch.append(window(torch_step))

    # the HIP step by entry point: events between the four calls train_step makes
    names = ("forward", "ce_loss", "backward", "adam")
    split = {n: [] for n in names}
    mw = eng.mlb_weights()
    for it in range(a.warmup + a.steps):
        ev = [torch.cuda.Event(enable_timing=True) for _ in range(5)]
        eng.step_count += 1
        d = eng._dims(feats, B, 1, eng.seed * 1000003 + eng.step_count, False)
        ev[0].record()
        logits, _ = ops.mlb_train_forward(d, feats, idx, q, mw, eng._ws); ev[1].record()
        r = ops.ce_loss(logits, tgt); ev[2].record()
        ops.mlb_train_backward(d, mw, eng._ws, r["dlogits"], eng.grads.views); ev[3].record()
        ops.adam_step(eng.params.flat, eng.grads.flat, eng.exp_avg, eng.exp_avg_sq, eng.step_count, lr=eng.lr); ev[4].record()
        torch.cuda.synchronize()
        if it >= a.warmup:
            for i, n in enumerate(names):
                split[n].append(ev[i].elapsed_time(ev[i + 1]))
    eng.check_targets()

    mh, mt = float(np.median(t_hip)), float(np.median(t_torch))
    sh, st = (max(t_hip) - min(t_hip)) / mh, (max(t_torch) - min(t_torch)) / mt
    flops = 2.0 * B * (dv * dh + dq * dh + dh * A) * 3 - 2.0 * B * (dv + dq) * dh       # forward + two products per layer backward, none for d feats / d q_emb
    res = dict(metric="mlb_train_step_ms", shape=dict(B=B, dv=dv, dq=dq, dh=dh, A=A), dropout=[0.5, 0.5, 0.5],
               steps=a.steps, warmup=a.warmup, repeats=a.repeats, device=torch.cuda.get_device_name(0),
               hip_ms=mh, hip_ms_windows=t_hip, hip_spread=sh, torch_ms=mt, torch_ms_windows=t_torch, torch_spread=st,
               speedup_vs_torch=mt / mh, bar="hip_ms <= torch_ms * (1 + max(spread))", bar_met=bool(mh <= mt * (1 + max(sh, st))),
               step_gflop=flops / 1e9, floor_ms=flops / PEAK_FP32_MFMA * 1e3, floor_with_dq_emb_ms=(flops + 2.0 * B * dh * dq) / PEAK_FP32_MFMA * 1e3,
               fraction_of_fp32_mfma_peak=flops / (mh * 1e-3) / PEAK_FP32_MFMA,
               hip_split_ms={n: float(np.median(v)) for n, v in split.items()})
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
