"""Training-step timing of the trainable scorers (ncx_pairlin_* / ncx_linctx_*; reference vqa/models/cx.py:139-156,379-425):
forward + ncx_loss_rank + backward + Adam per step, as the CLI's run_epoch does, at B = 512, K = 24 and the default widths
(dv 2048, dq 2400, dz 360, 2000 answers).  The engines' train_step on synthetic device inputs; HIP events over `--steps` steps
after `--warmup`, best of `--repeats`.  Prints one JSON line."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import torch
from neuralcx import ops
from neuralcx.scorers import LinearContextEngine, PairwiseLinearEngine

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=512); ap.add_argument("--K", type=int, default=24)
ap.add_argument("--dv", type=int, default=2048); ap.add_argument("--dq", type=int, default=2400); ap.add_argument("--dz", type=int, default=360)
ap.add_argument("--A", type=int, default=2000); ap.add_argument("--n_img", type=int, default=20000)
ap.add_argument("--steps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10); ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
B, K = a.B, a.K
batch = ops.Batch(torch.randn(a.n_img, a.dv, generator=g, device=dev) * 0.45,
                  torch.randint(0, a.n_img, (B, K + 1), generator=g, device=dev, dtype=torch.int32),
                  torch.randn(B, a.dq, generator=g, device=dev) * 0.45, torch.randn(B, a.dz, generator=g, device=dev) * 0.45,
                  torch.randn(B, K, a.dz, generator=g, device=dev) * 0.45, None,
                  torch.randint(0, a.A, (B,), generator=g, device=dev, dtype=torch.int32))
gt = torch.randint(0, K, (B,), generator=g, device=dev, dtype=torch.int32)


def time_engine(e):
    e.init_parameters(seed=1)
    for _ in range(a.warmup):
        e.train_step(batch, gt)
    torch.cuda.synchronize()
    best = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            e.train_step(batch, gt)
        e1.record(); e1.synchronize()
        best.append(e0.elapsed_time(e1) / a.steps)
    e.check_ids()
    return min(best), best


pl_ms, pl_all = time_engine(PairwiseLinearEngine(K=K, dv=a.dv, dq=a.dq, dz=a.dz, A=a.A, device=dev))
lc_ms, lc_all = time_engine(LinearContextEngine(K=K, dz=a.dz, device=dev))
M, H = B * K, ops.PAIRLIN_H
flop_pl = 2.0 * 2 * M * H * (a.dv + a.dz) + 2.0 * 2 * B * H * (a.dv + a.dq + a.dz + H) + 2.0 * B * H * H
print(json.dumps({
    "metric": "training step (forward + loss + backward + Adam) of the trainable scorers", "B": B, "K": K,
    "dv": a.dv, "dq": a.dq, "dz": a.dz, "A": a.A,
    "pairlin_ms_per_step": round(pl_ms, 4), "pairlin_gflop_per_step": round(flop_pl / 1e9, 2),
    "pairlin_tflops": round(flop_pl / (pl_ms * 1e-3) / 1e12, 1), "pairlin_target_ms": 0.5,
    "linctx_ms_per_step": round(lc_ms, 4), "linctx_z_mb": round(B * K * a.dz * 4 / 1e6, 2),
    "pairlin_ms_all": [round(x, 4) for x in pl_all], "linctx_ms_all": [round(x, 4) for x in lc_all]}))
