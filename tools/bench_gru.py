"""The question encoder at the full-batch shape (B = 512 questions padded to T = 26, embedding 620, GRU 2400): ops.gru_encode against
the torch path it replaces (nn.Embedding + nn.GRU over all T steps + last-step selection, no_grad, eval mode) in the same process.
Three length distributions:
  (a) all26    every question 26 words: equal work on both paths
  (b) uniform  lengths uniform on 3..26 (what the tests use)
  (c) vqa      VQA-like: len = 3 + Poisson(3) clipped to 3..26 -- mean ~ 6, the mass on 4..8, a thin tail (VQA v1 questions average
               a little over 6 words)
HIP events around --steps calls after --warmup calls; --repeats windows per path, the two paths alternating; reported: the median
window and the spread (max - min) / median of each path.  Prints one JSON line; --out writes it.
--x6: three paths alternate window by window, the fp32 step kernel (x6=False: the yardstick), the bf16 x 6 step kernel (x6=True,
NCX_F_X6: the x6_* fields) and torch."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neuralcx import ops  # noqa: E402
from vqa.models.seq2vec import GRUEncoder  # noqa: E402

PEAK_FP32_MFMA = 157.3e12      # MI355X matrix fp32, FLOP/s


def lengths(kind, B, T, rng):
    if kind == "all26":
        return np.full(B, T)
    if kind == "uniform":
        return rng.integers(3, T + 1, size=B)
    return np.clip(3 + rng.poisson(3.0, size=B), 3, T)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--steps-only", type=int, default=0, help="N calls of the HIP path on (b) and nothing else (for a kernel trace); "
                    "with --x6: N calls of each form on (a), where every step has n_t = B rows")
    ap.add_argument("--x6", action="store_true", help="time the bf16 x 6 step kernel beside the fp32 one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_gru.py needs the MI355X"
    B, T, de, dq, V = a.batch, 26, 620, 2400, 10000
    torch.manual_seed(1)
    enc = GRUEncoder(["w"] * V, dim_q=dq, dim_emb=de, dropout=0.25).cuda().eval()
    gw = ops.gru_weights(enc)
    rng = np.random.default_rng(0)
    flop_token = 2.0 * 3 * dq * (de + dq)                      # 43.5 MFLOP

    def make(kind):
        lens = lengths(kind, B, T, rng)
        w = np.zeros((B, T), np.int64)
        for b, n in enumerate(lens):
            w[b, :n] = rng.integers(1, V + 1, size=n)
        return torch.from_numpy(w).cuda(), lens

    if a.steps_only:
        w, _ = make("all26" if a.x6 else "uniform")
        for x6 in ((False, True) if a.x6 else (None,)):
            for _ in range(a.steps_only):
                ops.gru_encode(w, gw, x6=x6)
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

    res = dict(metric="gru_encoder_ms", shape=dict(B=B, T=T, dim_emb=de, dim_q=dq), steps=a.steps, warmup=a.warmup, repeats=a.repeats,
               mflop_per_valid_token=flop_token / 1e6, device=torch.cuda.get_device_name(0), cases={})
    for kind in ("all26", "uniform", "vqa"):
        w, lens = make(kind)

        def hip_step():
            return ops.gru_encode(w, gw, x6=False if a.x6 else None)

        def x6_step():
            return ops.gru_encode(w, gw, x6=True)

        @torch.no_grad()
        def torch_step():       # the path GRUEncoder.forward takes with use_hip off
            out, _ = enc.gru(enc.embedding(w))
            last = (w > 0).sum(1).clamp(min=1) - 1
            return out[torch.arange(B, device=w.device), last]

        t_hip, t_x6, t_torch = [], [], []
        for _ in range(a.repeats):
            t_hip.append(window(hip_step))
            if a.x6:
                t_x6.append(window(x6_step))
            t_torch.append(window(torch_step))
        err = float((hip_step() - torch_step()).abs().max())
        ops.check_gru_ids(device=w.device)
        mh, mt = float(np.median(t_hip)), float(np.median(t_torch))
        tokens = int(lens.sum())
        flops = tokens * flop_token
        res["cases"][kind] = dict(valid_tokens=tokens, padded_tokens=B * T, mean_len=float(lens.mean()), hip_ms=mh, hip_ms_windows=t_hip,
                                  hip_spread=(max(t_hip) - min(t_hip)) / mh, torch_ms=mt, torch_ms_windows=t_torch,
                                  torch_spread=(max(t_torch) - min(t_torch)) / mt, speedup_vs_torch=mt / mh, valid_gflop=flops / 1e9,
                                  hip_tflops_valid=flops / mh / 1e9, fraction_of_fp32_mfma_peak=flops / (mh * 1e-3) / PEAK_FP32_MFMA,
                                  torch_tflops_padded=B * T * flop_token / mt / 1e9, max_abs_diff_vs_torch=err)
        if a.x6:
            m6 = float(np.median(t_x6))
            res["cases"][kind].update(x6_ms=m6, x6_ms_windows=t_x6, x6_spread=(max(t_x6) - min(t_x6)) / m6, x6_speedup_vs_fp32=mh / m6,
                                      x6_tflops_valid=flops / m6 / 1e9, max_abs_diff_x6_vs_fp32=float((x6_step() - hip_step()).abs().max()))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
