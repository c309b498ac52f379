"""Training the two-layer LSTM question encoder at the full-batch shape (B = 512 questions padded to T = 26, embedding 620, 2 x LSTM 1200):
the HIP forward + backward (ops.lstm_train_forward / lstm_train_backward, dE included) against what it replaces, torch's TwoLSTM
(tanh(nn.Embedding) + two nn.LSTMs over all T steps + last-step selection, use_hip_bptt = False) forward + backward under autograd, in
the same process.  Both without dropout (the torch module in train mode, which the device RNN backward insists on, with p = 0).  The
protocol and the three length distributions of tools/bench_gru_train.py:
  (a) all26    every question 26 words: equal work on both paths
  (b) uniform  lengths uniform on 3..26
  (c) vqa      VQA-like: len = 3 + Poisson(3) clipped to 3..26 -- mean ~ 6
HIP events around --steps calls after --warmup calls; --repeats windows per path, the two paths alternating; reported: the median
window and the spread (max - min) / median of each path.  The packs are built once (they belong to a weight set, not to a step); the
workspace is allocated once.  Prints one JSON line; --out writes it.
--x6: three paths alternate window by window, the forward on the fp32 step kernel (x6=False: the yardstick), on the bf16 x 6 step
kernel (x6=True, NCX_F_X6: the x6_* fields; the backward is the same code on either stash) and torch."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

from neuralcx import ops  # noqa: E402
from vqa.models.seq2vec import TwoLSTM  # noqa: E402

from bench_gru import PEAK_FP32_MFMA, lengths  # noqa: E402

WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--x6", action="store_true", help="time the forward on the bf16 x 6 step kernel beside the fp32 one")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_lstm_train.py needs the MI355X"
    B, T, emb, H, V = a.batch, 26, 620, 1200, 10000
    torch.manual_seed(1)
    enc = TwoLSTM(["w"] * V, emb, H).cuda().train()
    enc.p_drop = 0.0
    assert enc.use_hip_bptt is False
    params = [enc.embedding.weight] + [getattr(r, k) for r in (enc.rnn_0, enc.rnn_1) for k in WKEYS]
    lw = ops.lstm_train_weights(*params)
    ws = ops.lstm_train_workspace(B, T, lw, "cuda")
    rng = np.random.default_rng(0)
    fwd_token = 2.0 * 4 * H * (emb + H) + 2.0 * 4 * H * 2 * H  # 40.5 MFLOP forward; backward twice that (the data products and the weight gradients)
    flop_token = 3 * fwd_token                                 # 121.5 MFLOP
    dq_out = torch.randn(B, 2 * H, device="cuda")

    def make(kind):
        lens = lengths(kind, B, T, rng)
        w = np.zeros((B, T), np.int64)
        for b, n in enumerate(lens):
            w[b, :n] = rng.integers(1, V + 1, size=n)
        return torch.from_numpy(w).cuda(), lens

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

    res = dict(metric="lstm_train_ms", shape=dict(B=B, T=T, emb=emb, H=H), steps=a.steps, warmup=a.warmup, repeats=a.repeats,
               mflop_per_valid_token=flop_token / 1e6, workspace_bytes=ws.numel() - 256, device=torch.cuda.get_device_name(0), cases={})
    for kind in ("all26", "uniform", "vqa"):
        w, lens = make(kind)

        def hip_step():
            ops.lstm_train_forward(w, lw, ws, x6=False if a.x6 else None)
            return ops.lstm_train_backward(w, lw, ws, dq_out)

        def x6_step():
            ops.lstm_train_forward(w, lw, ws, x6=True)
            return ops.lstm_train_backward(w, lw, ws, dq_out)

        def torch_step():       # the path TwoLSTM.forward takes with use_hip_bptt off, and its backward
            return torch.autograd.grad(enc(w), params, dq_out)

        t_hip, t_x6, t_torch = [], [], []
        for _ in range(a.repeats):
            t_hip.append(window(hip_step))
            if a.x6:
                t_x6.append(window(x6_step))
            t_torch.append(window(torch_step))
        g, ref = hip_step(), torch_step()
        ops.check_gru_ids(device=w.device)
        err = {k: float((g[k] - r).abs().max() / r.abs().max()) for k, r in zip(("E",) + ops.LSTM_GRADS, ref)}
        mh, mt = float(np.median(t_hip)), float(np.median(t_torch))
        tokens = int(lens.sum())
        flops = tokens * flop_token
        res["cases"][kind] = dict(valid_tokens=tokens, padded_tokens=B * T, mean_len=float(lens.mean()), hip_ms=mh, hip_ms_windows=t_hip,
                                  hip_spread=(max(t_hip) - min(t_hip)) / mh, torch_ms=mt, torch_ms_windows=t_torch,
                                  torch_spread=(max(t_torch) - min(t_torch)) / mt, speedup_vs_torch=mt / mh,
                                  faster_by_more_than_the_spreads=bool(mt - mh > (max(t_hip) - min(t_hip)) + (max(t_torch) - min(t_torch))),
                                  valid_gflop=flops / 1e9, hip_tflops_valid=flops / mh / 1e9,
                                  fraction_of_fp32_mfma_peak=flops / (mh * 1e-3) / PEAK_FP32_MFMA, max_rel_diff_vs_torch=err)
        if a.x6:
            m6, g6 = float(np.median(t_x6)), x6_step()
            err6 = {k: float((g6[k] - r).abs().max() / r.abs().max()) for k, r in zip(("E",) + ops.LSTM_GRADS, ref)}
            res["cases"][kind].update(x6_ms=m6, x6_ms_windows=t_x6, x6_spread=(max(t_x6) - min(t_x6)) / m6, x6_speedup_vs_fp32=mh / m6,
                                      x6_speedup_vs_torch=mt / m6, x6_tflops_valid=flops / m6 / 1e9, x6_max_rel_diff_vs_torch=err6)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
