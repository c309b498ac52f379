"""Training the question encoder at the full-batch shape (B = 512 questions padded to T = 26, embedding 620, GRU 2400): the HIP forward +
backward (ops.gru_train_forward / gru_train_backward, dE included) against what it replaces, torch's nn.Embedding + nn.GRU over all T
steps + last-step selection, forward + backward under autograd (train mode, no dropout), in the same process.  The protocol and the
three length distributions of tools/bench_gru.py:
  (a) all26    every question 26 words: equal work on both paths
  (b) uniform  lengths uniform on 3..26
  (c) vqa      VQA-like: len = 3 + Poisson(3) clipped to 3..26 -- mean ~ 6
HIP events around --steps calls after --warmup calls; --repeats windows per path, the two paths alternating; reported: the median
window and the spread (max - min) / median of each path.  The packs are built once (they belong to a weight set, not to a step); the
workspace is allocated once.  Prints one JSON line; --out writes it.
--x6: three paths alternate window by window, the forward on the fp32 step kernel (x6=False: the yardstick), on the bf16 x 6 step
kernel (x6=True, NCX_F_X6: the x6_* fields; the backward is the fp32 one on either stash) and torch.
--x6_bwd (implies --x6): a fourth path in the same alternation, X6 forward + X6 backward (ops.gru_train_backward x6=True: the x6b_* fields;
x6b_speedup_vs_x6 compares it with X6 forward + fp32 backward of the same run).
--steps-only N --path {fp32,x6fwd,x6}: N steps of that one path on the --kind length set and nothing else (the run a kernel trace wraps)."""
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

from bench_gru import PEAK_FP32_MFMA, lengths  # noqa: E402

WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--x6", action="store_true", help="time the forward on the bf16 x 6 step kernel beside the fp32 one")
    ap.add_argument("--x6_bwd", action="store_true", help="also time X6 forward + X6 backward (NCX_F_X6 on ncx_gru_train_backward_flags)")
    ap.add_argument("--steps-only", type=int, default=0, help="run this many steps of --path on --kind and exit (for a kernel trace)")
    ap.add_argument("--path", default="x6", choices=("fp32", "x6fwd", "x6"))
    ap.add_argument("--kind", default="all26", choices=("all26", "uniform", "vqa"))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    a.x6 = a.x6 or a.x6_bwd
    assert torch.cuda.is_available(), "bench_gru_train.py needs the MI355X"
    B, T, de, dq, V = a.batch, 26, 620, 2400, 10000
    torch.manual_seed(1)
    enc = GRUEncoder(["w"] * V, dim_q=dq, dim_emb=de, dropout=0.0).cuda().train()
    params = [enc.embedding.weight] + [getattr(enc.gru, k) for k in WKEYS]
    gw = ops.gru_train_weights(*params)
    ws = ops.gru_train_workspace(B, T, gw, "cuda")
    rng = np.random.default_rng(0)
    flop_token = 3 * 2.0 * 3 * dq * (de + dq)                  # forward + the two backward products of every weight: 130.5 MFLOP
    dq_out = torch.randn(B, dq, device="cuda")

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

    if a.steps_only:
        w, _ = make(a.kind)
        for _ in range(a.steps_only):
            ops.gru_train_forward(w, gw, ws, x6=a.path != "fp32")
            ops.gru_train_backward(w, gw, ws, dq_out, x6=a.path == "x6")
        torch.cuda.synchronize()
        ops.check_gru_ids(device=w.device)
        print(json.dumps(dict(steps_only=a.steps_only, path=a.path, kind=a.kind, bwd_form=ops.gru_bwd_form(de, dq, B, T, x6=a.path == "x6"))))
        return

    res = dict(metric="gru_train_ms", shape=dict(B=B, T=T, dim_emb=de, dim_q=dq), steps=a.steps, warmup=a.warmup, repeats=a.repeats,
               mflop_per_valid_token=flop_token / 1e6, workspace_bytes=ws.numel() - 256, device=torch.cuda.get_device_name(0), cases={})
    for kind in ("all26", "uniform", "vqa"):
        w, lens = make(kind)

        def hip_step():
            ops.gru_train_forward(w, gw, ws, x6=False if a.x6 else None)
            return ops.gru_train_backward(w, gw, ws, dq_out, x6=False if a.x6 else None)

        def x6_step():
            ops.gru_train_forward(w, gw, ws, x6=True)
            return ops.gru_train_backward(w, gw, ws, dq_out, x6=False)

        def x6b_step():
            ops.gru_train_forward(w, gw, ws, x6=True)
            return ops.gru_train_backward(w, gw, ws, dq_out, x6=True)

        def torch_step():       # the path GRUEncoder.forward takes with use_hip_train off, and its backward
            out, _ = enc.gru(enc.embedding(w))
            last = (w > 0).sum(1).clamp(min=1) - 1
            q = out[torch.arange(B, device=w.device), last]
            return torch.autograd.grad(q, params, dq_out)

        t_hip, t_x6, t_x6b, t_torch = [], [], [], []
        for _ in range(a.repeats):
            t_hip.append(window(hip_step))
            if a.x6:
                t_x6.append(window(x6_step))
            if a.x6_bwd:
                t_x6b.append(window(x6b_step))
            t_torch.append(window(torch_step))
        g, ref = hip_step(), torch_step()
        ops.check_gru_ids(device=w.device)
        err = {k: float((g[k] - r).abs().max() / r.abs().max()) for k, r in zip(("E", "w_ih", "w_hh", "b_ih", "b_hh"), ref)}
        mh, mt = float(np.median(t_hip)), float(np.median(t_torch))
        tokens = int(lens.sum())
        flops = tokens * flop_token
        res["cases"][kind] = dict(valid_tokens=tokens, padded_tokens=B * T, mean_len=float(lens.mean()), hip_ms=mh, hip_ms_windows=t_hip,
                                  hip_spread=(max(t_hip) - min(t_hip)) / mh, torch_ms=mt, torch_ms_windows=t_torch,
                                  torch_spread=(max(t_torch) - min(t_torch)) / mt, speedup_vs_torch=mt / mh, valid_gflop=flops / 1e9,
                                  hip_tflops_valid=flops / mh / 1e9, fraction_of_fp32_mfma_peak=flops / (mh * 1e-3) / PEAK_FP32_MFMA,
                                  max_rel_diff_vs_torch=err)
        if a.x6:
            m6, g6 = float(np.median(t_x6)), x6_step()
            err6 = {k: float((g6[k] - r).abs().max() / r.abs().max()) for k, r in zip(("E", "w_ih", "w_hh", "b_ih", "b_hh"), ref)}
            res["cases"][kind].update(x6_ms=m6, x6_ms_windows=t_x6, x6_spread=(max(t_x6) - min(t_x6)) / m6, x6_speedup_vs_fp32=mh / m6,
                                      x6_tflops_valid=flops / m6 / 1e9, x6_max_rel_diff_vs_torch=err6)
        if a.x6_bwd:
            m6b, g6b = float(np.median(t_x6b)), x6b_step()
            err6b = {k: float((g6b[k] - r).abs().max() / r.abs().max()) for k, r in zip(("E", "w_ih", "w_hh", "b_ih", "b_hh"), ref)}
            res["cases"][kind].update(x6b_ms=m6b, x6b_ms_windows=t_x6b, x6b_spread=(max(t_x6b) - min(t_x6b)) / m6b, x6b_speedup_vs_x6=m6 / m6b,
                                      x6b_speedup_vs_fp32=mh / m6b, x6b_tflops_valid=flops / m6b / 1e9, x6b_max_rel_diff_vs_torch=err6b,
                                      x6b_bwd_form=ops.gru_bwd_form(de, dq, B, T, x6=True))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
