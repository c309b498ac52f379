"""The two-layer LSTM question encoder at the full-batch shape (B = 512 questions padded to T = 26, embedding 620, 2 x LSTM 1200):
ops.lstm_encode against the torch path it replaces (the same TwoLSTM with use_hip = False: tanh(nn.Embedding) + two nn.LSTMs over all T
steps + last-step selection, no_grad, eval mode) in the same process.  Three length distributions:
  (a) all26    every question 26 words: equal work on both paths
  (b) uniform  lengths uniform on 3..26 (what the tests use)
  (c) vqa      VQA-like: len = 3 + Poisson(3) clipped to 3..26 -- mean ~ 6, the mass on 4..8, a thin tail
HIP events around --steps calls after --warmup calls; --repeats windows per path, the two paths alternating; reported: the median
window and the spread (max - min) / median of each path.  Also max |q - fp64| of both paths at the `real` test shape (B 40, lengths
3..26, weights x 3; the fp64 restatement is tests/lstm_ref.py).  Prints one JSON line; --out writes it.
--x6: three paths alternate window by window, the fp32 step kernel (x6=False: the yardstick), the bf16 x 6 step kernel (x6=True,
NCX_F_X6: the x6_* fields) and torch."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402
import torch  # noqa: E402

import lstm_ref  # noqa: E402
from neuralcx import ops  # noqa: E402
from vqa.models.seq2vec import TwoLSTM  # noqa: E402

PEAK_FP32_MFMA = 157.3e12      # MI355X matrix fp32, FLOP/s
KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def lengths(kind, B, T, rng):
    if kind == "all26":
        return np.full(B, T)
    if kind == "uniform":
        return rng.integers(3, T + 1, size=B)
    return np.clip(3 + rng.poisson(3.0, size=B), 3, T)


def make_wids(lens, T, V, rng):
    w = np.zeros((len(lens), T), np.int64)
    for b, n in enumerate(lens):
        w[b, :n] = rng.integers(1, V + 1, size=n)
    return w


def errors_vs_fp64(emb, H, T, V, x6=False):
    """max |q - fp64| of the HIP path (x6: of both its forms) and of torch's fp32 path on the device, B 40, lengths 3..26, nn.LSTM's init x 3"""
    torch.manual_seed(2)
    rng = np.random.default_rng(2)
    enc = TwoLSTM(["w"] * V, emb, H).eval()
    with torch.no_grad():
        enc.embedding.weight[0] = torch.randn(emb) * 0.5
        for p in list(enc.rnn_0.parameters()) + list(enc.rnn_1.parameters()):
            p.mul_(3.0)
    lens = rng.integers(3, T, size=40)
    lens[:24] = range(3, 27)
    wids = make_wids(lens, T, V, rng)
    ref = lstm_ref.lstm_encode(wids, enc.embedding.weight.detach().numpy(),
                               *[tuple(getattr(r, k).detach().numpy() for k in KEYS) for r in (enc.rnn_0, enc.rnn_1)])
    enc = enc.cuda()
    w = torch.from_numpy(wids).cuda()
    with torch.no_grad():
        enc.hip_x6 = False if x6 else None
        hip = enc(w).cpu().numpy()
        enc.hip_x6 = True
        hip6 = enc(w).cpu().numpy() if x6 else None
        enc.use_hip = False
        tor = enc(w).cpu().numpy()
    out = dict(B=40, hip_max_abs_err_vs_fp64=float(np.abs(hip - ref).max()), torch_fp32_max_abs_err_vs_fp64=float(np.abs(tor - ref).max()))
    if x6:
        out.update(x6_max_abs_err_vs_fp64=float(np.abs(hip6 - ref).max()))
    return out


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
    assert torch.cuda.is_available(), "bench_lstm.py needs the MI355X"
    B, T, emb, H, V = a.batch, 26, 620, 1200, 10000
    torch.manual_seed(1)
    enc = TwoLSTM(["w"] * V, emb, H).cuda().eval()
    ref_enc = TwoLSTM(["w"] * V, emb, H).cuda().eval()          # the same module with use_hip off
    ref_enc.load_state_dict(enc.state_dict())
    ref_enc.use_hip = False
    lw = ops.lstm_weights(enc)
    rng = np.random.default_rng(0)
    flop_token = 2.0 * 4 * H * (emb + H) + 2.0 * 4 * H * (H + H)    # 17.5 + 23.0 MFLOP

    if a.steps_only:
        w = torch.from_numpy(make_wids(lengths("all26" if a.x6 else "uniform", B, T, rng), T, V, rng)).cuda()
        for x6 in ((False, True) if a.x6 else (None,)):
            for _ in range(a.steps_only):
                ops.lstm_encode(w, lw, x6=x6)
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

    res = dict(metric="lstm2_encoder_ms", shape=dict(B=B, T=T, emb=emb, H=H), steps=a.steps, warmup=a.warmup, repeats=a.repeats,
               mflop_per_valid_token=flop_token / 1e6, packed_weight_mb=lw.packed.numel() * 4 / 1e6, device=torch.cuda.get_device_name(0), cases={})
    for kind in ("all26", "uniform", "vqa"):
        lens = lengths(kind, B, T, rng)
        w = torch.from_numpy(make_wids(lens, T, V, rng)).cuda()

        def hip_step():
            return ops.lstm_encode(w, lw, x6=False if a.x6 else None)

        def x6_step():
            return ops.lstm_encode(w, lw, x6=True)

        @torch.no_grad()
        def torch_step():
            return ref_enc(w)

        t_hip, t_x6, t_torch = [], [], []
        for _ in range(a.repeats):
            t_hip.append(window(hip_step))
            if a.x6:
                t_x6.append(window(x6_step))
            t_torch.append(window(torch_step))
        err = float((hip_step() - torch_step()).abs().max())
        ops.check_gru_ids(device=w.device)
        mh, mt = float(np.median(t_hip)), float(np.median(t_torch))
        sh, st = (max(t_hip) - min(t_hip)) / mh, (max(t_torch) - min(t_torch)) / mt
        tokens = int(lens.sum())
        flops = tokens * flop_token
        res["cases"][kind] = dict(valid_tokens=tokens, padded_tokens=B * T, mean_len=float(lens.mean()), hip_ms=mh, hip_ms_windows=t_hip,
                                  hip_spread=sh, torch_ms=mt, torch_ms_windows=t_torch, torch_spread=st, speedup_vs_torch=mt / mh,
                                  faster_by_more_than_the_spreads=bool((mt - mh) / mt > sh + st), valid_gflop=flops / 1e9,
                                  hip_tflops_valid=flops / mh / 1e9, fraction_of_fp32_mfma_peak=flops / (mh * 1e-3) / PEAK_FP32_MFMA,
                                  torch_tflops_padded=B * T * flop_token / mt / 1e9, max_abs_diff_vs_torch=err)
        if a.x6:
            m6 = float(np.median(t_x6))
            s6 = (max(t_x6) - min(t_x6)) / m6
            res["cases"][kind].update(x6_ms=m6, x6_ms_windows=t_x6, x6_spread=s6, x6_speedup_vs_fp32=mh / m6, x6_speedup_vs_torch=mt / m6,
                                      x6_faster_than_fp32_by_more_than_the_spreads=bool((mh - m6) / mh > sh + s6),
                                      x6_faster_than_torch_by_more_than_the_spreads=bool((mt - m6) / mt > st + s6),
                                      x6_tflops_valid=flops / m6 / 1e9, max_abs_diff_x6_vs_fp32=float((x6_step() - hip_step()).abs().max()))
    res["real_shape_errors"] = errors_vs_fp64(emb, H, T, 50, x6=a.x6)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
