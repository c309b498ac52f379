"""The MLB producer at the full-batch shape (frozen MLBNoAtt below the question encoder: B = 512 questions x 25 images from a feature
table, dv 2048, dq 2400, dh 1200, 2000 answers): ncx_mlb_forward against the same module's torch-op path in the same process.
HIP events around 50 steps after 10 warm-up steps, best of 3 windows, the two paths alternating.  Prints one JSON line; --out writes it.
--steps-only N: N steps of the HIP path and nothing else (the run a kernel trace is taken from)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import torch  # noqa: E402

import vqa.models as M  # noqa: E402
from neuralcx import ops  # noqa: E402

PEAK_FP32_MFMA = 157.3e12      # MI355X matrix fp32, FLOP/s


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=512)
    ap.add_argument("--n_img", type=int, default=82783)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mlb.py needs the MI355X"
    torch.manual_seed(1)
    dv, dq, dh, A, K1, B = 2048, 2400, 1200, 2000, 25, a.batch
    opt = dict(arch="MLBNoAtt", seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
               fusion=dict(dim_v=dv, dim_q=dq, dim_h=dh, dropout_v=0.5, dropout_q=0.5, activation_v="tanh", activation_q="tanh"),
               classif=dict(activation="tanh", dropout=0.5))
    vqa = M.factory(opt, ["w%d" % i for i in range(10)], ["a%d" % i for i in range(A)], cuda=True, data_parallel=False).eval()
    mw = ops.vqa_weights(vqa)
    feats = torch.randn(a.n_img, dv, device="cuda").abs() * 0.45
    idx = torch.randint(0, a.n_img, (B, K1), device="cuda", dtype=torch.int32)
    q = torch.randn(B, dq, device="cuda") * 0.3

    def hip_step():
        return ops.vqa_forward(feats, idx, q, mw, want_a_orig=False)

    @torch.no_grad()
    def torch_step():       # CXModelBase.vqa_forward's torch path below the encoder: dense gather, question rows repeated, fusion, classifier
        v = feats[idx.long().view(-1)]
        z = vqa._fusion(v, q.view(B, 1, dq).expand(B, K1, dq).reshape(B * K1, dq))
        return vqa._classif(z), z

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
    for _ in range(3):
        t_hip.append(window(hip_step))
        t_torch.append(window(torch_step))
    got, (a_ref, z_ref) = hip_step(), torch_step()
    err_z = float((got[3] - z_ref.view(B, K1, dh)[:, 1:]).abs().max())
    err_a = float((got[2] - a_ref.view(B, K1, A)[:, 1:]).abs().max())
    # algorithmic flops: x_v over B (K + 1) rows, x_q once per question, the classifier over the B K neighbour rows
    flops = 2.0 * B * K1 * dv * dh + 2.0 * B * dq * dh + 2.0 * B * (K1 - 1) * dh * A
    best = min(t_hip)
    res = dict(metric="mlb_producer_ms", shape=dict(B=B, K=K1 - 1, dv=dv, dq=dq, dh=dh, A=A, n_img=a.n_img), steps=a.steps, warmup=a.warmup,
               hip_ms=best, hip_ms_windows=t_hip, torch_ms=min(t_torch), torch_ms_windows=t_torch, speedup_vs_torch=min(t_torch) / best,
               algorithmic_gflop=flops / 1e9, hip_tflops=flops / best / 1e9, fraction_of_fp32_mfma_peak=flops / (best * 1e-3) / PEAK_FP32_MFMA,
               floor_ms_at_peak=flops / PEAK_FP32_MFMA * 1e3, max_abs_diff_vs_torch=dict(z_knns=err_z, a_knns=err_a), device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
