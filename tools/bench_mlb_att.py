"""The MLB attention model below the question encoder at full widths (dv 2048, dq 2400, attention dim_h 1200, fusion dim_h 1200, 2000
answers, 14 x 14 maps): ops.mlb_att_forward against the same module's torch path (use_hip = False) in the same process, at
B in {128, 512} and G in {4, 2}.  HIP events around --steps steps after --warmup warm-up steps, best of 3 windows, the two paths
alternating.  Prints one JSON line; --out writes it.
--x6: three paths instead of two, alternating window by window under the same protocol: the fp32 HIP forward (x6=False), the X6 HIP
forward (x6=True: NCX_F_X6 on the attention kernel) and the torch path; metric mlb_att_x6_forward_ms.
--steps-only N: N steps of the HIP path (the X6 form with --x6) at --batch / --glimpses and nothing else (the run a kernel trace is
taken from)."""
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
DV, DQ, DH_ATT, DH_F, A, GRID = 2048, 2400, 1200, 1200, 2000, 14


def build(G):
    opt = dict(arch="MLBAtt", dim_v=DV, dim_q=DQ, seq2vec=dict(arch="gru", emb_size=8, dropout=0.0),
               attention=dict(nb_glimpses=G, dim_h=DH_ATT, dropout_v=0.5, dropout_q=0.5, dropout_mm=0.5, activation_v="tanh",
                              activation_q="tanh", activation_mm="tanh"),
               fusion=dict(dim_h=DH_F, dropout_v=0.5, dropout_q=0.5, activation_v="tanh", activation_q="tanh"),
               classif=dict(activation="tanh", dropout=0.5))
    return M.factory(opt, ["w%d" % i for i in range(10)], ["a%d" % i for i in range(A)], cuda=True, data_parallel=False).eval()


def flops(B, G):
    P = GRID * GRID
    parts = dict(conv_v_att=2.0 * B * P * DV * DH_ATT, linear_q_att=2.0 * B * DQ * DH_ATT, conv_att=2.0 * B * P * DH_ATT * G,
                 pooling=2.0 * B * P * DV * G, glimpse_linears=2.0 * B * G * DV * DH_F, linear_q_fusion=2.0 * B * DQ * G * DH_F,
                 classifier=2.0 * B * G * DH_F * A)
    return sum(parts.values()), parts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--glimpses", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--x6", action="store_true", help="also time the X6 form of the attention kernel (three paths)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mlb_att.py needs the MI355X"
    torch.manual_seed(1)

    def paths(B, G):
        model = build(G)
        model.use_hip = False
        mw = ops.mlb_att_weights(model)
        v = torch.randn(B, DV, GRID, GRID, device="cuda").abs() * 0.45
        q = torch.randn(B, DQ, device="cuda") * 0.3

        def hip_step():
            return ops.mlb_att_forward(v, None, q, mw, x6=False) if a.x6 else ops.mlb_att_forward(v, None, q, mw)

        def x6_step():
            return ops.mlb_att_forward(v, None, q, mw, x6=True)

        @torch.no_grad()
        def torch_step():
            return model.forward_from_q(v, q), torch.stack(model.list_att, 1)

        return hip_step, torch_step, x6_step, mw

    if a.steps_only:
        hip_step, _, x6_step, _ = paths(a.batch, a.glimpses)
        for _ in range(a.steps_only):
            x6_step() if a.x6 else hip_step()
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

    cases = []
    for G in (4, 2):
        for B in (128, 512):
            hip_step, torch_step, x6_step, mw = paths(B, G)
            t_hip, t_torch, t_x6 = [], [], []
            for _ in range(3):
                t_hip.append(window(hip_step))
                if a.x6:
                    t_x6.append(window(x6_step))
                t_torch.append(window(torch_step))
            (l_h, a_h), (l_t, a_t) = hip_step(), torch_step()
            total, parts = flops(B, G)
            best, best_t = min(t_hip), min(t_torch)
            cases.append(dict(B=B, G=G, hip_ms=best, hip_ms_windows=t_hip, hip_spread=(max(t_hip) - best) / best,
                              torch_ms=best_t, torch_ms_windows=t_torch, torch_spread=(max(t_torch) - best_t) / best_t,
                              speedup_vs_torch=best_t / best, algorithmic_gflop=total / 1e9, conv_v_att_gflop=parts["conv_v_att"] / 1e9,
                              floor_ms_at_peak=total / PEAK_FP32_MFMA * 1e3, hip_tflops=total / best / 1e9,
                              fraction_of_fp32_mfma_peak=total / (best * 1e-3) / PEAK_FP32_MFMA,
                              max_abs_diff_vs_torch=dict(logits=float((l_h - l_t).abs().max()), att=float((a_h - a_t).abs().max()))))
            if a.x6:
                l_6, a_6 = x6_step()
                best6 = min(t_x6)
                win = best - best6 > max(max(t_hip) - best, max(t_x6) - best6)       # beats the fp32 form by more than the larger spread
                cases[-1].update(x6_ms=best6, x6_ms_windows=t_x6, x6_spread=(max(t_x6) - best6) / best6, x6_speedup_vs_fp32_hip=best / best6,
                                 x6_speedup_vs_torch=best_t / best6, x6_faster_than_fp32_hip_beyond_spreads=bool(win),
                                 x6_max_abs_diff_vs_fp32_hip=dict(logits=float((l_6 - l_h).abs().max()), att=float((a_6 - a_h).abs().max())),
                                 x6_logits_form=ops.mlb_att_logits_form(mw, B, GRID * GRID, B, x6=True))
            del hip_step, torch_step, x6_step, mw
            torch.cuda.empty_cache()
    res = dict(metric="mlb_att_x6_forward_ms" if a.x6 else "mlb_att_forward_ms", shape=dict(dv=DV, dq=DQ, dh_att=DH_ATT, dh_f=DH_F, A=A, grid=[GRID, GRID]), steps=a.steps,
               warmup=a.warmup, cases=cases, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
