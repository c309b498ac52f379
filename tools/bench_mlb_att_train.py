"""One training step of the MLB attention model below the question encoder at full widths (dv 2048, dq 2400, attention dim_h 1200,
fusion dim_h 1200, 2000 answers, 14 x 14 maps): forward + cross-entropy + backward through neuralcx.vqa_train.MlbAttTrainFunction
(the module with use_hip_train = True) against the same module's torch path under autograd, in the same process.  q_emb is given and
requires grad (d loss / d q_emb is computed on both sides); dropout runs at the YAML's p = 0.5 on both sides.  Runs: B = 128 and 512
with G = 4, B = 128 with G = 2.  HIP events around --steps steps after --warmup warm-up steps, best of 3 windows, the two paths
alternating.  Prints one JSON line; --out writes it.
--x6: four paths instead of two, alternating window by window: the HIP step with fp32 kernels (hip_x6 = False), the HIP step with
the X6 forward alone (NCX_F_X6 on the attention kernel, the backward's flag forced off), the HIP step with hip_x6 = True (the X6
forward and the X6 form of d conv_v_att.weight in the backward) and the torch path.
--steps-only N: N steps of the HIP path (hip_x6 = True with --x6) at --batch / --glimpses and nothing else (the run a kernel trace
is taken from)."""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import torch  # noqa: E402
import torch.nn.functional as F  # noqa: E402

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
    return M.factory(opt, ["w%d" % i for i in range(10)], ["a%d" % i for i in range(A)], cuda=True, data_parallel=False).train()


def flops(B, G):
    """Algorithmic FLOP of the step: the forward's products, and two products of the same size for each in the backward, except
    conv_v_att, whose input gradient is not taken (no gradient goes to the map)."""
    P = GRID * GRID
    fwd = dict(conv_v_att=2.0 * B * P * DV * DH_ATT, linear_q_att=2.0 * B * DQ * DH_ATT, conv_att=2.0 * B * P * DH_ATT * G,
               pooling=2.0 * B * P * DV * G, glimpse_linears=2.0 * B * G * DV * DH_F, linear_q_fusion=2.0 * B * DQ * G * DH_F,
               classifier=2.0 * B * G * DH_F * A)
    total = sum(fwd.values()) + fwd["conv_v_att"] + 2.0 * (sum(fwd.values()) - fwd["conv_v_att"]) - fwd["pooling"]
    return total, fwd


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--batch", type=int, default=128)
    ap.add_argument("--glimpses", type=int, default=4)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=10)
    ap.add_argument("--steps-only", type=int, default=0)
    ap.add_argument("--x6", action="store_true", help="also time the step with the X6 form of the attention kernel (three paths)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    assert torch.cuda.is_available(), "bench_mlb_att_train.py needs the MI355X"
    torch.manual_seed(1)

    def paths(B, G):
        model = build(G)
        v = torch.randn(B, DV, GRID, GRID, device="cuda").abs() * 0.45
        q = (torch.randn(B, DQ, device="cuda") * 0.3).requires_grad_(True)
        target = torch.randint(0, A, (B,), device="cuda")
        head = [p for n, p in model.named_parameters() if not n.startswith("seq2vec.")]

        def step(flag, x6=None, bwd_x6=None):
            model.use_hip_train = flag
            model.hip_x6 = x6
            force[0] = bwd_x6
            for p in head:
                p.grad = None
            q.grad = None
            loss = F.cross_entropy(model.forward_from_q(v, q), target)
            loss.backward()
            return loss

        return (lambda: step(True, False if a.x6 else None)), (lambda: step(False)), (lambda: step(True, True)), (lambda: step(True, True, False))

    force = [None]                 # the X6-forward-only column: the backward's x6 argument replaced by this when not None
    real_bwd = ops.mlb_att_train_backward
    ops.mlb_att_train_backward = lambda *ar, **kw: real_bwd(*ar, **(kw if force[0] is None else dict(kw, x6=force[0])))

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
    for B, G in ((128, 4), (512, 4), (128, 2)):
        hip_step, torch_step, x6_step, x6f_step = paths(B, G)
        t_hip, t_torch, t_x6, t_x6f = [], [], [], []
        for _ in range(3):
            t_hip.append(window(hip_step))
            if a.x6:
                t_x6f.append(window(x6f_step))
                t_x6.append(window(x6_step))
            t_torch.append(window(torch_step))
        torch.cuda.reset_peak_memory_stats()
        l_h = float(hip_step())
        mem_h = torch.cuda.max_memory_allocated()
        torch.cuda.reset_peak_memory_stats()
        l_t = float(torch_step())
        mem_t = torch.cuda.max_memory_allocated()
        total, fwd = flops(B, G)
        best, best_t = min(t_hip), min(t_torch)
        cases.append(dict(B=B, G=G, hip_ms=best, hip_ms_windows=t_hip, hip_spread=(max(t_hip) - best) / best,
                          torch_ms=best_t, torch_ms_windows=t_torch, torch_spread=(max(t_torch) - best_t) / best_t,
                          speedup_vs_torch=best_t / best, algorithmic_gflop=total / 1e9, dwv_att_gflop=fwd["conv_v_att"] / 1e9,
                          floor_ms_at_peak=total / PEAK_FP32_MFMA * 1e3, fraction_of_fp32_mfma_peak=total / (best * 1e-3) / PEAK_FP32_MFMA,
                          loss_hip=l_h, loss_torch=l_t, peak_memory_mb=dict(hip=mem_h / 2 ** 20, torch=mem_t / 2 ** 20)))
        if a.x6:
            best6, best6f = min(t_x6), min(t_x6f)

            def verdict(t_a, t_b):     # a against b: "win" / "loss" only beyond three times the larger spread of the two columns, else "level"
                d, sp = min(t_b) - min(t_a), 3.0 * max(max(t_a) - min(t_a), max(t_b) - min(t_b))
                return "win" if d > sp else "loss" if -d > sp else "level"

            win = best - best6 > max(max(t_hip) - best, max(t_x6) - best6)           # beats the fp32 step by more than the larger spread
            cases[-1].update(x6_ms=best6, x6_ms_windows=t_x6, x6_spread=(max(t_x6) - best6) / best6, x6_speedup_vs_fp32_hip=best / best6,
                             x6_speedup_vs_torch=best_t / best6, x6_faster_than_fp32_hip_beyond_spreads=bool(win), loss_x6=float(x6_step()),
                             x6_fwd_only_ms=best6f, x6_fwd_only_ms_windows=t_x6f, x6_fwd_only_spread=(max(t_x6f) - best6f) / best6f,
                             x6_bwd_vs_fp32_bwd=verdict(t_x6, t_x6f), x6_fwd_vs_fp32_fwd=verdict(t_x6f, t_hip),
                             x6_both_vs_fp32_hip=verdict(t_x6, t_hip), x6_both_vs_torch=verdict(t_x6, t_torch),
                             fp32_hip_vs_torch=verdict(t_hip, t_torch))
        del hip_step, torch_step, x6_step, x6f_step
        torch.cuda.empty_cache()
    res = dict(metric="mlb_att_x6_train_step_ms" if a.x6 else "mlb_att_train_step_ms", shape=dict(dv=DV, dq=DQ, dh_att=DH_ATT, dh_f=DH_F, A=A, grid=[GRID, GRID]), steps=a.steps,
               warmup=a.warmup, dropout_p=0.5, cases=cases, device=torch.cuda.get_device_name(0))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
