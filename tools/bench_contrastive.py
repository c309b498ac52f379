"""Timing of the contrastive path (ncx_contrastive_*; reference contrastive.py, vqa/models/cx.py:428-487) against the same steps
written with torch ops, in one process, at B = 512 and the default widths (dv 2048, dz 360):
  training step   P = 3: forward + both ContrastiveLoss terms + backward + Adam     (ContrastiveEngine.train_step)
  evaluation step P = 25: forward + distances + rank / Recall                        (ContrastiveEngine.eval_step)
Yardstick: index_select gather, cat, F.linear, relu, F.pairwise_distance, autograd, torch.optim.Adam; for the evaluation the
distances' topk(5) hit count (recallAtK, contrastive.py:320-325), on the device.  Both sides take the same resident feature
table, ids and z; neither syncs the host inside a step.  HIP events over `--steps` steps after `--warmup`, best of `--repeats`.
Launches per step are counted with torch.profiler (kernels + memcpys on the device, one step).  Prints one JSON line."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import torch
import torch.nn.functional as F
from neuralcx import ops
from neuralcx.contrastive import ContrastiveEngine

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=512); ap.add_argument("--K", type=int, default=24)
ap.add_argument("--dv", type=int, default=2048); ap.add_argument("--dz", type=int, default=360)
ap.add_argument("--A", type=int, default=2000); ap.add_argument("--n_img", type=int, default=82783)
ap.add_argument("--steps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10); ap.add_argument("--repeats", type=int, default=3)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
B, K = a.B, a.K
feats = torch.randn(a.n_img, a.dv, generator=g, device=dev).abs_() * 0.45


def make_batch(P):
    return ops.Batch(feats, torch.randint(0, a.n_img, (B, P), generator=g, device=dev, dtype=torch.int32), None,
                     torch.randn(B, a.dz, generator=g, device=dev), torch.randn(B, P - 1, a.dz, generator=g, device=dev), None)


b3, b25 = make_batch(3), make_batch(K + 1)
gt = torch.randint(0, K, (B,), generator=g, device=dev, dtype=torch.int32)
eng = ContrastiveEngine(dv=a.dv, dz=a.dz, A=a.A, device=dev)
eng.init_parameters(seed=1)

# ---- the yardstick: the same two steps with torch ops ----
lin = torch.nn.Linear(a.dv + a.dz, ops.CONTRASTIVE_H).to(dev)
with torch.no_grad():
    lin.weight.copy_(eng.params.views["linear.weight"]); lin.bias.copy_(eng.params.views["linear.bias"])
opt = torch.optim.Adam(lin.parameters(), lr=1e-4)


def torch_hidden(b):
    Bq, P = b.img_idx.shape
    v = feats.index_select(0, b.img_idx.reshape(-1).long()).view(Bq, P, -1)
    z = torch.cat([b.z_orig[:, None], b.z_knns], 1)
    return F.relu(F.linear(torch.cat([v, z], 2), lin.weight, lin.bias))


def torch_train():
    h = torch_hidden(b3)
    d1, d2 = F.pairwise_distance(h[:, 0], h[:, 1]), F.pairwise_distance(h[:, 0], h[:, 2])
    loss = torch.clamp(2.0 - d1, min=0.0).pow(2).mean() + d2.pow(2).mean()
    opt.zero_grad(set_to_none=True)
    loss.backward()
    opt.step()
    return loss


def torch_eval():
    with torch.no_grad():
        h = torch_hidden(b25)
        d = F.pairwise_distance(h[:, :1].expand(-1, K, -1).reshape(B * K, -1), h[:, 1:].reshape(B * K, -1)).view(B, K)
        return (d.topk(5).indices == gt.long()[:, None]).sum()


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    runs = []
    for _ in range(a.repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(a.steps):
            fn()
        e1.record(); e1.synchronize()
        runs.append(e0.elapsed_time(e1) / a.steps)
    return min(runs), runs


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    names = [e.name for e in prof.events() if str(e.device_type).endswith("CUDA")]
    return len(names), sorted(set(names))


res = {"metric": "contrastive path: HIP step vs the same step with torch ops", "B": B, "K": K, "dv": a.dv, "dz": a.dz, "n_img": a.n_img,
       "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats}
for name, hip_fn, torch_fn, flop in (
        ("train", lambda: eng.train_step(b3), torch_train, 2.0 * 2 * 3 * B * ops.CONTRASTIVE_H * (a.dv + a.dz)),
        ("eval", lambda: eng.eval_step(b25, gt), torch_eval, 2.0 * (K + 1) * B * ops.CONTRASTIVE_H * (a.dv + a.dz))):
    hip_ms, hip_all = timed(hip_fn)
    t_ms, t_all = timed(torch_fn)
    n_hip, k_hip = launches(hip_fn)
    n_t, _ = launches(torch_fn)
    res.update({name + "_hip_ms": round(hip_ms, 4), name + "_torch_ms": round(t_ms, 4), name + "_speedup": round(t_ms / hip_ms, 2),
                name + "_gflop": round(flop / 1e9, 2), name + "_hip_tflops": round(flop / (hip_ms * 1e-3) / 1e12, 1),
                name + "_hip_launches": n_hip, name + "_torch_launches": n_t, name + "_hip_kernels": k_hip,
                name + "_hip_ms_all": [round(x, 4) for x in hip_all], name + "_torch_ms_all": [round(x, 4) for x in t_all]})
eng.check_ids()
print(json.dumps(res))
