"""Timing of the similarity scorer (ncx_similarity_scores; reference vqa/models/cx.py:496-518) against the same scores computed
with torch ops in the same process: B = 512 questions x 24 candidates at the real widths (dv 2048, dz 360, A 2000) on the
resident 82 783-row feature table.
Yardstick: index_select gather, F.cosine_similarity twice, F.cross_entropy(reduction='none'), two adds -- vectorised over the
candidates (the reference loops over them in Python, three ops each), on the device, no host sync inside a call.
A pool of distinct batches (ids, z, logits), larger together than the last-level cache, is cycled so that every launch streams
its inputs from HBM.  HIP events over `--steps` calls after `--warmup`, best of `--repeats`; the two sides alternate.
Bytes: the unique bytes a batch has to read (feature rows, logits, z) -- the floor of this pure-bandwidth pass.
Prints one JSON line; --out writes it to a file as well."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import torch
import torch.nn.functional as F
from neuralcx import ops

ap = argparse.ArgumentParser()
ap.add_argument("--B", type=int, default=512); ap.add_argument("--K", type=int, default=24)
ap.add_argument("--dv", type=int, default=2048); ap.add_argument("--dz", type=int, default=360)
ap.add_argument("--A", type=int, default=2000); ap.add_argument("--n_img", type=int, default=82783)
ap.add_argument("--pool", type=int, default=4, help="distinct batches cycled (4 x 117 MB of logits and z, plus their table rows)")
ap.add_argument("--steps", type=int, default=50); ap.add_argument("--warmup", type=int, default=10); ap.add_argument("--repeats", type=int, default=3)
ap.add_argument("--out", type=str, default=None)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
B, K = a.B, a.K
feats = torch.randn(a.n_img, a.dv, generator=g, device=dev).abs_() * 0.45
pool = []
for _ in range(a.pool):
    aids = torch.randint(0, a.A, (B,), generator=g, device=dev, dtype=torch.int32)
    pool.append(dict(idx=torch.randint(0, a.n_img, (B, K + 1), generator=g, device=dev, dtype=torch.int32),
                     z_o=torch.randn(B, a.dz, generator=g, device=dev), z_k=torch.randn(B, K, a.dz, generator=g, device=dev),
                     a_k=torch.randn(B, K, a.A, generator=g, device=dev) * 2.0, aids=aids,
                     aids_rep=aids.long().repeat_interleave(K)))
flag = torch.zeros(1, dtype=torch.int32, device=dev)
step = [0]


def hip_call():
    p = pool[step[0] % a.pool]; step[0] += 1
    return ops.similarity_scores(feats, p["idx"], p["z_o"], p["z_k"], p["a_k"], p["aids"], bad_flag=flag)


def torch_call():
    p = pool[step[0] % a.pool]; step[0] += 1
    v = feats.index_select(0, p["idx"].reshape(-1).long()).view(B, K + 1, a.dv)
    vc = F.cosine_similarity(v[:, :1], v[:, 1:], dim=2)
    zc = F.cosine_similarity(p["z_o"][:, None], p["z_k"], dim=2)
    xe = F.cross_entropy(p["a_k"].view(B * K, a.A), p["aids_rep"], reduction="none").view(B, K)
    return vc + zc + xe


def timed(fn):
    for _ in range(a.warmup):
        fn()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(a.steps):
        fn()
    e1.record(); e1.synchronize()
    return e0.elapsed_time(e1) / a.steps


def launches(fn):
    from torch.profiler import ProfilerActivity, profile
    torch.cuda.synchronize()
    with profile(activities=[ProfilerActivity.CUDA]) as prof:
        fn()
        torch.cuda.synchronize()
    return len([e for e in prof.events() if str(e.device_type).endswith("CUDA")])


step[0] = 0; s_hip = hip_call(); step[0] = 0; s_torch = torch_call()
max_diff = float((s_hip - s_torch).abs().max())
hip_all, torch_all = [], []
for _ in range(a.repeats):                                    # alternating: both sides see the same machine state
    hip_all.append(timed(hip_call)); torch_all.append(timed(torch_call))
ops.check_similarity_ids(flag)
hip_ms, torch_ms = min(hip_all), min(torch_all)
b_feat, b_logit, b_z = B * (K + 1) * a.dv * 4, B * K * a.A * 4, B * (K + 1) * a.dz * 4
floor = b_feat + b_logit + b_z + B * (K + 2) * 4 + B * K * 4           # + ids and scores
res = {"metric": "similarity scorer: one HIP launch vs the same scores with torch ops", "B": B, "K": K, "dv": a.dv, "dz": a.dz, "A": a.A,
       "n_img": a.n_img, "pool": a.pool, "steps": a.steps, "warmup": a.warmup, "repeats": a.repeats,
       "hip_us": round(hip_ms * 1e3, 2), "torch_us": round(torch_ms * 1e3, 2), "speedup": round(torch_ms / hip_ms, 2),
       "hip_launches": launches(hip_call), "torch_launches": launches(torch_call),
       "unique_bytes_per_batch": floor, "feature_row_bytes": b_feat, "logit_bytes": b_logit, "z_bytes": b_z,
       "hip_gb_per_s": round(floor / (hip_ms * 1e-3) / 1e9, 1), "hip_frac_of_8tb_s": round(floor / (hip_ms * 1e-3) / 8e12, 3),
       "torch_gb_per_s_of_the_same_bytes": round(floor / (torch_ms * 1e-3) / 1e9, 1),
       "max_abs_diff_hip_vs_torch": max_diff,
       "hip_us_all": [round(x * 1e3, 2) for x in hip_all], "torch_us_all": [round(x * 1e3, 2) for x in torch_all]}
line = json.dumps(res)
print(line)
if a.out:
    with open(a.out, "w") as f:
        f.write(line + "\n")
