"""Full-validation timing of the semantic baseline scorer (ncx_semantic_scores; reference cx.py:182-209): 118 499 synthetic
triplets in batches of 512 (24 candidates, 2000 answers), each batch scored, then ranking_loss + Recall@1/@5
(ncx_loss_rank), as the CLI's evaluate loop does.  A pool of distinct logit blocks (larger than the last-level cache) is
cycled so that every batch streams its logits from HBM.  Device-synchronised timing (HIP events over the whole loop); the
cosine Gram build (ncx_cosine_gram, 2000 x 2400) is timed separately.  Prints one JSON line."""
import argparse, json, os, sys
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
import torch
from neuralcx import ops

ap = argparse.ArgumentParser()
ap.add_argument("--n", type=int, default=118499); ap.add_argument("--batch", type=int, default=512)
ap.add_argument("--K", type=int, default=24); ap.add_argument("--A", type=int, default=2000); ap.add_argument("--da", type=int, default=2400)
ap.add_argument("--pool", type=int, default=8, help="distinct logit blocks cycled (8 x 98 MB)")
ap.add_argument("--repeats", type=int, default=5); ap.add_argument("--lam", type=float, default=0.5)
a = ap.parse_args()
dev = torch.device("cuda:0")
g = torch.Generator(device=dev).manual_seed(0)
emb = torch.randn(a.A, a.da, generator=g, device=dev)
pool = [torch.randn(a.batch, a.K, a.A, generator=g, device=dev) * 2.0 for _ in range(a.pool)]
aids = torch.randint(0, a.A, (a.batch,), generator=g, device=dev, dtype=torch.int32)
gt = torch.randint(0, a.K, (a.batch,), generator=g, device=dev, dtype=torch.int32)
flag = torch.zeros(1, dtype=torch.int32, device=dev)
sizes = [min(a.batch, a.n - lo) for lo in range(0, a.n, a.batch)]


def ev():
    return torch.cuda.Event(enable_timing=True)


gram = ops.cosine_gram(emb)                                   # warm-up (module load)
torch.cuda.synchronize()
gram_ms = []
for _ in range(a.repeats):
    e0, e1 = ev(), ev(); e0.record(); gram = ops.cosine_gram(emb); e1.record(); e1.synchronize(); gram_ms.append(e0.elapsed_time(e1))


def run(with_loss):
    hits = torch.zeros(2, dtype=torch.int64, device=dev)
    for i, n in enumerate(sizes):
        sc = ops.semantic_scores(pool[i % a.pool][:n], aids[:n], gram, a.lam, bad_flag=flag)
        if with_loss:
            hits += ops.ranking_loss(sc, gt[:n], want_grad=False)["hits"]
    return hits


run(True); torch.cuda.synchronize()
loop_ms, scorer_ms = [], []
for _ in range(a.repeats):
    e0, e1 = ev(), ev(); e0.record(); hits = run(True); e1.record(); e1.synchronize(); loop_ms.append(e0.elapsed_time(e1))
    e0, e1 = ev(), ev(); e0.record(); run(False); e1.record(); e1.synchronize(); scorer_ms.append(e0.elapsed_time(e1))
ops.check_semantic_ids(flag)
nb = len(sizes)
loop, scorer = min(loop_ms), min(scorer_ms)
bytes_batch = a.batch * a.K * a.A * 4 + a.batch * a.A * 4 + a.batch * 4 + a.batch * a.K * 4     # logits + Gram rows + ids + scores
us_scorer = scorer * 1e3 / nb
print(json.dumps({
    "metric": "semantic baseline evaluation (scorer + ranking_loss + Recall@1/@5), full validation scale",
    "triplets": a.n, "batch": a.batch, "K": a.K, "A": a.A, "batches": nb,
    "triplets_per_s": round(a.n / (loop / 1e3), 1), "us_per_batch": round(loop * 1e3 / nb, 2),
    "scorer_us_per_batch": round(us_scorer, 2), "bytes_per_batch": bytes_batch,
    "scorer_gb_per_s": round(bytes_batch / (us_scorer * 1e-6) / 1e9, 1),
    "frac_of_8tb_s": round(bytes_batch / (us_scorer * 1e-6) / 8e12, 3), "target_us_per_batch": 20.0,
    "gram_ms": round(min(gram_ms), 3), "gram_tflops": round(2.0 * a.A * a.A * a.da / (min(gram_ms) * 1e-3) / 1e12, 1),
    "loop_ms_all": [round(x, 3) for x in loop_ms], "scorer_ms_all": [round(x, 3) for x in scorer_ms],
    "recall_5_random": round(float(hits[1]) / a.n, 4)}))
