"""Shapes, inputs and the planner's rules for the Gt + Sh pair launch (csrc/ncx_main.h: the PAIR form of k_main_fwd and k_main_fixup_pair;
csrc/ncx_plan.hip: plan_gtsh_pair), shared by tests/test_gtsh_pair_gpu.py and tests/test_gtsh_pair_cpu.py.

Gt = W1[:, a_other] . E^T and Sh = b1 + [v_o | q | z_o | E[aid]] . W1[:, shared]^T run as ONE launch of 64 x 64 tiles, each problem cut into
the k-chunks the generic engine gives it on a launch of its own (32-deep steps, chunk z of S takes steps [T z / S, T (z + 1) / S) of the
problem's chain), a workgroup running one or more consecutive chunks, raw partial tiles to a slab, one fix-up: the results are the two
launches' bit for bit.  The shapes are the smallest at which that can go wrong: a second column tile 6 wide (A = 70) and a full one
(A = 64), one row short of a tile and one over for Sh (B = 5, 65), H = 20 and 68 (Gt's rows, Sh's columns), every reduction extent ragged
(da = 36, dq = 100, dz = 12, dv = 520: last steps partly beyond the extent, chunk ends inside segments and on their boundaries), and a
shape whose two problems get different splits, both above 1 (da = 516)."""
import zlib

import numpy as np
import torch

from oracle import ncx_oracle as orc

K = 3
N_IMG = 7
SHAPES = {
    # id: B, A, H, dv, dq, dz, da
    "B5-A70-H20": dict(B=5, A=70, H=20, dv=520, dq=100, dz=12, da=36),
    "B65-A64-H68": dict(B=65, A=64, H=68, dv=520, dq=100, dz=12, da=36),
    "B5-A64-H68": dict(B=5, A=64, H=68, dv=520, dq=100, dz=12, da=36),
    "B65-A70-H20-da516": dict(B=65, A=70, H=20, dv=36, dq=100, dz=12, da=516),
}
# configs[1] of the benchmark and its 64-triplet data-parallel shard: planner checks only, never run by a test
WORKLOAD = {
    "configs1": dict(B=512, A=2000, H=256, dv=2048, dq=2400, dz=360, da=2400, K=24),
    "shard64": dict(B=64, A=2000, H=256, dv=2048, dq=2400, dz=360, da=2400, K=24),
}


def ksteps(k):
    return (k + 31) // 32


def chain_steps(s):
    """-> (T_gt, T_sh): 32-deep k-steps of the two chains."""
    return ksteps(s["da"]), ksteps(s["dv"]) + ksteps(s["dq"]) + ksteps(s["dz"]) + ksteps(s["da"])


def tiles(s):
    c = lambda a: (a + 63) // 64
    return c(s["H"]) * c(s["A"]), c(s["B"]) * c(s["H"])


def chunks(T, S):
    """The kernel's cut of T steps into S chunks."""
    return [(T * z // S, T * (z + 1) // S) for z in range(S)]


def check_plan(s, plan, gt_split, sh_split):
    """The rules for the joint plan.  The k-chunks are those of the two launches it replaces (gt_split, sh_split: ncx_plan_query of Gt and Sh),
    no chunk under 8 steps unless the problem is unsplit, each reduction covered exactly once; the workgroups (whole numbers of consecutive
    chunks each) fit one round of slots, on the chip and on every XCD: the kernel deals (row tile, workgroup) units round-robin over the 8
    XCDs and keeps a unit's column tiles together."""
    (t_gt, t_sh), c = chain_steps(s), (lambda a: (a + 63) // 64)
    assert (plan["s_gt"], plan["s_sh"]) == (gt_split, sh_split), plan
    for T, S, W in ((t_gt, plan["s_gt"], plan["w_gt"]), (t_sh, plan["s_sh"], plan["w_sh"])):
        assert S >= 1
        cs = chunks(T, S)
        assert S == 1 or min(b - a for a, b in cs) >= 8, (T, S, cs)
        assert cs[0][0] == 0 and cs[-1][1] == T and all(cs[i][1] == cs[i + 1][0] for i in range(S - 1)), cs
        assert max(b - a for a, b in cs) - min(b - a for a, b in cs) <= 1, cs
        if plan["taken"]:
            assert W >= 1 and S % W == 0, plan
    if plan["taken"]:
        assert plan["s_gt"] > 1 or plan["s_sh"] > 1, plan
        n_gt, n_sh = tiles(s)
        assert n_gt * plan["w_gt"] + n_sh * plan["w_sh"] <= plan["slots"], plan
        per_xcd = -(-c(s["H"]) * plan["w_gt"] // 8) * c(s["A"]) + -(-c(s["B"]) * plan["w_sh"] // 8) * c(s["H"])
        assert per_xcd * 8 <= plan["slots"], (plan, per_xcd)


def build(sid, lesion=False):
    """-> (orc.Dims, params, batch, table, img_idx): `batch` is what the fp64 restatement reads (dense image_features = table[img_idx]);
    the device reads `table` through `img_idx`.  Original images repeat across triplets, one triplet's original is the LAST table row,
    answer ids repeat and include A - 1."""
    s = SHAPES[sid]
    d = orc.Dims(K=K, dv=s["dv"], dq=s["dq"], dz=s["dz"], da=s["da"], A=s["A"], H=s["H"], L=1)
    B = s["B"]
    seed = zlib.crc32(sid.encode()) % (2 ** 31)
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    params = orc.init_params(d, seed=seed % 1000 + 1, gain=3.0)
    table = t(np.abs(rng.standard_normal((N_IMG, d.dv))) * 0.45)
    idx = rng.integers(0, N_IMG, size=(B, K + 1))
    idx[0, 0] = N_IMG - 1
    idx[B - 1, 0] = idx[B // 2, 0] = 2                      # a repeated original image
    idx[0, K] = N_IMG - 1
    aids = rng.integers(0, d.A, size=B)
    aids[0] = d.A - 1
    aids[B - 1] = aids[B // 2]
    img_idx = torch.from_numpy(idx.astype(np.int32))
    batch = dict(image_features=table[img_idx.long()], q_emb=t(rng.standard_normal((B, d.dq)) * 0.3), z_orig=t(rng.standard_normal((B, d.dz))),
                 z_knns=t(rng.standard_normal((B, K, d.dz))), a_knns=t(rng.standard_normal((B, K, d.A)) * 2),
                 answer_aids=torch.from_numpy(aids))
    if lesion:
        batch["a_knns"] = t(rng.random((B, K, d.da)))
        batch["a_emb_gt"] = t(rng.random((B, d.da)))
    return d, params, batch, table, img_idx


def c_dims(s, flags, k=K, n_img=N_IMG):
    from neuralcx import _lib
    n = _lib.NcxDims()
    n.B, n.K, n.dv, n.dq, n.dz, n.da, n.A, n.H, n.L = s["B"], s.get("K", k), s["dv"], s["dq"], s["dz"], s["da"], s["A"], s["H"], 1
    n.n_img = n_img
    n.flags = flags
    return n
