"""fp64 restatements of the kernels every trainable path ends in -- the listwise loss / rank (ncx_loss_rank, and the same arithmetic
inside ncx_train_tail), the cross-entropy head (ncx_ce_loss) and Adam (ncx_adam_step) -- with the seeded case builders the CPU and GPU
test files share (tests/test_loss_adam_cpu.py, tests/test_loss_adam_gpu.py).  No GPU, numpy only (plus the oracle's rank rule).

Tolerances live here too, next to the reasoning they come from:
  * listwise / CE: the yardstick is torch's own float32 error on the CPU against the fp64 restatement, per case family and per
    quantity (YARDSTICK below, measured by test_loss_adam_cpu.py, recorded in profiles/loss_adam_edges.json); the HIP kernel may be
    4 x that far off plus one ulp of the result (listwise_bounds).
  * Adam: a count of the fp32 roundings in k_adam (adam_bounds).
"""
import math

import numpy as np

from oracle import ncx_oracle as orc

U32 = 2.0 ** -24                      # unit roundoff of fp32 (half an ulp, relative)
FLT_MIN = float(np.finfo(np.float32).tiny)


def f32(x):
    """The value a C `float` argument receives."""
    return float(np.float32(x))


def ulp32(x):
    """One fp32 ulp at |x| (array or scalar), never below the smallest normal's."""
    return np.spacing(np.maximum(np.abs(np.asarray(x, np.float64)), FLT_MIN).astype(np.float32)).astype(np.float64)


# ---- listwise softmax cross-entropy + rank ---------------------------------------------------------------------------------------------
def kernel_scale(scale, B):
    """The scale the kernels use for a caller's `scale`: as given (a float) when positive, else 1.f / (float)B."""
    return f32(scale) if f32(scale) > 0.0 else float(np.float32(1.0) / np.float32(B))


def listwise_ref(scores_f32, gt, scale):
    """ncx_loss_rank in fp64 on the fp32 scores it is given.  `scale` is the caller's (<= 0: 1/B as the kernel forms it).
    -> dict(loss_rows [B], loss, dscores [B, K]: float64; rank [B] int32 by oracle.rank_of_gt's rule; hits [2] int: #rank<1, #rank<5)"""
    s32 = np.ascontiguousarray(scores_f32, dtype=np.float32)
    assert s32.ndim == 2
    B, K = s32.shape
    g = np.asarray(gt).astype(np.int64)
    assert g.shape == (B,) and (g >= 0).all() and (g < K).all()
    sc = kernel_scale(scale, B)
    s = s32.astype(np.float64)
    mx = s.max(1, keepdims=True)
    e = np.exp(s - mx)
    z = e.sum(1)
    sg = s[np.arange(B), g]
    rows = (np.log(z) - (sg - mx[:, 0])) * sc                   # (sg - mx is exact in fp64 for fp32 inputs of one binade range; no offset left)
    d = e / z[:, None]
    d[np.arange(B), g] -= 1.0
    rank = orc.rank_of_gt(s32, g)
    return dict(loss_rows=rows, loss=float(rows.sum()), dscores=d * sc, rank=rank,
                hits=np.array([(rank < 1).sum(), (rank < 5).sum()], dtype=np.int64), scale=sc)


def ce_ref(x, t, scale=None):
    """ncx_ce_loss in fp64 (moved here from tests/test_vqa_train_gpu.py, unchanged)."""
    x = x.astype(np.float64); B, A = x.shape
    scale = 1.0 / B if scale is None else scale
    mx = x.max(1, keepdims=True)
    lse = np.log(np.exp(x - mx).sum(1)) + mx[:, 0]
    xt = x[np.arange(B), t]
    dl = np.exp(x - lse[:, None]); dl[np.arange(B), t] -= 1.0
    rank = (x > xt[:, None]).sum(1) + ((x == xt[:, None]) & (np.arange(A)[None, :] < t[:, None])).sum(1)
    return dict(loss=float(((lse - xt) * scale).sum()), dl=dl * scale, rank=rank)


# Planted rows.  Row r of a case carries PLANTS[(r + rot) % len(PLANTS)] when K allows it (`need` candidates), else it stays a random row.
# The expected rank of each planted row is what test_loss_adam_cpu.py pins.
#   gt_first / gt_last   the ground truth at index 0 / K - 1 of a random row
#   fifth / sixth        six scores 3.00, 2.99 .. 2.95 at shuffled columns, the rest below -5: gt is the 5th (rank 4: a Recall@5 hit) /
#                        the 6th (rank 5: a miss); gaps of 0.01
#   tie_ahead            gt's score copied to a LOWER index: that copy ranks ahead (rank = #greater + 1)
#   tie_behind           gt's score copied to a HIGHER index: it does not (rank = #greater)
#   all_equal            every score 0.375: rank == gt
PLANTS = (("gt_first", 1), ("gt_last", 1), ("fifth", 6), ("sixth", 6), ("tie_ahead", 2), ("tie_behind", 2), ("all_equal", 1))
FAMILIES = ("ordinary", "spread80", "offset1e4")
SCALES = (0.0, 1.0 / 7.0, 1.0)          # 0: the kernel's 1 / B


def listwise_case(B, K, family="ordinary", seed=0, rot=0):
    """-> scores float32 [B, K], gt int32 [B], planted: {row: plant name}.  Rows are 2 N(0, 1) draws with the planted rows above;
    family "spread80": then one score of every row moved 80 above the row's maximum (even rows; a wrong candidate where K > 1, so the loss
    is ~80) or 80 below its minimum (odd rows; the ground truth where the row is not planted, so the loss is ~80 + log K);
    family "offset1e4": then the whole row shifted by +1e4 (even rows) or -1e4 (odd rows), in fp32 (the shift rounds the scores to the
    ~1e-3 grid there: the reference sees the rounded scores, ties and all)."""
    assert family in FAMILIES
    rng = np.random.default_rng(1000003 * seed + 1009 * B + K)
    s = (2.0 * rng.standard_normal((B, K))).astype(np.float32)
    gt = rng.integers(0, K, size=B).astype(np.int32)
    planted = {}
    for r in range(min(B, len(PLANTS))):
        name, need = PLANTS[(r + rot) % len(PLANTS)]
        if K < need:
            continue
        planted[r] = name
        if name == "gt_first":
            gt[r] = 0
        elif name == "gt_last":
            gt[r] = K - 1
        elif name in ("fifth", "sixth"):
            cols = rng.permutation(K)
            s[r, cols] = (-5.0 - 0.01 * np.arange(K)).astype(np.float32)
            s[r, cols[:6]] = (3.0 - 0.01 * np.arange(6)).astype(np.float32)
            gt[r] = cols[4 if name == "fifth" else 5]
        elif name == "tie_ahead":
            gt[r] = rng.integers(1, K)
            s[r, rng.integers(0, gt[r])] = s[r, gt[r]]
        elif name == "tie_behind":
            gt[r] = rng.integers(0, K - 1)
            s[r, rng.integers(gt[r] + 1, K)] = s[r, gt[r]]
        elif name == "all_equal":
            s[r] = 0.375
    if family == "spread80":
        for r in range(B):
            if r % 2 == 0:
                wrong = [k for k in range(K) if k != gt[r]]
                k = wrong[rng.integers(0, len(wrong))] if wrong else int(gt[r])
                s[r, k] = s[r].max() + np.float32(80.0)
            else:
                k = int(gt[r]) if r not in planted else int(rng.integers(0, K))
                s[r, k] = s[r].min() - np.float32(80.0)
    elif family == "offset1e4":
        sign = np.where(np.arange(B) % 2 == 0, 1.0, -1.0).astype(np.float32)
        s = (s + sign[:, None] * np.float32(1e4)).astype(np.float32)
    return np.ascontiguousarray(s), gt, planted


# The sweep of ncx_loss_rank: every K at B = 5, every B at K = 24 (B = 257, 1025: the strided loop of the finish kernel; B = 1, 3, 5:
# a last block with idle waves; K = 1: a softmax over one score; K = 25 .. 64: lanes the existing suite never fills)
LOSS_RANK_SHAPES = tuple((5, K) for K in (1, 2, 5, 23, 24, 25, 63, 64)) + tuple((B, 24) for B in (1, 3, 4, 257, 1025))

# torch's float32 error on the CPU against listwise_ref over LOSS_RANK_SHAPES x SCALES, per family (test_loss_adam_cpu.py measures it and
# checks these constants; profiles/loss_adam_edges.json holds the measured values with the HIP kernels' errors beside them).  Units: the
# error divided by the scale -- nats for loss_rows, probability for dscores -- and for `loss` divided by scale * B as well (the mean
# error per row; the ulp term of listwise_bounds carries the summation).
YARDSTICK = {
    "ordinary":  dict(loss_rows=1.5e-6, loss=1.0e-6, dscores=1.6e-7),
    "spread80":  dict(loss_rows=1.2e-5, loss=9.0e-6, dscores=1.6e-7),
    "offset1e4": dict(loss_rows=1.0e-6, loss=7.2e-7, dscores=2.2e-7),
}
YARDSTICK_FACTOR = 4.0                  # the kernel's __expf and its wave-tree summation order are not torch's


def listwise_bounds(ref, family, B):
    """Absolute bounds for a HIP result against `ref` = listwise_ref(...): 4 x torch-float32's own error plus one ulp of the result."""
    y, sc = YARDSTICK[family], ref["scale"]
    return dict(loss_rows=YARDSTICK_FACTOR * y["loss_rows"] * sc + ulp32(ref["loss_rows"]),
                loss=YARDSTICK_FACTOR * y["loss"] * sc * B + float(ulp32(ref["loss"])),
                dscores=YARDSTICK_FACTOR * y["dscores"] * sc + ulp32(ref["dscores"]))


def listwise_errors(got_rows, got_loss, got_d, ref, B):
    """Errors in the YARDSTICK's units (got_d may be None)."""
    sc = ref["scale"]
    out = dict(loss_rows=float(np.abs(np.asarray(got_rows, np.float64) - ref["loss_rows"]).max() / sc),
               loss=abs(float(got_loss) - ref["loss"]) / (sc * B))
    if got_d is not None:
        out["dscores"] = float(np.abs(np.asarray(got_d, np.float64) - ref["dscores"]).max() / sc)
    return out


def torch_f32_listwise(s32, gt, sc):
    """The same quantities by torch on the CPU in float32 (the yardstick's subject): log_softmax / softmax / F.cross_entropy(sum)."""
    import torch
    import torch.nn.functional as F
    s = torch.from_numpy(s32)
    g = torch.from_numpy(np.asarray(gt).astype(np.int64))
    sct = torch.tensor(sc, dtype=torch.float32)
    rows = -F.log_softmax(s, dim=1)[torch.arange(s.shape[0]), g] * sct
    loss = F.cross_entropy(s, g, reduction="sum") * sct
    d = F.softmax(s, dim=1)
    d[torch.arange(s.shape[0]), g] -= 1.0
    return rows.numpy(), float(loss), (d * sct).numpy()


# ---- cross-entropy head ----------------------------------------------------------------------------------------------------------------
CE_SHAPES = ((1, 1), (3, 255), (3, 256), (3, 257), (300, 7))


def ce_case(B, A, seed=0):
    """test_ce_loss_alone's rows at another shape, as far as B and A allow: row 0 one logit at +80 and the target at -80 (A >= 2), row 1 the
    target at the maximum, row 2 at the minimum, row 3 the target fifth, row 4 sixth (A > 5), row 5 an equal logit at index 0 ahead of the
    target at A - 1 (A >= 2).  -> logits float32 [B, A], target int32 [B], expect: {row: rank}."""
    rng = np.random.default_rng(7919 * seed + 31 * B + A)
    x = (rng.standard_normal((B, A)) * 2).astype(np.float32)
    t = rng.integers(0, A, size=B).astype(np.int32)
    expect = {}
    if A >= 2:
        x[0, 0], x[0, 1] = 80.0, -80.0
        t[0] = 1
        expect[0] = A - 1
    if B > 1:
        t[1] = int(x[1].argmax()); expect[1] = 0
    if B > 2:
        t[2] = int(x[2].argmin()); expect[2] = A - 1
    for r, place in ((3, 4), (4, 5)):
        if A > 5 and B > r:
            x[r] = -5.0 - 0.01 * np.arange(A)
            x[r, :6] = 3.0 - 0.01 * np.arange(6)
            t[r] = place
            expect[r] = place
    if B > 5 and A >= 2:
        x[5, 0] = x[5, A - 1] = x[5].max() + 1.0
        t[5] = A - 1
        expect[5] = 1
    return x, t, expect


# ---- Adam ------------------------------------------------------------------------------------------------------------------------------
HP_DEFAULT = dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8)
HP_ALT = dict(lr=1e-3, betas=(0.5, 0.9), eps=1e-3)
ADAM_STEPS = (1, 2, 10, 1000, 100000)
ADAM_GRAD_SCALES = (1.0, 1.0 / 8.0, 3.7)
ADAM_FAMILIES = ("normal", "zero", "tiny20", "tiny25", "mixed", "flip")
ADAM_SIZES = (1, 2, 3, 4, 5, 7, 1023, 1024, 1025)
ADAM_BIG = 4096 * 1024 + 1029          # past one pass of the 4096-block grid: the grid-stride loop, then a vector body, then a 1-element tail


def adam_ref_step(p, g, m, v, step, lr, b1, b2, eps, grad_scale=1.0, round_scalars=True):
    """ONE step of ncx_adam_step in fp64 from the given (fp32) state -> (p', m', v') float64.
    round_scalars: lr / b1 / b2 / eps / grad_scale are the fp32 values the C call receives, and the two bias-correction scalars are formed
    as the entry point forms them -- in double from those, then rounded to float.  False: plain doubles throughout (torch.optim.Adam in
    float64 is this)."""
    r = f32 if round_scalars else float
    lr, b1, b2, eps, gs = r(lr), r(b1), r(b2), r(eps), r(grad_scale)
    bc1 = 1.0 - math.pow(b1, step)
    bc2 = 1.0 - math.pow(b2, step)
    step_size = r(lr / bc1)
    inv_bc2_sqrt = r(1.0 / math.sqrt(bc2))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    gj = g * gs
    m1 = m + (gj - m) * (1.0 - b1)
    v1 = v * b2 + (1.0 - b2) * gj * gj
    den = np.sqrt(v1) * inv_bc2_sqrt + eps
    return p - step_size * (m1 / den), m1, v1


def adam_bounds(p, g, m, v, step, lr, b1, b2, eps, grad_scale=1.0):
    """Absolute bounds on |kernel - adam_ref_step| per element, from the fp32 roundings of k_adam (u = 2^-24 each, first order):
      g' = g * gscale                                1
      m' = m + (g' - m) * (1 - b1)                   3 (subtract, multiply, add; 1 - b1 is exact for b1 >= 0.5) + g' -> <= 4 u (|m| + |g'|)
      v' = v * b2 + (1 - b2) * g' * g'               4 (three products, one add) + g' twice                      -> <= 6 u (|v| + g'^2)
           ... + the smallest normal float: g'^2 may underflow, and whether the result is then a denormal or zero is not specified
      den = sqrtf(v') * inv_bc2_sqrt + eps           3 + half of v''s 6 (the square root halves a relative error; all terms positive)
      p' = p - step_size * (m' / den)                divide, multiply: 2; subtract: 1 on |p'| <= |p| + |dp|
    so |dp| carries 3 + 3 + 2 = 8 u and p' 1 u more: 9 u (|p| + |dp|).  On top of that p' inherits the error of the m' the kernel feeds
    it (the reference feeds its unrounded m'): step_size / den times m''s bound above -- where m and g' cancel, |dp| alone says nothing
    about it -- and the underflow floor of v' through the square root (sqrt(FLT_MIN) * inv_bc2_sqrt against den)."""
    lr, b1, b2, eps, gs = f32(lr), f32(b1), f32(b2), f32(eps), f32(grad_scale)
    step_size = f32(lr / (1.0 - math.pow(b1, step)))
    inv_bc2_sqrt = f32(1.0 / math.sqrt(1.0 - math.pow(b2, step)))
    p, g, m, v = (np.asarray(a, np.float64) for a in (p, g, m, v))
    p1, m1, v1 = adam_ref_step(p, g, m, v, step, lr, b1, b2, eps, gs)
    gj = np.abs(g * gs)
    tol_m = 4 * U32 * (np.abs(m) + gj)
    tol_v = 6 * U32 * (np.abs(v) + gj * gj) + FLT_MIN
    den = np.sqrt(v1) * inv_bc2_sqrt + eps
    dp = np.abs(p1 - p)
    tol_p = 9 * U32 * (np.abs(p) + dp) + step_size / den * tol_m + dp * (math.sqrt(FLT_MIN) * inv_bc2_sqrt / den)
    return tol_p, tol_m, tol_v


def adam_case(n, step, family, seed=0):
    """-> p, g, m, v float32 [n].  Step 1 starts from zero moments; later steps from random ones (signed m ~ 0.1 N(0, 1), positive
    v ~ 0.01 chi^2), not iterated from zero.  Gradient families:
      normal   N(0, 1)                      zero    all zero ("zero" with step 1 has m = 0: p must not move)
      tiny20   +-1e-20 x U(0.5, 2)          tiny25  +-1e-25 x U(0.5, 2)        (g^2 underflows: 1e-40 is a denormal, 1e-50 is zero)
      mixed    +-10^U(-6, 3)                flip    -sign(m) |N(0, 1)|         (the update crosses zero in m)"""
    assert family in ADAM_FAMILIES
    rng = np.random.default_rng(104729 * seed + 7 * n + step % 1000 + 13 * ADAM_FAMILIES.index(family))
    p = rng.standard_normal(n).astype(np.float32)
    if step == 1:
        m = np.zeros(n, np.float32); v = np.zeros(n, np.float32)
    else:
        m = (0.1 * rng.standard_normal(n)).astype(np.float32)
        v = (0.01 * rng.standard_normal(n) ** 2 + 1e-12).astype(np.float32)
    sign = np.where(rng.random(n) < 0.5, -1.0, 1.0)
    if family == "normal":
        g = rng.standard_normal(n)
    elif family == "zero":
        g = np.zeros(n)
    elif family in ("tiny20", "tiny25"):
        g = sign * (1e-20 if family == "tiny20" else 1e-25) * rng.uniform(0.5, 2.0, n)
    elif family == "mixed":
        g = sign * 10.0 ** rng.uniform(-6.0, 3.0, n)
    else:
        g = -np.where(m >= 0, 1.0, -1.0) * np.abs(rng.standard_normal(n))
    return p, g.astype(np.float32), m, v
