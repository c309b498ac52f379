"""The fused forward kernel (csrc/ncx_main.h: k_main_fwd, k_main_fixup) at its edge shapes: an fp64 restatement of the Linear layers
with a per-element rounding bound, and the table of cases.  Plain numpy / torch float64; tests/test_main_fwd_edges_cpu.py checks what
this file claims, tests/test_main_fwd_edges_gpu.py runs the kernels on the cases.

The restatement
    linear_1 in the kernel's association (cx.py:309-322 with softmax(a).E.W^T taken as softmax(a).(E.W^T)):
        pre_1[r] = x[r] . Wc^T + Sh[r // K],   x[r] = [v_k | v_o * v_k | dist, rank | z_k | softmax(a_k)]  (lesions: no v_o * v_k block,
        dist = 0, rank from the caller, the a_emb_other noise block in place of the softmax),  Wc = [W1 column slices | Gt],
        Gt = W1[:, a_emb_other] . E^T,  Sh[b] = b1 + [v_o | q | z_o | a_emb_gt] . W1[:, shared columns]^T
    hidden layers: pre_l = h_{l-1} . W_l^T + b_l
    h_l = mask_l * relu(pre_l) / (1 - p)       (eval mode: mask = 1, p = 0)
    S_l = (|x| . |W|^T + |Sh| + |bias|) / (1 - p): the magnitude sum of the products h_l is made of (Sh = 0 for l > 1; for l = 1 the bias is
        b1, which Sh holds)
everything from the fp32 inputs and weights, in float64.  Layer l > 1 takes the h_{l-1} it is GIVEN (the device's), so a layer is judged alone.

The bound    |h_dev - h_ref| <= c * 2^-24 * S_l   element by element.  Any order of a sum of n products is within n * 2^-24 * S of the
exact sum (to first order), so c < din always holds for a correct kernel; c is 4 x what torch's float32 oracle (orc.forward_faithful:
another summation order of the same products, not another algorithm) reaches on the same cases, per group: ORACLE32_RATIO, measured on
the CPU by test_main_fwd_edges_cpu.py and recorded in profiles/main_fwd_edges.json -- the margin and the reasoning of
profiles/loss_adam_edges.json.  relu is 1-Lipschitz and the mask and 1 / (1 - p) are exact factors of both sides, so the bound on pre_l
carries to h_l with S scaled by 1 / (1 - p).
"""
import zlib

import numpy as np
import torch

from oracle import ncx_oracle as orc

U24 = 2.0 ** -24
FEATS = ("image_features", "q_emb", "z_orig", "z_knns", "a_knns", "answer_aids")

# max |h_oracle32 - h_ref| / (2^-24 S) of torch-float32 (one thread) over the group's cases, rounded up, on the host that wrote
# profiles/main_fwd_edges.json; another CPU's BLAS sums in another order, so test_recorded_oracle32_ratios_reproduce asks for the same
# size (a factor of three), not the same digits.  The kernels' bound is C_MARGIN x this and does not move with the host.
ORACLE32_RATIO = {"A": 6.0, "B": 5.2, "C": 5.2, "D": 7.9, "E": 5.5, "F": 2.2, "G": 7.4, "H": 6.2, "I": 6.6}
C_MARGIN = 4.0


def bound_c(group):
    return C_MARGIN * ORACLE32_RATIO[group]


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)


class MainFwdRef:
    """fp64 restatement of one forward.  params: state_dict names -> fp32 tensors; batch: FEATS (+ a_emb_gt, v_rank under their lesions);
    masks: None (eval) or one [B*K, H] keep mask per layer."""

    def __init__(self, params, d, batch, spec=None, drop_p=0.0, masks=None):
        spec = dict(orc.DEFAULT_SPEC, **(spec or {}))
        self.d, self.spec, self.p = d, spec, float(np.float32(drop_p)) if masks is not None else 0.0
        self.masks = None if masks is None else [_f64(m) for m in masks]
        feats = _f64(batch["image_features"])
        B, K = feats.shape[0], d.K
        self.B, self.M = B, B * K
        W1, o = _f64(params["linear_1.weight"]), d.offsets()
        sl = lambda name, w: W1[:, o[name]: o[name] + w]
        E = _f64(params["answer_embedding.weight"])
        v_o, v_k = feats[:, 0], feats[:, 1:]                                             # [B, dv], [B, K, dv]
        if spec["a_emb"]:
            a_gt = E[np.asarray(batch["answer_aids"]).astype(np.int64)]
            a = _f64(batch["a_knns"])
            e = np.exp(a - a.max(-1, keepdims=True))
            x_a, w_a = e / e.sum(-1, keepdims=True), sl("a_emb_other", d.da) @ E.T          # softmax(a_k) [B, K, A] against Gt [H, A]
        else:
            a_gt, x_a, w_a = _f64(batch["a_emb_gt"]), _f64(batch["a_knns"]), sl("a_emb_other", d.da)
        # the per-triplet shared part (+ bias)
        xs = np.concatenate([v_o, _f64(batch["q_emb"]), _f64(batch["z_orig"]), a_gt], 1)
        ws = np.concatenate([sl("v_orig", d.dv), sl("q_emb", d.dq), sl("z_orig", d.dz), sl("a_emb_gt", d.da)], 1)
        self.b1 = _f64(params["linear_1.bias"])
        self.sh = xs @ ws.T + self.b1                                                     # [B, H]
        self.xs = xs                                                                      # (the shared row: tests/main_bwd_ref.py)
        # the candidate row, segment by segment
        dist = np.sqrt(((v_o[:, None, :] - v_k + 1e-6) ** 2).sum(-1, keepdims=True)) if spec["v_dist"] else np.zeros((B, K, 1))
        rank = np.broadcast_to(np.eye(K), (B, K, K)) if spec["v_rank"] else _f64(batch["v_rank"])
        xc, wc = [v_k], [sl("v_other", d.dv)]
        if spec["v_mult"]:
            xc.append(v_o[:, None, :] * v_k); wc.append(sl("v_mult", d.dv))
        xc += [dist, rank, _f64(batch["z_knns"]), x_a]
        wc += [sl("v_dist", 1), sl("v_rank", K), sl("z_other", d.dz), w_a]
        self.x = np.concatenate(xc, -1).reshape(self.M, -1)
        self.wc = np.concatenate(wc, 1)
        self.dist = dist.reshape(self.M)
        self.params = params

    def layer(self, l, h_prev=None):
        """-> (pre_l, h_l, S_l), each [B*K, H].  l > 1: from the h_{l-1} given (the device's, or the restatement's own)."""
        if l == 1:
            shr = np.repeat(self.sh, self.d.K, axis=0)
            pre = self.x @ self.wc.T + shr
            S = np.abs(self.x) @ np.abs(self.wc).T + np.abs(shr) + np.abs(self.b1)
        else:
            W, b = _f64(self.params["linear_%d.weight" % l]), _f64(self.params["linear_%d.bias" % l])
            hp = _f64(h_prev)
            pre = hp @ W.T + b
            S = np.abs(hp) @ np.abs(W).T + np.abs(b)
        h = np.maximum(pre, 0.0)
        if self.masks is not None:
            h = h * self.masks[l - 1] / (1.0 - self.p)
            S = S / (1.0 - self.p)
        return pre, h, S

    def chain(self):
        """The whole forward on the restatement's own activations -> dict(pre=[...], h=[...], S=[...], scores [B, K])."""
        out = dict(pre=[], h=[], S=[])
        h = None
        for l in range(1, self.d.L + 1):
            pre, h, S = self.layer(l, h)
            out["pre"].append(pre); out["h"].append(h); out["S"].append(S)
        out["scores"] = (h @ _f64(self.params["out.weight"]).T + _f64(self.params["out.bias"])).reshape(self.B, self.d.K)
        return out


def ratio(h_got, h_ref, S):
    """max |h_got - h_ref| / (2^-24 S) over the elements (an element whose S is 0 must be exact)."""
    err = np.abs(_f64(h_got) - h_ref)
    assert (err[S == 0] == 0).all()
    return float((err[S > 0] / (U24 * S[S > 0])).max())


def oracle32_ratio(case):
    """The float32 oracle's worst ratio over the layers of one case, every layer judged alone (its own h_{l-1} as the input); on one thread, so
    that the figure does not depend on the machine's core count."""
    d, params, batch, spec, masks = build(case)
    taps = {}
    threads = torch.get_num_threads()
    torch.set_num_threads(1)                 # (the BLAS behind torch picks its blocking, hence its summation order, by the thread count)
    try:
        with torch.no_grad():
            orc.forward_faithful(params, d, *[batch[k] for k in FEATS], spec=spec, drop_p=case["p"], keep_masks=masks,
                                 a_emb_gt_override=batch.get("a_emb_gt"), v_rank_override=batch.get("v_rank"), taps=taps)
    finally:
        torch.set_num_threads(threads)
    ref = MainFwdRef(params, d, batch, spec, case["p"], masks)
    worst, h32 = 0.0, None
    for l in range(1, d.L + 1):
        _, h_ref, S = ref.layer(l, h32)
        h32 = torch.relu(taps["pre%d" % l].reshape(-1, d.H))
        if masks is not None:
            h32 = h32 * masks[l - 1] / (1.0 - case["p"])
        worst = max(worst, ratio(h32, h_ref, S))
    return worst


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# Constants of the kernel the cases are placed around: 32-deep k-steps over operands whose 16-byte windows slide left at a segment's end
# against weight slices zero-padded to 32 columns; chain tiles 48x128 / 96x64 / 96x128 / 160x128 (NCX_MAIN_CFG 0..3) and 64x64 for short
# chains; fold tiles 48 / 96 / 192 rows x 64 (K = 24: 2 / 4 / 8 triplets; K = 48 on 96 / 192 only); 16-byte output pieces whose row-add,
# bias and mask operands come from a window slid left at the last columns (H % 4 != 0); split > 1: raw partial tiles to a slab,
# k_main_fixup adds them and runs the epilogue, 4 columns per thread.
BASE = dict(K=5, B=11, dv=36, dq=8, dz=20, da=12, A=44, H=37, L=1)
LESIONS = {"no_v_mult": dict(v_mult=False), "no_v_dist": dict(v_dist=False), "no_v_rank": dict(v_rank=False), "no_a_emb": dict(a_emb=False),
           "all_off": dict(v_mult=False, v_dist=False, v_rank=False, a_emb=False)}
DROP_SEED = 0x1234567890ABCDEF
CASES = []


def _case(group, tag, env=None, lesion=None, drop=None, p=0.0, fp32=False, tile=None, split=1, hidden_split=None, cu_dependent=False, **over):
    """One case.  env: experiment hooks (set with NCX_EXPERIMENT=1 before the workspace is sized).  The route the case must report
    (ncx_plan_query NCX_QUERY_FWD_ROUTE) is stated here, from the kernel family's rules as DESIGN.md gives them, not asked of the library:
    engine 2 (the per-triplet fold) for K = 24 / 48 with v_o * v_k present, whole 32-column v rows at least 64 wide, unsplit and not
    switched off; else engine 1.  The distance is taken inside the chain kernel when it sees whole unsplit v rows of both v segments."""
    c = dict(BASE, **over)
    env = dict(env or {})
    spec = LESIONS[lesion] if lesion else {}
    v_mult, v_dist = spec.get("v_mult", True), spec.get("v_dist", True)
    fold = c["K"] in (24, 48) and v_mult and c["dv"] % 32 == 0 and c["dv"] >= 64 and split == 1 and "NCX_NO_VFOLD" not in env
    if fold:
        tile = 192 if env.get("NCX_FOLD8") == "1" else 96 if (env.get("NCX_FOLD4") == "1" or c["K"] == 48) else 48
    dist = v_mult and v_dist and c["dv"] % 32 == 0 and split == 1 and not fold and "NCX_NO_DIST_IN_MAIN" not in env
    fused_hidden = c["H"] % 4 == 0
    route = dict(engine=2 if fold else 1, tile=tile if tile is not None else int(env.get("NCX_MAIN_CFG", 0)), split=split, dist_in_main=dist,
                 hidden_engine=-1 if c["L"] == 1 else int(fused_hidden))
    if c["L"] > 1 and fused_hidden:
        route["hidden_split"] = hidden_split if hidden_split is not None else split if "NCX_MAIN_SPLIT" in env else 1
    c.update(group=group, id="%s-%s" % (group, tag), env=env, lesion=lesion, drop=drop, p=p, fp32=fp32, route=route, cu_dependent=cu_dependent)
    CASES.append(c)
    return c


def _split_env(s):
    return {} if s == 1 else {"NCX_MAIN_SPLIT": str(s)}


# A: column edges x epilogue.  H % 4 = 0..3 below one 16-byte piece, around the 128-column tile edge; unsplit epilogue and k_main_fixup
for H in (4, 5, 6, 7, 127, 128, 129, 130, 131):
    for s in (1, 2, 3):
        _case("A", "H%d-s%d" % (H, s), env=_split_env(s), split=s, H=H)
# B: reduction extents, one width at a time (H = 37)
for dv in (4, 28, 32, 60, 64, 68, 100):
    _case("B", "dv%d" % dv, dv=dv)
for dz in (4, 28, 32, 36, 64):
    _case("B", "dz%d" % dz, dz=dz)
for A in (4, 28, 32, 36, 64, 68, 132):
    _case("B", "A%d" % A, A=A)
for da in (4, 28, 32, 36, 68):
    _case("B", "lesion-da%d" % da, lesion="no_a_emb", da=da, A=7)
_case("B", "dv256-natural-split", dv=256, split=2, cu_dependent=True)       # 20 k-steps: two chunks of >= 8 (a chip of 256 CUs)
# C: rows per triplet: the dist | rank segment's width, rowdiv, a triplet longer than a tile, M equal to a tile or one over
for K, B in ((3, 1), (3, 16), (3, 17), (4, 12), (7, 7), (23, 2), (24, 3), (25, 2), (47, 1), (48, 3), (49, 2), (63, 1), (64, 1), (64, 2)):
    _case("C", "K%d-B%d" % (K, B), K=K, B=B)
# D: operand sequences
for H in (37, 130):
    for name in LESIONS:
        _case("D", "%s-H%d" % (name, H), lesion=name, H=H)
# E: the distance inside the chain kernel, and the same shapes with k_prep computing it
for H in (37, 130):
    for K, dv, extra in ((5, 32, {}), (5, 64, {}), (5, 96, {}), (24, 32, {}), (24, 64, {"NCX_NO_VFOLD": "1"})):
        _case("E", "K%d-dv%d-H%d" % (K, dv, H), env=extra, K=K, dv=dv, H=H)
        _case("E", "K%d-dv%d-H%d-prep" % (K, dv, H), env=dict(extra, NCX_NO_DIST_IN_MAIN="1"), K=K, dv=dv, H=H)
# F: the fold forms (fp32 forms, named: the bf16 x 6 variant has another 192-row kernel).  One case per (shape, form); the GPU file also
# compares the forms of a shape bit for bit.
FOLD_FORMS = {48: {"NCX_FOLD4": "0", "NCX_FOLD8": "0"}, 96: {"NCX_FOLD4": "1", "NCX_FOLD8": "0"}, 192: {"NCX_FOLD4": "1", "NCX_FOLD8": "1"}}
for dv in (64, 96):
    for H in (5, 63, 65, 253):
        for B in (1, 2, 3, 5, 8, 9):
            for rows in (48, 96, 192):
                _case("F", "K24-dv%d-H%d-B%d-%d" % (dv, H, B, rows), env=FOLD_FORMS[rows], fp32=True, K=24, dv=dv, H=H, B=B)
for H in (63, 253):
    for B in (1, 3, 5):
        for rows in (96, 192):
            _case("F", "K48-dv64-H%d-B%d-%d" % (H, B, rows), env=FOLD_FORMS[rows], fp32=True, K=48, dv=64, H=H, B=B)
# G: the chain tile forms at M = BM and just over (K = 3; no K = 3 batch has 160 or 163 rows: 160 = 4 x 40, and 162 = 3 x 54)
for cfg, shapes in ((0, ((3, 16), (3, 17))), (1, ((3, 32), (3, 33))), (2, ((3, 32), (3, 33))), (3, ((4, 40), (3, 54)))):
    for K, B in shapes:
        for H in (63, 65, 129, 253):
            _case("G", "cfg%d-M%d-H%d" % (cfg, K * B, H), env={"NCX_MAIN_CFG": str(cfg)}, fp32=True, K=K, B=B, H=H)
_case("G", "short-natural", fp32=True, tile=4, cu_dependent=True, K=3, B=1367, H=516, dv=64)    # 8 k-steps, 585 tiles of 64 x 64
# H: hidden layers.  Fused (H % 4 == 0) on forms 0..2, split at H >= 132; mixed: linear_1 fused, layers 2+ on the generic engine
for H in (4, 36, 60, 64, 68, 132, 260):
    for L in (2, 3):
        for cfg in (0, 1, 2):
            _case("H", "H%d-L%d-cfg%d" % (H, L, cfg), env={"NCX_MAIN_CFG": str(cfg)}, fp32=True, H=H, L=L)
        if H >= 132:
            _case("H", "H%d-L%d-s2" % (H, L), env=_split_env(2), split=2, H=H, L=L)
for H in (37, 131):
    for L in (2, 3):
        _case("H", "mixed-H%d-L%d" % (H, L), H=H, L=L)
# I: dropout at ragged H: explicit masks and the kernel's counter-based generator, unsplit epilogue and k_main_fixup
for H in (5, 37, 131):
    for L in (1, 2):
        for drop in ("masks", "rng"):
            for s in (1, 2):
                _case("I", "H%d-L%d-%s-s%d" % (H, L, drop, s), env=_split_env(s), split=s, drop=drop, p=0.25, H=H, L=L)
# J: the whole step (forward, loss, backward) through compare_with_oracle: cases of the groups above at A in {36, 132}, da in {12, 100};
# the answer-embedding gradient (the same kernel family on its two-segment chain) also on forms 0..2
J_CASES = []
for tag, kw in (("A-H5-s1", dict(H=5)), ("A-H129-s2", dict(H=129, env=_split_env(2), split=2)), ("A-H131-s3", dict(H=131, env=_split_env(3), split=3)),
                ("B-dv68", dict(dv=68)), ("B-lesion-da100", dict(lesion="no_a_emb", da=100, A=7)), ("C-K49-B2", dict(K=49, B=2)),
                ("D-all_off-H130", dict(lesion="all_off", H=130)), ("E-K5-dv64-H37", dict(dv=64)),
                ("F-K24-dv64-H65-B5-96", dict(env=FOLD_FORMS[96], K=24, dv=64, H=65, B=5)), ("G-cfg1-M99-H129", dict(env={"NCX_MAIN_CFG": "1"}, K=3, B=33, H=129)),
                ("G-cfg2-M99-H65", dict(env={"NCX_MAIN_CFG": "2"}, K=3, B=33, H=65)), ("G-cfg0-M51-H253", dict(env={"NCX_MAIN_CFG": "0"}, K=3, B=17, H=253)),
                ("H-H132-L3-s2", dict(env=_split_env(2), split=2, H=132, L=3)), ("H-mixed-H131-L2", dict(H=131, L=2)),
                ("I-H37-L2-rng-s2", dict(env=_split_env(2), split=2, drop="rng", p=0.25, H=37, L=2))):
    for A, da in ((36, 12), (132, 100)) if "da" not in kw else ((kw["A"], kw["da"]),):
        kw2 = dict(kw, A=A, da=da)
        J_CASES.append(_case("J", "%s-A%d-da%d" % (tag, A, da), **kw2))
CASES = [c for c in CASES if c["group"] != "J"]
BY_ID = {c["id"]: c for c in CASES + J_CASES}
GROUPS = sorted({c["group"] for c in CASES})


def shape_key(c):
    """What the inputs and the restatement of a case depend on (not its hooks: the forms of one shape share them)."""
    return tuple(c[k] for k in ("K", "B", "dv", "dq", "dz", "da", "A", "H", "L", "lesion", "drop", "p"))


def build(c):
    """-> (orc.Dims, params, batch (with the lesions' inputs and `gt`), spec or None, keep masks or None), seeded by the shape."""
    d = orc.Dims(K=c["K"], dv=c["dv"], dq=c["dq"], dz=c["dz"], da=c["da"], A=c["A"], H=c["H"], L=c["L"])
    B = c["B"]
    seed = zlib.crc32(repr(shape_key(c)).encode()) % (2 ** 31)
    rng = np.random.default_rng(seed)
    t = lambda a: torch.from_numpy(np.asarray(a, np.float32))
    params = orc.init_params(d, seed=seed % 1000 + 1, gain=3.0)
    batch = dict(image_features=t(np.abs(rng.standard_normal((B, d.K + 1, d.dv))) * 0.45), q_emb=t(rng.standard_normal((B, d.dq)) * 0.3),
                 z_orig=t(rng.standard_normal((B, d.dz))), z_knns=t(rng.standard_normal((B, d.K, d.dz))),
                 a_knns=t(rng.standard_normal((B, d.K, d.A)) * 2), answer_aids=torch.from_numpy(rng.integers(0, d.A, size=B)),
                 gt=torch.from_numpy(rng.integers(0, d.K, size=B)))
    if B > 1:
        batch["answer_aids"][0] = batch["answer_aids"][B - 1]          # a duplicated answer id
    spec = None
    if c["lesion"]:
        spec = dict(orc.DEFAULT_SPEC, **LESIONS[c["lesion"]])
        if not spec["v_rank"]:
            batch["v_rank"] = t(rng.random((B, d.K, d.K)))
        if not spec["a_emb"]:
            batch["a_knns"] = t(rng.random((B, d.K, d.da)))
            batch["a_emb_gt"] = t(rng.random((B, d.da)))
    masks = None
    if c["drop"]:
        masks = [orc.dropout_keep_mask(DROP_SEED, l, B * d.K, d.H, c["p"]) for l in range(1, d.L + 1)]
    return d, params, batch, spec, masks


def din(c):
    return 3 * c["dv"] + 2 * c["da"] + 2 * c["dz"] + c["dq"] + c["K"] + 1
