"""The backward of the NeuralCX step (csrc/ncx_backward.hip, ncx_dwkm.hip, ncx_dwtn.hip, the grouped and chain GEMMs) product by product:
an fp64 restatement with a per-element rounding bound, the CPU yardstick the bound's constants come from, and the table of cases.  Plain
numpy / torch float64; tests/test_main_bwd_edges_cpu.py checks what this file claims, tests/test_main_bwd_edges_gpu.py runs the kernels.

Every product is judged ALONE, from what the device handed to the kernel that computes it: dpre_1 (NCX_WS_DPRE1), dpre_2 (NCX_WS_DPRE2),
h_1 .. h_L (NCX_WS_H*), the block dGt | dGgt (NCX_WS_DGT), dscores.  A product returns (g_ref, S, extra, n): the exact fp64 result, the
magnitude sum S of the products each element is made of, a further absolute term in units of 2^-24 (zero except for the dist column) and
the number n of terms of the reduction.  With x[r] the candidate row and xs[b] the shared row of MainFwdRef (main_fwd_ref.py):

  a  dW1[:, v_other] = dpre1^T . v_k        dW1[:, v_mult] = dpre1^T . (v_o * v_k)      S = |dpre1|^T . |x|; v_mult lesion: exactly zero
  b  dW1[:, v_dist | v_rank] = dpre1^T . [dist, one-hot rank]                          S likewise, + the dist term below
  c  dW1[:, z_other] = dpre1^T . z_k
  d  dGt = dpre1^T . softmax(a_k)  [H, A]   (a_emb lesion: dW1[:, a_other] = dpre1^T . a_knns)
  e  dSh[b] = sum_k dpre1[bK + k];  dW1[:, v_orig | q_emb | z_orig | a_emb_gt] = dSh^T . xs,   S = (sum_k |dpre1|)^T . |xs|  (n = B K terms:
     the two stages are one sum of B K products);  dGgt[:, a] = sum over {b: aid[b] = a} of dSh[b],  S = the same sum of sum_k |dpre1|
  f  from the DEVICE's block:  dW1[:, a_other] = dGt . E  (n = A)    dE = dGt^T . W1[:, a_other] + dGgt^T . W1[:, a_gt]  (n = 2 H)
  g  d linear_1.bias = colsum(dpre1),  d linear_2.bias = colsum(dpre2)                 S = colsum |dpre|
  h  dpre_L[r, n] = dscores[r] * w_out[n] * gate,  gate = 1 / (1 - p) where the device's h_L[r, n] > 0, else 0 (eval: p = 0)
     d out.weight = dscores^T . h_L,  S = |dscores|^T . |h_L|;   d out.bias = sum dscores,  S = sum |dscores|
  i  L = 2, from the device's dpre_2 and h_1:  dW_2 = dpre2^T . h_1;   dpre_1 = (dpre2 . W_2) * gate(h_1),  S = (|dpre2| . |W_2|) * gate

The bound    |g_dev - g_ref| <= 2^-24 * (c * S + extra)   element by element, ragged edges included.
  Reductions (everything but dpre_L): c = min(C_MARGIN x YARDSTICK[group], n + 2).  Any order of a sum of n products is within
  n * 2^-24 * S of the exact sum to first order (+ 2: the operand's own rounding in v_o * v_k, the gate's factor in i), so c < n always holds
  for a correct kernel and the constant only ever tightens that.  YARDSTICK is measured on the CPU, never on the kernels: the larger, over the
  group's cases, of max |g32 - g_ref| / (2^-24 S) for (1) torch float32 on one thread and (2) a plain float32 accumulation of the same products
  with the running sum updated one row of the reduction at a time -- the least accurate order a kernel that accumulates along k can
  legitimately take (splitting into chunks only improves on it; torch's blocked matmul is several times closer to fp64, so a bound set from it
  alone fails a correct kernel).  Both take the float32 inputs the device would be handed and form the operand (v_o * v_k, the softmax, the
  distance) in float32 too.  The margin C_MARGIN = 4 and its reasoning are those of profiles/loss_adam_edges.json and main_fwd_edges.json.
  dpre_L: no reduction.  fl(fl(dscores * w_out) * scale) is two roundings of the exact product, and the device's scale fl(1 / (1 - p)) a
  third in train mode:  |dpre_L - ref| <= (2 + [p > 0]) * 2^-24 * |ref| (1 + 2^-22) + 2^-149, stated, not measured; a gated element is exactly 0.
  dpre_1 of i: the gate's factor multiplies the finished sum: one more rounding, |.| <= S, so its c is the group's + 1.
  The dist term.  The restatement's dist is exact; the kernel's is sqrtf of a float32 sum of dv squares t^2, t = fl(fl(v_o - v_k) + 1e-6f):
  |dt| <= 2^-24 (|v_o - v_k| + |t| + 1e-6) <= 2^-23 (|t| + 1e-6) (two roundings, and the constant's own), t^2 another rounding, the sum of dv
  terms in any order (dv - 1) more, sqrtf at most 2: dist_dev = dist (1 + e 2^-24) with
      e <= ((dv - 1) + 1 + 4 (1 + 1e-6 sum |t| / sum t^2)) / 2 + 2
  per row, so the v_dist column gets extra[n] = sum_r |dpre1[r, n]| dist[r] e[r].  (dv - 1 holds for either kernel that computes the
  distance, k_prep and the fused forward kernel, whatever its lane partition.)

The X6 forms (NCX_F_X6) are held to the same c, and per product to the suite's fp32-grade rule: worst ratio <= 1.5 x the fp32 form's on the
same case + 1 (x6_rule), in units of 2^-24 S.  A lost plane product leaves a per-term error near 2^-17 with random sign, about 12 in these
units at M = 312 and under 3 at M = 6144: the forms run at their smallest shapes.
"""
import contextlib

import numpy as np
import torch

import main_fwd_ref as R
from helpers import condition_away_from_kinks
from main_fwd_ref import C_MARGIN, U24, MainFwdRef, _f64
from oracle import ncx_oracle as orc

TAU = 2e-5
# The larger of the two CPU ratios (torch float32 on one thread; float32 in row order) over the group's cases, rounded up, on the host that
# wrote profiles/main_bwd_edges.json.  test_recorded_yardsticks_reproduce asks another host for the same size (a factor of three): its BLAS
# blocks otherwise; the row-order figure does not depend on the host.  The kernels' c = C_MARGIN x this does not move.
YARDSTICK = {"a": 12.0, "b": 9.0, "c": 10.1, "d": 25.2, "e": 4.4, "f": 8.7, "g": 4.2, "h": 4.0, "i": 8.5}
GROUP_OF = {"v_other": "a", "v_mult": "a", "v_dist": "b", "v_rank": "b", "z_other": "c", "dGt": "d", "a_other_lesion": "d",
            "v_orig": "e", "q_emb": "e", "z_orig": "e", "a_emb_gt": "e", "dGgt": "e", "a_other": "f", "dE": "f",
            "b1": "g", "b2": "g", "w_out": "h", "b_out": "h", "w2": "i", "dpre1": "i"}
GROUPS = sorted(YARDSTICK)


def bound_c(name, n):
    """The constant of product `name` at a reduction of n terms."""
    c = C_MARGIN * YARDSTICK[GROUP_OF[name]] + (1.0 if name == "dpre1" else 0.0)
    return min(c, n + 2.0)


def x6_rule(ratio_x6, ratio_fp32):
    return ratio_x6 <= 1.5 * ratio_fp32 + 1.0


def ratio(got, ref, S, extra=0.0):
    """max (|got - ref| - 2^-24 extra) / (2^-24 S) over the elements: what the bound compares with c.  An element whose S is 0 must be exact."""
    err = np.abs(_f64(got).reshape(ref.shape) - ref)
    S = np.broadcast_to(S, ref.shape)
    assert (err[S == 0] == 0).all(), "an element made of no products is not exactly zero"
    if not (S > 0).any():
        return 0.0
    err = np.maximum(err - U24 * np.broadcast_to(extra, ref.shape), 0.0)
    return float((err[S > 0] / (U24 * S[S > 0])).max())


def _tsum(a, b):
    return a.T @ b


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
class MainBwdRef:
    """fp64 restatement of the backward's products on one case.  fwd: the case's MainFwdRef (its candidate row x, shared row xs, dist)."""

    def __init__(self, fwd, params, batch):
        self.f, self.d, self.spec, self.B, self.M = fwd, fwd.d, fwd.spec, fwd.B, fwd.M
        d = self.d
        self.scale = 1.0 / (1.0 - fwd.p) if fwd.masks is not None else 1.0
        self.training = fwd.masks is not None and fwd.p > 0
        self.W1 = _f64(params["linear_1.weight"])
        self.E = _f64(params["answer_embedding.weight"])
        self.w_out = _f64(params["out.weight"]).reshape(-1)
        self.params = params
        self.aid = np.asarray(batch["answer_aids"]).astype(np.int64)
        # the column blocks of the candidate row x, in MainFwdRef's order, and of the shared row xs
        cols, o = [], 0
        for name, w in (("v_other", d.dv), ("v_mult", d.dv if self.spec["v_mult"] else 0), ("v_dist", 1), ("v_rank", d.K), ("z_other", d.dz),
                        ("dGt" if self.spec["a_emb"] else "a_other_lesion", d.A if self.spec["a_emb"] else d.da)):
            cols.append((name, o, w)); o += w
        assert o == fwd.x.shape[1]
        self.cand_cols = cols
        self.shared_cols, o = [], 0
        for name, w in (("v_orig", d.dv), ("q_emb", d.dq), ("z_orig", d.dz), ("a_emb_gt", d.da)):
            self.shared_cols.append((name, o, w)); o += w
        self.offsets = d.offsets()
        # the distance's own error, per row, in units of 2^-24 dist (docstring)
        if self.spec["v_dist"]:
            feats = _f64(batch["image_features"])
            t = np.abs(feats[:, :1] - feats[:, 1:] + 1e-6).reshape(self.M, d.dv)
            self.dist_e = ((d.dv - 1) + 1 + 4 * (1 + 1e-6 * t.sum(1) / np.maximum((t * t).sum(1), 1e-300))) / 2 + 2
        else:
            self.dist_e = np.zeros(self.M)

    # a .. e, g: everything made from dpre_1
    def from_dpre1(self, dpre1):
        """dpre1 [B K, H] (the device's) -> {name: (ref, S, extra, n)} for the column blocks of dW1 that are reductions over rows (names of
        orc.Dims.offsets, a_other under the a_emb lesion as "a_other_lesion"), "dGt" and "dGgt" ([H, A]) and "b1"."""
        d, x, xs = self.d, self.f.x, self.f.xs
        g, ga = _f64(dpre1), np.abs(_f64(dpre1))
        out = {}
        ref, S = _tsum(g, x), _tsum(ga, np.abs(x))
        for name, o, w in self.cand_cols:
            if w:
                extra = _tsum(ga, (self.f.dist * self.dist_e)[:, None]) if name == "v_dist" else 0.0
                out[name] = (ref[:, o: o + w], S[:, o: o + w], extra, self.M)
        dsh, dsha = g.reshape(self.B, d.K, d.H).sum(1), ga.reshape(self.B, d.K, d.H).sum(1)
        ref, S = _tsum(dsh, xs), _tsum(dsha, np.abs(xs))
        for name, o, w in self.shared_cols:
            out[name] = (ref[:, o: o + w], S[:, o: o + w], 0.0, self.M)
        if self.spec["a_emb"]:
            hot = np.zeros((self.B, d.A)); hot[np.arange(self.B), self.aid] = 1.0
            out["dGgt"] = (_tsum(dsh, hot), _tsum(dsha, hot), 0.0, int(hot.sum(0).max()) * d.K)
        out["b1"] = (g.sum(0), ga.sum(0), 0.0, self.M)
        return out

    # f: from the block
    def from_block(self, dgt, dggt):
        """dgt, dggt [H, A] (the device's block, read in the layout the header documents) -> "a_other" [H, da], "dE" [A, da]."""
        o, d = self.offsets, self.d
        wak, wagt = self.W1[:, o["a_emb_other"]: o["a_emb_other"] + d.da], self.W1[:, o["a_emb_gt"]: o["a_emb_gt"] + d.da]
        g, gg = _f64(dgt), _f64(dggt)
        return {"a_other": (g @ self.E, np.abs(g) @ np.abs(self.E), 0.0, d.A),
                "dE": (_tsum(g, wak) + _tsum(gg, wagt), _tsum(np.abs(g), np.abs(wak)) + _tsum(np.abs(gg), np.abs(wagt)), 0.0, 2 * d.H)}

    # h: the out layer
    def from_dscores(self, dscores, h_last):
        """dscores [B, K], h_last [B K, H] (the device's) -> "dpreL": (ref, absolute tolerance), "w_out", "b_out"."""
        ds, h = _f64(dscores).reshape(-1), _f64(h_last)
        ref = ds[:, None] * self.w_out[None, :] * self.scale * (h > 0)
        tol = (3 if self.training else 2) * U24 * np.abs(ref) * (1 + 2.0 ** -22) + 2.0 ** -149
        return {"dpreL": (ref, tol), "w_out": (ds @ h, np.abs(ds) @ np.abs(h), 0.0, self.M), "b_out": (ds.sum(keepdims=True), np.abs(ds).sum(keepdims=True), 0.0, self.M)}

    # i (and g's b2): a hidden layer
    def from_dpre(self, l, dpre_l, h_prev):
        """Layer l >= 2, from the dpre_l and h_{l-1} given -> "w%d", "b%d", and "dpre%d" of the layer below."""
        g, h = _f64(dpre_l), _f64(h_prev)
        W = _f64(self.params["linear_%d.weight" % l])
        gate = self.scale * (h > 0)
        return {"w%d" % l: (_tsum(g, h), _tsum(np.abs(g), np.abs(h)), 0.0, self.M),
                "b%d" % l: (g.sum(0), np.abs(g).sum(0), 0.0, self.M),
                "dpre%d" % (l - 1): ((g @ W) * gate, (np.abs(g) @ np.abs(W)) * gate, 0.0, self.d.H)}

    def assemble(self, parts):
        """{name: ref ...} of from_dpre1 + from_block -> linear_1.weight's gradient [H, din] (the v_mult lesion's block stays zero)."""
        d, o = self.d, self.offsets
        g = np.zeros((d.H, d.din))
        width = dict(v_orig=d.dv, v_other=d.dv, v_mult=d.dv, v_dist=1, v_rank=d.K, q_emb=d.dq, z_orig=d.dz, z_other=d.dz, a_emb_gt=d.da, a_emb_other=d.da)
        for name, w in width.items():
            src = {"a_emb_other": "a_other" if self.spec["a_emb"] else "a_other_lesion"}.get(name, name)
            if src in parts:
                g[:, o[name]: o[name] + w] = parts[src][0]
        return g

    def whole(self, gt):
        """The whole backward on the restatement's own values (nothing of a device): {state_dict name: gradient} in float64."""
        d, ch = self.d, self.f.chain()
        s = ch["scores"]
        e = np.exp(s - s.max(1, keepdims=True))
        ds = e / e.sum(1, keepdims=True)
        ds[np.arange(self.B), np.asarray(gt).astype(np.int64)] -= 1.0
        ds /= self.B
        out = {}
        top = self.from_dscores(ds, ch["h"][-1])
        out["out.weight"], out["out.bias"] = top["w_out"][0].reshape(1, -1), top["b_out"][0]
        dpre = top["dpreL"][0]
        for l in range(d.L, 1, -1):
            p = self.from_dpre(l, dpre, ch["h"][l - 2])
            out["linear_%d.weight" % l], out["linear_%d.bias" % l] = p["w%d" % l][0], p["b%d" % l][0]
            dpre = p["dpre%d" % (l - 1)][0]
        parts = self.from_dpre1(dpre)
        out["linear_1.bias"] = parts["b1"][0]
        if self.spec["a_emb"]:
            parts.update(self.from_block(parts["dGt"][0], parts["dGgt"][0]))
            out["answer_embedding.weight"] = parts["dE"][0]
        else:
            out["answer_embedding.weight"] = np.zeros((d.A, d.da))
        out["linear_1.weight"] = self.assemble(parts)
        self.last_dpre1, self.last_dscores, self.last_chain = dpre, ds, ch
        return out


# ---- the CPU yardstick -------------------------------------------------------------------------------------------------------------------
@contextlib.contextmanager
def one_thread():
    n = torch.get_num_threads()
    torch.set_num_threads(1)             # (the BLAS behind torch picks its blocking, hence its summation order, by the thread count)
    try:
        yield
    finally:
        torch.set_num_threads(n)


def f32(a):
    return np.ascontiguousarray(np.asarray(a, dtype=np.float64).astype(np.float32))


def row_order(A, X, acc=None):
    """sum_r A[r, :]^T X[r, :] in float32, the running sum updated one row r at a time: acc <- fl(acc + fl(A[r, i] X[r, j]))."""
    A, X = np.asarray(A, np.float32), np.asarray(X, np.float32)
    acc = np.zeros((A.shape[1], X.shape[1]), np.float32) if acc is None else acc
    tmp = np.empty_like(acc)
    for r in range(A.shape[0]):
        np.multiply(A[r][:, None], X[r][None, :], out=tmp)
        acc += tmp
    return acc


def torch32(A, X):
    return (torch.from_numpy(np.asarray(A, np.float32)).T @ torch.from_numpy(np.asarray(X, np.float32))).numpy()


def operands32(fwd, batch):
    """The candidate row and the shared row formed in float32 from the float32 inputs (what a kernel can know): v_o * v_k, the softmax and
    the distance in torch float32; the gathers are exact."""
    d, spec = fwd.d, fwd.spec
    feats = batch["image_features"].float()
    v_o, v_k = feats[:, :1], feats[:, 1:]
    xc = [v_k]
    if spec["v_mult"]:
        xc.append(v_o * v_k)
    if spec["v_dist"]:
        dist = torch.nn.functional.pairwise_distance(v_o.expand_as(v_k).reshape(-1, d.dv), v_k.reshape(-1, d.dv)).reshape(fwd.B, d.K, 1)
    else:
        dist = torch.zeros(fwd.B, d.K, 1)
    o = d.dv * len(xc) + 1
    rank = torch.from_numpy(f32(fwd.x[:, o: o + d.K])).reshape(fwd.B, d.K, d.K)                   # (0 / 1, or the lesion's float32 input: exact)
    xc += [dist, rank, batch["z_knns"].float(), torch.softmax(batch["a_knns"].float(), -1) if spec["a_emb"] else batch["a_knns"].float()]
    return torch.cat(xc, -1).reshape(fwd.M, -1).numpy(), f32(fwd.xs)


def yardstick(case):
    """-> {group: (torch float32 ratio, row-order float32 ratio)} of one case: every product from the float32 roundings of the
    restatement's own dpre, h and block (correct inputs), computed both ways and judged like a kernel's result (extra term included)."""
    d, params, batch, spec, masks = build(case)
    fwd = MainFwdRef(params, d, batch, spec, case["p"], masks)
    ref = MainBwdRef(fwd, params, batch)
    ref.whole(batch["gt"])
    out = {g: [0.0, 0.0] for g in GROUPS}

    def judge(name, prod, g_torch, g_row):
        r, S, extra, n = prod
        for i, g in enumerate((g_torch, g_row)):
            out[GROUP_OF[name]][i] = max(out[GROUP_OF[name]][i], ratio(g, r, S, extra))

    with one_thread():
        ds, hL = f32(ref.last_dscores), f32(ref.last_chain["h"][-1])
        top = ref.from_dscores(ds, hL)
        judge("w_out", top["w_out"], torch32(ds.reshape(-1, 1), hL), row_order(ds.reshape(-1, 1), hL))
        judge("b_out", top["b_out"], torch.from_numpy(ds).sum().numpy(), np.cumsum(ds.reshape(-1), dtype=np.float32)[-1:])
        dpre = f32(top["dpreL"][0])
        for l in range(d.L, 1, -1):
            hp, W = f32(ref.last_chain["h"][l - 2]), params["linear_%d.weight" % l].numpy()
            p = ref.from_dpre(l, dpre, hp)
            gate = (np.float32(ref.scale) * (hp > 0)).astype(np.float32)
            if l == 2:
                judge("w2", p["w2"], torch32(dpre, hp), row_order(dpre, hp))
                judge("b2", p["b2"], torch.from_numpy(dpre).sum(0).numpy(), row_order(dpre, np.ones((len(dpre), 1), np.float32))[:, 0])
                judge("dpre1", p["dpre1"], torch32(dpre.T, W) * gate, row_order(dpre.T, W) * gate)
            dpre = f32(p["dpre%d" % (l - 1)][0])
        parts = ref.from_dpre1(dpre)
        xc, xs = operands32(fwd, batch)
        g_t, g_r = torch32(dpre, xc), row_order(dpre, xc)
        for name, o, w in ref.cand_cols:
            if w:
                judge(name, parts[name], g_t[:, o: o + w], g_r[:, o: o + w])
        # the shared part in two stages, as the kernels take it: dSh over the K rows of a triplet, then the product over the B triplets
        dsh_t = torch.from_numpy(dpre).reshape(fwd.B, d.K, d.H).sum(1).numpy()
        dsh_r = np.zeros((fwd.B, d.H), np.float32)
        for k in range(d.K):
            dsh_r += dpre.reshape(fwd.B, d.K, d.H)[:, k]
        g_t, g_r = torch32(dsh_t, xs), row_order(dsh_r, xs)
        for name, o, w in ref.shared_cols:
            judge(name, parts[name], g_t[:, o: o + w], g_r[:, o: o + w])
        judge("b1", parts["b1"], torch.from_numpy(dpre).sum(0).numpy(), row_order(dpre, np.ones((len(dpre), 1), np.float32))[:, 0])
        if fwd.spec["a_emb"]:
            hot = np.zeros((fwd.B, d.A), np.float32); hot[np.arange(fwd.B), ref.aid] = 1
            judge("dGgt", parts["dGgt"], torch32(dsh_t, hot), row_order(dsh_r, hot))
            dgt, dggt = f32(parts["dGt"][0]), f32(parts["dGgt"][0])
            blk = ref.from_block(dgt, dggt)
            o = ref.offsets
            W1 = params["linear_1.weight"].numpy()
            wak, wagt = W1[:, o["a_emb_other"]: o["a_emb_other"] + d.da], W1[:, o["a_emb_gt"]: o["a_emb_gt"] + d.da]
            E = params["answer_embedding.weight"].numpy()
            judge("a_other", blk["a_other"], torch32(dgt.T, E), row_order(dgt.T, E))
            judge("dE", blk["dE"], torch32(dgt, wak) + torch32(dggt, wagt), row_order(dggt, wagt, row_order(dgt, wak)))
    return {g: tuple(v) for g, v in out.items()}


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# The smallest shapes at which each form of the weight gradient still runs, from what the suite shows to select them (test_hip_parity,
# test_backward_routes_gpu).  fold / tn: the route the case must report (ncx_plan_query NCX_QUERY_DW1_ROUTE), in the vocabulary of
# test_backward_routes_gpu.expect; it is part of the id.  env: experiment hooks (with NCX_EXPERIMENT=1, set before the workspace is sized).
# emb_nt: the answer-embedding gradient's route (ncx_plan.hip: a_emb && !NCX_NO_EMB_NT; the planner has no query for it, the layout of
# the NCX_WS_DGT block follows it: dGt^T | dGgt^T, 2 x [A][pad4(H)], else dGt | dGgt, 2 x [H][A]).
CASES = []
KM = {"NCX_KM_FORCE": "1"}


def _case(tag, fold, tn, env=None, lesion=None, drop=None, p=0.0, neardup=False, **over):
    c = dict(K=24, dq=64, dz=24, da=orc.Dims().da, A=40, L=1)
    c.update(over)
    env = dict(env or {})
    c.update(id="%s-%s-%s" % (fold, tn, tag), fold=fold, tn=tn, env=env, lesion=lesion, drop=drop, p=p, neardup=neardup,
             emb_nt=(lesion != "no_a_emb") and "NCX_NO_EMB_NT" not in env)
    CASES.append(c)
    return c


# the fold forms, forced: (B, K, H, L, dv) of the 8-wave kernels (k_dw_km8; under NCX_F_X6 k_dw_km_x6) and of the general k_dw_km
for B, K, H, L, dv in ((1, 24, 256, 1, 64), (7, 24, 256, 2, 128), (13, 48, 256, 1, 192), (37, 24, 512, 1, 64)):
    _case("B%d-K%d-H%d-L%d-dv%d" % (B, K, H, L, dv), "fold8", "grouped", env=KM, B=B, K=K, H=H, L=L, dv=dv, dq=50, dz=18, A=45)
for B, K, H, L, dv in ((1, 24, 16, 1, 70), (7, 24, 20, 2, 64), (13, 48, 48, 1, 130), (40, 24, 200, 1, 96)):
    _case("B%d-K%d-H%d-L%d-dv%d" % (B, K, H, L, dv), "km", "grouped", env=KM, B=B, K=K, H=H, L=L, dv=dv, dq=50, dz=18, A=45)
# the balanced TN launch (k_dw_tn8; under NCX_F_X6 k_dw_tn8_x6), dv = 96, dq = 64, dz = 24, A = 40
TNW = dict(dv=96, dq=64, dz=24)
_case("B128-H256", "grouped", "tn8", B=128, H=256, **TNW)
_case("B160-H256-ragged-chunks", "grouped", "tn8", B=160, H=256, **TNW)
_case("B128-H512-L2", "grouped", "tn8", B=128, H=512, L=2, **TNW)
_case("B128-K48", "grouped", "tn8", B=128, K=48, H=256, **TNW)
_case("B128-no_a_emb", "grouped", "tn8", lesion="no_a_emb", B=128, H=256, **TNW)
_case("B128-no_v_mult", "grouped", "tn8", lesion="no_v_mult", B=128, H=256, **TNW)
_case("B128-dropout-rng", "grouped", "tn8", drop="rng", p=0.25, B=128, H=256, **TNW)
# A = 33 is one column past a 32-column tile of dGt, but no multiple of 4: the TN launch takes whole 16-byte windows, so the planner keeps
# this shape on the grouped GEMM (asserted); A = 36 is the first width past the tile that the TN launch takes; A = 200 is several tiles
_case("B128-A33", "grouped", "grouped", B=128, H=256, A=33, **TNW)
_case("B128-A36", "grouped", "tn8", B=128, H=256, A=36, **TNW)
_case("B128-A200", "grouped", "tn8", B=128, H=256, A=200, **TNW)
# neighbours that nearly equal the original image (v_k = v_o + 5e-4 N(0, 1)): the one place where the 1e-6 inside the distance shows
_case("B128-near-duplicates", "grouped", "tn8", neardup=True, B=128, H=256, **TNW)
# the grouped and chain GEMMs
_case("B96", "grouped", "grouped", B=96, H=256, dv=64, dq=64, dz=64, da=64)
for B, H in ((7, 20), (33, 96)):
    _case("ragged-B%d-H%d-L2" % (B, H), "grouped", "grouped", B=B, H=H, L=2, dv=70, dq=50, dz=18, A=45)
SPLIT_GIDS = (0, 1, 4, 6, 7, 9)                      # Gt, Sh, grouped dW1, dE, dW1ak, dW_l (test_forced_split_k_layouts_vs_oracle)
for S in (3, 8):
    _case("split%d-B44-H128-L2" % S, "grouped", "grouped", env={"NCX_SPLIT_%d" % g: str(S) for g in SPLIT_GIDS}, B=44, H=128, L=2, dv=70, dq=50, dz=18, A=45)
_case("B96-no-emb-nt", "grouped", "grouped", env={"NCX_NO_EMB_NT": "1"}, B=96, H=256, dv=64, dq=64, dz=64, da=64)
_case("ragged-B33-H96-L2-no-emb-nt", "grouped", "grouped", env={"NCX_NO_EMB_NT": "1"}, B=33, H=96, L=2, dv=70, dq=50, dz=18, A=45)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
# where the planted errors of test_main_bwd_edges_cpu.py are judged: M = 13 x 24 = 312 rows (the lost plane's 2^-17 shrinks like 1 / sqrt(M))
PLANTED = dict(BY_ID["fold8-grouped-B1-K24-H256-L1-dv64"], id="planted-B13", B=13)
PLANTED_NEARDUP = dict(PLANTED, id="planted-B13-near-duplicates", neardup=True)


def shape_key(c):
    return R.shape_key(c) + (c["neardup"],)


_BUILT = {}


def build(c):
    """-> (orc.Dims, params, batch, spec or None, keep masks or None) of a case, built once per shape and never modified: main_fwd_ref.build's
    inputs (seeded by the shape, one duplicated answer id), conditioned away from the ReLU kinks of every layer (helpers, tau = 2e-5).  Under
    the v_mult lesion the helper conditions the unlesioned network; nothing below depends on it, every product being judged from the
    device's own gates.  The dropout case has L = 1, where pre_1 does not depend on the mask."""
    key = shape_key(c)
    if key not in _BUILT:
        d, params, batch, spec, masks = R.build(c)
        seed = int(batch["answer_aids"].sum()) + 7 * c["B"]
        if c["neardup"]:
            rng = np.random.default_rng(seed)
            f = batch["image_features"]
            f[:, 1:] = f[:, :1] + torch.from_numpy((5e-4 * rng.standard_normal(tuple(f[:, 1:].shape))).astype(np.float32))
        assert not masks or d.L == 1
        for _ in range(10):
            condition_away_from_kinks(params, d, batch, seed, tau=TAU, spec=spec)
            if c["B"] == 1 or batch["answer_aids"][0] == batch["answer_aids"][c["B"] - 1]:
                break
            batch["answer_aids"][0] = batch["answer_aids"][c["B"] - 1]       # (a redraw took the duplicate away: put it back, check again)
        else:
            raise AssertionError("could not keep a duplicated answer id on a conditioned batch")
        _BUILT[key] = (d, params, batch, spec, masks)
    return _BUILT[key]
