"""The bf16 variant (NCX_F_BF16: csrc/ncx_bf16.hip and the pack branch of k_prep, csrc/ncx_forward.hip) product by product: the expected
bit patterns of the packed operands, an fp64 restatement of every bf16 product with a per-element bound, the CPU yardstick the bound's
constants come from, and the table of cases.  Plain numpy / torch; tests/test_bf16_edges_cpu.py checks what this file claims,
tests/test_bf16_edges_gpu.py runs the kernels.  U24, C_MARGIN, _f64, ratio, the shared part of linear_1 (MainFwdRef) and the products of the
fp32 groups e, g, h, i (MainBwdRef) are main_fwd_ref's and main_bwd_ref's, imported.

Why the variant admits a sharper test than the fp32 path.  A product of two bf16 values (8-bit significands) is exact in fp32, so GIVEN the
operands the device packed, the only error left in a bf16 product is the order of its fp32 accumulation.  The packed operands themselves are
checked bit for bit (the column layout is the library's: ncx_bf16_layout, never restated here), and each product is then judged alone from
the device's own operand bits against the exact fp64 sum.  "RNE" is round-to-nearest-even to bf16 (rne_bits).

Operands (Bf16Ref.xc_bounds, wc_expected).  Bit-exact: v_k = RNE(features); v_o * v_k = RNE of the ONE float32 product; the rank one-hot;
z_k; the zeros of every gap up to the next multiple of 8 and of the columns raw .. kc; Wc's W1 slices = RNE(host weights), its Gt columns =
RNE(the device's own fp32 Gt, NCX_WS_GT), its padding rows H .. Hp and columns.  Device-computed (k_prep: sqrtf, __expf, __log2f, exp2f): for
the fp64 value x and a relative half-width tau the device's bf16 must lie in [RNE(x (1 - tau)), RNE(x (1 + tau))]; where the two ends
coincide that is a bit-exact check too ("unambiguous").
  tau_dist[r] = e[r] 2^-24, the e of main_bwd_ref.py, "The dist term" (MainBwdRef.dist_e).
  TAU_SOFT: the kernel's formula restated in float32 -- row max m, s = sum exp(a - m), lse2 = m log2e + log2(s), exp2(fma(a, log2e, -lse2))
  (softmax32) -- deviates from the fp64 softmax by at most SOFT32_DEV (relative, the worst over every case's inputs, measured on the CPU by
  tau_soft_measure, never on a kernel); TAU_SOFT = C_MARGIN x that, the margin and the reasoning of the other yardsticks.  Its size is
  explained by the exponent's roundings: lse2 and a log2e - lse2, each below 32 in magnitude, carry an absolute float32 error of up to 2^-20
  apiece, i.e. 2 ln 2 x 2^-20 = 22 x 2^-24 relative after exp2, whichever library evaluates exp2; the measured worst is 24.7.
Caps, conditions on the INPUTS (from the fp64 reference alone): no dist element of a case is ambiguous (build redraws such triplets); at
most SOFT_AMBIGUOUS_CAP = 2 % of a case's softmax elements are (the expected share is about 512 tau: bf16 neighbours are 2^-8 .. 2^-7 apart).

Products: (ref, S, extra = 0, n) as in main_bwd_ref.py; S the sum of the operand magnitudes' products, n the reduction length.
  p  Gt = RNE(W1ak) . RNE(E)^T                         operands: host weights                                   n = da
  q  h_1 = epilogue(Sh[b] + Xc . Wc^T)                 the device's Xc, Wc bits; Sh and its share of S as MainFwdRef  n = raw + dv + dq + dz + da + 1
  r  dWc = RNE(dpre_1)^T . Xc                          the device's dpre_1 (NCX_WS_DPRE1) and Xc                 n = B K
     read back as dW1[:, v_other | v_mult | v_dist | v_rank | z_other] and dGt (NCX_WS_DGT: dGt | dGgt, 2 x [H][A]).  No dist term:
     the operand is the device's own.
  s  dW1[:, a_other] = RNE(dGt) . RNE(E)               the device's dGt                                         n = A
  t  dE = RNE([dGt; dGgt])^T . RNE([W1ak; W1agt])      the device's block                                       n = 2 H
The fp32 products the variant keeps (the shared segments' gradient, dGgt, the biases, dpre_L, the out layer, dW_2 and dpre_1 at L = 2:
groups e, g, h, i) and the hidden layers l > 1 (MainFwdRef.layer on the device's h_{l-1}) are main_bwd_ref's and main_fwd_ref's, unchanged,
with their recorded constants (hidden layers: main_fwd_ref's group H, with dropout its group I).

The bound    |got - ref| <= 2^-24 c S   element by element; S = 0: exactly zero.   c = min(C_MARGIN x YARDSTICK[group], n + 2): any order of a
sum of n exact products is within n 2^-24 S of it to first order.  YARDSTICK is measured on the CPU exactly as main_bwd_ref.py defines it
(the larger of torch float32 on one thread and a float32 accumulation one reduction row at a time, of the same exact bf16 products, over the
group's cases, rounded up), from ideal operands: the restatement's own values rounded to bf16.  Never from a kernel's output.

Rows.  M = B K with 3 <= K <= 64 (ncx_forward's limits), so the primes 191 and 193 are no row counts of this model: the 192-row kernel runs at
M = 189 (63 x 3), 192 (64 x 3) and 195 (65 x 3), one row tile three short, one full, two with the second three rows deep.
"""
import numpy as np
import torch

import main_bwd_ref as Bw
import main_fwd_ref as R
from helpers import condition_away_from_kinks, random_case_f32
from main_bwd_ref import f32, one_thread, row_order, torch32
from main_fwd_ref import C_MARGIN, U24, MainFwdRef, _f64
from oracle import ncx_oracle as orc

ratio = Bw.ratio
# tau_soft_measure's worst relative deviation over the table, in units of 2^-24, rounded up, on the host that wrote profiles/bf16_edges.json
SOFT32_DEV_U24 = 25.0
TAU_SOFT = C_MARGIN * SOFT32_DEV_U24 * U24
SOFT_AMBIGUOUS_CAP = 0.02
# The larger CPU ratio (torch float32 on one thread; float32 in row order) over every case, rounded up, on the same host; see main_bwd_ref.YARDSTICK
YARDSTICK = {"p": 2.1, "q": 7.2, "r": 7.6, "s": 6.8, "t": 1.9}
GROUP_OF = {"Gt": "p", "h1": "q", "v_other": "r", "v_mult": "r", "v_dist": "r", "v_rank": "r", "z_other": "r", "dGt": "r", "a_other": "s", "dE": "t"}
GROUPS = sorted(YARDSTICK)
BF16_SEGMENTS = ("v_other", "v_mult", "v_dist", "v_rank", "z_other", "dGt")
LOG2E = np.float32(1.44269504088896341)


def bound_c(name, n):
    """The constant of product `name` at a reduction of n terms: this file's groups, else main_bwd_ref's."""
    if name in GROUP_OF:
        return min(C_MARGIN * YARDSTICK[GROUP_OF[name]], n + 2.0)
    return Bw.bound_c(name, n)


# ---- bf16 ---------------------------------------------------------------------------------------------------------------------------------
def rne_bits(x):
    """float32 / float64 array -> uint16 bit patterns of the nearest bf16, ties to even (subnormals kept, overflow to infinity), in ONE
    rounding from the value given: the spacing of bf16 around x is 2^(max(e, -125) - 8) for x = m 2^e, 1/2 <= |m| < 1."""
    x = np.asarray(x, np.float64)
    _, e = np.frexp(x)
    ulp = np.ldexp(1.0, np.maximum(e, -125) - 8)
    with np.errstate(over="ignore"):
        v = (np.rint(x / ulp) * ulp).astype(np.float32)            # (a bf16 value: exact in float32; rint rounds halves to even)
    return (v.view(np.uint32) >> np.uint32(16)).astype(np.uint16)


def bf_val(bits):
    """uint16 (or int16) bf16 bit patterns -> float64 values."""
    b = np.ascontiguousarray(bits).view(np.uint16).astype(np.uint32) << np.uint32(16)
    return b.view(np.float32).astype(np.float64)


def bfr(x):
    """x rounded to bf16, as float64."""
    return bf_val(rne_bits(x))


def softmax32(a):
    """The softmax row as k_prep forms it, in float32 numpy: m = max, s = sum exp(a - m), lse2 = m log2e + log2(s), exp2(fma(a, log2e, -lse2))."""
    a = np.asarray(a, np.float32)
    m = a.max(-1, keepdims=True)
    s = np.exp(a - m, dtype=np.float32).sum(-1, keepdims=True, dtype=np.float32)
    lse2 = (m * LOG2E + np.log2(s, dtype=np.float32)).astype(np.float32)
    arg = (a.astype(np.float64) * np.float64(LOG2E) - lse2.astype(np.float64)).astype(np.float32)       # (the fma: one rounding)
    return np.exp2(arg, dtype=np.float32)


def softmax64(a):
    a = _f64(a)
    e = np.exp(a - a.max(-1, keepdims=True))
    return e / e.sum(-1, keepdims=True)


def tau_soft_measure(case):
    """Worst relative deviation of softmax32 from the fp64 softmax over a case's logits, in units of 2^-24."""
    a = build(case)[2]["a_knns"].numpy()
    x = softmax64(a)
    return float((np.abs(softmax32(a).astype(np.float64) - x) / x).max() / U24)


# ---- the restatement ---------------------------------------------------------------------------------------------------------------------
def ncx_dims(c):
    """The library's dims of a case (host only: for ncx_bf16_layout and the plan query)."""
    from neuralcx import _lib
    return _lib.NcxDims(B=c["B"], K=c["K"], dv=c["dv"], dq=c["dq"], dz=c["dz"], da=c["da"], A=c["A"], H=c["H"], L=c["L"],
                        n_img=c["B"] * (c["K"] + 1), flags=_lib.NCX_F_ALL | _lib.NCX_F_BF16)


def layout_of(c):
    from neuralcx import _lib
    return _lib.bf16_layout(ncx_dims(c))


class Bf16Ref:
    """One case: the expected operand bits and the fp64 products.  lay: the column layout, from the library (ops.bf16_layout)."""

    def __init__(self, params, d, batch, lay, drop_p=0.0, masks=None):
        self.d, self.lay, self.params = d, lay, params
        self.fwd = MainFwdRef(params, d, batch, None, drop_p, masks)
        self.bwd = Bw.MainBwdRef(self.fwd, params, batch)
        self.B, self.M = self.fwd.B, self.fwd.M
        feats = batch["image_features"].numpy().astype(np.float32)
        self.v_o = np.repeat(feats[:, 0], d.K, axis=0)                                        # [M, dv] float32
        self.v_k = feats[:, 1:].reshape(self.M, d.dv)
        self.z_k = batch["z_knns"].numpy().astype(np.float32).reshape(self.M, d.dz)
        self.soft = self.fwd.x[:, -d.A:]                                                      # fp64 softmax(a_k)
        self.tau_dist = self.bwd.dist_e * U24
        o = d.offsets()
        W1 = params["linear_1.weight"].numpy().astype(np.float32)
        self.W1 = W1
        self.w1ak, self.w1agt = W1[:, o["a_emb_other"]: o["a_emb_other"] + d.da], W1[:, o["a_emb_gt"]: o["a_emb_gt"] + d.da]
        self.E = params["answer_embedding.weight"].numpy().astype(np.float32)
        # (name, first packed column, first column of linear_1.weight, width) of the bf16 product's segments
        self.segments = (("v_other", lay["c_vk"], o["v_other"], d.dv), ("v_mult", lay["c_vm"], o["v_mult"], d.dv), ("v_dist", lay["c_misc"], o["v_dist"], 1),
                         ("v_rank", lay["c_misc"] + 1, o["v_rank"], d.K), ("z_other", lay["c_z"], o["z_other"], d.dz))
        assert o["v_rank"] == o["v_dist"] + 1
        self.n_h1 = lay["raw"] + d.dv + d.dq + d.dz + d.da + 1

    # -- operands
    def xc_bounds(self, tau_scale=1.0):
        """-> (lo, hi) uint16 [M][kc]: the device's Xc bits must lie in [lo, hi] (as uint16: the two-sided elements are positive).
        tau_scale = 0: the ideal operand, every element the RNE of its fp64 value."""
        d, L = self.d, self.lay
        lo = np.zeros((self.M, L["kc"]), np.uint16)
        lo[:, L["c_vk"]: L["c_vk"] + d.dv] = rne_bits(self.v_k)
        lo[:, L["c_vm"]: L["c_vm"] + d.dv] = rne_bits(np.multiply(self.v_o, self.v_k, dtype=np.float32))       # one float32 rounding, then RNE
        lo[np.arange(self.M), L["c_misc"] + 1 + np.arange(self.M) % d.K] = rne_bits(1.0)
        lo[:, L["c_z"]: L["c_z"] + d.dz] = rne_bits(self.z_k)
        hi = lo.copy()
        t = self.tau_dist * tau_scale
        lo[:, L["c_misc"]], hi[:, L["c_misc"]] = rne_bits(self.fwd.dist * (1 - t)), rne_bits(self.fwd.dist * (1 + t))
        t = TAU_SOFT * tau_scale
        lo[:, L["c_p"]: L["c_p"] + d.A], hi[:, L["c_p"]: L["c_p"] + d.A] = rne_bits(self.soft * (1 - t)), rne_bits(self.soft * (1 + t))
        assert L["c_p"] + d.A == L["raw"] <= L["kc"]
        return lo, hi

    def ambiguity(self):
        """-> (ambiguous dist elements, share of ambiguous softmax elements): conditions on the inputs, from the fp64 reference alone."""
        lo, hi = self.xc_bounds()
        L = self.lay
        soft = np.s_[:, L["c_p"]: L["c_p"] + self.d.A]
        return int((lo[:, L["c_misc"]] != hi[:, L["c_misc"]]).sum()), float((lo[soft] != hi[soft]).mean())

    def column_name(self, c):
        L, d = self.lay, self.d
        for name, c0, w in (("v_k", L["c_vk"], d.dv), ("v_o*v_k", L["c_vm"], d.dv), ("dist", L["c_misc"], 1), ("rank", L["c_misc"] + 1, d.K), ("z_k", L["c_z"], d.dz),
                            ("softmax / Gt", L["c_p"], d.A)):
            if c0 <= c < c0 + w:
                return "%s[%d]" % (name, c - c0)
        return "padding beyond raw" if c >= L["raw"] else "gap"

    def check_xc(self, bits):
        """The device's packed rows against the expected bits; -> the number of elements that were judged two-sided."""
        lo, hi = self.xc_bounds()
        got = np.ascontiguousarray(bits).view(np.uint16).reshape(lo.shape)
        bad = np.argwhere((got < lo) | (got > hi))
        assert bad.size == 0, "Xc: %d elements off, first row %d column %d (%s): got 0x%04x, expected 0x%04x .. 0x%04x" % (
            len(bad), bad[0][0], bad[0][1], self.column_name(bad[0][1]), got[tuple(bad[0])], lo[tuple(bad[0])], hi[tuple(bad[0])])
        return int((lo != hi).sum())

    def wc_expected(self, gt_dev):
        """gt_dev: the device's fp32 Gt [H][A] -> uint16 [Hp][kc], every element exact."""
        d, L = self.d, self.lay
        w = np.zeros((L["Hp"], L["kc"]), np.uint16)
        for name, c0, o0, width in self.segments:
            w[:d.H, c0: c0 + width] = rne_bits(self.W1[:, o0: o0 + width])
        w[:d.H, L["c_p"]: L["c_p"] + d.A] = rne_bits(np.asarray(gt_dev, np.float32).reshape(d.H, d.A))
        return w

    def check_wc(self, bits, gt_dev):
        want = self.wc_expected(gt_dev)
        got = np.ascontiguousarray(bits).view(np.uint16).reshape(want.shape)
        bad = np.argwhere(got != want)
        assert bad.size == 0, "Wc: %d elements off, first row %d%s column %d (%s): got 0x%04x, expected 0x%04x" % (
            len(bad), bad[0][0], " (padding row)" if bad[0][0] >= self.d.H else "", bad[0][1], self.column_name(bad[0][1]), got[tuple(bad[0])], want[tuple(bad[0])])

    # -- products
    def gt(self):
        a, e = bfr(self.w1ak), bfr(self.E)
        return a @ e.T, np.abs(a) @ np.abs(e).T, 0.0, self.d.da

    def h1(self, xc_bits, wc_bits, want_pre=False):
        """From the device's operand bits -> h_1 [M, H]; the shared part (and its share of S) as MainFwdRef.layer(1)."""
        X, W = bf_val(xc_bits).reshape(self.M, -1), bf_val(wc_bits).reshape(self.lay["Hp"], -1)[:self.d.H]
        shr = np.repeat(self.fwd.sh, self.d.K, axis=0)
        pre = X @ W.T + shr
        S = np.abs(X) @ np.abs(W).T + np.abs(shr) + np.abs(self.fwd.b1)
        if want_pre:
            return pre
        h = np.maximum(pre, 0.0)
        if self.fwd.masks is not None:
            h, S = h * self.fwd.masks[0] / (1.0 - self.fwd.p), S / (1.0 - self.fwd.p)
        return h, S, 0.0, self.n_h1

    def dwc(self, dpre1, xc_bits):
        """From the device's dpre_1 and Xc bits -> {segment of dW1 | "dGt": product}."""
        g, X = bfr(dpre1).reshape(self.M, self.d.H), bf_val(xc_bits).reshape(self.M, -1)
        ref, S = g.T @ X, np.abs(g).T @ np.abs(X)
        out = {name: (ref[:, c0: c0 + w], S[:, c0: c0 + w], 0.0, self.M) for name, c0, o0, w in self.segments}
        c0 = self.lay["c_p"]
        out["dGt"] = (ref[:, c0: c0 + self.d.A], S[:, c0: c0 + self.d.A], 0.0, self.M)
        return out

    def from_block(self, dgt, dggt):
        """From the device's block dGt | dGgt ([H][A] each) -> "a_other" [H, da], "dE" [A, da]."""
        g, e = bfr(np.concatenate([np.asarray(dgt, np.float32), np.asarray(dggt, np.float32)], 0)), bfr(self.E)
        w = bfr(np.concatenate([self.w1ak, self.w1agt], 0))
        H = self.d.H
        return {"a_other": (g[:H] @ e, np.abs(g[:H]) @ np.abs(e), 0.0, self.d.A),
                "dE": (g.T @ w, np.abs(g).T @ np.abs(w), 0.0, 2 * H)}


def judge(name, got, prod):
    """-> (ratio, elements over the bound as an index array, c).  An element whose S is 0 must be exactly zero (ratio asserts it)."""
    ref, S, extra, n = prod
    c = bound_c(name, n)
    got = _f64(got).reshape(ref.shape)
    assert np.isfinite(got).all(), (name, "non-finite elements")
    r = ratio(got, ref, S, extra)
    return r, np.argwhere(np.abs(got - ref) > U24 * (c * np.broadcast_to(S, ref.shape) + extra)), c


# ---- the CPU yardstick -------------------------------------------------------------------------------------------------------------------
def ideal(case):
    """-> (Bf16Ref, xc bits, wc bits, dpre1, dgt, dggt) with every operand the rounding of the restatement's own exact value."""
    d, params, batch, masks = build(case)
    ref = Bf16Ref(params, d, batch, layout_of(case), case["p"], masks)
    xc = ref.xc_bounds(0.0)[0]
    wc = ref.wc_expected(f32(ref.gt()[0]))
    ref.bwd.whole(batch["gt"])                         # (the fp32 network's backward: plausible values of dpre_1, nothing more is asked of them)
    dpre1 = f32(ref.bwd.last_dpre1)
    parts = ref.bwd.from_dpre1(dpre1)
    return ref, xc, wc, dpre1, f32(ref.dwc(dpre1, xc)["dGt"][0]), f32(parts["dGgt"][0])


def products32(case):
    """-> {name: (product, torch float32 result, row-order float32 result)} of one case from its ideal operands: the same exact bf16
    products summed in float32 in two orders."""
    ref, xc, wc, dpre1, dgt, dggt = ideal(case)
    d = ref.d
    X, W = bf_val(xc).astype(np.float32), bf_val(wc).astype(np.float32)[:d.H]
    out = {}
    with one_thread():
        a, e = bfr(ref.w1ak).astype(np.float32), bfr(ref.E).astype(np.float32)
        out["Gt"] = (ref.gt(), torch32(a.T, e.T), row_order(a.T, e.T))
        shr = f32(np.repeat(ref.fwd.sh, d.K, axis=0))
        scale = np.float32(1.0 / (1.0 - ref.fwd.p)) * f32(ref.fwd.masks[0]) if ref.fwd.masks is not None else np.float32(1.0)
        epi = lambda acc: np.maximum(acc + shr, np.float32(0)) * scale
        out["h1"] = (ref.h1(xc, wc), epi(torch32(X.T, W.T)), epi(row_order(X.T, W.T)))
        g = bfr(dpre1).astype(np.float32)
        g_t, g_r = torch32(g, X), row_order(g, X)
        for name, prod in ref.dwc(dpre1, xc).items():
            c0, w = {s[0]: (s[1], s[3]) for s in ref.segments}.get(name, (ref.lay["c_p"], d.A))
            out[name] = (prod, g_t[:, c0: c0 + w], g_r[:, c0: c0 + w])
        blk = ref.from_block(dgt, dggt)
        gb = bfr(np.concatenate([dgt, dggt], 0)).astype(np.float32)
        wb = bfr(np.concatenate([ref.w1ak, ref.w1agt], 0)).astype(np.float32)
        out["a_other"] = (blk["a_other"], torch32(gb[:d.H].T, e), row_order(gb[:d.H].T, e))
        out["dE"] = (blk["dE"], torch32(gb, wb), row_order(gb, wb))
    return out


def yardstick(case):
    """-> {group: (torch float32 ratio, row-order float32 ratio)} of one case."""
    out = {g: [0.0, 0.0] for g in GROUPS}
    for name, (prod, g_t, g_r) in products32(case).items():
        for i, got in enumerate((g_t, g_r)):
            out[GROUP_OF[name]][i] = max(out[GROUP_OF[name]][i], ratio(got, prod[0], prod[1]))
    return {g: tuple(v) for g, v in out.items()}


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# Constants of the kernels the cases are placed around (csrc/ncx_bf16.hip): packed rows in segments that start on multiples of 8 columns, kc
# = raw rounded up to 128; NT tiles 128 / 64 rows x 128 / 64 columns (forms 0..3) in 64-deep k-steps taken two at a time (kc = 128: the
# minimum; kc = 384: the clamp of the loads two and three steps ahead), or 192 rows x all 256 columns (form 8, Hp == 256 only); TN tiles 128
# x 128 (or 256 x 128: tn8, Hp == 256 only) over S k-chunks of `chunk` rows, chunk = ceil(ceil(M / S) / 64) 64, of which nz hold rows; the
# converters and packers take 4 columns per thread where the widths are multiples of 4; E, E^T, [W1ak; W1agt] and [dGt; dGgt] padded to dap,
# Ap = da, A rounded up to 128.
BASE = dict(K=5, B=11, dv=36, dq=8, dz=20, da=12, A=44, H=37, L=1)
CASES = []


def _case(tag, env=None, drop=None, p=0.0, cu_dependent=False, **over):
    """One case.  env: experiment hooks (set with NCX_EXPERIMENT=1 before the workspace is sized).  route: what ncx_plan_query(
    NCX_QUERY_BF16_ROUTE) must report, stated here from the kernel family's rules as DESIGN 5c gives them, not asked of the library.  Without
    hooks the small shapes of this table take the 64 x 64 NT tiles and the 128 x 128 TN kernel on 8 k-chunks on any chip with more than 5
    CUs (128 x 128 tiles need 2 per CU, the 8-wave kernels a batch in the thousands).  The forced 256 x 128 TN kernel takes min(8, CUs / (kc
    / 128)) k-chunks: 8 on a chip of 24 CUs or more, hence cu_dependent."""
    c = dict(BASE, **over)
    env = dict(env or {})
    M, hp256 = c["B"] * c["K"], (c["H"] + 127) // 128 * 128 == 256
    nt = int(env.get("NCX_BF16_NT_CFG", 3))
    assert nt in (0, 1, 2, 3) or (nt == 8 and hp256), "form 8 is only legal where Hp == 256"
    tn8 = "NCX_BF16_TN8" in env and "NCX_BF16_NO_TN8" not in env
    assert hp256 or not tn8, "the 256 x 128 TN kernel is only legal where Hp == 256"
    chunk = (-(-M // 8) + 63) // 64 * 64
    din = R.din(c)
    route = dict(nt=nt, tn8=tn8, S=8, chunk=chunk, nz=-(-M // chunk), vec_dpre=c["H"] % 4 == 0, vec_e=c["da"] % 4 == 0,
                 vec_w1a=c["da"] % 4 == 0 and din % 4 == 0, vec_dg=c["A"] % 4 == 0)
    c.update(id=tag, env=env, lesion=None, drop=drop, p=p, route=route, cu_dependent=cu_dependent or tn8, M=M)
    CASES.append(c)
    return c


_case("base")
# column layout
for dv in (40, 70):                                    # 36: a gap of 4; 40: no gap; 70: dv % 4 != 0
    _case("dv%d" % dv, dv=dv)
for K in (3, 7, 24, 48, 64):                           # K + 1 = 4, 8, 25, 49, 65
    _case("K%d" % K, K=K, B=3 if K > 7 else 11)
for dz in (4, 18, 24):
    _case("dz%d" % dz, dz=dz)
# Kc extent: raw = 2 up8(dv) + up8(K + 1) + up8(dz) + A
_case("raw92-kc128", dv=4)                             # the two-step minimum of the NT loop
_case("raw256-no-padding", A=144)                      # raw % 128 == 0
_case("raw129", A=17)                                  # raw % 128 == 1
_case("raw312-kc384", A=200)                           # the t + 3 clamp in the steady state
for A in (45, 128, 129, 132):                          # A % 4: the VEC / plain [dGt; dGgt] pack and the store_bf16x4 tail; Ap == A against Ap = 256
    _case("A%d" % A, A=A)
for da in (100, 128, 130):
    _case("da%d" % da, da=da)
for H in (128, 130, 200, 256, 257, 260):               # 257, 260: Hp = 384, three row tiles in TN, three column tiles in NT, neither 8-wave kernel
    _case("H%d" % H, H=H)
# rows M = B K
for K, B in ((3, 3), (3, 21), (5, 13), (5, 40), (4, 128), (3, 171)):      # 9: nz = 1; 63; 65; 200: chunk 64, nz 4; 512: 8 full chunks; 513: chunk 128, a last chunk of one row
    _case("M%d" % (K * B), K=K, B=B)
for B in (63, 64, 65):                                 # the 192-row kernel (docstring, "Rows") and the 256 x 128 TN kernel
    _case("M%d-H256-nt8-tn8" % (3 * B), env={"NCX_BF16_NT_CFG": "8", "NCX_BF16_TN8": "1"}, K=3, B=B, H=256)
# kernel forms: the forms of one shape must agree (FORM_SHAPES below) and hold the bound each alone
FORM_SHAPES = (("H200-M200", dict(H=200, K=5, B=40)), ("H256-M65", dict(H=256, K=5, B=13)))
for tag, shape in FORM_SHAPES:
    for nt in (0, 1, 2, 3, 8):
        for tn_tag, tn in (("tn", {"NCX_BF16_NO_TN8": "1"}), ("tn8", {"NCX_BF16_TN8": "1"})):
            _case("forms-%s-nt%d-%s" % (tag, nt, tn_tag), env=dict(tn, NCX_BF16_NT_CFG=str(nt)), **shape)
for nt in (0, 1, 2):                                   # several tiles both ways on the forced tiles, Hp = 384
    _case("forms-H260-M200-nt%d" % nt, env={"NCX_BF16_NT_CFG": str(nt), "NCX_BF16_NO_TN8": "1"}, H=260, K=5, B=40)
# depth and dropout at a ragged H
_case("L2-masks", drop="masks", p=0.25, L=2)
_case("L2-rng", drop="rng", p=0.25, L=2)
_case("L3", L=3)
# rows wider than k_prep keeps in registers: the non-resident branch of its pack
_case("wide-dv2052-A2049", dv=2052, A=2049, B=2, K=3, H=16)
BY_ID = {c["id"]: c for c in CASES}
assert len(BY_ID) == len(CASES)
# the values section 2 of the issue lists, for test_case_table_covers_the_listed_values
LISTED = dict(dv=(36, 40, 70), K=(3, 7, 24, 48, 64), dz=(4, 18, 24), A=(44, 45, 128, 129, 132), da=(12, 100, 128, 130), H=(37, 128, 130, 200, 256),
              M=(9, 63, 65, 200, 512, 513, 189, 192, 195), nt=(0, 1, 2, 3, 8), L=(1, 2, 3))


def shape_key(c):
    return R.shape_key(c)


_BUILT = {}


def build(c):
    """-> (orc.Dims, params, batch, keep masks or None) of a case, built once per shape and never modified: main_fwd_ref.build's inputs, kept
    away from the ReLU kinks of the bf16 network (helpers.condition_away_from_kinks; only the comparison of a shape's forms needs it, every
    product being judged from the device's own gates), and with every triplet redrawn whose distance is ambiguous at tau_dist."""
    key = shape_key(c)
    if key not in _BUILT:
        d, params, batch, spec, masks = R.build(c)
        assert spec is None
        seed = int(batch["answer_aids"].sum()) + 7 * c["B"]
        lay = layout_of(c)
        for rnd in range(40):
            condition_away_from_kinks(params, d, batch, seed + rnd, tau=Bw.TAU, bf16=True)
            ref = Bf16Ref(params, d, batch, lay, c["p"], masks)
            lo, hi = ref.xc_bounds()
            bad = np.unique(np.argwhere(lo[:, lay["c_misc"]] != hi[:, lay["c_misc"]])[:, 0] // d.K)
            if bad.size == 0:
                break
            fresh = random_case_f32(seed * 977 + rnd + 1, len(bad), d)
            for k in ("image_features", "q_emb", "z_orig", "z_knns", "a_knns", "answer_aids", "gt"):
                batch[k][torch.from_numpy(bad)] = fresh[k]
        else:
            raise AssertionError("could not draw a batch without an ambiguous distance")
        _BUILT[key] = (d, params, batch, masks)
    return _BUILT[key]
