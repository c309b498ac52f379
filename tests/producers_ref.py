"""The frozen VQA producers (csrc/ncx_vqa.hip + ncx_mutan.hip: ncx_vqa_forward; csrc/ncx_mlb.hip: ncx_mlb_forward) at their edge shapes:
an fp64 restatement that works product by product, a per-element rounding bound, and the table of cases.  Plain numpy / torch;
tests/test_producer_edges_cpu.py checks what this file claims, tests/test_producer_edges_gpu.py runs the kernels on the cases.

The restatement.  Every stage is restated from the inputs it is GIVEN (on the GPU: what the device produced for it, read through
ops.vqa_ws_view), so a stage is judged alone, and returns per element the value and the magnitude sum S of the terms it is made of.
    Mutan (fusion.py:78-121, noatt.py:24-29)
        xq  <- q_emb             act_q(q Wq^T + bq)                               S = |q| |Wq|^T + |bq|
        hq  <- xq                xq Whq^T + bhq          [B, R dz]                S = |xq| |Whq|^T + |bhq|
        xv  <- feats[img_idx]    act_v(v Wv^T + bv)      [B (K + 1), dhv]         S = |v| |Wv|^T + |bv|
        z   <- (xv, hq)          sum_r (xv Whv_r^T + bhv_r) hq_r[question]        S = sum_r (|xv| |Whv_r|^T + |bhv_r|) |hq_r|
        a   <- z                 z Wc^T + bc             (a_knns from z_knns, a_orig from z_orig)
    MLB (fusion.py:31-50, noatt.py:24-29)
        xq  <- q_emb
        xv  <- feats[img_idx]    generic route only (the fused route never stores it)
        z   <- (xv, xq)          xv xq[question]: one product                     S = |xv xq|
        z   <- (feats, xq)       fused route, one step: act_v(v Wv^T + bv) xq     S = S_xv |xq|   (S_xv with the tanh term below)
        t   <- z                 tanh(z) with classif.activation                  S = |z| (the one term of its argument)
        a   <- t or z
The bound   |got - ref| <= c 2^-24 S, the project's standing form; behind a tanh S + |ref| takes the place of S (tanh is 1-Lipschitz, so the
error of its argument carries over, and its own rounding is relative to the result).  c per case group is C_MARGIN x what a plain float32
restatement (torch on the CPU, one thread, op for op as oracle.mutan_vqa_forward / mlb_ref.mlb_vqa_forward write the models) reaches on the
group's cases, every stage judged alone: ORACLE32_RATIO, measured by test_producer_edges_cpu.py, recorded in profiles/producer_edges.json.
"""
import zlib

import numpy as np
import torch
import torch.nn.functional as F

U24 = 2.0 ** -24
LIM32 = (1 << 32) - 65536            # what the fused forward kernel's 32-bit byte offsets may address (csrc/ncx_internal.h)
CUS = 256                            # the chip the CU-dependent case is placed for (and what the library assumes without a device)

# max over the group's cases and stages of |x32 - ref| / (2^-24 S) for the float32 restatement, rounded up, on the host that wrote
# profiles/producer_edges.json (another CPU's BLAS sums in another order: test_recorded_oracle32_ratios_reproduce asks for the same size)
ORACLE32_RATIO = {"fold": 4.6, "engine": 4.6, "routes": 4.1, "mlb": 4.6, "big": 2.1}
C_MARGIN = 4.0


def bound_c(group):
    return C_MARGIN * ORACLE32_RATIO[group]


def _f64(t):
    return np.asarray(t.detach().cpu().numpy() if torch.is_tensor(t) else t, dtype=np.float64)


def ratio(got, ref, S):
    """max |got - ref| / (2^-24 S) over the elements (an element whose S is 0 must be exact)."""
    err = np.abs(_f64(got).reshape(ref.shape) - ref)
    assert (err[S == 0] == 0).all()
    return float((err[S > 0] / (U24 * S[S > 0])).max())


def _act(pre, S, act):
    if act == "tanh":
        v = np.tanh(pre)
        return v, S + np.abs(v)
    return pre, S


def _linear(x, W, b):
    x = _f64(x)
    return x @ W.T + b, np.abs(x) @ np.abs(W).T + np.abs(b)


def split_rows(x, B, K1):
    """[B (K + 1), n] -> (orig [B, n], knns [B K, n]): the row split of the producers' outputs."""
    x = x.reshape(B, K1, -1)
    return x[:, 0], x[:, 1:].reshape(B * (K1 - 1), -1)


# ---- the restatements --------------------------------------------------------------------------------------------------------------------
class MutanRef:
    """state: the MutanNoAtt state_dict (fp32 tensors); every stage -> (value, S) in fp64 from the inputs given."""

    def __init__(self, state, c):
        g = lambda k: _f64(state[k])
        self.c, R = c, c["R"]
        self.Wv, self.bv, self.Wq, self.bq = g("fusion.linear_v.weight"), g("fusion.linear_v.bias"), g("fusion.linear_q.weight"), g("fusion.linear_q.bias")
        self.Whv = np.stack([g("fusion.list_linear_hv.%d.weight" % r) for r in range(R)])      # [R, dz, dhv]
        self.bhv = np.stack([g("fusion.list_linear_hv.%d.bias" % r) for r in range(R)])        # [R, dz]
        self.Whq = np.concatenate([g("fusion.list_linear_hq.%d.weight" % r) for r in range(R)])  # [R dz, dhq]
        self.bhq = np.concatenate([g("fusion.list_linear_hq.%d.bias" % r) for r in range(R)])
        self.Wc, self.bc = g("linear_classif.weight"), g("linear_classif.bias")

    def xq(self, q_emb):
        return _act(*_linear(q_emb, self.Wq, self.bq), self.c["act"])

    def hq(self, xq):
        return _linear(xq, self.Whq, self.bhq)

    def xv(self, v_rows):
        """v_rows: feats[img_idx] as [B (K + 1), dv]."""
        return _act(*_linear(v_rows, self.Wv, self.bv), self.c["act"])

    def z(self, xv, hq):
        """-> z, S as [B (K + 1), dz] (rows in img_idx order; split_rows gives z_orig / z_knns)."""
        c = self.c
        B, K1, R, dz = c["B"], c["K1"], c["R"], c["dz"]
        xv = _f64(xv)
        h = np.repeat(_f64(hq).reshape(B, R, dz), K1, axis=0)                          # [B K1, R, dz]: the question's factors per image
        hv = np.einsum("mk,rjk->mrj", xv, self.Whv) + self.bhv
        Sv = np.einsum("mk,rjk->mrj", np.abs(xv), np.abs(self.Whv)) + np.abs(self.bhv)
        return (hv * h).sum(1), (Sv * np.abs(h)).sum(1)

    def a(self, z):
        return _linear(z, self.Wc, self.bc)

    def chain(self, v_rows, q_emb):
        """The whole producer on the restatement's own intermediates -> (a_orig, z_orig, a_knns, z_knns) as the oracle shapes them."""
        c = self.c
        xq = self.xq(q_emb)[0]
        z = self.z(self.xv(v_rows)[0], self.hq(xq)[0])[0]
        a = self.a(z)[0]
        sh = lambda x: x.reshape(c["B"], c["K1"], -1)
        return sh(a)[:, 0], sh(z)[:, 0], sh(a)[:, 1:], sh(z)[:, 1:]


class MlbRef:
    def __init__(self, state, c):
        g = lambda k: _f64(state[k])
        self.c = c
        self.Wv, self.bv, self.Wq, self.bq = g("fusion.linear_v.weight"), g("fusion.linear_v.bias"), g("fusion.linear_q.weight"), g("fusion.linear_q.bias")
        self.Wc, self.bc = g("linear_classif.weight"), g("linear_classif.bias")

    def xq(self, q_emb):
        return _act(*_linear(q_emb, self.Wq, self.bq), self.c["act"])

    def xv(self, v_rows):
        return _act(*_linear(v_rows, self.Wv, self.bv), self.c["act"])

    def z(self, xv, xq):
        z = _f64(xv) * np.repeat(_f64(xq), self.c["K1"], axis=0)
        return z, np.abs(z)

    def z_fused(self, v_rows, xq):
        """z from the feature rows and x_q in one step (the fused route: x_v exists only inside the kernel)."""
        xv, Sv = self.xv(v_rows)
        q = np.repeat(_f64(xq), self.c["K1"], axis=0)
        return xv * q, Sv * np.abs(q)

    def t(self, z):
        z = _f64(z)
        return np.tanh(z), np.abs(z) + np.abs(np.tanh(z))

    def a(self, x):
        return _linear(x, self.Wc, self.bc)

    def chain(self, v_rows, q_emb):
        c = self.c
        z = self.z(self.xv(v_rows)[0], self.xq(q_emb)[0])[0]
        a = self.a(self.t(z)[0] if c["act_c"] else z)[0]
        sh = lambda x: x.reshape(c["B"], c["K1"], -1)
        return sh(a)[:, 0], sh(z)[:, 0], sh(a)[:, 1:], sh(z)[:, 1:]


# ---- float32, op for op as the oracles write the models (the source of c) -----------------------------------------------------------------
def mutan_float32(vp, v_rows, q_emb, R, act):
    """oracle.mutan_vqa_forward's operations (F.linear, tanh, mul, stack.sum) with the intermediates kept and the activation optional."""
    f = torch.tanh if act == "tanh" else (lambda x: x)
    K1 = v_rows.shape[0] // q_emb.shape[0]
    x_v = f(F.linear(v_rows, vp["fusion.linear_v.weight"], vp["fusion.linear_v.bias"]))
    x_q = f(F.linear(q_emb, vp["fusion.linear_q.weight"], vp["fusion.linear_q.bias"]))
    x_qr = x_q.repeat_interleave(K1, 0)                                        # (cx.py:83-84 duplicates q before linear_q: the same rows)
    hq, x_mm = [], []
    for i in range(R):
        hv = F.linear(x_v, vp["fusion.list_linear_hv.%d.weight" % i], vp["fusion.list_linear_hv.%d.bias" % i])
        hq.append(F.linear(x_q, vp["fusion.list_linear_hq.%d.weight" % i], vp["fusion.list_linear_hq.%d.bias" % i]))
        x_mm.append(torch.mul(hq[-1].repeat_interleave(K1, 0), hv))
    z = torch.stack(x_mm, dim=1).sum(1)
    a = F.linear(z, vp["linear_classif.weight"], vp["linear_classif.bias"])
    return dict(xq=x_q, hq=torch.cat(hq, 1), xv=x_v, z=z, a=a, x_qr=x_qr)


def mlb_float32(vp, v_rows, q_emb, act, act_c):
    f = torch.tanh if act == "tanh" else (lambda x: x)
    K1 = v_rows.shape[0] // q_emb.shape[0]
    x_v = f(F.linear(v_rows, vp["fusion.linear_v.weight"], vp["fusion.linear_v.bias"]))
    x_q = f(F.linear(q_emb, vp["fusion.linear_q.weight"], vp["fusion.linear_q.bias"]))
    z = torch.mul(x_q.repeat_interleave(K1, 0), x_v)
    t = torch.tanh(z) if act_c else z
    a = F.linear(t, vp["linear_classif.weight"], vp["linear_classif.bias"])
    return dict(xq=x_q, xv=x_v, z=z, t=t, a=a)


def oracle32_ratio(case):
    """The float32 restatement's worst ratio over the stages of one case, every stage judged on float32's own inputs; one thread, so
    that the figure does not depend on the machine's core count."""
    state, table, idx, q_emb = build(case)
    v_rows = table[torch.from_numpy(idx.reshape(-1).astype(np.int64))]
    threads = torch.get_num_threads()
    torch.set_num_threads(1)
    try:
        with torch.no_grad():
            x = mutan_float32(state, v_rows, q_emb, case["R"], case["act"]) if case["kind"] == "mutan" else \
                mlb_float32(state, v_rows, q_emb, case["act"], case["act_c"])
    finally:
        torch.set_num_threads(threads)
    if case["kind"] == "mutan":
        ref = MutanRef(state, case)
        stages = [(x["xq"], ref.xq(q_emb)), (x["hq"], ref.hq(x["xq"])), (x["xv"], ref.xv(v_rows)), (x["z"], ref.z(x["xv"], x["hq"])), (x["a"], ref.a(x["z"]))]
    else:
        ref = MlbRef(state, case)
        stages = [(x["xq"], ref.xq(q_emb)), (x["xv"], ref.xv(v_rows)), (x["z"], ref.z(x["xv"], x["xq"])), (x["z"], ref.z_fused(v_rows, x["xq"])),
                  (x["a"], ref.a(x["t"]))]
        if case["act_c"]:
            stages.append((x["t"], ref.t(x["z"])))
    return max(ratio(got, *vs) for got, vs in stages)


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
# Constants the cases are placed on.  k_mutan_fold: 8 questions x 32 columns per workgroup, 32-deep k-steps over dhv (16-byte quads, clamped
# to dhv - 4), at most 32 rows per question, workgroup ids dealt over 8 XCDs.  The generic engine's FOLD chain: 64 x 64 tiles, R pairs,
# fold_div = rowsplit_g = K + 1.  The fused forward kernel takes x_v for whole 32-column feature rows from 64 on and a table below 4 GiB,
# and the classifier for dz % 4 == A % 4 == 0, against the weights in place (dz % 32 == 0) or a zero-padded copy.
CASES = []


def _route_mutan(c):
    main = "NCX_VQA_NO_MAIN" not in c["env"]
    main_v = main and c["dv"] % 32 == 0 and c["dv"] >= 64 and c["n_img"] * c["dv"] * 4 < LIM32
    fold = c["K1"] <= 32 and c["dhv"] % 4 == 0 and c["R"] <= 10 and "NCX_NO_MUTAN_FOLD" not in c["env"]
    return dict(main_v=main_v, fold_kernel=fold, classifier=_route_classifier(c, main))


def _route_classifier(c, main):
    if not (main and c["dz"] % 4 == 0 and c["A"] % 4 == 0):
        return "generic"
    return "main" if c["dz"] % 32 == 0 else "main_padded"


def _route_mlb(c):
    main = "NCX_VQA_NO_MAIN" not in c["env"]
    main_v = main and c["dv"] % 32 == 0 and c["dv"] >= 64 and c["n_img"] * c["dv"] * 4 < LIM32
    tiles96 = -(-c["B"] * c["K1"] // 96) * -(-c["dz"] // 128)
    return dict(main_v=main_v, v_tile=None if not main_v else "96x128" if tiles96 * 10 >= CUS * 9 else "48x128",
                classifier=_route_classifier(c, main), t_stored=bool(c["act_c"]))


def _mutan(group, tag, shape, act="tanh", a_orig=True, env=None, n_img=None, ids=None):
    B, K1, dv, dq, dhv, dhq, dz, R, A = shape
    c = dict(kind="mutan", group=group, id="%s-%s" % (group, tag), B=B, K1=K1, dv=dv, dq=dq, dhv=dhv, dhq=dhq, dz=dz, R=R, A=A, act=act, act_c=None,
             a_orig=a_orig, env=dict(env or {}), n_img=n_img or B * K1 + 7, ids=ids, cu_dependent=False)
    c["route"] = _route_mutan(c)
    c["ksteps"] = -(-dhv // 32)
    CASES.append(c)
    return c


def _mlb(tag, shape, act="tanh", a_orig=True, env=None, cu_dependent=False):
    B, K1, dv, dq, dh, A, act_c = shape
    c = dict(kind="mlb", group="mlb", id="mlb-%s" % tag, B=B, K1=K1, dv=dv, dq=dq, dz=dh, A=A, act=act, act_c=act_c, a_orig=a_orig, env=dict(env or {}),
             n_img=B * K1 + 7, ids=None, cu_dependent=cu_dependent)
    c["route"] = _route_mlb(c)
    CASES.append(c)
    return c


# fold: k_mutan_fold
_mutan("fold", "every-minimum", (1, 2, 64, 8, 4, 4, 4, 1, 4))                      # dhv = 4: every quad clamped to offset 0; a batch of one
_mutan("fold", "one-group-one-step", (8, 4, 64, 20, 32, 12, 32, 2, 8))             # exactly one group, one k-step, one column tile; Wc in place
_mutan("fold", "K1-32-no-padding", (9, 32, 96, 48, 36, 20, 36, 10, 40))            # no padding row; a partial second k-step; R = 10
_mutan("fold", "nine-groups", (65, 25, 96, 48, 68, 20, 100, 3, 52))                # two groups on XCD 0, early-exit ids; 3 k-steps; ragged 4th column tile
_mutan("fold", "dz37", (13, 25, 96, 48, 64, 20, 37, 4, 42))                        # 2 k-steps; dz % 4 != 0: the column guard, classifier generic; A % 4 != 0
_mutan("fold", "no-activation", (13, 25, 96, 48, 64, 20, 37, 4, 42), act=None, a_orig=False)
# engine: the FOLD instantiation of seg_gemm_kernel
_mutan("engine", "K1-33", (5, 33, 96, 48, 28, 20, 44, 4, 52))                      # the first K past the fold kernel
_mutan("engine", "K1-49", (3, 49, 96, 48, 40, 20, 70, 10, 40))                     # 147 rows: three row tiles, questions straddle them; ragged 2nd column tile
_mutan("engine", "dhv30", (13, 25, 96, 48, 30, 20, 44, 1, 52))                     # dhv % 4 != 0; R = 1
_mutan("engine", "nine-groups-hook", (65, 25, 96, 48, 68, 20, 100, 3, 52), env={"NCX_NO_MUTAN_FOLD": "1"})      # fold-nine-groups' inputs on the other route
# routes: x_v and the classifier
_mutan("routes", "dv64-dz32", (13, 25, 64, 48, 36, 20, 32, 4, 40), a_orig=False)   # the least width the fused kernel takes; Wc in place
_mutan("routes", "dv32-dz64", (13, 25, 32, 48, 36, 20, 64, 4, 40))                 # generic gather; Wc in place
_mutan("routes", "dv72-dz36", (13, 25, 72, 48, 36, 20, 36, 4, 40), a_orig=False)   # generic gather; padded copy
_mutan("routes", "dv70-dz37", (13, 25, 70, 48, 36, 20, 37, 4, 42))                 # 16-byte windows slide; classifier generic
_mutan("routes", "dv72-K1-33", (5, 33, 72, 48, 28, 20, 44, 4, 52))                 # generic gather in front of the FOLD engine
_mutan("routes", "dv64-K1-49", (3, 49, 64, 48, 40, 20, 64, 2, 40), a_orig=False)   # fused x_v in front of the FOLD engine; Wc in place
# mlb: K + 1 over both x_v routes and both classifier routes
_MLB_B = {2: 1, 4: 7, 32: 3, 33: 5, 49: 3}
for _i, _K1 in enumerate(sorted(_MLB_B)):
    for _dv in (96, 72):
        for _A in (40, 42):
            _odd = (_i + (_dv == 72) + (_A == 42)) % 2
            _mlb("K1-%d-dv%d-A%d" % (_K1, _dv, _A), (_MLB_B[_K1], _K1, _dv, 48, 64 if (_dv == 72 and _A == 40) else 36, _A, None if _odd else "tanh"),
                 a_orig=not _odd)
_mlb("no-activation", (5, 25, 96, 48, 36, 40, None), act=None)
# 24 x 10 tiles of 96 x 128, ragged on both sides: the larger tile form on a chip of 256 CUs, questions straddling 96-row tiles
_mlb("tiles-96x128", (89, 25, 64, 48, 1240, 40, "tanh"), cu_dependent=True)
# big: a feature table beyond 4 GiB (8192-byte rows: ids past 2^30, 2^31 and, for the last image, 2^32 bytes)
BIG_N_IMG = 525000
BIG_IDS = np.array([[BIG_N_IMG - 1, 5, 131073 + 10, BIG_N_IMG - 1], [262144 + 77, BIG_N_IMG - 1, 5, 400000]], np.int32)
_mutan("big", "table-beyond-4GiB", (2, 4, 2048, 16, 8, 8, 8, 2, 8), n_img=BIG_N_IMG, ids=BIG_IDS)

BY_ID = {c["id"]: c for c in CASES}
GROUPS = sorted({c["group"] for c in CASES})
assert len(BY_ID) == len(CASES)


def shape_key(c):
    """What the inputs and the restatement of a case depend on (not its hooks, not a_orig)."""
    return tuple(c.get(k) for k in ("kind", "B", "K1", "dv", "dq", "dhv", "dhq", "dz", "R", "A", "act", "act_c", "n_img"))


def _init_linear(out_f, in_f):
    """nn.Linear's own initialiser (kaiming_uniform(a = sqrt 5) and the matching bias: U(+-1 / sqrt(fan_in)) both), which the reference's
    models keep; |v| <~ 1 and |q| <~ 1.5 then leave tanh well off saturation (pre-activations of a few tenths)."""
    lin = torch.nn.Linear(in_f, out_f)
    return lin.weight.detach().clone(), lin.bias.detach().clone()


def build(c):
    """-> (state_dict of fp32 tensors, table [rows, dv] fp32, idx [B, K + 1] int32 into `table`, q_emb [B, dq] fp32), seeded by the shape.
    The table has spare rows, idx is shuffled and repeats one image inside a question and one across questions.  For the case beyond
    4 GiB the table holds only the rows used and idx points into it: c["ids"] are the ids of those rows in the device's table
    (device_rows)."""
    seed = zlib.crc32(repr(shape_key(c)).encode()) % (2 ** 31)
    rng = np.random.default_rng(seed)
    B, K1, dv, dq, dz, A = (c[k] for k in ("B", "K1", "dv", "dq", "dz", "A"))
    state = {}
    with torch.random.fork_rng(devices=[]):
        torch.manual_seed(seed)
        lin = lambda name, o, i: state.update(zip((name + ".weight", name + ".bias"), _init_linear(o, i)))
        if c["kind"] == "mutan":
            lin("fusion.linear_v", c["dhv"], dv); lin("fusion.linear_q", c["dhq"], dq)
            for r in range(c["R"]):
                lin("fusion.list_linear_hv.%d" % r, dz, c["dhv"]); lin("fusion.list_linear_hq.%d" % r, dz, c["dhq"])
        else:
            lin("fusion.linear_v", dz, dv); lin("fusion.linear_q", dz, dq)
        lin("linear_classif", A, dz)
    if c["ids"] is not None:
        uniq, inv = np.unique(c["ids"], return_inverse=True)
        rows, idx = len(uniq), inv.reshape(B, K1).astype(np.int32)
    else:
        rows = c["n_img"]
        idx = rng.permutation(rows)[:B * K1].reshape(B, K1).astype(np.int32)
        idx[0, K1 - 1] = idx[0, 0]                                       # one image twice inside a question
        if B > 1:
            idx[B - 1, 0] = idx[0, 1 % K1]                               # ... and one in two questions
    table = torch.from_numpy((np.abs(rng.standard_normal((rows, dv))) * 0.45).astype(np.float32))
    q_emb = torch.from_numpy((rng.standard_normal((B, dq)) * 0.5).astype(np.float32))
    return state, table, idx, q_emb


def device_rows(c):
    """Ids in the device's table of the rows build()'s table holds, in order (None: the table is the device's table)."""
    return None if c["ids"] is None else np.unique(c["ids"])


def stacked(state, c):
    """The state_dict in the layout of ops.MutanWeights.from_tensors / MlbWeights.from_tensors."""
    t = dict(wv=state["fusion.linear_v.weight"], bv=state["fusion.linear_v.bias"], wq=state["fusion.linear_q.weight"], bq=state["fusion.linear_q.bias"],
             wc=state["linear_classif.weight"], bc=state["linear_classif.bias"])
    if c["kind"] == "mutan":
        for k, name in (("whv", "hv"), ("whq", "hq")):
            t[k] = torch.cat([state["fusion.list_linear_%s.%d.weight" % (name, r)] for r in range(c["R"])])
            t["b" + name] = torch.cat([state["fusion.list_linear_%s.%d.bias" % (name, r)] for r in range(c["R"])])
    return t


ACT_CODE = {None: 0, "tanh": 2}


def c_dims_and_params(c):
    """(NcxDims, ncx_mutan_params / ncx_mlb_params) of a case for the host-only entries: the pointers are never followed there, so a non-NULL
    placeholder stands for every tensor."""
    from neuralcx import _lib
    d = _lib.NcxDims()
    d.B, d.K, d.dv, d.dq, d.dz, d.da, d.A, d.H, d.L, d.n_img = c["B"], c["K1"] - 1, c["dv"], c["dq"], c["dz"], 4, c["A"], 4, 1, c["n_img"]
    if c["kind"] == "mutan":
        m = _lib.NcxMutanParams()
        m.dhv, m.dhq, m.R, m.act_v, m.act_q = c["dhv"], c["dhq"], c["R"], ACT_CODE[c["act"]], ACT_CODE[c["act"]]
    else:
        m = _lib.NcxMlbParams()
        m.dh, m.act_v, m.act_q, m.act_c = c["dz"], ACT_CODE[c["act"]], ACT_CODE[c["act"]], ACT_CODE[c["act_c"]]
    for name, ctype in m._fields_:
        if ctype is _lib.C.c_void_p:
            setattr(m, name, 256)
    return d, m


def query_route(c):
    from neuralcx import _lib
    d, m = c_dims_and_params(c)
    return (_lib.vqa_route if c["kind"] == "mutan" else _lib.mlb_route)(d, m)
