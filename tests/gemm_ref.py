"""The generic GEMM engine (csrc/ncx_gemm.h: seg_gemm_kernel, split_fixup_kernel, WgMap; driven through run_gemm_planned) called directly
through ncx_diag_gemm: an fp64 restatement of what one launch computes, the same restatement in float32, a per-element rounding bound,
and the table of cases.  Plain numpy.  tests/test_gemm_engine_cpu.py checks what this file claims, tests/test_gemm_engine_gpu.py runs the
kernels on the cases.

The restatement.  A launch is `nseg` (a, b, klen) pairs.  An operand is a logical row-major matrix x(r, c) that is never materialised:
    plain        x = base[r ld + c]
    gather       x = base[idx[r stride] ld + c]
    gather-mul   x = base[idx[r stride] ld + c] base[idx2[r stride] ld + c]
    softmax      x = exp2(base[r ld + c] log2(e) - lse2[r])
and a pair's product is A B^T (NT: both [out, k]), A^T B (TN: both [k, out]) or A B (NN: A [M, k], B [k, N]).  A CHAIN sums its pairs
into one output, a GROUP keeps one output per pair, the FOLD chain computes z = sum_s (P_s + fold_bias[s]) fold_mul[r / fold_div, s].
A split problem is summed chunk by chunk: chunk z of S takes the 32-deep k-steps [T z / S, T (z + 1) / S) of the problem's T steps.
The epilogue, in the kernel's order: + rowadd[r / rowdiv], + bias, relu or tanh, dropout (mask or generator) x drop_scale, gate x
gate_scale; rowsplit_g only places rows.
Every element comes with S, the magnitude sum of the terms it is made of: |a| |b| per product term -- a softmax factor counts
(1 + |its exp2 argument|) times, its argument being rounded before the exponential --, |rowadd|, |bias|; behind tanh S + |ref|; a dropped
or gated-off element has S = 0 (it must be exactly 0); drop_scale and gate_scale multiply S.
The bound   |got - ref| <= c 2^-24 S   for every element.  c per case group is C_MARGIN x the largest ratio the float32 restatement
(numpy float32, op for op, one BLAS product per pair or chunk) reaches on the group's cases: ORACLE32_RATIO, measured by
test_gemm_engine_cpu.py and recorded in profiles/gemm_engine_edges.json.  It never comes from the kernel.
"""
import zlib

import numpy as np

U24 = 2.0 ** -24
LOG2E = 1.4426950408889634
NT, TN, NN = 0, 1, 2
FORM_NAME = ("nt", "tn", "nn")
CHAIN, GROUP = 0, 1
PLAIN, GATHER, GMUL, SOFTMAX = 0, 1, 2, 3
KIND_NAME = ("plain", "gather", "gmul", "softmax")
TILE = {0: (64, 64), 1: (128, 128), 2: (96, 128), 3: (96, 64), 4: (128, 64)}     # cfg code -> BM, BN (csrc/ncx_internal.h: TileCfg)
SUPPORTED = {NT: (0, 1, 2, 3), TN: (0, 1, 4), NN: (0, 1)}                        # the instantiations of csrc/ncx_gemm_inst.hip
# the ten kernels: (name, form, cfg, fold)
INSTANCES = [("nt-64x64", NT, 0, False), ("nt-96x64", NT, 3, False), ("nt-96x128", NT, 2, False), ("nt-128x128", NT, 1, False),
             ("tn-64x64", TN, 0, False), ("tn-128x64", TN, 4, False), ("tn-128x128", TN, 1, False),
             ("nn-64x64", NN, 0, False), ("nn-128x128", NN, 1, False), ("fold-64x64", NT, 0, True)]
MAX_SEG = 10
MARGIN = 64                          # NaN floats in front of and behind every buffer
OUT_FILL = 0x7FC0BEEF                # the NaN every output buffer is filled with: what the launch does not write keeps these bits
BK = 32
E_DIMS = -2

# max over the group's cases of |x32 - ref| / (2^-24 S) for the float32 restatement, rounded up, on the host that wrote
# profiles/gemm_engine_edges.json (another CPU's BLAS sums in another order: test_recorded_float32_ratios_reproduce asks for the same size)
ORACLE32_RATIO = {"tiles": 5.7, "kinds": 6.5, "chains": 2.5, "groups": 6.4, "split": 3.4, "epilogue": 4.0, "fold": 3.9, "persistent": 3.2}
C_MARGIN = 4.0


def bound_c(group):
    return C_MARGIN * ORACLE32_RATIO[group]


# ---- the cases ---------------------------------------------------------------------------------------------------------------------------
CASES = []


def seg(klen, n_cols, a=PLAIN, b=PLAIN, split=1, a_off=0, b_off=0, stride=1):
    return dict(klen=klen, n_cols=n_cols, split=split, a=dict(kind=a, off=a_off, stride=stride), b=dict(kind=b, off=b_off, stride=stride))


def _case(group, tag, form, cfg, M, segs, mode=CHAIN, fold=None, epi=None, env=None, ldo_pad=3):
    """epi: rowadd=(rowdiv, ld pad) | bias=True | act=0/1/2 | dropout=("mask", p, ld pad) or ("gen", p, seed, layer) | gate=(ld pad, scale) |
    rowsplit_g=g.  fold: dict(div=fold_div).  ldo = n_cols + ldo_pad."""
    c = dict(group=group, id="%s-%s" % (group, tag), form=form, cfg=cfg, M=M, segs=segs, mode=mode, fold=fold, epi=dict(epi or {}),
             env=dict(env or {}), ldo_pad=ldo_pad)
    assert len(segs) <= MAX_SEG and cfg in SUPPORTED[form]
    CASES.append(c)
    return c


def op_shape(form, side, M, N, k):
    """(rows, cols) of the logical operand matrix."""
    if side == "a":
        return (k, M) if form == TN else (M, k)
    return (N, k) if form == NT else (k, N)


def colk(form, side):
    """The reduction index runs along the operand's columns."""
    return form != TN if side == "a" else form == NT


def n_problems(c):
    return len(c["segs"]) if c["mode"] == GROUP else 1


def problem_segs(c, p):
    return [p] if c["mode"] == GROUP else list(range(len(c["segs"])))


def expected_rc(c):
    """What ncx_diag_gemm answers for the case: NCX_E_DIMS when an operand is narrower than a 16-byte window, else 0."""
    for i, s in enumerate(c["segs"]):
        N = c["segs"][i if c["mode"] == GROUP else 0]["n_cols"]
        for side in "ab":
            if op_shape(c["form"], side, c["M"], N, s["klen"])[1] < 4:
                return E_DIMS
    return 0


def tile_shapes(bm, bn):
    return [(1, 4), (bm - 1, bn + 1), (bm, bn), (bm + 1, bn - 1), (2 * bm + 3, 5), (bm + 17, 2 * bn + 7)]


TILE_KLEN = (4, 5, 31, 32, 33, 64, 65, 103, 160)
TILE_KLEN_96x128 = (96, 97, 128, 129)            # with the above: nfast 0 .. 4 of the depth-2 loop, with and without a tail

# tiles: every instantiation at its tile edges and reduction lengths, plain operands, no epilogue; bases 0 .. 3 floats off 16 bytes
for _name, _form, _cfg, _fold in INSTANCES:
    _bm, _bn = TILE[_cfg]
    _n = 0
    for _M, _N in tile_shapes(_bm, _bn):
        for _k in TILE_KLEN + (TILE_KLEN_96x128 if _cfg == 2 else ()):
            _case("tiles", "%s-M%d-N%d-k%d" % (_name, _M, _N, _k), _form, _cfg, _M, [seg(_k, _N, a_off=_n % 4, b_off=(_n // 4 + 1) % 4)],
                  fold=dict(div=1) if _fold else None)
            _n += 1

# kinds: the four operand kinds where the form takes them (NT, NN: A; TN: B), through the generic and the fast k-loop (klen 103, 160:
# three / five full steps), idx_stride 3 on the longest
for _name, _form, _cfg, _fold in INSTANCES:
    if _fold:
        continue
    _bm, _bn = TILE[_cfg]
    for _kind in (PLAIN, GATHER, GMUL, SOFTMAX):
        for _k in (5, 33, 103, 160):
            _kw = dict(b=_kind, b_off=_kind) if _form == TN else dict(a=_kind, a_off=_kind)
            _case("kinds", "%s-%s-k%d" % (_name, KIND_NAME[_kind], _k), _form, _cfg, _bm + 17, [seg(_k, _bn + 7, stride=3 if _k == 160 else 1, **_kw)])
# both operands indirect: no fast k-loop serves the pair
_case("kinds", "nt-64x64-gmul-x-gather", NT, 0, 70, [seg(103, 37, a=GMUL, b=GATHER)])
_case("kinds", "tn-64x64-softmax-x-gmul", TN, 0, 70, [seg(103, 37, a=SOFTMAX, b=GMUL)])
_case("kinds", "nn-64x64-gather-x-softmax", NN, 0, 70, [seg(103, 37, a=GATHER, b=SOFTMAX)])

# chains: a segment switch on a full step, on a tail and on a 4-wide segment
CHAIN_KLEN = (36, 32, 5, 64, 33, 4, 96, 31, 65, 160)
CHAIN_KINDS = (PLAIN, GATHER, GMUL, SOFTMAX)
for _name, _form, _cfg, _fold in INSTANCES:
    if _fold:
        continue
    _bm, _bn = TILE[_cfg]
    for _ns in (2, 3, 10):
        _segs = []
        for _i in range(_ns):
            _kind = CHAIN_KINDS[_i % 4]
            _kw = dict(b=_kind) if _form == TN else dict(a=_kind)
            _segs.append(seg(CHAIN_KLEN[_i], _bn + 7, a_off=_i % 4, b_off=(_i + 2) % 4, **_kw))
        _case("chains", "%s-%d" % (_name, _ns), _form, _cfg, _bm + 17, _segs)

# groups: problems of differing n_cols, klen and kind behind one M
GROUP_NCOLS = (5, 64, 37, 130, 4, 65, 129, 63, 200, 33)
for _name, _form, _cfg, _fold in INSTANCES:
    if _fold or _cfg in (1, 2, 3):
        continue
    _bm, _bn = TILE[_cfg]
    for _ns in (3, 10):
        _segs = []
        for _i in range(_ns):
            _kind = CHAIN_KINDS[(_i + 1) % 4]
            _kw = dict(b=_kind) if _form == TN else dict(a=_kind)
            _segs.append(seg(CHAIN_KLEN[(_i + 3) % 10], GROUP_NCOLS[_i], a_off=(_i + 1) % 4, b_off=_i % 4, **_kw))
        _case("groups", "%s-%d" % (_name, _ns), _form, _cfg, _bm + 17, _segs, mode=GROUP)
_case("groups", "tn-128x128-3", TN, 1, 145, [seg(65, 135, b=GATHER), seg(160, 5, b=SOFTMAX), seg(33, 257, b=GMUL)], mode=GROUP)
_case("groups", "nn-128x128-3", NN, 1, 145, [seg(65, 135, a=GATHER), seg(160, 5, a=SOFTMAX), seg(33, 257, a=GMUL)], mode=GROUP)

# split: S k-chunks per tile and the fix-up behind them.  klen 330 = 11 k-steps: S = 16 and 24 leave chunks empty; 70 x 200 is 2 x 4 tiles of
# 64 x 64 (tiles_m < tiles_n), 200 x 70 the reverse, 70 x 190 = 2 x 3: with S = 2 and 4 the chunk-per-XCD layout pads (odd major count)
SPLIT_S = (2, 3, 4, 5, 8, 16, 24)
for _form in (NT, TN, NN):
    for _M, _N in ((70, 200), (200, 70), (70, 190)):
        for _S in SPLIT_S:
            _case("split", "%s-64x64-M%d-N%d-S%d" % (FORM_NAME[_form], _M, _N, _S), _form, 0, _M, [seg(330, _N, split=_S, a_off=_S % 4, b_off=(_S + 1) % 4)])
for _name, _form, _cfg, _fold in INSTANCES:
    if _fold or _cfg == 0:
        continue
    _bm, _bn = TILE[_cfg]
    for _S in (2, 3, 8):
        _case("split", "%s-S%d" % (_name, _S), _form, _cfg, _bm + 17, [seg(330, 2 * _bn + 7, split=_S)])
_case("split", "nt-64x64-chain-S3", NT, 0, 70, [seg(36, 100, split=3), seg(32, 100, a=GATHER), seg(5, 100, a=SOFTMAX), seg(64, 100, a=GMUL)])
_case("split", "nt-64x64-bias-relu-S4", NT, 0, 70, [seg(330, 100, split=4)], epi=dict(bias=True, act=1))
_case("split", "nt-64x64-bias-tanh-S5", NT, 0, 70, [seg(330, 100, split=5)], epi=dict(bias=True, act=2))
_case("split", "tn-128x64-bias-tanh-S8", TN, 4, 145, [seg(330, 100, split=8)], epi=dict(bias=True, act=2))
# a group mixing unsplit and split problems (dw1c_seg_split gives the narrow column blocks of the grouped dW1 launch splits of their own)
_case("split", "tn-128x64-group-mixed", TN, 4, 145, [seg(330, 135, b=GATHER, split=4), seg(160, 25, split=1), seg(330, 70, b=SOFTMAX, split=8), seg(65, 5, split=1),
                                                      seg(330, 64, b=GMUL, split=3)], mode=GROUP)
_case("split", "tn-64x64-group-mixed", TN, 0, 70, [seg(330, 135, split=1), seg(160, 25, split=5), seg(330, 70, b=GATHER, split=2)], mode=GROUP, epi=dict(bias=True))

# epilogue: each term alone and all together, leading dimensions wider than N, on the tile forms whose epilogue code differs (the 4 x 4
# block tile keeps its row-block loop rolled)
EPI_TERMS = dict(rowadd=dict(rowadd=(3, 5)), bias=dict(bias=True), relu=dict(act=1), tanh=dict(act=2), mask=dict(dropout=("mask", 0.5, 2)),
                 gen=dict(dropout=("gen", 0.25, 0x1234567890ABCDEF, 2)), gate=dict(gate=(7, 1.25)), rowsplit4=dict(rowsplit_g=4), rowsplit25=dict(rowsplit_g=25))
EPI_ALL = dict(rowadd=(3, 5), bias=True, act=1, dropout=("mask", 0.5, 2), gate=(7, 1.25), rowsplit_g=4)
EPI_ALL_GEN = dict(rowadd=(3, 5), bias=True, act=2, dropout=("gen", 0.25, 0xFEDCBA9876543210, 3), gate=(7, 2.0), rowsplit_g=25)
for _t, _e in EPI_TERMS.items():
    _case("epilogue", "nt-64x64-%s" % _t, NT, 0, 81, [seg(65, 71)], epi=_e, ldo_pad=6)
for _name, _form, _cfg, _fold in INSTANCES:
    if _fold:
        continue
    _bm, _bn = TILE[_cfg]
    _case("epilogue", "%s-all" % _name, _form, _cfg, _bm + 17, [seg(65, _bn + 7)], epi=EPI_ALL, ldo_pad=6)
    _case("epilogue", "%s-all-gen" % _name, _form, _cfg, _bm + 17, [seg(33, _bn + 7)], epi=EPI_ALL_GEN, ldo_pad=6)
_case("epilogue", "tn-64x64-group-all", TN, 0, 81, [seg(65, 71), seg(33, 5, b=GATHER), seg(5, 130)], mode=GROUP, epi=dict(bias=True, act=1, gate=(7, 1.25)))

# fold: the FOLD recurrence (the MUTAN fusion: R pairs, fold_div = rowsplit_g = K + 1)
for _R in (1, 2, 10):
    for _div in (1, 25):
        for _M in (63, 64, 65):
            _case("fold", "R%d-div%d-M%d" % (_R, _div, _M), NT, 0, _M, [seg((36, 64, 5)[(_i + _R) % 3] if _R > 1 else 36, 70, a_off=_i % 4) for _i in range(_R)],
                  fold=dict(div=_div), epi=dict(rowsplit_g=25) if _div == 25 else {})

# persistent: more than twice the resident slots in work items under the opt-in persistent loop
_case("persistent", "nt-64x64-M2561-N2561-k4", NT, 0, 2561, [seg(4, 2561)], env={"NCX_EXPERIMENT": "1", "NCX_PERSISTENT": "1"})

BY_ID = {c["id"]: c for c in CASES}
GROUPS = sorted({c["group"] for c in CASES})
assert len(BY_ID) == len(CASES)


def instance_of(c):
    for name, form, cfg, fold in INSTANCES:
        if form == c["form"] and cfg == c["cfg"] and fold == bool(c["fold"]):
            return name
    raise KeyError(c["id"])


# ---- the inputs --------------------------------------------------------------------------------------------------------------------------
def _padded(values, ld, off, dtype=np.float32):
    """values [R, C] -> (flat buffer, first element): rows `ld` apart, NaN (ints: 0) in the gaps and in MARGIN + off elements around."""
    R, C = values.shape
    fill = np.nan if dtype == np.float32 else 0
    buf = np.full(MARGIN + off + R * ld + MARGIN, fill, dtype)
    buf[MARGIN + off:MARGIN + off + R * ld].reshape(R, ld)[:, :C] = values
    return buf, MARGIN + off


def view(buf, base, R, ld, C):
    return buf[base:base + R * ld].reshape(R, ld)[:, :C]


class Inputs:
    """bufs: name -> (flat numpy buffer, index of its first element).  ops[i][side]: the operand's description."""

    def __init__(self):
        self.bufs, self.ops, self.out = {}, [], []


def build(c):
    """The host arrays of a case, seeded by its id.  Every float buffer sits between NaN margins with NaN in the gap ld - cols; gather
    tables keep a NaN row 0 that no id names, ids repeat and name the table's last row, the entries a stride skips name row 0."""
    rng = np.random.default_rng(zlib.crc32(c["id"].encode()))
    X = Inputs()
    M, form = c["M"], c["form"]
    for i, s in enumerate(c["segs"]):
        N = c["segs"][i if c["mode"] == GROUP else 0]["n_cols"]
        ops = {}
        for side in "ab":
            o, name = s[side], "%s%d" % (side, i)
            rows, cols = op_shape(form, side, M, N, s["klen"])
            ld = cols + 3 + (i + (side == "b")) % 3
            d = dict(kind=o["kind"], rows=rows, cols=cols, ld=ld, stride=o["stride"], name=name)
            if o["kind"] in (GATHER, GMUL):
                T = rows + 5
                table = (rng.standard_normal((T, cols)) * 0.5).astype(np.float32)
                table[0] = np.nan
                X.bufs[name] = _padded(table, ld, o["off"])
                for key in ("idx", "idx2")[:1 + (o["kind"] == GMUL)]:
                    ids = rng.integers(1, T, size=rows)
                    ids[0] = T - 1
                    if rows > 2:
                        ids[rows - 1] = ids[1]
                    flat = np.zeros((rows, o["stride"]), np.int32)
                    flat[:, 0] = ids
                    X.bufs[name + "." + key] = (flat.reshape(-1).copy(), 0)
                d["T"] = T
            elif o["kind"] == SOFTMAX:
                logits = (rng.standard_normal((rows, cols)) * 1.5).astype(np.float32)
                lse = np.log2(np.exp(logits.astype(np.float64)).sum(1)).astype(np.float32)
                X.bufs[name] = _padded(logits, ld, o["off"])
                X.bufs[name + ".lse"] = _padded(lse[None, :], rows, 1)
            else:
                X.bufs[name] = _padded((rng.standard_normal((rows, cols)) * 0.5).astype(np.float32), ld, o["off"])
            ops[side] = d
        X.ops.append(ops)
    e, n_max = c["epi"], max(s["n_cols"] for s in c["segs"][:n_problems(c)])
    if e.get("rowadd"):
        div, pad = e["rowadd"]
        X.bufs["rowadd"] = _padded(rng.standard_normal((-(-M // div), n_max)).astype(np.float32), n_max + pad, 1)
    if e.get("bias"):
        X.bufs["bias"] = _padded(rng.standard_normal((1, n_max)).astype(np.float32), n_max, 3)
    if e.get("dropout") and e["dropout"][0] == "mask":
        X.bufs["mask"] = _padded((rng.random((M, n_max)) >= e["dropout"][1]).astype(np.float32), n_max + e["dropout"][2], 2)
    if e.get("gate"):
        X.bufs["gate"] = _padded(rng.standard_normal((M, n_max)).astype(np.float32), n_max + e["gate"][0], 1)
    if c["fold"]:
        R, N = len(c["segs"]), c["segs"][0]["n_cols"]
        X.bufs["fold_mul"] = _padded(rng.standard_normal((-(-M // c["fold"]["div"]), R * N)).astype(np.float32), R * N + 5, 1)
        X.bufs["fold_bias"] = _padded((rng.standard_normal((1, R * N)) * 0.3).astype(np.float32), R * N, 2)
    # outputs: [rows][ldo] per problem; rowsplit_g = g sends row g b to out0[b] and the others, closed up, to out
    g = e.get("rowsplit_g", 0)
    for p in range(n_problems(c)):
        N = c["segs"][p]["n_cols"]
        rows0 = -(-M // g) if g else 0
        X.out.append(dict(N=N, ldo=N + c["ldo_pad"], rows=M - rows0, rows0=rows0, ldo0=N + 1))
    return X


def drop_scale(p):
    return float(np.float32(1.0) / (np.float32(1.0) - np.float32(p)))


def keep_matrix(c, X, N):
    """The keep decisions [M, N] of the case's dropout (None: no dropout)."""
    d = c["epi"].get("dropout")
    if not d:
        return None
    if d[0] == "mask":
        buf, base = X.bufs["mask"]
        n_max = max(s["n_cols"] for s in c["segs"][:n_problems(c)])
        return view(buf, base, c["M"], n_max + d[2], N) != 0
    from oracle import ncx_oracle                # (conftest.py puts the repository root on sys.path)
    return ncx_oracle.dropout_keep_mask(d[2], d[3], c["M"], N, d[1]).numpy() != 0


# ---- the restatement (dtype = float64: the reference, with S; float32: the source of c) --------------------------------------------------------
def dense(X, i, side, dtype=np.float64, mut=None):
    """-> (x [rows, cols] in dtype, w: |x|, a softmax factor times (1 + |its exp2 argument|)) of operand `side` of pair i."""
    d = X.ops[i][side]
    buf, base = X.bufs[d["name"]]
    if d["kind"] in (GATHER, GMUL):
        st = view(buf, base, d["T"], d["ld"], d["cols"]).astype(dtype)
        x = st[X.bufs[d["name"] + ".idx"][0].reshape(d["rows"], d["stride"])[:, 0]]
        if d["kind"] == GMUL:
            x = x * st[X.bufs[d["name"] + ".idx2"][0].reshape(d["rows"], d["stride"])[:, 0]]
        w = np.abs(x)
    elif d["kind"] == SOFTMAX:
        lbuf, lbase = X.bufs[d["name"] + ".lse"]
        lse = lbuf[lbase:lbase + d["rows"]].astype(dtype)
        arg = view(buf, base, d["rows"], d["ld"], d["cols"]).astype(dtype) * dtype(LOG2E) - lse[:, None]
        x = np.exp2(arg)
        w = x * (1 + np.abs(arg))
    else:
        x = view(buf, base, d["rows"], d["ld"], d["cols"]).astype(dtype)
        w = np.abs(x)
    if mut and mut[0] == "shift_window" and mut[1] == (i, side):      # the row's last 16-byte window read one element to the left
        x = x.copy()
        x[:, d["cols"] - 3:] = x[:, d["cols"] - 4:-1]
    return x, w


def _prod(form, A, B):
    return A @ B.T if form == NT else A.T @ B if form == TN else A @ B


def _kslice(form, side, x, k0, k1):
    return x[:, k0:k1] if colk(form, side) else x[k0:k1]


def chunk_steps(c, p):
    """The k-steps (pair, k0, k1) of problem p, and per chunk z of its split S the range of them it sums."""
    steps = [(i, k0, min(k0 + BK, c["segs"][i]["klen"])) for i in problem_segs(c, p) for k0 in range(0, c["segs"][i]["klen"], BK)]
    S = max(c["segs"][p]["split"], 1)
    T = len(steps)
    return steps, [(T * z // S, T * (z + 1) // S) for z in range(S)]


def raw_product(c, X, p, dtype=np.float64, mut=None):
    """Problem p before the epilogue -> (P [M, N], S [M, N]).  Unsplit: one product per pair; split: one per chunk and pair, chunks summed z
    ascending like the fix-up."""
    form = c["form"]
    segs = problem_segs(c, p)
    if mut and mut[0] == "skip_seg":
        segs = [i for i in segs if i != mut[1]]
    ops = {i: (dense(X, i, "a", dtype, mut), dense(X, i, "b", dtype, mut)) for i in segs}
    M, N = c["M"], c["segs"][p]["n_cols"]
    split = max(c["segs"][p]["split"], 1)
    if c["fold"]:
        fm_buf, fm_base = X.bufs["fold_mul"]
        fb_buf, fb_base = X.bufs["fold_bias"]
        R, div = len(c["segs"]), c["fold"]["div"]
        fm = view(fm_buf, fm_base, -(-M // div), R * N + 5, R * N).astype(dtype)[np.arange(M) // div]
        fb = fb_buf[fb_base:fb_base + R * N].astype(dtype)
        P, S = np.zeros((M, N), dtype), np.zeros((M, N), dtype)
        for i in segs:
            (a, aw), (b, bw) = ops[i]
            P = P + (_prod(form, a, b) + fb[i * N:(i + 1) * N]) * fm[:, i * N:(i + 1) * N]
            S = S + (_prod(form, aw, bw) + np.abs(fb[i * N:(i + 1) * N])) * np.abs(fm[:, i * N:(i + 1) * N])
        return P, S
    P, S = np.zeros((M, N), dtype), np.zeros((M, N), dtype)
    if split == 1:
        for i in segs:
            (a, aw), (b, bw) = ops[i]
            P = P + _prod(form, a, b)
            S = S + _prod(form, aw, bw)
    else:
        steps, chunks = chunk_steps(c, p)
        for z, (s0, s1) in enumerate(chunks):
            if mut and mut[0] == "chunk_omit" and mut[1] == z:
                continue
            part, spart = np.zeros((M, N), dtype), np.zeros((M, N), dtype)
            for i in sorted({st[0] for st in steps[s0:s1]}):
                if i not in ops:
                    continue
                ks = [st for st in steps[s0:s1] if st[0] == i]
                k0, k1 = ks[0][1], ks[-1][2]
                (a, aw), (b, bw) = ops[i]
                part = part + _prod(form, _kslice(form, "a", a, k0, k1), _kslice(form, "b", b, k0, k1))
                spart = spart + _prod(form, _kslice(form, "a", aw, k0, k1), _kslice(form, "b", bw, k0, k1))
            rep = 2 if mut and mut[0] == "chunk_twice" and mut[1] == z else 1
            for _ in range(rep):
                P = P + part
            S = S + spart
    if mut and mut[0] == "drop_k":                  # one term a(r, k) b(n, k) of pair i left out
        _, i, r, n, k = mut
        (a, _), (b, _) = ops[i]
        ar = a[r, k] if colk(form, "a") else a[k, r]
        bn = b[n, k] if colk(form, "b") else b[k, n]
        P[r, n] -= ar * bn
    if mut and mut[0] == "lose_row":
        P[mut[1]] = 0
    if mut and mut[0] == "lose_col":
        P[:, mut[1]] = 0
    return P, S


EPI_ORDER = ("rowadd", "bias", "act", "dropout", "gate")


def epilogue(c, X, p, P, S, dtype=np.float64, order=EPI_ORDER):
    e, M, N = c["epi"], c["M"], c["segs"][p]["n_cols"]
    n_max = max(s["n_cols"] for s in c["segs"][:n_problems(c)])
    v, S = P, S
    for term in order:
        if term == "rowadd" and e.get("rowadd"):
            div, pad = e["rowadd"]
            buf, base = X.bufs["rowadd"]
            ra = view(buf, base, -(-M // div), n_max + pad, N).astype(dtype)[np.arange(M) // div]
            v, S = v + ra, S + np.abs(ra)
        elif term == "bias" and e.get("bias"):
            buf, base = X.bufs["bias"]
            b = buf[base:base + N].astype(dtype)
            v, S = v + b, S + np.abs(b)
        elif term == "act" and e.get("act") == 1:
            v = np.maximum(v, 0)
        elif term == "act" and e.get("act") == 2:
            v = np.tanh(v)
            S = S + np.abs(v)
        elif term == "dropout" and e.get("dropout"):
            keep = keep_matrix(c, X, N)
            sc = dtype(drop_scale(e["dropout"][1]))
            v, S = np.where(keep, v * sc, 0).astype(dtype), np.where(keep, S * sc, 0)
        elif term == "gate" and e.get("gate"):
            pad, gs = e["gate"]
            buf, base = X.bufs["gate"]
            on = view(buf, base, M, n_max + pad, N) > 0
            v, S = np.where(on, v * dtype(gs), 0).astype(dtype), np.where(on, S * gs, 0)
    return v, S


def restate(c, X, dtype=np.float64, mut=None, order=EPI_ORDER):
    """-> per problem (value [M, N], S [M, N]) as the launch defines them."""
    out = []
    for p in range(n_problems(c)):
        P, S = raw_product(c, X, p, dtype, mut)
        out.append(epilogue(c, X, p, P, S, dtype, order))
    return out


def ratio(got, ref, S):
    """max |got - ref| / (2^-24 S) over the elements; an element whose S is 0 must be exact, and nothing may be NaN."""
    got = np.asarray(got, np.float64).reshape(ref.shape)
    assert np.isfinite(got).all(), "non-finite output"
    err = np.abs(got - ref)
    assert (err[S == 0] == 0).all(), "an element with S = 0 is not exact"
    if not (S > 0).any():
        return 0.0
    return float((err[S > 0] / (U24 * S[S > 0])).max())


def float32_ratio(c, X=None):
    """The float32 restatement's worst ratio on one case."""
    X = X or build(c)
    ref = restate(c, X)
    x32 = restate(c, X, np.float32)
    return max(ratio(g[0], r[0], r[1]) for g, r in zip(x32, ref))


# ---- the launch description ----------------------------------------------------------------------------------------------------------------
def out_rows_map(c, p, X):
    """Where logical row r of problem p lands: (in_out0 [M] bool, row [M])."""
    M, g = c["M"], c["epi"].get("rowsplit_g", 0)
    r = np.arange(M)
    if not g:
        return np.zeros(M, bool), r
    b, j = r // g, r % g
    return j == 0, np.where(j == 0, b, b * (g - 1) + j - 1)


def fill_args(c, X, addr, no_fast=False, slab=0, slab_bytes=0):
    """ncx_diag_gemm_args of the case.  addr(name) -> address of element 0 of buffer `name` (inputs: X.bufs; outputs: "out<p>", "outz<p>",
    whose first MARGIN floats are margin)."""
    from neuralcx import _lib
    a = _lib.NcxDiagGemmArgs()
    ptr = lambda name: addr(name) + 4 * X.bufs[name][1]
    a.form, a.cfg, a.mode, a.nseg, a.M, a.fold, a.no_fast = c["form"], c["cfg"], c["mode"], len(c["segs"]), c["M"], 1 if c["fold"] else 0, int(no_fast)
    for i, s in enumerate(c["segs"]):
        for side in "ab":
            d, o = X.ops[i][side], getattr(a, side)[i]
            o.base, o.ld, o.kind, o.rows, o.cols, o.idx_stride = ptr(d["name"]), d["ld"], d["kind"], d["rows"], d["cols"], d["stride"]
            if d["kind"] in (GATHER, GMUL):
                o.idx = ptr(d["name"] + ".idx")
            if d["kind"] == GMUL:
                o.idx2 = ptr(d["name"] + ".idx2")
            if d["kind"] == SOFTMAX:
                o.lse2 = ptr(d["name"] + ".lse")
        a.klen[i] = s["klen"]
    e = c["epi"]
    n_max = max(s["n_cols"] for s in c["segs"][:n_problems(c)])
    for p, o in enumerate(X.out):
        a.n_cols[p], a.split[p], a.ldo[p] = o["N"], c["segs"][p]["split"], o["ldo"]
        a.out[p] = addr("out%d" % p) + 4 * MARGIN
    if e.get("rowadd"):
        a.rowadd, a.ld_rowadd, a.rowdiv = ptr("rowadd"), n_max + e["rowadd"][1], e["rowadd"][0]
    if e.get("bias"):
        a.bias = ptr("bias")
    a.act = e.get("act", 0)
    d = e.get("dropout")
    if d:
        a.drop_p, a.drop_scale = d[1], drop_scale(d[1])
        if d[0] == "mask":
            a.dropout, a.keep_mask, a.ld_mask = 2, ptr("mask"), n_max + d[2]
        else:
            a.dropout, a.seed_lo, a.seed_hi, a.layer = 1, d[2] & 0xFFFFFFFF, d[2] >> 32, d[3]
    if e.get("gate"):
        a.gate, a.ld_gate, a.gate_scale = ptr("gate"), n_max + e["gate"][0], e["gate"][1]
    if c["fold"]:
        R, N = len(c["segs"]), c["segs"][0]["n_cols"]
        a.fold_mul, a.fold_bias, a.ld_fold, a.fold_div = ptr("fold_mul"), ptr("fold_bias"), R * N + 5, c["fold"]["div"]
    if e.get("rowsplit_g"):
        a.rowsplit_g, a.out0, a.ldo0 = e["rowsplit_g"], addr("outz0") + 4 * MARGIN, X.out[0]["ldo0"]
    a.slab, a.slab_bytes = slab, slab_bytes
    return a


def fake_addr(name):
    """Addresses for the host-only entries, which never follow them."""
    return 1 << 20


def wgmap_count(tiles_m, tiles_n, S):
    """WgMap::count (csrc/ncx_gemm.h): workgroup ids of a problem, padding ids of the chunk-per-XCD layout included."""
    if S > 1 and 8 % S == 0 and S != 8:
        g = 8 // S
        return 8 * min(tiles_m, tiles_n) * -(-max(tiles_m, tiles_n) // g)
    return tiles_m * tiles_n * S


def work_items(c):
    """Work items of the case's GEMM launch (gemm_layout): the workgroup ids of every problem, padding ids included."""
    bm, bn = TILE[c["cfg"]]
    return sum(wgmap_count(-(-c["M"] // bm), -(-c["segs"][p]["n_cols"] // bn), max(c["segs"][p]["split"], 1)) for p in range(n_problems(c)))


def slab_floats(c):
    """What a split launch of the case needs: [workgroup ids of every problem][BM BN] (0: nothing is split)."""
    bm, bn = TILE[c["cfg"]]
    np_ = n_problems(c)
    if not any(c["segs"][p]["split"] > 1 for p in range(np_)):
        return 0
    return sum(wgmap_count(-(-c["M"] // bm), -(-c["segs"][p]["n_cols"] // bn), max(c["segs"][p]["split"], 1)) for p in range(np_)) * bm * bn


def kernel_k_order(K):
    """The order in which seg_gemm_kernel adds the K terms of one pair to an accumulator: per 32-deep step, sub-step t = 0 .. 3, e = 0, 1,
    one MFMA takes k = 8 t + 2 lk + e from the lane groups lk = 0 .. 3 (read_frags / mfma_frags, csrc/ncx_gemm.h)."""
    ks = [s + 8 * t + 2 * lk + e for s in range(0, K, BK) for t in range(4) for e in range(2) for lk in range(4)]
    return [k for k in ks if k < K]


def same_k_order(c):
    """Whether the fast and the generic k-loop sum every element's terms in the same order.  Both walk the k-steps of a chunk in order and
    feed the MFMAs of a step in the order k = 8 t + 2 (lane group) + e; the fast loop only changes when loads are issued and tiles
    stored.  So the order is the same for every case: no_fast on and off must agree bit for bit."""
    return True
