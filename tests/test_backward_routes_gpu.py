"""GPU: every route of linear_1's weight gradient against the oracle, at the shapes that pick it.

The planner routes the v columns to a per-triplet fold kernel (k_dw_km8, k_dw_km_x6, k_dw_km) or the grouped generic GEMM; dGt and every
other column block to one balanced TN launch (k_dw_tn8, k_dw_tn8_x6) or the grouped GEMM; dW1[:, a_other] to the TN kernel or the chain
GEMM.  Every parity case first asks the planner which route it takes (ncx_plan_query, NCX_QUERY_DW1_ROUTE) and asserts the one named in
its id: a case that lands on the generic engine by accident fails.  Bounds are the suite's (test_hip_parity): logits <= 1e-4, loss <= 1e-5,
every gradient <= 1e-4 of its tensor's max with no floor, ranks exact away from near-ties.
"""
import os
import re

import pytest

from oracle import ncx_oracle as orc
from helpers import GOLDEN, check_phased_backward_bit_identical, compare_with_oracle, full_size_case

pytestmark = pytest.mark.gpu

LESION = dict(orc.DEFAULT_SPEC, a_emb=False)
_CASES = {}      # conditioned inputs and the oracle's result per case: the X6 copies compare against the same reference
# Distance from the ReLU kinks the inputs are conditioned to, on every hidden layer.  The suite's 2e-5 (set at H = 256, L = 1) flags nearly
# every batch row at H = 1024 with two layers (49 152 pre-activations per row), so no row could be drawn; 2e-6 is still well above the fp32
# rounding of a pre-activation at these widths.
TAU = 2e-6


def _x6():
    from neuralcx import _lib, ops
    return bool(ops.EXTRA_FLAGS & _lib.NCX_F_X6)


def route(d, B, spec=None):
    """The planner's DW1_ROUTE answer for a backward of batch B (the dims make_dims builds for the tests' dense batches)."""
    from neuralcx import _lib, ops
    n = _lib.NcxDims()
    n.B, n.K, n.dv, n.dq, n.dz, n.da, n.A, n.H, n.L = B, d.K, d.dv, d.dq, d.dz, d.da, d.A, d.H, d.L
    n.n_img = B * (d.K + 1)
    n.flags = ops.flags_from_spec(spec) | ops.EXTRA_FLAGS
    return _lib.plan_query(n, "DW1_ROUTE")


def expect(d, B, spec, fold, tn):
    """Assert the route: fold in ("fold8", "km", "grouped"), tn in ("tn8", "grouped"); fold8 / tn8 name the 8-wave kernels, whose
    three-plane copies run under NCX_F_X6 (the TN one up to B = 2048)."""
    r = route(d, B, spec)
    x6 = _x6()
    want_fold = {"fold8": "k_dw_km_x6" if x6 else "k_dw_km8", "km": "k_dw_km", "grouped": "grouped"}[fold]
    want_tn = {"tn8": "k_dw_tn8_x6" if x6 and B <= 2048 else "k_dw_tn8", "grouped": "grouped"}[tn]
    assert (r["fold"], r["tn"]) == (want_fold, want_tn), r
    aemb = spec is None or spec.get("a_emb", True)
    assert r["a_other_on_tn"] == (tn == "tn8" and aemb), r
    if tn == "tn8":
        assert 1 <= r["tn_pieces"] <= r["tn_max_pieces"], r
    return r


def _reference_option(name):
    """dim_h and n_layers of one of the reference's option files (tests/golden/g9_reference_options_cx)."""
    txt = open(os.path.join(GOLDEN, "g9_reference_options_cx", name + ".yaml")).read()
    return int(re.search(r"\n\s+dim_h:\s*(\d+)", txt).group(1)), int(re.search(r"\n\s+n_layers:\s*(\d+)", txt).group(1))


def _run(key, d, B, seed, spec=None):
    """Compare the HIP path with the oracle on conditioned inputs (built once per key)."""
    if key not in _CASES:
        aemb = spec is None or spec.get("a_emb", True)
        params, batch = full_size_case(d, B, seed, a_emb=aemb, tau=TAU)
        extra = {} if aemb else {"a_emb_gt": batch.pop("a_emb_gt")}
        ob = dict(batch, **extra)
        _CASES[key] = (params, batch, extra, orc.loss_and_grads(params, d, ob, spec=spec))
    params, batch, extra, ref = _CASES[key]
    compare_with_oracle(d, spec, params, batch, extra=extra or None, ref=ref)


@pytest.fixture
def x6(monkeypatch):
    from neuralcx import _lib, ops
    monkeypatch.setattr(ops, "EXTRA_FLAGS", _lib.NCX_F_X6)


# ---- a. the reference's own configs at their widths ---------------------------------------------------------------------------------------
# B = 64 as shipped (fast forward, generic backward); B = 512, the bench batch: the fold and TN kernels with 2 (H = 512) or 4 (H = 1024) row tiles
CONFIGS = [("neuralcx_512_1_all", 64, "grouped", "grouped"), ("neuralcx_512_2_all", 64, "grouped", "grouped"),
           ("neuralcx_1024_1_all", 64, "grouped", "grouped"), ("neuralcx_1024_2_all", 64, "grouped", "grouped"),
           ("neuralcx_512_1_all", 512, "fold8", "tn8"), ("neuralcx_512_2_all", 512, "fold8", "tn8"),
           ("neuralcx_1024_1_all", 512, "fold8", "tn8"), ("neuralcx_1024_2_all", 512, "fold8", "tn8")]


def _config_case(name, B, fold, tn):
    H, L = _reference_option(name)
    d = orc.Dims(H=H, L=L)
    expect(d, B, None, fold, tn)
    _run((name, B), d, B, 5000 + H + 10 * L + B)


@pytest.mark.parametrize("name,B,fold,tn", CONFIGS, ids=["%s-B%d-%s-%s" % c for c in CONFIGS])
def test_reference_config_widths_vs_oracle(name, B, fold, tn):
    """The reference's neuralcx_{512,1024}_{1,2}_all at full widths (dv 2048, dq 2400, dz 360, da 2400, A 2000), L up to 2."""
    _config_case(name, B, fold, tn)


@pytest.mark.parametrize("name,B,fold,tn", [c for c in CONFIGS if c[1] == 512], ids=["%s-B%d-%s-%s" % c for c in CONFIGS if c[1] == 512])
def test_x6_reference_config_widths_vs_oracle(name, B, fold, tn, x6):
    _config_case(name, B, fold, tn)


def test_counterexamples_default_width_general_fold_vs_oracle():
    """counterexamples_default's dim_h = 300 (not a multiple of 256) at full widths, L = 1, B = 256: the general k_dw_km fold
    (ragged row tiles) and the grouped GEMM for everything else."""
    H, _ = _reference_option("counterexamples_default")
    d = orc.Dims(H=H, L=1)
    expect(d, 256, None, "km", "grouped")
    _run("cx_default", d, 256, 300)


def test_three_hidden_layers_full_width_vs_oracle():
    """H = 256, L = 3 at full widths, B = 256: the fold and TN kernels under two hidden layers' chain (conditioned on every layer)."""
    d = orc.Dims(H=256, L=3)
    expect(d, 256, None, "fold8", "tn8")
    _run("L3", d, 256, 333)


# ---- b. plans with more pieces per workgroup than the TN kernel's table: the grouped GEMM (these raised NCX_E_DIMS before) -----------------
OVERFLOW = [("a_emb_lesion-K24-H1024", 24, 1024, LESION), ("full-K48-H2048", 48, 2048, None)]


@pytest.mark.parametrize("K,H,spec", [o[1:] for o in OVERFLOW], ids=[o[0] for o in OVERFLOW])
def test_tn_plan_overflow_falls_back_to_grouped_vs_oracle(K, H, spec):
    """At full widths and B = 128 the balanced TN plan needs more than TN8_MAX_SEG pieces per workgroup (the a_emb lesion puts the
    2400-column a_other block in the rest sequence; K = 48 doubles the candidate rows): the planner keeps those products, the shared
    segments and dW1[:, a_other] on the generic engine, and the gradient is right."""
    d = orc.Dims(K=K, H=H)
    r = expect(d, 128, spec, "grouped", "grouped")
    assert r["tn_pieces"] > r["tn_max_pieces"], r
    _run(("overflow", K, H), d, 128, 7000 + K + H, spec)


# ---- c. the piece limit at its edge (reduced widths; the CU count is the device's) ---------------------------------------------------------
def _edge_widths():
    """The widest da (a multiple of 64) whose plan needs exactly the limit of pieces, and the next one (over it)."""
    d0 = orc.Dims(K=48, dv=128, dq=64, dz=64, A=40, H=768)
    last = None
    for da in range(64, 8192 + 1, 64):
        r = route(orc.Dims(**dict(d0.__dict__, da=da)), 128, LESION)
        if r["tn_pieces"] > r["tn_max_pieces"]:
            assert last is not None and route(orc.Dims(**dict(d0.__dict__, da=last)), 128, LESION)["tn_pieces"] == r["tn_max_pieces"], (last, r)
            return last, da
        last = da
    raise AssertionError("no da up to 8192 overflows the TN plan")


def _edge_case(side):
    fits, over = _edge_widths()
    da = fits if side == "fits" else over
    d = orc.Dims(K=48, dv=128, dq=64, dz=64, da=da, A=40, H=768)
    expect(d, 128, LESION, "grouped", "tn8" if side == "fits" else "grouped")
    _run(("edge", side, da), d, 128, 8000 + da, LESION)


@pytest.mark.parametrize("side", ["fits", "over"])
def test_tn_piece_limit_edge_vs_oracle(side):
    """a_emb lesion, K = 48, H = 768 (three row tiles), B = 128, da varied: at the widest da whose plan needs exactly TN8_MAX_SEG pieces the
    TN launch runs; one column tile more and the products go to the grouped GEMM.  Both against the oracle."""
    _edge_case(side)


@pytest.mark.parametrize("side", ["fits", "over"])
def test_x6_tn_piece_limit_edge_vs_oracle(side, x6):
    _edge_case(side)


# ---- d. batch edges of the predicates (reduced widths) -------------------------------------------------------------------------------------
BATCH_EDGES = [(96, 24, "grouped", "grouped"),     # below the TN minimum
               (128, 24, "grouped", "tn8"),        # TN minimum; fold needs B >= 256
               (160, 24, "grouped", "tn8"),
               (256, 24, "fold8", "tn8"),          # the fold kernel joins
               (4096, 24, "fold8", "tn8"),         # TN maximum: the LDS index tables are largest
               (4128, 24, "fold8", "grouped"),     # past it: the grouped GEMM
               (256, 32, "grouped", "tn8")]        # K % 24 != 0: no fold, TN on


@pytest.mark.parametrize("B,K,fold,tn", BATCH_EDGES, ids=["B%d-K%d-%s-%s" % e for e in BATCH_EDGES])
def test_batch_edges_of_the_routes_vs_oracle(B, K, fold, tn):
    """dv = dq = dz = da = 64, A = 40, H = 256 at the batch sizes where a predicate changes its answer."""
    d = orc.Dims(K=K, dv=64, dq=64, dz=64, da=64, A=40, H=256)
    expect(d, B, None, fold, tn)
    _run(("batch", B, K), d, B, 9000 + B + K)


@pytest.mark.parametrize("B", [2048, 2080])
def test_x6_batch_edge_of_the_three_plane_tn_kernel_vs_oracle(B, x6):
    """Under NCX_F_X6 the TN launch takes k_dw_tn8_x6 up to B = 2048 (TN6_MAX_B) and the plain k_dw_tn8 above, inside an X6 run."""
    d = orc.Dims(K=24, dv=64, dq=64, dz=64, da=64, A=40, H=256)
    r = expect(d, B, None, "fold8", "tn8")
    assert r["tn"] == ("k_dw_tn8_x6" if B <= 2048 else "k_dw_tn8")
    _run(("batch", B, 24), d, B, 9000 + B + 24)


# ---- e. the phased backward on the new routes ----------------------------------------------------------------------------------------------
PHASED = [("fallback-K48-H2048-B128", 48, 2048, 1, 128, "grouped", "grouped"), ("tn8-H1024-L2-B512", 24, 1024, 2, 512, "fold8", "tn8")]


@pytest.mark.parametrize("K,H,L,B,fold,tn", [p[1:] for p in PHASED], ids=[p[0] for p in PHASED])
def test_phased_backward_is_bit_identical_on_wide_routes(K, H, L, B, fold, tn):
    """Phases 1 | 2, 3 | 4 and 5 | 2 | 4 equal the one-call backward bit for bit where the TN plan overflows (full model, K = 48, H = 2048)
    and at neuralcx_1024_2's shape on the TN and fold kernels."""
    d = orc.Dims(K=K, H=H, L=L)
    expect(d, B, None, fold, tn)
    params, batch = full_size_case(d, B, 11000 + H, tau=TAU)
    check_phased_backward_bit_identical(d, params, batch)
