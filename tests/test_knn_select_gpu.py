"""ncx_knn against the fp64 reference of tests/knn_ref.py on the tables that drive every path of the selector: each
refinement depth, outlier rows, signed and offset features, near-duplicate clusters, exact ties at the candidate cut and
beyond the buffer, the edges of n / k / dv / query blocks, and non-finite input.  Every row of every case is held to the
tau rule, and to the exact order wherever the inputs guarantee it (knn_ref.assert_exact_index_precondition)."""
import importlib.util
import os

import numpy as np
import pytest
import torch

import knn_ref as R
from conftest import PKG

pytestmark = pytest.mark.gpu


def _knn(c, **kw):
    from neuralcx.knn import knn
    q = None if c["q"] is None else torch.from_numpy(c["q"]).cuda()
    idx, dist = knn(torch.from_numpy(c["x"]).cuda(), k=c["k"], queries=q, **kw)
    return idx.cpu().numpy(), dist.cpu().numpy()


def _check(name):
    c = R.case(name)
    idx, dist = _knn(c)
    excess, tau = R.check_knn(idx, dist, c["queries"], c["x"], c["k"], c["exact"], c["d2"], c["order"])
    print("knn %s: largest d2 - D_k %.4g, smallest tau %.4g, exact-order rows %d of %d" % (
        name, excess, tau, int(c["exact"].sum()), c["exact"].size))
    return c, idx, dist


@pytest.mark.parametrize("name", ["depth_a", "depth_b", "depth_c", "depth_d", "depth_e", "depth_three"])
def test_refinement_depth(name):
    """One, two and three levels of the histogram select; (c)-(e) and `three` through outlier rows, whose own queries must
    return themselves first at distance 0."""
    c, idx, dist = _check(name)
    for r in c.get("outliers", ()):
        assert idx[r, 0] == r and dist[r, 0] == 0.0, (r, idx[r], dist[r])


def test_refinement_exhausted_raises():
    """Distinct products still overflow the candidate buffer after the last level: an error, never a plausible answer."""
    from neuralcx import _lib
    c = R.case("depth_exhausted")
    with pytest.raises(_lib.NcxError):
        _knn(c)
    _check("depth_a")                                                   # the next call starts clean


def test_products_overflowing_fp32_raise():
    """A finite table whose products q.x - |x|^2/2 leave fp32 (features ~1e20): an error, never a plausible answer."""
    from neuralcx import _lib
    from neuralcx.knn import knn
    x = R.lattice(9, 300, 64) * np.float32(1e20)
    assert np.isfinite(x).all()
    with pytest.raises(_lib.NcxError, match="overflow"):
        knn(torch.from_numpy(x).cuda(), k=25)
    _check("one_query")                                                 # the next call starts clean


@pytest.mark.parametrize("name", ["signed_normal", "offset50_dv64", "offset50_dv2048"])
def test_sign_and_offset(name):
    _check(name)


@pytest.mark.parametrize("name", ["cluster_1e-2", "cluster_1e-3", "cluster_1e-4"])
def test_near_duplicate_cluster(name):
    _check(name)


@pytest.mark.parametrize("name", ["tie_groups", "zero_table", "near_block"])
def test_exact_ties_lowest_index(name):
    _check(name)


def test_mass_ties_bit_identical_across_calls():
    c = R.case("zero_table")
    first = _knn(c)
    for _ in range(2):
        again = _knn(c)
        assert np.array_equal(first[0], again[0]) and np.array_equal(first[1].view(np.int32), again[1].view(np.int32))


@pytest.mark.parametrize("name", [n for n in R.CASES if n.startswith(("edge_", "dv"))] + ["one_query", "other_queries"])
def test_edges_of_n_k_dv(name):
    _check(name)


@pytest.mark.parametrize("block_rows", [1, 7])
def test_query_blocks_bit_identical(block_rows):
    """norms_ready reuse and the ragged last block: 20 queries in blocks of 1 and 7 equal one unblocked call bit for bit, and
    the exact order (lattice queries: the products are exact)."""
    c = dict(x=R.lattice(9, 300, 64), q=R.lattice(12, 20, 64), k=25)
    whole, parts = _knn(c), _knn(c, block_rows=block_rows)
    assert np.array_equal(whole[0], parts[0]) and np.array_equal(whole[1].view(np.int32), parts[1].view(np.int32))
    R.check_knn(parts[0], parts[1], c["q"], c["x"], 25, True)


@pytest.mark.parametrize("where", ["table", "queries"])
@pytest.mark.parametrize("bad", [np.inf, -np.inf, np.nan])
def test_non_finite_input_raises(where, bad):
    from neuralcx.knn import knn
    x, q = R.lattice(9, 300, 64), R.lattice(11, 37, 64)
    (x if where == "table" else q)[17, 5] = bad
    with pytest.raises(ValueError):
        knn(torch.from_numpy(x).cuda(), k=25, queries=torch.from_numpy(q).cuda())


def test_non_finite_input_raises_in_cli(tmp_path):
    spec = importlib.util.spec_from_file_location("ncx_knn_cli", os.path.join(PKG, "knn.py"))
    cli = importlib.util.module_from_spec(spec); spec.loader.exec_module(cli)
    x = R.lattice(9, 300, 64)
    x[200, 63] = np.inf
    np.save(os.path.join(tmp_path, "trainset.npy"), x)
    with pytest.raises(ValueError):
        cli.main([str(tmp_path), "--hdf5_file", "trainset.hdf5", "--save_dir", str(tmp_path), "-k", "25"])
