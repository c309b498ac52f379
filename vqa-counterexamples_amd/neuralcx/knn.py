"""k nearest neighbours of image-feature rows on the GPU.

Same result as the reference's knn.py:41-58 -- sklearn `NearestNeighbors(n_neighbors=k).fit(features)` followed by
`kneighbors(features[i:i+b])` over the whole table (brute force, euclidean; each row's first neighbour is itself) --
computed by ncx_knn: one fp32 MFMA GEMM per block of queries + an on-device select / exact re-rank.
"""
import ctypes as C

import torch

from . import _lib
from .ops import _ptr, _stream


def knn(table: torch.Tensor, k: int = 25, queries: torch.Tensor = None, block_rows: int = 4096):
    """table [n, dv] fp32 on the GPU; queries default to the table itself (what knn.py does).
    -> (indices int64 [nq, k], distances fp32 [nq, k]), neighbours in ascending distance (ties by row index).

    Precision contract.  The k + 8 candidates of a query are the largest fp32 products V32(j) ~ q.x_j - |x_j|^2/2, ordered by
    (V32 descending, j ascending); their distances are then recomputed exactly (fp64 sum of (q - x)^2, rounded once to fp32) and
    the first k by (distance, j) are returned.  The returned distance is always that of the returned row.  A returned row r
    that displaced a true neighbour t passed the candidate cut where t did not, V32(r) >= V32(t), so with d2 = |q|^2 - 2 V
        d2(r) - d2(t) = 2 (V(t) - V(r)) <= 4 max_j |V32(j) - V(j)| <= tau,
        tau = 4 (dv + 2) 2^-24 max_j (sum_t |q_t x_jt| + |x_j|^2 / 2)
    (the dot-product rounding bound (dv + 2) u sum|terms|, which holds for any summation order).  Where the exact squared
    distances around the k-th neighbour are further apart than tau, or the rows are exact copies, the result is the exact one,
    lowest index first among equals, and the same bits on every call.  tau grows with the features' common offset: centre
    them if neighbours closer than tau matter.

    Raises ValueError on non-finite input (checked before any launch), NcxError if some query keeps more rows with
    distinct products in one histogram bin than the candidate buffer holds after the last refinement level (nested
    outliers a factor ~1000 apart in squared norm: rescale them) or if the products overflow fp32; no output then."""
    if not table.is_cuda:
        raise _lib.NcxError("knn needs the feature table on the GPU (no CPU fallback)")
    if table.dtype != torch.float32 or table.dim() != 2:
        raise ValueError("table must be a [n, dv] float32 tensor")
    table = table.contiguous()
    q = table if queries is None else queries.to(table.device, torch.float32).contiguous()
    n, dv = table.shape
    if q.dim() != 2 or q.shape[1] != dv:
        raise ValueError("queries must be [nq, %d]" % dv)
    if not 1 <= k <= min(n, 120):
        raise ValueError("k must be in 1..min(n, 120)")
    if not (bool(torch.isfinite(table).all()) and (queries is None or bool(torch.isfinite(q).all()))):
        raise ValueError("knn needs finite features (inf or nan in the table or the queries)")
    nq = q.shape[0]
    block_rows = max(1, min(block_rows, nq))
    L = _lib.lib()
    need = L.ncx_knn_workspace_bytes(n, block_rows) + 256
    ws = torch.empty(need, dtype=torch.uint8, device=table.device)
    base = (ws.data_ptr() + 255) // 256 * 256
    idx = torch.empty(nq, k, dtype=torch.int64, device=table.device)
    dist = torch.empty(nq, k, dtype=torch.float32, device=table.device)
    for i in range(0, nq, block_rows):
        m = min(block_rows, nq - i)
        qb, ib, db = q[i:i + m], idx[i:i + m], dist[i:i + m]
        _lib.check(L.ncx_knn(_ptr(table, torch.float32, "table"), n, C.c_void_p(qb.data_ptr()), m, dv, k, 1 if i else 0,
                             C.c_void_p(base), C.c_size_t(need - 256), C.c_void_p(ib.data_ptr()), C.c_void_p(db.data_ptr()),
                             _stream()), "ncx_knn")
    off = (base - ws.data_ptr()) + L.ncx_knn_status_offset(n)              # two status words, read once per call
    exhausted, nonfinite = ws[off:off + 8].view(torch.int32).tolist()
    if nonfinite:
        raise _lib.NcxError("ncx_knn: the products q.x - |x|^2/2 overflow fp32 (features too large)")
    if exhausted:
        raise _lib.NcxError("ncx_knn: a query keeps more rows with distinct products in one bin than the candidate buffer holds "
                            "after the last refinement level (nested outlier rows); no result")
    return idx, dist
