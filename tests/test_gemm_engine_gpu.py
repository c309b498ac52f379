"""GPU: the generic GEMM engine (csrc/ncx_gemm.h) called directly through ncx_diag_gemm on the cases of tests/gemm_ref.py: every
instantiation at its tile edges, the operand kinds, chains, groups, split-K with its fix-up, the epilogue, the FOLD recurrence and the
persistent loop.  Every launch reads operands that sit between NaN margins with NaN in the gap ld - cols, writes into outputs filled with
one NaN pattern and, when split, into a slab filled with 0xFF.  Per case: every element within c 2^-24 S of the fp64 restatement, margins
and the columns beyond N bit-unchanged, a second run bit-identical, and the generic k-loop (no_fast) within the same bound and
bit-identical to the fast one (gemm_ref.same_k_order says why), and the grid the launch was given: one workgroup per work item, or --
the persistent case -- fewer than half as many.  The worst ratio per (group, instance) is printed and must be the one that
profiles/gemm_engine_edges.json records for it ("gpu_instances": the kernels are deterministic); with NCX_GEMM_EDGES_RECORD=<file> the
test appends what it measured to that file as JSON lines, which is how the profile's entries are written."""
import json
import os

import numpy as np
import pytest
import torch

import gemm_ref as G

from conftest import ROOT

pytestmark = pytest.mark.gpu
PROFILE = os.path.join(ROOT, "profiles", "gemm_engine_edges.json")
PARAMS = sorted({(c["group"], G.instance_of(c)) for c in G.CASES})


class Launch:
    """The device buffers of one case; run() -> the raw bits of every output buffer."""

    def __init__(self, c, X):
        from neuralcx import ops
        self.c, self.X, self.ops = c, X, ops
        self.dev = {name: torch.from_numpy(buf).cuda() for name, (buf, _) in X.bufs.items()}
        self.sizes = {}
        for p, o in enumerate(X.out):
            self.sizes["out%d" % p] = 2 * G.MARGIN + o["rows"] * o["ldo"]
            if o["rows0"]:
                self.sizes["outz%d" % p] = 2 * G.MARGIN + o["rows0"] * o["ldo0"]
        need = ops.diag_gemm_slab_bytes(G.fill_args(c, X, self._addr_inputs_only))
        assert need == 4 * G.slab_floats(c), (c["id"], need)
        self.slab_bytes = need

    def _addr_inputs_only(self, name):
        return self.dev[name].data_ptr() if name in self.dev else 1 << 20

    def run(self, no_fast):
        outs = {name: torch.full((n,), G.OUT_FILL, dtype=torch.int32, device="cuda") for name, n in self.sizes.items()}
        slab = torch.full((max(self.slab_bytes, 16),), 0xFF, dtype=torch.uint8, device="cuda")
        addr = lambda name: (outs[name] if name in outs else self.dev[name]).data_ptr()
        a = G.fill_args(self.c, self.X, addr, no_fast=no_fast, slab=slab.data_ptr() if self.slab_bytes else 0, slab_bytes=self.slab_bytes)
        old = {k: os.environ.get(k) for k in self.c["env"]}
        os.environ.update(self.c["env"])
        try:
            self.ops.diag_gemm(a)
            torch.cuda.synchronize()
            self.grid = int(a.grid)
        finally:
            for k, v in old.items():
                if v is None:
                    del os.environ[k]
                else:
                    os.environ[k] = v
        return {name: t.cpu().numpy().view(np.uint32) for name, t in outs.items()}


def logical(c, X, bits):
    """The raw output buffers -> per problem the [M, N] values, after checking that nothing else was written."""
    res = []
    fill = np.uint32(G.OUT_FILL)
    for p, o in enumerate(X.out):
        M, N = c["M"], o["N"]
        in0, row = G.out_rows_map(c, p, X)
        val = np.empty((M, N), np.float32)
        for name, rows, ld, sel in (("out%d" % p, o["rows"], o["ldo"], ~in0), ("outz%d" % p, o["rows0"], o["ldo0"], in0)):
            if not rows:
                continue
            buf = bits[name]
            assert (buf[:G.MARGIN] == fill).all() and (buf[-G.MARGIN:] == fill).all(), (c["id"], name, "margin written")
            body = buf[G.MARGIN:-G.MARGIN].reshape(rows, ld)
            assert (body[:, N:] == fill).all(), (c["id"], name, "columns beyond N written")
            assert sorted(row[sel].tolist()) == list(range(rows))
            val[sel] = body[row[sel], :N].view(np.float32)
        res.append(val)
    return res


@pytest.mark.parametrize("group,instance", PARAMS, ids=["%s-%s" % p for p in PARAMS])
def test_engine_case_group(group, instance):
    from neuralcx import ops
    cases = [c for c in G.CASES if c["group"] == group and G.instance_of(c) == instance]
    cbound = G.bound_c(group)
    worst, worst_id, worst_eq32, ran = 0.0, None, None, 0
    for c in cases:
        X = G.build(c)
        if G.expected_rc(c) == G.E_DIMS:              # an operand narrower than a 16-byte window: refused before any launch
            a = G.fill_args(c, X, G.fake_addr)
            assert ops.diag_gemm_rc(a) == G.E_DIMS, c["id"]
            continue
        ref = G.restate(c, X)
        L = Launch(c, X)
        fast = L.run(no_fast=False)
        again = L.run(no_fast=False)
        slow = L.run(no_fast=True)
        for name in fast:
            assert (fast[name] == again[name]).all(), (c["id"], name, "a second run differs")
        items = G.work_items(c)
        if c["group"] == "persistent":                # the grid is one workgroup per resident slot: a multiple of 8, less than half the items
            assert L.grid % 8 == 0 and 0 < 2 * L.grid < items, (c["id"], L.grid, items, "the persistent loop was not taken")
        else:
            assert L.grid == items, (c["id"], L.grid, items)
        x32 = G.restate(c, X, np.float32)
        for tag, bits in (("fast", fast), ("no_fast", slow)):
            for p, (got, (r, S)) in enumerate(zip(logical(c, X, bits), ref)):
                ratio = G.ratio(got, r, S)
                if ratio > worst:
                    err = np.where(S > 0, np.abs(got.astype(np.float64) - r) / (G.U24 * np.where(S > 0, S, 1)), 0)
                    at = np.unravel_index(err.argmax(), err.shape)
                    worst, worst_id = ratio, "%s[%d] %s at %s" % (c["id"], p, tag, tuple(int(i) for i in at))
                    # whether the float32 restatement has the same float at that element, and in how many elements overall
                    worst_eq32 = (bool(got[at] == x32[p][0][at]), int((got == x32[p][0]).sum()), int(got.size))
                assert ratio <= cbound, (c["id"], p, tag, ratio, cbound)
        if G.same_k_order(c):
            for name in fast:
                assert (fast[name] == slow[name]).all(), (c["id"], name, "the generic k-loop differs from the fast one")
        ran += 1
    print("gemm engine ratio group %s instance %s: max %.3f of c = %.1f over %d cases (%s; the float32 restatement has %s there, and the "
          "same float in %d of that output's %d elements)" % ((group, instance, worst, cbound, ran, worst_id, "the same float" if worst_eq32[0] else "another float") + worst_eq32[1:]))
    rec = dict(group=group, instance=instance, gpu_max_ratio=round(worst, 3), at=worst_id, float32_same_float_there=worst_eq32[0],
               float32_same_float_elements=list(worst_eq32[1:]))
    if os.environ.get("NCX_GEMM_EDGES_RECORD"):
        with open(os.environ["NCX_GEMM_EDGES_RECORD"], "a") as f:
            f.write(json.dumps(rec) + "\n")
    recorded = json.load(open(PROFILE))["gpu_instances"]["%s/%s" % (group, instance)]
    assert abs(recorded["gpu_max_ratio"] - worst) <= 0.0015 and recorded["gpu_max_ratio"] <= cbound, (recorded, worst)
