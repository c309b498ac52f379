"""GPU: Adam applied by the launch of the answer-embedding gradient (ncx_backward_adam) against ncx_backward + ncx_adam_step, bit for bit.

1. k_adam, rebuilt on the shared device function adam_update (csrc/ncx_adam.h), returns the bits it returned before: a golden file of the
   earlier library's outputs (tests/golden/adam_bits.npz, written once by tools/make_adam_golden.py; n = 4099: 1024 quads + a ragged tail).
2. The fused call equals the two separate calls on cloned state -- parameters, both moments and every gradient, three consecutive steps
   (bias correction, non-zero moments).  The fused route needs the 64 x 64 form of the product, i.e. at least two tiles per workgroup slot
   (ceil(A / 64) * ceil(da / 64) >= 512 on the MI355X): the fused cases are the smallest such shapes with A and da off the tile (2000 x 1028,
   1028 x 2020, 4100 x 516), H = 32 and 256, B = 3 and 33, L = 1 and 2, K = 24; the shapes below that size (A = 68 / 132, da = 36 / 100)
   do not take the route and are skipped loudly.  The permuted-row form (de_skip) and, under the hook NCX_NO_DE_SKIP, the plain form; a
   grad_scale != 1; training mode with dropout.  (The hooks are read at call time, so they are set in-process like the de_skip tests do.)
3. Passenger slicing: a flat buffer without padding between tensors (tail length % 4 == 1), passenger counts that do not divide the tail
   (5, the default) and more passengers than the tail has quads (a tail shorter than one slice each); sentinels behind every buffer.
4. Fallbacks of the same call: the hook NCX_NO_FUSED_ADAM, the a_emb lesion, the bf16 variant.
Nothing here carries a tolerance: every comparison is torch.equal / array_equal.
"""
import math
import os

import numpy as np
import pytest
import torch

from conftest import GOLDEN
from helpers import dev, random_case_f32, to_dev_batch
from oracle import ncx_oracle as orc

pytestmark = pytest.mark.gpu

NAMES = ("answer_embedding.weight", "linear_1.weight", "linear_1.bias", "linear_2.weight", "linear_2.bias", "out.weight", "out.bias")
SENTINEL = 7.0


# ---- 1. k_adam kept its bits ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("step,gscale", [(1, 1.0), (7, 0.5)])
def test_k_adam_returns_the_bits_of_the_golden(step, gscale):
    from neuralcx import ops
    g = np.load(os.path.join(GOLDEN, "adam_bits.npz"))
    p, gr, m, v = (torch.from_numpy(g[k + "0"]).to(dev()) for k in "pgmv")
    assert p.numel() == 4099
    ops.adam_step(p, gr, m, v, step, lr=1e-3, grad_scale=gscale)
    torch.cuda.synchronize()
    for k, t in (("p", p), ("m", m), ("v", v)):
        ref = g["%s_step%d" % (k, step)]
        got = t.cpu().numpy()
        assert np.array_equal(got.view(np.uint32), ref.view(np.uint32)), (k, int((got.view(np.uint32) != ref.view(np.uint32)).sum()))


# ---- state: flat buffers the way the engine lays them out (pad = True) or without padding between tensors -----------------------------
class _State:
    def __init__(self, d, params, pad=True):
        self.offsets, off = {}, 0
        for n in NAMES:
            if n in params:
                self.offsets[n] = off
                k = params[n].numel()
                off += (k + 3) // 4 * 4 if pad else k
        self.n, self.shapes = off, {n: tuple(params[n].shape) for n in self.offsets}
        mk = lambda fill: torch.cat([torch.full((off,), fill, device=dev()), torch.full((16,), SENTINEL, device=dev())])
        self.bufs = {k: mk(0.0) for k in ("param", "grad", "exp_avg", "exp_avg_sq")}
        for n, o in self.offsets.items():
            self.bufs["param"][o:o + params[n].numel()] = params[n].reshape(-1).to(dev())
        self.n_emb = self.offsets["linear_1.weight"]

    def flat(self, k):
        return self.bufs[k][: self.n]

    def fields(self, k):
        from helpers import FIELD
        return {FIELD[n]: self.bufs[k][o:o + math.prod(self.shapes[n])].view(self.shapes[n]) for n, o in self.offsets.items()}

    def snapshot(self):
        return {k: v.clone() for k, v in self.bufs.items()}


def _dims(d, b, flags=None, training=False, gb=None):
    from neuralcx import ops, _lib
    return ops.make_dims(b, H=d.H, L=d.L, da=d.da, A=d.A, flags=_lib.NCX_F_ALL if flags is None else flags, training=training,
                         drop_p=0.25 if training else 0.0, seed=11, loss_scale=0.0 if gb is None else 1.0 / gb)


def _train(d, params, batch, fused, steps=3, pad=True, flags=None, training=False, gscale=1.0, extra=None):
    """`steps` training steps from zero moments on fresh buffers; -> (dims, the buffers after every step)."""
    from neuralcx import ops
    st = _State(d, params, pad)
    b = to_dev_batch(batch, extra=extra)
    dims = _dims(d, b, flags, training)
    ws = ops.alloc_workspace(dims, dev())
    gt = batch["gt"].to(dev()).to(torch.int32)
    out = []
    for step in range(1, steps + 1):
        dims.seed = 11 + step
        for v in st.fields("grad").values():
            v.fill_(float("nan"))                                     # (the padding between tensors stays 0: Adam runs over it too)
        scores = ops.forward(dims, b, st.fields("param"), ws)
        lr = ops.ranking_loss(scores, gt)
        kw = dict(lr=1e-3, grad_scale=gscale)
        if fused:
            ops.backward_adam(dims, b, st.fields("param"), ws, lr["dscores"], st.fields("grad"), st.flat("param"), st.flat("grad"),
                              st.flat("exp_avg"), st.flat("exp_avg_sq"), st.n_emb, step, **kw)
        else:
            ops.backward(dims, b, st.fields("param"), ws, lr["dscores"], st.fields("grad"))
            ops.adam_step(st.flat("param"), st.flat("grad"), st.flat("exp_avg"), st.flat("exp_avg_sq"), step, **kw)
        torch.cuda.synchronize()
        out.append(st.snapshot())
    return dims, out


def _assert_same(a, b):
    for s, (x, y) in enumerate(zip(a, b)):
        for k in x:
            assert torch.isfinite(y[k]).all(), (s, k)
            assert torch.equal(x[k], y[k]), (s + 1, k, int((x[k] != y[k]).sum()))
            assert (y[k][-16:] == SENTINEL).all(), (s, k)
    assert not torch.equal(a[0]["param"], a[-1]["param"])               # the steps moved the parameters


# id: (B, A, H, da, L, distinct answers in the batch, training, grad_scale, NCX_NO_DE_SKIP)
CASES = {
    "A2000-da1028-H32-B3-L1": (3, 2000, 32, 1028, 1, 2, False, 1.0, False),
    "A1028-da2020-H256-B33-L2-dropout-gscale": (33, 1028, 256, 2020, 2, 20, True, 0.5, False),
    "A4100-da516-H32-B33-L2": (33, 4100, 32, 516, 2, 33, False, 1.0, False),
    "A2000-da1028-H256-B33-L1-plain-rows": (33, 2000, 256, 1028, 1, 5, False, 0.25, True),
    "A2000-da1028-H32-B3-L2-plain-rows-dropout": (3, 2000, 32, 1028, 2, 3, True, 1.0, True),
    "A68-da36-H32-B3-L1": (3, 68, 32, 36, 1, 2, False, 1.0, False),
    "A132-da100-H256-B33-L2": (33, 132, 256, 100, 2, 20, False, 1.0, False),
}
_INPUTS = {}


def _inputs(name):
    if name not in _INPUTS:
        B, A, H, da, L, distinct = CASES[name][:6]
        d = orc.Dims(K=24, dv=16, dq=8, dz=8, da=da, A=A, H=H, L=L)
        params = orc.init_params(d, seed=33, gain=3.0)
        batch = random_case_f32(500 + B + A, B, d)
        rng = np.random.default_rng(A + B)
        ids = rng.permutation(A)[:distinct]
        batch["answer_aids"] = torch.from_numpy(np.concatenate([ids, rng.choice(ids, size=B - distinct)]).astype(np.int64))
        _INPUTS[name] = (d, params, batch)
    return _INPUTS[name]


def _route(d, batch, flags=None, extra=None):
    from neuralcx import _lib
    return _lib.plan_query(_dims(d, to_dev_batch(batch, extra=extra), flags), "FUSED_ADAM")


@pytest.mark.parametrize("name", list(CASES))
def test_fused_equals_backward_then_adam(name, monkeypatch):
    training, gscale, no_skip = CASES[name][6:]
    d, params, batch = _inputs(name)
    if no_skip:
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        monkeypatch.setenv("NCX_NO_DE_SKIP", "1")
    if not _route(d, batch)["fused"]:
        pytest.skip("%s: the answer-embedding gradient does not take the 64 x 64 form here, no fused route" % name)
    from neuralcx import ops
    dims, sep = _train(d, params, batch, False, training=training, gscale=gscale)
    assert (ops.ws_de_perm_view(dims, ops.alloc_workspace(dims, dev())).numel() == 0) == no_skip
    _, fus = _train(d, params, batch, True, training=training, gscale=gscale)
    _assert_same(sep, fus)


def test_at_least_four_cases_take_the_fused_route():
    taken = [name for name in CASES if _route(_inputs(name)[0], _inputs(name)[2])["fused"]]
    assert len(taken) >= 4, taken


# ---- 3. passenger slicing ---------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("passengers", [None, 5, 70000])
def test_passenger_slices_cover_a_ragged_tail_once(passengers, monkeypatch):
    """No padding between tensors: the tail is H * din + 2 H + 1 elements, % 4 == 1.  5 and the default count do not divide its quads; with
    70 000 passengers most have nothing and the rest one quad.  An element updated twice or not at all differs from ncx_adam_step's."""
    d, params, batch = _inputs("A2000-da1028-H32-B3-L1")
    assert _route(d, batch)["fused"]
    _, sep = _train(d, params, batch, False, steps=2, pad=False)
    if passengers is not None:
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        monkeypatch.setenv("NCX_ADAM_PASS", str(passengers))
    if passengers == 5:      # ... and placed inside the grid (the default at the flagship size: behind the first round of tiles), tiles on both sides
        monkeypatch.setenv("NCX_ADAM_PASS_AT", "101")
    n_pass = _route(d, batch)["passengers"]
    st = _State(d, params, pad=False)
    tail = st.n - st.n_emb
    assert tail % 4 == 1 and ((tail + 3) // 4) % n_pass != 0 and (passengers != 70000 or (tail + 3) // 4 < n_pass)
    _, fus = _train(d, params, batch, True, steps=2, pad=False)
    _assert_same(sep, fus)


# ---- 4. fallbacks: the same call, the two-step result -----------------------------------------------------------------------------------
@pytest.mark.parametrize("how", ["hook", "a_emb-lesion", "bf16"])
def test_fallbacks_return_the_unfused_result(how, monkeypatch):
    from neuralcx import _lib, ops
    d, params, batch = _inputs("A2000-da1028-H32-B3-L1")
    flags, extra = None, None
    if how == "hook":
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        monkeypatch.setenv("NCX_NO_FUSED_ADAM", "1")
    elif how == "bf16":
        flags = _lib.NCX_F_ALL | _lib.NCX_F_BF16
    else:
        batch = dict(batch)
        rng = np.random.default_rng(9)
        batch["a_knns"] = torch.from_numpy(rng.random((3, d.K, d.da), dtype=np.float32))
        extra = dict(a_emb_gt=torch.from_numpy(rng.random((3, d.da), dtype=np.float32)))
        flags = ops.flags_from_spec(dict(orc.DEFAULT_SPEC, a_emb=False))
    assert not _route(d, batch, flags, extra)["fused"]
    _, sep = _train(d, params, batch, False, steps=2, flags=flags, extra=extra)
    _, fus = _train(d, params, batch, True, steps=2, flags=flags, extra=extra)
    _assert_same(sep, fus)
