"""GPU: the Adam epilogue of the answer-embedding gradient's launch with p, m, v loaded ahead (csrc/ncx_main.h, `CFG::ADAM`), bit for bit.

A thread of a 64 x 64 tile owns four 16-byte pieces (tile rows t / 16 + 16 i, one column quad).  It requests the parameter and both moments of
all four before the accumulators are staged through LDS and consumes them in an unrolled loop; under the row map it reads the output row of
each piece from the permutation table itself.  What that can get wrong while tests/test_fused_adam_gpu.py stays green: a wrong row under the
map, a ragged tile reading or using a piece whose address was clamped, the pairing of piece and row after unrolling.  So, with the harness of
that file (flat buffers with sentinels behind each, three consecutive steps from zero moments, the fused call against ncx_backward +
ncx_adam_step on cloned state, torch.equal on the parameters, both moments and every gradient), H = 32 and K = 24 throughout:

* A = 1985, da = 1028 (32 x 17 = 544 tiles): the last row tile has ONE row, the last column tile one quad; B = 3 and B = 33;
* A = 1087, da = 1980 (17 x 31 = 527 tiles): the last row tile has 63 rows, the last column tile 60 columns; B = 33;
* the permuted-row form with a permutation far from the identity: every answer of the batch among the highest ids (they move to the front),
  and all B triplets sharing one answer (a single present row: every row tile but the first stops after the first segment); the same batch
  on the plain form (hook NCX_NO_DE_SKIP, set in-process: it is read at call time);
* grad_scale = 0.5 with training-mode dropout;
* da = 1030: the route admits da % 4 != 0 whenever A * da % 4 == 0 (the flat buffer's tail stays 16-byte aligned), so A = 1986, da = 1030
  (32 x 17 tiles) runs the scalar right-edge path (the last quad of a row has two columns) beside prefetched pieces on rows that are only
  8-byte aligned.

The fused route needs ceil(A / 64) * ceil(da / 64) >= 512 on the MI355X; a case that does not take it FAILS (nothing here skips).
No comparison carries a tolerance.
"""
import numpy as np
import pytest
import torch

from helpers import dev, random_case_f32
from oracle import ncx_oracle as orc
from test_fused_adam_gpu import _assert_same, _route, _train

pytestmark = pytest.mark.gpu

# id: (B, A, da, L, answers, training, grad_scale, NCX_NO_DE_SKIP)
#   answers: "random" = `distinct` ids drawn from all A; "top" = the B highest ids, in descending order; "one" = one id for the whole batch
CASES = {
    "A1985-da1028-B3": (3, 1985, 1028, 1, "random", False, 1.0, False),
    "A1985-da1028-B33": (33, 1985, 1028, 1, "random", False, 1.0, False),
    "A1087-da1980-B33": (33, 1087, 1980, 1, "random", False, 1.0, False),
    "A1985-da1028-B33-highest-ids": (33, 1985, 1028, 1, "top", False, 1.0, False),
    "A1087-da1980-B33-one-answer": (33, 1087, 1980, 1, "one", False, 1.0, False),
    "A1985-da1028-B33-highest-ids-plain-rows": (33, 1985, 1028, 1, "top", False, 1.0, True),
    "A1087-da1980-B33-dropout-gscale": (33, 1087, 1980, 2, "random", True, 0.5, False),
    "A1986-da1030-B33-scalar-right-edge": (33, 1986, 1030, 1, "random", False, 1.0, False),
    "A1986-da1030-B3-scalar-right-edge-plain-rows": (3, 1986, 1030, 1, "top", False, 1.0, True),
}
_INPUTS = {}


def _inputs(name):
    if name not in _INPUTS:
        B, A, da, L, answers = CASES[name][:5]
        d = orc.Dims(K=24, dv=16, dq=8, dz=8, da=da, A=A, H=32, L=L)
        params = orc.init_params(d, seed=35, gain=3.0)
        batch = random_case_f32(700 + B + A, B, d)
        rng = np.random.default_rng(A + B)
        if answers == "top":
            ids = np.arange(A - 1, A - 1 - B, -1)
        elif answers == "one":
            ids = np.full(B, A - 2)
        else:
            distinct = max(2, (2 * B) // 3)
            first = rng.permutation(A)[:distinct]
            ids = np.concatenate([first, rng.choice(first, size=B - distinct)])
        batch["answer_aids"] = torch.from_numpy(ids.astype(np.int64))
        _INPUTS[name] = (d, params, batch)
    return _INPUTS[name]


@pytest.mark.parametrize("name", list(CASES))
def test_prefetched_epilogue_equals_backward_then_adam(name, monkeypatch):
    training, gscale, no_skip = CASES[name][5:]
    d, params, batch = _inputs(name)
    A, da = CASES[name][1:3]
    assert ((A + 63) // 64) * ((da + 63) // 64) >= 512
    if no_skip:
        monkeypatch.setenv("NCX_EXPERIMENT", "1")
        monkeypatch.setenv("NCX_NO_DE_SKIP", "1")
    assert _route(d, batch)["fused"], "%s does not take the fused route" % name
    from neuralcx import ops
    dims, sep = _train(d, params, batch, False, training=training, gscale=gscale)
    assert (ops.ws_de_perm_view(dims, ops.alloc_workspace(dims, dev())).numel() == 0) == no_skip      # which form of the product ran
    _, fus = _train(d, params, batch, True, training=training, gscale=gscale)
    _assert_same(sep, fus)
    # the embedding gradient is not trivially zero where the batch has answers, and the rows without one still moved through dGt
    g = fus[-1]["grad"][: A * da].view(A, da)
    assert int((g != 0).any(dim=1).sum()) > A // 2
