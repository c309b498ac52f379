"""The edge shapes and the seeded inputs of the three VQA trainers' GPU tests (tests/test_vqa_train_gpu.py, test_mlb_train_gpu.py,
test_mlb_att_train_gpu.py), in one place so that tools/ab_trainers.py runs the same cases without importing a test module.

The small shapes reach every code path of the trainers' own kernels: one row, odd row counts, widths that are no multiple of a GEMM
tile, more than one workgroup, R = 1 and R = 10, every tile form and the P < 4 kernel of the attention model.  All their widths are
multiples of 4, so the element-wise kernels take their 16-byte lanes; the RAGGED shapes (odd widths) take the one-element forms."""
import numpy as np

import mlb_train_ref
import vqa_train_ref

# (B, dv, dq, dhv, dhq, dz, R, A)
MUTAN_EDGE = [(1, 36, 20, 12, 8, 4, 1, 8), (33, 100, 68, 36, 44, 20, 3, 52), (70, 132, 96, 44, 40, 40, 10, 100), (130, 64, 48, 32, 32, 36, 10, 2000)]
MUTAN_RAGGED = (3, 37, 21, 9, 9, 13, 2, 7)
# (B, dv, dq, dh, A)
MLB_EDGE = [(1, 36, 20, 4, 8), (33, 100, 68, 20, 52), (70, 132, 96, 44, 100), (130, 64, 48, 36, 2000)]
MLB_RAGGED = (3, 37, 21, 13, 7)
# (B, dv, dq, dh_att, G, dh_f, A, W, H)
ATT_EDGE = [(5, 64, 48, 32, 2, 24, 40, 5, 7),           # P = 35, ragged 64-row tile
            (3, 36, 20, 70, 3, 12, 9, 14, 14),          # P = 196: the 208-row tile; two hidden tiles, the second ragged; dv = one whole step + 4
            (4, 33, 12, 65, 8, 5, 7, 5, 13),            # P = 65, two position tiles; G = 8; odd widths
            (2, 8, 8, 4, 1, 4, 4, 1, 2),                # the P < 4 kernel; minimal widths; G = 1
            (2, 8, 8, 8, 2, 4, 4, 1, 1),                # P = 1: ds is exactly zero
            (13, 40, 16, 48, 2, 8, 6, 3, 3)]            # repeated, non-identity img_idx; uneven image groups of the dWv_att split


def _vq_case(params, B, dv, dq, dz, A, seed, n_extra):
    rng = np.random.default_rng(seed + B)
    feats = (np.abs(rng.standard_normal((B + n_extra, dv))) * 0.45).astype(np.float32)
    q = (rng.standard_normal((B, dq)) * 0.3).astype(np.float32)
    idx = np.arange(B, dtype=np.int32)
    target = rng.integers(0, A, size=B).astype(np.int32)
    masks = tuple((rng.random((B, w)) >= 0.5).astype(np.float32) for w in (dv, dq, dz))
    return params, feats, q, idx, target, masks


def mutan_case(shape, seed=0, gain=2.0, n_extra=3):
    """Seeded inputs: a feature table with n_extra spare rows, an identity index, q, targets, p = 0.5 keep masks."""
    B, dv, dq, dhv, dhq, dz, Rk, A = shape
    return _vq_case(vqa_train_ref.init_params(seed + 1, dv, dq, dhv, dhq, dz, Rk, A, gain=gain), B, dv, dq, dz, A, seed, n_extra)


def mlb_case(shape, seed=0, gain=2.0, n_extra=3):
    """Seeded inputs: a feature table with n_extra spare rows, an identity index, q, targets, p = 0.5 keep masks."""
    B, dv, dq, dh, A = shape
    return _vq_case(mlb_train_ref.init_params(seed + 1, dv, dq, dh, A, gain=gain), B, dv, dq, dh, A, seed, n_extra)


def gathered_33(feats, out_of_table):
    """The B = 33 shapes run with a non-identity index: a repeated image and an all-zero feature row (feats is modified); with
    out_of_table also two ids outside the table, which the kernels clamp."""
    feats[35] = 0.0
    idx = np.random.default_rng(5).permutation(33).astype(np.int32)
    idx[3] = idx[7]; idx[11] = 35
    if out_of_table:
        idx[20] = -4; idx[21] = 99
    return idx


# ---- the attention model: state dict -> ops.MlbAttWeights ----
ACT_CODE = {None: 0, "": 0, "tanh": 2}
ACT_FIELD = dict(att_v="act_v_att", att_q="act_q_att", att_mm="act_mm", v="act_v", q="act_q", c="act_c")


def att_weights(state, acts=None, dev="cuda:0"):
    import torch
    from neuralcx import ops
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)
    G = state["conv_att.weight"].shape[0]
    tens = dict(wv_att=t(state["conv_v_att.weight"].reshape(state["conv_v_att.weight"].shape[0], -1)), bv_att=t(state["conv_v_att.bias"]),
                wq_att=t(state["linear_q_att.weight"]), bq_att=t(state["linear_q_att.bias"]),
                wa=t(state["conv_att.weight"].reshape(G, -1)), ba=t(state["conv_att.bias"]),
                wg=t(np.stack([state["list_linear_v_fusion.%d.weight" % g] for g in range(G)])),
                bg=t(np.stack([state["list_linear_v_fusion.%d.bias" % g] for g in range(G)])),
                wqf=t(state["linear_q_fusion.weight"]), bqf=t(state["linear_q_fusion.bias"]),
                wc=t(state["linear_classif.weight"]), bc=t(state["linear_classif.bias"]))
    codes = {ACT_FIELD[k]: ACT_CODE[v] for k, v in (acts or {}).items()}
    return ops.MlbAttWeights.from_tensors(tens, **codes)
