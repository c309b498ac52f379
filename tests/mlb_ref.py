"""fp64 restatement of CXModelBase.vqa_forward below the question encoder for the MLB no-attention model (reference
vqa/models/cx.py:64-104, fusion.py:31-50, noatt.py:24-29; eval mode, every dropout the identity).  numpy only."""
import numpy as np

_ACT = {None: lambda x: x, "": lambda x: x, "tanh": np.tanh}


def mlb_vqa_forward(state, feats, img_idx, q_emb, act_v="tanh", act_q="tanh", act_c=None):
    """state: the model's state_dict as arrays (fusion.linear_v.*, fusion.linear_q.*, linear_classif.*); feats [n_img, dv];
    img_idx [B, K + 1]; q_emb [B, dq]  ->  (a_orig [B, A], z_orig [B, dh], a_knns [B, K, A], z_knns [B, K, dh]) in fp64."""
    f64 = lambda k: np.asarray(state[k], np.float64)
    x_q = _ACT[act_q](np.asarray(q_emb, np.float64) @ f64("fusion.linear_q.weight").T + f64("fusion.linear_q.bias"))       # [B, dh]
    v = np.asarray(feats, np.float64)[np.asarray(img_idx, np.int64)]                                                         # [B, K + 1, dv]
    x_v = _ACT[act_v](v @ f64("fusion.linear_v.weight").T + f64("fusion.linear_v.bias"))
    z = x_q[:, None, :] * x_v
    a = _ACT[act_c](z) @ f64("linear_classif.weight").T + f64("linear_classif.bias")
    return a[:, 0], z[:, 0], a[:, 1:], z[:, 1:]
