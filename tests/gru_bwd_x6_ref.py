"""CPU emulation of the bf16 x 6 (NCX_F_X6) form of the GRU encoder's backward through time (csrc/ncx_gru_train_x6.hip), in torch fp32.

The forward runs in fp64 (the recurrence of tests/gru_train_ref.py) and leaves the stash the device keeps -- x_t, h_{t-1}, r, z, n, hn per
step, rounded to fp32 once.  The backward is then restated in fp32 with its four matrix products behind one function each:

    sweep   dGh_t . W_hh            bit 0 of ncx_gru_bwd_form
    dX      dGx_t . W_ih            bit 1
    dW_hh   dGh_t^T h_{t-1}         bit 2
    dW_ih   dGx_t^T x_t             bit 3

A product whose bit is in `mask` runs over truncated bf16 planes with fp32 accumulation, as the kernels do: a = a1 + a2 + a3 exactly
(a1 = a & 0xFFFF0000, a2 = (a - a1) & 0xFFFF0000, a3 = a - a1 - a2), and `nprod` of the nine plane products, largest first:
    3   a1 b1 + a1 b2 + a2 b1
    5   ... + a2 b2 + a1 b3                     (one of the three 2^-16 terms is missing)
    6   ... + a3 b1                             (the forward step kernels' form)
    8   ... + a2 b3 + a3 b2                     (the backward kernels' form; a1 b1 on one accumulator, the small seven on a second)
The other products are plain fp32 matmuls; mask = 0 is the fp32 backward's restatement (`err_fp32` of the bound)."""
import numpy as np
import torch

from gru_ref import lengths
from x6_ref import cut

SWEEP, DX, DWHH, DWIH = 1, 2, 4, 8
SHIPPED_MASK = SWEEP | DX | DWHH | DWIH    # what ncx_gru_bwd_form reports under NCX_F_X6
SHIPPED_NPROD = 8
ORDER = ((0, 0), (0, 1), (1, 0), (1, 1), (0, 2), (2, 0), (1, 2), (2, 1))
GRADS = ("E", "w_ih", "w_hh", "b_ih", "b_hh")


def plane_matmul(a, b, nprod):
    """a @ b over the planes: the leading product on one fp32 accumulator, the small ones (smallest first) on a second."""
    pa, pb = cut(a), cut(b)
    small = None
    for i, j in reversed(ORDER[1:nprod]):
        term = pa[i] @ pb[j]
        small = term if small is None else small + term
    return pa[0] @ pb[0] + small


def forward_stash(wids, E, w_ih, w_hh, b_ih, b_hh):
    """The fp64 forward of gru_train_ref.gru_train; -> (lens, [(act, x, h_prev, r, z, n, hn) per step]) rounded to fp32 torch tensors."""
    wids = np.asarray(wids)
    E, w_ih, w_hh, b_ih, b_hh = (np.asarray(a, np.float64) for a in (E, w_ih, w_hh, b_ih, b_hh))
    B, T = wids.shape
    dq = w_hh.shape[1]
    sig = lambda a: 1.0 / (1.0 + np.exp(-a))
    lens = lengths(wids)
    h = np.zeros((B, dq))
    stash = []
    f32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    for t in range(T):
        act = lens > t
        x = E[wids[act, t]]
        gx = x @ w_ih.T + b_ih
        gh = h[act] @ w_hh.T + b_hh
        r = sig(gx[:, :dq] + gh[:, :dq])
        z = sig(gx[:, dq:2 * dq] + gh[:, dq:2 * dq])
        hn = gh[:, 2 * dq:]
        n = np.tanh(gx[:, 2 * dq:] + r * hn)
        stash.append((act, f32(x), f32(h[act]), f32(r), f32(z), f32(n), f32(hn)))
        h[act] = (1.0 - z) * n + z * h[act]
    return lens, stash


def backward(wids, E, w_ih, w_hh, dq_out, lens, stash, mask=0, nprod=SHIPPED_NPROD):
    """-> {"E", "w_ih", "w_hh", "b_ih", "b_hh"} as float32 numpy arrays: the backward in fp32, the products of `mask` over `nprod` planes."""
    wids = np.asarray(wids)
    t32 = lambda a: torch.from_numpy(np.ascontiguousarray(a, np.float32))
    w_ih, w_hh, dq_out = t32(w_ih), t32(w_hh), t32(dq_out)
    B, T = wids.shape
    dq = w_hh.shape[1]
    mm = lambda bit, a, b: plane_matmul(a, b, nprod) if mask & bit else a @ b
    g = {"E": torch.zeros(E.shape, dtype=torch.float32), "w_ih": torch.zeros_like(w_ih), "w_hh": torch.zeros_like(w_hh),
         "b_ih": torch.zeros(3 * dq), "b_hh": torch.zeros(3 * dq)}
    dh = torch.zeros(B, dq)
    for t in range(T - 1, -1, -1):
        act, x, hp, r, z, n, hn = stash[t]
        act_t, last = torch.from_numpy(act), torch.from_numpy(lens - 1 == t)
        dh[last] += dq_out[last]
        d = dh[act_t]
        dn, dz = d * (1.0 - z), d * (hp - n)
        da_n, da_z = dn * (1.0 - n * n), dz * z * (1.0 - z)
        da_r, da_hn = da_n * hn * r * (1.0 - r), da_n * r
        dgx, dgh = torch.cat([da_r, da_z, da_n], 1), torch.cat([da_r, da_z, da_hn], 1)
        g["w_ih"] += mm(DWIH, dgx.t(), x)
        g["b_ih"] += dgx.sum(0)
        g["b_hh"] += dgh.sum(0)
        if t >= 1:
            g["w_hh"] += mm(DWHH, dgh.t(), hp)
        g["E"].index_add_(0, torch.from_numpy(wids[act, t]), mm(DX, dgx, w_ih))
        dh[act_t] = d * z + mm(SWEEP, dgh, w_hh)
    g["E"][0] = 0.0
    return {k: v.numpy() for k, v in g.items()}


def errors(got, ref):
    """-> {tensor: max|got - fp64|}"""
    return {k: float(np.abs(got[k].astype(np.float64) - ref[k]).max()) for k in GRADS}


def bound(err_fp32, ref, c):
    """The fp32-grade bound per gradient tensor: 1.5 err_fp32 + c max|ref|."""
    return {k: 1.5 * err_fp32[k] + c * float(np.abs(ref[k]).max()) for k in GRADS}
