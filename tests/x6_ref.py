"""The cut of the bf16 x 6 (NCX_F_X6) kernels (csrc/ncx_x6.h), restated in torch for the CPU emulations of those kernels."""
import torch


def cut(x):
    """fp32 tensor -> its three truncated bf16 planes (as fp32 tensors), x1 + x2 + x3 == x exactly: x1 = x & 0xFFFF0000,
    x2 = (x - x1) & 0xFFFF0000, x3 = the high half of x - x1 - x2 (which holds every bit that is left)."""
    hi = lambda v: (v.contiguous().view(torch.int32) & -65536).view(torch.float32)
    x1 = hi(x)
    r1 = x - x1
    x2 = hi(r1)
    return x1, x2, hi(r1 - x2)
