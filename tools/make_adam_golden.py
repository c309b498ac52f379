"""Writes tests/golden/adam_bits.npz: what ncx_adam_step returns, bit for bit, on seeded random buffers with a ragged tail.

Run ONCE, on the GPU, with the library of the commit BEFORE the Adam update moved into the shared device function of csrc/ncx_adam.h
(NCX_LIB=<that build's libneuralcx_hip.so>): tests/test_fused_adam_gpu.py then holds every later k_adam to those bits.  The file holds
this project's own inputs and outputs.

    NCX_LIB=/path/to/parent/libneuralcx_hip.so python tools/make_adam_golden.py [out.npz]
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "vqa-counterexamples_amd"))

N = 4099                                   # 1024 full quads + a 3-element tail (a pair and an odd last element)
CASES = ((1, 1.0), (7, 0.5))               # (step, grad_scale)


def inputs():
    rng = np.random.default_rng(20261020)
    f = lambda a: np.ascontiguousarray(a, np.float32)
    return dict(p=f(rng.standard_normal(N)), g=f(rng.standard_normal(N) * 0.1), m=f(rng.standard_normal(N) * 0.05),
                v=f(rng.random(N) * 1e-2))


def main():
    import ctypes as C
    import torch                            # first: the library shares torch's HIP runtime (neuralcx/_lib.py)
    # the raw export, not neuralcx._lib: an older library lacks symbols the current binding asks for
    L = C.CDLL(os.environ.get("NCX_LIB") or os.path.join(ROOT, "vqa-counterexamples_amd", "lib", "libneuralcx_hip.so"))
    L.ncx_version.restype = C.c_char_p
    L.ncx_adam_step.restype = C.c_int
    L.ncx_adam_step.argtypes = [C.c_void_p] * 4 + [C.c_size_t] + [C.c_float] * 4 + [C.c_int32, C.c_float, C.c_void_p]
    out = sys.argv[1] if len(sys.argv) > 1 else os.path.join(ROOT, "tests", "golden", "adam_bits.npz")
    dev = torch.device("cuda:0")
    x = inputs()
    rec = {k + "0": v for k, v in x.items()}
    for step, gs in CASES:
        p, g, m, v = (torch.from_numpy(x[k]).to(dev) for k in "pgmv")
        rc = L.ncx_adam_step(p.data_ptr(), g.data_ptr(), m.data_ptr(), v.data_ptr(), N, 1e-3, 0.9, 0.999, 1e-8, step, gs,
                             C.c_void_p(torch.cuda.current_stream().cuda_stream))
        assert rc == 0, rc
        torch.cuda.synchronize()
        for k, t in (("p", p), ("m", m), ("v", v)):
            rec["%s_step%d" % (k, step)] = t.cpu().numpy()
    version = L.ncx_version().decode()
    rec["lib"] = np.frombuffer(version.encode(), np.uint8)
    np.savez_compressed(out, **rec)
    print("wrote", out, "from", version)


if __name__ == "__main__":
    main()
