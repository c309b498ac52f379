"""Writes tests/golden/g19_lstm.npz.  Data only: names, shapes, inputs and recorded outputs.

From the REFERENCE's TwoLSTM (vqa/models/seq2vec.py:11-25, 48-76, loaded from the reference checkout $NCX_REFERENCE with `skipthoughts` stubbed by an empty
module; this script fails hard without the checkout), at V 30, emb 22, H 50:
  ref/sd_names, ref/sd_shapes     its state_dict
  ref/wids, ref/lengths           process_lengths on planted rows: all padding, a zero inside a question, a full row, a length-1 row
  ref/sel_x, ref/sel_out          select_last on a seeded x with those lengths
  ref/fwd, ref/fwd_swapped        its forward AS WRITTEN (recurrence over the batch axis) of one batch and of the same batch with rows
                                  1 and 2 swapped (ref/swap)
From the project's TwoLSTM on the CPU in eval mode (torch's nn.LSTM with batch_first, which is what pins the arithmetic), emb 22, H 50,
B 9, T 7, E[0] nonzero; c0 default init, c1 the LSTM weights x 3 so that gates leave the linear range:
  c*/wids, c*/E, c*/rnn_{0,1}.{weight,bias}_{ih,hh}_l0, c*/x0, c*/x1 (both layers at the selected step), c*/q"""
import importlib.util
import os
import sys
import types

import numpy as np
import torch

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd")]
REF = os.environ.get("NCX_REFERENCE", "")               # the reference checkout (the directory that holds vqa/models/seq2vec.py)
V, EMB, H, B, T = 30, 22, 50, 9, 7
KEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")


def reference_module():
    path = os.path.join(REF, "vqa", "models", "seq2vec.py")
    if not REF or not os.path.isfile(path):
        raise SystemExit("make_golden_lstm.py: set NCX_REFERENCE to the reference checkout (got %r)" % REF)
    sys.modules.setdefault("skipthoughts", types.ModuleType("skipthoughts"))
    spec = importlib.util.spec_from_file_location("ref_seq2vec", path)
    m = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(m)
    return m


def planted_wids(rng, lens):
    wids = np.zeros((len(lens), T), np.int64)
    for b, n in enumerate(lens):
        wids[b, :n] = rng.integers(1, V + 1, size=n)
    return wids


def from_reference(out):
    ref = reference_module()
    torch.manual_seed(0)
    rng = np.random.default_rng(0)
    m = ref.TwoLSTM(["w%d" % i for i in range(V)], EMB, H).eval()
    sd = m.state_dict()
    out["ref/sd_names"] = np.array(list(sd.keys()))
    out["ref/sd_shapes"] = np.array([list(v.shape) + [0] * (2 - v.dim()) for v in sd.values()], np.int64)
    wids = planted_wids(rng, [0, 5, T, 1, 3])
    wids[1, 2] = 0                                                # a zero inside the question: 4 nonzero ids
    lens = ref.process_lengths(torch.from_numpy(wids))
    out["ref/wids"] = wids
    out["ref/lengths"] = np.array([int(n) for n in lens], np.int64)
    x = torch.randn(wids.shape[0], T, 6)
    out["ref/sel_x"] = x.numpy()
    out["ref/sel_out"] = ref.select_last(x, lens).numpy()
    with torch.no_grad():
        m.embedding.weight[0] = torch.randn(EMB) * 0.5
        fw = planted_wids(rng, [T, 4, 6, 2])
        swap = np.array([0, 2, 1, 3])                             # question fw[1] sits at batch position 1, then at position 2
        out["ref/fwd_wids"] = fw
        out["ref/swap"] = swap
        out["ref/fwd"] = m(torch.from_numpy(fw)).numpy()
        out["ref/fwd_swapped"] = m(torch.from_numpy(fw[swap])).numpy()


def from_project(out):
    from vqa.models.seq2vec import TwoLSTM
    for ci, seed in enumerate((0, 1)):
        torch.manual_seed(seed)
        rng = np.random.default_rng(seed)
        enc = TwoLSTM(["w%d" % i for i in range(V)], EMB, H).eval()
        with torch.no_grad():
            enc.embedding.weight[0] = torch.randn(EMB) * 0.5      # padding_idx only zeroes the row at construction
            for p in list(enc.rnn_0.parameters()) + list(enc.rnn_1.parameters()):
                p.mul_(3.0 if ci else 1.0)
        wids = planted_wids(rng, [T, 1, 0, 5, T] + list(rng.integers(1, T + 1, size=B - 5)))
        wids[3, 2] = 0                                            # a zero inside the question: 4 nonzero ids, stepped over t < 4
        n = (wids != 0).sum(1)
        last = np.where(n > 0, n, T) - 1
        with torch.no_grad():
            w = torch.from_numpy(wids)
            q = enc(w).numpy()
            x_0, _ = enc.rnn_0(torch.tanh(enc.embedding(w)))
            x_1, _ = enc.rnn_1(x_0)
        c = "c%d/" % ci
        out[c + "wids"], out[c + "q"] = wids, q
        out[c + "x0"], out[c + "x1"] = x_0.numpy()[np.arange(B), last], x_1.numpy()[np.arange(B), last]
        out[c + "E"] = enc.embedding.weight.detach().numpy()
        for r in ("rnn_0", "rnn_1"):
            for k in KEYS:
                out[c + r + "." + k] = getattr(getattr(enc, r), k).detach().numpy()


def main():
    out = {}
    from_reference(out)
    from_project(out)
    path = os.path.join(ROOT, "tests", "golden", "g19_lstm.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
