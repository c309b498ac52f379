"""A/B of two builds of the library on the question encoders: every output of the GRU and the TwoLSTM entry points on the edge cases of
tests/gru_edge_cases.py and tests/lstm_edge_cases.py, written to an .npz by one process per build (NCX_LIB names the library, as for
every tool), then compared bit for bit.  The four entry families are run-to-run bit-identical, so a difference between two builds is the
builds'.

  NCX_LIB=/path/to/a.so python tools/ab_encoders.py --out a.npz           (GPU) per case and encoder: the device packs (packed, packed_t),
  NCX_LIB=/path/to/b.so python tools/ab_encoders.py --out b.npz                 q of *_encode, q of *_train_forward, every gradient of
                                                                                *_train_backward with dE and without
  ... --sizes --out a_sizes.npz                                           (no GPU) the four *_workspace_bytes and the four *packed*_bytes
                                                                                functions over a grid holding the edge and the real shapes
  python tools/ab_encoders.py --compare a.npz b.npz [--json result.json]  (no GPU) fails unless the two files hold the same arrays and every
                                                                                pair is array_equal; the JSON lists case and array names"""
import argparse
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd"), os.path.join(ROOT, "tests")]
import numpy as np  # noqa: E402

WKEYS = ("weight_ih_l0", "weight_hh_l0", "bias_ih_l0", "bias_hh_l0")
REAL = {"gru": (620, 2400), "lstm": (620, 1200)}                 # (emb, hidden) of the encoders the VQA models are built with
SIZE_FNS = {"gru": ("ncx_gru_workspace_bytes", "ncx_gru_train_workspace_bytes", "ncx_gru_packed_bytes", "ncx_gru_packed_t_bytes"),
            "lstm": ("ncx_lstm2_workspace_bytes", "ncx_lstm2_train_workspace_bytes", "ncx_lstm2_packed_bytes", "ncx_lstm2_packed_t_bytes")}


def run_sizes():
    from gru_edge_cases import CASES
    from neuralcx import _lib
    L = _lib.lib()
    dims = sorted({c[:2] for c in CASES.values()} | set(REAL.values()) | {(0, 8), (8, 0), (31, 32), (32, 31), (64, 64), (1 << 24, 8)})
    rows = sorted({c[2] for c in CASES.values()} | {1, 63, 64, 256, 257, 512, 0})
    steps = sorted({c[3] for c in CASES.values()} | {1, 26, 63, 65, 0})
    out = {"dims": np.array(dims, np.int64), "rows": np.array(rows, np.int64), "steps": np.array(steps, np.int64)}
    for enc, (ws, ws_train, packed, packed_t) in SIZE_FNS.items():
        for fn in (packed, packed_t):
            out["sizes/%s/%s" % (enc, fn)] = np.array([getattr(L, fn)(e, h) for e, h in dims], np.uint64)
        for fn in (ws, ws_train):
            out["sizes/%s/%s" % (enc, fn)] = np.array([getattr(L, fn)(b, t, e, h) for (e, h), b, t in itertools.product(dims, rows, steps)],
                                                      np.uint64)
    return out


def run_gru(name, dev, out):
    import torch
    from gru_edge_cases import CASES, V, make
    from neuralcx import ops
    from vqa.models.seq2vec import GRUEncoder
    de, dq, _, _ = CASES[name]
    wids, E, w_ih, w_hh, b_ih, b_hh, dq_out = make(name)
    enc = GRUEncoder(["w%d" % i for i in range(V)], dim_q=dq, dim_emb=de, dropout=0.25).eval()
    sd = {"embedding.weight": torch.from_numpy(E)}
    sd.update({"gru." + k: torch.from_numpy(a) for k, a in zip(WKEYS, (w_ih, w_hh, b_ih, b_hh))})
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev)
    w, dqo = torch.from_numpy(wids).to(dev), torch.from_numpy(dq_out).to(dev)
    put = lambda key, t: out.__setitem__("gru/%s/%s" % (name, key), t.cpu().numpy())
    put("encode.q", ops.gru_encode(w, ops.gru_weights(enc)))
    gw = ops.gru_train_weights(enc.embedding.weight.detach(), *[getattr(enc.gru, k).detach() for k in WKEYS])
    put("packed", gw.packed)
    put("packed_t", gw.packed_t)
    for tag, want_dE in (("dE", True), ("no_dE", False)):
        ws = ops.gru_train_workspace(w.shape[0], w.shape[1], gw, dev)
        put("train_%s.q" % tag, ops.gru_train_forward(w, gw, ws))
        for k, g in ops.gru_train_backward(w, gw, ws, dqo, want_dE=want_dE).items():
            if g is not None:
                put("train_%s.d%s" % (tag, k), g)
    ops.check_gru_ids(device=dev)


def run_lstm(name, dev, out):
    import torch
    from lstm_edge_cases import CASES, V, make
    from neuralcx import ops
    from vqa.models.seq2vec import TwoLSTM
    emb, H, _, _ = CASES[name]
    wids, E, l0, l1, dq_out = make(name)
    enc = TwoLSTM(["w%d" % i for i in range(V)], emb, H).eval()
    sd = {"embedding.weight": torch.from_numpy(E)}
    sd.update({"rnn_%d.%s" % (l, k): torch.from_numpy(a) for l, layer in enumerate((l0, l1)) for k, a in zip(WKEYS, layer)})
    enc.load_state_dict(sd, strict=True)
    enc = enc.to(dev)
    w, dqo = torch.from_numpy(wids).to(dev), torch.from_numpy(dq_out).to(dev)
    put = lambda key, t: out.__setitem__("lstm/%s/%s" % (name, key), t.cpu().numpy())
    put("encode.q", ops.lstm_encode(w, ops.lstm_weights(enc)))
    lw = ops.lstm_train_weights(enc.embedding.weight.detach(), *[getattr(r, k).detach() for r in (enc.rnn_0, enc.rnn_1) for k in WKEYS])
    put("packed", lw.packed)
    put("packed_t", lw.packed_t)
    for tag, want_dE in (("dE", True), ("no_dE", False)):
        ws = ops.lstm_train_workspace(w.shape[0], w.shape[1], lw, dev)
        put("train_%s.q" % tag, ops.lstm_train_forward(w, lw, ws))
        for k, g in ops.lstm_train_backward(w, lw, ws, dqo, want_dE=want_dE).items():
            if g is not None:
                put("train_%s.d%s" % (tag, k), g)
    ops.check_gru_ids(device=dev)


def run_encoders():
    import torch
    from gru_edge_cases import CASES
    assert torch.cuda.is_available(), "ab_encoders.py runs the kernels: it needs the GPU (--sizes and --compare do not)"
    out = {}
    for name in CASES:
        run_gru(name, "cuda:0", out)
        run_lstm(name, "cuda:0", out)
    torch.cuda.synchronize()
    return out


def compare(path_a, path_b, json_path):
    a, b = np.load(path_a), np.load(path_b)
    missing = sorted(set(a.files) ^ set(b.files))
    differ = [k for k in sorted(set(a.files) & set(b.files))
              if a[k].shape != b[k].shape or a[k].dtype != b[k].dtype or not np.array_equal(a[k], b[k], equal_nan=True)]
    cases = {}
    for k in sorted(a.files):
        group, _, arr = k.rpartition("/")
        cases.setdefault(group or "grid", []).append(arr)
    res = dict(a=os.path.basename(path_a), b=os.path.basename(path_b), arrays=len(a.files), cases=cases, only_in_one=missing, differ=differ,
               all_equal=not missing and not differ)
    line = json.dumps(res)
    print(line)
    if json_path:
        os.makedirs(os.path.dirname(os.path.abspath(json_path)), exist_ok=True)
        with open(json_path, "w") as f:
            f.write(line + "\n")
    return 0 if res["all_equal"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="the .npz to write (run modes)")
    ap.add_argument("--sizes", action="store_true", help="record the host-only size functions instead of running the kernels")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--json", help="with --compare: where to write the result line")
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.json)
    if not a.out:
        ap.error("--out is required")
    from neuralcx import _lib
    out = run_sizes() if a.sizes else run_encoders()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print(json.dumps(dict(lib=_lib.LIB_PATH, out=a.out, arrays=len(out))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
