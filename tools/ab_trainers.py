"""A/B of two builds of the library on the three VQA trainers below the question encoder (MutanNoAtt, MLBNoAtt, MLBAtt): every output of
their forward / backward entry points on the edge cases of tests/trainer_edge_cases.py, written to an .npz by one process per build
(NCX_LIB names the library, as for every tool), then compared bit for bit with tools/ab_encoders.py's compare.  The trainers are
run-to-run bit-identical, so a difference between two builds is the builds'.

  NCX_LIB=/path/to/a.so python tools/ab_trainers.py --out a.npz           (GPU) per trainer, shape and variant: logits, z / att, every
  NCX_LIB=/path/to/b.so python tools/ab_trainers.py --out b.npz                 *_ws_region (after the forward; MLBAtt's again after the
                                                                                backward), every gradient, dq_emb
  ... --sizes --out a_sizes.npz                                           (no GPU) the three *_train_workspace_bytes and every *_ws_region
                                                                                offset and size over a grid holding the edge, the ragged
                                                                                and the real shapes
  python tools/ab_trainers.py --compare a.npz b.npz [--json result.json]  (no GPU) fails unless the two files hold the same arrays and every
                                                                                pair is array_equal
  python tools/ab_trainers.py --compare-sizes a.npz b.npz [--mutan-idx-gone] [--json ...]
                                                                          (no GPU) the same for two --sizes files; with --mutan-idx-gone b's
                                                                                Mutan workspace must be exactly one [B] int32 region
                                                                                (4 B bytes rounded up to 256) smaller at every grid point
                                                                                and its region offsets lower by as much; nothing else
                                                                                may differ

Variants of a shape: dropout mode 0; mode 1 (the generator) at p = 0.5 under two seeds and once with one layer at p = 0 and the others
on; mode 2 (explicit masks, p = 0.5); each with and without dq_emb; each activation switched off once (mode 2, with dq_emb); MLBAtt
under flags 0 and NCX_F_X6."""
import argparse
import ctypes as C
import itertools
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "vqa-counterexamples_amd"), os.path.join(ROOT, "tests"), os.path.dirname(os.path.abspath(__file__))]
import numpy as np  # noqa: E402

from ab_encoders import compare  # noqa: E402

DEV = "cuda:0"
SEEDS = (0x1234567855AA, 0x1234567855AB)
REAL_MUTAN, REAL_MLB, REAL_ATT = (48, 2048, 2400, 360, 360, 360, 10, 2000), (48, 2048, 2400, 1200, 2000), (128, 2048, 2400, 1200, 4, 1200, 2000, 14, 14)


def variants(n_layers, act_names):
    """-> [(tag, mode, p, seed, want_dq, acts off)]"""
    half, out = (0.5,) * n_layers, []
    one_off = tuple(0.0 if i == 1 else 0.5 for i in range(n_layers))
    for want_dq in (True, False):
        dq = "dq" if want_dq else "nodq"
        out.append(("mode0/" + dq, 0, (0.0,) * n_layers, 0, want_dq, ()))
        for i, s in enumerate(SEEDS):
            out.append(("gen_seed%d/%s" % (i, dq), 1, half, s, want_dq, ()))
        out.append(("gen_layer2_p0/" + dq, 1, one_off, SEEDS[0], want_dq, ()))
        out.append(("masks/" + dq, 2, half, 0, want_dq, ()))
    for a in act_names:
        out.append(("masks_no_act_%s/dq" % a, 2, half, 0, True, (a,)))
    return out


def _t(a, dt=None):
    import torch
    t = torch.from_numpy(np.ascontiguousarray(a)).to(DEV)
    return t if dt is None else t.to(dt)


def _nan_grads(mw):
    import torch
    return {k: torch.full_like(v, float("nan")) for k, v in mw.t.items()}


def run_vq(name, shapes, make_case, make_weights, out_of_table, fns, act_names, out):
    """Mutan and MLB: the same dims struct, loss and ops signatures."""
    import torch
    import trainer_edge_cases as E
    from neuralcx import ops
    workspace, forward, backward, region = fns
    for shape in shapes:
        P, feats, q, idx, target, masks = make_case(shape)
        if shape[0] == 33:
            idx = E.gathered_33(feats, out_of_table)
        B, dv, dq, A = shape[0], shape[1], shape[2], shape[-1]
        dz = P["wc"].shape[1]
        f_d, i_d, q_d, t_d = _t(feats), _t(idx, torch.int32), _t(q), _t(target, torch.int32)
        mk_all = torch.cat([_t(m).reshape(-1) for m in masks])
        for tag, mode, p, seed, want_dq, off in variants(3, act_names):
            mw = make_weights(P, shape, off)
            d = ops.vqa_train_dims(B, dv, dq, dz, A, feats.shape[0], p=p, dropout_mode=mode, seed=seed, want_dq=want_dq)
            ws = workspace(d, mw, DEV)
            ws.fill_(0xFF)
            mk = mk_all if mode == 2 else None
            key = "%s/%s/%s/" % (name, "x".join(map(str, shape)), tag)
            logits, z = forward(d, f_d, i_d, q_d, mw, ws, masks=mk)
            out[key + "logits"], out[key + "z"] = logits.cpu().numpy(), z.cpu().numpy()
            for which, rn in ((ops.VT_WS_VD, "ws_vd"), (ops.VT_WS_QD, "ws_qd"), (ops.VT_WS_ZC, "ws_zc")):
                out[key + rn] = region(d, mw, ws, which).cpu().numpy()
            ce = ops.ce_loss(logits, t_d)
            grads = _nan_grads(mw)
            dqe = backward(d, mw, ws, ce["dlogits"], grads, masks=mk)
            out[key + "loss"] = ce["loss"].cpu().numpy()
            for k, g in grads.items():
                out[key + "d" + k] = g.cpu().numpy()
            if dqe is not None:
                out[key + "dq_emb"] = dqe.cpu().numpy()
    torch.cuda.synchronize()
    ops.check_vqa_targets(device=DEV)


def run_att(out):
    import torch
    import mlb_att_ref as R
    import mlb_att_train_ref as TR
    import trainer_edge_cases as E
    from neuralcx import ops
    for shape in E.ATT_EDGE:
        B, dv, dq, dh_att, G, dh_f, A, W, H = shape
        st, maps, q, _ = R.peaked_case(51, *shape, acts={})
        rng = np.random.default_rng(51 + 1000)
        target = rng.integers(0, A, size=B).astype(np.int32)
        mk_all = _t(TR.concat_masks(TR.random_masks(rng, (0.5,) * 6, B, W * H, dv, dq, dh_att, G, dh_f)))
        idx = np.arange(B, dtype=np.int32)
        if B == 13:                                  # a table with repeated, non-identity indices
            idx = rng.integers(0, B, size=B).astype(np.int32)
            idx[1] = idx[0]
        f_d, i_d, q_d, t_d = _t(maps), _t(idx), _t(q), _t(target)
        for (tag, mode, p, seed, want_dq, off), x6 in itertools.product(variants(6, tuple(E.ACT_FIELD)), (False, True)):
            mw = E.att_weights(st, {a: None for a in off}, DEV)
            dt = ops.mlb_att_train_dims(mw, B, W * H, maps.shape[0], p=p, dropout_mode=mode, seed=seed, want_dq=want_dq)
            ws = ops.mlb_att_train_workspace(dt, mw, torch.device(DEV))
            ws.fill_(0xFF)
            mk = mk_all if mode == 2 else None
            key = "mlb_att/%s/%s/%s/" % ("x".join(map(str, shape)), tag, "x6" if x6 else "fp32")
            regions = ((ops.AT_WS_XV, "ws_xv"), (ops.AT_WS_VATT, "ws_vatt"), (ops.AT_WS_T, "ws_t"), (ops.AT_WS_VD, "ws_vd"), (ops.AT_WS_DWV, "ws_dwv"))
            logits, att = ops.mlb_att_train_forward(dt, f_d, i_d, q_d, mw, ws, masks=mk, x6=x6)
            out[key + "logits"], out[key + "att"] = logits.cpu().numpy(), att.cpu().numpy()
            for which, rn in regions[:4]:            # (the dWv_att slab is written by the backward)
                out[key + rn] = ops.mlb_att_train_ws_region(dt, mw, ws, which).cpu().numpy()
            ce = ops.ce_loss(logits, t_d)
            grads = _nan_grads(mw)
            dqe = ops.mlb_att_train_backward(dt, f_d, i_d, q_d, mw, ws, att, ce["dlogits"], grads, masks=mk, x6=x6)
            out[key + "loss"] = ce["loss"].cpu().numpy()
            for which, rn in regions:
                out[key + "bwd_" + rn] = ops.mlb_att_train_ws_region(dt, mw, ws, which).cpu().numpy()
            for k, g in grads.items():
                out[key + "d" + k] = g.cpu().numpy()
            if dqe is not None:
                out[key + "dq_emb"] = dqe.cpu().numpy()
    torch.cuda.synchronize()
    ops.check_vqa_targets(device=DEV)


def run_trainers():
    import torch
    import trainer_edge_cases as E
    from neuralcx import ops
    assert torch.cuda.is_available(), "ab_trainers.py runs the kernels: it needs the GPU (--sizes and the compare modes do not)"
    out = {}
    mutan_w = lambda P, shape, off: ops.MutanWeights.from_tensors({k: _t(v) for k, v in P.items()}, shape[6], *(0 if a in off else 2 for a in "vq"))
    mlb_w = lambda P, shape, off: ops.MlbWeights.from_tensors({k: _t(v) for k, v in P.items()}, *(0 if a in off else 2 for a in "vqc"))
    run_vq("mutan", E.MUTAN_EDGE + [E.MUTAN_RAGGED], E.mutan_case, mutan_w, False,
           (ops.vqa_train_workspace, ops.vqa_train_forward, ops.vqa_train_backward, ops.vqa_train_ws_view), "vq", out)
    run_vq("mlb", E.MLB_EDGE + [E.MLB_RAGGED], E.mlb_case, mlb_w, True,
           (ops.mlb_train_workspace, ops.mlb_train_forward, ops.mlb_train_backward, ops.mlb_train_ws_region), "vqc", out)
    run_att(out)
    return out


# ---- the host-only size functions ------------------------------------------------------------------------------------------------------
def run_sizes():
    import trainer_edge_cases as E
    from neuralcx import _lib
    L = _lib.lib()
    off, nb = C.c_size_t(), C.c_size_t()
    out = {}

    def regions(fn, args, whichs):
        row = []
        for w in whichs:
            rc = fn(*args, w, C.byref(off), C.byref(nb))
            row += [rc, off.value if rc == 0 else 0, nb.value if rc == 0 else 0]
        return row

    drops = [(0, 0.0), (1, 0.5), (1, 0.0), (2, 0.5), (2, 0.0)]
    # Mutan and MLB: rows of (workspace bytes, then rc / offset / bytes of the three regions and of an unknown one)
    vq = (("mutan", E.MUTAN_EDGE + [E.MUTAN_RAGGED, REAL_MUTAN, (0, 8, 8, 8, 8, 8, 1, 8), (4, 8, 8, 8, 8, 8, 11, 8)],
           L.ncx_vqa_train_workspace_bytes, L.ncx_vqa_train_ws_region, ((2, 2), (0, 2), (2, 0))),
          ("mlb", E.MLB_EDGE + [E.MLB_RAGGED, REAL_MLB, (0, 8, 8, 8, 8), (4, 8, 8, 3, 8)],
           L.ncx_mlb_train_workspace_bytes, L.ncx_mlb_train_ws_region, ((2, 2, 2), (2, 2, 0), (0, 2, 2))))
    for name, shapes, ws_bytes, ws_region, act_sets in vq:
        rows = []
        for shape, (mode, p), acts in itertools.product(shapes, drops, act_sets):
            d = _lib.NcxVqaTrainDims()
            d.B, d.dv, d.dq, d.A, d.n_img = shape[0], shape[1], shape[2], shape[-1], shape[0] + 3
            d.p_v, d.p_q, d.p_c, d.dropout_mode = p, p, p, mode
            if name == "mutan":
                m = _lib.NcxMutanParams()
                m.dhv, m.dhq, d.dz, m.R = shape[3:7]
                m.act_v, m.act_q = acts
            else:
                m = _lib.NcxMlbParams()
                m.dh = d.dz = shape[3]
                m.act_v, m.act_q, m.act_c = acts
            a = (C.byref(d), C.byref(m))
            rows.append([ws_bytes(*a)] + regions(ws_region, a, (1, 2, 3, 9)))
        out["sizes/%s" % name] = np.array(rows, np.int64)
        out["grid/%s_B" % name] = np.array([shape[0] for shape, _, _ in itertools.product(shapes, drops, act_sets)], np.int64)
    rows = []
    for shape, (mode, p), p1 in itertools.product(E.ATT_EDGE + [REAL_ATT, (0, 8, 8, 8, 1, 4, 4, 1, 1), (2, 8, 8, 8, 9, 4, 4, 1, 1)], drops, (None, 0.0)):
        B, dv, dq, dh_att, G, dh_f, A, W, H = shape
        one = C.c_void_p(256)                        # never dereferenced: sizing reads dims and activation codes only
        m = _lib.NcxMlbAttParams(**{n: (one if i < 12 else 2) for i, (n, _) in enumerate(_lib.NcxMlbAttParams._fields_)})
        d = _lib.NcxMlbAttDims(B=B, P=W * H, dv=dv, dq=dq, dh_att=dh_att, G=G, dh_f=dh_f, A=A, n_img=B)
        t = _lib.NcxMlbAttTrain(p_att_v=p if p1 is None else p1, p_att_q=p, p_att_mm=p, p_v=p, p_q=p, p_c=p, dropout_mode=mode)
        a = (C.byref(d), C.byref(t), C.byref(m))
        rows.append([L.ncx_mlb_att_train_workspace_bytes(*a)] + regions(L.ncx_mlb_att_train_ws_region, a, (1, 2, 3, 4, 5, 9)))
    out["sizes/mlb_att"] = np.array(rows, np.int64)
    return out


def compare_sizes(path_a, path_b, idx_gone, json_path):
    """b == a; with idx_gone, except Mutan: b's workspace is align_up(4 B, 256) bytes smaller and its region offsets as much lower
    wherever a answers at all."""
    a, b = np.load(path_a), np.load(path_b)
    want = {k: a[k].copy() for k in a.files}
    m = want["sizes/mutan"]
    ok = m[:, 0] > 0
    shift = (4 * a["grid/mutan_B"] + 255) // 256 * 256 if idx_gone else np.zeros(len(m), np.int64)
    m[ok, 0] -= shift[ok]
    for c in (1, 4, 7):                              # (rc, offset, bytes) of the regions VD, QD, ZC: rc == 0 there
        m[ok, c + 1] -= shift[ok]
    differ = sorted(k for k in want if k not in b.files or want[k].shape != b[k].shape or not np.array_equal(want[k], b[k]))
    res = dict(a=os.path.basename(path_a), b=os.path.basename(path_b), arrays=len(a.files), grid_points={k: int(a[k].shape[0]) for k in a.files},
               mutan_points_answered=int(ok.sum()), mutan_shift_bytes=sorted(set(shift[ok].tolist())), only_in_one=sorted(set(a.files) ^ set(b.files)), differ=differ,
               as_expected=not differ and set(a.files) == set(b.files))
    line = json.dumps(res)
    print(line)
    if json_path:
        os.makedirs(os.path.dirname(os.path.abspath(json_path)), exist_ok=True)
        with open(json_path, "w") as f:
            f.write(line + "\n")
    return 0 if res["as_expected"] else 1


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--out", help="the .npz to write (run modes)")
    ap.add_argument("--sizes", action="store_true", help="record the host-only size functions instead of running the kernels")
    ap.add_argument("--compare", nargs=2, metavar=("A", "B"))
    ap.add_argument("--compare-sizes", nargs=2, metavar=("A", "B"))
    ap.add_argument("--mutan-idx-gone", action="store_true", help="with --compare-sizes: B's Mutan workspace lacks the [B] int32 region")
    ap.add_argument("--json", help="with a compare mode: where to write the result line")
    a = ap.parse_args()
    if a.compare:
        return compare(a.compare[0], a.compare[1], a.json)
    if a.compare_sizes:
        return compare_sizes(a.compare_sizes[0], a.compare_sizes[1], a.mutan_idx_gone, a.json)
    if not a.out:
        ap.error("--out is required")
    from neuralcx import _lib
    out = run_sizes() if a.sizes else run_trainers()
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    np.savez(a.out, **out)
    print(json.dumps(dict(lib=_lib.LIB_PATH, out=a.out, arrays=len(out))))
    return 0


if __name__ == "__main__":
    sys.exit(main())
