#!/usr/bin/env python
"""SDDMM (gl_sddmm): one score per stored entry of A from the k features of its row and of its column, on the stand-ins under
(+,x), one GPU, one process, next to the way the scores are computed without it: torch gathers of the two k-column blocks and a
row-wise dot on the device.

Per (stand-in, k) one JSON line:
  sddmm_ms         one gl_sddmm call by HIP events on the library's stream: median / min / max of `runs` after three untimed calls
  torch_ms         (X[row_of] * Y[col]).sum(1) * a in torch on the same device, in slabs of entries that keep the gathered blocks
                   under 512 MiB, timed by torch events around all slabs; ALTERNATED run by run with the call above
  speedup          torch_ms / sddmm_ms (medians)
  paths            rows on the short path, pieces on the piece path, feature tiles
  model_bytes      what the model moves: per entry 8 bytes (column, value) + 4 k bytes of Y + 4 bytes out, per row 4 k bytes of X;
                   model_gbs = model_bytes / sddmm_ms
The scores of the first 50000 entries' rows are checked with app.validate_sddmm before anything is timed.  --sweep adds, per stand-in at
k = 64, one line per (sddmm_cut, sddmm_piece) pair of the sweep (the knobs are read by every call; cut -1 = sddmm_short=0).
    python benchmarks/bench_sddmm.py [--graphs googleplus] [--scale 0.125] [--ks 4,16,64,256] [--sweep] [--out profiles/sddmm.jsonl]
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SWEEP_CUTS, SWEEP_PIECES = (-1, 8, 32, 128), (64, 256, 1024, 4096)


def timed(fn):
    from graphlily_amd import capi
    capi.span_begin()
    fn()
    return capi.span_end()


def torch_timed(fn):
    import torch
    t0, t1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    t0.record()
    fn()
    t1.record()
    t1.synchronize()
    return t0.elapsed_time(t1)


def set_knobs(cut, piece):
    if cut is None:
        os.environ.pop("GRAPHLILY_DEBUG", None)
    else:
        os.environ["GRAPHLILY_DEBUG"] = ("sddmm_short=0" if cut < 0 else "sddmm_cut=%d" % cut) + ",sddmm_piece=%d" % piece


def run_graph(name, g, ks, runs=9, sweep=False):
    import torch
    from graphlily_amd import app, module as M
    n, nc, nnz = g.num_rows, g.num_cols, g.nnz
    rng = np.random.default_rng(7)
    dev = torch.device("cuda:0")
    indptr = np.asarray(g.adj_indptr).astype(np.int64)
    t_row = torch.from_numpy(np.repeat(np.arange(n), np.diff(indptr[:n + 1]))).to(dev)
    t_col = torch.from_numpy(np.asarray(g.adj_indices[:nnz]).astype(np.int64)).to(dev)
    t_a = torch.from_numpy(np.asarray(g.adj_data[:nnz], np.float32)).to(dev)
    mm = M.SDDMMModule()
    mm.set_semiring(M.ArithmeticSemiring)
    mm.load_and_format_matrix(g)
    mm.send_matrix_host_to_device()
    check_rows = (0, max(1, int(np.searchsorted(indptr[:n + 1], 50000, side="right")) - 1))     # the rows of the first 50000 entries
    out = []
    for k in ks:
        x, y = rng.standard_normal((n, k)).astype(np.float32), rng.standard_normal((nc, k)).astype(np.float32)
        mm.send_features_host_to_device(x, y)
        t_x, t_y, t_out = torch.from_numpy(x).to(dev), torch.from_numpy(y).to(dev), torch.empty(nnz, dtype=torch.float32, device=dev)
        slab = max(1, (512 << 20) // (8 * k))

        def torch_once():
            for b in range(0, nnz, slab):
                e = min(nnz, b + slab)
                t_out[b:e] = (t_x[t_row[b:e]] * t_y[t_col[b:e]]).sum(1) * t_a[b:e]

        def sddmm_once():
            mm.plan_.sddmm(mm.a_val_buf, mm.x_buf, mm.y_buf, mm.results_buf, k, M.kMulAdd, 0.0)

        for cut, piece in [(None, None)] + ([(c, p) for c in SWEEP_CUTS for p in SWEEP_PIECES] if sweep and k == 64 else []):
            set_knobs(cut, piece)
            mm.run()
            checked = int(indptr[check_rows[1]])
            if checked <= 200000:      # (a hub row among the first would make the f64 reference of k columns per entry too large)
                app.validate_sddmm(g, x, y, mm.results_buf.read(np.float32, checked), M.ArithmeticSemiring, rows=check_rows)
            for _ in range(3):
                timed(sddmm_once)
                if cut is None:
                    torch_timed(torch_once)
            t_mm, t_th = [], []
            for _ in range(runs):
                t_mm.append(timed(sddmm_once))
                if cut is None:
                    t_th.append(torch_timed(torch_once))
            model = nnz * (8 + 4 * k + 4) + 4 * n * k
            med = float(np.median(t_mm))
            rec = {"graph": name, "k": k, "n": n, "nnz": nnz, "knobs": os.environ.get("GRAPHLILY_DEBUG", ""), "paths": list(mm.stats_),
                   "entries_checked": checked if checked <= 200000 else 0,
                   "sddmm_ms": round(med, 4), "sddmm_min_ms": round(min(t_mm), 4), "sddmm_max_ms": round(max(t_mm), 4),
                   "model_bytes": model, "model_gbs": round(model / (1e-3 * med) / 1e9, 1) if med > 0 else None}
            if t_th:
                med_th = float(np.median(t_th))
                rec.update({"torch_ms": round(med_th, 4), "torch_min_ms": round(min(t_th), 4), "torch_max_ms": round(max(t_th), 4),
                            "speedup": round(med_th / med, 3) if med > 0 else None})
            out.append(rec)
        set_knobs(None, None)
    return out


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(datasets.PAPER_GRAPHS))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--ks", default="4,16,64,256")
    ap.add_argument("--sweep", action="store_true", help="at k = 64, every (sddmm_cut, sddmm_piece) pair of the sweep")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "sddmm.jsonl"))
    ap.add_argument("--runs", type=int, default=9)
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        g = datasets.paper_graph(name, args.scale, device=dev)
        for rec in run_graph(name, g, [int(k) for k in args.ks.split(",")], runs=args.runs, sweep=args.sweep):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
