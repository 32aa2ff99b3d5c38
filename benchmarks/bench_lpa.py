#!/usr/bin/env python
"""Label propagation communities (gl_lpa) on the six stand-ins and on orkut_community, one GPU.

Per graph one JSON line for the colour-class schedule under gl_color's largest-first colouring of the same plan:
  call_ms          gl_lpa alone (it synchronises itself), wall clock: median of `runs` after three untimed runs; call_ms_min /
                   call_ms_max: the spread.  The plan's first call (verdicts, scratch) is timed once as first_call_ms
  sweeps, changes, evaluations, launches, converged, colours
                   gl_lpa's statistics and the classes swept; ms_per_sweep = call_ms / sweeps
  communities, largest_community, modularity
                   over the real vertices; Newman's modularity on the host (app.LabelPropagation.modularity's formula)
  color_ms         gl_color on the same plan in the same process; call_over_color = call_ms / color_ms
  sweep_bytes      8 * entries: 4 B index + one 4 B label gather per entry, what a sweep over every row must move at least
  model_ms         sweeps * sweep_bytes at 6.29 TB/s (the measured float4-copy rate of the card): every sweep as ONE streaming
                   pass over the entries; call_over_model = call_ms / model_ms
  sync_ms, sync_sweeps, sync_ms_per_sweep, sync_converged
                   the synchronous schedule (no colouring) on the same plan, capped at the colour-class run's sweeps
  purity           orkut_community only: the share of the real vertices whose planted community is the most frequent one
                   among the vertices carrying their label (a reported figure, not a bar)
--ab adds one short line per knob value ("ab": "lpa_cut=0", call_ms and the statistics), timed on the same plan in the same
process right behind the default line (the knobs are read per call): lpa_cut 0 / 4 / 8, lpa_grid 2 / 4 / 8 / 16, lpa_batch
1 / 2 / 4 / 8 / 16, lpa_table 128 / 256 / 512 / 1024 / 2048, lpa_active 0 / 1.
Knobs for same-box A/B pairs go through GRAPHLILY_DEBUG and are recorded with every line.

    python benchmarks/bench_lpa.py [--graphs googleplus,orkut_community] [--scale 0.125] [--ab] [--out profiles/lpa.jsonl]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "benchmarks"))

from bench_kcore import wall_ms  # noqa: E402
from bench_msf import COPY_BYTES_PER_S  # noqa: E402
from bench_truss import _with_knob  # noqa: E402

LPA_CUT, LPA_GRID, LPA_BATCH, LPA_TABLE, LPA_ACTIVE = 8, 8, 4, 2048, 1          # the library's defaults (csrc/gl_lpa.hip)

AB = [("lpa_cut", v) for v in (0, 4, 8)] + [("lpa_grid", v) for v in (2, 4, 8, 16)] + [("lpa_batch", v) for v in (1, 2, 4, 8, 16)] + \
     [("lpa_table", v) for v in (128, 256, 512, 1024, 2048)] + [("lpa_active", v) for v in (0, 1)]


def planted_communities(n, seed, mean_size=2048):
    """the community of every vertex of datasets.community_torch(n, ..., seed) without shuffling: its sizes, drawn again"""
    rs = np.random.default_rng(seed)
    sizes, total = [], 0
    while total < n:
        sz = max(16, int(mean_size * 2.0 ** rs.uniform(-2.0, 2.0)))
        sizes.append(min(sz, n - total))
        total += sizes[-1]
    return np.repeat(np.arange(len(sizes)), sizes)


def purity_of(labels, planted):
    """the share of the vertices whose planted community is the most frequent one among the vertices carrying their label"""
    _, ident = np.unique(labels, return_inverse=True)
    key, count = np.unique(ident.astype(np.int64) * (int(planted.max()) + 1) + planted, return_counts=True)
    best = np.zeros(int(ident.max()) + 1, dtype=np.int64)
    np.maximum.at(best, key // (int(planted.max()) + 1), count)
    return float(best.sum()) / labels.shape[0]


def modularity_of(sym, deg, labels):
    _, ident = np.unique(labels, return_inverse=True)
    rows = np.repeat(np.arange(sym.num_rows, dtype=np.int64), np.diff(sym.adj_indptr.astype(np.int64)))
    same = ident[rows] == ident[sym.adj_indices.astype(np.int64)]
    inside = np.bincount(ident[rows][same], minlength=int(ident.max()) + 1)
    degree = np.bincount(ident, weights=deg.astype(np.float64), minlength=inside.shape[0])
    return float(np.sum(inside / float(sym.nnz) - (degree / float(sym.nnz)) ** 2)) if sym.nnz else 0.0


def run_graph(name, raw, runs=5, ab=False, max_sweeps=100, planted=None):
    from graphlily_amd import capi, io
    t0 = time.perf_counter()
    padded = raw.copy()
    io.util_round_csr_matrix_dim(padded, 128, 128)
    sym, deg = io.symmetrize_simple(padded)
    prepare_s = time.perf_counter() - t0
    n, nnz, n_real = sym.num_rows, sym.nnz, raw.num_rows
    plan = capi.SpMVPlan(n, n, sym.adj_indptr, sym.adj_indices, sym.adj_data, 0, n, flags=capi.GL_PLAN_BOOLEAN)
    label, color = capi.DeviceBuffer(4 * max(1, n)), capi.DeviceBuffer(4 * max(1, n))
    prio = capi.DeviceBuffer.from_host(io.coloring_priorities(deg, "largest_first", 0))
    color_stats = plan.color(prio, color)
    color_ms = wall_ms(lambda: plan.color(prio, color), runs)
    capi.sync()
    t0 = time.perf_counter()
    stats = plan.lpa(label, color, None, max_sweeps)
    first_call_ms = (time.perf_counter() - t0) * 1e3
    print("%s: %d sweeps, %d changes, %d evaluations, %d launches, converged %d" % ((name,) + stats), file=sys.stderr, flush=True)
    call_ms = wall_ms(lambda: plan.lpa(label, color, None, max_sweeps), runs)
    got = label.read(np.uint32, n)
    sizes = np.unique(got[:n_real], return_counts=True)[1]
    sync_stats = plan.lpa(label, None, None, stats[0])
    sync_ms = wall_ms(lambda: plan.lpa(label, None, None, stats[0]), runs)
    model_ms = stats[0] * 8.0 * nnz / COPY_BYTES_PER_S * 1e3
    knobs = dict(kv.split("=", 1) for kv in os.environ.get("GRAPHLILY_DEBUG", "").split(",") if kv)
    rec = {"graph": name, "n": n, "nnz": raw.nnz, "symmetric_entries": nnz, "longest_row": int(deg.max()) if n else 0,
           "sweeps": stats[0], "changes": stats[1], "evaluations": stats[2], "launches": stats[3], "converged": stats[4],
           "colours": color_stats[0], "communities": int(sizes.shape[0]), "largest_community": int(sizes.max()),
           "modularity": round(modularity_of(sym, deg, got), 6),
           "call_ms": round(call_ms[0], 4), "call_ms_min": round(call_ms[1], 4), "call_ms_max": round(call_ms[2], 4),
           "first_call_ms": round(first_call_ms, 4), "ms_per_sweep": round(call_ms[0] / stats[0], 4),
           "color_ms": round(color_ms[0], 4), "call_over_color": round(call_ms[0] / color_ms[0], 3) if color_ms[0] > 0 else None,
           "sweep_bytes": 8 * nnz, "model_ms": round(model_ms, 4), "call_over_model": round(call_ms[0] / model_ms, 2) if model_ms > 0 else None,
           "sync_ms": round(sync_ms[0], 4), "sync_sweeps": sync_stats[0], "sync_converged": sync_stats[4],
           "sync_ms_per_sweep": round(sync_ms[0] / sync_stats[0], 4), "runs": runs, "prepare_s": round(prepare_s, 3),
           "lpa_cut": int(knobs.get("lpa_cut", LPA_CUT)), "lpa_grid": int(knobs.get("lpa_grid", LPA_GRID)),
           "lpa_batch": int(knobs.get("lpa_batch", LPA_BATCH)), "lpa_table": int(knobs.get("lpa_table", LPA_TABLE)),
           "lpa_active": int(knobs.get("lpa_active", LPA_ACTIVE)), "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}
    if planted is not None:
        rec["purity"] = round(purity_of(got[:n_real], planted[:n_real]), 4)
        rec["planted_communities"] = int(planted.max()) + 1
    yield rec
    for key, value in AB if ab else ():
        res = _with_knob(key, value, lambda: (plan.lpa(label, color, None, max_sweeps), wall_ms(lambda: plan.lpa(label, color, None, max_sweeps), runs)))
        assert (res[0][0], res[0][1], res[0][4]) == (stats[0], stats[1], stats[4]) and np.array_equal(label.read(np.uint32, n), got)
        yield {"graph": name, "ab": "%s=%d" % (key, value), "call_ms": round(res[1][0], 4), "call_ms_min": round(res[1][1], 4),
               "call_ms_max": round(res[1][2], 4), "launches": res[0][3], "evaluations": res[0][2], "sweeps": stats[0], "runs": runs,
               "knobs": os.environ.get("GRAPHLILY_DEBUG", "")}


def main():
    ap = argparse.ArgumentParser()
    from graphlily_amd import datasets
    ap.add_argument("--graphs", default=",".join(list(datasets.PAPER_GRAPHS) + ["orkut_community"]))
    ap.add_argument("--scale", type=float, default=0.125, help="of the paper graphs' vertices and entries")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "lpa.jsonl"))
    ap.add_argument("--runs", type=int, default=5)
    ap.add_argument("--max-sweeps", type=int, default=100)
    ap.add_argument("--ab", action="store_true", help="also time every knob value on the same plan")
    args = ap.parse_args()
    import torch
    from graphlily_amd import capi
    dev = torch.device("cuda:0")
    capi.init(0)
    for name in args.graphs.split(","):
        raw = datasets.paper_graph(name, args.scale, device=dev)
        planted = None
        if name == "orkut_community":
            planted = planted_communities(raw.num_rows, datasets.EXTRA_GRAPHS[name]["seed"])
        for rec in run_graph(name, raw, runs=args.runs, ab=args.ab, max_sweeps=args.max_sweeps, planted=planted):
            rec["scale"] = args.scale
            rec["data"] = "synthetic stand-in"
            print(json.dumps(rec), flush=True)
            if args.out:
                os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
                with open(args.out, "a") as f:
                    f.write(json.dumps(rec) + "\n")


if __name__ == "__main__":
    main()
