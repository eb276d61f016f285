#!/usr/bin/env python3
"""A sweep of the threshold T over the bench's workload: one cut tree against one cut per threshold.

`--chunks` chunks of `synthetic_chunk(--points, seed, tarl=True)` (the bench's configuration: alpha = 1, theta = 0.5, 12 chunks of
200 000 points), their graphs resident on one context.  Timed warm, alternated in one process, the median of `--reps`:
  (a) one `ncuts_tree_batch` at T_max = 0.075 plus one `relabel` at the k = 16 thresholds;
  (b) what the library offered before the tree: 16 `ncuts_labels_batch` calls, one per threshold;
  (c) one `ncuts_labels_batch` at 0.075.
(a)'s labels must equal (b)'s bit for bit at every threshold and chunk (asserted).  (a) / (c) is what the tree costs on top of the
cut that is made anyway; the spread of (c) stands next to it.  One JSON line, printed and written to `--out` (default
profiles/tsweep_line.json).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

T_MAX = 0.075


def thresholds():
    """16 values in [0.005, 0.075]: the three shipped configuration values among a geometric ladder."""
    ts = sorted(set(np.geomspace(0.005, T_MAX, 15).tolist() + [0.03]))
    ts[-1] = T_MAX
    assert len(ts) == 16 and 0.005 in ts and 0.03 in ts
    return ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=12)
    ap.add_argument("--points", type=int, default=200000)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "tsweep_line.json"), help="file that receives the JSON line ('' : none)")
    args = ap.parse_args()
    from autoinst_amd import ncuts_api as api, synth
    ctx = api.Context(0)
    chunks = [synth.synthetic_chunk(args.points, seed=s, tarl=True) for s in range(args.chunks)]
    graphs = [api.build_affinity(c["points"], c["tarl"], alpha=1.0, theta=0.5, gamma=0.0, ctx=ctx) for c in chunks]
    del chunks
    ts = thresholds()
    out = {}

    def tree_relabel():
        trees = api.ncuts_tree_batch(graphs, None, T_MAX, ctx=ctx)
        out["trees"] = trees
        out["a"] = api.relabel(trees, ts, ctx=ctx)

    def direct_sweep():
        out["b"] = [api.ncuts_labels_batch(graphs, None, T, ctx=ctx)[:2] for T in ts]

    def single_cut():
        out["c"] = api.ncuts_labels_batch(graphs, None, T_MAX, ctx=ctx)[:2]

    def timed(fn):
        t0 = time.perf_counter()
        fn()            # every leg ends with its results on the host
        return time.perf_counter() - t0

    legs = (tree_relabel, direct_sweep, single_cut)
    for fn in legs:     # warm: the context's workspace, the code objects
        timed(fn)
    times = {fn.__name__: [] for fn in legs}
    for _ in range(args.reps):
        for fn in legs:
            times[fn.__name__].append(timed(fn))
    labs, counts = out["a"]
    for t, (blabs, bngs) in enumerate(out["b"]):
        assert [int(x) for x in counts[t]] == bngs, f"group counts differ at T = {ts[t]}"
        for c in range(args.chunks):
            assert np.array_equal(labs[t][c], blabs[c]), f"labels differ at T = {ts[t]}, chunk {c}"
    clabs, cngs = out["c"]
    assert all(np.array_equal(t.labels, l) for t, l in zip(out["trees"], clabs)) and [t.n_groups for t in out["trees"]] == cngs
    t_relabel = [timed(lambda: api.relabel(out["trees"], ts, ctx=ctx)) for _ in range(args.reps)]
    med = {k: statistics.median(v) for k, v in times.items()}
    tc = times["single_cut"]
    line = {"tool": "run_tsweep", "chunks": args.chunks, "points": args.points, "T_max": T_MAX, "k": len(ts), "thresholds": ts, "reps": args.reps,
            "groups_at_T_max": int(sum(cngs)), "groups_per_threshold": [int(x) for x in counts.sum(axis=1)],
            "tree_relabel_ms": 1e3 * med["tree_relabel"], "direct_sweep_ms": 1e3 * med["direct_sweep"], "single_cut_ms": 1e3 * med["single_cut"],
            "relabel_alone_ms": 1e3 * statistics.median(t_relabel),
            "tree_relabel_ms_all": [round(1e3 * t, 3) for t in times["tree_relabel"]],
            "direct_sweep_ms_all": [round(1e3 * t, 3) for t in times["direct_sweep"]],
            "single_cut_ms_all": [round(1e3 * t, 3) for t in tc],
            "tree_over_single_cut": med["tree_relabel"] / med["single_cut"], "single_cut_spread": (max(tc) - min(tc)) / med["single_cut"],
            "direct_sweep_over_tree": med["direct_sweep"] / med["tree_relabel"], "labels_equal": True}
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    for g in graphs:
        g.free()
    ctx.close()


if __name__ == "__main__":
    main()
