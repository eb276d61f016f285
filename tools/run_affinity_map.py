#!/usr/bin/env python3
"""The affinity graphs of a map's chunks: ONE `ncuts_api.build_affinity_batch` call against the loop of `build_affinity` calls
(DESIGN.md section 24).

Three sets of synthetic TARL + Spatial chunks (`synth.synthetic_chunk`, 96-d features, seeds 1000 + i), all resident on the device:
  map     the 72 chunks of tools/run_cfg3.py (`chunk_sizes(False)`: 64 of 3k-30k points + 8 of 200k);
  small   its 64 small chunks alone;
  bench   the bench's batch, 12 chunks of 200k points.
Both ways run in this process on one context, from the same resident tensors (the batch takes the concatenated tensors and the
offsets, the loop the per-chunk views), and free their graphs inside the timed window.  After a warm-up of both, windows of
the two ways alternate (`--rounds` each); a window repeats its way until more than `--window` seconds have passed and ends in
a device synchronise; a way's figure is the median over its windows of seconds per repetition.  Every graph of the batch is
compared with the loop's on the device first (row pointers, columns, values, row order: equal bits or the tool stops).

Beside the times: the bytes the build must move by DESIGN section 5's formula, N (3*8 + F*8) + E (4 + 8) + 4 (N + 1), at the
copy rate `bench_copy` measures here; and the launches and host synchronisations of one repetition of each way, counted from
the runtime calls torch's profiler records in this process (kernel launches; memory copies and fills; stream / event
synchronisations and blocking copies; the binding's wait for torch's stream before
each library call is one of them), not estimated.

One JSON line, printed and written to `--out` (default profiles/affinity_map_line.json).  Kernel times come from a separate
run of the small set, both ways in one process: `rocprofv3 --kernel-trace --stats -- python tools/run_affinity_map.py --sets small
--trace --out ""` (profiles/affinity_map_kernels.txt): `--trace` runs each way `--trace-reps` times after the warm-up and
nothing else.
"""
import argparse
import collections
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))

KW = dict(alpha=1.0, theta=0.5, gamma=0.0)
LAUNCH = ("hipLaunchKernel", "hipModuleLaunchKernel", "hipExtLaunchKernel", "hipExtModuleLaunchKernel", "hipLaunchCooperativeKernel",
          "hipExtLaunchMultiKernelMultiDevice", "hipHccModuleLaunchKernel")
COPY = ("hipMemcpyAsync", "hipMemsetAsync", "hipMemcpyDtoDAsync", "hipMemcpyHtoDAsync", "hipMemcpyDtoHAsync", "hipMemsetD8Async",
        "hipMemsetD32Async", "hipMemcpyWithStream")
# (hipDeviceSynchronize is left out: neither way calls it, the two the profiler shows are this tool's own and the profiler's)
SYNC = ("hipStreamSynchronize", "hipEventSynchronize", "hipMemcpy", "hipMemcpyDtoH", "hipMemcpyHtoD", "hipMemcpyDtoD", "hipMemset")
ALLOC = ("hipMalloc", "hipFree", "hipMallocAsync", "hipFreeAsync", "hipHostMalloc", "hipHostFree")


def chunk_set(name):
    from run_cfg3 import chunk_sizes
    sizes = chunk_sizes(False)
    if name == "map":
        return sizes, list(range(len(sizes)))
    if name == "small":
        return sizes[:64], list(range(64))
    if name == "bench":
        return [200_000] * 12, list(range(64, 76))
    raise ValueError(name)


class Work:
    """One set, resident: the concatenated tensors with their offsets, and the per-chunk views of the same memory."""

    def __init__(self, name, cache):
        import torch
        from autoinst_amd import synth
        self.name = name
        self.sizes, ids = chunk_set(name)
        for i, n in zip(ids, self.sizes):
            if (i, n) not in cache:
                d = synth.synthetic_chunk(n, seed=1000 + i, tarl=True)
                cache[(i, n)] = (torch.from_numpy(d["points"]).cuda(), torch.from_numpy(np.ascontiguousarray(d["tarl"], dtype=np.float64)).cuda())
        self.pts = torch.cat([cache[(i, n)][0] for i, n in zip(ids, self.sizes)])
        self.tarl = torch.cat([cache[(i, n)][1] for i, n in zip(ids, self.sizes)])
        self.off = np.concatenate([[0], np.cumsum(self.sizes)]).astype(np.int64)
        self.views = [(self.pts[a:b], self.tarl[a:b]) for a, b in zip(self.off[:-1], self.off[1:])]

    def batch(self, api, ctx, group_rows=None):
        return api.build_affinity_batch(self.pts, self.tarl, offsets=self.off, group_rows=group_rows, ctx=ctx, **KW)

    def loop(self, api, ctx):
        return [api.build_affinity(p, t, ctx=ctx, **KW) for p, t in self.views]


def _free(graphs):
    for g in graphs:
        g.free()


def same_bits(ga, gb):
    """Two device graphs hold the same bits in rowptr / col / val / orig (read through their exports: original order, sorted columns)."""
    A, B = ga.to_scipy(), gb.to_scipy()
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and \
        np.array_equal(A.data.view(np.int64), B.data.view(np.int64))


def window(fn, seconds, sync):
    """Repeat fn (build + free) until `seconds` have passed; -> (seconds per repetition, repetitions)."""
    sync()
    reps, t0 = 0, time.perf_counter()
    while True:
        _free(fn())
        reps += 1
        if time.perf_counter() - t0 > seconds:
            break
    sync()
    return (time.perf_counter() - t0) / reps, reps


def count_calls(fn, sync):
    """Runtime calls of ONE repetition of fn, by the names torch's profiler records on the host side."""
    from torch.profiler import ProfilerActivity, profile
    sync()
    with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
        _free(fn())
        sync()
    names = collections.Counter(e.name for e in prof.events() if e.name.startswith("hip"))
    pick = lambda keys: int(sum(names.get(k, 0) for k in keys))
    kernels = sum(1 for e in prof.events() if str(e.device_type).endswith("CUDA") and not e.name.lower().startswith(("memcpy", "memset")))
    return {"kernel_launches": pick(LAUNCH), "copies_and_fills": pick(COPY), "host_synchronisations": pick(SYNC),
            "allocations": pick(ALLOC), "device_kernels_seen": int(kernels), "calls": dict(sorted(names.items()))}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sets", default="map,small,bench")
    ap.add_argument("--window", type=float, default=1.0, help="least seconds of one timed window")
    ap.add_argument("--rounds", type=int, default=3, help="windows per way, alternating")
    ap.add_argument("--group-rows", type=int, default=0, help="group budget of the batched call (0: the library's default)")
    ap.add_argument("--trace", action="store_true", help="after the warm-up run each way --trace-reps times and stop (for rocprofv3)")
    ap.add_argument("--trace-reps", type=int, default=5)
    ap.add_argument("--no-counts", action="store_true", help="skip the profiler pass that counts launches and synchronisations")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "affinity_map_line.json"), help="file for the JSON line ('': none)")
    args = ap.parse_args()
    import torch
    from autoinst_amd import ncuts_api as api
    ctx = api.default_context()
    sync = torch.cuda.synchronize
    cache, line = {}, {"tool": "run_affinity_map", "weights": KW, "tarl_dim": 96, "window_s": args.window, "rounds": args.rounds,
                       "group_rows": args.group_rows or 1 << 21}
    if not args.trace:
        line["copy_GBps"] = api.bench_copy(ctx)
    for name in args.sets.split(","):
        w = Work(name, cache)
        ways = {"batch": lambda: w.batch(api, ctx, args.group_rows or None), "loop": lambda: w.loop(api, ctx)}
        # warm-up of both (workspace, graph-buffer cache, code objects) and the comparison
        ga, gb = ways["batch"](), ways["loop"]()
        nnz = [g.nnz for g in gb]
        equal = all(same_bits(a, b) for a, b in zip(ga, gb)) if not args.trace else None
        _free(ga + gb)
        if equal is False:
            raise SystemExit(f"{name}: a graph of the batched call differs from the single build's")
        for fn in ways.values():
            _free(fn())
        sync()
        if args.trace:
            for fn in ways.values():
                for _ in range(args.trace_reps):
                    _free(fn())
                sync()
            line[name] = {"chunks": len(w.sizes), "points": int(w.off[-1]), "trace_reps_per_way": args.trace_reps}
            continue
        per = {k: [] for k in ways}
        reps = {k: [] for k in ways}
        for _ in range(args.rounds):
            for k, fn in ways.items():
                t, r = window(fn, args.window, sync)
                per[k].append(t)
                reps[k].append(r)
        n, e = int(w.off[-1]), int(sum(nnz))
        must = n * (3 * 8 + 96 * 8) + e * (4 + 8) + 4 * (n + len(w.sizes))
        rec = {"chunks": len(w.sizes), "points": n, "entries": e, "graphs_equal_bits": equal,
               "batch_ms": 1e3 * statistics.median(per["batch"]), "loop_ms": 1e3 * statistics.median(per["loop"]),
               "batch_ms_all": [round(1e3 * t, 3) for t in per["batch"]], "loop_ms_all": [round(1e3 * t, 3) for t in per["loop"]],
               "reps_per_window": {k: reps[k] for k in ways}, "bytes_must_move": must, "ms_at_copy_rate": 1e3 * must / (line["copy_GBps"] * 1e9)}
        rec["loop_over_batch"] = rec["loop_ms"] / rec["batch_ms"]
        if not args.no_counts:
            rec["counts"] = {k: count_calls(fn, sync) for k, fn in ways.items()}
        line[name] = rec
        del w, ways
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
