#!/usr/bin/env python3
"""The tail of the reference's loop (run_pipeline.py:214-238) for 16 label maps of one merged map: one `labels_api.label_tables`
call against what the package offered before it, on the same resident data.

The map is `tools/run_merge.py`'s synthetic street (72 chunks with bit-identical overlaps), merged by `merge_map`.  The ground truth
is the street's object id per point, carried into the merged order by the source positions `merge_map` returns.  The 16 label rows
unite the merged instance ids under 16 seeded maps, coarser from row to row; in every row the ground (id 0) is united with a few
objects, so that row has a label that `remove_semantics` removes, and a tenth of the ids map to labels of their own that stay
small.  Everything stays on the device.

In one process, warm, each leg ending in a device synchronise, (a) and (b) alternating `--reps` (>= 10) times:
  (a) one label_tables call with return_labels=True;
  (b) per row ai_label_pairs with AI_MEM_DEVICE through ctypes, rules S2 / S3 decided on the host from the pairs, and a torch
      gather through a per-label table for pred_removed and pred_scored;
  (c) tests/score_ref.py's NumPy remove_semantics of row 0 on one core, once (`--no-restated` skips it).
(a) and (b) must agree in every byte.  Reported: median and spread (max - min) of (a) and (b), the host arithmetic of `score_sweep`
on (a)'s tables on its own, and (d) the bytes (a) must move -- (k + 1) * 4 * n read, 4 * k * n written per label output -- with the
time they take at the box's copy rate (`ai_bench_copy`).  One JSON line, printed and written to `--out` (default
profiles/score_map_line.json).  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/run_score.py --only-tables --reps 1 --out ""` run (profiles/score_map_kernels.txt).

The score itself, on the same rows and alternating in the same way:
  (e) `score_sweep(..., instance_level="device")`: the greedy matching and S_assoc on the device (`ai_label_scores`), AP on the host
      from the hit flags;
  (f) `score_sweep(..., instance_level="host")`: `label_tables`, then the instance-level arithmetic on dense tables on the host.
(e) and (f) must give equal dicts.  Reported in a second JSON line (`--inst-out`, default profiles/score_inst_line.json): median and
spread of both, the device call and the host finish of (e) on their own, and the host synchronisations of one call.  `--only-scores`
runs (e) and (f) alone, `--only-device-scores` (e) alone -- for the kernel trace (profiles/score_inst_kernels.txt).
"""
import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tools"))


def label_rows(torch, g, k, seed=0):
    """(k, n) int32: the merged ids united under k seeded maps.  Row t has about top / (t + 2) labels; id 0 shares its label with
    the ids the map sends there; every tenth id keeps a label of its own above the united ones."""
    top = int(g.max()) + 1
    rows = []
    for t in range(k):
        rng = np.random.default_rng([seed, t])
        groups = max(top // (t + 2), 2)
        m = 1 + rng.integers(0, groups, top)
        own = rng.random(top) < 0.1
        m[own] = groups + 1 + np.flatnonzero(own)
        rows.append(torch.from_numpy(m.astype(np.int32)).cuda()[g.long()])
    return torch.stack(rows).contiguous()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=72)
    ap.add_argument("--rows", type=int, default=16)
    ap.add_argument("--reps", type=int, default=11)
    ap.add_argument("--step", type=float, default=0.2)
    ap.add_argument("--threshold", type=float, default=0.8)
    ap.add_argument("--min-points", type=int, default=200)
    ap.add_argument("--only-tables", action="store_true", help="(a) alone: for a rocprofv3 kernel trace")
    ap.add_argument("--no-restated", action="store_true", help="skip (c), the NumPy restatement on one core")
    ap.add_argument("--only-scores", action="store_true", help="(e) and (f) alone")
    ap.add_argument("--only-device-scores", action="store_true", help="(e) alone: for a rocprofv3 kernel trace")
    ap.add_argument("--inst-out", default=os.path.join(ROOT, "profiles", "score_inst_line.json"),
                    help="file that receives the JSON line of (e) and (f) ('' : none)")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "score_map_line.json"), help="file that receives the JSON line ('' : none)")
    args = ap.parse_args()
    import torch
    import run_merge
    from autoinst_amd import _ffi, labels_api, ncuts_api
    ctx = ncuts_api.default_context()
    lib = _ffi.load()
    rng = np.random.default_rng(0)
    pts, gt = run_merge.build_street(rng, 22.0 * (args.chunks - 1) + 25.0, args.step)
    host = run_merge.cut(rng, pts, gt, args.chunks)
    points = [torch.from_numpy(p).cuda() for p, _, _ in host]
    inst = [torch.from_numpy(i).cuda() for _, i, _ in host]
    _, g, src = labels_api.merge_map(points, inst, ctx=ctx)
    gt_map = torch.from_numpy(np.concatenate([h[2] for h in host])).cuda()[src].to(torch.int32).contiguous()
    preds = label_rows(torch, g, args.rows)
    k, n = int(preds.shape[0]), int(preds.shape[1])
    sync = torch.cuda.synchronize
    out = {}

    def one_call():
        out["a"] = labels_api.label_tables(preds, gt_map, threshold=args.threshold, min_points=args.min_points, return_labels=True, ctx=ctx)

    def composition():
        tabs, rem, sco = [], torch.empty_like(preds), torch.empty_like(preds)
        cap = 1 << 16
        pa, pb, cnt = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int64)
        total = C.c_int64(0)
        sync()
        for t in range(k):
            _ffi.check(lib.ai_label_pairs(ctx._h, C.c_void_p(preds[t].data_ptr()), C.c_void_p(gt_map.data_ptr()), n, _ffi.AI_MEM_DEVICE, cap,
                                          pa.ctypes.data, pb.ctypes.data, cnt.ctypes.data, C.byref(total)), "ai_label_pairs")
            assert total.value <= cap
            a, b, c = pa[:total.value].copy(), pb[:total.value].copy(), cnt[:total.value].copy()
            u, at = np.unique(a, return_inverse=True)
            m = np.bincount(at, weights=c, minlength=u.size)
            z = np.bincount(at[b == 0], weights=c[b == 0], minlength=u.size)
            removed, small = z > args.threshold * m, m < args.min_points
            tabs.append((a, b, c, removed[at], small[at]))
            lut = torch.zeros(int(u[-1]) - int(u[0]) + 1, dtype=torch.uint8)
            lut[torch.from_numpy((u - int(u[0])).astype(np.int64))] = torch.from_numpy((removed.astype(np.uint8) | (small.astype(np.uint8) << 1)))
            f = lut.cuda()[(preds[t] - int(u[0])).long()]
            rem[t] = torch.where((f & 1) != 0, 0, preds[t])
            sco[t] = torch.where(f != 0, 0, preds[t])
        out["b"] = (tabs, rem, sco)

    def timed(fn):
        sync()
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0

    def score_legs():
        """(e) against (f); with --only-device-scores (e) alone."""
        res = {}

        def leg(level):
            def run():
                res[level] = labels_api.score_sweep(preds, gt_map, args.min_points, remove=True, threshold=args.threshold,
                                                    instance_level=level, ctx=ctx)
            return run
        levels = ("device",) if args.only_device_scores else ("device", "host")
        times = {level: [] for level in levels}
        for level in levels:
            timed(leg(level))
        for _ in range(max(args.reps, 10) if len(levels) == 2 else args.reps):
            for level in levels:
                times[level].append(timed(leg(level)))
        td, tf = [], []
        for _ in range(max(args.reps, 10)):                                 # (e) in its two parts
            rows = []

            def call():
                rows[:] = labels_api._device_scores(preds, gt_map, args.threshold, args.min_points, True, ctx)
            td.append(timed(call))
            t0 = time.perf_counter()
            finished = [labels_api._score_from_hits(*row) for row in rows]
            tf.append(time.perf_counter() - t0)
        assert all(str(a) == str(b) for a, b in zip(finished, res["device"]))
        med = statistics.median
        # by the header's count, not measured: pass 1 synchronises once per table size a row needs, then the result (and the hit bytes)
        largest = max(int(t[0].size) for t in labels_api.label_tables(preds, gt_map, threshold=args.threshold, min_points=args.min_points, ctx=ctx))
        syncs = 2 + int(largest > 4096) + int(largest > 65536)
        inst = {"tool": "run_score", "legs": "scores", "chunks": args.chunks, "rows": k, "points": n, "threshold": args.threshold,
                "min_points": args.min_points, "device_ms": 1e3 * med(times["device"]),
                "device_spread_ms": 1e3 * (max(times["device"]) - min(times["device"])),
                "device_ms_all": [round(1e3 * t, 3) for t in times["device"]],
                "device_call_ms": 1e3 * med(td), "host_finish_ms": 1e3 * med(tf), "host_finish_share": med(tf) / med(times["device"]),
                "scored_labels_per_row": [s["n_pred"] for s in res["device"]], "ap_per_row": [round(s["ap"], 6) for s in res["device"]],
                "pairs_in_largest_row": largest, "host_synchronisations_device": syncs + 1, "host_synchronisations_host": syncs}
        if "host" in res:
            equal = all(str(a) == str(b) for a, b in zip(res["device"], res["host"]))      # str: NaN equals NaN
            assert equal, "(e) and (f) differ"
            inst.update({"host_ms": 1e3 * med(times["host"]), "host_spread_ms": 1e3 * (max(times["host"]) - min(times["host"])),
                         "host_ms_all": [round(1e3 * t, 3) for t in times["host"]], "equal": equal,
                         "host_over_device": med(times["host"]) / med(times["device"]),
                         "device_below_host": bool(med(times["device"]) < med(times["host"]))})
        print(json.dumps(inst), flush=True)
        if args.inst_out:
            with open(args.inst_out, "w") as f:
                f.write(json.dumps(inst) + "\n")
    if args.only_scores or args.only_device_scores:
        score_legs()
        return
    timed(one_call)
    gbps = C.c_double(0.0)
    _ffi.check(lib.ai_bench_copy(ctx._h, 1 << 28, 10, C.byref(gbps)), "ai_bench_copy")
    bytes_min = (k + 1) * 4 * n + 4 * k * n
    line = {"tool": "run_score", "chunks": args.chunks, "rows": k, "points": n, "threshold": args.threshold, "min_points": args.min_points,
            "bytes_min": bytes_min, "bytes_moved": bytes_min + 4 * k * n, "copy_gbps": gbps.value,
            "bytes_min_ms": bytes_min / (gbps.value * 1e9) * 1e3}
    if args.only_tables:
        ta = [timed(one_call) for _ in range(args.reps)]
    else:
        timed(composition)
        ta, tb = [], []
        for _ in range(max(args.reps, 10)):
            ta.append(timed(one_call))
            tb.append(timed(composition))
        (at, ar, asc), (bt, br, bsc) = out["a"], out["b"]
        equal = bool(torch.equal(ar, br) and torch.equal(asc, bsc)) and all(
            x.tobytes() == y.tobytes() for ra, rb in zip(at, bt) for x, y in zip(ra, rb))
        assert equal, "(a) and (b) differ"
        sb = max(tb) - min(tb)
        line.update({"composition_ms": 1e3 * statistics.median(tb), "composition_spread_ms": 1e3 * sb,
                     "composition_ms_all": [round(1e3 * t, 3) for t in tb], "equal_to_composition": equal,
                     "composition_over_label_tables": statistics.median(tb) / statistics.median(ta),
                     "within_speed_bar": bool(statistics.median(ta) <= statistics.median(tb) + sb)})
    tabs = out["a"][0]
    line.update({"label_tables_ms": 1e3 * statistics.median(ta), "label_tables_spread_ms": 1e3 * (max(ta) - min(ta)),
                 "label_tables_ms_all": [round(1e3 * t, 3) for t in ta],
                 "pairs_per_row": [int(t[0].size) for t in tabs], "labels_removed_per_row": [int(np.unique(t[0][t[3]]).size) for t in tabs],
                 "labels_small_per_row": [int(np.unique(t[0][t[4]]).size) for t in tabs],
                 "ground_pair_share": float(max(int(t[2].max()) for t in tabs) / n)})
    th = []
    for _ in range(3):
        t0 = time.perf_counter()
        scores = labels_api._sweep_scores(tabs, args.min_points, True)
        th.append(time.perf_counter() - t0)
    line.update({"host_arithmetic_ms": 1e3 * statistics.median(th), "ap_per_row": [round(s["ap"], 6) for s in scores]})
    if not args.only_tables and not args.no_restated:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import score_ref
        p0, g0 = preds[0].cpu().numpy(), gt_map.cpu().numpy()
        t0 = time.perf_counter()
        ref = score_ref.remove_semantics(g0, p0, args.threshold)
        line["numpy_one_row_one_core_ms"] = 1e3 * (time.perf_counter() - t0)
        line["equal_to_numpy"] = bool(np.array_equal(ref, out["a"][1][0].cpu().numpy()))
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")
    if not args.only_tables:
        score_legs()


if __name__ == "__main__":
    main()
