"""One seeded RANSAC ground plane per scan of a synthetic street, on the device (one JSON line).

synth.labelled_scans(--scans 1000, --points 120000): ~120 M float32 points in their sensor frames with label words -- the street of
tools/run_aggregate.py.  Every scan gets --hypotheses 2000 planes, each scored on all of its kept points (rules G1-G7,
DESIGN.md section 18).  Timed, each the median of --reps calls after one warm-up call (wall clock around calls that end in a device
synchronise):
  resident_s    -- (a) prep_api.ground_planes from resident tensors (points and words on the GPU; the outputs stay there);
  chained_s     -- (b) prep_api.aggregate_scans(ground="ransac") from the same tensors: (a) and the aggregation, nothing crossing
                   to the host in between;
  restated_s    -- (c) the NumPy restatement tests/ground_ref.py on one core of the same host for the first --restated-scans scans
                   ONLY, and `restated_s_per_scan` x scans as the extrapolation to the map (stated as such).  It stands in for
                   open3d's segment_plane loop, which cannot run here for lack of open3d;
  fp64_bound_s  -- (d) the float64 vector instructions of G4 alone -- 3 multiplications, 3 additions and 1 comparison per (kept or
                   staged point, hypothesis), counted over the INPUT points a scoring block stages -- at the chip's float64 vector
                   rate from the data sheet (78.6 TFLOPS = 39.3 T instructions-lanes per second, a fused multiply-add counting
                   two; G4 may not fuse).  Not measured: it is arithmetic.  `fp64_fraction` = fp64_bound_s / resident_s.
The device result is compared with the restatement (equality of every output) on the first --check-scans scans before anything is
timed.

    python tools/run_ground.py [--scans 1000] [--points 120000] [--hypotheses 2000] [--reps 5] [--out profiles/ground_street_line.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

FP64_VECTOR_LANE_OPS_PER_S = 78.6e12 / 2.0    # data sheet: 78.6 TFLOPS of vector float64 with an FMA counted as two
G4_FP64_INSTRUCTIONS = 7                      # 3 v_mul_f64, 3 v_add_f64, 1 v_cmp_lt_f64 per point and hypothesis


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1000)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--hypotheses", type=int, default=2000)
    ap.add_argument("--threshold", type=float, default=0.4)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-scans", type=int, default=2)
    ap.add_argument("--restated-scans", type=int, default=2)
    ap.add_argument("--no-chained", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    os.environ.setdefault("OMP_NUM_THREADS", "1")   # (c) is a one-core figure
    import numpy as np
    import torch
    torch.cuda.init()
    import ground_ref
    from autoinst_amd import prep_api, synth
    from autoinst_amd.ncuts_api import Context

    def note(msg):
        print(f"[run_ground] {msg}", file=sys.stderr, flush=True)

    t0 = time.perf_counter()
    m = synth.labelled_scans(a.scans, a.points, seed=a.seed, spacing=0.7)
    t_synth = time.perf_counter() - t0
    note(f"{a.scans} scans made in {t_synth:.1f} s")
    filt = dict(moving_index=251, range_min=3.0, range_max=35.0)
    opts = dict(distance_threshold=a.threshold, num_iterations=a.hypotheses, seed=a.seed)
    off = np.cumsum([0] + [s.shape[0] for s in m["scans"]]).astype(np.int64)
    M = int(off[-1])
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    xyz_d = torch.as_tensor(np.concatenate(m["scans"]), device=dev)
    words_d = torch.as_tensor(np.concatenate(m["labels"]).view(np.int32), device=dev).view(torch.uint32) \
        if hasattr(torch, "uint32") else torch.as_tensor(np.concatenate(m["labels"]).astype(np.int64), device=dev)

    def resident():
        return prep_api.ground_planes(xyz_d, labels=words_d, scan_offsets=off, ctx=ctx, **filt, **opts)

    def chained():
        return prep_api.aggregate_scans(xyz_d, m["poses"], labels=words_d, ground="ransac", ground_options=opts, scan_offsets=off,
                                        ctx=ctx, **filt)

    def restated():
        k = min(a.restated_scans, a.scans)
        return ground_ref.ground_planes(m["scans"][:k], m["labels"][:k], **filt, **opts)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    def median_of(fn, reps):
        note(f"timing {fn.__name__}")
        timed(fn)   # warm-up: code objects, workspace
        ts = [timed(fn)[0] for _ in range(reps)]
        return statistics.median(ts), ts

    # the result is right before it is timed
    k = min(a.check_scans, a.scans)
    exp = ground_ref.ground_planes(m["scans"][:k], m["labels"][:k], **filt, **opts)
    got = prep_api.ground_planes(xyz_d[:off[k]], labels=words_d[:off[k]], scan_offsets=off[:k + 1], return_counts=True, ctx=ctx,
                                 **filt, **opts)
    names = ("flags", "planes", "best_hyp", "best_count", "hyp_count")
    if not all(g.cpu().numpy().tobytes() == exp[n].tobytes() for g, n in zip(got, names)):
        raise SystemExit("the device result differs from the restatement")
    del got, exp

    _, (flags, planes, best_hyp, best_count) = timed(resident)
    # the full-size call against itself: a scan's flags sum to its count, and the last scan segmented alone with its own key
    # (its ranks then come from a small scan of the kept flags, not from the map's) has the same plane and flags
    sums = torch.zeros(a.scans, dtype=torch.int64, device=dev).index_add_(
        0, torch.repeat_interleave(torch.arange(a.scans, device=dev), torch.as_tensor(np.diff(off), device=dev)), flags.long())
    last = a.scans - 1
    alone = prep_api.ground_planes(xyz_d[off[last]:], labels=words_d[off[last]:], scan_offsets=off[last:] - off[last], scan_base=last,
                                   ctx=ctx, **filt, **{k: v for k, v in opts.items()})
    if not (torch.equal(sums, best_count.long()) and torch.equal(alone[0], flags[off[last]:]) and torch.equal(alone[1][0], planes[last])):
        raise SystemExit("the full-size result is not consistent with itself")
    del sums, alone
    road = torch.as_tensor(np.concatenate(m["ground"]), device=dev)
    res = {
        "what": "scans of a street -> one seeded RANSAC ground plane per scan and the per-point ground flags "
                "(moving-object and range filter on)",
        "scans": a.scans, "points": M, "hypotheses": a.hypotheses, "distance_threshold": a.threshold, "synth_s": t_synth,
        "equals_restatement_on_first_scans": k,
        "scans_without_plane": int((best_hyp < 0).sum()), "flagged": int(flags.sum()),
        "road_points_flagged_fraction": float(flags[road].float().mean()),
        "max_one_minus_abs_c": float((1.0 - planes[:, 2].abs()).max()),
    }
    del flags, planes, best_hyp, best_count, road
    res["resident_s"], res["resident_s_all"] = median_of(resident, a.reps)
    res["workspace"] = ctx.mem_info()
    if not a.no_chained:
        res["chained_s"], res["chained_s_all"] = median_of(chained, a.reps)
    kr = min(a.restated_scans, a.scans)
    t_r, ts_r = median_of(restated, 1)
    res["restated_scans"], res["restated_s"] = kr, t_r
    res["restated_s_per_scan"] = t_r / kr
    res["restated_s_extrapolated_to_all_scans"] = t_r / kr * a.scans
    res["restated_extrapolated_over_resident"] = res["restated_s_extrapolated_to_all_scans"] / res["resident_s"]
    staged = M    # every input point is staged once per block of 256 hypotheses; lanes past the last hypothesis compute too
    lanes = -(-a.hypotheses // 256) * 256
    res["fp64_rate_source"] = "data sheet, 78.6 TFLOPS vector float64 (FMA = 2); not measured"
    res["fp64_lane_instructions"] = G4_FP64_INSTRUCTIONS * staged * lanes
    res["fp64_bound_s"] = res["fp64_lane_instructions"] / FP64_VECTOR_LANE_OPS_PER_S
    res["fp64_fraction"] = res["fp64_bound_s"] / res["resident_s"]
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
