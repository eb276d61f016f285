"""The aggregated raw clouds of a synthetic street from its scans, on the device (one JSON line).

synth.labelled_scans(--scans 1000, --points 120000): ~120 M float32 points in their sensor frames with label words, ground masks
and poses.  Timed, each the median of --reps calls after one warm-up call (wall clock around calls that end in a device
synchronise):
  resident_s   -- (a) prep_api.aggregate_scans from resident tensors (points, words, flags on the GPU; outputs stay there);
  numpy_s      -- (b) the same call from NumPy lists (concatenation, upload, the call, download);
  restated_s   -- (c) the NumPy restatement tests/aggregate_ref.py on one core of the same host.  It stands in for the
                  reference's loop (aggregate_pointcloud.py:99-186), which cannot run here for lack of open3d; that loop does
                  the same array work per scan plus open3d conversions and a growing map += pcd;
  copy_bound_s -- (d) the bytes the call must move (17 per input point read twice -- classify, then classify again and write --
                  and 24 + 12 per kept point written, no source positions in this call) over ai_bench_copy's rate on the same box; `copy_fraction` =
                  copy_bound_s / resident_s.
Then prep_api.downsample_map on the resident result (downsample_s).  The device result is compared with the restatement
(equality) before anything is timed, on the first --check-scans scans.

    python tools/run_aggregate.py [--scans 1000] [--points 120000] [--reps 5] [--no-restated] [--out profiles/aggregate_street_line.json]
"""
from __future__ import annotations

import argparse
import ctypes as C
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=1000)
    ap.add_argument("--points", type=int, default=120_000)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--check-scans", type=int, default=20)
    ap.add_argument("--no-restated", action="store_true")
    ap.add_argument("--no-numpy", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    os.environ.setdefault("OMP_NUM_THREADS", "1")   # (c) is a one-core figure
    import numpy as np
    import torch
    torch.cuda.init()
    import aggregate_ref
    from autoinst_amd import _ffi, prep_api, synth
    from autoinst_amd.ncuts_api import Context

    t0 = time.perf_counter()
    m = synth.labelled_scans(a.scans, a.points, seed=a.seed, spacing=0.7)
    t_synth = time.perf_counter() - t0
    print(f"[run_aggregate] {a.scans} scans made in {t_synth:.1f} s", file=sys.stderr, flush=True)
    filt = dict(moving_index=251, range_min=3.0, range_max=35.0)
    off = np.cumsum([0] + [s.shape[0] for s in m["scans"]]).astype(np.int64)
    M = int(off[-1])
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    xyz_d = torch.as_tensor(np.concatenate(m["scans"]), device=dev)
    words_d = torch.as_tensor(np.concatenate(m["labels"]).view(np.int32), device=dev).view(torch.uint32) \
        if hasattr(torch, "uint32") else torch.as_tensor(np.concatenate(m["labels"]).astype(np.int64), device=dev)
    ground_d = torch.as_tensor(np.concatenate(m["ground"]), device=dev)

    def resident():
        return prep_api.aggregate_scans(xyz_d, m["poses"], labels=words_d, ground=ground_d, scan_offsets=off, ctx=ctx, **filt)

    def from_numpy():
        return prep_api.aggregate_scans(m["scans"], m["poses"], labels=m["labels"], ground=m["ground"], ctx=ctx, **filt)

    def restated():
        return aggregate_ref.aggregate(m["scans"], m["poses"], m["labels"], m["ground"], **filt)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    def note(msg):
        print(f"[run_aggregate] {msg}", file=sys.stderr, flush=True)

    def median_of(fn):
        note(f"timing {fn.__name__}")
        timed(fn)   # warm-up: code objects, workspace, page faults of fresh host arrays
        ts = [timed(fn)[0] for _ in range(a.reps)]
        return statistics.median(ts), ts

    # the result is right before it is timed
    k = min(a.check_scans, a.scans)
    sub = dict(scans=m["scans"][:k], poses=m["poses"][:k], labels=m["labels"][:k], ground=m["ground"][:k], **filt)
    exp = aggregate_ref.aggregate(**sub)
    g, ng, lab = prep_api.aggregate_scans(xyz_d[:off[k]], m["poses"][:k], labels=words_d[:off[k]], ground=ground_d[:off[k]],
                                          scan_offsets=off[:k + 1], ctx=ctx, **filt)
    same = (g.cpu().numpy().tobytes() == exp["xyz_ground"].tobytes() and ng.cpu().numpy().tobytes() == exp["xyz_nonground"].tobytes()
            and all(np.array_equal(lab[key].cpu().numpy().astype(np.uint32), exp[key]) for key in lab))
    if not same:
        raise SystemExit("the device result differs from the restatement")
    del g, ng, lab, exp

    _, (g, ng, lab) = timed(resident)
    n_g, n_ng = int(g.shape[0]), int(ng.shape[0])
    res = {
        "what": "scans of a street -> aggregated ground / non-ground clouds + decoded labels (moving-object and range filter on)",
        "scans": a.scans, "points": M, "kept_ground": n_g, "kept_nonground": n_ng, "synth_s": t_synth,
        "equals_restatement_on_first_scans": k,
    }
    t_ds, _ = timed(lambda: prep_api.downsample_map(ng, g, lab, ctx=ctx))
    ds = [timed(lambda: prep_api.downsample_map(ng, g, lab, ctx=ctx))[0] for _ in range(a.reps)]
    res["downsample_s"], res["downsample_s_all"] = statistics.median(ds), ds
    del g, ng, lab
    res["resident_s"], res["resident_s_all"] = median_of(resident)
    res["workspace"] = ctx.mem_info()
    if not a.no_numpy:
        res["numpy_s"], res["numpy_s_all"] = median_of(from_numpy)
    if not a.no_restated:
        res["restated_s"], res["restated_s_all"] = median_of(restated)
        res["restated_over_resident"] = res["restated_s"] / res["resident_s"]
    gbps = C.c_double(0.0)
    _ffi.check(_ffi.load().ai_bench_copy(ctx._h, 1 << 30, 10, C.byref(gbps)), "ai_bench_copy")
    moved = 2 * 17 * M + (24 + 3 * 4) * (n_g + n_ng)      # no source output in this call: 36 bytes per kept point
    res["copy_gbps"], res["bytes_moved"] = gbps.value, moved
    res["copy_bound_s"] = moved / (gbps.value * 1e9)
    res["copy_fraction"] = res["copy_bound_s"] / res["resident_s"]
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
