#!/usr/bin/env python3
"""DBSCAN of a street's non-ground minor points on the device vs scikit-learn on the host (one JSON line).

The map is `synth.street_map(--length)` (0.05 m surfaces: two facades, objects, outliers; 1600 m gives 72 chunk boxes and
~12.6 M non-ground points), eps = 0.7, min_samples = 20, from resident device tensors, warm, median of --reps, each call
ending in a device synchronise:
  (a)  one `cluster_api.dbscan` call on the whole map as one cloud;
  (a') the same points as the street's chunk crops (`prep_api.box_select` of the 25 m boxes along the trajectory, which
       overlap by 3 m), all crops as clouds of ONE call;
  (b)  `sklearn.cluster.DBSCAN` on this box's host, on the first --sklearn-length metres of the street only: scikit-learn keeps
       every neighbourhood in memory (some 600 neighbours of 8 bytes per point at this density), which the whole map does not
       allow.  The device clusters the same stretch on its own and the number of points whose label differs is REPORTED, not
       asserted: at this size nobody has checked that no pair lies within rounding of eps.  `same_host` is false when
       scikit-learn does not import here (the leg is then left out);
  (d)  the number of D1 distance tests of the three searches, from the cell occupancies (arithmetic on the grid the library
       builds, not a measurement): every point of search 2 (core points) and search 3 (the others) tests all points of its 27
       cells; search 1 stops at min_samples neighbours, so it lies between min_samples tests and the same full count.  The tests per
       second that (a) implies are given for both ends.
Kernel times come from a separate `rocprofv3 --kernel-trace --stats -- python tools/run_dbscan.py --only-device --reps 1 --out ""`
run (profiles/dbscan_street_kernels.txt).
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


def d1_tests(points, core, eps):
    """(candidates summed over core points, over the other points): a point's candidates are the points of its 27 cells."""
    import torch
    cell = eps * (1.0 + 1e-6)
    mn = points.min(dim=0).values
    c = torch.floor((points - mn) * (1.0 / cell)).long()
    nx, ny, nz = (int(v) + 1 for v in c.max(dim=0).values)
    assert nx * ny * nz <= 1 << 27, "the library would grow the cell: count on its grid instead"
    key = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    occ = torch.bincount(key, minlength=nx * ny * nz).reshape(1, 1, nz, ny, nx).double()
    ring = torch.nn.functional.conv3d(occ, torch.ones(1, 1, 3, 3, 3, dtype=torch.float64, device=occ.device), padding=1).reshape(-1)
    cand = ring[key]
    return int(cand[core].sum().item()), int(cand[~core].sum().item())


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=float, default=1600.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--eps", type=float, default=0.7)
    ap.add_argument("--min-samples", type=int, default=20)
    ap.add_argument("--sklearn-length", type=float, default=60.0, help="metres of street given to scikit-learn (0: skip the leg)")
    ap.add_argument("--only-device", action="store_true", help="(a) and (a') alone: for a rocprofv3 kernel trace")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "dbscan_street_line.json"), help="'' : no file")
    a = ap.parse_args()

    import torch
    torch.cuda.init()
    from autoinst_amd import cluster_api, prep_api, synth
    from autoinst_amd.config import CHUNK_SIZE
    from autoinst_amd.ncuts_api import Context

    m = synth.street_map(a.length, seed=a.seed)
    host = m["nonground"]
    dev = torch.device("cuda", 0)
    ctx = Context(0)
    pts = torch.as_tensor(host, device=dev)
    centres, _ = prep_api.chunk_centres(m["T_pcd"], m["positions"], m["first_position"], m["indices"])
    half = 0.5 * np.asarray(CHUNK_SIZE, dtype=np.float64)
    crops = [pts[i] for i in prep_api.box_select(pts, [np.concatenate([c - half, c + half]) for c in centres], ctx=ctx)]
    eps, ms = a.eps, a.min_samples

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def whole():
        return cluster_api.dbscan(pts, eps, ms, return_counts=True, ctx=ctx)

    def chunked():
        return cluster_api.dbscan(crops, eps, ms, ctx=ctx)

    timed(whole)
    timed(chunked)   # warm-up: code objects, workspace
    ta, tc = [], []
    for _ in range(a.reps):   # alternating
        ta.append(timed(whole)[0])
        tc.append(timed(chunked)[0])
    labels, n_clusters, counts = whole()
    crop_labels, crop_found = chunked()
    again = whole()[0]
    core = counts >= ms
    out = {"metric": "dbscan_street", "length_m": a.length, "eps": eps, "min_samples": ms, "points": int(pts.shape[0]),
           "whole_ms": round(statistics.median(ta), 3), "whole_ms_all": [round(x, 3) for x in ta],
           "whole_clusters": int(n_clusters), "whole_noise": int((labels < 0).sum().item()), "whole_core": int(core.sum().item()),
           "whole_repeat_equal": bool(torch.equal(labels, again)),
           "chunks": len(crops), "chunk_points": int(sum(int(c.shape[0]) for c in crops)),
           "chunks_ms": round(statistics.median(tc), 3), "chunks_ms_all": [round(x, 3) for x in tc],
           "chunks_clusters_min_max": [int(min(crop_found)), int(max(crop_found))],
           "chunks_noise": int(sum(int((x < 0).sum().item()) for x in crop_labels))}
    t23_core, t23_other = d1_tests(pts, core, eps)
    lower, upper = t23_core + t23_other + ms * int(pts.shape[0]), 2 * (t23_core + t23_other)
    out.update({"d1_tests_union_search": t23_core, "d1_tests_border_search": t23_other,
                "d1_tests_count_search_bounds": [ms * int(pts.shape[0]), t23_core + t23_other],
                "d1_tests_note": "arithmetic from the cell occupancies, not measured",
                "d1_tests_per_s_bounds": [round(lower / (out["whole_ms"] * 1e-3), 1), round(upper / (out["whole_ms"] * 1e-3), 1)]})
    if not a.only_device and a.sklearn_length > 0:
        sel = np.flatnonzero(host[:, 0] < a.sklearn_length)
        sub = np.ascontiguousarray(host[sel])
        sub_labels = cluster_api.dbscan(torch.as_tensor(sub, device=dev), eps, ms, ctx=ctx)[0].cpu().numpy()
        out.update({"sklearn_length_m": a.sklearn_length, "sklearn_points": int(sub.shape[0])})
        try:
            import sklearn
            from sklearn.cluster import DBSCAN
            t = time.perf_counter()
            sk = DBSCAN(eps=eps, min_samples=ms).fit(sub).labels_
            sk_s = time.perf_counter() - t
            out.update({"same_host": True, "sklearn_s": round(sk_s, 3), "sklearn_version": sklearn.__version__,
                        "sklearn_differing_labels": int((sk != sub_labels).sum()),
                        "sklearn_us_per_point": round(sk_s * 1e6 / max(1, sub.shape[0]), 3),
                        "device_us_per_point_whole": round(out["whole_ms"] * 1e3 / int(pts.shape[0]), 5)})
        except ImportError:
            out["same_host"] = False
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
