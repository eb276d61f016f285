#!/usr/bin/env python3
"""TARL scan features of a whole map: one `points_api.tarl_pool_map` call against the per-chunk composition.

The map is synthetic: a street along x (an undulating ground 16 m wide between two 8 m facades).  `--scans` sampled scans, each
`--scan-points` surface points within `--range` m of its pose and given in the sensor frame (poses with yaw, pitch and roll), with
96-d float32 features; `--chunks` chunks 22 m apart (CHUNK_SIZE 25 m less OVERLAP 3 m) with major-voxel points on a 0.35 m
jittered grid of the same surface; each chunk's window is the reference's (10, 10) slice around the scan nearest to its centre.

Timed warm, median of `--reps`, each ending in a device synchronise:
  (a) tarl_pool_map from resident tensors;  (b) tarl_pool_map from NumPy inputs;
  (c) the per-chunk composition on the same inputs: one tarl_features_per_patch per chunk (fixed-order transform);
  and sharding.run_chunks on the same chunks with the pooled features.
One JSON line, printed and written to `--out` (default profiles/tarl_map_line.json).  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/run_tarl_map.py --only-resident --reps 1 --out ""` run
(profiles/tarl_map_kernels.txt).
"""
import argparse
import json
import os
import statistics
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def _rigid(yaw, pitch, roll, t):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    R = (np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]])
         @ np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]]))
    T = np.eye(4)
    T[:3, :3] = R
    T[:3, 3] = t
    return T


def _surface(rng, n, x0, x1):
    """n points of the street between x0 and x1: half on the ground, a quarter on each facade."""
    x = rng.uniform(x0, x1, n)
    kind = rng.integers(0, 4, n)
    y = np.where(kind < 2, rng.uniform(-8.0, 8.0, n), np.where(kind == 2, -8.0, 8.0))
    ground = 0.3 * np.sin(x / 7.0) + 0.1 * np.cos(y / 2.0)
    z = np.where(kind < 2, ground, rng.uniform(0.0, 8.0, n))
    return np.stack([x, y, z], 1) + rng.normal(0.0, 0.01, (n, 3))


def _major(rng, cx, step=0.35):
    """A chunk's major-voxel points: a jittered `step` grid of the ground and the facades inside the 25 m box around x = cx."""
    u = np.arange(cx - 12.4, cx + 12.4, step)
    gx, gy = np.meshgrid(u, np.arange(-8.0, 8.0, step), indexing="ij")
    ground = np.stack([gx.ravel(), gy.ravel(), 0.3 * np.sin(gx.ravel() / 7.0) + 0.1 * np.cos(gy.ravel() / 2.0)], 1)
    fx, fz = np.meshgrid(u, np.arange(0.0, 8.0, step), indexing="ij")
    walls = [np.stack([fx.ravel(), np.full(fx.size, s), fz.ravel()], 1) for s in (-8.0, 8.0)]
    p = np.concatenate([ground] + walls)
    return p + rng.uniform(-0.1, 0.1, p.shape)


def build_map(n_scans, scan_points, n_chunks, lidar_range, seed=0):
    rng = np.random.default_rng(seed)
    length = 22.0 * (n_chunks - 1)
    sx = np.linspace(-5.0, length + 5.0, n_scans)
    scans, feats, Ts = [], [], []
    for s in range(n_scans):
        T = _rigid(0.05 * np.sin(s / 9.0), 0.01 * np.cos(s / 5.0), 0.01 * np.sin(s / 7.0), (sx[s], rng.uniform(-1.0, 1.0), 1.7))
        w = _surface(rng, scan_points, sx[s] - lidar_range, sx[s] + lidar_range)
        Ti = np.linalg.inv(T)
        scans.append(w @ Ti[:3, :3].T + Ti[:3, 3])
        feats.append(rng.standard_normal((scan_points, 96), dtype=np.float32))
        Ts.append(T)
    centers = np.array([[22.0 * c, 0.0, 1.0] for c in range(n_chunks)])
    chunks = [_major(rng, c[0]) for c in centers]
    center_ids = [int(np.argmin(np.abs(sx - c[0]))) for c in centers]
    return {"scans": scans, "feats": feats, "T": np.array(Ts), "chunks": chunks, "centers": centers, "center_ids": center_ids}


class _Dataset:
    def __init__(self, m):
        self.m = m

    def get_tarl_features(self, i):
        return self.m["feats"][i]

    def get_point_cloud(self, i):
        return self.m["scans"][i]

    def get_pose(self, i):
        return self.m["T"][i]


class _Cloud:
    def __init__(self, points):
        self.points = points


def _median(fn, reps, sync):
    fn()          # warm: the context's workspace, the code objects
    sync()
    ts = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        sync()
        ts.append(time.perf_counter() - t0)
    return statistics.median(ts), ts


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--scans", type=int, default=240)
    ap.add_argument("--scan-points", type=int, default=30_000)
    ap.add_argument("--chunks", type=int, default=72)
    ap.add_argument("--range", type=float, default=25.0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--only-resident", action="store_true", help="(a) alone: for a rocprofv3 kernel trace")
    ap.add_argument("--out", default=os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "profiles",
                                                  "tarl_map_line.json"), help="file that receives the JSON line ('' : none)")
    args = ap.parse_args()
    import torch
    from autoinst_amd import camera_api, ncuts_api, points_api, sharding
    from autoinst_amd.config import ADJACENT_FRAMES_TARL, CHUNK_SIZE
    ctx = ncuts_api.default_context()
    m = build_map(args.scans, args.scan_points, args.chunks, args.range)
    ids = list(range(args.scans))
    wins = np.array([points_api.tarl_window(ids, c, ADJACENT_FRAMES_TARL) for c in m["center_ids"]])
    half = 0.5 * np.asarray(CHUNK_SIZE)
    boxes = np.concatenate([m["centers"] - half, m["centers"] + half], 1)
    sync = torch.cuda.synchronize
    d_scan = torch.from_numpy(np.concatenate(m["scans"])).cuda()
    d_feat = torch.from_numpy(np.concatenate(m["feats"])).cuda()
    d_q = torch.from_numpy(np.concatenate(m["chunks"])).cuda()
    soff = np.arange(args.scans + 1, dtype=np.int64) * args.scan_points
    qoff = np.concatenate([[0], np.cumsum([c.shape[0] for c in m["chunks"]])]).astype(np.int64)
    out = {}

    def resident():
        out["dev"] = points_api.tarl_pool_map(d_scan, d_feat, m["T"], d_q, boxes, wins, scan_offsets=soff, chunk_offsets=qoff,
                                              return_count=True, ctx=ctx)
    t_a, all_a = _median(resident, args.reps, sync)
    rows, cnt = out["dev"]
    line = {"tool": "run_tarl_map", "scans": args.scans, "scan_points": args.scan_points, "source_points": int(soff[-1]),
            "chunks": args.chunks, "query_points": int(qoff[-1]), "window": list(ADJACENT_FRAMES_TARL), "dim": 96,
            "members_per_query_mean": float(torch.cat(cnt).double().mean()), "queries_with_members": int((torch.cat(cnt) > 0).sum()),
            "pool_map_resident_ms": 1e3 * t_a, "pool_map_resident_ms_all": [round(1e3 * t, 3) for t in all_a]}
    if not args.only_resident:
        def host():
            out["host"] = points_api.tarl_pool_map(m["scans"], m["feats"], m["T"], m["chunks"], boxes, wins, ctx=ctx)
        t_b, all_b = _median(host, args.reps, sync)
        assert all(np.array_equal(h, d.cpu().numpy()) for h, d in zip(out["host"], rows))
        ds = _Dataset(m)

        def per_chunk():
            out["one"] = [points_api.tarl_features_per_patch(ds, _Cloud(m["chunks"][c]), np.eye(4), m["centers"][c],
                                                             list(range(*wins[c])), transform_pcd=camera_api.transform_points, ctx=ctx)
                          for c in range(args.chunks)]
        t_c, all_c = _median(per_chunk, args.reps, sync)
        worst = max(float(np.abs(a - b).max()) for a, b in zip(out["one"], out["host"]))
        chunks_dev = [d_q[qoff[c]:qoff[c + 1]] for c in range(args.chunks)]

        def cut():
            out["labels"] = sharding.run_chunks(list(zip(chunks_dev, rows)), alpha=1.0, theta=0.5, gamma=0.0, T=0.03)
        t_cut, all_cut = _median(cut, args.reps, sync)
        line.update({"pool_map_numpy_ms": 1e3 * t_b, "pool_map_numpy_ms_all": [round(1e3 * t, 3) for t in all_b],
                     "per_chunk_ms": 1e3 * t_c, "per_chunk_ms_all": [round(1e3 * t, 3) for t in all_c],
                     "per_chunk_over_resident": t_c / t_a, "per_chunk_over_numpy": t_c / t_b,
                     "max_abs_diff_vs_per_chunk": worst, "run_chunks_ms": 1e3 * t_cut,
                     "run_chunks_ms_all": [round(1e3 * t, 3) for t in all_cut], "run_chunks_over_resident": t_cut / t_a,
                     "groups_total": int(sum(int(np.asarray(l).max()) + 1 for l in out["labels"]))})
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
