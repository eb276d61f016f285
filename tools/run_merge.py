#!/usr/bin/env python3
"""The step that turns the chunks into the map, for a whole map: one `labels_api.merge_map` call against the colour-identified
`labels_api.merge_chunks_unite_instances2` loop on the same data.

The map is synthetic and has TRUE overlaps: one cloud of a street along x is built once and cut into `--chunks` boxes of 25 m
every 22 m, so the points of an overlap are bit-identical in both neighbours.  The cloud: a ground plane 16 m wide on a jittered
`--step` grid (id 0), the two 8 m facades in 11 m segments and a box-shaped object of 2 x 1.5 x 1.5 m every 6 m on either side
of the road, each segment and each object one instance.  Every chunk numbers the objects it sees 1 .. k in its own permuted
order; the global object id of every point is kept as the ground truth.

Timed warm, from resident device tensors, each leg ending in a device synchronise, the median of `--reps`:
  (a) one merge_map call;
  (b) the colour path on the same data, `--colour-reps` times (it is slow): ids to colours on the host -- colour (g, 0, 0) for the
      provisional global id g, under which the lexicographic colour order is the id order (rule M11) -- then
      merge_chunks_unite_instances2;
  (c) tests/merge_map_ref.py (NumPy) on one core, once (`--no-restated` skips it).
(a) and (b) must agree: the points bit for bit, and the colours are those of (a)'s ids, which is more than the same partition.
The ground truth rides along through `source`: cat(gt)[source] must be constant on every merged instance that (b) agrees on.
Also printed: the bytes (a) cannot avoid (points and ids read once, the kept points, ids and sources written once) and the time
they take at the box's copy rate (`ai_bench_copy`).  One JSON line, printed and written to `--out` (default
profiles/merge_street_line.json).  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/run_merge.py --only-map --reps 1 --out ""` run (profiles/merge_street_kernels.txt).
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


def _grid(rng, u0, u1, v0, v1, step):
    uu, vv = np.meshgrid(np.arange(u0, u1, step), np.arange(v0, v1, step), indexing="ij")
    return uu.ravel() + rng.random(uu.size) * step, vv.ravel() + rng.random(vv.size) * step


def build_street(rng, length, step):
    """(points, global object id): ground 0, facade segments and boxes 1 .."""
    pts, ids = [], []
    gx, gy = _grid(rng, 0.0, length, -8.0, 8.0, step)
    pts.append(np.stack([gx, gy, 0.02 * np.sin(gx * 0.3) + 0.01 * rng.standard_normal(gx.size)], 1))
    ids.append(np.zeros(gx.size, dtype=np.int64))
    nxt = 1
    for side in (-8.0, 8.0):
        for x0 in np.arange(0.0, length, 11.0):
            fx, fz = _grid(rng, x0, min(x0 + 10.5, length), 0.2, 8.0, step)
            pts.append(np.stack([fx, side + 0.01 * rng.standard_normal(fx.size), fz], 1))
            ids.append(np.full(fx.size, nxt, dtype=np.int64))
            nxt += 1
        for x0 in np.arange(2.0, length - 2.0, 6.0):
            y0 = side * 0.7
            faces = []
            for (a0, a1, b0, b1, fixed, axis) in ((x0, x0 + 2.0, 0.1, 1.6, y0 - 0.75, 1), (x0, x0 + 2.0, 0.1, 1.6, y0 + 0.75, 1),
                                                  (y0 - 0.75, y0 + 0.75, 0.1, 1.6, x0, 0), (y0 - 0.75, y0 + 0.75, 0.1, 1.6, x0 + 2.0, 0),
                                                  (x0, x0 + 2.0, y0 - 0.75, y0 + 0.75, 1.6, 2)):
                u, v = _grid(rng, a0, a1, b0, b1, step / 2.0)
                f = np.full(u.size, fixed)
                faces.append(np.stack({0: [f, u, v], 1: [u, f, v], 2: [u, v, f]}[axis], 1))
            box = np.concatenate(faces)
            pts.append(box)
            ids.append(np.full(box.shape[0], nxt, dtype=np.int64))
            nxt += 1
    pts, ids = np.concatenate(pts), np.concatenate(ids)
    perm = rng.permutation(pts.shape[0])
    return np.ascontiguousarray(pts[perm]), ids[perm]


def cut(rng, pts, gt, n_chunks):
    """Boxes of 25 m every 22 m; per chunk the points, the chunk-local ids (1 .. k, permuted; ground 0) and the ground truth."""
    out = []
    for c in range(n_chunks):
        sel = (pts[:, 0] >= 22.0 * c) & (pts[:, 0] < 22.0 * c + 25.0)
        p, g = pts[sel], gt[sel]
        objs = np.unique(g[g > 0])
        local = np.zeros(int(gt.max()) + 1, dtype=np.int32)
        local[objs] = rng.permutation(objs.size).astype(np.int32) + 1
        out.append((np.ascontiguousarray(p), local[g], g))
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=72)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--colour-reps", type=int, default=1, help="runs of (b), the colour-identified loop (slow)")
    ap.add_argument("--step", type=float, default=0.2, help="grid step of ground and facades in metres (objects: half of it)")
    ap.add_argument("--only-map", action="store_true", help="(a) alone: for a rocprofv3 kernel trace")
    ap.add_argument("--no-restated", action="store_true", help="skip (c), the NumPy restatement on one core")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "merge_street_line.json"),
                    help="file that receives the JSON line ('' : none)")
    args = ap.parse_args()
    import torch
    from autoinst_amd import _ffi, labels_api, ncuts_api
    ctx = ncuts_api.default_context()
    rng = np.random.default_rng(0)
    pts, gt = build_street(rng, 22.0 * (args.chunks - 1) + 25.0, args.step)
    host = cut(rng, pts, gt, args.chunks)
    points = [torch.from_numpy(p).cuda() for p, _, _ in host]
    inst = [torch.from_numpy(i).cuda() for _, i, _ in host]
    gt_all = torch.from_numpy(np.concatenate([g for _, _, g in host])).cuda()
    sync = torch.cuda.synchronize
    out = {}

    def whole_map():
        out["a"] = labels_api.merge_map(points, inst, return_stats=True, ctx=ctx)

    def colour_loop():
        goff = np.concatenate([[0], np.cumsum([int(i.max()) if i.numel() else 0 for i in inst])])
        chunks = []
        for c, (p, i) in enumerate(zip(points, inst)):
            i = i.cpu().numpy().astype(np.int64)
            col = np.zeros((i.size, 3))
            col[:, 0] = np.where(i > 0, goff[c] + i, 0)
            chunks.append((p.cpu().numpy(), col))
        out["b"] = labels_api.merge_chunks_unite_instances2(chunks, ctx=ctx)

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0
    timed(whole_map)     # warm: the context's workspace, the code objects, torch's allocator
    ta = [timed(whole_map) for _ in range(args.reps)]
    p, g, src, stats = out["a"]
    m = int(sum(x.shape[0] for x in points))
    gbps = C.c_double(0.0)
    _ffi.check(_ffi.load().ai_bench_copy(ctx._h, 1 << 28, 10, C.byref(gbps)), "ai_bench_copy")
    bytes_min = 28 * m + 36 * int(p.shape[0])
    gt_merged = gt_all[src]
    line = {"tool": "run_merge", "chunks": args.chunks, "step": args.step, "points_in": m, "points_out": int(p.shape[0]),
            "local_ids": int(sum(int(i.max()) for i in inst)), "objects": int(gt.max()), "instances_out": int(torch.unique(g[g > 0]).numel()),
            "cropped_points_per_step": float(stats[1:, 0].mean()), "map_instances_per_step": float(stats[1:, 1].mean()),
            "relabelled": int(stats[:, 3].sum()),
            "merge_map_ms": 1e3 * statistics.median(ta), "merge_map_ms_all": [round(1e3 * t, 3) for t in ta],
            "bytes_min": bytes_min, "copy_gbps": gbps.value, "bytes_min_ms": bytes_min / (gbps.value * 1e9) * 1e3,
            # every merged instance is one object of the ground truth, carried along by `source` alone
            "instances_pure_in_gt": bool(torch.unique(torch.stack([g[g > 0].long(), gt_merged[g > 0]]), dim=1).shape[1]
                                         == torch.unique(g[g > 0]).numel())}
    if not args.only_map:
        tb = [timed(colour_loop) for _ in range(args.colour_reps)]
        bp, bc = out["b"]
        assert bp.tobytes() == p.cpu().numpy().tobytes(), "(a) and (b) differ in the points"
        assert not bc[:, 1:].any() and np.array_equal(bc[:, 0], g.cpu().numpy().astype(np.float64)), "(a) and (b) differ in the instances"
        line.update({"colour_loop_ms": 1e3 * statistics.median(tb), "colour_loop_ms_all": [round(1e3 * t, 3) for t in tb],
                     "colour_loop_over_merge_map": statistics.median(tb) / statistics.median(ta), "equal_to_colour_loop": True})
        if not args.no_restated:
            sys.path.insert(0, os.path.join(ROOT, "tests"))
            import merge_map_ref
            t0 = time.perf_counter()
            ref = merge_map_ref.merge_map([h[0] for h in host], [h[1] for h in host])
            line["numpy_one_core_ms"] = 1e3 * (time.perf_counter() - t0)
            line["numpy_over_merge_map"] = line["numpy_one_core_ms"] / line["merge_map_ms"]
            line["equal_to_numpy"] = bool(ref["points"].tobytes() == bp.tobytes() and np.array_equal(ref["inst"], g.cpu().numpy())
                                          and np.array_equal(ref["src"], src.cpu().numpy()))
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
