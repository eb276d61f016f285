#!/usr/bin/env python3
"""The tail of ncuts_chunk for a whole map: one `points_api.finish_chunks` call against the per-chunk composition of the
single-cloud entries.

The map is synthetic: `--chunks` chunks of a street along x, 22 m apart (CHUNK_SIZE 25 m less OVERLAP 3 m), each with its own
25 m box of points: the fine cloud is a jittered 0.1 m grid of the two 8 m facades (~40 k points), the major cloud the same
surface on a 0.35 m grid (~3.3 k points, group id = index mod 50), the ground a jittered 0.1 m grid of a 16 m wide plane with
a kerb raised by 0.9 m beyond y = 6.5 (~40 k points); `--ground-outliers F` adds a fraction F of
points 2 - 12 m above it.  Those matter for the time: ai_statistical_inliers' grid rule, which each chunk keeps, takes its cell
from the bounding box's volume per point, so a few high points make the cells of a flat cloud coarse (0.56 m instead of 0.22 m
at F = 0.005, some 30 points per cell instead of 5) and the kNN search slow.

Timed from resident device tensors, warm, alternating (a), (b) in one process `--reps` times, each ending in a device synchronise:
  (a) one finish_chunks call for all chunks;
  (b) per chunk: ai_nn1_project and ai_statistical_inliers on the chunk's device buffers, then torch for the rest (label gather,
      z of the inliers, mean, compare, index, concatenate) -- what the library offered before ai_chunk_finish;
  (c) tests/finish_ref.py (NumPy / cKDTree) on one core, once (`--no-restated` skips it).
(a) and (b) are compared chunk by chunk (indices and labels equal, coordinates bit for bit).  One JSON line, printed and written
to `--out` (default profiles/finish_street_line.json).  Kernel times come from a separate
`rocprofv3 --kernel-trace --stats -- python tools/run_finish.py --only-batched --reps 1 --out ""` run
(profiles/finish_street_kernels.txt).
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


def build_chunk(rng, cx, ground_outliers=0.0):
    x0, x1 = cx - 12.4, cx + 12.4
    fine, major = [], []
    for side in (-8.0, 8.0):
        for step, dst in ((0.1, fine), (0.35, major)):
            fx, fz = _grid(rng, x0, x1, 0.0, 8.0, step)
            dst.append(np.stack([fx, side + 0.01 * rng.standard_normal(fx.size), fz], 1))
    gx, gy = _grid(rng, x0, x1, -8.0, 8.0, 0.1)
    gz = 0.02 * np.sin(gx * 0.3) + 0.01 * rng.standard_normal(gx.size) + np.where(gy > 6.5, 0.9, 0.0)
    ground = np.stack([gx, gy, gz], 1)
    n_out = int(ground.shape[0] * ground_outliers)
    out = np.stack([rng.uniform(x0, x1, n_out), rng.uniform(-12.0, 12.0, n_out), rng.uniform(2.0, 12.0, n_out)], 1)
    ground = np.concatenate([ground, out])
    return (np.concatenate(fine), np.concatenate(major), np.ascontiguousarray(ground[rng.permutation(ground.shape[0])]))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--chunks", type=int, default=72)
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--ground-outliers", type=float, default=0.0, help="fraction of ground points 2 - 12 m above the plane")
    ap.add_argument("--only-batched", action="store_true", help="(a) alone: for a rocprofv3 kernel trace")
    ap.add_argument("--no-restated", action="store_true", help="skip (c), the NumPy restatement on one core")
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "finish_street_line.json"),
                    help="file that receives the JSON line ('' : none)")
    args = ap.parse_args()
    import torch
    from autoinst_amd import _ffi, ncuts_api, points_api
    from autoinst_amd.config import MEAN_HEIGHT
    ctx = ncuts_api.default_context()
    lib = _ffi.load()
    rng = np.random.default_rng(0)
    host = [build_chunk(rng, 22.0 * c, args.ground_outliers) for c in range(args.chunks)]
    labels_h = [(np.arange(m.shape[0]) % 50).astype(np.int32) for _, m, _ in host]
    fine = [torch.from_numpy(f).cuda() for f, _, _ in host]
    major = [torch.from_numpy(m).cuda() for _, m, _ in host]
    ground = [torch.from_numpy(g).cuda() for _, _, g in host]
    labels = [torch.from_numpy(l).cuda() for l in labels_h]
    sync = torch.cuda.synchronize
    out = {}

    def batched():
        out["a"] = points_api.finish_chunks(fine, major, labels, ground, ctx=ctx)

    def per_chunk():
        res = []
        for f, m, lab, g in zip(fine, major, labels, ground):
            nf, ng = f.shape[0], g.shape[0]
            nn = torch.empty(nf, dtype=torch.int32, device=f.device)
            keep = torch.empty(ng, dtype=torch.int32, device=f.device)
            nk = C.c_int64(0)
            sync()   # torch's allocations and the previous chunk's torch work are done before the library's stream starts
            _ffi.check(lib.ai_nn1_project(ctx._h, C.c_void_p(f.data_ptr()), nf, C.c_void_p(m.data_ptr()), m.shape[0], _ffi.AI_MEM_DEVICE,
                                          C.c_void_p(nn.data_ptr()), None), "ai_nn1_project")
            _ffi.check(lib.ai_statistical_inliers(ctx._h, C.c_void_p(g.data_ptr()), ng, 20, 2.0, _ffi.AI_MEM_DEVICE,
                                                  C.c_void_p(keep.data_ptr()), C.byref(nk), None, None), "ai_statistical_inliers")
            inl = keep[:nk.value].long()
            fl = lab[nn.long()]
            z = g[inl, 2]
            kept = inl[z < (z.mean() + MEAN_HEIGHT)]
            res.append({"merged_points": torch.cat([f, g[kept]]), "fine_instance": fl, "ground_keep": kept,
                        "merged_instance": torch.cat([fl + 1, torch.zeros(kept.shape[0], dtype=torch.int32, device=f.device)])})
        out["b"] = res

    def timed(fn):
        t0 = time.perf_counter()
        fn()
        sync()
        return time.perf_counter() - t0
    timed(batched)     # warm: the context's workspace, the code objects, torch's allocator
    if args.only_batched:
        ta = [timed(batched) for _ in range(args.reps)]
        tb = []
    else:
        timed(per_chunk)
        ta, tb = [], []
        for _ in range(args.reps):
            ta.append(timed(batched))
            tb.append(timed(per_chunk))
    a = out["a"]
    line = {"tool": "run_finish", "chunks": args.chunks, "ground_outliers": args.ground_outliers, "fine_points": int(sum(f.shape[0] for f in fine)),
            "major_points": int(sum(m.shape[0] for m in major)), "ground_points": int(sum(g.shape[0] for g in ground)),
            "ground_kept": int(sum(d["ground_keep"].shape[0] for d in a)),
            "finish_chunks_ms": 1e3 * statistics.median(ta), "finish_chunks_ms_all": [round(1e3 * t, 3) for t in ta]}
    if tb:
        for c, (x, y) in enumerate(zip(a, out["b"])):
            for k in ("fine_instance", "ground_keep", "merged_instance"):
                assert torch.equal(x[k], y[k]), (c, k)
            assert x["merged_points"].cpu().numpy().tobytes() == y["merged_points"].cpu().numpy().tobytes(), c
        spread = max(tb) - min(tb)
        line.update({"per_chunk_ms": 1e3 * statistics.median(tb), "per_chunk_ms_all": [round(1e3 * t, 3) for t in tb],
                     "per_chunk_spread_ms": 1e3 * spread, "per_chunk_over_finish_chunks": statistics.median(tb) / statistics.median(ta),
                     "batched_not_slower": bool(statistics.median(ta) <= statistics.median(tb) + spread), "equal_to_per_chunk": True})
    if not args.only_batched and not args.no_restated:
        sys.path.insert(0, os.path.join(ROOT, "tests"))
        import finish_ref
        t0 = time.perf_counter()
        ref = finish_ref.finish_chunks([h[0] for h in host], [h[1] for h in host], labels_h, [h[2] for h in host], workers=1)
        line["numpy_one_core_ms"] = 1e3 * (time.perf_counter() - t0)
        line["numpy_over_finish_chunks"] = line["numpy_one_core_ms"] / line["finish_chunks_ms"]
        line["chunks_equal_to_numpy"] = int(sum(np.array_equal(d["ground_keep"].cpu().numpy(), r["keep"]) and
                                                np.array_equal(d["fine_instance"].cpu().numpy(), r["fine_label"])
                                                for d, r in zip(a, ref)))
    print(json.dumps(line), flush=True)
    if args.out:
        with open(args.out, "w") as f:
            f.write(json.dumps(line) + "\n")


if __name__ == "__main__":
    main()
