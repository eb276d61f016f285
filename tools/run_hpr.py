"""Hidden point removal of the rig's 29 views on the device vs scipy's qhull on the host (one JSON line).

On synth.camera_rig (29 views) with the chunk's crop of the map (~358 k points) resident on the GPU:
  device_ms           -- warm wall time of ONE camera_api.visible_sets call for all views (the call ends in a device
                         synchronise; the index tensors are formed behind it by torch), median of --reps; device_ms_per_view;
  flags_ms            -- the same without forming the index tensors: the library call alone (flags, counts, status);
  qhull_s_per_view    -- camera_api.hidden_point_removal of every view's crop on the host (--qhull-views of them, default all),
                         min / median / max, and qhull_s_total their sum;
  local_share         -- the share of the points that the local pass settles (proves hidden), mean over the views;
  resolves_mean / max -- re-solves per point over all views;
  differing_locations -- per compared view, distinct locations on which the device and qhull disagree (tests/test_gpu_hpr.py).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (with --qhull-views 0 --reps 1).

    python tools/run_hpr.py [--reps 5] [--qhull-views 29] [--out profiles/hpr_rig_line.json]
"""
from __future__ import annotations

import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--qhull-views", type=int, default=29)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.init()
    from autoinst_amd import camera_api, synth
    from autoinst_amd.config import HPR_RADIUS
    from autoinst_amd.ncuts_api import Context

    rig = synth.camera_rig(n_views=29, seed=a.seed)
    cloud = rig["pcd"][rig["chunk_indices"]]
    T = rig["T_pcd2cam"]
    V, n = int(T.shape[0]), int(cloud.shape[0])
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    cloud_d = torch.as_tensor(cloud, device=dev)

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    def on_device():
        return camera_api.visible_sets(cloud_d, T, radius_factor=HPR_RADIUS, return_stats=True, ctx=ctx)

    timed(on_device)   # warm-up: code objects, workspace
    dt = [timed(on_device)[0] for _ in range(a.reps)]
    sets, stats = on_device()
    # the library call alone: what visible_sets does before it forms the index tensors
    from autoinst_amd import _ffi
    lib = _ffi.load()
    flags = torch.empty((V, n), dtype=torch.uint8, device=dev)
    counts, status = np.zeros(V, np.int64), np.zeros(V, np.int32)
    Tc = np.ascontiguousarray(T, dtype=np.float64)

    def flags_only():
        return lib.ai_hidden_points(ctx._h, cloud_d.data_ptr(), n, None, 0, Tc.ctypes.data, V, float(HPR_RADIUS), _ffi.AI_MEM_DEVICE,
                                    flags.data_ptr(), counts.ctypes.data, status.ctypes.data, None)
    timed(flags_only)
    ft = [timed(flags_only)[0] for _ in range(a.reps)]
    assert flags_only() == 0 and not status.any()

    visible = [int(s.numel()) for s in sets]
    out = {"metric": "hidden_point_removal", "views": V, "points": n, "radius_factor": HPR_RADIUS,
           "device_ms": round(statistics.median(dt), 3), "device_ms_all": [round(x, 3) for x in dt],
           "device_ms_per_view": round(statistics.median(dt) / V, 3),
           "flags_ms": round(statistics.median(ft), 3), "flags_ms_per_view": round(statistics.median(ft) / V, 3),
           "visible_min_max": [min(visible), max(visible)],
           "local_share": round(float(stats[:, 0].sum()) / (V * n), 4),
           "resolves_mean": round(float(stats[:, 1].sum()) / (V * n), 3), "resolves_max": int(stats[:, 2].max())}
    qt, differing = [], []
    for v in range(min(a.qhull_views, V)):
        cam = camera_api.transform_points(cloud, T[v])
        t = time.perf_counter()
        hull = camera_api.hidden_point_removal(cam, radius_factor=HPR_RADIUS)
        qt.append(time.perf_counter() - t)
        got = sets[v].cpu().numpy()
        _, loc = np.unique(cam, axis=0, return_inverse=True)
        loc = loc.reshape(-1)
        k = int(loc.max()) + 1
        differing.append(int(((np.bincount(loc[got], minlength=k) > 0) != (np.bincount(loc[hull], minlength=k) > 0)).sum()))
    if qt:
        out.update({"qhull_views": len(qt), "qhull_s_per_view": [round(min(qt), 3), round(statistics.median(qt), 3), round(max(qt), 3)],
                    "qhull_s_total": round(sum(qt), 3), "differing_locations": differing,
                    "speedup_per_view": round(statistics.median(qt) * 1e3 / (statistics.median(dt) / V), 1)})
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
