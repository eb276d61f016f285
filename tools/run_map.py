"""The minor-voxel map of a raw street on the device: the fused entry vs the calls it replaces (one JSON line).

A synthetic raw-density street (synth.street_map(length, step=0.02): ~65 M points at the default 720 m) is made resident on the
GPU; then, warm, alternating, --reps times each (wall clock around calls that end in a device synchronise):
  fused_s     -- prep_api.downsample_map: both clouds to 0.05 m voxels, nearest raw point of every mean, four label gathers;
  composed_s  -- the same result from the entry points that existed before: prep_api.voxel_down_sample, then ai_nn1_project
                 (points_api.nn1_index's kernel, called on the same resident tensors) from the means to the raw cloud, then the
                 same gathers.  The two results are compared (equal indices and labels) before anything is timed.
  prep_s_720  -- the chunk preparation of the 720 m minor map (profiles/prep_street720_line.json), for scale.
`workspace` is Context.mem_info() after the fused calls.  Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a
run of its own (with --reps 1 --no-composed).

    python tools/run_map.py [--length 720] [--reps 5] [--no-composed] [--out profiles/map_street_line.json]
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
sys.path[:0] = [ROOT]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=float, default=720.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-composed", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    torch.cuda.init()
    from autoinst_amd import _ffi, prep_api, synth
    from autoinst_amd.ncuts_api import Context

    t0 = time.perf_counter()
    m = synth.street_map(a.length, seed=a.seed, step=0.02)
    t_synth = time.perf_counter() - t0
    dev = torch.device("cuda", 0)
    ng = torch.as_tensor(m["nonground"], device=dev)
    gr = torch.as_tensor(m["ground"], device=dev)
    labels = {k: torch.as_tensor(v, device=dev) for k, v in m["labels"].items()}
    ctx = Context(0)
    lib = _ffi.load()

    def fused():
        return prep_api.downsample_map(ng, gr, labels, ctx=ctx)

    def composed():
        minor, kitti = {}, {}
        for cloud, raw in (("ground", gr), ("nonground", ng)):
            out = prep_api.voxel_down_sample(raw, 0.05, ctx=ctx)
            idx = torch.empty(out.shape[0], dtype=torch.int32, device=dev)
            _ffi.check(lib.ai_nn1_project(ctx._h, C.c_void_p(out.data_ptr()), out.shape[0], C.c_void_p(raw.data_ptr()), raw.shape[0],
                                          _ffi.AI_MEM_DEVICE, C.c_void_p(idx.data_ptr()), None), "ai_nn1_project")
            minor[cloud] = out
            for kind in ("seg", "instance"):
                kitti[f"{kind}_{cloud}"] = labels[f"{kind}_{cloud}"].reshape(-1).index_select(0, idx.long())
        return minor["ground"], minor["nonground"], kitti

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return time.perf_counter() - t, r

    _, f = timed(fused)   # warm-up: code objects, workspace
    res = {
        "what": "raw street -> 0.05 m minor-voxel maps + labels of the nearest raw point, both clouds, resident tensors",
        "length_m": a.length, "raw_points_nonground": int(ng.shape[0]), "raw_points_ground": int(gr.shape[0]),
        "minor_points_nonground": int(f[1].shape[0]), "minor_points_ground": int(f[0].shape[0]), "synth_s": t_synth,
    }
    ft, ct = [], []
    if not a.no_composed:
        _, c = timed(composed)
        same = bool(torch.equal(f[0], c[0]) and torch.equal(f[1], c[1]) and all(torch.equal(f[2][k], c[2][k]) for k in f[2]))
        res["composed_equals_fused"] = same
        if not same:
            raise SystemExit("the composed calls and the fused entry disagree: " + json.dumps(res))
        del c
    for _ in range(a.reps):
        ft.append(timed(fused)[0])
        if not a.no_composed:
            ct.append(timed(composed)[0])
    res["workspace"] = ctx.mem_info()
    res["fused_s"], res["fused_s_all"], res["fused_spread_s"] = statistics.median(ft), ft, max(ft) - min(ft)
    if ct:
        res["composed_s"], res["composed_s_all"], res["composed_spread_s"] = statistics.median(ct), ct, max(ct) - min(ct)
        res["composed_over_fused"] = res["composed_s"] / res["fused_s"]
        res["bar_met"] = bool(res["composed_s"] - res["fused_s"] > max(res["fused_spread_s"], res["composed_spread_s"]))
    try:
        with open(os.path.join(ROOT, "profiles", "prep_street720_line.json")) as fh:
            res["prep_s_720"] = json.loads(fh.readline())["prep_s"]
    except (OSError, KeyError, ValueError):
        res["prep_s_720"] = None
    res["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as fh:
            fh.write(line + "\n")


if __name__ == "__main__":
    main()
