"""Chunk preparation of a whole map on the device vs cutting its chunks (one JSON line).

A synthetic street (synth.street_map, >= 10 M minor points at the default length) is made resident on the GPU; then
  prep_s   -- warm wall time of prep_api.chunk_and_downsample_point_clouds from the resident tensors (crop of every chunk,
              statistical outlier filter per chunk, 0.35 m voxels; both clouds), median of --reps;
  cut_s    -- warm wall time of sharding.run_chunks over the same map's non-ground major chunks (CONFIG_SPATIAL: the map has no
              TARL features), median of --reps;
  cpu_restatement_s -- the same preparation by tests/prep_ref.py on this host (cKDTree, workers=16): a restatement of open3d's
              rules, NOT open3d (not installed), run once (--no-cpu skips it).
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (with --no-cpu --reps 1).

    python tools/run_prep.py [--length 720] [--reps 3] [--no-cpu] [--out profiles/prep_line.json]
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


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--length", type=float, default=720.0)
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import torch
    torch.cuda.init()
    from autoinst_amd import prep_api, sharding, synth
    from autoinst_amd.config import CONFIG_SPATIAL
    from autoinst_amd.ncuts_api import Context

    t0 = time.perf_counter()
    m = synth.street_map(a.length, seed=a.seed)
    t_synth = time.perf_counter() - t0
    dev = torch.device("cuda", 0)
    ng = torch.as_tensor(m["nonground"], device=dev)
    gr = torch.as_tensor(m["ground"], device=dev)
    labels = {k: torch.as_tensor(v, device=dev) for k, v in m["labels"].items()}
    ctx = Context(0)
    args = (ng, gr, m["T_pcd"], m["positions"], m["first_position"], m["indices"], labels)

    def prep():
        torch.cuda.synchronize()
        t = time.perf_counter()
        d = prep_api.chunk_and_downsample_point_clouds(*args, ctx=ctx)
        torch.cuda.synchronize()
        return time.perf_counter() - t, d

    _, d = prep()   # warm-up: code objects, workspace
    prep_times = [prep()[0] for _ in range(a.reps)]
    major = d["pcd_nonground_chunks_major_downsampling"]
    cfg = dict(alpha=CONFIG_SPATIAL["alpha"], theta=0.0, gamma=0.0, T=CONFIG_SPATIAL["T"])
    ctxs = [Context(0) for _ in range(2)]
    chunks = [(x, None) for x in major]
    sharding.run_chunks(chunks, contexts=ctxs, **cfg)   # warm-up
    cut_times = []
    for _ in range(a.reps):
        torch.cuda.synchronize()
        t = time.perf_counter()
        sharding.run_chunks(chunks, contexts=ctxs, **cfg)
        torch.cuda.synchronize()
        cut_times.append(time.perf_counter() - t)
    res = {
        "what": "chunk preparation (crop + statistical outliers + 0.35 m voxels, both clouds) vs the cut of the same map",
        "length_m": a.length, "points_nonground": int(ng.shape[0]), "points_ground": int(gr.shape[0]),
        "chunks": len(major), "crop_points_nonground": int(sum(int(x.numel()) for x in d["indices"])),
        "crop_points_ground": int(sum(int(x.numel()) for x in d["indices_ground"])),
        "major_points_nonground": int(sum(int(x.shape[0]) for x in major)),
        "prep_s": statistics.median(prep_times), "prep_s_all": prep_times,
        "cut_s": statistics.median(cut_times), "cut_s_all": cut_times, "cut_config": "CONFIG_SPATIAL, run_chunks threads=2 batch=12",
        "synth_s": t_synth,
    }
    res["prep_over_cut"] = res["prep_s"] / res["cut_s"]
    if not a.no_cpu:
        import prep_ref
        t = time.perf_counter()
        prep_ref.chunk_and_downsample_point_clouds(m["nonground"], m["ground"], m["T_pcd"], m["positions"], m["first_position"],
                                                   m["indices"], m["labels"], workers=16)
        res["cpu_restatement_s"] = time.perf_counter() - t
        res["cpu_restatement_note"] = "tests/prep_ref.py (cKDTree workers=16, NumPy): a restatement of open3d's rules, not open3d"
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
