"""The camera projection on the device vs its CPU restatement and the host hidden point removal (one JSON line).

On synth.camera_rig (29 views, 27 x 88 x 384 float32 feature maps, 376 x 1241 SAM label images) at the rig chunk's ~33 k points
and at 200 k points drawn from the chunk's minor points:
  device_ms           -- warm wall time of camera_api.camera_features with every input resident on the GPU (torch tensors; the
                         call ends in a device synchronise), median of --reps;
  host_inputs_ms      -- the same from NumPy inputs: the feature maps (105 MB) and SAM images are copied to the device by the call;
  cpu_restatement_s   -- the same call by tests/camera_ref.py, run once (--no-cpu skips it): single-threaded, since its
                         cKDTree queries run with workers=1 and the rest is element-wise NumPy (no BLAS);
  hpr_s_per_view      -- camera_api.hidden_point_removal (scipy's qhull, host) of one view's crop of the map (the chunk box,
                         ~360 k points): what image_based_features_per_patch spends per view when no hpr_masks are given.
Kernel times: run this under `rocprofv3 --kernel-trace --stats` in a run of its own (with --no-cpu --reps 1).

    python tools/run_camera.py [--reps 5] [--no-cpu] [--out profiles/camera_rig_line.json]
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
    ap.add_argument("--seed", type=int, default=0)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--no-cpu", action="store_true")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()

    import numpy as np
    import torch
    torch.cuda.init()
    from autoinst_amd import camera_api, synth
    from autoinst_amd.ncuts_api import Context

    rig = synth.camera_rig(n_views=29, seed=a.seed)
    cloud = rig["pcd"][rig["chunk_indices"]]
    vis = [np.where(m[rig["chunk_indices"]])[0] for m in rig["hpr_masks"]]
    rng = np.random.default_rng(7)
    q200 = cloud[rng.choice(cloud.shape[0], 200_000, replace=False)] + rng.normal(0.0, 0.05, (200_000, 3))
    ctx = Context(0)
    dev = torch.device("cuda", 0)
    fm_d = torch.as_tensor(rig["feature_maps"], device=dev)
    sam_d = torch.as_tensor(rig["sam_images"], device=dev)
    cloud_d = torch.as_tensor(cloud, device=dev)
    vis_d = [torch.as_tensor(v, device=dev) for v in vis]
    fixed = (rig["T_pcd2cam"], rig["K"], rig["image_hw"])

    def timed(fn):
        torch.cuda.synchronize()
        t = time.perf_counter()
        r = fn()
        torch.cuda.synchronize()
        return (time.perf_counter() - t) * 1e3, r

    out = {"metric": "camera_features", "views": 29, "feature_map": list(rig["feature_maps"].shape[1:]),
           "image_hw": list(rig["image_hw"]), "cloud_points": int(cloud.shape[0])}
    for name, q in (("rig", rig["points"]), ("200k", q200)):
        q_d = torch.as_tensor(q, device=dev)

        def on_device():
            return camera_api.camera_features(q_d, cloud_d, vis_d, *fixed, feature_maps=fm_d, sam_images=sam_d, ctx=ctx)

        def from_host():
            return camera_api.camera_features(q, cloud, vis, *fixed, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"],
                                              ctx=ctx)
        timed(on_device)   # warm-up: code objects, workspace
        timed(from_host)
        dt = [timed(on_device)[0] for _ in range(a.reps)]
        ht = [timed(from_host)[0] for _ in range(a.reps)]
        r = on_device()
        rec = {"n": int(q.shape[0]), "device_ms": round(statistics.median(dt), 3), "device_ms_all": [round(x, 3) for x in dt],
               "host_inputs_ms": round(statistics.median(ht), 3), "pairs_labelled": int((r["sam"] != -1).sum().item()),
               "mean_views": round(float(r["dino_views"].double().mean().item()), 3)}
        if not a.no_cpu:
            import camera_ref
            t = time.perf_counter()
            camera_ref.camera_features(q, cloud, vis, *fixed, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"])
            rec["cpu_restatement_s"] = round(time.perf_counter() - t, 3)
        out[name] = rec
    # host hidden point removal of one view's crop (image_utils.py:158-179 with the chunk's box)
    pts = rig["pcd"][rig["chunk_indices"]]
    cam = camera_api.transform_points(pts, rig["T_pcd2cam"][14])
    t = time.perf_counter()
    v = camera_api.hidden_point_removal(cam)
    out["hpr_s_per_view"] = round(time.perf_counter() - t, 3)
    out["hpr_points"] = int(pts.shape[0])
    out["hpr_visible"] = int(v.size)
    out["device"] = torch.cuda.get_device_name(0)
    line = json.dumps(out)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()
