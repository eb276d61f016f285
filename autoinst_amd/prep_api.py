"""The step that produces the chunks: ``chunk_and_downsample_point_clouds`` (``pipeline/dataset/dataset_utils.py:489-567``,
called at ``run_pipeline.py:129``) on arrays instead of open3d clouds.

* `box_select` -- the crop of every chunk from the whole minor-voxel map (``chunk_generation.py:134-137``), all chunks in one
  pass over the map;
* `statistical_inlier_indices` -- ``get_statistical_inlier_indices`` (``point_cloud_utils.py:198-202``), i.e. open3d 0.17's
  ``PointCloud::RemoveStatisticalOutliers`` as it is written:

  - ``k = min(nb_neighbors, n)``; ``avg[i]`` = mean of the Euclidean distances of the k nearest points of point i (i itself
    included, at distance 0), summed in ascending distance order;
  - ``mean`` = sum of all ``avg > 0`` divided by the number of ALL points (the ``avg == 0`` ones count in the denominator);
  - ``std = sqrt(sum over avg > 0 of (avg - mean)^2 / (n - 1))``;
  - a point is kept iff ``avg > 0 and avg < mean + std_ratio * std``; the kept indices are ascending;
  - ``nb_neighbors < 1`` or ``std_ratio <= 0`` raises ``ValueError``; an empty cloud (and a single point) keeps nothing;
* `voxel_down_sample` -- open3d ``PointCloud::VoxelDownSample`` (``dataset_utils.py:534-535``): ``vmin = min_bound -
  voxel_size / 2``, voxel ``floor((p - vmin) / voxel_size)``, output point = sum of the voxel's points in input order / count.
  open3d's output order is that of a hash map and means nothing; ours is ascending ``(ix, iy, iz)``;
* `chunks_from_pointcloud` / `chunk_and_downsample_point_clouds` -- the reference's two functions
  (``chunk_generation.py:96-180``, ``dataset_utils.py:489-567``) with point arrays where the reference has open3d clouds;
* `voxel_down_sample_nearest` / `downsample_map` -- one step earlier, ``load_and_downsample_point_clouds``
  (``dataset_utils.py:201-384``, called at ``run_pipeline.py:110``): the aggregated raw clouds go to ``MINOR_VOXEL_SIZE`` voxels
  and every minor point takes the label of its nearest RAW point (the four KD-tree loops of ``:299-370``).  Nearest = smallest
  ``(dx*dx + dy*dy) + dz*dz``, ties to the smaller raw index: the tie rule is ours, open3d's KD-tree defines none.  Not
  reproduced: the order of open3d's hash map (ours is ascending voxel order), open3d's choice among tied points, and the
  coloured clouds of ``color_pcd_by_labels``, which the reference only uses as KD-tree carriers.

All kernels are HIP (``csrc/ai_prep.hip``); there is no CPU fallback.  Inputs are NumPy arrays or float64 torch tensors
on the context's GPU; device inputs give device outputs, so map -> major chunks -> `ncuts_api.build_affinity` /
`sharding.run_chunks` copies no points to the host (only counts come back).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from .config import CHUNK_SIZE, MAJOR_VOXEL_SIZE, MINOR_VOXEL_SIZE, OVERLAP
from .ncuts_api import Context, _is_device_tensor, default_context


def _points(points, name="points"):
    """(n, 3) float64 contiguous array or device tensor; an object with ``.points`` (an open3d cloud) gives its points."""
    if not _is_device_tensor(points) and hasattr(points, "points") and not isinstance(points, np.ndarray):
        points = np.asarray(points.points)
    if _is_device_tensor(points):
        import torch
        if points.dtype != torch.float64 or points.dim() != 2 or points.shape[1] != 3:
            raise ValueError(f"{name} on the device must be a float64 (n, 3) tensor")
        return points.contiguous()
    a = np.ascontiguousarray(points, dtype=np.float64)
    if a.size == 0:
        a = a.reshape(0, 3)
    if a.ndim != 2 or a.shape[1] != 3:
        raise ValueError(f"{name} must be (n, 3)")
    return a


def _call_args(pts):
    """(pointer, mem_kind, torch-or-None) of a point buffer; waits for torch's producers of a device buffer."""
    if _is_device_tensor(pts):
        import torch
        torch.cuda.current_stream(pts.device).synchronize()
        return C.c_void_p(pts.data_ptr()), _ffi.AI_MEM_DEVICE, torch
    return pts.ctypes.data, _ffi.AI_MEM_HOST, None


def box_select(points, boxes, *, ctx: Context | None = None):
    """For every box ``(lo, hi)`` (two 3-vectors) the ascending indices of the points with ``lo < p < hi`` on all three axes
    (``chunk_generation.py:134-137``).  One pass over the map for all boxes.  Returns a list of int64 arrays (device tensors
    for device points)."""
    ctx = ctx or default_context()
    pts = _points(points)
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 6))
    nb = b.shape[0]
    if nb == 0:
        return []
    ptr, mem, torch = _call_args(pts)
    n = int(pts.shape[0])
    offs = np.zeros(nb + 1, dtype=np.int64)
    total = C.c_int64(0)
    lib = _ffi.load()
    cap = 2 * n + 1024
    while True:
        out = torch.empty(cap, dtype=torch.int32, device=pts.device) if torch else np.empty(cap, dtype=np.int32)
        optr = C.c_void_p(out.data_ptr()) if torch else out.ctypes.data
        _ffi.check(lib.ai_box_select(ctx._h, ptr, n, b.ctypes.data, nb, mem, cap, optr, offs.ctypes.data, C.byref(total)),
                   "ai_box_select")
        if total.value <= cap:
            break
        cap = int(total.value)
    full = out[:total.value].long() if torch else out[:total.value].astype(np.int64)
    return [full[offs[i]:offs[i + 1]] for i in range(nb)]


def statistical_inlier_indices(points, nb_neighbors=20, std_ratio=2.0, *, return_stats=False, ctx: Context | None = None):
    """Ascending indices of the points open3d's ``remove_statistical_outlier(nb_neighbors, std_ratio)`` keeps (the rules are in
    the module docstring).  With ``return_stats``: ``(indices, avg, {"mean", "std", "threshold"})``, avg per point."""
    ctx = ctx or default_context()
    pts = _points(points)
    nb_neighbors = int(nb_neighbors)
    n = int(pts.shape[0])
    ptr, mem, torch = _call_args(pts)
    if torch:
        keep = torch.empty(max(n, 1), dtype=torch.int32, device=pts.device)
        avg = torch.empty(max(n, 1), dtype=torch.float64, device=pts.device)
        kptr, aptr = C.c_void_p(keep.data_ptr()), C.c_void_p(avg.data_ptr())
    else:
        keep = np.empty(max(n, 1), dtype=np.int32)
        avg = np.empty(max(n, 1), dtype=np.float64)
        kptr, aptr = keep.ctypes.data, avg.ctypes.data
    stats = np.full(3, np.nan)
    nk = C.c_int64(0)
    _ffi.check(_ffi.load().ai_statistical_inliers(ctx._h, ptr, n, nb_neighbors, float(std_ratio), mem, kptr, C.byref(nk), aptr,
                                                  stats.ctypes.data), "ai_statistical_inliers")
    idx = keep[:nk.value].long() if torch else keep[:nk.value].astype(np.int64)
    if not return_stats:
        return idx
    return idx, avg[:n], {"mean": float(stats[0]), "std": float(stats[1]), "threshold": float(stats[2])}


def voxel_down_sample(points, voxel_size=MAJOR_VOXEL_SIZE, *, return_trace=False, ctx: Context | None = None):
    """open3d ``voxel_down_sample(voxel_size)``: the mean point of every occupied voxel, in ascending ``(ix, iy, iz)`` order.
    With ``return_trace``: ``(points, trace)``, ``trace[i]`` = output row of input point i (int32)."""
    ctx = ctx or default_context()
    pts = _points(points)
    n = int(pts.shape[0])
    ptr, mem, torch = _call_args(pts)
    if torch:
        out = torch.empty((max(n, 1), 3), dtype=torch.float64, device=pts.device)
        tr = torch.empty(max(n, 1), dtype=torch.int32, device=pts.device) if return_trace else None
        optr, tptr = C.c_void_p(out.data_ptr()), (C.c_void_p(tr.data_ptr()) if tr is not None else None)
    else:
        out = np.empty((max(n, 1), 3), dtype=np.float64)
        tr = np.empty(max(n, 1), dtype=np.int32) if return_trace else None
        optr, tptr = out.ctypes.data, (tr.ctypes.data if tr is not None else None)
    m = C.c_int64(0)
    _ffi.check(_ffi.load().ai_voxel_down_sample(ctx._h, ptr, n, float(voxel_size), mem, optr, C.byref(m), tptr),
               "ai_voxel_down_sample")
    res = out[:m.value]
    return (res, tr[:n]) if return_trace else res


def voxel_down_sample_nearest(points, voxel_size=MINOR_VOXEL_SIZE, *, return_trace=False, return_dist=False,
                              ctx: Context | None = None):
    """`voxel_down_sample` plus, for every output point, the index of the input point nearest to it (int64): the point whose
    label ``load_and_downsample_point_clouds`` copies (``dataset_utils.py:306-311``).  Smallest ``(dx*dx + dy*dy) + dz*dz``,
    ties to the smaller input index.  Returns ``(points_out, nearest_index)``, then ``trace`` (int32, as `voxel_down_sample`)
    with ``return_trace`` and the distances (float64) with ``return_dist``, in that order.  One sort serves both results."""
    ctx = ctx or default_context()
    pts = _points(points)
    n = int(pts.shape[0])
    ptr, mem, torch = _call_args(pts)
    cap = max(n, 1)
    if torch:
        def new(shape, dtype):
            return torch.empty(shape, dtype=dtype, device=pts.device)

        def addr(a):
            return C.c_void_p(a.data_ptr()) if a is not None else None
        f64, i32 = torch.float64, torch.int32
    else:
        def new(shape, dtype):
            return np.empty(shape, dtype=dtype)

        def addr(a):
            return a.ctypes.data if a is not None else None
        f64, i32 = np.float64, np.int32
    out, nn = new((cap, 3), f64), new(cap, i32)
    tr = new(cap, i32) if return_trace else None
    dist = new(cap, f64) if return_dist else None
    m = C.c_int64(0)
    _ffi.check(_ffi.load().ai_voxel_down_sample_nearest(ctx._h, ptr, n, float(voxel_size), mem, addr(out), C.byref(m), addr(tr),
                                                        addr(nn), addr(dist)), "ai_voxel_down_sample_nearest")
    res = [out[:m.value], nn[:m.value].long() if torch else nn[:m.value].astype(np.int64)]
    if return_trace:
        res.append(tr[:n])
    if return_dist:
        res.append(dist[:m.value])
    return tuple(res)


LABEL_KEYS = ("seg_ground", "seg_nonground", "instance_ground", "instance_nonground")   # dataset_utils.py:192-196


def downsample_map(pcd_nonground, pcd_ground, labels, voxel_size=MINOR_VOXEL_SIZE, *, ctx: Context | None = None):
    """``load_and_downsample_point_clouds`` (``dataset_utils.py:201-384``) on arrays: the two aggregated clouds go to
    ``voxel_size`` voxels and every minor point takes the labels of its nearest raw point.  ``labels`` holds the reference's
    ``seg_ground``, ``seg_nonground``, ``instance_ground``, ``instance_nonground`` (``kitti_labels_*.npz``, ``:186-197``), each
    ``(n,)`` or ``(n, 1)`` of any integer dtype, host array or device tensor.  Returns ``(pcd_ground_minor,
    pcd_nonground_minor, kitti_labels)`` -- the first three values of ``load_downsampled_pcds`` (``:417-453``) -- with
    ``kitti_labels[key] = labels[key].reshape(-1)[nearest_index]``; it goes unchanged into
    `chunk_and_downsample_point_clouds`.  Device clouds give device clouds, and device labels stay on the device."""
    ctx = ctx or default_context()
    missing = [k for k in LABEL_KEYS if k not in labels]
    if missing:
        raise ValueError(f"labels lacks {missing}")
    clouds = {"ground": _points(pcd_ground, "pcd_ground"), "nonground": _points(pcd_nonground, "pcd_nonground")}
    flat = {}
    for k in LABEL_KEYS:
        a = labels[k]
        a = a.reshape(-1) if _is_device_tensor(a) else np.asarray(a).reshape(-1)
        if a.shape[0] != clouds[k.split("_")[1]].shape[0]:
            raise ValueError(f"labels[{k!r}] has {a.shape[0]} entries for {clouds[k.split('_')[1]].shape[0]} points")
        integer = not (a.dtype.is_floating_point or a.dtype.is_complex) if _is_device_tensor(a) else a.dtype.kind in "iub"
        if not integer:
            raise ValueError(f"labels[{k!r}] must be an integer array")
        flat[k] = a
    minor, kitti_labels = {}, {}
    for cloud, pts in clouds.items():
        minor[cloud], nearest = voxel_down_sample_nearest(pts, voxel_size, ctx=ctx)
        for kind in ("seg", "instance"):
            kitti_labels[f"{kind}_{cloud}"] = _take(flat[f"{kind}_{cloud}"], nearest)
    return minor["ground"], minor["nonground"], kitti_labels


def chunk_centres(T_pcd, positions, first_position, indices, *, chunk_size=CHUNK_SIZE, overlap=OVERLAP):
    """The trajectory walk of ``chunks_from_pointcloud``: the path length since the last chunk grows position by position; once
    it exceeds ``min(chunk_size[:2]) - overlap`` a chunk is centred at that position, in the map's frame
    (``inv(T_pcd[:3, :3]) @ (position - first_position)``), and the length starts again from 0.  Returns
    ``(centres, centre_ids)``: the centres and the ``indices`` entries of their positions."""
    step = min(float(chunk_size[0]), float(chunk_size[1])) - overlap
    R_inv = np.linalg.inv(np.asarray(T_pcd, dtype=np.float64)[:3, :3])
    first = np.asarray(first_position, dtype=np.float64)
    centres, ids = [], []
    travelled, prev = 0.0, None
    for pos, idx in zip(positions, indices):
        pos = np.asarray(pos, dtype=np.float64)
        if prev is not None:
            travelled += np.linalg.norm(pos - prev)
            if travelled > step:
                centres.append(R_inv @ (pos - first))
                ids.append(idx)
                travelled = 0.0
        prev = pos
    return centres, ids


def _take(a, idx):
    """a[idx] for a host array or a device tensor (host indices are moved to wherever `a` lives)."""
    if _is_device_tensor(a):
        if not _is_device_tensor(idx):
            import torch
            idx = torch.as_tensor(np.asarray(idx), device=a.device)
        return a.index_select(0, idx.to(a.device))
    if _is_device_tensor(idx):
        idx = idx.cpu().numpy()
    return np.asarray(a)[idx]


def chunks_from_pointcloud(points, T_pcd, positions, first_position, indices, labels=None, ground=False, *,
                           chunk_size=CHUNK_SIZE, overlap=OVERLAP, nb_neighbors=20, std_ratio=2.0, ctx: Context | None = None):
    """``chunks_from_pointcloud`` (``chunk_generation.py:96-180``) on arrays: returns the reference's 7-tuple
    ``(chunks, chunk_indices, center_positions, center_ids, chunk_bounds, kitti_out, obbs)`` where ``chunks[c]`` are the
    points of chunk c (its crop, then the statistical outlier filter), ``chunk_indices[c]`` the crop's map indices and
    ``kitti_out`` (when ``labels`` is given) ``labels[...][ids][inliers]`` per chunk.  The crop of all chunks is one
    `box_select`; the filter runs per chunk on the device."""
    ctx = ctx or default_context()
    pts = _points(points)
    centres, centre_ids = chunk_centres(T_pcd, positions, first_position, indices, chunk_size=chunk_size, overlap=overlap)
    half = 0.5 * np.asarray(chunk_size, dtype=np.float64)
    bounds = [(c - half, c + half) for c in centres]
    ids_all = box_select(pts, [np.concatenate(b) for b in bounds], ctx=ctx) if bounds else []
    kitti_out = {"panoptic": [], "semantic": [], "instance": []} if labels is not None else None
    sem_key, inst_key = ("seg_ground", "instance_ground") if ground else ("seg_nonground", "instance_nonground")
    chunks = []
    for ids in ids_all:
        crop = _take(pts, ids)
        inl = statistical_inlier_indices(crop, nb_neighbors, std_ratio, ctx=ctx)
        chunks.append(_take(crop, inl))
        if kitti_out is not None:
            kitti_out["semantic"].append(_take(_take(labels[sem_key], ids), inl))
            kitti_out["instance"].append(_take(_take(labels[inst_key], ids), inl))
    return chunks, list(ids_all), centres, centre_ids, bounds, kitti_out, [0] * len(centres)


def chunk_and_downsample_point_clouds(pcd_nonground_minor, pcd_ground_minor, T_pcd, positions, first_position,
                                      sampled_indices_global, kitti_labels=None, *, voxel_size=MAJOR_VOXEL_SIZE,
                                      ctx: Context | None = None):
    """``chunk_and_downsample_point_clouds`` (``dataset_utils.py:489-567``): the same arguments and a dict with the reference's
    keys.  Point clouds are (n, 3) arrays / device tensors; the major-voxel chunks are in ascending voxel order."""
    ctx = ctx or default_context()
    ng, ng_ids, centres, centre_ids, bounds, k_ng, _ = chunks_from_pointcloud(
        pcd_nonground_minor, T_pcd, positions, first_position, sampled_indices_global, labels=kitti_labels, ctx=ctx)
    gr, gr_ids, _, _, _, k_gr, obbs = chunks_from_pointcloud(
        pcd_ground_minor, T_pcd, positions, first_position, sampled_indices_global, labels=kitti_labels, ground=True, ctx=ctx)
    return {
        "pcd_nonground_chunks": ng,
        "pcd_ground_chunks": gr,
        "pcd_nonground_chunks_major_downsampling": [voxel_down_sample(c, voxel_size, ctx=ctx) for c in ng],
        "pcd_ground_chunks_major_downsampling": [voxel_down_sample(c, voxel_size, ctx=ctx) for c in gr],
        "indices": ng_ids,
        "indices_ground": gr_ids,
        "center_positions": centres,
        "center_ids": centre_ids,
        "chunk_bounds": bounds,
        "kitti_labels": {"nonground": k_ng, "ground": k_gr},
        "obbs": obbs,
    }
