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
  coloured clouds of ``color_pcd_by_labels``, which the reference only uses as KD-tree carriers;
* `aggregate_scans` / `aggregate_pointcloud` -- the head of the chain, ``aggregate_pointcloud``
  (``pipeline/utils/point_cloud/aggregate_pointcloud.py:12-188``, called at ``run_pipeline.py:102``) with the dataset's filter
  chain and label decodes: all scans of a map go to the two aggregated raw clouds in one device call (``csrc/ai_aggregate.hip``,
  rules A1-A6 in ``include/autoinst_hip.h``).  Patchwork++ stays an input: per-scan masks or index lists.  Not reproduced: ICP
  registration, the bits of open3d's unseeded RANSAC plane, and the order of the ground segmentation's index list (each map is
  in ascending input position);
* `ground_planes` -- the other ground segmentation of the reference, ``segment_plane(distance_threshold=0.4, ransac_n=3,
  num_iterations=2000)`` (``aggregate_pointcloud.py:115-123``), as one seeded RANSAC plane per scan for all scans of a map in
  one device call (``csrc/ai_ground.hip``, rules G1-G7); ``aggregate_scans(ground="ransac")`` and
  ``aggregate_pointcloud(ground_segmentation="ransac")`` feed its flags to the aggregation on the device.  Not reproduced:
  open3d's generator, its rmse tie-break, its early exit and its refit.

All kernels are HIP (``csrc/ai_prep.hip``); there is no CPU fallback.  Inputs are NumPy arrays or float64 torch tensors
on the context's GPU; device inputs give device outputs, so map -> major chunks -> `ncuts_api.build_affinity` /
`sharding.run_chunks` copies no points to the host (only counts come back).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from . import _ffi
from .config import CHUNK_SIZE, MAJOR_VOXEL_SIZE, MINOR_VOXEL_SIZE, OVERLAP
from ._buffers import grow, offsets_of, place_of, points_f64
from .ncuts_api import Context, _is_device_tensor, default_context


def box_select(points, boxes, *, ctx: Context | None = None):
    """For every box ``(lo, hi)`` (two 3-vectors) the ascending indices of the points with ``lo < p < hi`` on all three axes
    (``chunk_generation.py:134-137``).  One pass over the map for all boxes.  Returns a list of int64 arrays (device tensors
    for device points)."""
    ctx = ctx or default_context()
    pts = points_f64(points)
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 6))
    nb = b.shape[0]
    if nb == 0:
        return []
    place = place_of(pts)
    n = int(pts.shape[0])
    offs = np.zeros(nb + 1, dtype=np.int64)
    lib = _ffi.load()

    def select(cap):
        out, total = place.new(cap, np.int32), C.c_int64(0)
        place.sync()
        _ffi.check(lib.ai_box_select(ctx._h, place.addr(pts), n, b.ctypes.data, nb, place.mem, cap, place.addr(out), offs.ctypes.data,
                                     C.byref(total)), "ai_box_select")
        return total.value, out
    total, out = grow(select, 2 * n + 1024)
    full = place.index64(out[:total])
    return [full[offs[i]:offs[i + 1]] for i in range(nb)]


def statistical_inlier_indices(points, nb_neighbors=20, std_ratio=2.0, *, return_stats=False, ctx: Context | None = None):
    """Ascending indices of the points open3d's ``remove_statistical_outlier(nb_neighbors, std_ratio)`` keeps (the rules are in
    the module docstring).  With ``return_stats``: ``(indices, avg, {"mean", "std", "threshold"})``, avg per point."""
    ctx = ctx or default_context()
    pts = points_f64(points)
    nb_neighbors = int(nb_neighbors)
    n = int(pts.shape[0])
    place = place_of(pts)
    keep, avg = place.new(max(n, 1), np.int32), place.new(max(n, 1), np.float64)
    stats = np.full(3, np.nan)
    nk = C.c_int64(0)
    place.sync()
    _ffi.check(_ffi.load().ai_statistical_inliers(ctx._h, place.addr(pts), n, nb_neighbors, float(std_ratio), place.mem, place.addr(keep),
                                                  C.byref(nk), place.addr(avg), stats.ctypes.data), "ai_statistical_inliers")
    idx = place.index64(keep[:nk.value])
    if not return_stats:
        return idx
    return idx, avg[:n], {"mean": float(stats[0]), "std": float(stats[1]), "threshold": float(stats[2])}


def voxel_down_sample(points, voxel_size=MAJOR_VOXEL_SIZE, *, return_trace=False, ctx: Context | None = None):
    """open3d ``voxel_down_sample(voxel_size)``: the mean point of every occupied voxel, in ascending ``(ix, iy, iz)`` order.
    With ``return_trace``: ``(points, trace)``, ``trace[i]`` = output row of input point i (int32)."""
    ctx = ctx or default_context()
    pts = points_f64(points)
    n = int(pts.shape[0])
    place = place_of(pts)
    out = place.new((max(n, 1), 3), np.float64)
    tr = place.new(max(n, 1), np.int32) if return_trace else None
    m = C.c_int64(0)
    place.sync()
    _ffi.check(_ffi.load().ai_voxel_down_sample(ctx._h, place.addr(pts), n, float(voxel_size), place.mem, place.addr(out), C.byref(m),
                                                place.addr(tr)), "ai_voxel_down_sample")
    res = out[:m.value]
    return (res, tr[:n]) if return_trace else res


def voxel_down_sample_nearest(points, voxel_size=MINOR_VOXEL_SIZE, *, return_trace=False, return_dist=False,
                              ctx: Context | None = None):
    """`voxel_down_sample` plus, for every output point, the index of the input point nearest to it (int64): the point whose
    label ``load_and_downsample_point_clouds`` copies (``dataset_utils.py:306-311``).  Smallest ``(dx*dx + dy*dy) + dz*dz``,
    ties to the smaller input index.  Returns ``(points_out, nearest_index)``, then ``trace`` (int32, as `voxel_down_sample`)
    with ``return_trace`` and the distances (float64) with ``return_dist``, in that order.  One sort serves both results."""
    ctx = ctx or default_context()
    pts = points_f64(points)
    n = int(pts.shape[0])
    place = place_of(pts)
    cap = max(n, 1)
    out, nn = place.new((cap, 3), np.float64), place.new(cap, np.int32)
    tr = place.new(cap, np.int32) if return_trace else None
    dist = place.new(cap, np.float64) if return_dist else None
    m = C.c_int64(0)
    place.sync()
    _ffi.check(_ffi.load().ai_voxel_down_sample_nearest(ctx._h, place.addr(pts), n, float(voxel_size), place.mem, place.addr(out),
                                                        C.byref(m), place.addr(tr), place.addr(nn), place.addr(dist)),
               "ai_voxel_down_sample_nearest")
    res = [out[:m.value], place.index64(nn[:m.value])]
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
    clouds = {"ground": points_f64(pcd_ground, "pcd_ground"), "nonground": points_f64(pcd_nonground, "pcd_nonground")}
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
    pts = points_f64(points)
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


AGGREGATE_LABEL_KINDS = ("seg", "instance", "panoptic")   # aggregate_pointcloud.py:175-182


def _scan_points(scan_points, scan_offsets):
    """(xyz (M, 3) float32 contiguous array or device tensor, offsets (n_scans + 1) int64) of either input form."""
    if isinstance(scan_points, (list, tuple)):
        if scan_offsets is not None:
            raise ValueError("scan_offsets goes with one (M, 3) array, not with a list of scans")
        if any(_is_device_tensor(p) for p in scan_points):
            import torch
            if not all(_is_device_tensor(p) and p.dtype == torch.float32 and p.dim() == 2 and p.shape[1] in (3, 4) for p in scan_points):
                raise ValueError("scans on the device must all be float32 (n, 3) or (n, 4) tensors")
            off = offsets_of([int(p.shape[0]) for p in scan_points])
            return torch.cat([p[:, :3] for p in scan_points]).contiguous(), off
        parts = []
        for k, p in enumerate(scan_points):
            a = np.asarray(p)
            if a.size == 0:
                a = np.zeros((0, 3), dtype=np.float32)
            if a.dtype != np.float32 or a.ndim != 2 or a.shape[1] not in (3, 4):
                raise ValueError(f"scan {k} must be a float32 (n, 3) or (n, 4) array, as dataset.get_point_cloud returns it")
            parts.append(a[:, :3])
        xyz = np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, 3), dtype=np.float32)
        return xyz, offsets_of([a.shape[0] for a in parts])
    if scan_offsets is None:
        raise ValueError("one array of points needs scan_offsets=")
    off = np.ascontiguousarray(np.asarray(scan_offsets, dtype=np.int64).reshape(-1))
    if off.shape[0] < 1:
        raise ValueError("scan_offsets must hold n_scans + 1 entries")
    if _is_device_tensor(scan_points):
        import torch
        if scan_points.dtype != torch.float32 or scan_points.dim() != 2 or scan_points.shape[1] != 3:
            raise ValueError("scan_points on the device must be a float32 (M, 3) tensor")
        xyz = scan_points.contiguous()
    else:
        xyz = np.asarray(scan_points)
        if xyz.size == 0:
            xyz = np.zeros((0, 3), dtype=np.float32)
        if xyz.dtype != np.float32 or xyz.ndim != 2 or xyz.shape[1] != 3:
            raise ValueError("scan_points must be a float32 (M, 3) array")
        xyz = np.ascontiguousarray(xyz)
    if int(off[-1]) != int(xyz.shape[0]):
        raise ValueError(f"scan_offsets ends at {int(off[-1])} for {int(xyz.shape[0])} points")
    return xyz, off


def _label_words(labels, off, like):
    """The raw label words of all scans as one buffer of 32-bit words where `like` lives (device: an int32 tensor with the
    words' bits).  Any integer dtype whose values fit uint32."""
    M = int(off[-1])
    if isinstance(labels, (list, tuple)):
        if len(labels) != off.shape[0] - 1:
            raise ValueError(f"{len(labels)} label arrays for {off.shape[0] - 1} scans")
        if any(_is_device_tensor(a) for a in labels):
            import torch
            labels = torch.cat([a.reshape(-1) for a in labels]) if labels else torch.zeros(0, dtype=torch.int64, device=like.device)
        else:
            for k, a in enumerate(labels):
                if np.asarray(a).size != off[k + 1] - off[k]:
                    raise ValueError(f"labels of scan {k} have {np.asarray(a).size} entries for {off[k + 1] - off[k]} points")
            labels = np.concatenate([np.asarray(a).reshape(-1) for a in labels]) if labels else np.zeros(0, dtype=np.uint32)
    if _is_device_tensor(labels):
        import torch
        t = labels.reshape(-1)
        if t.dtype.is_floating_point or t.dtype.is_complex or t.dtype == torch.bool:
            raise ValueError("labels must be an integer tensor")
        if t.shape[0] != M:
            raise ValueError(f"labels have {t.shape[0]} entries for {M} points")
        if t.dtype == getattr(torch, "uint32", None):
            words = t.contiguous().view(torch.int32)
        else:
            t = t.to(torch.int64)
            if M and (int(t.min()) < 0 or int(t.max()) > 0xFFFFFFFF):
                raise ValueError("a label word does not fit uint32")
            words = torch.where(t >= 2 ** 31, t - 2 ** 32, t).to(torch.int32)
        return words.to(like.device) if _is_device_tensor(like) else words.cpu().numpy().view(np.uint32)
    a = np.asarray(labels).reshape(-1)
    if a.dtype.kind not in "iu":
        raise ValueError("labels must be an integer array")
    if a.shape[0] != M:
        raise ValueError(f"labels have {a.shape[0]} entries for {M} points")
    if a.dtype != np.uint32:
        if M and (int(a.min()) < 0 or int(a.max()) > 0xFFFFFFFF):
            raise ValueError("a label word does not fit uint32")
        a = a.astype(np.uint32)
    a = np.ascontiguousarray(a)
    if _is_device_tensor(like):
        import torch
        return torch.as_tensor(a.view(np.int32), device=like.device)
    return a


def _ground_flags(ground, off, like):
    """One byte per input point, non-zero = ground, from per-scan boolean masks or per-scan index lists (which index the INPUT
    scan: a duplicate or out-of-range index is a ValueError), or from one (M,) mask."""
    M = int(off[-1])
    if _is_device_tensor(ground):
        import torch
        if ground.reshape(-1).shape[0] != M:
            raise ValueError(f"ground has {ground.reshape(-1).shape[0]} entries for {M} points")
        flags = (ground.reshape(-1) != 0).to(torch.uint8).contiguous()
        return flags.to(like.device) if _is_device_tensor(like) else flags.cpu().numpy()
    if isinstance(ground, np.ndarray) and ground.dtype == np.bool_ and ground.ndim == 1:      # one mask for all scans
        if ground.shape[0] != M:
            raise ValueError(f"a ground mask for all scans must have {M} entries")
        ground = [ground[off[k]:off[k + 1]] for k in range(off.shape[0] - 1)]
    if len(ground) != off.shape[0] - 1:
        raise ValueError(f"{len(ground)} ground entries for {off.shape[0] - 1} scans")
    flags = np.zeros(M, dtype=np.uint8)
    for k, g in enumerate(ground):
        n = int(off[k + 1] - off[k])
        g = np.asarray(g.cpu() if _is_device_tensor(g) else g).reshape(-1)
        view = flags[off[k]:off[k + 1]]
        if g.dtype == np.bool_:
            if g.shape[0] != n:
                raise ValueError(f"the ground mask of scan {k} has {g.shape[0]} entries for {n} points")
            view[g] = 1
        else:
            if g.size and g.dtype.kind not in "iu":
                raise ValueError(f"the ground entry of scan {k} must be a boolean mask or an integer index array")
            g = g.astype(np.int64)
            if g.size and (int(g.min()) < 0 or int(g.max()) >= n):
                raise ValueError(f"a ground index of scan {k} is outside [0, {n})")
            if np.unique(g).shape[0] != g.shape[0]:
                raise ValueError(f"the ground indices of scan {k} hold a duplicate")
            view[g] = 1
    if _is_device_tensor(like):
        import torch
        return torch.as_tensor(flags, device=like.device)
    return flags


def _widen_words(a):
    """uint32 bits held in an int32 device tensor -> int64 values: one cast where torch casts uint32, else a cast and a mask."""
    import torch
    if hasattr(torch, "uint32"):
        try:
            return a.view(torch.uint32).to(torch.int64)
        except (RuntimeError, TypeError):   # a build whose uint32 has no cast on this device
            pass
    return a.to(torch.int64) & 0xFFFFFFFF


def _range_args(range_min, range_max):
    """(range_min, range_max) as the C entries take them: (0, -1) switches the range filter off."""
    if range_min is None and range_max is None:
        return 0.0, -1.0
    rmin = 0.0 if range_min is None else float(range_min)
    rmax = float("inf") if range_max is None else float(range_max)
    if rmax < 0.0:
        raise ValueError("range_max must not be negative")
    return rmin, rmax


GROUND_OPTIONS = ("distance_threshold", "num_iterations", "seed", "scan_base")


def _ground_planes(ctx, xyz, off, words, moving_index, rmin, rmax, distance_threshold=0.4, num_iterations=2000, seed=0, scan_base=0,
                   return_counts=False):
    """``ai_ground_planes`` on prepared buffers: (flags uint8 (M,), planes, best_hyp, best_count, counts or None), where `xyz`
    lives."""
    n_scans, M = off.shape[0] - 1, int(xyz.shape[0])
    n_hyp = int(num_iterations)
    place = place_of(xyz)
    flags, planes = place.new(max(M, 1), np.uint8), place.new((max(n_scans, 1), 4), np.float64)
    best_hyp, best_count = place.new(max(n_scans, 1), np.int32), place.new(max(n_scans, 1), np.int32)
    counts = place.new((max(n_scans, 1), max(min(n_hyp, 4096), 1)), np.int32) if return_counts else None
    place.sync()
    _ffi.check(_ffi.load().ai_ground_planes(
        ctx._h, place.addr(xyz), off.ctypes.data, n_scans, place.addr(words), -1 if moving_index is None else int(moving_index), rmin, rmax,
        float(distance_threshold), n_hyp, int(seed) & 0xFFFFFFFFFFFFFFFF, int(scan_base), place.mem, place.addr(flags), place.addr(planes),
        place.addr(best_hyp), place.addr(best_count), place.addr(counts)), "ai_ground_planes")
    return flags[:M], planes[:n_scans], best_hyp[:n_scans], best_count[:n_scans], (counts[:n_scans] if return_counts else None)


def ground_planes(scan_points, *, labels=None, moving_index=None, range_min=None, range_max=None, distance_threshold=0.4,
                  num_iterations=2000, seed=0, scan_base=0, scan_offsets=None, return_counts=False, ctx: Context | None = None):
    """The ground / non-ground split of every scan in one device call (``ai_ground_planes``, rules G1-G7 in
    ``include/autoinst_hip.h``): one RANSAC plane per scan, the ``segment_plane(distance_threshold=0.4, ransac_n=3,
    num_iterations=2000)`` branch of ``aggregate_pointcloud`` (``aggregate_pointcloud.py:115-123``) with a counter-based sampler,
    so that the result is a function of ``(points, seed, scan_base + scan index)`` alone.

    ``scan_points``, ``labels``, ``moving_index``, ``range_min`` / ``range_max`` and ``scan_offsets`` are those of
    `aggregate_scans`: a filtered point takes no part (never sampled, counted or flagged).  ``num_iterations`` (1 .. 4096) is the
    number of hypotheses; every one is scored on all kept points, and the plane with the most inliers (``dist <
    distance_threshold``, strict) wins, ties to the smallest hypothesis index.  There is no early exit and no refit.

    Returns ``(flags, planes, best_hyp, best_count)``: ``flags`` one ``(M,)`` boolean array over the INPUT points (it goes
    unchanged into ``aggregate_scans(ground=flags)``), ``planes`` ``(n_scans, 4)`` float64 ``(a, b, c, d)`` with a unit normal
    (zeros for a scan without a plane: fewer than 3 kept points, or only degenerate samples), ``best_hyp`` int32 (-1 without a
    plane) and ``best_count`` int32.  With ``return_counts`` also the ``(n_scans, num_iterations)`` int32 inlier counts of every
    hypothesis (-1 for a degenerate one).  Device points give device tensors."""
    ctx = ctx or default_context()
    xyz, off = _scan_points(scan_points, scan_offsets)
    words = _label_words(labels, off, xyz) if labels is not None else None
    rmin, rmax = _range_args(range_min, range_max)
    flags, planes, best_hyp, best_count, counts = _ground_planes(
        ctx, xyz, off, words, moving_index, rmin, rmax, distance_threshold, num_iterations, seed, scan_base, return_counts)
    out = (flags.view(place_of(flags).dtype(np.bool_)), planes, best_hyp, best_count)
    return out + (counts,) if return_counts else out


def aggregate_scans(scan_points, poses, *, labels=None, ground=None, moving_index=None, range_min=None, range_max=None,
                    return_source=False, scan_offsets=None, ground_options=None, ctx: Context | None = None):
    """All scans of a map to the two aggregated raw clouds in one device call (``ai_aggregate_scans``): the loop of
    ``aggregate_pointcloud`` (``aggregate_pointcloud.py:99-186``) with the dataset's filters (``kitti_gt_mo_filter.py:40-51``,
    ``range_filter.py:23-36``) and label decodes (``kitti_odometry_dataset.py:73-104``).

    ``scan_points``: a list of float32 ``(n_s, 3)`` or ``(n_s, 4)`` arrays in their sensor frames, as
    ``dataset.get_point_cloud`` returns them (column 3, the intensity, is ignored), or one float32 ``(M, 3)`` array / device
    tensor with ``scan_offsets=`` (``n_scans + 1`` entries).  ``poses``: ``(n_scans, 4, 4)``, last rows exactly ``0 0 0 1``.
    ``labels``: the raw ``.label`` words, in the same forms, uint32 or any integer dtype whose values fit.  ``ground``: per-scan
    boolean masks or per-scan index arrays into the INPUT scan (what Patchwork++'s ``getGroundIndices`` returns), one ``(M,)``
    mask, ``None`` (every kept point is non-ground), or ``"ransac"``: the flags of `ground_planes` with this call's own filter
    arguments and ``ground_options`` (``distance_threshold``, ``num_iterations``, ``seed``, ``scan_base``), which stay where the
    points are -- with device points nothing crosses to the host between the two device calls.  ``moving_index`` (the
    reference's 251) keeps a point iff ``(word & 0xFFFF) < moving_index``; ``range_min`` / ``range_max`` keep it iff its float32 norm lies in ``[range_min, range_max]``, both ends
    inclusive; ``None`` switches a filter off (``range_min`` alone defaults the other end to 0 / infinity).

    Returns ``(pcd_ground, pcd_nonground, labels_dict)``: float64 ``(n, 3)`` clouds in the map frame, each in ascending input
    position, and (when ``labels`` is given) ``seg_*``, ``instance_*``, ``panoptic_*`` for ``ground`` and ``nonground`` as
    ``(n,)`` arrays -- ``np.uint32`` on the host; int64 tensors holding the same values on the device (torch's uint32 cannot
    index).  ``instance`` is the reference's ``(word & 0xFFFF0000) * (word & 0xFFFF + 10)``, i.e. the mask 0x10009 and a product
    modulo 2^32.  With ``return_source`` also ``source_ground`` / ``source_nonground`` (int64: the input position of every output
    point) and ``offsets_ground`` / ``offsets_nonground`` (host int64, ``n_scans + 1``: where each scan's run starts).  Device
    points give device outputs; the result goes unchanged into ``downsample_map(pcd_nonground, pcd_ground, labels_dict)``.

    `scan_calibration_stays_on_host`: the vertical-angle correction of ``_correct_scan_calibration``
    (``kitti_odometry_dataset.py:306-335``) is NOT part of this call.  Its float32 result depends on NumPy's scalar promotion
    rules (which differ between NumPy 1.24 and 2.x) and on ``einsum``'s summation order, and ``get_point_cloud`` caches it
    anyway: pass the scans as the dataset returns them."""
    ctx = ctx or default_context()
    xyz, off = _scan_points(scan_points, scan_offsets)
    n_scans, M = off.shape[0] - 1, int(xyz.shape[0])
    T = np.ascontiguousarray(np.asarray(poses, dtype=np.float64).reshape(-1, 16))
    if T.shape[0] != n_scans:
        raise ValueError(f"{T.shape[0]} poses for {n_scans} scans")
    words = _label_words(labels, off, xyz) if labels is not None else None
    rmin, rmax = _range_args(range_min, range_max)
    if isinstance(ground, str):
        if ground != "ransac":
            raise ValueError('ground must be None, per-scan masks or index lists, one mask, or "ransac"')
        opts = dict(ground_options or {})
        unknown = sorted(set(opts) - set(GROUND_OPTIONS))
        if unknown:
            raise ValueError(f"ground_options has no {unknown}: the options are {list(GROUND_OPTIONS)}")
        flags = _ground_planes(ctx, xyz, off, words, moving_index, rmin, rmax, **opts)[0]   # stays where the points are
    else:
        if ground_options is not None:
            raise ValueError('ground_options goes with ground="ransac"')
        flags = _ground_flags(ground, off, xyz) if ground is not None else None
    place = place_of(xyz)
    cap = max(M, 1)
    out = {c: place.new((cap, 3), np.float64) for c in ("ground", "nonground")}
    lab = {f"{k}_{c}": (place.new(cap, np.uint32) if words is not None else None) for k in AGGREGATE_LABEL_KINDS for c in ("ground", "nonground")}
    src = {c: (place.new(cap, np.int32) if return_source else None) for c in ("ground", "nonground")}
    class_off = np.zeros(2 * (n_scans + 1), dtype=np.int64)
    ng, nn = C.c_int64(0), C.c_int64(0)
    place.sync()
    _ffi.check(_ffi.load().ai_aggregate_scans(
        ctx._h, place.addr(xyz), off.ctypes.data, n_scans, T.ctypes.data, place.addr(words), place.addr(flags),
        -1 if moving_index is None else int(moving_index), rmin, rmax, place.mem, place.addr(out["ground"]), place.addr(out["nonground"]),
        place.addr(lab["seg_ground"]), place.addr(lab["seg_nonground"]), place.addr(lab["instance_ground"]),
        place.addr(lab["instance_nonground"]), place.addr(lab["panoptic_ground"]), place.addr(lab["panoptic_nonground"]),
        place.addr(src["ground"]), place.addr(src["nonground"]), class_off.ctypes.data, C.byref(ng), C.byref(nn)), "ai_aggregate_scans")
    count = {"ground": ng.value, "nonground": nn.value}
    labels_dict = {}
    for key, a in lab.items():
        if a is not None:
            a = a[:count[key.split("_")[1]]]
            labels_dict[key] = _widen_words(a) if place.device is not None else a
    if return_source:
        for i, c in enumerate(("ground", "nonground")):
            labels_dict[f"source_{c}"] = place.index64(src[c][:count[c]])
            labels_dict[f"offsets_{c}"] = class_off[i * (n_scans + 1):(i + 1) * (n_scans + 1)].copy()
    return out["ground"][:ng.value], out["nonground"][:nn.value], labels_dict


def _patchwork_segmenter():
    try:
        import pypatchworkpp
    except ImportError as e:
        raise ImportError('ground_segmentation="patchwork" needs the pypatchworkpp module (Patchwork++ is an external C++ library that '
                          "is not part of this package): install it, or pass a callable (points, intensity) -> ground indices") from e
    params = pypatchworkpp.Parameters()
    params.verbose = False
    model = pypatchworkpp.patchworkpp(params)

    def segment(points, intensity):
        model.estimateGround(np.hstack((points, np.asarray(intensity).reshape(-1, 1))))
        return model.getGroundIndices()
    return segment


def aggregate_pointcloud(dataset, ind_start, ind_end, ground_segmentation=None, icp=False, *, ground_options=None,
                         ctx: Context | None = None):
    """Drop-in for ``aggregate_pointcloud`` (``aggregate_pointcloud.py:12``): reads ``dataset[i]`` (already filtered by the
    dataset's own chain) and ``dataset.get_pose(i)`` for ``ind_start <= i < ind_end`` and makes ONE `aggregate_scans` call with
    the filters off.  ``ground_segmentation``: ``None``; a callable ``(points (n, 3), intensity (n,)) -> ground indices``;
    ``"patchwork"``, which imports ``pypatchworkpp`` (``ImportError`` when it is missing); or ``"ransac"``: one seeded RANSAC
    plane per scan on the device (`ground_planes`, options in ``ground_options``), scan key = the position in the range.
    Returns the reference's ``(map_pcd_ground, map_pcd_nonground, poses, world_pose, labels)`` with ``(n, 3)`` float64 arrays for the clouds and, per
    key of ``labels``, the ``(n, 1)`` column that ``np.vstack`` makes of the reference's per-scan lists
    (``dataset_utils.py:193-196``); with ``ground_segmentation=None`` the 2-tuple ``(map_pcd, poses)``.

    ``"open3d"`` raises ``NotImplementedError``: its plane comes from open3d's RANSAC with an unseeded random generator, so there
    is nothing to reproduce; ``"ransac"`` is the same search with a seeded sampler.  ``icp=True`` raises too: ICP registration
    is not ported.  The scan calibration correction stays on the host, inside the dataset (see `aggregate_scans`)."""
    if icp:
        raise NotImplementedError("icp=True: ICP registration (open3d registration_icp against the growing map) is not ported")
    if isinstance(ground_segmentation, str):
        if ground_segmentation == "open3d":
            raise NotImplementedError('ground_segmentation="open3d" is a RANSAC plane from an unseeded random generator: '
                                      'it has no reproducible result to port (ground_segmentation="ransac" is the seeded one)')
        if ground_segmentation not in ("patchwork", "ransac"):
            raise ValueError('ground_segmentation must be None, "patchwork", "ransac", "open3d" or a callable')
        if ground_segmentation == "patchwork":
            ground_segmentation = _patchwork_segmenter()
    ransac = ground_segmentation == "ransac"
    if ground_options is not None and not ransac:
        raise ValueError('ground_options goes with ground_segmentation="ransac"')
    scans, poses, ground = [], [], []
    cols = {k: [] for k in AGGREGATE_LABEL_KINDS}
    for i in range(ind_start, ind_end):
        entry = dataset[i]
        p = np.asarray(entry.point_cloud)[:, :3]
        p32 = np.ascontiguousarray(p, dtype=np.float32)
        if p.dtype != np.float32 and not np.array_equal(p32, p):
            raise ValueError(f"the point cloud of entry {i} is not float32 (dataset.get_point_cloud returns float32)")
        scans.append(p32)
        poses.append(np.asarray(dataset.get_pose(i), dtype=np.float64))
        if ground_segmentation is not None:
            if not ransac:
                ground.append(np.asarray(ground_segmentation(p32, np.asarray(entry.intensity).reshape(-1))).reshape(-1))
            for kind, attr in (("seg", "semantic_labels"), ("instance", "instance_labels"), ("panoptic", "panoptic_labels")):
                cols[kind].append(np.asarray(getattr(entry, attr)).reshape(-1, 1))
    stacked = np.stack(poses) if poses else np.zeros((0, 4, 4))
    if ground_segmentation is None:
        _, map_pcd, _ = aggregate_scans(scans, stacked, ctx=ctx)
        return map_pcd, poses
    g, ng, info = aggregate_scans(scans, stacked, ground="ransac" if ransac else ground, ground_options=ground_options,
                                  return_source=True, ctx=ctx)
    labels = {}
    for kind in AGGREGATE_LABEL_KINDS:
        col = np.vstack(cols[kind]) if cols[kind] else np.zeros((0, 1), dtype=np.uint32)
        for cloud in ("ground", "nonground"):
            labels[f"{kind}_{cloud}"] = col[info[f"source_{cloud}"]]
    return g, ng, poses, np.eye(4), labels
