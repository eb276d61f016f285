"""Host-side mirror of the two point-cloud steps around the NCuts hot path.

* `tarl_pool` -- the radius-mean pooling loop of ``tarl_features_per_patch``
  (``pipeline/utils/point_cloud/chunk_generation.py:243-256``);
* `nn1_reproject` -- ``kDTree_1NN_feature_reprojection``
  (``pipeline/utils/point_cloud/point_cloud_utils.py:144-174``).
* `tarl_pool_map` / `tarl_features_per_map` -- the same pooling for every chunk of a map in one device call
  (``ai_scan_pool``, ``csrc/ai_scanpool.hip``): the pose transform, the crop to each chunk's box, the choice of each
  chunk's scans and the radius mean (``chunk_generation.py:221-256``), with every scan read and uploaded once.
* `finish_chunks` / `finish_map` / `get_corrected_ground` -- the tail of ``ncuts_chunk`` (``pipeline/ncuts/ncuts_utils.py:
  177-204``) and ``get_corrected_ground`` (``point_cloud_utils.py:331-342``) for every chunk of a map in one device call
  (``ai_chunk_finish``, ``csrc/ai_finish.hip``): the group of every fine point, the corrected ground and the merged chunk
  that `labels_api.merge_chunks_unite_instances2` takes.
All run as HIP kernels over cell lists; there is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _ffi
from .config import ADJACENT_FRAMES_TARL, CHUNK_SIZE, MAJOR_VOXEL_SIZE, MEAN_HEIGHT, NUM_TARL_FEATURES, TARL_NORM
from ._buffers import cat_int32, concat, place_of, segmented
from .ncuts_api import Context, _is_device_tensor, default_context


def tarl_pool(points_major, tarl_points, tarl_features, *, radius=MAJOR_VOXEL_SIZE / 2.0, return_count=False,
              ctx: Context | None = None):
    """(N, F) float64: mean TARL feature within `radius` of every major-voxel point, zero row if none.

    ``tarl_points`` (M, 3) are the concatenated, already transformed and cropped scan points and
    ``tarl_features`` (M, F) their float32 features (``chunk_generation.py:218-241`` stay in Python:
    they are dataset I/O).  A scan point is in the mean iff ``(dx*dx + dy*dy) + dz*dz``, each step
    rounded, is strictly below ``radius * radius``: open3d's (nanoflann's) radius search.  With
    ``return_count`` also the (N,) int32 number of scan points in each mean.
    """
    ctx = ctx or default_context()
    q = np.ascontiguousarray(points_major, dtype=np.float64)
    s = np.ascontiguousarray(tarl_points, dtype=np.float64)
    f = np.ascontiguousarray(tarl_features, dtype=np.float32)
    if q.ndim != 2 or q.shape[1] != 3 or s.ndim != 2 or s.shape[1] != 3 or f.ndim != 2 or f.shape[0] != s.shape[0]:
        raise ValueError("points must be (N, 3) / (M, 3) and features (M, F)")
    out = np.zeros((q.shape[0], f.shape[1]), dtype=np.float64)
    cnt = np.zeros(q.shape[0], dtype=np.int32)
    if s.shape[0] == 0:
        return (out, cnt) if return_count else out  # tarl_features stays all-zero in the reference too
    _ffi.check(_ffi.load().ai_radius_mean_pool(ctx._h, q.ctypes.data, q.shape[0], s.ctypes.data, s.shape[0], f.ctypes.data,
                                               f.shape[1], float(radius), _ffi.AI_MEM_HOST, out.ctypes.data, cnt.ctypes.data),
               "ai_radius_mean_pool")
    return (out, cnt) if return_count else out


def _transform_points(points, T):
    """open3d ``PointCloud.transform``: homogeneous 4x4 applied to every point, divided by w."""
    # a matrix product: rounds differently from `camera_api.transform_points` (fixed order) on purpose, the two stay two functions
    p = np.asarray(points, dtype=np.float64)
    T = np.asarray(T, dtype=np.float64)
    q = p @ T[:3, :3].T + T[:3, 3]
    w = p @ T[3, :3] + T[3, 3]
    return q / w[:, None]


def tarl_features_per_patch(dataset, pcd, T_pcd, center_position, tarl_indices, *, chunk_size=CHUNK_SIZE,
                            major_voxel_size=MAJOR_VOXEL_SIZE, tarl_norm=TARL_NORM, transform_pcd=None,
                            ctx: Context | None = None):
    """Drop-in for ``tarl_features_per_patch`` (``chunk_generation.py:205-258``, same five positional
    arguments): the scan loop (:222-241, dataset reads, pose transform, crop to the chunk box) stays
    on the host, the per-point radius search and mean (:243-256) run on the device.  ``dataset`` needs
    ``get_tarl_features`` / ``get_point_cloud`` / ``get_pose`` like the reference's; ``pcd`` needs
    ``.points``.  ``transform_pcd`` may be the reference's own function (open3d); the default applies
    the same homogeneous transform in NumPy.
    """
    tf = transform_pcd or _transform_points
    center_position = np.asarray(center_position, dtype=np.float64)
    max_position = center_position + 0.5 * np.asarray(chunk_size, dtype=np.float64)            # :219-220
    min_position = center_position - 0.5 * np.asarray(chunk_size, dtype=np.float64)
    pts_list, feat_list = [], []
    for points_index in tarl_indices:                                                            # :222
        tarl_features = np.asarray(dataset.get_tarl_features(points_index))
        coords = np.asarray(dataset.get_point_cloud(points_index))
        T_local2global = np.linalg.inv(T_pcd) @ dataset.get_pose(points_index)                   # :229-231
        coords = np.asarray(tf(coords, T_local2global))
        mask = np.where(np.all(coords > min_position, axis=1) & np.all(coords < max_position, axis=1))[0]   # :233-236
        pts_list.append(coords[mask])
        feat_list.append(np.asarray(tarl_features[mask], dtype=np.float32))
    points_major = np.asarray(pcd.points)
    if not pts_list:
        return np.zeros((points_major.shape[0], 96))                                              # :246 with no scan at all
    out = tarl_pool(points_major, np.concatenate(pts_list), np.concatenate(feat_list),
                    radius=major_voxel_size / 2.0, ctx=ctx)                                       # :243-252
    if tarl_norm:                                                                                # :253-254
        nrm = np.linalg.norm(out, axis=1)
        has = out.any(axis=1)
        out[has] /= nrm[has, None]
    return out


def tarl_pool_map(scan_points, scan_features, T_scan2pcd, chunk_points, boxes, scan_windows, *, radius=MAJOR_VOXEL_SIZE / 2.0,
                  return_count=False, scan_offsets=None, chunk_offsets=None, ctx: Context | None = None):
    """The TARL matrix of every chunk of a map in one device call (``ai_scan_pool``): a list with one (N_c, F) float64 array
    per chunk, what `tarl_pool` gives for the chunk's transformed and cropped scans.

    ``scan_points`` / ``scan_features``: one (n_s, 3) float64 and one (n_s, F) float32 array per sampled scan, each scan in its
    own sensor frame -- or the concatenated arrays with ``scan_offsets`` (S + 1).  ``T_scan2pcd``: S 4x4 transforms to the pcd
    frame (last row 0 0 0 1), applied in the fixed order of `camera_api.transform_points`.  ``chunk_points``: one (N_c, 3)
    array of major-voxel points per chunk -- or the concatenated array with ``chunk_offsets`` (C + 1).  ``boxes``: (C, 6) or
    (C, 2, 3), lo and hi of each chunk's crop.  ``scan_windows``: (C, 2), chunk c takes the scans at positions
    ``first <= s < last`` of the scan list.

    Scan point p of scan s is in the mean of a point q of chunk c iff s is in c's window, the transformed p lies strictly
    inside c's box, and ``(dx*dx + dy*dy) + dz*dz < radius * radius`` (`tarl_pool`'s test).  The members are summed in float64
    in an order that depends on their coordinates alone, so a chunk's rows are bit-identical whichever other chunks or scans
    the call holds.  With float64 / float32 torch tensors on the context's GPU the inputs are used in place and the outputs are
    device tensors, which `ncuts_api.build_affinity` and `sharding.run_chunks` take as they are.  With ``return_count`` also
    the list of (N_c,) int32 member counts.
    """
    ctx = ctx or default_context()
    first = scan_points if scan_offsets is not None else next(iter(scan_points), None)
    qfirst = chunk_points if chunk_offsets is not None else next(iter(chunk_points), None)
    place = place_of(first if first is not None else qfirst)
    xyz, soff = segmented(scan_points, scan_offsets, 3, np.float64, "scan_points", place)
    feat, foff = segmented(scan_features, scan_offsets, None, np.float32, "scan_features", place)
    q, qoff = segmented(chunk_points, chunk_offsets, 3, np.float64, "chunk_points", place)
    if not np.array_equal(soff, foff) or int(feat.shape[0]) != int(xyz.shape[0]):
        raise ValueError("scan_features: one feature row per scan point expected")
    dim = int(feat.shape[1])
    if int(xyz.shape[0]) == 0 and dim == 0:
        dim = NUM_TARL_FEATURES   # no scan at all, so no width either: the reference's tarl_features stay np.zeros((N, 96))
    n_scans, n_chunks = soff.size - 1, qoff.size - 1
    if n_scans < 0 or n_chunks < 0:
        raise ValueError("offsets must hold at least one entry")
    if int(xyz.shape[0]) != (int(soff[-1]) if n_scans >= 0 else 0) or int(q.shape[0]) != int(qoff[-1]):
        raise ValueError("the last offset must be the number of rows")
    T = np.ascontiguousarray(np.asarray(T_scan2pcd, dtype=np.float64).reshape(-1, 16))
    b = np.ascontiguousarray(np.asarray(boxes, dtype=np.float64).reshape(-1, 6))
    w = np.asarray(scan_windows).reshape(-1, 2)
    if T.shape[0] != n_scans or b.shape[0] != n_chunks or w.shape[0] != n_chunks:
        raise ValueError(f"{n_scans} transforms, {n_chunks} boxes and {n_chunks} windows expected, got {T.shape[0]}, {b.shape[0]}, "
                         f"{w.shape[0]}")
    if w.size and (w.min() < -2 ** 31 or w.max() >= 2 ** 31):
        raise ValueError("scan_windows do not fit int32")
    w = np.ascontiguousarray(w.astype(np.int32))
    nq = int(q.shape[0])
    out, cnt = place.new((nq, dim), np.float64), place.new((nq,), np.int32)
    place.sync()
    _ffi.check(_ffi.load().ai_scan_pool(   # this entry takes NULL for every buffer without elements, the outputs included
        ctx._h, place.addr_or_null(xyz), soff.ctypes.data, n_scans, T.ctypes.data, place.addr_or_null(feat), dim, place.addr_or_null(q),
        qoff.ctypes.data, n_chunks, b.ctypes.data, w.ctypes.data, float(radius), place.mem, place.addr_or_null(out),
        place.addr_or_null(cnt)), "ai_scan_pool")
    rows = [out[qoff[c]:qoff[c + 1]] for c in range(n_chunks)]
    if return_count:
        return rows, [cnt[qoff[c]:qoff[c + 1]] for c in range(n_chunks)]
    return rows


def tarl_window(sampled_indices_global, center_id, adjacent_frames=ADJACENT_FRAMES_TARL):
    """[first, last) positions in ``sampled_indices_global`` of the scans the reference pools for a chunk whose centre scan is
    ``center_id``: the slice of ``get_indices_feature_reprojection`` (``chunk_generation.py:261-271``)."""
    idx = list(sampled_indices_global)
    i = idx.index(center_id)
    return max(0, i - adjacent_frames[0]), max(0, min(len(idx), i + adjacent_frames[1]))


def tarl_features_per_map(dataset, chunk_downsample_dict, T_pcd, sampled_indices_global, *, adjacent_frames=ADJACENT_FRAMES_TARL,
                          chunk_size=CHUNK_SIZE, major_voxel_size=MAJOR_VOXEL_SIZE, tarl_norm=TARL_NORM,
                          ctx: Context | None = None):
    """The TARL matrices of all chunks of a map: the list of what ``ncuts_chunk`` (``ncuts_utils.py:40-49, 136-142``) computes
    chunk by chunk with ``tarl_features_per_patch``, from one `tarl_pool_map` call.

    ``chunk_downsample_dict`` needs ``center_ids``, ``center_positions`` and ``pcd_nonground_chunks_major_downsampling``
    (arrays or objects with ``.points``).  Chunk c pools the scans of `tarl_window` around ``center_ids[c]``; every scan in the
    union of the windows is read once (``get_tarl_features``, ``get_point_cloud``, ``get_pose``), with ``T = inv(T_pcd) @
    pose`` applied in the fixed order of `camera_api.transform_points`.  ``ai_scan_pool`` takes affine transforms only, and a
    floating-point inverse and product need not return the last row 0 0 0 1 exactly: a last row within rounding of it (64 ulps
    of the largest entry of T) is set to it, anything further off raises ``ValueError`` here, naming the scan.
    """
    idx = list(sampled_indices_global)
    centers = np.asarray(chunk_downsample_dict["center_positions"], dtype=np.float64).reshape(-1, 3)
    chunks = []
    for pc in chunk_downsample_dict["pcd_nonground_chunks_major_downsampling"]:
        chunks.append(np.asarray(pc.points if hasattr(pc, "points") and not isinstance(pc, np.ndarray) else pc, dtype=np.float64))
    wins = np.array([tarl_window(idx, cid, adjacent_frames) for cid in chunk_downsample_dict["center_ids"]],
                    dtype=np.int64).reshape(-1, 2)
    used = np.zeros(len(idx) + 1, dtype=np.int64)
    for a, b in wins:
        used[a:b] = 1
    rank = np.concatenate([[0], np.cumsum(used)])   # position in the list of sampled scans -> position among the scans read
    pts, feats, Ts = [], [], []
    T_inv = np.linalg.inv(np.asarray(T_pcd, dtype=np.float64))
    for pos in np.flatnonzero(used):
        points_index = idx[pos]
        feats.append(np.asarray(dataset.get_tarl_features(points_index), dtype=np.float32))
        pts.append(np.asarray(dataset.get_point_cloud(points_index), dtype=np.float64))
        T = T_inv @ np.asarray(dataset.get_pose(points_index), dtype=np.float64)                 # :229-231
        if np.abs(T[3] - [0.0, 0.0, 0.0, 1.0]).max() > 64 * np.finfo(np.float64).eps * max(1.0, np.abs(T[:3]).max()):
            raise ValueError(f"tarl_features_per_map: inv(T_pcd) @ pose of scan {points_index} is not affine (last row {T[3]})")
        T[3] = [0.0, 0.0, 0.0, 1.0]
        Ts.append(T)
    half = 0.5 * np.asarray(chunk_size, dtype=np.float64)
    boxes = np.concatenate([centers - half, centers + half], axis=1)                             # :219-220
    out = tarl_pool_map(pts, feats, np.array(Ts).reshape(-1, 4, 4), chunks, boxes, rank[wins], radius=major_voxel_size / 2.0, ctx=ctx)
    if tarl_norm:                                                                                # :253-254
        for o in out:
            nrm = np.linalg.norm(o, axis=1)
            has = o.any(axis=1)
            o[has] /= nrm[has, None]
    return out


def nn1_index(points_to, points_from, *, ctx: Context | None = None):
    """(index[Nt] int32, distance[Nt] float64) of the nearest `points_from` row for every `points_to` row.

    A NaN or infinite coordinate in ``points_to`` raises ``ValueError``: ``ai_nn1_project`` answers such a row with index -1,
    which as a NumPy index would silently mean the last source."""
    ctx = ctx or default_context()
    t = np.ascontiguousarray(points_to, dtype=np.float64)
    f = np.ascontiguousarray(points_from, dtype=np.float64)
    if not np.isfinite(t).all():
        raise ValueError("nn1_index: points_to has NaN or infinite coordinates, which have no nearest point")
    idx = np.empty(t.shape[0], dtype=np.int32)
    dist = np.empty(t.shape[0], dtype=np.float64)
    _ffi.check(_ffi.load().ai_nn1_project(ctx._h, t.ctypes.data, t.shape[0], f.ctypes.data, f.shape[0], _ffi.AI_MEM_HOST,
                                          idx.ctypes.data, dist.ctypes.data), "ai_nn1_project")
    return idx, dist


def nn1_reproject(features_to, points_to, features_from, points_from, max_radius=None, no_feature_label=(1, 0, 0), *,
                  ctx: Context | None = None):
    """Drop-in arithmetic of ``kDTree_1NN_feature_reprojection`` on arrays (no open3d objects)."""
    features_to = np.array(features_to, copy=True)
    if not np.isfinite(np.asarray(points_to, dtype=np.float64)).all():
        raise ValueError("nn1_reproject: points_to has NaN or infinite coordinates, no feature can be re-projected onto them")
    idx, dist = nn1_index(points_to, points_from, ctx=ctx)
    features_to[:] = np.asarray(features_from)[idx]
    if max_radius is not None:
        features_to[dist > max_radius] = np.asarray(no_feature_label, dtype=features_to.dtype)
    return features_to


FINISH_STATS = ("mean", "std", "threshold", "n_inliers", "mean_z", "z_limit")   # ai_chunk_finish's ground_stats, per chunk


def finish_chunks(fine, major, major_labels, ground, *, nb_neighbors=20, std_ratio=2.0, mean_height=MEAN_HEIGHT,
                  return_stats=False, ctx: Context | None = None):
    """The tail of ``ncuts_chunk`` (``ncuts_utils.py:185-199``) for all chunks of a map in one device call
    (``ai_chunk_finish``, rules F1-F7 in ``include/autoinst_hip.h``).

    ``fine``, ``major``, ``ground``: one (n, 3) float64 array or device tensor per chunk -- the minor non-ground chunk points
    (``pcd_nonground_chunks``), the major-voxel points the cut labelled and the ground chunk points (``pcd_ground_chunks``).
    ``major_labels``: one integer group id per major point and chunk (what `sharding.run_chunks` returns), or ``None``.

    Per chunk: every fine point takes the group of its nearest major point of the SAME chunk (smallest ``(dx*dx + dy*dy) +
    dz*dz``, ties to the smaller index); the ground loses open3d's statistical outliers (`prep_api.statistical_inlier_indices`'
    rules, bit for bit) and then every inlier with ``z >= mean z of the inliers + mean_height``.  Returns one dict per chunk:
    ``merged_points`` (the fine points, then the kept ground points in ascending order), ``merged_instance`` (int32: group + 1
    for a fine point, 0 for ground -- the merge's "no instance"), ``fine_instance`` (int32, the group of every fine point) and
    ``ground_keep`` (int64: the chunk-local indices the reference writes ``[inliers][in_idcs]``).  Without ``major_labels`` the
    first three are ``None``.  With ``return_stats`` also ``fine_nn`` (int32, chunk-local), ``fine_dist``, ``ground_avg`` and
    ``stats`` (`FINISH_STATS`).  Device tensors in give device tensors out; only offsets, counts and the statistics cross to the
    host.  Errors of the list in the header raise ``ValueError``."""
    ctx = ctx or default_context()
    n = len(ground)
    if len(fine) != n or len(major) != n or (major_labels is not None and len(major_labels) != n):
        raise ValueError("fine, major, major_labels and ground must hold one entry per chunk")
    place = place_of(*fine, *major, *ground)
    f, foff = concat(list(fine), 3, np.float64, "fine", place)
    m, moff = concat(list(major), 3, np.float64, "major", place)
    g, goff = concat(list(ground), 3, np.float64, "ground", place)
    lab = None
    if major_labels is not None:
        parts = []
        for c, a in enumerate(major_labels):
            a = a.reshape(-1) if _is_device_tensor(a) else np.asarray(a).reshape(-1)
            if int(a.shape[0]) != int(moff[c + 1] - moff[c]):
                raise ValueError(f"major_labels[{c}] has {int(a.shape[0])} entries for {int(moff[c + 1] - moff[c])} major points")
            parts.append(a)
        lab = cat_int32(parts, place)
        if lab.shape[0] == 0:
            lab = place.new(1, np.int32)   # a call without major points: not NULL (NULL means "no labels"), never read
    nf, ng = int(foff[-1]), int(goff[-1])
    nn = place.new(max(nf, 1), np.int32) if return_stats else None
    dist = place.new(max(nf, 1), np.float64) if return_stats else None
    avg = place.new(max(ng, 1), np.float64) if return_stats else None
    keep = place.new(max(ng, 1), np.int32)
    flab = place.new(max(nf, 1), np.int32) if lab is not None else None
    mxyz = place.new((max(nf + ng, 1), 3), np.float64) if lab is not None else None
    mlab = place.new(max(nf + ng, 1), np.int32) if lab is not None else None
    koff = np.zeros(n + 1, dtype=np.int64)
    merged_off = np.zeros(n + 1, dtype=np.int64) if lab is not None else None
    stats = np.full((n, len(FINISH_STATS)), np.nan)
    # an empty input is NULL; an output is never NULL because it is empty: there NULL means "not wanted"
    place.sync()
    _ffi.check(_ffi.load().ai_chunk_finish(
        ctx._h, place.addr_or_null(f), foff.ctypes.data, place.addr_or_null(m), moff.ctypes.data, place.addr(lab), place.addr_or_null(g),
        goff.ctypes.data, n, int(nb_neighbors), float(std_ratio), float(mean_height), place.mem, place.addr(nn), place.addr(dist),
        place.addr(flab), place.addr(avg), place.addr(keep), koff.ctypes.data, stats.ctypes.data, place.addr(mxyz), place.addr(mlab),
        merged_off.ctypes.data if merged_off is not None else None), "ai_chunk_finish")
    res = []
    for c in range(n):
        k = keep[koff[c]:koff[c + 1]]
        d = {"merged_points": None, "merged_instance": None, "fine_instance": None,
             "ground_keep": place.index64(k)}
        if lab is not None:
            d["merged_points"] = mxyz[merged_off[c]:merged_off[c + 1]]
            d["merged_instance"] = mlab[merged_off[c]:merged_off[c + 1]]
            d["fine_instance"] = flab[foff[c]:foff[c + 1]]
        if return_stats:
            d["fine_nn"], d["fine_dist"] = nn[foff[c]:foff[c + 1]], dist[foff[c]:foff[c + 1]]
            d["ground_avg"] = avg[goff[c]:goff[c + 1]]
            d["stats"] = {k_: float(v) for k_, v in zip(FINISH_STATS, stats[c])}
        res.append(d)
    return res


def _chunk_points(a):
    """(n, 3) points of a dict entry: an array, a device tensor, or an object with ``.points`` (an open3d cloud)."""
    if not _is_device_tensor(a) and hasattr(a, "points") and not isinstance(a, np.ndarray):
        a = np.asarray(a.points)
    return a if _is_device_tensor(a) else np.asarray(a, dtype=np.float64).reshape(-1, 3)


def _index(a, idx):
    """a[idx] where `a` lives (`idx`: int64 array or tensor)."""
    if _is_device_tensor(a):
        import torch
        return a.reshape(-1).index_select(0, idx.to(a.device) if _is_device_tensor(idx) else torch.as_tensor(np.asarray(idx), device=a.device))
    return np.asarray(a).reshape(-1)[idx.cpu().numpy() if _is_device_tensor(idx) else idx]


def _host(a):
    return a.cpu().numpy() if _is_device_tensor(a) else np.asarray(a)


def finish_map(chunk_downsample_dict, labels, *, nb_neighbors=20, std_ratio=2.0, mean_height=MEAN_HEIGHT, color_seed=0,
               ctx: Context | None = None):
    """From the cut's labels to the merge's input for a whole map, without open3d: ``chunk_downsample_dict`` is the dict of
    `prep_api.chunk_and_downsample_point_clouds`, ``labels`` the list `sharding.run_chunks` returns for its
    ``pcd_nonground_chunks_major_downsampling``.  One `finish_chunks` call.

    Returns ``(chunks, pairs)``.  ``chunks[c]`` holds the five values ``ncuts_chunk`` returns (``ncuts_utils.py:204``) as arrays
    -- ``merged_chunk`` (points), ``pcd_chunk`` (the fine points), ``cut_hight`` (the kept ground points), ``inst_ground``,
    ``seg_ground`` (``kitti_labels["ground"][...][c][ground_keep]``; ``None`` without labels in the dict) -- plus
    ``merged_instance``, ``fine_instance`` and ``ground_keep``; device inputs give device tensors.  ``pairs[c]`` is the host
    ``(points, colours)`` pair `labels_api.merge_chunks_unite_instances2` takes: the instance as the colour
    (`formats.labels_to_colors`, seeded per chunk as the reference draws fresh colours per chunk; ground is black)."""
    from .formats import labels_to_colors
    fine = [_chunk_points(a) for a in chunk_downsample_dict["pcd_nonground_chunks"]]
    major = [_chunk_points(a) for a in chunk_downsample_dict["pcd_nonground_chunks_major_downsampling"]]
    ground = [_chunk_points(a) for a in chunk_downsample_dict["pcd_ground_chunks"]]
    done = finish_chunks(fine, major, labels, ground, nb_neighbors=nb_neighbors, std_ratio=std_ratio, mean_height=mean_height, ctx=ctx)
    kitti = (chunk_downsample_dict.get("kitti_labels") or {}).get("ground")
    chunks, pairs = [], []
    for c, d in enumerate(done):
        nf = int(fine[c].shape[0])
        out = {"merged_chunk": d["merged_points"], "pcd_chunk": d["merged_points"][:nf], "cut_hight": d["merged_points"][nf:],
               "inst_ground": None, "seg_ground": None, "merged_instance": d["merged_instance"],
               "fine_instance": d["fine_instance"], "ground_keep": d["ground_keep"]}
        if kitti is not None:
            out["inst_ground"] = _index(kitti["instance"][c], d["ground_keep"])                   # ncuts_utils.py:201-202
            out["seg_ground"] = _index(kitti["semantic"][c], d["ground_keep"])
        chunks.append(out)
        pairs.append((_host(d["merged_points"]), labels_to_colors(_host(d["merged_instance"]), seed=color_seed + c)))
    return chunks, pairs


def get_corrected_ground(chunk_downsample_dict, sequence, mean_height=MEAN_HEIGHT, *, ctx: Context | None = None):
    """Drop-in for ``get_corrected_ground`` (``point_cloud_utils.py:331-342``) on arrays: ``(input_pcd, inst_ground)``, the
    points of ``pcd_nonground_chunks[sequence]`` followed by the corrected ground of that chunk, and
    ``kitti_labels["ground"]["instance"][sequence]`` of the kept ground points.  A one-chunk `finish_chunks` call with no fine
    points."""
    ground = _chunk_points(chunk_downsample_dict["pcd_ground_chunks"][sequence])
    nonground = _chunk_points(chunk_downsample_dict["pcd_nonground_chunks"][sequence])
    if _is_device_tensor(ground):
        import torch
        empty = torch.zeros((0, 3), dtype=torch.float64, device=ground.device)
        cat = torch.cat
    else:
        empty = np.zeros((0, 3))
        cat = np.concatenate
    d = finish_chunks([empty], [empty], [np.zeros(0, dtype=np.int32)], [ground], mean_height=mean_height, ctx=ctx)[0]
    inst = chunk_downsample_dict["kitti_labels"]["ground"]["instance"][sequence]
    return cat([nonground, d["merged_points"]]), _index(inst, d["ground_keep"])
