"""CPU restatement of the chunk preparation (``chunk_and_downsample_point_clouds``, reference
``pipeline/dataset/dataset_utils.py:489-567``) that `autoinst_amd.prep_api` runs on the device.

open3d is not available, so this is a restatement of the rules open3d 0.17 is written with, not open3d itself:

* crop: NumPy ``np.all(p > lo) & np.all(p < hi)`` (``chunk_generation.py:134-137``);
* statistical outliers (``PointCloud::RemoveStatisticalOutliers``): a cKDTree kNN, the k distances summed sequentially in
  ascending order; ``mean`` over ALL points, ``std`` with n - 1, kept iff ``0 < avg < mean + std_ratio * std``;
* voxels (``PointCloud::VoxelDownSample``): ``floor((p - (min - v / 2)) / v)``, sums by ``np.add.at`` in input order, output in
  ascending ``(ix, iy, iz)``;
* the trajectory walk of ``chunks_from_pointcloud`` (``chunk_generation.py:120-170``).
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

CHUNK_SIZE = np.array([25.0, 25.0, 25.0])   # config.py:57
OVERLAP = 3                                  # config.py:58
MAJOR_VOXEL_SIZE = 0.35                      # config.py:56


def box_select(points, boxes):
    """Per box (lo, hi): ascending indices of the points strictly inside."""
    points = np.asarray(points, dtype=np.float64)
    return [np.where(np.all(points > np.asarray(lo), axis=1) & np.all(points < np.asarray(hi), axis=1))[0] for lo, hi in boxes]


def _sequential_mean(d, k):
    s = d[:, 0].copy()
    for j in range(1, k):
        s = s + d[:, j]
    return s / k


def knn_avg(points, nb_neighbors, workers=1):
    """avg[i]: the mean distance of the k = min(nb_neighbors, n) nearest points (i itself included), summed ascending."""
    points = np.asarray(points, dtype=np.float64)
    n = points.shape[0]
    k = min(int(nb_neighbors), n)
    d, _ = cKDTree(points).query(points, k=k, workers=workers)
    return _sequential_mean(np.asarray(d, dtype=np.float64).reshape(n, k), k)


def knn_avg_brute(points, nb_neighbors):
    """The same from the full distance matrix (small clouds only): np.partition, then an ascending sort of the k smallest."""
    points = np.asarray(points, dtype=np.float64)
    n = points.shape[0]
    k = min(int(nb_neighbors), n)
    D = np.sqrt(((points[:, None, :] - points[None, :, :]) ** 2).sum(-1))
    part = np.sort(np.partition(D, k - 1, axis=1)[:, :k], axis=1)
    return _sequential_mean(part, k)


def statistical_from_avg(avg, std_ratio):
    """(kept indices, mean, std, threshold) from the per-point averages, by open3d's rules."""
    n = avg.shape[0]
    pos = avg > 0
    mean = avg[pos].sum() / n
    with np.errstate(divide="ignore", invalid="ignore"):
        std = np.sqrt(((avg[pos] - mean) ** 2).sum() / (n - 1)) if n > 1 else np.float64(np.nan)
    thr = mean + std_ratio * std
    return np.where(pos & (avg < thr))[0], float(mean), float(std), float(thr)


def statistical_inliers(points, nb_neighbors=20, std_ratio=2.0, workers=1, brute=False):
    """(kept indices, avg, mean, std, threshold); raises ValueError on open3d's illegal parameters."""
    if nb_neighbors < 1 or std_ratio <= 0:
        raise ValueError("nb_neighbors and std_ratio must be positive")
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if points.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0), float("nan"), float("nan"), float("nan")
    avg = knn_avg_brute(points, nb_neighbors) if brute else knn_avg(points, nb_neighbors, workers)
    idx, mean, std, thr = statistical_from_avg(avg, std_ratio)
    return idx, avg, mean, std, thr


def voxel_down_sample(points, voxel_size):
    """(points, trace): voxel means in ascending (ix, iy, iz) order and every input point's output row."""
    points = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if points.shape[0] == 0:
        return np.zeros((0, 3)), np.zeros(0, np.int64)
    vmin = points.min(axis=0) - voxel_size * 0.5
    vox = np.floor((points - vmin) / voxel_size).astype(np.int64)
    _, inv = np.unique(vox, axis=0, return_inverse=True)
    inv = inv.reshape(-1)
    m = int(inv.max()) + 1
    out = np.zeros((m, 3))
    np.add.at(out, inv, points)
    cnt = np.bincount(inv, minlength=m).astype(np.float64)
    return out / cnt[:, None], inv


def chunk_centres(T_pcd, positions, first_position, indices):
    centres, ids = [], []
    distance, last = 0.0, None
    rot = np.linalg.inv(np.asarray(T_pcd)[:3, :3])
    for position, index in zip(positions, indices):
        if last is not None:
            distance += np.linalg.norm(position - last)
            if distance > (min(CHUNK_SIZE[0], CHUNK_SIZE[1]) - OVERLAP):
                centres.append(rot @ (position - first_position))
                ids.append(index)
                distance = 0
        last = position
    return centres, ids


def chunks_from_pointcloud(points, T_pcd, positions, first_position, indices, labels=None, ground=False, workers=1):
    points = np.asarray(points, dtype=np.float64)
    centres, centre_ids = chunk_centres(T_pcd, positions, first_position, indices)
    bounds = [(c - 0.5 * CHUNK_SIZE, c + 0.5 * CHUNK_SIZE) for c in centres]
    ids_all = box_select(points, bounds)
    kitti_out = {"panoptic": [], "semantic": [], "instance": []} if labels is not None else None
    chunks, inliers, avgs = [], [], []
    for ids in ids_all:
        crop = points[ids]
        inl, avg, *_ = statistical_inliers(crop, 20, 2.0, workers=workers)
        chunks.append(crop[inl])
        inliers.append(inl)
        avgs.append(avg)
        if kitti_out is not None:
            sk, ik = ("seg_ground", "instance_ground") if ground else ("seg_nonground", "instance_nonground")
            kitti_out["semantic"].append(labels[sk][ids][inl])
            kitti_out["instance"].append(labels[ik][ids][inl])
    return (chunks, ids_all, centres, centre_ids, bounds, kitti_out, [0] * len(centres)), inliers, avgs


def chunk_and_downsample_point_clouds(pcd_nonground_minor, pcd_ground_minor, T_pcd, positions, first_position,
                                      sampled_indices_global, kitti_labels=None, workers=1):
    """The reference's dict, plus ``_inliers`` / ``_avg`` (per cloud, per chunk) for tolerance-aware comparisons."""
    (ng, ng_ids, centres, centre_ids, bounds, k_ng, _), ng_inl, ng_avg = chunks_from_pointcloud(
        pcd_nonground_minor, T_pcd, positions, first_position, sampled_indices_global, kitti_labels, workers=workers)
    (gr, gr_ids, _, _, _, k_gr, obbs), gr_inl, gr_avg = chunks_from_pointcloud(
        pcd_ground_minor, T_pcd, positions, first_position, sampled_indices_global, kitti_labels, ground=True, workers=workers)
    return {
        "pcd_nonground_chunks": ng,
        "pcd_ground_chunks": gr,
        "pcd_nonground_chunks_major_downsampling": [voxel_down_sample(c, MAJOR_VOXEL_SIZE)[0] for c in ng],
        "pcd_ground_chunks_major_downsampling": [voxel_down_sample(c, MAJOR_VOXEL_SIZE)[0] for c in gr],
        "indices": ng_ids,
        "indices_ground": gr_ids,
        "center_positions": centres,
        "center_ids": centre_ids,
        "chunk_bounds": bounds,
        "kitti_labels": {"nonground": k_ng, "ground": k_gr},
        "obbs": obbs,
        "_inliers": {"nonground": ng_inl, "ground": gr_inl},
        "_avg": {"nonground": ng_avg, "ground": gr_avg},
    }
