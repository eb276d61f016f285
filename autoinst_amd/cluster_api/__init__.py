"""DBSCAN on the device: the clustering baseline the reference compares NCuts against, for one cloud or many in one call.

``AggregationClustering.clusters_hdbscan`` / ``clusterize_pcd`` (``pipeline/utils/aggregate.py:253-327``) run
``sklearn.cluster.DBSCAN(eps=0.7, min_samples=20)`` on the non-ground points, keep the 50 largest clusters and mark the rest
-1 and the ground -10.  `dbscan` gives scikit-learn's ``labels_`` label for label (`ai_dbscan`, rules D1-D6 in
``include/autoinst_hip.h`` and DESIGN.md section 23); `clusters_dbscan` and `clusterize_pcd` are the drop-ins.  The label
post-processing (`keep_largest_labels`, `delimited_labels`, `ground_labels`) touches no device and is tested on the host.
"""
from __future__ import annotations

import numpy as np

from .. import _ffi
from .._buffers import concat, is_device_tensor, place_of, points_f64

GROUND_LABEL = -10   # the reference's ground mark (aggregate.py:303, 315)


def keep_largest_labels(labels, sizes, k):
    """``labels`` with every cluster outside the ``k`` largest set to -1, where the labels live.  Clusters are ranked by (size
    descending, label ascending) -- a stable sort of the sizes -- and the kept ones keep their label values: the reference's
    convention (aggregate.py:282-287), with its undefined order among equal sizes replaced by this rule.  ``sizes[c]`` is the
    size of cluster c; a label outside ``0 .. len(sizes) - 1`` (-1, noise) stays what it is."""
    k = int(k)
    if k < 0:
        raise ValueError("keep_largest must not be negative")
    if is_device_tensor(labels):
        import torch
        sizes = torch.as_tensor(sizes, device=labels.device)
        order = torch.sort(sizes, descending=True, stable=True).indices
        keep = torch.zeros(int(sizes.shape[0]) + 1, dtype=torch.bool, device=labels.device)   # the last entry serves label -1
        keep[order[:k]] = True
        return torch.where(keep[labels.long()], labels, torch.full_like(labels, -1))
    labels, sizes = np.asarray(labels), np.asarray(sizes)
    order = np.argsort(-sizes.astype(np.int64), kind="stable")
    keep = np.zeros(sizes.shape[0] + 1, dtype=bool)
    keep[order[:k]] = True
    return np.where(keep[labels], labels, np.asarray(-1, dtype=labels.dtype))


def delimited_labels(points_set, cluster):
    """float64 labels of ``points_set`` (n, >= 3): rows that are all ``-inf`` are the delimiters between aggregated clouds
    (aggregate.py:262-266), keep label ``-inf`` and are not clustered; the others get ``cluster(their (m, 3) coordinates)``."""
    points_set = np.asarray(points_set, dtype=np.float64)
    if points_set.ndim != 2 or points_set.shape[1] < 3:
        raise ValueError("points_set must be (n, >= 3)")
    inf_rows = np.all(points_set == -np.inf, axis=1)
    labels = np.full(points_set.shape[0], -np.inf)
    labels[~inf_rows] = np.asarray(cluster(np.ascontiguousarray(points_set[~inf_rows, :3])), dtype=np.float64)
    return labels


def ground_labels(points, ground, cluster):
    """(n, 1) float64 labels: -10 where ``ground == -10``, else ``cluster(the other rows of points)`` (aggregate.py:298-327)."""
    points = np.asarray(points, dtype=np.float64)
    is_ground = np.asarray(ground).reshape(-1) == GROUND_LABEL
    if points.ndim != 2 or points.shape[1] < 3 or is_ground.shape[0] != points.shape[0]:
        raise ValueError("points must be (n, >= 3) and ground must have one entry per point")
    labels = np.full(points.shape[0], -1.0)
    labels[~is_ground] = np.asarray(cluster(points[~is_ground]), dtype=np.float64).reshape(-1)
    labels[is_ground] = GROUND_LABEL
    return labels.reshape(-1, 1)


def dbscan(points, eps=0.7, min_samples=20, *, keep_largest=None, return_counts=False, return_sizes=False, ctx=None):
    """scikit-learn's ``DBSCAN(eps, min_samples).fit(points).labels_`` on the device, for one cloud or a list of clouds.

    points: an (n, 3) array or float64 device tensor, or a list of such: many clouds in ONE library call, clustered
    independently (points of different clouds never count as neighbours); a cloud may be empty.  Returns
    ``(labels, n_clusters[, counts][, sizes])``: labels int32 where the input lives, -1 for noise; n_clusters the number of
    clusters found; counts (``return_counts``) int32 ``min(neighbours within eps, min_samples)``, the point itself included
    (a core point has ``min_samples``); sizes (``return_sizes``) int32, one per cluster found, border points included.  For a
    list every entry of the result is a list with one item per cloud.

    keep_largest=K: the labels of all clusters but the K largest become -1 (`keep_largest_labels`: size descending, then label
    ascending; the kept clusters keep their numbers).  n_clusters and sizes still describe every cluster found.

    ValueError: eps not positive or not finite, min_samples < 1, 2^30 points or more, a coordinate that is not finite.
    """
    from ..ncuts_api import default_context
    many = isinstance(points, (list, tuple))
    clouds = [points_f64(a) for a in (points if many else [points])]
    place = place_of(*clouds)
    xyz, off = concat(clouds, 3, np.float64, "points", place)
    if keep_largest is not None and int(keep_largest) < 0:
        raise ValueError("keep_largest must not be negative")
    if int(min_samples) != min_samples or not -2**31 <= int(min_samples) < 2**31:
        raise ValueError("min_samples must be an integer that fits 32 bits")
    ctx = ctx or default_context()
    n, n_clouds = int(off[-1]), len(clouds)
    want_sizes = return_sizes or keep_largest is not None
    labels = place.new(n, np.int32)
    counts = place.new(n, np.int32) if return_counts else None
    sizes = place.new(n, np.int32) if want_sizes else None
    found = np.zeros(n_clouds, dtype=np.int32)
    place.sync()
    code = _ffi.load().ai_dbscan(ctx._h, place.addr_or_null(xyz), off.ctypes.data, n_clouds, float(eps), int(min_samples), place.mem,
                                 place.addr_or_null(labels), found.ctypes.data, place.addr_or_null(counts), place.addr_or_null(sizes))
    _ffi.check(code, "ai_dbscan")
    out_l, out_n, out_c, out_s = [], [], [], []
    for c in range(n_clouds):
        a, b, k = int(off[c]), int(off[c + 1]), int(found[c])
        lab = labels[a:b]
        if keep_largest is not None:
            lab = keep_largest_labels(lab, sizes[a:a + k], keep_largest)
        out_l.append(lab)
        out_n.append(k)
        if return_counts:
            out_c.append(counts[a:b])
        if return_sizes:
            out_s.append(sizes[a:a + k])
    result = [out_l, out_n] + ([out_c] if return_counts else []) + ([out_s] if return_sizes else [])
    return tuple(result) if many else tuple(r[0] for r in result)


def clusters_dbscan(points_set, n_clusters=50, *, eps=0.7, min_samples=20, ctx=None):
    """The drop-in for ``AggregationClustering.clusters_hdbscan`` with ``clusterer='dbscan'`` (aggregate.py:253-296): float64
    labels of ``points_set`` (n, >= 3) -- DBSCAN of the rows that are not all ``-inf``, the ``n_clusters`` largest clusters kept
    under their own numbers, every other point -1, the delimiter rows ``-inf``.

    Two things differ from the reference on purpose: equal sizes are ranked by label (`keep_largest_labels`),
    and the reference's ``lbls[1:]``, which turns cluster 0 into noise when no point is noise, is not reproduced."""
    return delimited_labels(points_set, lambda p: dbscan(p, eps, min_samples, keep_largest=n_clusters, ctx=ctx)[0])


def clusterize_pcd(points, ground, n_clusters=50, *, eps=0.7, min_samples=20, ctx=None):
    """The drop-in for ``AggregationClustering.clusterize_pcd`` (aggregate.py:298-327): (n, 1) float64 labels, -10 where
    ``ground == -10``, else `clusters_dbscan` of the other points."""
    return ground_labels(points, ground, lambda p: clusters_dbscan(p, n_clusters, eps=eps, min_samples=min_samples, ctx=ctx))
