"""ORACLE -- test infrastructure.  NumPy / SciPy restatement of the two point-cloud steps next to the
hot path: ``chunk_generation.py:243-256`` (radius-mean TARL pooling) and
``point_cloud_utils.py:144-174`` (1-NN re-projection).  The reference runs them on open3d's
KDTreeFlann, absent offline; cKDTree finds the candidates and the rules below decide.
Parity unpinned by the reference (it has no tests); pinned by brute force on small inputs and on boundary cases
(tests/edge_geometry.py) in tests/.

Both steps square distances in one order, ``(dx*dx + dy*dy) + dz*dz`` with every product and sum rounded on its own:
nanoflann's ``L2_Adaptor`` (what ``KDTreeFlann`` runs) and scipy's cdist alike, and the HIP kernels with contraction off.

* pooling: a scan point is in the mean iff that square is strictly below ``radius * radius`` (rounded once) --
  nanoflann's radius search, to which open3d passes the squared radius;
* 1-NN: the source with the smallest square, ties to the smaller source index; the distance returned is the correctly
  rounded sqrt of that square (open3d keeps the first of a tie it meets in tree order, which no index rule restates).
"""
import numpy as np
from scipy.spatial import cKDTree


def _sq(a, b):
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def tarl_pool(points_major, tarl_points, tarl_features, radius=0.175):
    pts = np.asarray(points_major, dtype=np.float64)
    src = np.asarray(tarl_points, dtype=np.float64)
    feats = np.asarray(tarl_features).astype(np.float64)       # np.concatenate with a float64 seed, :240-242
    out = np.zeros((pts.shape[0], feats.shape[1]))             # :245
    if src.shape[0] == 0:
        return out
    tree = cKDTree(src)
    r2 = float(radius) * float(radius)
    # cKDTree rounds its own way: gather a hair wider, then the rule decides
    for i, idx in enumerate(tree.query_ball_point(pts, radius * (1 + 1e-9))):
        idx = np.asarray(idx, dtype=np.int64)
        if idx.size:
            idx = idx[_sq(pts[i], src[idx]) < r2]              # nanoflann: dist^2 < radius^2
        if idx.size:
            out[i] = np.mean(feats[idx], axis=0)               # :251-252
    return out


def nn1_index(points_to, points_from):
    """(index[Nt] int64, distance[Nt] float64) of the nearest ``points_from`` row for every ``points_to`` row."""
    t = np.asarray(points_to, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(points_from, dtype=np.float64).reshape(-1, 3)
    tree = cKDTree(f)
    k = min(2, f.shape[0])
    d, idx = tree.query(t, k=k)
    d, idx = d.reshape(t.shape[0], k), idx.reshape(t.shape[0], k)
    best = idx[:, 0].astype(np.int64)
    # where the runner-up is within a hair, every source that close is a candidate and the rule picks
    close = np.flatnonzero(d[:, -1] <= d[:, 0] * (1 + 1e-9) + 1e-12) if k > 1 else np.zeros(0, np.int64)
    for i, cand in zip(close, tree.query_ball_point(t[close], d[close, 0] * (1 + 1e-9) + 1e-12)):
        cand = np.asarray(cand, dtype=np.int64)
        s = _sq(t[i], f[cand])
        best[i] = cand[s == s.min()].min()
    return best, np.sqrt(_sq(t, f[best]))


def nn1_reproject(features_to, points_to, features_from, points_from, max_radius=None, no_feature_label=(1, 0, 0)):
    features_to = np.array(features_to, copy=True)
    idx, d = nn1_index(points_to, points_from)
    features_to[:] = np.asarray(features_from)[idx]
    if max_radius is not None:
        features_to[d > max_radius] = np.asarray(no_feature_label, dtype=features_to.dtype)
    return features_to
