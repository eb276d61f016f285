"""Rules D1-D5 of `ai_dbscan` (include/autoinst_hip.h) restated in NumPy / SciPy: what the device is compared with, bit for bit.

`dbscan` finds candidates with a cKDTree at a radius a hair above eps and filters them with the exact D1 predicate, so the
tree's own rounding never decides; `dbscan_brute` is the same rules on the full distance matrix, for tiny clouds.  Both return
``(labels int32, n_clusters, counts int32 saturated at min_samples, sizes int32 per cluster)``.
"""
import numpy as np


def d1_sq_dist(a, b):
    """(dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own (NumPy does not fuse)."""
    d = a - b
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def neighbour_pairs(points, eps):
    """All ordered pairs (i, j), i != j, with D1 true, as two int64 arrays sorted by (i, j)."""
    from scipy.spatial import cKDTree
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if p.shape[0] == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    # the tree works on coordinates relative to the cloud's first point (a translation changes no candidate set that a radius
    # 1e-9 wider does not cover for the clouds of the tests); the exact predicate below uses the points themselves
    pairs = cKDTree(p - p[0]).query_pairs(eps * (1.0 + 1e-9) + 1e-12 * float(np.abs(p - p[0]).max() + 1.0), output_type="ndarray")
    i, j = pairs[:, 0].astype(np.int64), pairs[:, 1].astype(np.int64)
    ok = d1_sq_dist(p[i], p[j]) <= eps * eps
    i, j = i[ok], j[ok]
    ii, jj = np.concatenate([i, j]), np.concatenate([j, i])
    o = np.lexsort((jj, ii))
    return ii[o], jj[o]


def _from_pairs(n, ii, jj, min_samples):
    import scipy.sparse as sp
    from scipy.sparse.csgraph import connected_components
    neighbours = np.bincount(ii, minlength=n) + 1                       # D1: i is its own neighbour
    core = neighbours >= min_samples                                    # D2
    counts = np.minimum(neighbours, min_samples).astype(np.int32)
    cc = core[ii] & core[jj]
    g = sp.coo_matrix((np.ones(int(cc.sum()), np.int8), (ii[cc], jj[cc])), shape=(n, n)).tocsr()
    _, comp = connected_components(g, directed=False)                   # D3 (points that are not core are singletons here)
    core_idx = np.flatnonzero(core)
    # D4: number the components of the core points by their smallest core index
    first = np.full(n, n, dtype=np.int64)
    np.minimum.at(first, comp[core_idx], core_idx)
    roots = np.sort(first[first < n])
    number_of_comp = np.full(n, -1, dtype=np.int64)
    number_of_comp[comp[roots]] = np.arange(roots.shape[0])
    labels = np.full(n, -1, dtype=np.int64)
    labels[core_idx] = number_of_comp[comp[core_idx]]
    # D5: the smallest cluster number among the core neighbours
    b = ~core[ii] & core[jj]
    best = np.full(n, np.iinfo(np.int64).max)
    np.minimum.at(best, ii[b], labels[jj[b]])
    border = ~core & (best < np.iinfo(np.int64).max)
    labels[border] = best[border]
    k = int(roots.shape[0])
    sizes = np.bincount(labels[labels >= 0], minlength=k).astype(np.int32)
    return labels.astype(np.int32), k, counts, sizes


def dbscan(points, eps, min_samples):
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    ii, jj = neighbour_pairs(p, eps)
    return _from_pairs(p.shape[0], ii, jj, int(min_samples))


def dbscan_brute(points, eps, min_samples):
    """The same rules from the full matrix of D1 distances, with a plain union-find in index order."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    nb = d1_sq_dist(p[:, None, :], p[None, :, :]) <= eps * eps if n else np.zeros((0, 0), bool)
    neighbours = nb.sum(1)
    core = neighbours >= min_samples
    parent = np.arange(n)

    def find(a):
        while parent[a] != a:
            a = parent[a]
        return a
    for a, b in zip(*np.nonzero(nb & core[:, None] & core[None, :])):
        if b < a:
            ra, rb = find(a), find(b)
            if ra != rb:
                parent[max(ra, rb)] = min(ra, rb)
    root = np.array([find(a) for a in range(n)], dtype=np.int64)
    roots = np.unique(root[core])
    labels = np.full(n, -1, dtype=np.int32)
    for i in range(n):
        if core[i]:
            labels[i] = np.searchsorted(roots, root[i])
        else:
            c = np.flatnonzero(nb[i] & core)
            if c.size:
                labels[i] = np.searchsorted(roots, root[c].min())
    k = int(roots.shape[0])
    return (labels, k, np.minimum(neighbours, min_samples).astype(np.int32),
            np.bincount(labels[labels >= 0], minlength=k).astype(np.int32))


def keep_largest(labels, sizes, k):
    """Clusters ranked by (size descending, label ascending); all but the first k become -1, the others keep their numbers."""
    ranked = sorted(range(len(sizes)), key=lambda c: (-int(sizes[c]), c))[:k]
    labels = np.asarray(labels)
    return np.where(np.isin(labels, ranked), labels, -1).astype(labels.dtype)


def clusters_dbscan(points_set, n_clusters, eps, min_samples):
    """float64 labels: -inf on the all(-inf) delimiter rows, else DBSCAN of the other rows with the n_clusters largest kept."""
    ps = np.asarray(points_set, dtype=np.float64)
    inf_rows = np.all(ps == -np.inf, axis=1)
    out = np.full(ps.shape[0], -np.inf)
    lab, _, _, sizes = dbscan(ps[~inf_rows, :3], eps, min_samples)
    out[~inf_rows] = keep_largest(lab, sizes, n_clusters)
    return out


def clusterize_pcd(points, ground, n_clusters, eps, min_samples):
    points = np.asarray(points, dtype=np.float64)
    g = np.asarray(ground).reshape(-1) == -10
    out = np.full(points.shape[0], -1.0)
    out[~g] = clusters_dbscan(points[~g], n_clusters, eps, min_samples)
    out[g] = -10
    return out.reshape(-1, 1)
