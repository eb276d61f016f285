"""ORACLE -- test infrastructure, NOT the product.

CPU restatement (NumPy / SciPy) of the reference's NCuts hot path, written from the
reference's behaviour, each function citing the reference lines it
follows.  Only ``tests/``, ``__graft_entry__.smoke()`` and ``bench.py``'s
``cpu_baseline`` leg may import this package; the product (``autoinst_amd``) never
does and fails loudly when its HIP library is missing.

Parity pin: rows a9-a12 (``normalized_cut``) are pinned by golden vectors generated
by importing the reference's own ``pipeline/ncuts/normalized_cut.py`` in the build
container (``oracle/gen_golden.py`` -> ``tests/golden/*.npz``).  Rows a1-a8 (affinity)
cannot be pinned by running the reference (``ncuts_utils.py`` needs open3d / cv2 /
pykitti, absent offline -- an ordinary ModuleNotFoundError) and the reference has no
tests of its own, so they are pinned by the closed form of the ~25 arithmetic lines
(`affinity_dense` restates them literally, `affinity_sparse` must equal it).

Third-party arithmetic the reference delegates to (not under /root/reference):
scipy.spatial.distance.cdist, scipy.sparse, scipy.sparse.linalg.eigsh (ARPACK +
SuperLU).  The reference leaves SciPy unpinned (``setup.sh:8-9``); goldens were made
with scipy 1.15.3 / numpy 2.2.6 and record that.
"""
from __future__ import annotations

import numpy as np
import scipy.sparse as sp
import scipy.sparse.linalg as spla
from scipy.spatial import cKDTree
from scipy.spatial.distance import cdist

NUM_CUTS = 10  # normalized_cut.py:54


# --------------------------------------------------------------------------- affinity
def sam_label_distance(sam_features, spatial_distance, proximity_threshold, beta):
    """``utils/image/image_utils.py:64-89`` literally: per pair inside the radius, the fraction of the
    views in which both points carry a SAM id (!= -1) and the ids differ; weight exp(-beta * fraction)."""
    mask = np.where(spatial_distance <= proximity_threshold)
    num_points, num_views = sam_features.shape
    distance_matrix = np.zeros((num_points, num_points))
    for (point1, point2) in zip(*mask):
        view_counter = 0
        for view in range(num_views):
            instance_id1 = sam_features[point1, view]
            instance_id2 = sam_features[point2, view]
            if instance_id1 != -1 and instance_id2 != -1:
                view_counter += 1
                if instance_id1 != instance_id2:
                    distance_matrix[point1, point2] += 1
        if view_counter:
            distance_matrix[point1, point2] /= view_counter
    mask = np.where(spatial_distance <= proximity_threshold, 1, 0)
    return mask * np.exp(-beta * distance_matrix), mask


def affinity_dense(points, tarl=None, dino=None, *, alpha=1.0, theta=0.0, gamma=0.0, radius=1.0, sam=None, beta=0.0):
    """Literal dense restatement of ``ncuts_utils.py:60-67, 112-156``.

    Returns the dense (N,N) float64 matrix A = tarl_w * spatial_w * sam_w * dino_w.  ``sam`` is the
    per-camera list of (N, views) SAM id matrices (or one such matrix).  Only for small N (O(N^2)
    memory, like the reference).
    """
    points = np.asarray(points, dtype=np.float64)
    spatial_distance = cdist(points, points)                        # :60
    mask = np.where(spatial_distance <= radius, 1, 0)               # :61
    if alpha:                                                       # :63-66
        spatial_w = mask * np.exp(-alpha * spatial_distance)
    else:
        spatial_w = mask
    sam_w = mask.copy()                                             # :112
    dino_w = mask.copy()                                            # :113
    if beta:                                                        # :115-123
        sam_list = [] if sam is None else (list(sam) if isinstance(sam, (list, tuple)) else [sam])
        if len(sam_list) == 0:
            raise ValueError("The length should be longer than 0!")  # :116-117
        for sam_features_major in sam_list:
            cam_w, _ = sam_label_distance(np.asarray(sam_features_major), spatial_distance, radius, beta)
            sam_w = sam_w * cam_w
    if gamma:                                                       # :125-133
        dino_list = [] if dino is None else (list(dino) if isinstance(dino, (list, tuple)) else [dino])
        if len(dino_list) == 0:
            raise ValueError("The length should be longer than 0!")  # :126-127
        for dinov2_features_major in dino_list:                     # :128-133, one factor per camera
            dino_distance = cdist(dinov2_features_major, dinov2_features_major)
            dino_w = dino_w * np.exp(-gamma * dino_distance)
    if theta:                                                       # :135-147
        tarl = np.asarray(tarl, dtype=np.float64)
        no_tarl = ~np.array(tarl).any(1)
        tarl_distance = cdist(tarl, tarl)
        tarl_distance[no_tarl] = 0
        tarl_distance[:, no_tarl] = 0
        tarl_w = mask * np.exp(-theta * tarl_distance)
    else:
        tarl_w = mask                                               # :149
    return tarl_w * spatial_w * sam_w * dino_w                      # :151-156


def remove_isolated_points(A):
    """``point_cloud_utils.py:189-195``: keep rows that are not all-zero.

    Because A_ii = exp(0) = 1 no row is ever all-zero, so this is the identity on the
    hot path; returned mask lets tests assert that.
    """
    keep = ~np.all(A == 0, axis=1)
    return keep, A[keep][:, keep]


def affinity_sparse(points, tarl=None, dino=None, *, alpha=1.0, theta=0.0, gamma=0.0, radius=1.0, sam=None, beta=0.0):
    """Sparse restatement: same values as `affinity_dense` on the radius graph.

    CSR float64, int32 indices sorted per row, diagonal 1 stored -- i.e. exactly
    ``scipy.sparse.csr_matrix(A)`` of ``ncuts_utils.py:167``.  Factors are multiplied
    in the reference's order (tarl * spatial * sam * dino) so values are bit-equal to
    the dense path wherever cdist's per-pair result is.
    """
    points = np.asarray(points, dtype=np.float64)
    n = points.shape[0]
    tree = cKDTree(points)
    # cKDTree tests d <= r with the same sqrt-of-sum-of-squares as cdist up to rounding;
    # query a hair wider, then apply the reference's own test on the cdist-style distance
    pairs = tree.query_pairs(radius * (1 + 1e-9) + 1e-12, output_type="ndarray")
    i = np.concatenate([pairs[:, 0], pairs[:, 1], np.arange(n)])
    j = np.concatenate([pairs[:, 1], pairs[:, 0], np.arange(n)])
    d = _rowwise_euclid(points, i, j)
    keep = d <= radius
    i, j, d = i[keep], j[keep], d[keep]
    spatial_w = np.exp(-alpha * d) if alpha else np.ones_like(d)
    w = np.ones_like(d)
    if theta:
        tarl = np.asarray(tarl, dtype=np.float64)
        no_tarl = ~tarl.any(1)
        t = _rowwise_euclid(tarl, i, j)
        t[no_tarl[i] | no_tarl[j]] = 0.0
        w = w * np.exp(-theta * t)
    w = w * spatial_w
    if beta:
        sam_list = [] if sam is None else (list(sam) if isinstance(sam, (list, tuple)) else [sam])
        if len(sam_list) == 0:
            raise ValueError("The length should be longer than 0!")
        sam_w = np.ones_like(d)
        for sf in sam_list:
            sf = np.asarray(sf)
            both = (sf[i] != -1) & (sf[j] != -1)
            co = both.sum(1)
            diff = (both & (sf[i] != sf[j])).sum(1).astype(np.float64)
            frac = np.divide(diff, co, out=np.zeros_like(diff), where=co > 0)
            sam_w = sam_w * np.exp(-beta * frac)
        w = w * sam_w
    if gamma:
        dino_list = [] if dino is None else (list(dino) if isinstance(dino, (list, tuple)) else [dino])
        if len(dino_list) == 0:
            raise ValueError("The length should be longer than 0!")
        dino_w = np.ones_like(d)
        for dn in dino_list:
            dino_w = dino_w * np.exp(-gamma * _rowwise_euclid(np.asarray(dn, dtype=np.float64), i, j))
        w = w * dino_w
    A = sp.csr_matrix((w, (i, j)), shape=(n, n))
    A.sum_duplicates()
    A.sort_indices()
    return A


def _rowwise_euclid(X, i, j, block=1 << 18):
    """sqrt(sum((X[i]-X[j])**2)) like cdist's euclidean kernel, blocked over pairs.

    For 3-D points the squares are added in cdist's order, ``(dx*dx + dy*dy) + dz*dz``: einsum may pair them otherwise,
    and one ulp decides the radius test of a pair at the radius (tests/test_edge_geometry.py)."""
    out = np.empty(i.shape[0], dtype=np.float64)
    for s in range(0, i.shape[0], block):
        e = min(s + block, i.shape[0])
        diff = X[i[s:e]] - X[j[s:e]]
        if diff.shape[1] == 3:
            sq = diff * diff
            out[s:e] = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
        else:
            out[s:e] = np.sqrt(np.einsum("ij,ij->i", diff, diff))
    return out


# --------------------------------------------------------------------------- normalized cut
def cut_cost(W, mask):
    """``normalized_cut.py:4-5``."""
    return (np.sum(W) - np.sum(W[mask][:, mask]) - np.sum(W[~mask][:, ~mask])) / 2


def ncut_cost(W, d, cut):
    """``normalized_cut.py:7-11`` with ``D.todense()[cut].sum()`` restated as ``d[cut].sum()``.

    The reference densifies the N x N diagonal matrix only to sum its diagonal under a
    row mask: ``D.todense()[cut]`` selects rows, ``.sum()`` adds every entry, and every
    off-diagonal entry is zero, so the value is the sum of d over the mask.
    """
    cost = cut_cost(W, cut)
    assoc_a = d[cut].sum()
    assoc_b = d[~cut].sum()
    return (cost / assoc_a) + (cost / assoc_b)


def _edge_view(w):
    coo = w.tocoo()
    return coo.row, coo.col, coo.data


def ncut_cost_fast(edges, d, cut):
    """Same quantity from an edge list: cut = sum_{i in A, j in B} w_ij."""
    r, c, v = edges
    cost = v[cut[r] & ~cut[c]].sum()
    return (cost / d[cut].sum()) + (cost / d[~cut].sum())


def get_min_ncut(ev, d, w, num_cuts, fast=False):
    """``normalized_cut.py:13-34``: 10 strict thresholds, first strictly-smaller cost wins."""
    mcut = np.inf
    mn = ev.min()
    mx = ev.max()
    min_mask = np.zeros_like(ev, dtype=bool)
    if np.allclose(mn, mx):
        return min_mask, mcut
    edges = _edge_view(w) if fast else None
    with np.errstate(divide="ignore", invalid="ignore"):
        for t in np.linspace(mn, mx, num_cuts, endpoint=False):
            mask = ev > t
            cost = ncut_cost_fast(edges, d, mask) if fast else ncut_cost(w, d, mask)
            if cost < mcut:
                min_mask = mask
                mcut = cost
    return min_mask, mcut


def laplacian_sym(w):
    """``normalized_cut.py:38,42-47``: W = w + I, d = colsum(W), A = D^-1/2 (D - W) D^-1/2."""
    W = w + sp.identity(w.shape[0])
    d = np.array(W.sum(axis=0))[0]
    d2 = np.reciprocal(np.sqrt(d))
    D = sp.diags(d)
    D2 = sp.diags(d2)
    return D2 * (D - W) * D2, d


def fiedler(w):
    """``normalized_cut.py:49-53``: eigsh(A, 2, sigma=1e-10, which='LM'), 2nd-smallest pair."""
    A, d = laplacian_sym(w)
    eigvals, eigvecs = spla.eigsh(A, 2, sigma=1e-10, which="LM")
    index2 = np.argsort(eigvals)[1]
    return eigvals, eigvecs[:, index2], d


def normalized_cut(w, num_points_orig, labels, T=0.01, split_lim=0.01, fast=False, stats=None):
    """``normalized_cut.py:37-63`` -- recursive 2-way normalized cut.

    Note the reference's recursive calls pass ``T`` but rely on the default
    ``split_lim=0.01`` (``:57-58``); reproduced.  ``fast=True`` swaps the per-threshold
    sparse fancy-index slices for an edge-list pass (same value up to summation order);
    ``stats`` (a dict) collects the number of eigsh calls.
    """
    n = w.shape[0]
    split_percentage = labels.shape[0] / (num_points_orig + 1e-8)
    if n > 2 and split_percentage > split_lim:
        _, ev, d = fiedler(w)
        if stats is not None:
            stats["eigsh"] = stats.get("eigsh", 0) + 1
        mask, mcut = get_min_ncut(ev, d, w, NUM_CUTS, fast=fast)
        if mcut < T:
            l1 = normalized_cut(w[mask][:, mask], num_points_orig, labels[mask], T=T, fast=fast, stats=stats)
            l2 = normalized_cut(w[~mask][:, ~mask], num_points_orig, labels[~mask], T=T, fast=fast, stats=stats)
            return l1 + l2
        return [labels]
    return [labels]


def ncuts(points, tarl=None, dino=None, *, alpha=1.0, theta=0.0, gamma=0.0, T=0.03,
          split_lim=0.01, radius=1.0, fast=True, stats=None):
    """Array-level ``ncuts_chunk`` lines 60-174: affinity -> CSR -> normalized_cut."""
    A = affinity_sparse(points, tarl, dino, alpha=alpha, theta=theta, gamma=gamma, radius=radius)
    n = A.shape[0]
    return normalized_cut(A, n, np.arange(n), T=T, split_lim=split_lim, fast=fast, stats=stats)


# --------------------------------------------------------------------------- partition helpers
def groups_to_labels(groups, n):
    """list of index arrays -> label array (group k -> k); -1 where uncovered."""
    lab = np.full(n, -1, dtype=np.int64)
    for k, g in enumerate(groups):
        lab[np.asarray(g, dtype=np.int64)] = k
    return lab


def canonical_labels(lab):
    """Relabel so that groups are numbered by their smallest member (order-free form)."""
    lab = np.asarray(lab)
    _, first, inv = np.unique(lab, return_index=True, return_inverse=True)
    order = np.argsort(np.argsort(first))
    return order[inv]


def partitions_equal(a, b):
    return np.array_equal(canonical_labels(a), canonical_labels(b))


def adjusted_rand_index(a, b):
    a = canonical_labels(a)
    b = canonical_labels(b)
    n = a.shape[0]
    ct = sp.coo_matrix((np.ones(n), (a, b))).tocsr()
    ct.sum_duplicates()
    nij = ct.data
    ai = np.asarray(ct.sum(1)).ravel()
    bj = np.asarray(ct.sum(0)).ravel()
    comb = lambda x: x * (x - 1) / 2.0
    s = comb(nij).sum()
    sa, sb = comb(ai).sum(), comb(bj).sum()
    exp = sa * sb / comb(n)
    mx = 0.5 * (sa + sb)
    if mx == exp:
        return 1.0
    return float((s - exp) / (mx - exp))
