"""CPU restatement of ``ai_chunk_finish`` (rules F1-F6 in ``include/autoinst_hip.h``): the tail of ``ncuts_chunk``
(reference ``pipeline/ncuts/ncuts_utils.py:185-204``) and ``get_corrected_ground`` (``point_cloud_utils.py:331-342``) on arrays.

* F2: nearest major point by ``(dx*dx + dy*dy) + dz*dz`` (NumPy rounds every step), ties to the smaller index: brute force, or a
  cKDTree that proposes candidates whose squares are then formed by that expression;
* F3: `prep_ref.statistical_inliers`;
* F4: `f4_sum`, the sum of z over the inliers in the order the header writes down;
* F5 / F6: comparisons and concatenations.

``variant`` switches ONE rule to a plausible wrong one, so that `test_finish_ref.py` can show that the right rules are told
from them: ``"le"`` (``<=`` in the height cut), ``"mean_all"`` (mean z over all ground points), ``"keep_in_inliers"``
(``ground_keep`` indexes the inlier list), ``"tie_larger"``, ``"no_plus_one"``, and for `finish_chunks` ``"neighbour_chunk"``
(a fine point sees every chunk's major points).
"""
from __future__ import annotations

import numpy as np
from scipy.spatial import cKDTree

import prep_ref

MEAN_HEIGHT = 0.6   # config.py:68


def sq_dist(p, q):
    d = p - q
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def nearest_brute(fine, major, larger=False):
    """(index, distance, tied): `tied[i]` = number of further majors at exactly the nearest squared distance."""
    fine, major = np.asarray(fine, np.float64).reshape(-1, 3), np.asarray(major, np.float64).reshape(-1, 3)
    d2 = sq_dist(fine[:, None, :], major[None, :, :])
    best = d2.min(axis=1)
    hit = d2 == best[:, None]
    idx = (major.shape[0] - 1 - np.argmax(hit[:, ::-1], axis=1)) if larger else np.argmax(hit, axis=1)
    return idx.astype(np.int64), np.sqrt(best), hit.sum(axis=1) - 1


def nearest(fine, major, larger=False, k=6, workers=1):
    """`nearest_brute` for large clouds: the k nearest by cKDTree are the candidates; a point whose k-th candidate is not
    strictly farther than its nearest (by the stated expression, with a margin for the tree's own rounding) goes to brute force."""
    fine, major = np.asarray(fine, np.float64).reshape(-1, 3), np.asarray(major, np.float64).reshape(-1, 3)
    nf, nm = fine.shape[0], major.shape[0]
    if nf == 0:
        return np.zeros(0, np.int64), np.zeros(0), np.zeros(0, np.int64)
    if nm <= k:
        return nearest_brute(fine, major, larger)
    _, cand = cKDTree(major).query(fine, k=k, workers=workers)
    d2 = sq_dist(fine[:, None, :], major[cand])
    best = d2.min(axis=1)
    hit = d2 == best[:, None]
    ci = np.where(hit, cand, -1 if larger else nm)
    idx = ci.max(axis=1) if larger else ci.min(axis=1)
    tied = hit.sum(axis=1) - 1
    unsure = np.flatnonzero(d2.max(axis=1) <= best * (1.0 + 1e-9))   # all k candidates (nearly) tied: others may be as well
    if unsure.size:
        bi, _, bt = nearest_brute(fine[unsure], major, larger)
        idx[unsure], tied[unsure] = bi, bt
    return idx.astype(np.int64), np.sqrt(best), tied


def _block_sum(v):
    """ai_block_sum_first over 256 values: four waves of 64, each a pairwise tree, then ((w0 + w1) + w2) + w3."""
    w = np.asarray(v, np.float64).reshape(4, 64)
    while w.shape[1] > 1:
        w = w[:, 0::2] + w[:, 1::2]
    w = w[:, 0]
    return ((w[0] + w[1]) + w[2]) + w[3]


def f4_sum(z, flag):
    """The sum of z[i] over flag[i] in F4's order: slot s = i mod 65536 adds its members in ascending i; the 256 slots of a block
    go through `_block_sum`, and so do the 256 block sums."""
    z, flag = np.asarray(z, np.float64), np.asarray(flag, bool)
    acc = np.zeros(65536)
    for s in range(0, z.shape[0], 65536):
        zz = np.where(flag[s:s + 65536], z[s:s + 65536], 0.0)   # + 0.0 changes no partial sum
        acc[:zz.shape[0]] = acc[:zz.shape[0]] + zz
    blocks = np.array([_block_sum(acc[b * 256:(b + 1) * 256]) for b in range(256)])
    return _block_sum(blocks)


def corrected_ground(ground, nb_neighbors=20, std_ratio=2.0, mean_height=MEAN_HEIGHT, *, variant=None, workers=1, brute=False):
    """dict: keep (chunk-local indices, ascending), inliers, avg, mean, std, threshold, n_inliers, mean_z, z_limit."""
    ground = np.asarray(ground, np.float64).reshape(-1, 3)
    n = ground.shape[0]
    inl, avg, mean, std, thr = prep_ref.statistical_inliers(ground, nb_neighbors, std_ratio, workers=workers, brute=brute)
    flag = np.zeros(n, bool)
    flag[inl] = True
    z = ground[:, 2]
    with np.errstate(invalid="ignore", divide="ignore"):
        if variant == "mean_all":
            mean_z = np.float64(f4_sum(z, np.ones(n, bool))) / np.float64(n)
        else:
            mean_z = np.float64(f4_sum(z, flag)) / np.float64(inl.size)
    z_limit = mean_z + np.float64(mean_height)
    with np.errstate(invalid="ignore"):
        below = (z <= z_limit) if variant == "le" else (z < z_limit)
    keep = np.flatnonzero(flag & below)
    if variant == "keep_in_inliers":
        keep = np.flatnonzero(below[inl])
    return {"keep": keep.astype(np.int64), "inliers": inl, "avg": avg, "mean": mean, "std": std, "threshold": thr,
            "n_inliers": int(inl.size), "mean_z": float(mean_z), "z_limit": float(z_limit)}


def finish_chunk(fine, major, labels, ground, nb_neighbors=20, std_ratio=2.0, mean_height=MEAN_HEIGHT, *, variant=None, workers=1,
                 brute=False):
    """One chunk: `corrected_ground`'s dict plus fine_nn, fine_dist, fine_tied, fine_label, merged_points, merged_label."""
    fine = np.asarray(fine, np.float64).reshape(-1, 3)
    major = np.asarray(major, np.float64).reshape(-1, 3)
    ground = np.asarray(ground, np.float64).reshape(-1, 3)
    if fine.shape[0] and not major.shape[0]:
        raise ValueError("a chunk with fine points and no major points")
    if not (np.isfinite(fine).all() and np.isfinite(major).all() and np.isfinite(ground).all()):
        raise ValueError("coordinates are not finite")
    find = nearest_brute if brute else (lambda f, m, larger: nearest(f, m, larger, workers=workers))
    nn, dist, tied = find(fine, major, variant == "tie_larger")
    out = corrected_ground(ground, nb_neighbors, std_ratio, mean_height, variant=variant, workers=workers, brute=brute)
    lab = np.asarray(labels, np.int32).reshape(-1)[nn]
    out.update(fine_nn=nn.astype(np.int32), fine_dist=dist, fine_tied=tied, fine_label=lab,
               merged_points=np.concatenate([fine, ground[out["keep"]]]),
               merged_label=np.concatenate([lab + (0 if variant == "no_plus_one" else 1),
                                            np.zeros(out["keep"].size, np.int32)]).astype(np.int32))
    return out


def finish_chunks(fine, major, labels, ground, nb_neighbors=20, std_ratio=2.0, mean_height=MEAN_HEIGHT, *, variant=None, workers=1,
                  brute=False):
    """All chunks, each by itself (F1).  ``variant="neighbour_chunk"``: every fine point searches all chunks' major points."""
    if variant == "neighbour_chunk":
        all_major = np.concatenate([np.asarray(m, np.float64).reshape(-1, 3) for m in major])
        all_labels = np.concatenate([np.asarray(l).reshape(-1) for l in labels])
        return [finish_chunk(f, all_major, all_labels, g, nb_neighbors, std_ratio, mean_height, workers=workers, brute=brute)
                for f, g in zip(fine, ground)]
    return [finish_chunk(f, m, l, g, nb_neighbors, std_ratio, mean_height, variant=variant, workers=workers, brute=brute)
            for f, m, l, g in zip(fine, major, labels, ground)]


def street_fixture(workers=1):
    """The fixture of tests/test_gpu_finish.py: `synth.street_map(72.0, seed=3, step=0.1)` with the ground of y > 6.5 raised by
    0.9 m (a kerb above mean_z + 0.6), chunked by `prep_ref.chunk_and_downsample_point_clouds`.  Returns (map, dict)."""
    from autoinst_amd import synth
    m = synth.street_map(72.0, seed=3, step=0.1)
    g = m["ground"].copy()
    g[g[:, 1] > 6.5, 2] += 0.9
    m["ground"] = g
    d = prep_ref.chunk_and_downsample_point_clouds(m["nonground"], m["ground"], m["T_pcd"], m["positions"], m["first_position"],
                                                   m["indices"], m["labels"], workers=workers)
    return m, d
