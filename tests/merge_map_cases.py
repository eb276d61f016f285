"""Fixtures of the whole-map merge (``ai_merge_map``, rules M1-M10): the seeded random maps of rule M11, the hand-made cases and
the colouring under which ``oracle/merge_ref.py`` and the id-identified merge are the same function.  Shared by the CPU checks of
the restatement (``test_merge_map_ref.py``) and the device checks (``test_gpu_merge_map.py``)."""
from __future__ import annotations

import warnings

import numpy as np

from oracle import merge_ref

SIDE = 40.0


# ------------------------------------------------------------------------------------------------- M11: ids as colours
def goff_of(instances):
    nloc = [int(np.max(i)) if np.size(i) else 0 for i in instances]
    return np.concatenate([[0], np.cumsum(nloc)]).astype(np.int64)


def colour(gid):
    """colour(global id g) = (g, 0, 0), black for 0: the lexicographic colour order is the id order."""
    c = np.zeros((np.size(gid), 3))
    c[:, 0] = np.asarray(gid, dtype=np.float64)
    return c


def colour_chunks(points, instances):
    """The (points, colours) pairs the colour-identified merges take, every chunk's local ids coloured as their provisional
    global ids (M1)."""
    goff = goff_of(instances)
    out = []
    for c, (p, i) in enumerate(zip(points, instances)):
        i = np.asarray(i, dtype=np.int64)
        out.append((np.asarray(p, dtype=np.float64).reshape(-1, 3), colour(np.where(i > 0, goff[c] + i, 0))))
    return out


def oracle(points, instances):
    """`oracle.merge_ref.merge_chunks_unite_instances2` on the coloured chunks: (points, global ids).  The reference takes
    np.mean of an empty chunk (NaN, with a warning) and crops nothing with it."""
    with warnings.catch_warnings(), np.errstate(all="ignore"):
        warnings.simplefilter("ignore")
        p, c = merge_ref.merge_chunks_unite_instances2(colour_chunks(points, instances))
    assert not c[:, 1:].any() and np.array_equal(c[:, 0], np.round(c[:, 0]))
    return p, c[:, 0].astype(np.int64)


def mean_centers(points):
    """The centres the reference computes itself (:397-403), np.mean per axis; NaN -> 0 for an empty chunk (never used)."""
    out = np.zeros((len(points), 3))
    for c, p in enumerate(points):
        p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
        if p.shape[0]:
            out[c] = [p[:, 0].mean(), p[:, 1].mean(), p[:, 2].mean()]
    return out


def face_distance(points, centers, side=SIDE):
    """The smallest distance of an earlier point's coordinate to a face of a later chunk's crop cube."""
    best = np.inf
    for c in range(1, len(points)):
        prev = [np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in points[:c] if np.size(p)]
        if not prev or not np.size(points[c]):
            continue
        prev = np.concatenate(prev)
        for b in (centers[c] - side / 2.0, centers[c] + side / 2.0):
            best = min(best, float(np.abs(prev - b).min()))
    return best


def random_map(rng):
    """One small random map: 1-5 chunks cut from one cloud on a 0.25 m grid (shared points and shared scalars), some chunks
    shifted copies, some all street, some with duplicates inside the chunk that carry other instances, a few -0.0."""
    n_chunks = int(rng.integers(1, 6))
    base = np.round(rng.normal(0, 6, (int(rng.integers(30, 300)), 3)) * 4) / 4
    base[rng.random(base.shape) < 0.02] *= -0.0
    points, instances = [], []
    for c in range(n_chunks):
        sel = rng.random(base.shape[0]) < 0.7
        sel[int(rng.integers(0, base.shape[0]))] = True
        pts = base[sel] + (0.0 if rng.random() < 0.6 else np.round(rng.normal(0, 0.5, 3) * 4) / 4)
        k = int(rng.integers(1, 6))
        inst = rng.integers(0, k + 1, pts.shape[0])
        if rng.random() < 0.5:                                   # duplicates inside the chunk, with ids of their own
            dup = rng.integers(0, pts.shape[0], int(rng.integers(1, 12)))
            pts = np.concatenate([pts, pts[dup]])
            inst = np.concatenate([inst, rng.integers(0, k + 1, dup.size)])
            perm = rng.permutation(pts.shape[0])
            pts, inst = pts[perm], inst[perm]
        if rng.random() < 0.15:
            inst = np.zeros_like(inst)                           # all street
        points.append(np.ascontiguousarray(pts))
        instances.append(inst.astype(np.int32))
    return points, instances


def random_maps(count, seed=2024):
    rng = np.random.default_rng(seed)
    return [random_map(rng) for _ in range(count)]


# ------------------------------------------------------------------------------------------------- hand-made cases
def _scalar_cloud(lo, hi, n_distinct, start, step=0.03125):
    """Points whose box is [lo, hi]^3 and whose pooled coordinates have exactly n_distinct distinct values: the two corners and
    n_distinct - 2 values start, start + step, ... strictly inside (odd multiples of 2^-6: exact, never an integer), the last
    repeated to fill a row."""
    inner = start + step * np.arange(n_distinct - 2)
    assert lo < inner.min() and inner.max() < hi
    inner = np.concatenate([inner, np.repeat(inner[-1], (-inner.size) % 3)])
    return np.concatenate([[[lo] * 3, [hi] * 3], inner.reshape(-1, 3)])


def _case(points, instances, centers, **expect):
    return dict(points=[np.asarray(p, dtype=np.float64).reshape(-1, 3) for p in points],
                instances=[np.asarray(i, dtype=np.int32).reshape(-1) for i in instances],
                centers=np.asarray(centers, dtype=np.float64).reshape(len(points), 3), **expect)


def hand_cases():
    """name -> dict(points, instances, centers, inst=expected global ids of the output, src=expected sources).  Every centre is
    given, (0, 0, 0) unless the case is about the crop."""
    z = [0.0, 0.0, 0.0]
    cases = {}
    # M3: at step 1 chunk 0 still has its duplicate (1,1,1) of instance 2, which stretches 2's box to [1, 5]^3 (:406 crops the
    # un-deduplicated first chunk); both points of the new instance lie in it: inter 2, S1 = {1, 5}, S2 = {2, 3}, iou 2/4
    cases["step1_duplicate_stretches_box"] = _case(
        [[[0, 0, 0], [1, 1, 1], [5, 5, 5], [1, 1, 1]], [[3, 3, 3], [2, 2, 2]]], [[1, 1, 2, 2], [1, 1]], [z, z],
        inst=[1, 1, 2, 2, 2], src=[0, 1, 2, 4, 5])
    # M3: from step 2 on the duplicate is gone (:489 ran): 2's box is the point (5,5,5), nothing lies in it, the id stays 2 + 1
    cases["step2_sees_kept_points_only"] = _case(
        [[[1, 1, 1], [5, 5, 5], [1, 1, 1]], [[10, 10, 10]], [[3, 3, 3], [2, 2, 2]]], [[1, 2, 2], [0], [1, 1]], [z, z, z],
        inst=[1, 2, 0, 3, 3], src=[0, 1, 3, 4, 5])
    # M2: one chunk, the loop (:395) does not run, nothing is removed
    cases["one_chunk_keeps_duplicates"] = _case([[[0, 0, 0], [0, 0, 0], [-0.0, 0, 0], [1, 2, 3]]], [[1, 2, 0, 2]], [z],
                                                inst=[1, 2, 0, 2], src=[0, 1, 2, 3])
    # M9: instance 1 (box [0, 4]^3, 44 scalars) holds one of the two points, 1 / (44 + 6); instance 2 (box [-1, 15]^3, 94 scalars)
    # holds both, 2 / (94 + 6): equal doubles, :474 replaces only on a strictly larger iou, so the first (smaller) id stays
    two = [[1, 2, 3], [11, 12, 13]]
    g1, g2 = _scalar_cloud(0, 4, 44, 0.515625), _scalar_cloud(-1, 15, 94, 4.515625)
    cases["iou_tie_keeps_smaller_id"] = _case([np.concatenate([g1, g2]), two], [[1] * len(g1) + [2] * len(g2), [1, 1]], [z, z],
                                              inst=[1] * len(g1) + [2] * len(g2) + [1, 1], src=list(range(len(g1) + len(g2) + 2)))
    # the same with the ids of the two clouds swapped: now the large box comes first and stays
    cases["iou_tie_keeps_smaller_id_swapped"] = _case(
        [np.concatenate([g2, g1]), two], [[1] * len(g2) + [2] * len(g1), [1, 1]], [z, z],
        inst=[1] * len(g2) + [2] * len(g1) + [1, 1], src=list(range(len(g1) + len(g2) + 2)))
    # M8: 1 / (94 + 6) is the double 0.01, which is not above 0.01 (:459): no association, the id stays 1 + 1
    g = _scalar_cloud(0, 4, 94, 0.515625)
    cases["iou_exactly_iou_min"] = _case([g, two], [[1] * len(g), [1, 1]], [z, z],
                                         inst=[1] * len(g) + [2, 2], src=list(range(len(g) + 2)))
    # M5: (20, 0, 0) lies ON the cube's face x = 0 + 40 / 2 and is cropped in (:406-417, open3d's crop is inclusive); without it
    # the box would be the point (18,-1,-1) and hold nothing.  S1 = {20, 0, 18, -1}, S2 = {19, -0.5}: 1 / 6
    cases["crop_face_inclusive"] = _case([[[20, 0, 0], [18, -1, -1]], [[19, -0.5, -0.5]]], [[1, 1], [1]], [z, z],
                                         inst=[1, 1, 1], src=[0, 1, 2])
    # M8: (9, 0, -1) lies on the faces y = max and z = min of the box [8, 10] x [-1, 0] x [-1, 0] (:451-456, >= and <=)
    cases["box_face_inclusive"] = _case([[[10, 0, 0], [8, -1, -1]], [[9, 0, -1]]], [[1, 1], [1]], [z, z],
                                        inst=[1, 1, 1], src=[0, 1, 2])
    # M9: both local instances lie in the one map instance's box and take its id (:479-481 re-colours each)
    cases["two_locals_take_one_map_instance"] = _case(
        [[[0, 0, 0], [6, 6, 6]], [[1, 1, 1], [2, 2, 2], [4, 4, 4], [5, 5, 5], [30, 30, 30]]], [[1, 1], [1, 1, 2, 2, 3]], [z, z],
        inst=[1, 1, 1, 1, 1, 1, 4], src=[0, 1, 2, 3, 4, 5, 6])
    # M3: the empty chunk in the middle adds nothing; the third chunk meets chunk 0's instance, and its copy of (0,0,0) is dropped
    cases["empty_chunk_in_the_middle"] = _case(
        [[[0, 0, 0], [6, 6, 6]], np.zeros((0, 3)), [[1, 1, 1], [0, 0, 0], [2, 2, 2]]], [[1, 1], [], [2, 2, 2]], [z, z, z],
        inst=[1, 1, 1, 1], src=[0, 1, 2, 4])
    return cases
