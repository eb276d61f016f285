"""NumPy restatement of ``ai_merge_map``'s rules M1-M10 (``include/autoinst_hip.h``): sequential, one chunk after the other,
written from the rules.  ``tests/test_merge_map_ref.py`` holds it against ``oracle/merge_ref.py`` (rule M11: with the colour
``(g, 0, 0)`` for global id ``g`` the colour-identified reference and this id-identified merge are the same function), and
``tests/test_gpu_merge_map.py`` holds the device entry against it.

``variant`` switches ONE rule to a plausible wrong one; the tests show that each is told apart from the reference:

    dedup_first     chunk 0 loses its duplicates before step 1 (M3's exception dropped)
    crop_all        a step sees every earlier point, not only the kept ones (M3)
    tie_larger      among equal iou the LARGER map id wins (M9)
    ge              iou >= iou_min qualifies (M8)
    exclusive_face  the upper face of the crop cube and of a box is exclusive (M5, M8)
    point_union     union = distinct points of both instances instead of distinct scalars (M6-M8)
    keep_own        a matched local instance keeps its provisional id (M9)
"""
from __future__ import annotations

import numpy as np

VARIANTS = ("dedup_first", "crop_all", "tie_larger", "ge", "exclusive_face", "point_union", "keep_own")
SLOTS, BLOCK, WAVE = 65536, 256, 64          # M4 / F4: 65536 slots = 256 blocks of 256 threads = four waves of 64 each


def _block_sums(v):
    """(nb * 256,) -> (nb,): per block four waves of 64, each a pairwise tree over neighbours, then ((0 + w0) + w1) + w2) + w3."""
    w = v.reshape(-1, BLOCK // WAVE, WAVE)
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    r = np.zeros(w.shape[0])
    for k in range(BLOCK // WAVE):
        r = r + w[:, k]
    return r


def f4_sum(x):
    """The float64 sum of a 1-D array in F4's order (M4): slot s = i mod 65536 adds its rows in ascending order, the slots
    of a block are summed by `_block_sums`, the 256 block sums the same way."""
    x = np.asarray(x, dtype=np.float64)
    rows = -(-x.shape[0] // SLOTS)
    pad = np.zeros(max(rows, 1) * SLOTS)
    pad[:x.shape[0]] = x
    s = np.zeros(SLOTS)
    for row in pad.reshape(-1, SLOTS):     # absent rows add +0.0, which changes no partial sum (none is -0.0: each starts at +0.0)
        s = s + row
    return float(_block_sums(_block_sums(s))[0])


def center_m4(pts):
    """M4 without a given centre: per axis `f4_sum` divided once by the count (NaN for an empty chunk)."""
    n = pts.shape[0]
    with np.errstate(invalid="ignore", divide="ignore"):
        return np.array([np.float64(f4_sum(pts[:, a])) / np.float64(n) for a in range(3)])


def _first_occurrence(xyz):
    """keep[i] = no earlier point has the same three coordinate VALUES (-0.0 == +0.0)."""
    keep = np.zeros(xyz.shape[0], dtype=bool)
    if xyz.shape[0]:
        _, first = np.unique(xyz + 0.0, axis=0, return_index=True)
        keep[first] = True
    return keep


def merge_map(points, instances, centers=None, side_length=40.0, iou_min=0.01, variant=None):
    """dict(points, inst, src, table, stats, centers).  ``table[c][l]`` = the global id local id l of chunk c ended with;
    ``stats[c]`` = (cropped map points, map instances in the crop, pairs above iou_min, local instances re-labelled), all 0 for a
    step that does nothing (chunk 0, an empty chunk, a chunk without an instance, no map before it)."""
    assert variant is None or variant in VARIANTS
    n_chunks = len(points)
    pts = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3) for p in points]
    ins = [np.asarray(i).reshape(-1).astype(np.int64) for i in instances]
    if not (side_length > 0.0) or not np.isfinite(side_length):
        raise ValueError("side_length must be positive")
    if not np.isfinite(iou_min):
        raise ValueError("iou_min is not finite")
    for c in range(n_chunks):
        if ins[c].shape[0] != pts[c].shape[0]:
            raise ValueError(f"chunk {c}: one id per point")
        if not np.isfinite(pts[c]).all():
            raise ValueError(f"chunk {c} has a coordinate that is not finite")
        if (ins[c] < 0).any():
            raise ValueError(f"chunk {c} has a negative local instance id")
        if centers is not None and not np.isfinite(np.asarray(centers[c], dtype=np.float64)).all():
            raise ValueError(f"the centre of chunk {c} is not finite")
    off = np.zeros(n_chunks + 1, dtype=np.int64)
    off[1:] = np.cumsum([p.shape[0] for p in pts])
    m = int(off[-1])
    xyz = np.concatenate(pts) if n_chunks else np.zeros((0, 3))
    loc = np.concatenate(ins) if n_chunks else np.zeros(0, dtype=np.int64)
    nloc = np.array([int(i.max()) if i.size else 0 for i in ins], dtype=np.int64)                      # M1
    goff = np.concatenate([[0], np.cumsum(nloc)]).astype(np.int64)
    table = [goff[c] + np.arange(nloc[c] + 1, dtype=np.int64) for c in range(n_chunks)]
    for t in table:
        t[0] = 0
    keep = np.ones(m, dtype=bool) if n_chunks == 1 else _first_occurrence(xyz)                           # M2
    gid = np.zeros(m, dtype=np.int64)
    stats = np.zeros((n_chunks, 4), dtype=np.int64)
    used = np.full((n_chunks, 3), np.nan)
    half = side_length / 2.0
    hi_ok = (lambda p, b: p < b) if variant == "exclusive_face" else (lambda p, b: p <= b)
    for c in range(n_chunks):
        a, b = int(off[c]), int(off[c + 1])
        used[c] = np.asarray(centers[c], dtype=np.float64) if centers is not None else center_m4(pts[c])   # M4
        if b == a:
            continue                                                                                        # M3: skipped
        if c >= 1 and a > 0 and nloc[c] > 0:
            seen = gid[:a] > 0                                                                              # M3
            if variant != "crop_all" and not (c == 1 and variant != "dedup_first"):
                seen &= keep[:a]
            lo, hi = used[c] - half, used[c] + half                                                        # M5, as written
            seen &= np.all(xyz[:a] >= lo, axis=1) & np.all(hi_ok(xyz[:a], hi), axis=1)
            mp, mg = xyz[:a][seen], gid[:a][seen]
            stats[c, 0] = mp.shape[0]
            present = np.unique(mg)                                                                         # ascending
            stats[c, 1] = present.size
            cp, cl = xyz[a:b], loc[a:b]
            best = {}                                                                                       # l -> (iou, g)
            for g in present:
                p1 = mp[mg == g]
                bmin, bmax = p1.min(0), p1.max(0)                                                           # M6
                s1 = np.unique(p1.ravel() + 0.0)
                inside = np.all(cp >= bmin, axis=1) & np.all(hi_ok(cp, bmax), axis=1)                       # M8
                count = np.bincount(cl[inside], minlength=int(nloc[c]) + 1)
                for l in np.flatnonzero(count):                                                             # only inter > 0 counts
                    if l == 0:
                        continue
                    inter = int(count[l])
                    p2 = cp[cl == l]                                                                        # M7: all of them
                    if variant == "point_union":
                        union = np.unique(np.concatenate([p1, p2]) + 0.0, axis=0).shape[0]
                    else:
                        s2 = np.unique(p2.ravel() + 0.0)
                        union = s1.size + s2.size - np.intersect1d(s1, s2).size
                    iou = float(inter) / float(union)
                    if not (iou >= iou_min if variant == "ge" else iou > iou_min):
                        continue
                    stats[c, 2] += 1
                    l = int(l)
                    old = best.get(l)                                                                       # M9: g ascends
                    if old is None or iou > old[0] or (variant == "tie_larger" and iou == old[0]):
                        best[l] = (iou, int(g))
            stats[c, 3] = len(best)
            if variant != "keep_own":
                for l, (_, g) in best.items():
                    table[c][l] = g
        gid[a:b] = table[c][loc[a:b]]
    src = np.flatnonzero(keep).astype(np.int64)
    return {"points": xyz[src], "inst": gid[src].astype(np.int32), "src": src, "table": [t.astype(np.int32) for t in table],
            "stats": stats, "centers": used}
