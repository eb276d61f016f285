"""The yardstick of `ai_label_scores` (rules Q1-Q8 of ``include/autoinst_hip.h``): a NumPy restatement on pair lists, and the
fixtures tests/test_gpu_score_inst.py runs through the device.

Pure NumPy, no GPU and no library.  `ref_row` takes one row of `label_tables` -- the distinct pairs in ascending (pred, gt) order with
their counts and flags -- and walks those pairs alone: no dense (pred x gt) table is formed anywhere, so a row of 70 000 pairs costs
what its pairs cost.  `ref_dict` finishes it into `labels_api._score_tables`' dict with `_average_precision`'s own loop over the hits.
tests/test_score_inst_ref.py proves both equal to the dense host path, bit for bit, where that path is affordable.
"""
from __future__ import annotations

import os
import re
from fractions import Fraction

import numpy as np

import score_ref as sr

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "autoinst_amd", "csrc", "ai_score.hip")

OVERLAPS = [0.25, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]          # metrics_class.py:37
AP_OVERLAPS = OVERLAPS[1:]
OVERLAP_FRACTIONS = [(1, 4), (1, 2), (11, 20), (3, 5), (13, 20), (7, 10), (3, 4), (4, 5), (17, 20), (9, 10), (19, 20)]
BOUNDARY_SCALES = (1, 7, 99_991)
BOUNDARY_MISS_SCALES = (1, 7)


def constants():
    with open(_SRC) as f:
        text = f.read()
    out = {}
    for name in ("KQ_WAVE", "KQ_TAKEN_LDS", "KQ_MAX_OVERLAPS", "KS_TABLE_MIN", "KS_TABLE_MAX", "KS_LOAD_DEN", "KS_MAX_ROWS"):
        m = re.search(r"^\s*#define\s+" + name + r"\s+(\d+)\s*(?://.*)?$", text, re.M)
        if not m:
            raise RuntimeError(f"#define {name} <integer> not found in ai_score.hip")
        out[name] = int(m.group(1))
    return out


K = constants()
WAVE = K["KQ_WAVE"]
TAKEN_LDS = K["KQ_TAKEN_LDS"]
MAX_OVERLAPS = K["KQ_MAX_OVERLAPS"]
FIT_MIN = K["KS_TABLE_MIN"] // K["KS_LOAD_DEN"]
FIT_MAX = K["KS_TABLE_MAX"] // K["KS_LOAD_DEN"]


# ------------------------------------------------------------------------------------------------- Q2-Q7 on pair lists
def ref_row(pa, pb, cnt, removed, small, min_points, remove, overlaps=OVERLAPS):
    """Rules Q2-Q7 for one row: dict(hits (n_overlaps, n_pred) uint8, n_pred, n_gt_labels, gt_zero, tp (n_overlaps), s_assoc)."""
    pa, pb, cnt = np.asarray(pa, np.int64), np.asarray(pb, np.int64), np.asarray(cnt, np.int64)
    removed, small = np.asarray(removed, bool), np.asarray(small, bool)
    labels, li = np.unique(pa, return_inverse=True)
    gts, gi = np.unique(pb, return_inverse=True)
    li, gi = li.reshape(-1), gi.reshape(-1)
    ap, ag = np.zeros(labels.size, np.int64), np.zeros(gts.size, np.int64)
    np.add.at(ap, li, cnt)                                                      # Q3
    np.add.at(ag, gi, cnt)
    flagged = (removed | small) if remove else small                            # Q2
    scored_pair = (pa != 0) & ~flagged
    scored_label = np.zeros(labels.size, bool)
    scored_label[li[scored_pair]] = True
    rank = np.cumsum(scored_label) - 1
    n_pred = int(scored_label.sum())
    iou = cnt.astype(np.float64) / np.maximum(ap[li] + ag[gi] - cnt, 1).astype(np.float64)      # Q4
    hits = np.zeros((len(overlaps), n_pred), np.uint8)
    for j, o in enumerate(overlaps):                                            # Q5: the pairs are in (label, gt) order already
        taken = np.zeros(gts.size, bool)
        for q in np.flatnonzero(scored_pair & (pb != 0) & (iou >= o)):
            r = rank[li[q]]
            if hits[j, r] or taken[gi[q]]:
                continue
            taken[gi[q]] = True
            hits[j, r] = 1
    # Q7: gt-major, the association labels ascending inside a gt
    assoc_pair = (pa > 0) & ~small
    order = np.lexsort((li, gi))
    start = np.searchsorted(gi[order], np.arange(gts.size + 1))
    kept = [g for g in range(gts.size) if gts[g] != 0 and ag[g] > min_points]
    outer = 0.0
    for g in kept:
        ga, inner = int(ag[g]), 0.0
        if gts[g] > 0:
            for q in order[start[g]:start[g + 1]]:
                if assoc_pair[q]:
                    t = int(cnt[q])
                    inner += t * (t / (ga + int(ap[li[q]]) - t))
        outer += float(inner) / float(ga)
    return {"hits": hits, "n_pred": n_pred, "n_gt_labels": int((gts != 0).sum()), "gt_zero": bool((gts == 0).any()),
            "tp": hits.sum(1).astype(np.int32), "s_assoc": outer / len(kept) if kept else float("nan")}


def ap_by_the_loop(hits, n_gt_labels):
    """`labels_api._average_precision`'s loop (``metrics_class.py:181-235``) on a list of hit flags."""
    precision, recall = [1.0], [0.0]
    tp = fp = 0
    fn = int(n_gt_labels)
    for hit in hits:
        if hit:
            tp += 1
            fn -= 1
        else:
            fp += 1
        precision.append(tp / float(tp + fp))
        recall.append(tp / float(tp + fn))
    trapz = getattr(np, "trapezoid", None) or np.trapz
    return float(trapz(precision, recall))


def ref_dict(row):
    """`labels_api._score_tables`' dict from `ref_row`'s result (at `OVERLAPS`)."""
    tps, n_pred = int(row["tp"][OVERLAPS.index(0.5)]), row["n_pred"]
    n_gt = row["n_gt_labels"] if row["gt_zero"] else 0
    prec = tps / n_pred if n_pred else float("nan")
    rec = tps / n_gt if n_gt else float("nan")
    try:
        f1 = 2 * (prec * rec) / (prec + rec)
    except ZeroDivisionError:
        f1 = 0
    aps = {o: ap_by_the_loop(row["hits"][j], row["n_gt_labels"]) for j, o in enumerate(OVERLAPS)}
    ap = sum(aps[o] for o in AP_OVERLAPS) / float(len(AP_OVERLAPS))
    return {"p": prec, "r": rec, "f1": f1, "ap": ap, "ap0.25": aps[0.25], "ap0.5": aps[0.5], "S_assoc": row["s_assoc"],
            "tps": tps, "n_pred": n_pred, "n_gt": n_gt}


def ref_rows(preds, gt, threshold=0.8, min_points=200, remove=True, overlaps=OVERLAPS):
    """`ref_row` of every row of ``preds`` (k, n), the tables by `score_ref.ref_tables_fast`."""
    tables, _, _ = sr.ref_tables_fast(preds, gt, threshold, min_points)
    return [ref_row(*t, min_points, remove, overlaps) for t in tables]


def same_value(a, b):
    """Equal, or both NaN."""
    return a == b or (isinstance(a, float) and isinstance(b, float) and np.isnan(a) and np.isnan(b))


def same_dict(got, exp, what=""):
    assert set(got) == set(exp), (what, sorted(got), sorted(exp))
    for key, v in exp.items():
        assert same_value(got[key], v), (what, key, got[key], v)


# ------------------------------------------------------------------------------------------------- fixtures
def points_of(pairs):
    """(pred, gt) int32 point arrays that hold every ``(u, v, count)`` of ``pairs``."""
    pa, pb, cnt = (np.array(x, np.int64) for x in zip(*pairs))
    return np.repeat(pa, cnt).astype(np.int32), np.repeat(pb, cnt).astype(np.int32)


def random_points(seed, n=3000, negative=True, gt_zero=True, gt_labels=True):
    """One label map over a ground truth with about a third of the points on gt 0: labels that follow the truth's instances, split
    and united, some noise, and label sizes from a handful to a few hundred."""
    rng = np.random.default_rng([9, seed])
    n_inst = int(rng.integers(3, 25))
    gt = rng.integers(1, n_inst + 1, n)
    if negative:
        gt = np.where(gt % 7 == 3, -gt, gt)
    if gt_zero:
        gt = np.where(rng.random(n) < 0.35, 0, gt)
    if not gt_labels:
        gt = np.zeros(n, np.int64)
    maps = rng.integers(-3 if negative else 0, n_inst + 3, 2 * n_inst + 2)
    pred = maps[np.abs(gt) * 2 + (rng.random(n) < 0.3)]
    noise = rng.random(n) < 0.08
    pred = np.where(noise, rng.integers(-4 if negative else 0, 3 * n_inst, n), pred)
    return pred.astype(np.int32), gt.astype(np.int32)


def boundary_pairs(first_label=10):
    """For every overlap p / q of `OVERLAP_FRACTIONS` and scale c of `BOUNDARY_SCALES` a label alone on its own gt with intersection
    p c and union q c -- IoU exactly p / q, a hit at that overlap -- and for every c of `BOUNDARY_MISS_SCALES` one with intersection
    1000 p c - 1 and union 1000 q c, a miss there.  (1000 x 99 991 is left out: 20 000 x 99 991 points for one label, eleven such
    labels, is more than the 2^31 - 2 points a call takes.)  The rest of a union is gt points under label 0, which is never
    scored.  About 13 M points.  Returns (pairs, {label: (overlap index, hit expected)})."""
    pairs, what = [], {}
    u = first_label
    for j, (p, q) in enumerate(OVERLAP_FRACTIONS):
        cases = [(p * c, q * c, True) for c in BOUNDARY_SCALES] + [(1000 * p * c - 1, 1000 * q * c, False) for c in BOUNDARY_MISS_SCALES]
        for inter, union, hit in cases:
            pairs.append((u, u, inter))
            pairs.append((0, u, union - inter))
            what[u] = (j, hit)
            u += 1
    return pairs, what


def sorted_pair_arrays(pairs):
    """(pred, gt, count) arrays of a list of distinct ``(u, v, count)`` in ascending (pred, gt) order."""
    pa, pb, cnt = (np.array(x, np.int64) for x in zip(*pairs))
    order = np.lexsort((pb, pa))
    return pa[order].astype(np.int32), pb[order].astype(np.int32), cnt[order]


def quotient_is_the_literal(p, q, c):
    """(p c) / (q c) in float64 is the float64 literal of p / q, and one point less of intersection at 1000 times the scale is below."""
    lit = OVERLAPS[OVERLAP_FRACTIONS.index((p, q))]
    assert Fraction(p, q) == Fraction(str(lit))
    return np.float64(p * c) / np.float64(q * c) == np.float64(lit) and np.float64(1000 * p * c - 1) / np.float64(1000 * q * c) < np.float64(lit)


def pair_row(d, n_gt, seed=0):
    """Exactly d distinct pairs ``(u, v, count)`` over gt 0 and every one of the gts 1 .. n_gt (d >= 2 n_gt + 8), made for the
    matching to have work: label 0 (never scored) meets every gt once; every label u >= 1 has one main pair of 20-40 points on a
    gt that about two labels share -- so IoUs around 0.3-0.5 and a contest for the gt -- and up to four small pairs of 1-3 points,
    one of them often on gt 0.  Labels are added until d pairs are there; the last label is cut short."""
    rng = np.random.default_rng([5, seed, d, n_gt])
    pairs = [(0, v, 1) for v in range(n_gt + 1)]
    u = 0
    while len(pairs) < d:
        u += 1
        main = int(rng.integers(1, n_gt + 1)) if rng.random() < 0.8 else 1 + (u // 2) % n_gt
        mine = {main: int(rng.integers(20, 41))}
        for v in rng.integers(0, n_gt + 1, int(rng.integers(0, 5))):
            mine.setdefault(int(v), int(rng.integers(1, 4)))
        if rng.random() < 0.5:
            mine.setdefault(0, int(rng.integers(1, 30)))
        pairs += [(u, v, c) for v, c in sorted(mine.items())]
    return pairs[:d]


def big_rows(d, seed=0):
    """(preds (2, n), gt): row 0 has exactly d distinct pairs (d a multiple of 3), row 1 has three, over the gts 0, 1, 2.  Pair
    number i of row 0 is (1 + i // 3, i % 3) with one point; max(d, 8192) further points lie on gt 1 under label 1 and on gt 2
    under label 2 in turn, so that these two labels have an IoU above 0.5 with their gt whatever d is, and are the only ones."""
    assert d % 3 == 0
    i = np.arange(d)
    j = np.arange(max(d, 8192))
    pred = np.concatenate([1 + i // 3, 1 + j % 2])
    gt = np.concatenate([i % 3, 1 + j % 2])
    perm = np.random.default_rng([7, seed, d]).permutation(pred.size)
    preds = np.stack([pred[perm], np.full(pred.size, 9)])
    return preds.astype(np.int32), gt[perm].astype(np.int32)


def shuffled_points(pairs, seed=0):
    pred, gt = points_of(pairs)
    perm = np.random.default_rng([6, seed]).permutation(pred.size)
    return pred[perm], gt[perm]
