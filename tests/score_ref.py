"""The yardstick of `ai_label_tables` (rules S1-S5 of ``include/autoinst_hip.h``): NumPy restatements, label by label, from the rules.

Pure NumPy, no GPU and no library.  `remove_semantics` is the reference's function (``pipeline/utils/point_cloud/
point_cloud_utils.py:249-287``) said again in our own words: per distinct prediction the indices that carry it, how many of them lie
on ground truth 0, one float64 multiply and one strict comparison.  `filter_labels` is ``pipeline/metrics/metrics_class.py:302-309``.
`ref_tables` puts S1-S4 together the long way round: it filters AFTER the removal, as the scorer does, so that the flags the device
decides before the removal (S3) are checked against the two-step order.
"""
from __future__ import annotations

import numpy as np

import label_cases as lc


def remove_semantics(labels, preds, threshold=0.8):
    """A copy of ``preds`` in which a label is 0 when more than ``threshold`` of its points have ground truth (``labels``) 0."""
    labels, preds = np.asarray(labels), np.asarray(preds)
    on_ground = np.flatnonzero(labels == 0)
    out = preds.copy()
    for u in np.unique(preds):
        mine = np.flatnonzero(preds == u)
        z = int(np.isin(mine, on_ground).sum())
        if z > threshold * len(mine):
            out[mine] = 0
    return out


def filter_labels(labels, min_points):
    """A copy in which every label with fewer than ``min_points`` points is 0."""
    labels = np.asarray(labels)
    out = labels.copy()
    for u, c in zip(*np.unique(labels, return_counts=True)):
        if c < min_points:
            out[labels == u] = 0
    return out


def label_flags(pred, gt, threshold, min_points):
    """{label: (removed, small)} of one row, from m and z counted per label (S2, S3 as the header states them)."""
    pred, gt = np.asarray(pred), np.asarray(gt)
    out = {}
    for u in np.unique(pred):
        sel = pred == u
        m, z = int(sel.sum()), int((sel & (gt == 0)).sum())
        out[int(u)] = (bool(np.float64(z) > np.float64(threshold) * np.float64(m)), bool(m < min_points))
    return out


def ref_tables(preds, gt, threshold=0.8, min_points=200):
    """(tables, pred_removed, pred_scored) as `labels_api.label_tables(..., return_labels=True)` returns them: per row
    ``(pred, gt, count, removed, small)`` with the pairs by `label_cases.ref_label_pairs`; ``pred_removed`` by `remove_semantics`
    and ``pred_scored`` by `filter_labels` of that -- removal first, filter second."""
    preds = np.asarray(preds, np.int32).reshape(len(preds), -1)
    gt = np.asarray(gt, np.int32)
    tables, rem, sco = [], np.empty_like(preds), np.empty_like(preds)
    for t, p in enumerate(preds):
        pa, pb, cnt = lc.ref_label_pairs(p, gt)
        flags = label_flags(p, gt, threshold, min_points)
        tables.append((pa, pb, cnt, np.array([flags[int(u)][0] for u in pa], bool), np.array([flags[int(u)][1] for u in pa], bool)))
        rem[t] = remove_semantics(gt, p, threshold)
        sco[t] = filter_labels(rem[t], min_points)
    return tables, rem, sco


def ref_tables_fast(preds, gt, threshold=0.8, min_points=200):
    """`ref_tables` without a pass per label, for rows with many labels: m and z by ``np.unique`` / ``np.bincount`` of the label's
    rank (proven equal to `ref_tables` on the small fixtures in tests/test_score_cases.py)."""
    preds = np.asarray(preds, np.int32).reshape(len(preds), -1)
    gt = np.asarray(gt, np.int32)
    tables, rem, sco = [], np.empty_like(preds), np.empty_like(preds)
    for t, p in enumerate(preds):
        pa, pb, cnt = lc.ref_label_pairs(p, gt)
        if p.size == 0:
            tables.append((pa, pb, cnt, np.zeros(0, bool), np.zeros(0, bool)))
            continue
        u, inv = np.unique(p, return_inverse=True)
        inv = inv.reshape(-1)
        m = np.bincount(inv, minlength=u.size)
        z = np.bincount(inv[gt == 0], minlength=u.size)
        removed = z.astype(np.float64) > np.float64(threshold) * m.astype(np.float64)
        small = m < min_points
        at = np.searchsorted(u, pa)
        tables.append((pa, pb, cnt, removed[at], small[at]))
        rem[t] = np.where(removed[inv], 0, p)
        sco[t] = np.where(removed[inv] | small[inv], 0, p)
    return tables, rem, sco


def check_tables(name, got, exp):
    """Every row of ``got`` equals ``exp``: pairs, counts and flags, exactly."""
    assert len(got) == len(exp), f"{name}: {len(got)} rows instead of {len(exp)}"
    for t, (g, e) in enumerate(zip(got, exp)):
        for what, a, b in zip(("pred", "gt", "count", "removed", "small"), g, e):
            assert np.asarray(a).dtype == np.asarray(b).dtype, f"{name} row {t} {what}: dtype {np.asarray(a).dtype}"
            d = lc.first_difference(a, b)
            assert d is None, f"{name} row {t} {what}: {d}"
