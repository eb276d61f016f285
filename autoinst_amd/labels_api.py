"""Host-side mirror of the scorer and of the chunk merge.

The per-point passes run on the device (``csrc/ai_labels.hip``): one contingency table of two label
arrays (`label_pairs`), the crop / bounding-box / shared-coordinate counts of one merge iteration
(`merge_associate`) and duplicate-point removal (`unique_points`).  What is left on the host is
arithmetic over instances, a few hundred numbers per map, written here in the reference's order so
that results are bit-equal:

* `Metrics` / `score` -- ``pipeline/metrics/metrics_class.py`` (``update_stats:137-179``,
  ``filter_labels:302-309``, ``get_tp_fp:60-114``, ``average_precision:181-235``,
  ``calculate_full_stats:315-340``) and ``pipeline/metrics/modified_LSTQ.py:23-80``;
* `merge_chunks_unite_instances2` -- ``pipeline/utils/point_cloud/point_cloud_utils.py:387-491``.

`merge_map` is the same merge for a whole map in one resident device call (``csrc/ai_merge.hip``, rules M1-M10 of
``include/autoinst_hip.h``), with the instance id as the identity instead of the colour.

`label_tables` is the scorer's per-point part for k label maps of one map in one device call (``csrc/ai_score.hip``, rules S1-S5):
the k contingency tables with ``remove_semantics`` and ``filter_labels`` decided per label; `remove_semantics`, `score_sweep` and
`Metrics.update_stats` on device tensors go through it.

`label_scores` is the scorer's instance-level part for the same k label maps on the device (``ai_label_scores``, rules Q1-Q8): the
greedy matching at every overlap and S_assoc from the rows' sorted pairs; the host forms AP from one hit flag per overlap and scored
label.  `score_sweep` uses it by default, and so do `score` / `Metrics.update_stats` on device tensors.

There is no CPU fallback: every function raises when the HIP library or a gfx950 device is missing.
"""
from __future__ import annotations

import numpy as np

from . import _ffi
from ._buffers import cat_int32, concat, grow, place_of
from .ncuts_api import Context, _is_device_tensor, default_context

OVERLAPS = [0.25, 0.5, 0.55, 0.6, 0.65, 0.7, 0.75, 0.8, 0.85, 0.9, 0.95]   # metrics_class.py:37
AP_OVERLAPS = OVERLAPS[1:]                                                  # :38


def _as_i32(x, what):
    a = np.asarray(x)
    if a.ndim != 1:
        raise ValueError(f"{what} must be one-dimensional")
    if a.dtype != np.int32:
        if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
            raise ValueError(f"{what} does not fit in int32")
        a = a.astype(np.int32)
    return np.ascontiguousarray(a)


def label_pairs(a, b, *, ctx: Context | None = None):
    """Distinct ``(a[i], b[i])`` pairs in ascending order with their counts: (pa, pb, count)."""
    ctx = ctx or default_context()
    a, b = _as_i32(a, "a"), _as_i32(b, "b")
    if a.shape != b.shape:
        raise ValueError("label arrays differ in length")
    lib = _ffi.load()

    def pairs(cap):
        pa, pb, cnt = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int64)
        total = _ffi.C.c_int64(0)
        _ffi.check(lib.ai_label_pairs(ctx._h, a.ctypes.data, b.ctypes.data, a.shape[0], _ffi.AI_MEM_HOST, cap, pa.ctypes.data,
                                      pb.ctypes.data, cnt.ctypes.data, _ffi.C.byref(total)), "ai_label_pairs")
        return total.value, (pa, pb, cnt)
    cap = 1 << 16
    k, (pa, pb, cnt) = grow(pairs, cap)
    return pa[:k].copy(), pb[:k].copy(), cnt[:k].copy()


class _Table:
    """Dense contingency table of (row label, gt label) with sorted label axes."""

    def __init__(self, pa, pb, cnt):
        self.rows, ri = np.unique(pa, return_inverse=True)
        self.cols, ci = np.unique(pb, return_inverse=True)
        self.m = np.zeros((self.rows.size, self.cols.size), dtype=np.int64)
        np.add.at(self.m, (ri, ci), cnt)

    def filtered(self, min_points):
        """``filter_labels`` (:302-309) applied to the row labels: instances with fewer than
        min_points points become background 0.  Returns a new table."""
        area = self.m.sum(1)
        small = area < min_points
        new_label = np.where(small, 0, self.rows)
        t = _Table.__new__(_Table)
        t.rows, ri = np.unique(new_label, return_inverse=True)
        t.cols = self.cols
        t.m = np.zeros((t.rows.size, self.cols.size), dtype=np.int64)
        np.add.at(t.m, ri, self.m)
        return t


def _iou(table):
    ap, ag = table.m.sum(1), table.m.sum(0)
    union = ap[:, None] + ag[None, :] - table.m
    return table.m / np.maximum(union, 1)       # intersection.size / union.size, :296-300


def _greedy(table, iou, thresh):
    """Matching order of ``get_tp_fp`` / ``average_precision``: predictions ascending, the first
    unused non-background gt (ascending) with IoU >= thresh."""
    used = np.zeros(table.cols.size, dtype=bool)
    gt_ok = table.cols != 0
    hits = []
    for a in range(table.rows.size):
        if table.rows[a] == 0:
            continue
        cand = np.flatnonzero((iou[a] >= thresh) & ~used & gt_ok)
        if cand.size:
            used[cand[0]] = True
            hits.append(True)
        else:
            hits.append(False)
    return hits


def _average_precision(table, iou, thresh):
    """``metrics_class.py:181-235`` with every confidence 0.5 (:193-195)."""
    precision, recall = [1.0], [0.0]
    tp = fp = 0
    fn = int((table.cols != 0).sum())
    for hit in _greedy(table, iou, thresh):
        if hit:
            tp += 1
            fn -= 1
        else:
            fp += 1
        precision.append(tp / float(tp + fp))
        recall.append(tp / float(tp + fn))
    trapz = getattr(np, "trapezoid", None) or np.trapz
    return float(trapz(precision, recall))


def _s_assoc(table, min_points):
    """``modified_LSTQ.py:23-80`` for one batch, from the (filtered all_labels, gt) table."""
    p_keep = (table.rows != 0) & (table.rows != -1)
    p_area = table.m.sum(1)
    g_area = table.m.sum(0)
    g_keep = (table.cols != 0) & (g_area > min_points)
    if not g_keep.any():
        return float("nan")
    outer = 0.0
    for g in np.flatnonzero(g_keep):
        ga = int(g_area[g])
        inner = 0.0
        if table.cols[g] > 0:
            for p in np.flatnonzero(p_keep & (table.rows > 0) & (table.m[:, g] > 0)):
                t = int(table.m[p, g])
                inner += t * (t / (ga + int(p_area[p]) - t))
        outer += float(inner) / float(ga)
    return outer / int(g_keep.sum())


def _score_tables(pred, alll, min_points):
    """The instance-level arithmetic of one ``update_stats`` from the two filtered tables."""
    iou = _iou(pred)
    tps = int(sum(_greedy(pred, iou, 0.5)))
    n_pred = int((pred.rows != 0).sum())
    n_gt = pred.cols.size - 1 if (pred.cols == 0).any() else 0          # calculate_full_stats:323-325
    prec = tps / n_pred if n_pred else float("nan")
    rec = tps / n_gt if n_gt else float("nan")
    try:
        f1 = 2 * (prec * rec) / (prec + rec)
    except ZeroDivisionError:
        f1 = 0
    aps = {o: _average_precision(pred, iou, o) for o in OVERLAPS}
    ap = sum(aps[o] for o in AP_OVERLAPS) / float(len(AP_OVERLAPS))
    return {"p": prec, "r": rec, "f1": f1, "ap": ap, "ap0.25": aps[0.25], "ap0.5": aps[0.5],
            "S_assoc": _s_assoc(alll, min_points), "tps": tps, "n_pred": n_pred, "n_gt": n_gt}


def score(all_labels, pred_labels, gt_labels, min_points=200, *, ctx: Context | None = None):
    """One ``Metrics.update_stats`` on a fresh scorer: dict(p, r, f1, ap, ap0.25, ap0.5, S_assoc)."""
    if any(_is_device_tensor(a) for a in (all_labels, pred_labels, gt_labels)):
        return _score_resident(all_labels, pred_labels, gt_labels, min_points, ctx)
    pred = _Table(*label_pairs(pred_labels, gt_labels, ctx=ctx)).filtered(min_points)
    alll = pred if all_labels is pred_labels else _Table(*label_pairs(all_labels, gt_labels, ctx=ctx)).filtered(min_points)
    return _score_tables(pred, alll, min_points)


# ----------------------------------------------------------------------------- k label maps in one call
def _stack_rows(preds, gt):
    """(place, (k, n) int32 buffer, n int32 buffer) of the label maps and the ground truth.  ``preds``: one (k, n) array or tensor,
    or a list of k one-dimensional ones; a row that is itself a list (`relabel`'s per-chunk views of one threshold) is concatenated."""
    if isinstance(preds, (list, tuple)):
        rows = list(preds)
    elif getattr(preds, "ndim", None) == 2:
        if _is_device_tensor(preds) and not preds.is_floating_point():   # already one buffer: no row is copied on its own
            place = place_of(preds)
            g = cat_int32([gt if _is_device_tensor(gt) else _as_i32(gt, "gt")], place)
            if int(preds.shape[1]) != int(g.shape[0]):
                raise ValueError("label_tables: every label map must have one label per ground-truth point")
            return place, preds.to(dtype=place.dtype(np.int32)).contiguous(), g
        rows = [preds[t] for t in range(int(preds.shape[0]))]
    else:
        raise ValueError("label_tables: preds must be a (k, n) array or tensor, or a list of k label arrays")
    place = place_of(gt, *[x for r in rows for x in (r if isinstance(r, (list, tuple)) else (r,))])
    flat = []
    for t, r in enumerate(rows):
        parts = list(r) if isinstance(r, (list, tuple)) else [r]
        for a in parts:
            if _is_device_tensor(a) and (a.is_floating_point() or a.dim() != 1):
                raise ValueError(f"label_tables: preds[{t}] must be one-dimensional integers")
        flat.append(cat_int32([a if _is_device_tensor(a) else _as_i32(a, f"preds[{t}]") for a in parts], place))
    g = cat_int32([gt if _is_device_tensor(gt) else _as_i32(gt, "gt")], place)
    n = int(g.shape[0])
    if any(int(f.shape[0]) != n for f in flat):
        raise ValueError("label_tables: every label map must have one label per ground-truth point")
    if place.device is not None:
        import torch
        stacked = torch.stack(flat).contiguous() if flat else place.zeros((0, n), np.int32)
    else:
        stacked = np.ascontiguousarray(np.stack(flat)) if flat else np.zeros((0, n), np.int32)
    return place, stacked, g


def label_tables(preds, gt, *, threshold=0.8, min_points=200, return_labels=False, ctx: Context | None = None):
    """What the scorer needs of k label maps against one ground truth, in one device call (``ai_label_tables``, rules S1-S5 of
    ``include/autoinst_hip.h``).

    ``preds``: a (k, n) array or tensor, a list of k label arrays, or `ncuts_api.relabel`'s per-threshold buffers; ``gt``: n labels.
    On the host or on one GPU.  Returns a list of k tables ``(pred, gt, count, removed, small)``: the distinct pairs of row t in
    ascending order with their int64 counts, and per pair whether ``remove_semantics`` at ``threshold`` removes its label and
    whether ``filter_labels`` at ``min_points`` finds it small.  With ``return_labels`` also ``pred_removed`` and ``pred_scored``,
    (k, n) int32 where the inputs live: the labels after the removal, and after the removal and the filter."""
    ctx = ctx or default_context()
    place, p, g = _stack_rows(preds, gt)
    k, n = int(p.shape[0]), int(g.shape[0])
    rem = place.new((k, n), np.int32) if return_labels else None
    sco = place.new((k, n), np.int32) if return_labels else None
    off = np.zeros(k + 1, dtype=np.int64)
    lib, mem = _ffi.load(), place.mem

    def tables(cap):
        pa, pb, cnt, fl = np.empty(cap, np.int32), np.empty(cap, np.int32), np.empty(cap, np.int64), np.empty(cap, np.uint8)
        place.sync()
        _ffi.check(lib.ai_label_tables(ctx._h, place.addr_or_null(p), place.addr_or_null(g), k, n, float(threshold), int(min_points),
                                       mem, cap, pa.ctypes.data, pb.ctypes.data, cnt.ctypes.data, fl.ctypes.data, off.ctypes.data,
                                       place.addr_or_null(rem), place.addr_or_null(sco)), "ai_label_tables")
        return int(off[k]), (pa, pb, cnt, fl)
    _, (pa, pb, cnt, fl) = grow(tables, 1 << 16)
    out = []
    for t in range(k):
        s = slice(int(off[t]), int(off[t + 1]))
        out.append((pa[s].copy(), pb[s].copy(), cnt[s].copy(), (fl[s] & 1).astype(bool), (fl[s] & 2).astype(bool)))
    return (out, rem, sco) if return_labels else out


def remove_semantics(labels, preds, threshold=0.8, num_threads=4, *, ctx: Context | None = None):
    """``point_cloud_utils.py:260-287`` with the reference's argument order (``labels`` is the ground truth) and return value: a copy
    of ``preds`` in which every label whose points lie on ground truth 0 by more than ``threshold`` of their number is 0 -- an array
    of ``preds``' dtype, or a tensor where ``preds`` lives.  ``num_threads`` is accepted and ignored."""
    _, rem, _ = label_tables([preds], labels, threshold=threshold, min_points=0, return_labels=True, ctx=ctx)
    if _is_device_tensor(preds):
        return rem[0].to(device=preds.device, dtype=preds.dtype)
    if _is_device_tensor(rem):
        rem = rem.cpu().numpy()
    return rem[0].astype(np.asarray(preds).dtype)


def _flagged_table(pa, pb, cnt, zero):
    """The contingency table of a label map whose labels flagged in ``zero`` (per pair) are 0."""
    return _Table(np.where(zero, 0, pa).astype(np.int32), pb, cnt)


def _sweep_scores(tables, min_points, remove):
    out = []
    for pa, pb, cnt, removed, small in tables:
        alll = _flagged_table(pa, pb, cnt, small)
        pred = _flagged_table(pa, pb, cnt, removed | small) if remove else alll
        out.append(_score_tables(pred, alll, min_points))
    return out


def _ap_from_hits(hits, n_gt_labels):
    """``average_precision`` (``metrics_class.py:181-235``, every confidence 0.5) from the hit flags of the scored labels in matching
    order (rule Q5) and the number of non-zero ground-truth labels: the precision / recall lists of `_average_precision` as arrays,
    summed by the same ``trapz``."""
    n = int(hits.size)
    if n and not n_gt_labels:
        raise ZeroDivisionError("float division by zero")         # `tp / float(tp + fn)` of the first scored label
    tp = np.cumsum(hits, dtype=np.int64)
    precision = np.concatenate([[1.0], tp / np.arange(1, n + 1, dtype=np.float64)])
    recall = np.concatenate([[0.0], tp / np.float64(max(n_gt_labels, 1))])
    trapz = getattr(np, "trapezoid", None) or np.trapz
    return float(trapz(precision, recall))


def _score_from_hits(hits, n_pred, n_gt_labels, gt_zero, tps, s_assoc):
    """`_score_tables`' dict from what ``ai_label_scores`` returns for one row: ``hits`` (len(OVERLAPS), n_pred) flags, the counts of
    rule Q6, the hits at overlap 0.5 and S_assoc."""
    n_gt = n_gt_labels if gt_zero else 0                                # calculate_full_stats:323-325
    prec = tps / n_pred if n_pred else float("nan")
    rec = tps / n_gt if n_gt else float("nan")
    try:
        f1 = 2 * (prec * rec) / (prec + rec)
    except ZeroDivisionError:
        f1 = 0
    aps = {o: _ap_from_hits(hits[j], n_gt_labels) for j, o in enumerate(OVERLAPS)}
    ap = sum(aps[o] for o in AP_OVERLAPS) / float(len(AP_OVERLAPS))
    return {"p": prec, "r": rec, "f1": f1, "ap": ap, "ap0.25": aps[0.25], "ap0.5": aps[0.5],
            "S_assoc": s_assoc, "tps": tps, "n_pred": n_pred, "n_gt": n_gt}


def _device_scores(preds, gt, threshold, min_points, remove, ctx):
    """``ai_label_scores`` at `OVERLAPS`: per row ``(hits (len(OVERLAPS), n_pred) uint8, n_pred, distinct gt != 0, whether gt 0 occurs,
    hits at 0.5, S_assoc)``, the arguments of `_score_from_hits`."""
    ctx = ctx or default_context()
    place, p, g = _stack_rows(preds, gt)
    k, n = int(p.shape[0]), int(g.shape[0])
    ov = np.asarray(OVERLAPS, dtype=np.float64)
    no = int(ov.size)
    hit_off, counts = np.zeros(k + 1, dtype=np.int64), np.zeros((k, 3), dtype=np.int32)
    tp, sa = np.zeros((k, no), dtype=np.int32), np.zeros(k, dtype=np.float64)
    lib, mem = _ffi.load(), place.mem

    def scores(cap):
        hits = np.empty(cap, np.uint8)
        place.sync()
        _ffi.check(lib.ai_label_scores(ctx._h, place.addr_or_null(p), place.addr_or_null(g), k, n, float(threshold), int(min_points), mem,
                                       1 if remove else 0, ov.ctypes.data, no, cap, hits.ctypes.data, hit_off.ctypes.data,
                                       counts.ctypes.data, tp.ctypes.data, sa.ctypes.data), "ai_label_scores")
        return int(hit_off[k]) * no, hits
    _, hits = grow(scores, 1 << 16)
    half = OVERLAPS.index(0.5)
    out = []
    for t in range(k):
        n_pred = int(counts[t, 0])
        h = hits[int(hit_off[t]) * no:int(hit_off[t + 1]) * no].reshape(no, n_pred)
        out.append((h, n_pred, int(counts[t, 1]), bool(counts[t, 2]), int(tp[t, half]), float(sa[t])))
    return out


def label_scores(preds, gt, *, threshold=0.8, min_points=200, remove=True, ctx: Context | None = None):
    """`score` of k label maps against one ground truth with the instance-level arithmetic on the device (``ai_label_scores``, rules
    Q1-Q8 of ``include/autoinst_hip.h``): a list of k dicts with `_score_tables`' keys.  ``preds`` and ``gt`` as for `label_tables`.
    The greedy matching at every overlap and S_assoc are computed from the rows' sorted pairs where they lie; the host forms the
    average precision from one hit flag per (overlap, scored label) -- NumPy's ``trapz`` is the reference's sum -- and p, r, f1."""
    return [_score_from_hits(*row) for row in _device_scores(preds, gt, threshold, min_points, remove, ctx)]


def score_sweep(preds, gt, min_points=200, *, remove=True, threshold=0.8, instance_level="device", ctx: Context | None = None):
    """`score` of k label maps against one ground truth from one device call: a list of k dicts.  With ``remove`` dict t is
    ``score(preds[t], remove_semantics(gt, preds[t], threshold), gt, min_points)``, lines 223-238 of the reference's loop; without,
    ``score(preds[t], preds[t], gt, min_points)``.  No label array crosses to the host.  ``instance_level``: ``"device"`` is
    `label_scores`; ``"host"`` takes the flagged pairs of `label_tables` to the host and runs the arithmetic there on dense tables
    (rule S4) -- the same dicts, bit for bit."""
    if instance_level == "device":
        return label_scores(preds, gt, threshold=threshold, min_points=min_points, remove=remove, ctx=ctx)
    if instance_level != "host":
        raise ValueError("score_sweep: instance_level must be 'device' or 'host'")
    return _sweep_scores(label_tables(preds, gt, threshold=threshold, min_points=min_points, ctx=ctx), min_points, remove)


def _score_resident(all_labels, pred_labels, gt_labels, min_points, ctx):
    """`score` for label arrays of which at least one is a device tensor: one ``ai_label_scores`` call without removal on the rows
    [pred, all]; the matching is the pred row's, S_assoc the all row's."""
    same = all_labels is pred_labels
    rows = _device_scores([pred_labels] if same else [pred_labels, all_labels], gt_labels, 0.0, min_points, False, ctx)
    return _score_from_hits(*rows[0][:5], rows[-1][5])


class Metrics:
    """The reference's scorer object (``metrics_class.py:15``): same constructor arguments,
    ``update_stats`` signature, return value and ``sequence_metrics`` bookkeeping; precision /
    recall accumulate over calls like ``all_tp`` / ``all_pred_size`` / ``all_gt_size`` (:321-329)."""

    def __init__(self, name="NCuts", min_points=200, thresh=0.5, *, ctx: Context | None = None):
        self.name, self.min_points, self.thresh = name, min_points, thresh
        self._ctx = ctx
        self.all_tp = self.all_pred_size = self.all_gt_size = 0
        self.s_assoc_list = []
        self.ap = {}
        self.sequence_metrics = {'ap0.5': [], 'ap0.25': [], 'ap': [], 'p': [], 'r': [], 'f1': [], 'S_assoc': []}

    def update_stats(self, all_labels, pred_labels, gt_labels, confs=[], calc_all=True, calc_lstq=True):
        """Host arrays go through `label_pairs`; with a device tensor among the three the labels stay where they are (`label_tables`)."""
        if len(confs):
            raise NotImplementedError("per-instance confidences are never passed by the reference pipeline")
        s = score(all_labels, pred_labels, gt_labels, self.min_points, ctx=self._ctx)
        self.all_tp += s["tps"]
        self.all_pred_size += s["n_pred"]
        self.all_gt_size += s["n_gt"]
        prec = self.all_tp / self.all_pred_size
        rec = self.all_tp / self.all_gt_size
        try:
            f1 = 2 * (prec * rec) / (prec + rec)
        except ZeroDivisionError:
            f1 = 0
        out = {"fScore": f1, "precision": prec, "recall": rec}
        self.s_assoc_list.append(s["S_assoc"])
        lstq = float(np.average(self.s_assoc_list))                      # modified_LSTQ.py:80
        self.ap = {o: s[k] for o, k in ((0.25, "ap0.25"), (0.5, "ap0.5"))}
        for k, v in (('p', prec), ('r', rec), ('f1', f1), ('ap0.25', s["ap0.25"]), ('ap0.5', s["ap0.5"]), ('ap', s["ap"]),
                     ('S_assoc', lstq)):
            self.sequence_metrics[k].append(v)
        return out, {"0.25": s["ap0.25"], "0.5": s["ap0.5"], "ap": s["ap"], "lstq": lstq}


# ----------------------------------------------------------------------------- chunk merge
def unique_points(points, *, ctx: Context | None = None):
    """Indices (ascending) of the first point of every distinct coordinate triple."""
    ctx = ctx or default_context()
    p = np.ascontiguousarray(points, dtype=np.float64)
    if p.ndim != 2 or p.shape[1] != 3:
        raise ValueError("points must be (N, 3)")
    keep = np.empty(p.shape[0], dtype=np.int32)
    n_keep = _ffi.C.c_int64(0)
    _ffi.check(_ffi.load().ai_unique_points(ctx._h, p.ctypes.data, p.shape[0], _ffi.AI_MEM_HOST, keep.ctypes.data,
                                            _ffi.C.byref(n_keep)), "ai_unique_points")
    return keep[: n_keep.value].copy()


def merge_associate(map_points, map_inst, chunk_points, chunk_inst, center, n_inst1, n_inst2, side_length=40.0, *,
                    ctx: Context | None = None):
    """Per-point counts of one merge iteration: dict(inter, common, n_scalars1, n_scalars2, n_points1)."""
    ctx = ctx or default_context()
    mp = np.ascontiguousarray(map_points, dtype=np.float64)
    cp = np.ascontiguousarray(chunk_points, dtype=np.float64)
    mi, ci = _as_i32(map_inst, "map_inst"), _as_i32(chunk_inst, "chunk_inst")
    if mp.ndim != 2 or mp.shape[1] != 3 or cp.ndim != 2 or cp.shape[1] != 3 or mi.shape[0] != mp.shape[0] or ci.shape[0] != cp.shape[0]:
        raise ValueError("points must be (N, 3) with one instance id per point")
    c = np.ascontiguousarray(center, dtype=np.float64)
    inter = np.empty((n_inst1, n_inst2), np.int32)
    common = np.empty((n_inst1, n_inst2), np.int32)
    ns1, ns2, np1 = np.empty(n_inst1, np.int32), np.empty(n_inst2, np.int32), np.empty(n_inst1, np.int32)
    _ffi.check(_ffi.load().ai_merge_associate(ctx._h, mp.ctypes.data, mi.ctypes.data, mp.shape[0], cp.ctypes.data, ci.ctypes.data,
                                              cp.shape[0], c.ctypes.data, float(side_length), n_inst1, n_inst2, _ffi.AI_MEM_HOST,
                                              inter.ctypes.data, common.ctypes.data, ns1.ctypes.data, ns2.ctypes.data, np1.ctypes.data),
               "ai_merge_associate")
    return {"inter": inter, "common": common, "n_scalars1": ns1, "n_scalars2": ns2, "n_points1": np1}


def _color_ids(colors):
    """(unique colours in np.unique(axis=0) order with black first if present, id per point);
    id 0 is reserved for black = street (:430, :438), instances are 1.. in lexicographic order."""
    c = np.ascontiguousarray(colors, dtype=np.float64)
    key = (c + 0.0).view(np.dtype((np.void, 24))).ravel()           # + 0.0 folds -0.0 into +0.0
    ukey, first, inv = np.unique(key, return_index=True, return_inverse=True)
    ucol = c[first]
    order = np.lexsort((ucol[:, 2], ucol[:, 1], ucol[:, 0]))          # numeric lexicographic, as np.unique(axis=0)
    black = np.all(ucol[order] == 0.0, axis=1)
    order = np.concatenate([order[black], order[~black]])
    rank = np.empty(order.size, dtype=np.int32)
    rank[order] = np.arange(order.size, dtype=np.int32) + (0 if black.any() else 1)
    table = np.zeros((order.size + (0 if black.any() else 1), 3))
    table[rank] = ucol
    return table, rank[inv.ravel()]


def _points_colors(chunk):
    if isinstance(chunk, (tuple, list)):
        return np.asarray(chunk[0], dtype=np.float64), np.asarray(chunk[1], dtype=np.float64)
    return np.asarray(chunk.points, dtype=np.float64), np.asarray(chunk.colors, dtype=np.float64)   # open3d-like


def merge_chunks_unite_instances2(chunks, icp=False, *, ctx: Context | None = None):
    """``point_cloud_utils.py:387-491`` on arrays: ``chunks`` is a list of ``(points, colors)`` pairs
    (or objects with ``.points`` / ``.colors``); returns the merged ``(points, colors)``.

    Instance identity is the colour, as in the reference.  Per new chunk the device does the crop,
    the boxes, the inside counts, the shared-coordinate counts and the duplicate removal; the
    association (:444-477) runs here over the few candidate pairs.
    """
    merge_p, merge_c = _points_colors(chunks[0])
    merge_p, merge_c = merge_p.copy(), merge_c.copy()
    for chunk in chunks[1:]:
        new_p, new_c = _points_colors(chunk)
        center = np.array([new_p[:, 0].mean(), new_p[:, 1].mean(), new_p[:, 2].mean()])      # :397-403
        table1, inst1 = _color_ids(merge_c)
        table2, inst2 = _color_ids(new_c)
        r = merge_associate(merge_p, inst1, new_p, inst2, center, table1.shape[0], table2.shape[0], 40.0, ctx=ctx)
        inter = r["inter"].astype(np.int64)
        union = r["n_scalars1"].astype(np.int64)[:, None] + r["n_scalars2"].astype(np.int64)[None, :] - r["common"]
        ids_chunk_1, ids_chunk_2, ious = [], [], []
        for id1, id2 in np.argwhere(inter > 0):                                               # row-major = the loops of :446-463
            iou = float(inter[id1, id2]) / float(union[id1, id2])
            if not iou > 0.01:
                continue
            if id2 not in ids_chunk_2:                                                        # :465-477
                ids_chunk_1.append(id1)
                ids_chunk_2.append(id2)
                ious.append(iou)
            else:
                i = ids_chunk_2.index(id2)
                if iou > ious[i]:
                    ious[i] = iou
                    ids_chunk_1[i] = id1
        colors_2 = new_c.copy()
        for id1, id2 in zip(ids_chunk_1, ids_chunk_2):                                        # :479-481
            colors_2[inst2 == id2] = table1[id1]
        merge_p = np.concatenate([merge_p, new_p])                                            # :488
        merge_c = np.concatenate([merge_c, colors_2])
        keep = unique_points(merge_p, ctx=ctx)                                                # :489
        merge_p, merge_c = merge_p[keep], merge_c[keep]
    return merge_p, merge_c


MERGE_STATS = ("cropped_points", "map_instances", "pairs", "relabelled")   # ai_merge_map's stats, per chunk


def merge_map(points, instances, *, centers=None, side_length=40.0, iou_min=0.01, return_table=False, return_stats=False,
              ctx: Context | None = None):
    """``merge_chunks_unite_instances2`` for all chunks of a map in one device call (``ai_merge_map``, rules M1-M10 in
    ``include/autoinst_hip.h``), the instance id being the identity: ``(points, instance, source)``.

    ``points`` / ``instances``: one (n, 3) float64 array or device tensor and one integer id per point and chunk; ids are
    chunk-local, 0 is "no instance" (`points_api.finish_chunks`' ``merged_points`` / ``merged_instance``).  ``centers``: one crop
    centre per chunk, or ``None`` for the chunk means (M4).  Returns the merged points (first occurrences of the concatenation, in
    order), their int32 global instance id (local id ``l`` of chunk ``c`` starts as ``sum(max id of chunks < c) + l`` and takes the
    id of the map instance it was united with) and ``source`` (int64): the position of every merged point in the concatenation, so
    that ``cat(per_chunk_values)[source]`` carries any per-point value -- ground-truth labels for one -- into the merged map's
    order.  With ``return_table`` a fourth value, a list with one int32 array per chunk: entry ``l`` is the global id local id
    ``l`` ended with; with ``return_stats`` a last value, an (n_chunks, 4) int64 array (`MERGE_STATS`).  Device tensors in give
    device tensors out; only counts cross to the host.  Errors of M10 raise ``ValueError``."""
    ctx = ctx or default_context()
    if not isinstance(points, (list, tuple)) or not isinstance(instances, (list, tuple)) or len(points) != len(instances):
        raise ValueError("merge_map: points and instances must be lists with one entry per chunk")
    n = len(points)
    place = place_of(*points, *instances)
    xyz, off = concat(list(points), 3, np.float64, "points", place)
    m = int(off[-1])
    parts = []
    for c, a in enumerate(instances):
        if _is_device_tensor(a):
            a = a.reshape(-1)
            if a.is_floating_point():
                raise ValueError(f"merge_map: instances[{c}] must be integers")
        else:
            a = np.asarray(a).reshape(-1)
            if a.size and not np.issubdtype(a.dtype, np.integer):
                raise ValueError(f"merge_map: instances[{c}] must be integers")
            if a.size and (a.min() < -2 ** 31 or a.max() >= 2 ** 31):
                raise ValueError(f"merge_map: instances[{c}] does not fit in int32")
        if int(a.shape[0]) != int(off[c + 1] - off[c]):
            raise ValueError(f"merge_map: instances[{c}] has {int(a.shape[0])} entries for {int(off[c + 1] - off[c])} points")
        parts.append(a)
    cen = None
    if centers is not None:
        cen = np.ascontiguousarray(centers, dtype=np.float64)
        if cen.shape != (n, 3):
            raise ValueError("merge_map: centers must be (n_chunks, 3)")
    inst = cat_int32(parts, place)
    out_p, out_i, out_s = place.new((max(m, 1), 3), np.float64), place.new(max(m, 1), np.int32), place.new(max(m, 1), np.int64)
    table = stats = None
    if return_table:
        nmax = [int(inst[off[c]:off[c + 1]].max()) if off[c + 1] > off[c] else 0 for c in range(n)]
        goff = np.concatenate([[0], np.cumsum(np.maximum(nmax, 0), dtype=np.int64)]).astype(np.int64)
        table = np.zeros(int(goff[-1]) + 1, dtype=np.int32)
    if return_stats:
        stats = np.zeros((n, len(MERGE_STATS)), dtype=np.int64)
    n_out = _ffi.C.c_int64(0)
    # an empty input is NULL; the outputs are never NULL
    place.sync()
    _ffi.check(_ffi.load().ai_merge_map(
        ctx._h, place.addr_or_null(xyz), place.addr_or_null(inst), off.ctypes.data, n, cen.ctypes.data if cen is not None else None,
        float(side_length), float(iou_min), place.mem, place.addr(out_p), place.addr(out_i), place.addr(out_s), _ffi.C.byref(n_out),
        table.ctypes.data if table is not None else None, stats.ctypes.data if stats is not None else None, None), "ai_merge_map")
    k = int(n_out.value)
    res = [out_p[:k], out_i[:k], out_s[:k]]
    if return_table:
        res.append([np.concatenate([[0], table[goff[c] + 1:goff[c + 1] + 1]]).astype(np.int32) for c in range(n)])
    if return_stats:
        res.append(stats)
    return tuple(res)
