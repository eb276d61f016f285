"""Host-side mirror of the reference's NCuts interface, backed by ``libautoinst_hip.so``.

Reference surface (paths relative to the reference root):

* ``normalized_cut(w, num_points_orig, labels, T=0.01, split_lim=0.01)`` --
  ``pipeline/ncuts/normalized_cut.py:37-63``: same arguments, same return type (a list of
  ``labels`` slices, groups in the recursion's emission order, members ascending);
* ``ncuts_chunk(...)`` -- ``pipeline/ncuts/ncuts_utils.py:28-204``: same signature and 5-tuple;
  its lines 60-174 (affinity + normalized cut) become one call into this module, the open3d
  glue stays as the reference wrote it and needs the reference's own ``utils`` package;
* ``get_affinity_matrix`` / ``ncuts`` -- names from the project brief that do NOT exist in the
  reference at this commit; provided as the array-level entries.

Nothing here computes on the CPU: every numeric step is a HIP kernel.  Without the shared
library or without a gfx950 device the calls raise.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np
import scipy.sparse as sp

from . import _ffi
from ._buffers import HOST, Place, cat_int32, is_device_tensor as _is_device_tensor, offsets_of, place_of, segmented
from .config import CONFIG, PROXIMITY_THRESHOLD, SPLIT_LIM

__all__ = ["Context", "DeviceGraph", "get_affinity_matrix", "build_affinity", "build_affinity_batch", "normalized_cut", "ncuts",
           "ncuts_labels", "ncuts_labels_batch", "ncuts_chunk", "default_context", "last_stats",
           "CutTree", "ncuts_tree", "ncuts_tree_batch", "relabel", "normalized_cut_sweep"]


class Context:
    """One main + one check HIP stream, workspace arena and graph-buffer cache on one GPU (``ai_ctx``).

    Not thread-safe: one per host thread (several per process are fine and are how one GPU is kept busy, see bench.py);
    ``device`` defaults to ``LOCAL_RANK``."""

    def __init__(self, device: int | None = None):
        lib = _ffi.load()
        if device is None:
            device = int(os.environ.get("LOCAL_RANK", "0"))
        h = C.c_void_p()
        _ffi.check(lib.ai_ctx_create(int(device), C.byref(h)), "ai_ctx_create")
        self._h = h
        self.device = int(device)

    def mem_info(self) -> dict:
        """Device memory the context holds between calls (``ai_ctx_mem_info``), in bytes."""
        out = (C.c_int64 * 4)()
        _ffi.check(_ffi.load().ai_ctx_mem_info(self._h, out), "ai_ctx_mem_info")
        return {"workspace": out[0], "workspace_blocks": out[1], "graphs_live": out[2], "graphs_kept": out[3]}

    def close(self):
        if getattr(self, "_h", None):
            _ffi.load().ai_ctx_destroy(self._h)
            self._h = None

    def __del__(self):
        try:
            self.close()
        except Exception:
            pass


_default_ctx = None
_last_stats: dict | None = None


def default_context() -> Context:
    global _default_ctx
    if _default_ctx is None:
        _default_ctx = Context()
    return _default_ctx


def last_stats() -> dict | None:
    """Counters and device timings of the most recent ``ai_ncut`` call of this process."""
    return _last_stats


def _has_duplicates(w: sp.csr_matrix) -> bool:
    """Whether a CSR matrix stores some (row, col) twice; reads the arrays (not SciPy's cached flags) and changes nothing."""
    if w.nnz < 2:
        return False
    step_ok = np.diff(w.indices) > 0
    starts = w.indptr[1:-1]
    step_ok[starts[(starts > 0) & (starts < w.nnz)] - 1] = True     # the step from one row into the next
    if step_ok.all():
        return False                                                # every row ascends strictly
    key = np.repeat(np.arange(w.shape[0], dtype=np.int64), np.diff(w.indptr)) * w.shape[1] + w.indices
    return np.unique(key).shape[0] != key.shape[0]


class DeviceGraph:
    """Symmetric affinity graph resident in HBM (``ai_csr``)."""

    def __init__(self, ctx: Context, handle):
        self.ctx = ctx
        self._h = handle
        n, nnz = C.c_int64(), C.c_int64()
        _ffi.check(_ffi.load().ai_csr_dims(handle, C.byref(n), C.byref(nnz)), "ai_csr_dims")
        self.n, self.nnz = int(n.value), int(nnz.value)
        self.shape = (self.n, self.n)

    @classmethod
    def from_scipy(cls, w, ctx: Context | None = None) -> "DeviceGraph":
        """Upload a SciPy matrix (``ai_csr_from_host``).  SciPy defines a matrix by its value, the device entry by what is
        stored, so duplicate entries are summed and stored zeros dropped here, on a copy; a matrix that has neither goes up as it
        is stored, columns unsorted included.  Values that are not finite or negative and a matrix that is not symmetric to the bit
        raise ``ValueError`` with the library's message ("The caller's CSR at the door")."""
        ctx = ctx or default_context()
        w = sp.csr_matrix(w)
        if w.shape[0] != w.shape[1]:
            raise ValueError("affinity matrix must be square")
        if np.any(w.data == 0) or _has_duplicates(w):
            w = w.copy()
            w.sum_duplicates()
            w.eliminate_zeros()
        indptr = np.ascontiguousarray(w.indptr, dtype=np.int64)
        indices = np.ascontiguousarray(w.indices, dtype=np.int32)
        data = np.ascontiguousarray(w.data, dtype=np.float64)
        h = C.c_void_p()
        _ffi.check(_ffi.load().ai_csr_from_host(ctx._h, w.shape[0], indptr.ctypes.data, indices.ctypes.data,
                                                data.ctypes.data, C.byref(h)), "ai_csr_from_host")
        return cls(ctx, h)

    def to_scipy(self) -> sp.csr_matrix:
        """``scipy.sparse.csr_matrix(A)`` of ``ncuts_utils.py:167``: original order, sorted columns."""
        indptr = np.empty(self.n + 1, dtype=np.int64)
        indices = np.empty(self.nnz, dtype=np.int32)
        data = np.empty(self.nnz, dtype=np.float64)
        _ffi.check(_ffi.load().ai_csr_export(self.ctx._h, self._h, indptr.ctypes.data, indices.ctypes.data,
                                             data.ctypes.data), "ai_csr_export")
        return sp.csr_matrix((data, indices, indptr), shape=self.shape)

    def free(self):
        if getattr(self, "_h", None):
            _ffi.load().ai_csr_free(self.ctx._h, self._h)
            self._h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


def _as_f64(a, cols, name, place):
    """(n, cols) float64 at `place`: a host array is converted; a torch tensor already resident in HBM is used in place, so it
    must be float64 and contiguous as it is."""
    if place.device is not None:
        if a.dtype != place.dtype(np.float64) or not a.is_contiguous() or a.dim() != 2 or (cols is not None and a.shape[1] != cols):
            raise ValueError(f"{name} on the device must be a contiguous float64 (n, {cols or 'F'}) tensor")
        return a
    a = np.ascontiguousarray(a, dtype=np.float64)
    if a.ndim != 2 or (cols is not None and a.shape[1] != cols):
        raise ValueError(f"{name} must be 2-D" + (f" with {cols} columns" if cols else ""))
    return a


def build_affinity(points, tarl=None, dino=None, *, alpha=CONFIG["alpha"], theta=CONFIG["theta"],
                   gamma=CONFIG["gamma"], radius=PROXIMITY_THRESHOLD, sam=None, beta=0.0,
                   ctx: Context | None = None) -> DeviceGraph:
    """Affinity graph of one chunk, left on the device (``ncuts_utils.py:60-67,112-167``).

    ``A_ij = 1[d_ij <= radius] * exp(-theta t_ij) * exp(-alpha d_ij) * exp(-beta s_ij) * exp(-gamma g_ij)``
    with the reference's rules: a falsy weight drops its factor, all-zero TARL rows have t = 0, A_ii = 1;
    ``s_ij`` = fraction of the views in which both points carry a SAM id and the ids differ (``sam``:
    (N, views) int ids of one camera, -1 = none; ``utils/image/image_utils.py:64-89``; beta is 0 in every
    shipped config).  Inputs are NumPy arrays (copied to the device by the call) or torch tensors that
    already live on the context's GPU (used in place; PyTorch here is only the owner of the HBM buffer).
    """
    ctx = ctx or default_context()
    # one matrix per camera (ncuts_utils.py:118-123, :128-133 loop over them); a bare array is one camera
    dino_list = list(dino) if isinstance(dino, (list, tuple)) else ([] if dino is None else [dino])
    sam_list = list(sam) if isinstance(sam, (list, tuple)) else ([] if sam is None else [sam])
    if gamma and not dino_list:
        raise ValueError("The length should be longer than 0!")  # ncuts_utils.py:126-127
    if beta and not sam_list:
        raise ValueError("The length should be longer than 0!")  # ncuts_utils.py:116-117
    dino = dino_list[0] if (gamma and dino_list) else None
    sam = sam_list[0] if (beta and sam_list) else None
    extra_dino = dino_list[1:] if gamma else []
    extra_sam = sam_list[1:] if beta else []
    if theta and tarl is None:
        raise ValueError("theta != 0 needs TARL features")
    place = place_of(points)
    i32 = place.dtype(np.int32)
    pts = _as_f64(points, 3, "points", place)
    t = _as_f64(tarl, None, "tarl", place) if theta else None
    d = _as_f64(dino, None, "dino", place) if gamma else None
    sm = None
    if place.device is not None:
        for f in (t, d):
            if f is not None and not _is_device_tensor(f):
                raise ValueError("points are on the device, so features must be too")
        if beta:
            if not _is_device_tensor(sam) or sam.dtype != i32 or not sam.is_contiguous() or sam.dim() != 2:
                raise ValueError("points are on the device, so sam must be a contiguous int32 (N, views) tensor there too")
            sm = sam
    elif beta:
        sm = np.ascontiguousarray(np.asarray(sam), dtype=np.int32)
        if sm.ndim != 2:
            raise ValueError("sam must be (N, views)")
    n = pts.shape[0]
    for f, nm in ((t, "tarl"), (d, "dino"), (sm, "sam")):
        if f is not None and f.shape[0] != n:
            raise ValueError(f"{nm} has {f.shape[0]} rows for {n} points")
    h = C.c_void_p()
    place.sync()   # the producers of the caller's buffers have finished
    st = _ffi.load().ai_affinity_build_sam(
        ctx._h, place.addr(pts), n, place.addr(t), t.shape[1] if t is not None else 0, place.addr(d), d.shape[1] if d is not None else 0,
        place.addr(sm), sm.shape[1] if sm is not None else 0, float(alpha or 0.0), float(beta or 0.0), float(gamma or 0.0),
        float(theta or 0.0), float(radius), place.mem, C.byref(h))
    _ffi.check(st, "ai_affinity_build")
    graph = DeviceGraph(ctx, h)
    for c in range(max(len(extra_dino), len(extra_sam))):
        ed = extra_dino[c] if c < len(extra_dino) else None
        es = extra_sam[c] if c < len(extra_sam) else None
        ed = _as_f64(ed, None, "dino", place) if ed is not None else None
        if place.device is not None:
            if es is not None and (not _is_device_tensor(es) or es.dtype != i32 or not es.is_contiguous()):
                raise ValueError("points are on the device, so sam must be a contiguous int32 tensor there too")
        elif es is not None:
            es = np.ascontiguousarray(np.asarray(es), dtype=np.int32)
        for f, nm in ((ed, "dino"), (es, "sam")):
            if f is not None and f.shape[0] != n:
                graph.free()
                raise ValueError(f"{nm} has {f.shape[0]} rows for {n} points")
        place.sync()
        _ffi.check(_ffi.load().ai_affinity_apply_camera(ctx._h, graph._h, place.addr(ed), ed.shape[1] if ed is not None else 0,
                                                        place.addr(es), es.shape[1] if es is not None else 0,
                                                        float(beta if es is not None else 0.0), float(gamma if ed is not None else 0.0),
                                                        place.mem), "ai_affinity_apply_camera")
    return graph


def _batch_inputs(points, tarl, dino, offsets, theta, gamma):
    """The checked inputs of `build_affinity_batch`: (place, points, tarl, dino, offsets).  Touches no library."""
    if gamma and isinstance(dino, (list, tuple)) and offsets is not None:
        raise ValueError("dino: a list is one matrix per camera, which the batched build does not take (apply the extra cameras per "
                         "graph); with offsets pass one concatenated matrix")
    if gamma and (dino is None or (isinstance(dino, (list, tuple)) and not dino)):
        raise ValueError("The length should be longer than 0!")  # ncuts_utils.py:126-127
    if theta and tarl is None:
        raise ValueError("theta != 0 needs TARL features")
    first = points if offsets is not None else next(iter(points), None)
    place = place_of(first)
    used = [(f, nm) for f, w, nm in ((tarl, theta, "tarl"), (dino, gamma, "dino")) if w]
    for f, _ in [(points, "points")] + used:
        for a in (f if isinstance(f, (list, tuple)) else [f]):
            if _is_device_tensor(a) != (place.device is not None):
                raise ValueError("host arrays and device tensors are mixed: points and features of every chunk live in one place")
    if offsets is None:
        if not isinstance(points, (list, tuple)):
            raise ValueError("points: a list of per-chunk arrays, or one array together with its offsets, is expected")
        for f, nm in used:
            if not isinstance(f, (list, tuple)) or len(f) != len(points):
                raise ValueError(f"{nm}: one matrix per chunk expected, as for points ({len(points)} chunks); a list of cameras is "
                                 "not taken here")
    pts, off = segmented(points, offsets, 3, np.float64, "points", place)
    if off.size < 2 or int(off[0]) != 0 or int(off[-1]) != int(pts.shape[0]):
        raise ValueError("offsets must start at 0, end at the number of rows and hold at least one chunk")
    out = []
    for f, w, nm in ((tarl, theta, "tarl"), (dino, gamma, "dino")):
        if not w:
            out.append(None)
            continue
        m, foff = segmented(f, offsets, None, np.float64, nm, place)
        if int(m.shape[0]) != int(pts.shape[0]) or not np.array_equal(foff, off):
            raise ValueError(f"{nm} has {int(m.shape[0])} rows for {int(pts.shape[0])} points (one feature row per point of every chunk)")
        out.append(m)
    return place, pts, out[0], out[1], off


def build_affinity_batch(points, tarl=None, dino=None, *, offsets=None, alpha=CONFIG["alpha"], theta=CONFIG["theta"],
                         gamma=CONFIG["gamma"], radius=PROXIMITY_THRESHOLD, group_rows=None, ctx: Context | None = None):
    """`build_affinity` for every chunk of a map in ONE device call (``ai_affinity_build_batch``): a list of `DeviceGraph`, each bit
    for bit the graph `build_affinity` gives for its chunk alone, whichever chunks share the call.

    ``points`` / ``tarl`` / ``dino``: one array per chunk, or the concatenated rows with ``offsets`` (C + 1) -- NumPy arrays, or
    float64 torch tensors on the context's GPU, used in place (`points_api.tarl_pool_map`'s concatenated output and its
    ``chunk_offsets`` go straight in).  ``group_rows``: rows of the chunks that are built together (None: the library's 2^21);
    it bounds the call's workspace and changes no bit.  No SAM factor and one camera: extra cameras are applied per graph."""
    place, pts, t, d, off = _batch_inputs(points, tarl, dino, offsets, theta, gamma)
    ctx = ctx or default_context()
    k = int(off.size) - 1
    hs = (C.c_void_p * k)()
    mem = place.mem
    place.sync()   # the producers of the caller's buffers have finished
    st = _ffi.load().ai_affinity_build_batch(
        ctx._h, place.addr(pts), off.ctypes.data, k, place.addr(t), t.shape[1] if t is not None else 0, place.addr(d),
        d.shape[1] if d is not None else 0, float(alpha or 0.0), float(theta or 0.0), float(gamma or 0.0), float(radius),
        int(group_rows or 0), mem, hs)
    _ffi.check(st, "ai_affinity_build_batch")
    return [DeviceGraph(ctx, C.c_void_p(h)) for h in hs]


def get_affinity_matrix(points, tarl=None, dino=None, *, alpha=CONFIG["alpha"], theta=CONFIG["theta"],
                        gamma=CONFIG["gamma"], radius=PROXIMITY_THRESHOLD, sam=None, beta=0.0,
                        ctx: Context | None = None) -> sp.csr_matrix:
    """The CSR matrix the reference hands to ``normalized_cut`` (``ncuts_utils.py:167``)."""
    g = build_affinity(points, tarl, dino, alpha=alpha, theta=theta, gamma=gamma, radius=radius, sam=sam, beta=beta, ctx=ctx)
    try:
        return g.to_scipy()
    finally:
        g.free()


def _opts(tol, max_iter, check_every, time_spmv=False, window_rows=None):
    """``time_spmv``: every SpMV launch stamps its span on the device clock (fills ``ms_spmv``).
    ``window_rows``: points of the chunks of a batched call that iterate at one time (None: the library's default)."""
    flag = 2 if time_spmv else 0
    return _ffi.NcutOpts(float(tol or 0.0), int(max_iter or 0), int(check_every or 0), flag, int(window_rows or 0))


def ncuts_labels(graph: DeviceGraph, num_points_orig: int, T: float, split_lim: float = SPLIT_LIM, *,
                 tol=None, max_iter=None, check_every=None, time_spmv=False, ctx: Context | None = None):
    """Run the recursion on a device graph; returns (labels[int32 n], n_groups, stats dict).

    ``ctx``: the context (streams, workspace) the call runs on; default: the one that built the graph.  A context serves ONE thread at a
    time: a thread that cuts graphs another thread's context built passes its own."""
    global _last_stats
    lab = np.empty(graph.n, dtype=np.int32)
    ng = C.c_int32()
    stats = _ffi.NcutStats()
    o = _opts(tol, max_iter, check_every, time_spmv)
    status = _ffi.load().ai_ncut((ctx or graph.ctx)._h, graph._h, int(num_points_orig), float(T), float(split_lim),
                                 C.byref(o), lab.ctypes.data, C.byref(ng), C.byref(stats))
    _last_stats = stats.as_dict()   # filled on AI_ERR_NO_CONVERGENCE too
    _ffi.check(status, "ai_ncut")
    return lab, int(ng.value), _last_stats


def ncuts_labels_batch(graphs, num_points_orig=None, T=CONFIG["T"], split_lim=SPLIT_LIM, *, tol=None, max_iter=None,
                       check_every=None, time_spmv=False, window_rows=None, ctx: Context | None = None):
    """`ncuts_labels` for several independent chunks in ONE call (``ai_ncut_batch``).

    The connected segments of all chunks iterate in one pool and share every kernel launch, which is
    how a GPU is kept busy by a map's many chunks; chunks beyond ``window_rows`` points wait inside the
    call and are admitted as earlier ones finish.  Returns ([labels_c], [n_groups_c], stats);
    each chunk's result is what `ncuts_labels` gives for it alone.

    ``ctx``: the context the call runs on (default: the one that built the first graph).  A context serves ONE thread at a time, so a
    thread that cuts graphs a builder thread's context has built passes its own (`sharding.run_chunks`, `bench.py`).
    """
    global _last_stats
    graphs = list(graphs)
    if not graphs:
        return [], [], None
    ctx = ctx or graphs[0].ctx
    k = len(graphs)
    norig = [g.n for g in graphs] if num_points_orig is None else [int(x) for x in num_points_orig]
    labs = [np.empty(g.n, dtype=np.int32) for g in graphs]
    gh = (C.c_void_p * k)(*[g._h for g in graphs])
    lp = (C.c_void_p * k)(*[a.ctypes.data for a in labs])
    no = (C.c_int64 * k)(*norig)
    ng = (C.c_int32 * k)()
    stats = _ffi.NcutStats()
    o = _opts(tol, max_iter, check_every, time_spmv, window_rows)
    status = _ffi.load().ai_ncut_batch(ctx._h, gh, k, no, float(T), float(split_lim), C.byref(o), lp, ng, C.byref(stats))
    _last_stats = stats.as_dict()   # filled on AI_ERR_NO_CONVERGENCE too (`last_stats()` after the exception)
    _ffi.check(status, "ai_ncut_batch")
    return labs, [int(x) for x in ng], _last_stats


# --------------------------------------------------------------------------- cut tree: every threshold from one cut
def _check_threshold(T, T_max, what="T"):
    T = float(T)
    if not np.isfinite(T):
        raise ValueError(f"{what} = {T} is not a finite threshold")
    if T > T_max:
        raise ValueError(f"{what} = {T} lies above T_max = {T_max}: the tree holds no cut that expensive (cut again at a larger T_max)")
    return T


class CutTree:
    """The recursion of one chunk at ``T_max``, flat (``ai_ncut_tree``).

    ``labels`` / ``n_groups`` are what `ncuts_labels` returns at ``T_max``.  ``cut_height[g]`` (g >= 1) is the threshold above which
    the boundary between groups g - 1 and g exists: the largest cost among the cut that made it and that cut's ancestors (a Fiedler
    cut costs its mcut, a split into connected components 0.0); ``cut_height[0]`` is -inf.  ``leaf_cost[g]`` is the mcut of the cut
    group g was refused (>= T_max, +inf where the sweep found none, NaN where the group was never solved), so ``min(leaf_cost)`` is
    the smallest threshold above ``T_max`` at which the partition would change.  Any ``T <= T_max`` is answered from these arrays;
    the comparison is strict as in the cut itself (a boundary of height h is absent at T = h), and T <= 0 gives one group."""

    def __init__(self, labels, n_groups, cut_height, leaf_cost, T_max, ctx: Context | None = None):
        self.labels = labels
        self.n_groups = int(n_groups)
        self.cut_height = np.ascontiguousarray(cut_height, dtype=np.float64)
        self.leaf_cost = None if leaf_cost is None else np.ascontiguousarray(leaf_cost, dtype=np.float64)
        self.T_max = float(T_max)
        self.ctx = ctx
        if self.cut_height.ndim != 1 or self.cut_height.shape[0] != self.n_groups:
            raise ValueError(f"cut_height has shape {self.cut_height.shape} for {self.n_groups} groups")
        if self.n_groups and self.cut_height[0] != -np.inf:
            raise ValueError("cut_height[0] must be -inf")

    def n_groups_at(self, T) -> int:
        T = _check_threshold(T, self.T_max)
        return int(np.count_nonzero(self.cut_height < T)) if self.n_groups else 0

    def labels_at(self, T):
        """The labels `ncuts_labels` gives at ``T`` (int32, where ``labels`` lives), computed on the device from the tree."""
        _check_threshold(T, self.T_max)
        return relabel([self], [T])[0][0][0]

    def groups_at(self, T, ids=None):
        """The partition at ``T`` in the form `normalized_cut` returns: a list of arrays of ``ids`` (default: row numbers)."""
        lab = self.labels_at(T)
        if _is_device_tensor(lab):
            lab = lab.cpu().numpy()
        ids = np.arange(lab.shape[0]) if ids is None else np.asarray(ids)
        if ids.shape[0] != lab.shape[0]:
            raise ValueError(f"ids has {ids.shape[0]} entries for {lab.shape[0]} points")
        return _groups_from_labels(lab, self.n_groups_at(T), ids)


def ncuts_tree(graph: DeviceGraph, num_points_orig: int, T_max: float, split_lim: float = SPLIT_LIM, *,
               tol=None, max_iter=None, check_every=None, time_spmv=False, ctx: Context | None = None) -> CutTree:
    """`ncuts_labels` at ``T_max`` that keeps what the recursion learned: a `CutTree`, which answers every T <= T_max.
    The statistics of the call are `last_stats()`."""
    global _last_stats
    ctx = ctx or graph.ctx
    lab = np.empty(graph.n, dtype=np.int32)
    hgt = np.empty(graph.n, dtype=np.float64)
    cst = np.empty(graph.n, dtype=np.float64)
    ng = C.c_int32()
    stats = _ffi.NcutStats()
    o = _opts(tol, max_iter, check_every, time_spmv)
    status = _ffi.load().ai_ncut_tree(ctx._h, graph._h, int(num_points_orig), float(T_max), float(split_lim), C.byref(o),
                                      lab.ctypes.data, C.byref(ng), hgt.ctypes.data, cst.ctypes.data, C.byref(stats))
    _last_stats = stats.as_dict()
    _ffi.check(status, "ai_ncut_tree")
    g = int(ng.value)
    return CutTree(lab, g, hgt[:g].copy(), cst[:g].copy(), T_max, ctx)


def ncuts_tree_batch(graphs, num_points_orig=None, T_max=CONFIG["T"], split_lim=SPLIT_LIM, *, tol=None, max_iter=None,
                     check_every=None, time_spmv=False, window_rows=None, ctx: Context | None = None):
    """`ncuts_labels_batch` at ``T_max`` that returns one `CutTree` per chunk (``ai_ncut_tree_batch``); each is what `ncuts_tree`
    gives for its chunk alone.  The statistics of the call are `last_stats()`."""
    global _last_stats
    graphs = list(graphs)
    if not graphs:
        return []
    ctx = ctx or graphs[0].ctx
    k = len(graphs)
    norig = [g.n for g in graphs] if num_points_orig is None else [int(x) for x in num_points_orig]
    labs = [np.empty(g.n, dtype=np.int32) for g in graphs]
    hgts = [np.empty(max(g.n, 1), dtype=np.float64) for g in graphs]
    csts = [np.empty(max(g.n, 1), dtype=np.float64) for g in graphs]
    gh = (C.c_void_p * k)(*[g._h for g in graphs])
    lp = (C.c_void_p * k)(*[a.ctypes.data for a in labs])
    hp = (C.c_void_p * k)(*[a.ctypes.data for a in hgts])
    cp = (C.c_void_p * k)(*[a.ctypes.data for a in csts])
    no = (C.c_int64 * k)(*norig)
    ng = (C.c_int32 * k)()
    stats = _ffi.NcutStats()
    o = _opts(tol, max_iter, check_every, time_spmv, window_rows)
    status = _ffi.load().ai_ncut_tree_batch(ctx._h, gh, k, no, float(T_max), float(split_lim), C.byref(o), lp, ng, hp, cp, C.byref(stats))
    _last_stats = stats.as_dict()
    _ffi.check(status, "ai_ncut_tree_batch")
    return [CutTree(labs[c], ng[c], hgts[c][:ng[c]].copy(), csts[c][:ng[c]].copy(), T_max, ctx) for c in range(k)]


def relabel(trees, thresholds, device=None, *, ctx: Context | None = None):
    """The labels of several chunks at several thresholds from their trees, in one device call (``ai_ncut_relabel``).

    ``trees``: `CutTree`s (their labels host arrays, or int32 tensors on one GPU); ``thresholds``: finite values <= every tree's
    ``T_max``.  ``device``: a torch device to upload host labels to and leave the results on (default: where the labels live).
    Returns ``(labels, n_groups)``: ``labels[t][c]`` is chunk c's label array at ``thresholds[t]`` (a view of one buffer per
    threshold), ``n_groups[t, c]`` its number of groups there."""
    trees = list(trees)
    if not trees or not all(isinstance(t, CutTree) for t in trees):
        raise ValueError("relabel: a non-empty list of CutTree objects is expected")
    thr = np.ascontiguousarray(np.atleast_1d(np.asarray(thresholds, dtype=np.float64)))
    if thr.ndim != 1 or thr.shape[0] < 1:
        raise ValueError("relabel: at least one threshold is expected")
    t_max = min(t.T_max for t in trees)
    for x in thr:
        _check_threshold(x, t_max, "threshold")
    place = place_of(*[t.labels for t in trees]) if device is None else Place(device)
    for t in trees:
        if place.device is None and _is_device_tensor(t.labels):
            raise ValueError("relabel: labels on the host and on a device are mixed")
    ctx = ctx or next((t.ctx for t in trees if t.ctx is not None), None) or default_context()
    lab = cat_int32([t.labels for t in trees], place)
    off = offsets_of([int(t.labels.shape[0]) for t in trees])
    goff = offsets_of([t.n_groups for t in trees])
    hgt = np.concatenate([t.cut_height for t in trees]) if goff[-1] else np.zeros(0, dtype=np.float64)
    if place.device is not None:
        import torch
        hgt = torch.as_tensor(hgt, device=place.device)
    n, k, nc = int(off[-1]), int(thr.shape[0]), len(trees)
    out = place.new((k, n), np.int32)
    counts = np.empty((k, nc), dtype=np.int32)
    mem = place.mem
    place.sync()
    _ffi.check(_ffi.load().ai_ncut_relabel(ctx._h, place.addr_or_null(lab), off.ctypes.data, nc, place.addr_or_null(hgt), goff.ctypes.data,
                                           float(t_max), thr.ctypes.data, k, mem, place.addr_or_null(out), counts.ctypes.data),
               "ai_ncut_relabel")
    return [[out[t, off[c]:off[c + 1]] for c in range(nc)] for t in range(k)], counts


def normalized_cut_sweep(w, num_points_orig, labels, Ts, split_lim=0.01, *, ctx: Context | None = None, tol=None, max_iter=None):
    """`normalized_cut` at every threshold of ``Ts`` for the cost of the one at ``max(Ts)``: ``{T: list[np.ndarray]}``."""
    labels = np.asarray(labels)
    Ts = [float(T) for T in Ts]
    if not Ts or not all(np.isfinite(T) for T in Ts):
        raise ValueError("normalized_cut_sweep: Ts must be a non-empty list of finite thresholds")
    own = not isinstance(w, DeviceGraph)
    g = DeviceGraph.from_scipy(w, ctx) if own else w
    try:
        if labels.shape[0] != g.n:
            raise ValueError(f"labels has {labels.shape[0]} entries for a {g.n}-row matrix")
        tree = ncuts_tree(g, int(num_points_orig), max(Ts), split_lim, tol=tol, max_iter=max_iter)
    finally:
        if own:
            g.free()
    labs, counts = relabel([tree], Ts)
    return {T: _groups_from_labels(labs[t][0], int(counts[t, 0]), labels) for t, T in enumerate(Ts)}


def _groups_from_labels(lab, ng, labels):
    order = np.argsort(lab, kind="stable")
    counts = np.bincount(lab, minlength=ng)
    return [labels[idx] for idx in np.split(order, np.cumsum(counts)[:-1])]


def normalized_cut(w, num_points_orig, labels, T=0.01, split_lim=0.01, *, ctx: Context | None = None,
                   tol=None, max_iter=None):
    """Drop-in for ``pipeline/ncuts/normalized_cut.py:37`` on the GPU.

    ``w``: SciPy sparse matrix (any format, float) or a `DeviceGraph`; ``labels``: the ids of
    w's rows.  Returns ``list[np.ndarray]`` -- a partition of ``labels``.
    """
    labels = np.asarray(labels)
    own = not isinstance(w, DeviceGraph)
    g = DeviceGraph.from_scipy(w, ctx) if own else w
    try:
        if labels.shape[0] != g.n:
            raise ValueError(f"labels has {labels.shape[0]} entries for a {g.n}-row matrix")
        lab, ng, _ = ncuts_labels(g, int(num_points_orig), T, split_lim, tol=tol, max_iter=max_iter)
    finally:
        if own:
            g.free()
    return _groups_from_labels(lab, ng, labels)


def ncuts(points, tarl=None, dino=None, *, alpha=CONFIG["alpha"], theta=CONFIG["theta"], gamma=CONFIG["gamma"],
          T=CONFIG["T"], split_lim=SPLIT_LIM, radius=PROXIMITY_THRESHOLD, sam=None, beta=0.0,
          ctx: Context | None = None, tol=None, max_iter=None):
    """Array-level ``ncuts_chunk`` lines 60-174: points (+features) -> list of index arrays."""
    g = build_affinity(points, tarl, dino, alpha=alpha, theta=theta, gamma=gamma, radius=radius, sam=sam, beta=beta, ctx=ctx)
    try:
        lab, ng, _ = ncuts_labels(g, g.n, T, split_lim, tol=tol, max_iter=max_iter)
    finally:
        g.free()
    return _groups_from_labels(lab, ng, np.arange(g.n))


def fiedler(graph: DeviceGraph, *, tol=None, max_iter=None):
    """Test hook: (lambda2, ev[n], iterations, residual) of the whole graph (``ai_fiedler``)."""
    ev = np.empty(graph.n, dtype=np.float64)
    lam, it, rs = C.c_double(), C.c_int32(), C.c_double()
    o = _opts(tol, max_iter, None)
    _ffi.check(_ffi.load().ai_fiedler(graph.ctx._h, graph._h, C.byref(o), C.byref(lam), ev.ctypes.data,
                                      C.byref(it), C.byref(rs)), "ai_fiedler")
    return float(lam.value), ev, int(it.value), float(rs.value)


def sweep(graph: DeviceGraph, ev):
    """Test hook: (costs[10], mask[n] bool, mcut) of ``get_min_ncut`` for a given ev (``ai_sweep``)."""
    ev = np.ascontiguousarray(ev, dtype=np.float64)
    costs = np.empty(_ffi.NUM_CUTS, dtype=np.float64)
    mask = np.empty(graph.n, dtype=np.uint8)
    mcut = C.c_double()
    _ffi.check(_ffi.load().ai_sweep(graph.ctx._h, graph._h, ev.ctypes.data, costs.ctypes.data, mask.ctypes.data,
                                    C.byref(mcut)), "ai_sweep")
    return costs, mask.astype(bool), float(mcut.value)


def lsym_apply(graph: DeviceGraph, x):
    """Test hook: ``L_sym @ x`` through the SpMV kernel (``ai_lsym_apply``)."""
    x = np.ascontiguousarray(x, dtype=np.float64)
    y = np.empty_like(x)
    _ffi.check(_ffi.load().ai_lsym_apply(graph.ctx._h, graph._h, x.ctypes.data, y.ctypes.data), "ai_lsym_apply")
    return y


def eigs_smallest(graph: DeviceGraph, k: int, *, tol=None, max_iter=None, check_every=None):
    """k smallest eigenpairs of L_sym (``ai_eigs_smallest``): (evals[k], evecs[n, k], steps, max residual)."""
    evals = np.empty(k, dtype=np.float64)
    vecs = np.empty((k, graph.n), dtype=np.float64)
    it, mr = C.c_int32(), C.c_double()
    o = _opts(tol, max_iter, check_every)
    _ffi.check(_ffi.load().ai_eigs_smallest(graph.ctx._h, graph._h, int(k), C.byref(o), evals.ctypes.data, vecs.ctypes.data,
                                            C.byref(it), C.byref(mr)), "ai_eigs_smallest")
    return evals, vecs.T, int(it.value), float(mr.value)


def bench_spmv(graph: DeviceGraph, reps=50):
    """(average kernel ms, algorithmic bytes per launch) of the fused Lanczos SpMV kernel."""
    ms, by = C.c_double(), C.c_double()
    _ffi.check(_ffi.load().ai_bench_spmv(graph.ctx._h, graph._h, int(reps), C.byref(ms), C.byref(by)), "ai_bench_spmv")
    return float(ms.value), float(by.value)


def bench_copy(ctx: "Context", nbytes=1 << 30, reps=10):
    """GB/s (read + written) of a plain device-to-device copy with 16-byte accesses: the box's stream rate."""
    g = C.c_double()
    _ffi.check(_ffi.load().ai_bench_copy(ctx._h, int(nbytes), int(reps), C.byref(g)), "ai_bench_copy")
    return float(g.value)


# --------------------------------------------------------------------------- reference call surface
def ncuts_chunk(dataset, chunk_downsample_dict, pcd_nonground_minor, T_pcd, sampled_indices_global,
                sequence=None, patchwise_indices=None):
    """Drop-in for ``pipeline/ncuts/ncuts_utils.py:28-204`` (same arguments, same 5-tuple).

    Must be imported from inside the reference's ``pipeline/`` tree (it uses the reference's own
    ``utils`` / ``config`` modules and open3d for everything that is not the hot path: feature
    pooling upstream, colour painting and ground handling downstream).  Lines 60-174 of the
    reference -- the dense affinity matrices, ``remove_isolated_points`` and ``normalized_cut`` --
    are replaced by `build_affinity` + `ncuts_labels`, the TARL radius-mean pooling (:136-142 ->
    chunk_generation.py:243-256) by `points_api.tarl_features_per_patch`, and the 1-NN colour
    re-projection (:185-188) by `points_api.nn1_reproject`.
    """
    import open3d as o3d  # noqa: F401  (reference dependency, not present in the build containers)
    import config as refcfg
    from utils.image.image_utils import dinov2_mean, image_based_features_per_patch
    from utils.point_cloud.chunk_generation import get_indices_feature_reprojection
    from utils.point_cloud.point_cloud_utils import get_statistical_inlier_indices, get_subpcd, transform_pcd
    from utils.visualization_utils import generate_random_colors

    cfg = refcfg.CONFIG
    first_id = patchwise_indices[sequence][0]
    center_id = chunk_downsample_dict["center_ids"][sequence]
    center_position = chunk_downsample_dict["center_positions"][sequence]
    chunk_indices = chunk_downsample_dict["indices"][sequence]
    cam_indices_global, _ = get_indices_feature_reprojection(sampled_indices_global, first_id,
                                                             adjacent_frames=refcfg.ADJACENT_FRAMES_CAM)
    tarl_indices_global, _ = get_indices_feature_reprojection(sampled_indices_global, center_id,
                                                              adjacent_frames=refcfg.ADJACENT_FRAMES_TARL)
    pcd_chunk = chunk_downsample_dict["pcd_nonground_chunks"][sequence]
    pcd_ground_chunk = chunk_downsample_dict["pcd_ground_chunks"][sequence]
    chunk_major = chunk_downsample_dict["pcd_nonground_chunks_major_downsampling"][sequence]
    points_major = np.asarray(chunk_major.points)
    num_points_major = points_major.shape[0]

    dino = sam = None
    sam_list, point2dino_list = [], []
    # the three call forms of ncuts_utils.py:69-110 (their return shapes differ)
    if cfg["beta"] and not cfg["gamma"]:
        sam_list = image_based_features_per_patch(dataset, pcd_nonground_minor, chunk_indices, chunk_major, T_pcd, cam_indices_global,
                                                  sam=True, dino=False)
    elif cfg["gamma"] and not cfg["beta"]:
        point2dino_list, _ = image_based_features_per_patch(dataset, pcd_nonground_minor, chunk_indices, chunk_major, T_pcd,
                                                            cam_indices_global, sam=False, dino=True, pcd_chunk=pcd_chunk)
    elif cfg["beta"] and cfg["gamma"]:
        sam_list, point2dino_list = image_based_features_per_patch(dataset, pcd_nonground_minor, chunk_indices, chunk_major, T_pcd,
                                                                   cam_indices_global, sam=True, dino=True)
    if cfg["beta"]:
        if len(sam_list) == 0:
            raise ValueError("The length should be longer than 0!")
        sam = [np.asarray(x) for x in sam_list]
    if cfg["gamma"]:
        feats = [dinov2_mean(p2d) for p2d in point2dino_list]
        if len(feats) == 0:
            raise ValueError("The length should be longer than 0!")
        dino = feats
    tarl = None
    if cfg["theta"]:
        # tarl_features_per_patch (chunk_generation.py:205-258): its per-point radius search and mean run on the device
        from .points_api import tarl_features_per_patch
        tarl = tarl_features_per_patch(dataset, chunk_major, T_pcd, center_position, tarl_indices_global,
                                       chunk_size=refcfg.CHUNK_SIZE, major_voxel_size=refcfg.MAJOR_VOXEL_SIZE,
                                       tarl_norm=refcfg.TARL_NORM, transform_pcd=transform_pcd)

    graph = build_affinity(points_major, tarl, dino, alpha=cfg["alpha"], theta=cfg["theta"], gamma=cfg["gamma"],
                           radius=refcfg.PROXIMITY_THRESHOLD, sam=sam, beta=cfg["beta"])
    try:
        lab, ng, _ = ncuts_labels(graph, num_points_major, cfg["T"], refcfg.SPLIT_LIM)
    finally:
        graph.free()
    grouped_labels = _groups_from_labels(lab, ng, np.arange(num_points_major))

    random_colors = generate_random_colors(600)
    pcd_color = np.zeros((num_points_major, 3))
    for i, s in enumerate(grouped_labels):
        pcd_color[s] = np.array(random_colors[i]) / 255
    pcd_chunk.paint_uniform_color([0, 0, 0])
    # kDTree_1NN_feature_reprojection (point_cloud_utils.py:144-174, a Python loop over the fine points) on the device
    from .points_api import nn1_reproject
    colors = nn1_reproject(np.asarray(pcd_chunk.colors), np.asarray(pcd_chunk.points), pcd_color, points_major)
    pcd_chunk.colors = o3d.utility.Vector3dVector(colors)

    inliers = get_statistical_inlier_indices(pcd_ground_chunk)
    ground_inliers = get_subpcd(pcd_ground_chunk, inliers)
    mean_hight = np.mean(np.asarray(ground_inliers.points)[:, 2])
    in_idcs = np.where(np.asarray(ground_inliers.points)[:, 2] < (mean_hight + refcfg.MEAN_HEIGHT))[0]
    cut_hight = get_subpcd(ground_inliers, in_idcs)
    cut_hight.paint_uniform_color([0, 0, 0])
    merged_chunk = pcd_chunk + cut_hight
    inst_ground = chunk_downsample_dict["kitti_labels"]["ground"]["instance"][sequence][inliers][in_idcs]
    seg_ground = chunk_downsample_dict["kitti_labels"]["ground"]["semantic"][sequence][inliers][in_idcs]
    return merged_chunk, pcd_chunk, cut_hight, inst_ground, seg_ground
