"""Fixtures, host models and truths for the chunk preparation (``autoinst_amd/csrc/ai_prep.hip``: `ai_box_select`,
`ai_statistical_inliers`, `ai_voxel_down_sample`) at its kernel limits.

Plain NumPy, seeded, no GPU and no library: tests/test_prep_cases.py proves on the CPU that every fixture sits in the regime its
name claims and that a list of deliberately wrong rules is rejected; tests/test_gpu_prep_cases.py feeds the device's answers to
the same truths.

The limits are READ from the sources (`constants`): a changed constant moves the fixtures with it, and the CPU test proves the
regime claims again.

Models (they restate the device code, grid and all):

* `knn_grid` / `kcells` restate the host grid of `ai_statistical_inliers` (bounds, thin-axis volume, cube root, growth loop,
  nx / ny / nz) and `kcell_of`;
* `knn_model` restates `kq_knn_avg`'s ring search with a pluggable stop rule: ``"shipped"`` (`kp_nn1`'s face bound with its
  counted slack, for the k-th best) or ``"parent"`` (``sqrt(kth) <= r * cell``, the rule before the rounding of `kcell_of` was
  counted);
* `box_model` restates `kb_count` / the scan / `kb_fill` (tiles, waves, ballot ranks, the ``cap`` guard);
* `voxel_keys` / `voxel_model` restate the host part of `ai_voxel_down_sample` (vmin, the bit counts, the refusals), `kv_keys`,
  the stable sort and `kv_mean`.

Truths (no grid): `knn_avg_exact` (the full matrix of plain squares, the k smallest, ``np.sqrt``, sequential ascending sum, one
division), `prep_ref.box_select`, `prep_ref.voxel_down_sample`, and `stats_ref` (``math.fsum`` over ``avg > 0``), against which
the device's fixed-order sums are bounded by `stats_bound`.
"""
from __future__ import annotations

import functools
import math
import os
import re
from dataclasses import dataclass, field

import numpy as np

import prep_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "autoinst_amd", "csrc")
EPS = float(np.finfo(np.float64).eps)      # 2^-52, the kernels' `eps`
U = 2.0 ** -53                             # the unit roundoff
INT_MAX = 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------- constants from the sources
def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _groups(text, pattern, what):
    m = re.search(pattern, text, re.M)
    if not m:
        raise RuntimeError(f"{what} not found in the sources")
    return m.groups()


def _find(text, pattern, what):
    return _groups(text, pattern, what)[0]


_SLACK = r"const double slack = ([0-9.]+) \* eps \* fmax\(fmax\(axis_mag\(x, g\.minx, %s, g\.nx\)"
_STOP = r"sqrt\(%s\) \* \(1\.0 \+ ([0-9.]+) \* eps\) <= lb"


def stop_constants(text, cell, best, what):
    """(slack ulps, stop ulps) of one ring search's stop rule."""
    return (float(_find(text, _SLACK % cell, f"the slack of {what}")), float(_find(text, _STOP % best, f"the stop rule of {what}")))


def constants():
    """The limits of the three entries, parsed out of ``ai_common.h`` and ``ai_prep.hip``."""
    common, prep = _read(_CSRC, "ai_common.h"), _read(_CSRC, "ai_prep.hip")
    ka, kb, kc, kd, ke = _groups(prep, r"if \(k <= (\d+)\)\s*hipLaunchKernelGGL\(kq_knn_avg<(\d+)>, KQ_ARGS\);\s*else if \(k <= (\d+)\)\s*"
                                 r"hipLaunchKernelGGL\(kq_knn_avg<(\d+)>, KQ_ARGS\);\s*else\s*hipLaunchKernelGGL\(kq_knn_avg<(\d+)>",
                                 "the template instances of kq_knn_avg")
    if ka != kb or kc != kd:
        raise RuntimeError("an instance of kq_knn_avg no longer serves k up to its own length")
    kmax, nmax = _groups(prep, r"nb_neighbors > (\d+) && n > (\d+)", "the largest k of ai_statistical_inliers")
    if not (int(kmax) == int(nmax) == int(ke)):
        raise RuntimeError("the largest k is no longer the longest instance of kq_knn_avg")
    row_a, row_b = _groups(prep, r"fy \* fz <= ([0-9.]+) \* \(double\)n \+ ([0-9.]+)\)", "the row cap of the kNN grid")
    thin_rel, thin_abs = _groups(prep, r"std::max\(ext\[a\], std::max\(([0-9.e-]+) \* emax, ([0-9.e-]+)\)\)", "the thin-axis floors")
    slack, stop = stop_constants(prep, r"g\.cell", "kth", "kq_knn_avg")
    c = dict(AI_BLOCK=int(_find(common, r"^\s*#define\s+AI_BLOCK\s+(\d+)", "AI_BLOCK")),
             RED_BLOCKS=int(_find(prep, r"constexpr int RED_BLOCKS = (\d+);", "RED_BLOCKS")),
             KNN_LENGTHS=(int(ka), int(kc), int(ke)),
             GROW=float(_find(prep, r"^\s*cell \*= ([0-9.]+);", "the growth factor of the kNN grid")),
             ROW_CAP=(float(row_a), float(row_b)),
             X_CAP=float(_find(prep, r"if \(fx < ([0-9.e]+) &&", "the x-cell cap of the kNN grid")),
             THIN_REL=float(thin_rel), THIN_ABS=float(thin_abs),
             EXTENT_LIMIT=float(_find(prep, r"mx\[a\] - mn\[a\] < ([0-9.e+]+)\)", "the extent limit of bounds()")),
             MAX_BOXES=int(_find(prep, r"n_boxes > (\d+)", "the box limit of ai_box_select")),
             MAX_KEY_BITS=int(_find(prep, r"bits\[0\] \+ bits\[1\] \+ bits\[2\] > (\d+)", "the key bits of ai_voxel_down_sample")),
             SLACK_ULPS=slack, STOP_ULPS=stop)
    if c["AI_BLOCK"] % 64 or c["RED_BLOCKS"] != c["AI_BLOCK"]:
        raise RuntimeError("kq_finish no longer takes one partial per thread of a block of whole waves")
    return c


K = constants()
BLOCK = K["AI_BLOCK"]
WAVE = 64
RED_BLOCKS = K["RED_BLOCKS"]
KNN_LENGTHS = K["KNN_LENGTHS"]
MAX_K = KNN_LENGTHS[-1]
LAP = RED_BLOCKS * BLOCK                  # points one lap of kq_partial's grid-stride loop covers
MAX_BOXES = K["MAX_BOXES"]


def knn_instance(k):
    """The compile-time list length of the `kq_knn_avg` instance that serves k."""
    return next(length for length in KNN_LENGTHS if k <= length)


# ------------------------------------------------------------------------------------------------- squares, as sq_dist3
def sq_plain(a, b):
    """(dx*dx + dy*dy) + dz*dz, every product and sum rounded on its own (broadcasts over the leading axes)."""
    d = np.asarray(a, dtype=np.float64) - np.asarray(b, dtype=np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _seq_mean(d, k):
    s = d[:, 0].copy()
    for j in range(1, d.shape[1]):
        s = s + d[:, j]
    return s / float(k)


AVG_MUTANTS = ("sum_before_sort", "divide_by_nb")


def knn_avg_exact(points, nb_neighbors, groups=None, mutant=None, block=512):
    """The truth, no grid: per point the k = min(nb_neighbors, n) smallest plain squares of the full matrix (the point itself
    included), ``np.sqrt`` of each, summed one after the other in ascending order, one division by k.

    ``groups`` (one id per point) says that the cloud falls into far-apart groups, each holding every k-nearest neighbour of its
    own members: the matrix is then formed per group.  The claim is checked, not trusted: k points must fit a group, and every
    group's bounding box must lie farther from every other box than its own diagonal is long.
    ``mutant``: ``"sum_before_sort"`` adds the k distances in descending order; ``"divide_by_nb"`` divides by nb_neighbors."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    k = min(int(nb_neighbors), n)
    div = nb_neighbors if mutant == "divide_by_nb" else k
    avg = np.empty(n)
    if groups is None:
        parts = [np.arange(n)]
    else:
        groups = np.asarray(groups)
        ids = np.unique(groups)
        parts = [np.flatnonzero(groups == g) for g in ids]
        lo = np.array([p[m].min(axis=0) for m in parts])
        hi = np.array([p[m].max(axis=0) for m in parts])
        diag = np.sqrt(((hi - lo) ** 2).sum(axis=1))
        gap = np.maximum(np.maximum(lo[:, None, :] - hi[None, :, :], lo[None, :, :] - hi[:, None, :]), 0.0)
        apart = np.sqrt((gap ** 2).sum(axis=2))
        np.fill_diagonal(apart, np.inf)
        if min(m.size for m in parts) < k or not (apart.min(axis=1) > 1.001 * diag).all():
            raise ValueError("the groups do not hold their members' k nearest neighbours")
    for m in parts:
        q = p[m]
        for a in range(0, q.shape[0], block):
            d2 = sq_plain(q[a:a + block, None, :], q[None, :, :])
            best = np.sort(np.partition(d2, k - 1, axis=1)[:, :k], axis=1)
            d = np.sqrt(best)
            avg[m[a:a + block]] = _seq_mean(d[:, ::-1] if mutant == "sum_before_sort" else d, div)
    return avg


# ------------------------------------------------------------------------------------------------- the grid of the kNN
@dataclass
class KGrid:
    mn: np.ndarray          # (3,)
    mx: np.ndarray
    cell: float             # the grown cell
    cell0: float            # the cube root of the volume per point
    n: np.ndarray           # (3,) int64: nx, ny, nz
    steps: int              # how often the growth loop multiplied the cell

    @property
    def inv(self):
        return 1.0 / self.cell

    @property
    def rows(self):
        return int(self.n[1] * self.n[2])


def _host_cbrt():
    """The C library's ``cbrt``, which is what ``std::cbrt`` calls on the host.  It is not correctly rounded, and ``np.cbrt`` is
    another function (it differs in the last bit for nearly half of all arguments): a model of the grid that is to put a point
    on a cell border needs the same one.  ``math.cbrt`` (Python 3.11) is the C library's; before that, ctypes reaches it."""
    if hasattr(math, "cbrt"):
        return math.cbrt
    import ctypes
    import ctypes.util
    f = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").cbrt
    f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double]
    return f


host_cbrt = _host_cbrt()


def knn_grids(clouds, grow=True, cbrt=None):
    """The host part of `ai_statistical_inliers` for T clouds (T, n, 3) at once: (mn (T, 3), mx, cell (T,), cell0, n (T, 3) int64,
    steps (T,)).  Bounds (non-finite coordinates and extents of 1e15 are refused), the volume with thin axes floored, multiplied
    in axis order, the cube root per point, the growth loop, nx / ny / nz.  ``grow=False`` is a wrong rule."""
    p = np.asarray(clouds, dtype=np.float64)
    n = p.shape[1]
    if not np.isfinite(p).all():
        raise ValueError("coordinates are not finite")
    mn, mx = p.min(axis=1), p.max(axis=1)
    ext = mx - mn
    if not (ext < K["EXTENT_LIMIT"]).all():
        raise ValueError("coordinates are not finite")
    floor_ = np.maximum(K["THIN_REL"] * ext.max(axis=1), K["THIN_ABS"])
    vol = np.ones(p.shape[0])
    for a in range(3):
        vol = vol * np.maximum(ext[:, a], floor_)
    cell0 = np.array([(cbrt or host_cbrt)(float(x)) for x in vol / float(n)])
    cell, steps = cell0.copy(), np.zeros(p.shape[0], np.int64)
    while True:
        f = np.floor(ext / cell[:, None]) + 1.0
        big = ~((f[:, 0] < K["X_CAP"]) & (f[:, 1] * f[:, 2] <= K["ROW_CAP"][0] * float(n) + K["ROW_CAP"][1]))
        if not grow or not big.any():
            break
        cell = np.where(big, cell * K["GROW"], cell)
        steps += big
    return mn, mx, cell, cell0, f.astype(np.int64), steps


def knn_grid(points, grow=True, cbrt=None):
    """`knn_grids` for one cloud (n, 3), as a `KGrid`.  ``cbrt`` replaces the C library's cube root (the issue's example was found
    with ``np.cbrt``)."""
    mn, mx, cell, cell0, n, steps = knn_grids(np.asarray(points, dtype=np.float64).reshape(1, -1, 3), grow, cbrt)
    return KGrid(mn[0], mx[0], float(cell[0]), float(cell0[0]), n[0], int(steps[0]))


def kcells(g, points, clamp=True):
    """`kcell_of`: floor((p - min) * inv_cell), clamped to the grid."""
    p = np.asarray(points, dtype=np.float64)
    c = np.floor((p - g.mn) * g.inv).astype(np.int64)
    return np.clip(c, 0, g.n - 1) if clamp else c


# ------------------------------------------------------------------------------------------------- kq_knn_avg, ring by ring
def _col(cell):
    c = np.asarray(cell, dtype=np.float64)
    return c[:, None] if c.ndim else c


def _stop_parent(mn, nn, cell, q, qc, r, kth):
    return np.sqrt(kth) <= float(r) * cell


def stop_slack(mn, nn, cell, q):
    """The slack of `kq_knn_avg`: SLACK_ULPS ulps of the largest |min| + (n + 1) * cell + |x| over the axes.  One grid (mn, nn
    of shape (3,), a scalar cell) for all queries q (t, 3), or a grid per query ((t, 3), (t, 3), (t,))."""
    mag = ((np.abs(mn) + (nn + 1).astype(np.float64) * _col(cell)) + np.abs(q)).max(axis=1)
    return K["SLACK_ULPS"] * EPS * mag


def face_bound(mn, nn, cell, q, qc, r):
    """min over the axes of `face_gap`: the distance to the nearest face of the box of rings 0..r that has cells beyond it."""
    c = _col(cell)
    with np.errstate(invalid="ignore"):
        lo = np.where(qc - r - 1 >= 0, q - (mn + (qc - r).astype(np.float64) * c), np.inf)
        hi = np.where(qc + r + 1 <= nn - 1, (mn + (qc + r + 1).astype(np.float64) * c) - q, np.inf)
    return np.fmin(lo, hi).min(axis=1)


def _stop_shipped(mn, nn, cell, q, qc, r, kth):
    return np.sqrt(kth) * (1.0 + K["STOP_ULPS"] * EPS) <= face_bound(mn, nn, cell, q, qc, r) - stop_slack(mn, nn, cell, q)


STOP_RULES = {"parent": _stop_parent, "shipped": _stop_shipped}
KNN_MUTANTS = ("no_clamp",)


def knn_model(points, nb_neighbors, *, stop="shipped", mutant=None, grid=None, chunk=512):
    """`kq_knn_avg` on the CPU: dict(avg, rings, grid).  Ring r of a query is every point whose STORED cell lies at Chebyshev
    distance r from the query's cell; the model keeps the k smallest plain squares seen, and once k points have been seen asks
    the stop rule after each ring, up to ring max(nx, ny, nz).  avg = the k square roots summed in ascending order / k.
    ``mutant="no_clamp"``: `kcell_of` without its clamp -- a point whose index leaves the grid lies in no row that is searched."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    k = min(int(nb_neighbors), n)
    g = knn_grid(p) if grid is None else grid
    cells = kcells(g, p, clamp=mutant != "no_clamp")
    stored = ((cells >= 0) & (cells <= g.n - 1)).all(axis=1)
    rule = STOP_RULES[stop]
    rmax = int(g.n.max())
    avg, rings = np.empty(n), np.empty(n, np.int64)
    for a in range(0, n, chunk):
        q, qc = p[a:a + chunk], cells[a:a + chunk]
        t = q.shape[0]
        ring = np.abs(cells[None, :, :] - qc[:, None, :]).max(axis=2)
        ring = np.where(stored[None, :], ring, rmax + 1)
        d2 = sq_plain(q[:, None, :], p[None, :, :])
        best = np.full((t, k), np.inf)
        used = np.zeros(t, np.int64)
        live = np.arange(t)
        for r in range(rmax + 1):
            vis = ring[live] <= r
            d2m = np.where(vis, d2[live], np.inf)
            b = np.sort(np.partition(d2m, k - 1, axis=1)[:, :k], axis=1)
            best[live], used[live] = b, r
            with np.errstate(invalid="ignore", over="ignore"):
                done = (vis.sum(axis=1) >= k) & rule(g.mn, g.n, g.cell, q[live], qc[live], r, b[:, k - 1])
            live = live[~done]
            if live.size == 0:
                break
        with np.errstate(invalid="ignore"):
            avg[a:a + chunk] = _seq_mean(np.sqrt(best), k)
        rings[a:a + chunk] = used
    return {"avg": avg, "rings": rings, "grid": g}


# ------------------------------------------------------------------------------------------------- statistics
STATS_MUTANTS = ("keep_zero", "mean_over_positive", "std_with_n", "le_threshold")


def stats_ref(avg, std_ratio, mutant=None):
    """dict(mean, std, threshold, keep) by open3d's rules with correctly rounded sums: ``mean = fsum(avg > 0) / n`` (the
    ``avg == 0`` points count in the denominator), ``std = sqrt(fsum((avg - mean)^2 over avg > 0) / (n - 1))``, kept iff
    ``0 < avg < mean + std_ratio * std``.  ``mutant`` breaks one rule on purpose."""
    a = np.asarray(avg, dtype=np.float64)
    n = a.shape[0]
    pos = a[a > 0]
    mean = math.fsum(pos) / float(pos.size if mutant == "mean_over_positive" else n)
    dev = pos - mean
    den = float(n if mutant == "std_with_n" else n - 1)
    tot = math.fsum(dev * dev)
    std = math.sqrt(tot / den) if den > 0 else float("nan")
    thr = mean + std_ratio * std
    with np.errstate(invalid="ignore"):
        low = a >= 0 if mutant == "keep_zero" else a > 0
        keep = np.flatnonzero(low & (a <= thr if mutant == "le_threshold" else a < thr))
    return {"mean": mean, "std": std, "threshold": thr, "keep": keep}


def _block_sum(v):
    """`ai_block_sum_first` over the last axis (AI_BLOCK values): per wave the pairwise tree over the lanes (neighbours, pairs
    of 2, 4, ..., 32), then ((0 + w0) + w1) + w2 + w3 in wave order."""
    w = v.reshape(v.shape[:-1] + (BLOCK // WAVE, WAVE))
    while w.shape[-1] > 1:
        w = w[..., 0::2] + w[..., 1::2]
    w = w[..., 0]
    r = np.zeros(w.shape[:-1])
    for i in range(BLOCK // WAVE):
        r = r + w[..., i]
    return r


def _device_total(terms):
    """`kq_partial` + `kq_finish`: thread t of block b adds the terms b * AI_BLOCK + t, + RED_BLOCKS * AI_BLOCK, ... in ascending
    order; the block's values and then the RED_BLOCKS block sums go through `_block_sum`.  (A skipped term adds nothing: 0.)"""
    laps = max(1, -(-terms.shape[0] // LAP))
    x = np.zeros(laps * LAP)
    x[:terms.shape[0]] = terms
    x = x.reshape(laps, RED_BLOCKS, BLOCK)
    s = np.zeros((RED_BLOCKS, BLOCK))
    for j in range(laps):
        s = s + x[j]
    return float(_block_sum(_block_sum(s)))


def stats_model(avg, std_ratio):
    """The device's statistics in the device's order of additions (every step rounded on its own; the compiler may fuse the
    square into the sum on the device, which rounds once less): dict(mean, std, threshold).  It is here to check `stats_bound`
    on the CPU, not to be compared bit for bit."""
    a = np.asarray(avg, dtype=np.float64)
    n = a.shape[0]
    pos = a > 0
    mean = _device_total(np.where(pos, a, 0.0)) / float(n)
    with np.errstate(invalid="ignore", divide="ignore"):
        std = float(np.sqrt(np.float64(_device_total(np.where(pos, (a - mean) * (a - mean), 0.0))) / np.float64(n - 1)))
    return {"mean": mean, "std": std, "threshold": mean + std_ratio * std}


def keep_from(avg, threshold):
    """The kept set as `kq_keep_flags` forms it from the device's own avg and threshold."""
    a = np.asarray(avg)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((a > 0) & (a < threshold))


def reduction_depth(n):
    """The longest chain of rounded additions on the way from one avg to a total of `kq_partial` + `kq_finish`: a thread adds its
    ceil(n / (RED_BLOCKS * AI_BLOCK)) laps one after the other, its wave adds 6 tree steps, the block adds its 4 waves; the 256
    block sums go through the same tree and the same 4 waves once more."""
    laps = -(-int(n) // LAP)
    tree = int(math.log2(WAVE)) + BLOCK // WAVE
    return laps + 2 * tree


def stats_bound(avg, std_ratio):
    """dict(mean, std, threshold): how far the device's statistics may lie from `stats_ref`'s, in absolute terms.

    With u = 2^-53 and D = `reduction_depth`: a sum of non-negative terms through a chain of at most D rounded additions is within
    g(D) = D u / (1 - D u) of the exact sum, relatively.
    mean: g(D) for the device's sum, u for its division; the reference rounds twice (fsum, the division): (g(D) + 3u) * mean.
    std: the device squares v - c around ITS mean c, off by dm <= the bound above.  sum (v - c)^2 - sum (v - m)^2 =
    -2 (c - m) sum (v - m) + P (c - m)^2 over the P positive avg, so the total moves by at most 2 dm |sum (v - m)| + P dm^2.
    Each term carries three roundings (the difference once, which counts twice in the square, and the product), the sum g(D); the
    reference's terms carry the same three and one for fsum: (g(D) + 7u) * sum (|v - m| + dm)^2 more.  The division by n - 1 and
    the root add 2u on each side.  std lies between the roots of the total less and plus all that.
    threshold = mean + std_ratio * std: the two bounds, plus one rounding of the product and one of the sum on each side."""
    a = np.asarray(avg, dtype=np.float64)
    n = a.shape[0]
    pos = a[a > 0]
    ref = stats_ref(a, std_ratio)
    d = reduction_depth(n)
    g = d * U / (1.0 - d * U)
    dm = (g + 3.0 * U) * abs(ref["mean"]) * (1.0 + 8.0 * U)
    if n < 2:
        return {"mean": dm, "std": float("nan"), "threshold": float("nan")}
    dev = pos - ref["mean"]
    tot = math.fsum(dev * dev)
    dtot = 2.0 * dm * abs(math.fsum(dev)) + pos.size * dm * dm + (g + 7.0 * U) * math.fsum((np.abs(dev) + dm) ** 2)
    hi = math.sqrt((tot + dtot) / (n - 1.0)) * (1.0 + 4.0 * U)
    lo = math.sqrt(max(tot - dtot, 0.0) / (n - 1.0)) * (1.0 - 4.0 * U)
    ds = max(hi - ref["std"], ref["std"] - lo)
    dt = dm + std_ratio * ds + 4.0 * U * (abs(std_ratio * ref["std"]) + abs(ref["threshold"]))
    return {"mean": dm, "std": ds, "threshold": dt}


def near_threshold(avg, std_ratio):
    """The points whose place relative to the device's threshold the bound leaves open: avg > 0 within `stats_bound` of the
    reference's threshold."""
    a = np.asarray(avg, dtype=np.float64)
    ref, bound = stats_ref(a, std_ratio), stats_bound(a, std_ratio)
    with np.errstate(invalid="ignore"):
        return np.flatnonzero((a > 0) & (np.abs(a - ref["threshold"]) <= bound["threshold"]))


# ------------------------------------------------------------------------------------------------- box select
BOX_MUTANTS = ("le_faces", "wave_rank_only")


def inside(points, boxes, mutant=None):
    """(n_boxes, n) bool: lo < p < hi on all three axes (NaN compares false)."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)[None, :, :]
    b = np.asarray(boxes, dtype=np.float64).reshape(-1, 6)
    lo, hi = b[:, None, :3], b[:, None, 3:]
    with np.errstate(invalid="ignore"):
        if mutant == "le_faces":
            return ((p >= lo) & (p <= hi)).all(axis=2)
        return ((p > lo) & (p < hi)).all(axis=2)


def box_model(points, boxes, cap=None, mutant=None, poison=-7):
    """`ai_box_select` on the CPU: (out_index, box_offsets, total).  `kb_count` counts per (box, tile of AI_BLOCK points); the
    exclusive scan is box-major; `kb_fill` puts point i at its tile's offset + the inside lanes below it in its wave + the counts
    of the earlier waves of its tile.  With ``total > cap`` (or no point inside) nothing is written: the buffer keeps ``poison``.
    ``mutant="wave_rank_only"`` forgets the earlier waves."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    m = inside(p, boxes, mutant)
    nbox = m.shape[0]
    ntile = -(-n // BLOCK) if n else 0
    pad = np.zeros((nbox, ntile * BLOCK), bool)
    pad[:, :n] = m
    lanes = pad.reshape(nbox, ntile, BLOCK // WAVE, WAVE)
    wave_cnt = lanes.sum(axis=3)
    cnt = wave_cnt.sum(axis=2).reshape(-1)
    off = np.concatenate([[0], np.cumsum(cnt)]).astype(np.int64)
    total = int(off[-1])
    offsets = off[::ntile].copy() if ntile else np.zeros(nbox + 1, np.int64)   # box b starts at off[b * ntile]
    cap = total if cap is None else cap
    out = np.full(max(cap, 0), poison, np.int32)
    if total > cap or total == 0:
        return out, offsets, total
    before = np.cumsum(wave_cnt, axis=2) - wave_cnt
    if mutant == "wave_rank_only":
        before = np.zeros_like(before)
    tile_off = off[:-1].reshape(nbox, ntile)
    for a in range(0, nbox, 2048):          # a slab of boxes at a time: the ranks of 65 536 boxes do not fit one array
        ln = lanes[a:a + 2048]
        below = np.cumsum(ln, axis=3, dtype=np.int32) - ln
        pos = tile_off[a:a + 2048, :, None, None] + before[a:a + 2048, :, :, None] + below
        idx = np.broadcast_to(np.arange(ntile * BLOCK).reshape(1, ntile, BLOCK // WAVE, WAVE), ln.shape)
        ok = ln & (pos < cap)
        out[pos[ok]] = idx[ok]
    return out, offsets, total


# ------------------------------------------------------------------------------------------------- voxels
VOXEL_MUTANTS = ("inverse", "no_half", "sorted_sum")


def bits_for(count):
    """Bits that hold 0 .. count - 1 (the host's `bits_for`)."""
    b = 0
    while b < 63 and (1 << b) < count:
        b += 1
    return b


def voxel_keys(points, voxel, mutant=None):
    """The host part of `ai_voxel_down_sample` and `kv_keys`: dict(vmin, index (n, 3) int64, bits (3,), key (n,) of Python
    ints).  Raises ValueError with the entry's text where the entry refuses: input that is not finite, an index beyond the int
    range, more than 64 key bits.  ``mutant``: ``"inverse"`` multiplies by 1 / voxel, ``"no_half"`` leaves vmin at the minimum."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    v = float(voxel)
    if not np.isfinite(p).all() or not ((p.max(axis=0) - p.min(axis=0)) < K["EXTENT_LIMIT"]).all():
        raise ValueError("coordinates are not finite")
    mn, mx = p.min(axis=0), p.max(axis=0)
    vmin = mn if mutant == "no_half" else mn - v * 0.5
    span = float(((mx + v * 0.5) - vmin).max())
    if v * float(INT_MAX) < span:
        raise ValueError("voxel_size is too small")
    index = np.floor((p - vmin) * (1.0 / v) if mutant == "inverse" else (p - vmin) / v).astype(np.int64)
    bits = np.array([bits_for(int(math.floor((mx[a] - vmin[a]) / v)) + 1) for a in range(3)])
    if int(bits.sum()) > K["MAX_KEY_BITS"]:
        raise ValueError(f"the voxel grid needs {int(bits.sum())} key bits")
    sz, sy = int(bits[2]), int(bits[1] + bits[2])
    key = [(int(i) << sy) | (int(j) << sz) | int(k) for i, j, k in index]
    return {"vmin": vmin, "index": index, "bits": bits, "key": key}


def voxel_model(points, voxel, mutant=None):
    """`ai_voxel_down_sample` on the CPU: (means (m, 3), trace (n,) int32).  A stable sort by the 64-bit key, then per voxel the
    sum of its points in input order, one division by the count.  ``mutant="sorted_sum"`` adds each voxel's points in ascending
    coordinate order instead."""
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    key = voxel_keys(p, voxel, mutant)["key"]
    order = sorted(range(p.shape[0]), key=lambda i: key[i])
    out, trace = [], np.empty(p.shape[0], np.int32)
    a = 0
    while a < len(order):
        b = a
        while b < len(order) and key[order[b]] == key[order[a]]:
            b += 1
        members = order[a:b]
        trace[members] = len(out)
        rows = p[members]
        if mutant == "sorted_sum":
            rows = np.sort(rows, axis=0)
        s = np.zeros(3)
        for row in rows:
            s = s + row
        out.append(s / float(b - a))
        a = b
    return np.array(out).reshape(-1, 3), trace


# ------------------------------------------------------------------------------------------------- fixtures
@dataclass
class BoxCase:
    name: str
    points: np.ndarray
    boxes: np.ndarray                       # (n_boxes, 6): lo, hi
    claims: dict = field(default_factory=dict)

    @functools.cached_property
    def truth(self):
        """(out_index int32, box_offsets int64) of `prep_ref.box_select`."""
        ids = prep_ref.box_select(self.points, [(b[:3], b[3:]) for b in self.boxes])
        off = np.concatenate([[0], np.cumsum([i.size for i in ids])]).astype(np.int64)
        return np.concatenate(ids).astype(np.int32), off


@dataclass
class KnnCase:
    name: str
    points: np.ndarray
    nb: int
    std_ratio: float = 2.0
    claims: dict = field(default_factory=dict)
    groups: np.ndarray | None = None

    @property
    def n(self):
        return self.points.shape[0]

    @property
    def k(self):
        return min(self.nb, self.n)

    @functools.cached_property
    def avg(self):
        return knn_avg_exact(self.points, self.nb, self.groups)

    @functools.cached_property
    def ref(self):
        return stats_ref(self.avg, self.std_ratio)

    @functools.cached_property
    def bound(self):
        return stats_bound(self.avg, self.std_ratio)

    @functools.cached_property
    def near(self):
        return near_threshold(self.avg, self.std_ratio)


@dataclass
class VoxCase:
    name: str
    points: np.ndarray
    voxel: float
    claims: dict = field(default_factory=dict)

    @functools.cached_property
    def truth(self):
        out, trace = prep_ref.voxel_down_sample(self.points, self.voxel)
        return out, trace.astype(np.int32)


# ---- box select
BOX_SIZES = (1, WAVE - 1, WAVE, WAVE + 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1)
FACE_BOX = np.array([0.1, 0.2, 0.3, 0.7, 0.8, 0.9])          # no face is a dyadic number


def _ulps(x):
    return np.array([np.nextafter(x, -np.inf), x, np.nextafter(x, np.inf)])


@functools.lru_cache(maxsize=None)
def box_cases():
    rng = np.random.default_rng(4101)
    unit = np.r_[np.zeros(3), np.ones(3)]
    out = []
    for n in BOX_SIZES:                     # a partial box, a box that holds all, and one that holds none
        p = rng.random((n, 3))
        out.append(BoxCase(f"box_n{n}", p, np.array([np.r_[0.2, 0.1, 0.0, 0.9, 0.8, 0.7], np.r_[-1.0, -1, -1, 2, 2, 2], unit + 5.0]),
                           dict(tiles=-(-n // BLOCK))))
    n = 2 * BLOCK + 1
    for name, lanes in (("lane0", np.arange(n) % WAVE == 0), ("lane63", np.arange(n) % WAVE == WAVE - 1),
                        ("all", np.ones(n, bool)), ("none", np.zeros(n, bool))):
        p = np.where(lanes[:, None], rng.uniform(0.25, 0.75, (n, 3)), rng.uniform(1.5, 2.5, (n, 3)))
        out.append(BoxCase(f"box_{name}_inside", p, unit[None, :].copy(), dict(inside=int(lanes.sum()))))
    mid = 0.5 * (FACE_BOX[:3] + FACE_BOX[3:])
    rows = []
    for face in range(6):                   # on the face, one ulp inside it, one ulp outside it
        for v in _ulps(FACE_BOX[face]):
            q = mid.copy()
            q[face % 3] = v
            rows.append(q)
    out.append(BoxCase("box_faces", np.array(rows), FACE_BOX[None, :].copy(), dict(inside=6)))
    zero = np.array([[-0.0, 0.5, 0.5], [0.5, -0.0, 0.5], [0.5, 0.5, -0.0], [0.0, 0.5, 0.5], [5e-324, 0.5, 0.5], [-5e-324, -0.5, -0.5],
                     [-0.0, -0.5, -0.5], [-0.5, -0.5, -0.0]])
    out.append(BoxCase("box_signed_zero", zero, np.array([unit, np.r_[-np.ones(3), np.zeros(3)], np.r_[-np.ones(3), -0.0, -0.0, -0.0]]),
                       dict(inside=3)))
    bad = [rng.uniform(-1.0, 1.0, (20, 3))]
    for a in range(3):
        for v in (np.nan, np.inf, -np.inf):
            q = np.zeros(3)
            q[a] = v
            bad.append(q[None, :])
    everywhere = np.r_[np.full(3, -np.inf), np.full(3, np.inf)]
    out.append(BoxCase("box_nonfinite_points", np.concatenate(bad), np.array([everywhere, np.r_[-2.0, -2, -2, 2, 2, 2]]),
                       dict(inside=40)))
    p = rng.uniform(-1.0, 1.0, (300, 3))
    half = np.r_[-0.5, -0.5, -0.5, 0.5, 0.5, 0.5]
    out.append(BoxCase("box_identical_nested_inverted", p,
                       np.array([half, half, 0.5 * half, np.r_[half[3:], half[:3]], everywhere, np.r_[-np.inf, -0.5, -0.5, 0.0, 0.5, np.inf]])))
    for nbox in (1, 2, MAX_BOXES):
        lo = rng.uniform(-1.2, 0.6, (nbox, 3))
        out.append(BoxCase(f"box_{nbox}_boxes", p, np.concatenate([lo, lo + rng.uniform(0.0, 1.2, (nbox, 3))], axis=1), dict(n_boxes=nbox)))
    return out


# ---- kNN: ring stop
ISSUE_LINE = (0.0, 39.246153092755, 0.4590257911993334, 0.22951289559966667, 0.6885386867990001)     # k = 2: the third misses the fifth
ISSUE_AVG = ("0x1.d60adb64e2fb5p-4", "0x1.d60adb64e2fb4p-4")                                        # parent rule, truth
RING_KS = (2, KNN_LENGTHS[0])


def _query_knn(clouds, qi, k, stop):
    """`knn_model` for point ``qi`` of each of T clouds (T, n, 3), every cloud on its own grid: the k best squares (T, k), sorted."""
    P = np.asarray(clouds, dtype=np.float64)
    T = P.shape[0]
    mn, _, cell, _, nn, _ = knn_grids(P)
    cells = np.clip(np.floor((P - mn[:, None, :]) * (1.0 / cell)[:, None, None]).astype(np.int64), 0, (nn - 1)[:, None, :])
    q, qc = P[:, qi], cells[:, qi]
    ring = np.abs(cells - qc[:, None, :]).max(axis=2)
    d2 = sq_plain(q[:, None, :], P)
    best = np.full((T, k), np.inf)
    live = np.arange(T)
    rule = STOP_RULES[stop]
    for r in range(int(nn.max()) + 1):
        vis = ring[live] <= r
        b = np.sort(np.where(vis, d2[live], np.inf), axis=1)[:, :k]
        best[live] = b
        with np.errstate(invalid="ignore", over="ignore"):
            done = (vis.sum(axis=1) >= k) & rule(mn[live], nn[live], cell[live], q[live], qc[live], r, b[:, k - 1])
        live = live[~done & (r < nn[live].max(axis=1))]
        if live.size == 0:
            break
    return best


def ring_stop_search(tries, seed, k, keep=0):
    """The construction of tests/points_cases.py's ring-stop cases, for the kNN: a line of points on a random axis, with a
    negative minimum (the anchor) and a far end that fix the grid; a query q a few ulps below a cell border; a point B a few
    ulps below the border r cells further on, in direction ``sgn``; a point A at r cells from q on the other side; and k - 2
    copies of q, so that A is q's k-th neighbour once ring r has been searched.  A power of two (in metres from the minimum)
    lies between the two borders or on the lower one: whether ``fl(p - min)`` rounds the upper point onto its border, which
    stores it one cell further from the other than it lies, is left to chance.

    Returns dict(tries, miss_parent, miss_shipped, cases): the number of tries in which the query's k best squares under
    either stop rule differ from the k smallest of the whole cloud, and up to ``keep`` missed clouds per (axis, sgn, r)."""
    rng = np.random.default_rng(seed)
    T, n = int(tries), 5 + (k - 2)
    axis, sgn, r = rng.integers(0, 3, T), rng.choice([-1, 1], T), rng.integers(1, 4, T)
    mn = np.where(rng.random(T) < 0.5, -np.round(rng.uniform(5.0, 60.0, T), 1), -rng.uniform(5.0, 60.0, T))
    far = mn + rng.uniform(60.0, 120.0, T)
    t = np.arange(T)
    pts = np.zeros((T, n, 3))
    pts[t, :, axis] = mn[:, None]
    pts[t, 1, axis] = far
    cell = knn_grids(pts)[2]                                   # the grid depends on the ends, the axis and n alone
    P = 2.0 ** rng.integers(3, 6, T)                           # 8 .. 32 m from the minimum the spacing of the doubles doubles
    kl = np.floor(P / cell).astype(np.int64) - rng.integers(0, 3, T) % r
    ku = kl + r
    kq, kb = np.where(sgn > 0, kl, ku), np.where(sgn > 0, ku, kl)
    h = np.spacing(P)
    xq = mn + kq * cell - rng.uniform(0.0, 2.0, T) * h
    xb = mn + kb * cell - rng.uniform(0.0, 2.0, T) * h
    xa = xq - sgn * (r * cell)
    b_first = rng.random(T) < 0.5
    pts[t, 2, axis] = xq
    pts[t, 3, axis] = np.where(b_first, xb, xa)
    pts[t, 4, axis] = np.where(b_first, xa, xb)
    pts[t, 5:, axis] = xq[:, None]
    truth = np.sort(sq_plain(pts[:, 2, None, :], pts), axis=1)[:, :k]
    miss = {rule: (_query_knn(pts, 2, k, rule) != truth).any(axis=1) for rule in STOP_RULES}
    cases, seen = [], {}
    for i in np.flatnonzero(miss["parent"]) if keep else ():
        key = (int(axis[i]), int(sgn[i]), int(r[i]))
        if seen.get(key, 0) < keep:
            seen[key] = seen.get(key, 0) + 1
            cases.append(dict(axis=key[0], sgn=key[1], r=key[2], k=k, points=pts[i].copy()))
    return {"tries": T, "miss_parent": int(miss["parent"].sum()), "miss_shipped": int(miss["shipped"].sum()), "cases": cases}


RING_SEARCH = {2: (150_000, 21), KNN_LENGTHS[0]: (150_000, 22)}   # k: (tries, seed) of the fixtures' search


@functools.lru_cache(maxsize=None)
def ring_stop_cases():
    """Line clouds on which the stop rule ``sqrt(kth) <= r * cell`` ends the query's search one ring early and an average comes
    out wrong: one found case per axis, direction, ring 1 .. 3 and k = 2 / 20; ``claims["query"]`` is the point that misses a
    neighbour.  `ring_stop_search` models the host's own cube root, so the found cases hold on the device.
    In front of them the line written out in the issue, on each axis (k = 2).  It was found on a grid whose cell is ``np.cbrt``
    of the volume per point; the host takes the C library's ``cbrt``, whose cell differs in the last bit there, and on that grid
    the old rule happens to get the line right.  It stays a fixture (``claims["issue"]``): the averages must be exact on it
    whatever the cell is."""
    out = []
    for a in range(3):
        p = np.zeros((5, 3))
        p[:, a] = ISSUE_LINE
        out.append(KnnCase(f"ring_stop_issue_{'xyz'[a]}", p, 2, claims=dict(query=2, axis=a, issue=True)))
    for k, (tries, seed) in RING_SEARCH.items():
        found, have = [], set()
        for batch in range(8):                # one batch finds all 18 (axis, direction, ring); a rarer one is sought further
            for c in ring_stop_search(tries, seed + 1000 * batch, k, keep=1)["cases"]:
                if (c["axis"], c["sgn"], c["r"]) not in have:
                    have.add((c["axis"], c["sgn"], c["r"]))
                    found.append(c)
            if len(have) == 18:
                break
        found.sort(key=lambda c: (c["r"], c["axis"], c["sgn"]))
        for c in found:
            out.append(KnnCase(f"ring_stop_k{k}_{'xyz'[c['axis']]}{'+' if c['sgn'] > 0 else '-'}_r{c['r']}", c["points"], k,
                               claims=dict(query=2, axis=c["axis"], sgn=c["sgn"], r=c["r"], k=k)))
    return out


# ---- kNN: the grid's limits
def max_corner_search(seed, tries=400):
    """3 x 3 x 3 lattices of random spacing and origin: the cell is the spacing up to the rounding of the cube root, so
    ``floor(ext / cell) + 1`` may count 2 cells where ``floor(ext * inv_cell)`` puts the far corner into a third, which only
    the clamp of `kcell_of` brings back.  Returns (tries used, the first such lattice or None)."""
    rng = np.random.default_rng(seed)
    lat = np.stack(np.meshgrid(*[np.arange(3.0)] * 3, indexing="ij"), -1).reshape(-1, 3)
    for t in range(tries):
        p = lat * rng.uniform(0.1, 3.0) + rng.uniform(-50.0, 50.0, 3)
        g = knn_grid(p)
        if (kcells(g, p, clamp=False) > g.n - 1).any():
            return t + 1, p
    return tries, None


KNN_KS = (1, 2, KNN_LENGTHS[0] - 1, KNN_LENGTHS[0], KNN_LENGTHS[0] + 1, KNN_LENGTHS[1], KNN_LENGTHS[1] + 1, MAX_K - 1, MAX_K)
CLUSTER = BLOCK                              # points per cluster of the second-lap cloud


def second_lap_cloud():
    """RED_BLOCKS * AI_BLOCK + 1 points: `kq_partial`'s thread 0 of block 0 takes a second lap.  A regular arrangement whose
    truth the full matrix gives per group: one pattern of AI_BLOCK points on a 2^-10 lattice inside a unit cube, repeated at
    16 x 16 dyadic translates 8 apart (every sum and difference is exact, so the squares do not depend on the translate), and
    one more point inside the first cube.  Returns (points, groups)."""
    rng = np.random.default_rng(65537)
    side = int(round(math.sqrt(LAP // CLUSTER)))
    assert side * side * CLUSTER == LAP
    pattern = rng.integers(0, 1024, (CLUSTER, 3)) / 1024.0
    shift = np.stack(np.meshgrid(np.arange(side) * 8.0, np.arange(side) * 8.0, indexing="ij"), -1).reshape(-1, 2)
    p = np.tile(pattern[None, :, :], (side * side, 1, 1))
    p[:, :, :2] += shift[:, None, :]
    groups = np.repeat(np.arange(side * side), CLUSTER)
    order = rng.permutation(LAP)                         # the input order is not the cell order
    p, groups = p.reshape(-1, 3)[order], groups[order]
    extra = np.array([[0.5 + 2.0 ** -11, 0.5, 0.5 - 2.0 ** -11]])
    return np.concatenate([p, extra]), np.concatenate([groups, [0]])


@functools.lru_cache(maxsize=None)
def knn_cases():
    rng = np.random.default_rng(4102)
    out = list(ring_stop_cases())
    n = 300
    plane = np.zeros((n, 3))
    plane[:, 1:] = rng.uniform(0.0, 20.0, (n, 2))
    out.append(KnnCase("knn_plane_yz_grown", plane + [3.25, 0, 0], 20, claims=dict(grown=True)))
    for a, b, name in ((0, 1, "xy"), (0, 2, "xz")):
        q = np.zeros((n, 3))
        q[:, [a, b]] = rng.uniform(-10.0, 10.0, (n, 2))
        out.append(KnnCase(f"knn_plane_{name}", q + [0.1, -0.2, 0.3], 20))
    for a in range(3):
        q = np.tile(rng.uniform(-5.0, 5.0, 3), (200, 1))
        q[:, a] = rng.uniform(-30.0, 30.0, 200)
        out.append(KnnCase(f"knn_line_{'xyz'[a]}", q, 20))
    out.append(KnnCase("knn_identical", np.tile(np.array([[1.5, -2.25, 3.0]]), (100, 1)), 20, claims=dict(all_zero=True)))
    two = np.concatenate([rng.uniform(0.0, 0.5, (30, 3)), rng.uniform(0.0, 0.5, (30, 3)) + [0.0, 400.0, 400.0]])
    out.append(KnnCase("knn_two_clusters", two, 40, claims=dict(min_rings=8)))
    tries, corner = max_corner_search(4103)
    if corner is not None:
        out.append(KnnCase("knn_max_corner", corner, 7, claims=dict(clamped=True, tries=tries)))
    cloud = np.concatenate([rng.normal(0.0, 1.0, (200, 3)), rng.uniform(-4.0, 4.0, (100, 3))])
    for k in KNN_KS:
        out.append(KnnCase(f"knn_k{k}", cloud, k, claims=dict(instance=knn_instance(k))))
    for m in (1, 2, 3, MAX_K):
        out.append(KnnCase(f"knn_nb_above_n{m}", rng.uniform(-1.0, 1.0, (m, 3)), MAX_K + 36,
                           claims=dict(k=m, on_threshold=m == 2)))      # two points: two equal averages, std 0
    k = KNN_LENGTHS[0]
    copies = np.concatenate([rng.uniform(-3.0, 3.0, (200, 3)), np.tile(np.array([[0.5, 0.25, -0.125]]), (k, 1)),
                             np.tile(np.array([[-1.5, 1.25, 0.375]]), (k - 1, 1))])
    out.append(KnnCase("knn_k_copies", copies[rng.permutation(copies.shape[0])], k, claims=dict(zeros=k)))
    cube = np.stack(np.meshgrid(*[np.array([0.0, 2.0])] * 3, indexing="ij"), -1).reshape(-1, 3) + [-4.0, 8.0, 16.0]
    out.append(KnnCase("knn_dyadic_cube", cube, 8, claims=dict(on_threshold=True)))
    for m in (BLOCK - 1, BLOCK, BLOCK + 1):
        out.append(KnnCase(f"knn_n{m}", rng.uniform(-2.0, 2.0, (m, 3)) * [3.0, 2.0, 1.0], 20))
    p, groups = second_lap_cloud()
    out.append(KnnCase(f"knn_n{LAP + 1}_second_lap", p, 20, claims=dict(laps=2), groups=groups))
    return out


# ---- voxels
VOXEL_SIZES = (0.35, 0.05)


def inverse_mismatch_search(voxel, seed, tries=200_000, keep=12):
    """Points p >= 0 (the cloud's minimum is the origin) for which ``floor((p - vmin) / v)`` and ``floor((p - vmin) * (1 / v))``
    differ: random multiples of the voxel size, where the quotient is an integer up to rounding.  Returns (tries, coordinates)."""
    rng = np.random.default_rng(seed)
    vmin = 0.0 - voxel * 0.5
    x = vmin + rng.integers(1, 4000, tries) * voxel
    x = np.where(rng.random(tries) < 0.5, x, np.nextafter(x, -np.inf))
    d = x - vmin
    hit = np.floor(d / voxel) != np.floor(d * (1.0 / voxel))
    return tries, np.unique(x[hit & (x >= 0)])[:keep]


@functools.lru_cache(maxsize=None)
def voxel_cases():
    rng = np.random.default_rng(4104)
    out = []
    for v in VOXEL_SIZES:
        low = np.array([-3.3, -1.7, -0.4])
        vmin = low - v * 0.5
        rows = [low]
        for a in range(3):
            for j in (1, 2, 5, 17, 40):
                for x in _ulps(vmin[a] + j * v):
                    q = low.copy()
                    q[a] = x
                    rows.append(q)
        out.append(VoxCase(f"voxel_borders_{v}", np.array(rows), v))
        tries, xs = inverse_mismatch_search(v, 4105)
        rows = [np.zeros(3)]
        for a in range(3):
            for x in xs:                      # with the centres of both voxels in question: the trace shows which one x joins
                d = x - (0.0 - v * 0.5)
                for y in (x, (np.floor(d / v) + 0.5) * v - v * 0.5, (np.floor(d * (1.0 / v)) + 0.5) * v - v * 0.5):
                    q = np.zeros(3)
                    q[a] = y
                    rows.append(q)
        out.append(VoxCase(f"voxel_inverse_mismatch_{v}", np.array(rows), v, dict(found=int(xs.size), tries=tries)))
    for a in range(3):
        for count, tag in ((8, "pow2"), (9, "pow2_plus_1")):          # the largest index + 1 on this axis
            q = rng.integers(0, 3, (40, 3)).astype(np.float64)
            q[:, a] = rng.integers(0, count, 40)
            q[0], q[1, a] = 0.0, count - 1.0
            bits = [2, 2, 2]
            bits[a] = 3 if count == 8 else 4
            out.append(VoxCase(f"voxel_{tag}_{'xyz'[a]}", q, 1.0, dict(bits=tuple(bits))))
    out.append(VoxCase("voxel_single", np.array([1.0, 2.0, 3.0]) + rng.uniform(0.0, 0.1, (5, 3)), 1.0, dict(bits=(0, 0, 0), voxels=1)))
    wide = [2.0 ** 22 - 1.0, 2.0 ** 21 - 1.0, 2.0 ** 21 - 1.0]
    out.append(VoxCase("voxel_64_key_bits", np.array([[0.0, 0, 0], wide]), 1.0, dict(bits=(22, 21, 21), voxels=2)))
    out.append(VoxCase("voxel_65_key_bits", np.array([[0.0, 0, 0], [wide[0] + 1.0, wide[1], wide[2]]]), 1.0, dict(refused="key bits")))
    a, b, c = 0.1, 0.2, 0.3
    assert (a + b) + c != a + (b + c)
    triple = np.array([[a, a, a], [b, b, b], [c, c, c]])
    out.append(VoxCase("voxel_triple_abc", triple, 1.0, dict(voxels=1)))
    out.append(VoxCase("voxel_triple_cba", triple[::-1].copy(), 1.0, dict(voxels=1)))
    out.append(VoxCase("voxel_1000_in_one", np.array([7.0, -7.0, 0.5]) + rng.uniform(0.0, 0.3, (1000, 3)), 0.35 * 2, dict(voxels=1)))
    for m in (BLOCK, BLOCK + 1):
        q = np.zeros((m, 3))
        q[:, 2] = rng.permutation(m) * 0.35 + 0.01
        out.append(VoxCase(f"voxel_{m}_voxels", q, 0.35, dict(voxels=m)))
    return out


# ---- input that is not finite
def nonfinite_clouds():
    """(name, cloud): 300 finite points and one coordinate that is NaN, +inf or -inf, on each axis."""
    rng = np.random.default_rng(4106)
    base = rng.uniform(-5.0, 5.0, (300, 3))
    out = []
    for a in range(3):
        for tag, v in (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf)):
            p = base.copy()
            p[137 + a, a] = v
            out.append((f"{tag}_{'xyz'[a]}", p))
    return out
