"""Fixtures, a host model of the device's search and brute-force truths for DBSCAN on the device
(``autoinst_amd/csrc/ai_dbscan.hip``, rules D1-D6 of ``include/autoinst_hip.h``) at the limits of its kernels.

Plain NumPy / SciPy, seeded, no GPU and no library: tests/test_dbscan_cases.py proves on the CPU that every fixture sits where
its name says and that four deliberately wrong searches are rejected; tests/test_gpu_dbscan_cases.py compares the device with
the same truths, everything equal.

The limits are READ from the sources (`constants`): a changed constant moves the fixtures with it.

* `search_model` restates the search of `db_neighbours` over `build_cells`' grid (`points_cases.grid_of` / `cells_of` with
  ``cell = eps * (1 + DB_CELL_SLACK)``): the clamped +-1 ring by linear cell key, the cloud filter, ``<=`` on
  `dbscan_ref.d1_sq_dist`; rules D2-D5 follow from its pairs as they do on the device, by the ranks of the roots.  ``variant``
  breaks one place (`VARIANTS`).
* The truth is per cloud, alone: `dbscan_ref.dbscan_brute` (the full D1 matrix) up to `BRUTE_MAX` points, `dbscan_ref.dbscan`
  (candidates from a tree at a wider radius, the exact D1 predicate) above.
"""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass, field

import numpy as np

import dbscan_ref
import edge_geometry as eg
import points_cases as pc


# ------------------------------------------------------------------------------------------------- constants from the sources
def constants():
    """The limits of `ai_dbscan`, parsed out of ``ai_dbscan.hip``, ``ai_scan.hip``, ``ai_common.h`` and (through
    `points_cases.K`) ``ai_cells.inc``."""
    db, scan = pc._read(pc._CSRC, "ai_dbscan.hip"), pc._read(pc._CSRC, "ai_scan.hip")
    if not re.search(r"#define\s+SCAN_TILE\s+\(AI_BLOCK\s*\*\s*SCAN_ITEMS\)", scan):
        raise RuntimeError("SCAN_TILE is no longer AI_BLOCK * SCAN_ITEMS")
    if not re.search(r"build_cells\(ctx, dx, n, eps \* \(1\.0 \+ DB_CELL_SLACK\), C, \"ai_dbscan\"\)", db):
        raise RuntimeError("ai_dbscan no longer asks build_cells for eps * (1 + DB_CELL_SLACK)")
    return dict(DB_CELL_SLACK=float(pc._find(db, r"^\s*#define\s+DB_CELL_SLACK\s+([0-9.e+-]+)", "DB_CELL_SLACK")),
                AI_BLOCK=pc.K["AI_BLOCK"],
                SCAN_TILE=pc.K["AI_BLOCK"] * int(pc._find(scan, r"^\s*#define\s+SCAN_ITEMS\s+(\d+)", "SCAN_ITEMS")),
                CELL_CAP=pc.K["CELL_CAP"], GROW=pc.K["GROW"], EXTENT_LIMIT=pc.K["EXTENT_LIMIT"],
                N_LIMIT=1 << int(pc._find(db, r"n >= \(\(int64_t\)1 << (\d+)\)\) return bad", "the point limit of ai_dbscan")))


K = constants()
SLACK = K["DB_CELL_SLACK"]
BLOCK = K["AI_BLOCK"]
SCAN_TILE = K["SCAN_TILE"]
BRUTE_MAX = 3000
VARIANTS = ("no_slack", "lt", "no_clamp_hi", "same_cloud_ignored")


# ------------------------------------------------------------------------------------------------- fixtures and their truth
@dataclass
class Case:
    name: str
    clouds: list            # (n_c, 3) float64 each; one entry: a single-cloud call
    eps: float
    ms: int
    claims: dict = field(default_factory=dict)
    below: bool = False     # also compared at nextafter(eps, 0)

    @property
    def n(self):
        return sum(c.shape[0] for c in self.clouds)

    @functools.cached_property
    def truth(self):
        return truth_of(self.clouds, self.eps, self.ms)

    @functools.cached_property
    def truth_below(self):
        return truth_of(self.clouds, float(np.nextafter(self.eps, 0)), self.ms)


def truth_one(p, eps, ms):
    return dbscan_ref.dbscan_brute(p, eps, ms) if p.shape[0] <= BRUTE_MAX else dbscan_ref.dbscan(p, eps, ms)


def truth_of(clouds, eps, ms):
    """Per cloud, alone: [(labels, n_clusters, counts, sizes)].  Bit-equal clouds share one computation."""
    seen, out = {}, []
    for c in clouds:
        key = c.tobytes()
        if key not in seen:
            seen[key] = truth_one(c, eps, ms)
        out.append(seen[key])
    return out


def same(got, want):
    """Labels, cluster count, saturated counts and sizes of one cloud, all equal."""
    return (int(got[1]) == int(want[1]) and all(np.asarray(g).shape == np.asarray(w).shape and np.array_equal(g, w)
                                                for g, w in zip((got[0], got[2], got[3]), (want[0], want[2], want[3]))))


# ------------------------------------------------------------------------------------------------- the device's search
def device_grid(points, eps, variant=None):
    """`build_cells`' grid over all points of a call, for the cell `ai_dbscan` asks for."""
    return pc.grid_of(points, eps if variant == "no_slack" else eps * (1.0 + SLACK))


def search_pairs(points, cloud_of, eps, variant=None):
    """Every (i, j) that `db_neighbours` hands to its caller, i != j first of all, as the device finds them: j is a point of a
    cell of i's ring, of i's cloud, with D1 true.  The ring is the 27 cells (cz + dz, cy + dy, cx + dx) that survive the clamp,
    addressed by the linear key (z * ny + y) * nx + x as the table is.

    ``no_slack``: cells of eps itself.  ``lt``: ``<`` for ``<=``.  ``no_clamp_hi``: the ring's upper ends are cx + 1, cy + 1 and
    cz + 1 whatever the grid's size, so the key of a cell past a row's end is another cell's (one past the table's end counts as
    empty) and that cell's points are met a second time.  ``same_cloud_ignored``: no cloud filter."""
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    n = p.shape[0]
    g = device_grid(p, eps, variant)
    c = pc.cells_of(g, p[None])[0]
    nx, ny, nz = (int(v) for v in g.n[0])
    key = (c[:, 2] * ny + c[:, 1]) * nx + c[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    e2 = eps * eps
    ii, jj = [], []
    me = np.arange(n)
    for dz in (-1, 0, 1):
        for dy in (-1, 0, 1):
            for dx in (-1, 0, 1):
                x, y, z = c[:, 0] + dx, c[:, 1] + dy, c[:, 2] + dz
                ok = (x >= 0) & (y >= 0) & (z >= 0)
                if variant != "no_clamp_hi":
                    ok &= (x < nx) & (y < ny) & (z < nz)
                k = (z * ny + y) * nx + x
                ok &= k < nx * ny * nz
                lo = np.searchsorted(skey, k, "left")
                cnt = np.where(ok, np.searchsorted(skey, k, "right") - lo, 0)
                tot = int(cnt.sum())
                if tot == 0:
                    continue
                i = np.repeat(me, cnt)
                j = order[np.repeat(lo, cnt) + (np.arange(tot) - np.repeat(np.cumsum(cnt) - cnt, cnt))]
                keep = np.ones(tot, bool) if variant == "same_cloud_ignored" else cloud_of[i] == cloud_of[j]
                if (dx, dy, dz) == (0, 0, 0):
                    keep &= i != j                                   # the point itself: counted by rule D1, not as a pair
                i, j = i[keep], j[keep]
                d2 = dbscan_ref.d1_sq_dist(p[i], p[j])
                near = d2 < e2 if variant == "lt" else d2 <= e2
                ii.append(i[near])
                jj.append(j[near])
    if not ii:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    return np.concatenate(ii).astype(np.int64), np.concatenate(jj).astype(np.int64)


def search_model(clouds, eps, ms, variant=None):
    """`ai_dbscan` on the CPU, per cloud (labels, n_clusters, counts, sizes).  The pairs come from `search_pairs` over all
    points of the call; D2-D5 then as the device has them: one numbering of all roots of the call by index, a cloud's labels
    are its roots' ranks less the rank at the cloud's first point."""
    off = np.concatenate([[0], np.cumsum([c.shape[0] for c in clouds])]).astype(np.int64)
    n = int(off[-1])
    if n == 0:
        return [(np.zeros(0, np.int32), 0, np.zeros(0, np.int32), np.zeros(0, np.int32)) for _ in clouds]
    p = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds])
    cloud_of = np.repeat(np.arange(len(clouds)), np.diff(off))
    ii, jj = search_pairs(p, cloud_of, eps, variant)
    lab, k, counts, _ = dbscan_ref._from_pairs(n, ii, jj, ms)
    core = counts >= ms
    root = np.full(k, n, dtype=np.int64)                             # the smallest core index of every cluster
    np.minimum.at(root, lab[core], np.flatnonzero(core))
    out = []
    for c in range(len(clouds)):
        a, b = int(off[c]), int(off[c + 1])
        before = int(np.searchsorted(root, a))
        kc = int(np.searchsorted(root, b)) - before
        lc = np.where(lab[a:b] >= 0, lab[a:b] - before, -1).astype(np.int32)
        sizes = np.bincount(lc[lc >= 0], minlength=kc).astype(np.int32)
        out.append((lc, kc, counts[a:b], sizes))
    return out


def rejects(case, variant):
    """True when the wrong search gives another answer than the truth on this fixture, at eps or (``below``) a step under it."""
    runs = [(case.eps, case.truth)] + ([(float(np.nextafter(case.eps, 0)), case.truth_below)] if case.below else [])
    return any(not all(same(g, w) for g, w in zip(search_model(case.clouds, e, case.ms, variant), t)) for e, t in runs)


# ------------------------------------------------------------------------------------------------- border pairs
ISSUE_PAIR = dict(eps=0.3907553365008748, a=0.7815106730017495, b=1.1722660095026243)
BIG_K = 8192        # "cell indices around 1e4": at a power of two the spacing of the doubles changes between the pair's products
PAIR_AXES = ("x", "y", "z", "xy")


def border_pair_search(tries, seed, *, big, mn):
    """1-D pairs (a, b) on a grid whose minimum is ``mn``, with b - a = eps exactly (so D1 holds with equality and fails one step
    below eps) and with cells TWO apart when the cell is eps itself: ``floor((a - mn) * fl(1 / eps))`` is k - 1 because the
    product rounds below k, and b's product reaches k + 1.  eps is a multiple of 2^-36 and a = mn + k * eps, so every sum here is
    exact whatever ``mn`` (a multiple of 2^-2) is; the issue's example is the first try when ``mn`` is 0 and k is small.
    Returns [(eps, a, b, k)]."""
    rng = np.random.default_rng(seed)
    eps = np.round(rng.uniform(0.2, 0.9, tries) * 2.0 ** 36) / 2.0 ** 36
    k = np.full(tries, BIG_K) if big else rng.integers(3, 40, tries)
    a = mn + k * eps
    b = a + eps
    if not big and mn == 0.0:
        eps[0], a[0], b[0], k[0] = ISSUE_PAIR["eps"], ISSUE_PAIR["a"], ISSUE_PAIR["b"], 2
    d = a - b
    e2, below = eps * eps, np.nextafter(eps, 0)
    inv = 1.0 / eps
    ca, cb = np.floor((a - mn) * inv), np.floor((b - mn) * inv)
    hit = (d * d <= e2) & (d * d > below * below) & (cb - ca == 2) & (ca == k - 1)
    return [(float(eps[i]), float(a[i]), float(b[i]), int(k[i])) for i in np.flatnonzero(hit)]


def _filler(rng, mn, eps, axis, lo, hi, count=12):
    """Lonely points: a lattice 3 eps wide on the two other axes (none within eps of another, nor of a pair at 4.5 eps on both),
    anywhere in [lo, hi] on ``axis``; the first is the grid's minimum corner."""
    u, v = (axis + 1) % 3, (axis + 2) % 3
    spots = [(i, j) for i in range(4) for j in range(4)][1:]
    f = np.empty((count, 3))
    for r, s in enumerate(rng.permutation(len(spots))[:count]):
        f[r, u], f[r, v] = mn[u] + 3.0 * eps * spots[s][0], mn[v] + 3.0 * eps * spots[s][1]
    f[:, axis] = rng.uniform(lo, hi, count)
    f[0] = mn                                                        # alone on its spot
    return f


@functools.lru_cache(maxsize=None)
def border_pair_case(axis, size, origin):
    """One found pair as the whole evidence of a cloud: with ``min_samples = 2`` the pair is the one cluster and every other
    point is noise; take one of the two away and the other is noise too.  ``xy``: the pair lies along x and straddles a cell
    border of y as well (one step of the doubles apart there: the squared distance does not feel it)."""
    ax = 0 if axis == "xy" else "xyz".index(axis)
    mn = np.zeros(3) if origin == "zero" else eg.MAP_ORIGIN.copy()
    seed = [71, PAIR_AXES.index(axis), size == "big", origin == "map"]
    found = border_pair_search(4000 if size == "small" else 400_000, seed, big=size == "big", mn=float(mn[ax]))
    eps, a, b, k = found[0]
    rng = np.random.default_rng(seed + [1])
    u, v = (ax + 1) % 3, (ax + 2) % 3
    pa = mn + 4.5 * eps
    pa[ax] = a
    pb = pa.copy()
    pb[ax] = b
    if axis == "xy":
        cell = eps * (1.0 + SLACK)
        border = mn[1] + 5.0 * cell
        ys = border + np.arange(-4, 5) * abs(np.spacing(border))
        cy = np.floor((ys - mn[1]) * (1.0 / cell))
        j = int(np.flatnonzero(np.diff(cy) == 1)[0])
        pa[1], pb[1] = ys[j], ys[j + 1]
    f = _filler(rng, mn, eps, ax, mn[ax], b + 3.0 * eps)             # b is not the axis' maximum: the clamp cannot step in
    f[1, ax] = b + 3.0 * eps
    cloud = np.concatenate([f[:5], [pb], f[5:9], [pa], f[9:]])
    return Case(f"border_{axis}_{size}_{origin}", [cloud], eps, 2, dict(a=10, b=5, axis=ax, k=k, tries=len(found)), below=True)


# ------------------------------------------------------------------------------------------------- grids
GROWN_EPS = 0.0625          # dyadic: a pair at exactly eps has a square of exactly eps * eps


@functools.lru_cache(maxsize=None)
def grown_grid_case():
    """eps = 1 / 16 over `points_cases.GROWN_EXTENT` (16 000 x 16 000 x 320 cells of eps: `build_cells` grows the cell several
    times).  30 tight clusters, and on dyadic coordinates pairs at exactly eps (neighbours: D1 is ``<=``) and pairs 2^-30 farther
    apart (not neighbours), along each axis; every pair is far from everything else."""
    rng = np.random.default_rng(2801)
    o = eg.MAP_ORIGIN
    src = pc._clusters(rng, o, o + np.array(pc.GROWN_EXTENT), 30, 40, 0.03)
    pairs, at = [], []
    for ax in range(3):
        for gap, tag in ((GROWN_EPS, "at"), (GROWN_EPS + 2.0 ** -30, "beyond")):
            for _ in range(4):
                a = o + np.round(rng.uniform(1.0, 19.0, 3) * 64.0) / 64.0
                a[:2] += np.round(rng.uniform(0.0, 900.0, 2))
                b = a.copy()
                b[ax] += gap
                at.append((tag, src.shape[0] + len(pairs), src.shape[0] + len(pairs) + 1))
                pairs += [a, b]
    return Case("grown_grid", [np.concatenate([src, np.array(pairs)])], GROWN_EPS, 2, dict(pairs=at))


@functools.lru_cache(maxsize=None)
def one_cell_case():
    """Every extent below eps: one cell on every axis, and the box's diagonal above eps, so not every pair is a neighbour."""
    rng = np.random.default_rng(2802)
    return Case("one_cell", [eg.MAP_ORIGIN + rng.uniform(0.0, 0.9 * 0.7, (300, 3))], 0.7, 230)


@functools.lru_cache(maxsize=None)
def last_cell_case(axis):
    """A pair at eps (dyadic, exact) along ``axis`` whose lower point is the minimum and whose upper point is the maximum of
    that axis: ONE cell there (the cell is eps and a hair), so the ring's upper end is the clamp.  The lonely points around it
    make the grid 9 cells wide on the other axes.  ``min_samples = 3``: the pair has two points, nobody is core -- unless a cell is
    met twice, as it is when the ring runs past the end of a row of x or y (past z there is only the table's end)."""
    ax = "xyz".index(axis)
    rng = np.random.default_rng([2803, ax])
    eps, mn = 0.5, eg.MAP_ORIGIN.copy()
    f = _filler(rng, mn, eps, ax, mn[ax], mn[ax] + eps)
    pa = mn + 4.5 * eps
    pa[ax] = mn[ax]
    pb = pa.copy()
    pb[ax] = mn[ax] + eps
    return Case(f"last_cell_{axis}", [np.concatenate([f[:6], [pa, pb], f[6:]])], eps, 3, dict(a=6, b=7, axis=ax))


@functools.lru_cache(maxsize=None)
def last_cell_wide_case():
    """The same pair at the far end of a 40-cell axis: its upper point is the maximum of x, in cell nx - 1."""
    rng = np.random.default_rng(2804)
    eps, mn = 0.5, eg.MAP_ORIGIN.copy()
    top = mn[0] + 39.0 * eps + 0.25
    f = _filler(rng, mn, eps, 0, mn[0], top - 2.0 * eps)
    pb = mn + 4.5 * eps
    pb[0] = top
    pa = pb.copy()
    pa[0] = top - eps
    return Case("last_cell_wide", [np.concatenate([f[:6], [pa, pb], f[6:]])], eps, 2, dict(a=6, b=7, axis=0))


# ------------------------------------------------------------------------------------------------- many clouds in one call
N_CLOUDS = 300
CLOUDS_EMPTY = (0, 100, 101, 102, 103, 104, N_CLOUDS - 1)
CLOUDS_SINGLE = (10, 11, N_CLOUDS - 2)
CLOUDS_EQUAL = (20, 21)
CLOUD_NOISE_FIRST = 30
CLOUD_NO_CLUSTER, CLOUD_AFTER_IT = 40, 41


@functools.lru_cache(maxsize=None)
def clouds_300_case():
    """300 clouds, jittered copies of one 40-point base (four blobs of eight and eight strays), so that they share their cells
    and only the cloud filter keeps them apart.  Empty clouds first, last and five in a row; single points; two bit-equal
    clouds; a cloud whose first point is noise; a cloud without a cluster right before one with clusters."""
    rng = np.random.default_rng(2805)
    eps = 0.3
    centres = np.array([[0.0, 0.0, 0.0], [1.5, 0.2, 0.1], [0.3, 1.6, -0.2], [1.7, 1.8, 0.3]])
    base = np.concatenate([(centres[:, None, :] + rng.normal(0.0, 0.15, (4, 8, 3))).reshape(-1, 3), rng.uniform(-0.5, 2.3, (8, 3))])
    perm = rng.permutation(40)
    base = eg.MAP_ORIGIN + base[np.roll(perm, -int(np.argmax(perm < 32)))]  # a blob's point first
    clouds = []
    for c in range(N_CLOUDS):
        p = base + rng.normal(0.0, 0.07, base.shape)
        if c in CLOUDS_EMPTY:
            p = np.zeros((0, 3))
        elif c in CLOUDS_SINGLE:
            p = p[c % 40:c % 40 + 1]
        elif c == CLOUDS_EQUAL[1]:
            p = clouds[CLOUDS_EQUAL[0]].copy()
        elif c == CLOUD_NOISE_FIRST:
            p[0] = eg.MAP_ORIGIN + [0.9, 0.9, 1.6]                   # inside the base's box, more than eps from everything
        elif c == CLOUD_NO_CLUSTER:
            p = eg.MAP_ORIGIN + 0.9 + (p - eg.MAP_ORIGIN - 0.9) * 6.0 # blown up about the centre: nobody has a neighbour
        clouds.append(np.ascontiguousarray(p))
    return Case("clouds_300", clouds, eps, 4)


# ------------------------------------------------------------------------------------------------- long chains
CHAIN_N = 20_000
CHAIN_EPS = 0.7
CHAIN_ORDERS = ("ascending", "descending", "evens_up_odds_down")
ROW, GAP = 60, 4            # 60 points a row, the rows 4 steps apart


def snake_path(n, eps):
    """n points 0.9 eps apart along a boustrophedon path: 60 points a row along x, then 4 steps along y to the next row.  The
    path of `test_gpu_dbscan.snake`, restated here so that the fixtures need no other test module."""
    step = np.zeros((n, 3))
    for i in range(1, n):
        k = i % (ROW + GAP - 1)
        if k >= ROW or k == 0:
            step[i, 1] = 1.0
        else:
            step[i, 0] = 1.0 if (i // (ROW + GAP - 1)) % 2 == 0 else -1.0
    return np.cumsum(step, axis=0) * (0.9 * eps)


@functools.lru_cache(maxsize=None)
def chain_case(order):
    """One path of 20 000 points 0.9 eps apart, ``min_samples = 2`` (every point is core): one cluster, number 0.  The index runs
    along the path, so every point's only smaller neighbour is its predecessor (``ascending``), or the union meets chains as
    long as the cluster: `db_find`, `db_unite` and `kd_flatten` walk them."""
    path = snake_path(CHAIN_N, CHAIN_EPS)
    i = np.arange(CHAIN_N)
    perm = {"ascending": i, "descending": i[::-1], "evens_up_odds_down": np.concatenate([i[::2], i[1::2][::-1]])}[order]
    return Case(f"chain_{order}", [np.ascontiguousarray(path[perm])], CHAIN_EPS, 2, dict(perm=perm))


def over_path(n, eps):
    """A second path for `snake_path`: its rows lie in the plane of the first path's, 1.01 eps beside them (the other side is
    2.59 eps away), three points shorter at either end; from the end of a row it climbs 1.8 eps, crosses the first path's row
    above it and comes down at the start of its next row.  Consecutive points are 0.9 eps apart."""
    s = 0.9 * eps
    pts, r = [], 0
    while len(pts) < n:
        xs = np.arange(3, ROW - 3) * s
        xs = xs if r % 2 == 0 else xs[::-1]
        y = r * GAP * s + 1.01 * eps
        pts += [(x, y, 0.0) for x in xs]
        pts += [(xs[-1], y, s), (xs[-1], y, 2 * s)] + [(xs[-1], y + k * s, 2 * s) for k in range(1, GAP + 1)] + [(xs[-1], y + GAP * s, s)]
        r += 1
    return np.array(pts[:n])


def _two_paths(n_each):
    """`snake_path` and `over_path`; the longer rows of the first reach past the ends of the second's."""
    a = snake_path(n_each, CHAIN_EPS)
    rows = int(round(a[:, 1].max() / (GAP * 0.9 * CHAIN_EPS)))
    b = over_path(n_each, CHAIN_EPS)
    b = b[b[:, 1] < (rows - 1) * GAP * 0.9 * CHAIN_EPS]              # stay beside rows the first path has
    return a, b


@functools.lru_cache(maxsize=None)
def two_chains_case():
    """Two paths with rows interleaved 1.01 eps apart, their indices interleaved too: exactly two clusters, the first path (index
    0) number 0."""
    a, b = _two_paths(CHAIN_N // 2)
    m = b.shape[0]
    both = np.empty((2 * m, 3))
    both[0::2], both[1::2] = a[:m], b
    p = np.concatenate([both, a[m:]])
    lab = np.zeros(p.shape[0], np.int32)
    lab[1:2 * m:2] = 1
    return Case("two_chains", [p], CHAIN_EPS, 2, dict(labels=lab, sizes=[a.shape[0], m]))


def _bridge_spot(a, b):
    """Half way between a point of the first path and the point of the second path 1.01 eps beside it, in the middle of a row:
    0.505 eps from both, 1.03 eps from their neighbours along the rows."""
    j = int(np.flatnonzero((np.abs(b[:, 0] - 30 * 0.9 * CHAIN_EPS) < 1e-9) & (b[:, 2] == 0.0))[5])
    i = int(np.argmin(((a - b[j]) ** 2).sum(axis=1)))
    return i, j, 0.5 * (a[i] + b[j])


@functools.lru_cache(maxsize=None)
def bridge_core_case():
    """The two paths one after the other in the index, and behind them one point between two of their rows, a neighbour of one
    point of each: with ``min_samples = 2`` it is core and the last index joins two clusters of ten thousand into one."""
    a, b = _two_paths((CHAIN_N - 2) // 2)
    i, j, spot = _bridge_spot(a, b)
    p = np.concatenate([a, b, [spot]])
    return Case("bridge_core", [p], CHAIN_EPS, 2, dict(touch=(i, a.shape[0] + j), bridge=p.shape[0] - 1))


@functools.lru_cache(maxsize=None)
def bridge_border_case():
    """The same joint with ``min_samples = 4``.  Every point of the paths comes twice (bit-equal, next to each other in the
    index), but for the two the joint touches: path points have 5 or 6 neighbours and are core, the joint has 3 (itself and one
    of each path) and is not.  Two clusters; the joint is a border point of both and takes number 0."""
    a, b = _two_paths((CHAIN_N - 2) // 4)
    i, j, spot = _bridge_spot(a, b)
    da, db = np.delete(np.repeat(a, 2, axis=0), 2 * i, axis=0), np.delete(np.repeat(b, 2, axis=0), 2 * j, axis=0)
    p = np.concatenate([da, db, [spot]])
    return Case("bridge_border", [p], CHAIN_EPS, 4, dict(touch=(2 * i, da.shape[0] + 2 * j), bridge=p.shape[0] - 1, split=da.shape[0]))


# ------------------------------------------------------------------------------------------------- the scan's tile edge
SCAN_NS = (SCAN_TILE - 1, SCAN_TILE, SCAN_TILE + 1)


@functools.lru_cache(maxsize=None)
def scan_edge_case(n):
    """``min_samples = 1``: every point is core.  n - 40 lonely points on a lattice 3 eps wide and 20 pairs 0.5 eps apart, shuffled,
    the last index a lonely point: a root, whose rank is the last entry the scan writes before ``rank[n]``."""
    rng = np.random.default_rng([2806, n])
    eps = 0.5
    m = n - 20
    side = int(np.ceil(m ** (1 / 3)))
    ijk = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:m]
    spots = eg.MAP_ORIGIN + 3.0 * eps * ijk[rng.permutation(m)]
    twins = spots[:20] + [0.5 * eps, 0.0, 0.0]
    p = np.concatenate([spots[:-1], twins])[rng.permutation(n - 1)]
    return Case(f"scan_edge_{n}", [np.concatenate([p, spots[-1:]])], eps, 1, dict(k=m))


# ------------------------------------------------------------------------------------------------- refusals
REFUSED_EPS = (1e-170, 1e160)         # eps * eps underflows to 0, overflows to inf


def refused_extent_cloud():
    p = np.random.default_rng(2807).uniform(0.0, 1.0, (50, 3))
    p[17, 1] = K["EXTENT_LIMIT"]
    return p


# ------------------------------------------------------------------------------------------------- every fixture
def cases():
    """name -> builder."""
    out = {}
    for axis in PAIR_AXES:
        for size in ("small", "big"):
            for origin in ("zero", "map"):
                out[f"border_{axis}_{size}_{origin}"] = functools.partial(border_pair_case, axis, size, origin)
    out.update(grown_grid=grown_grid_case, one_cell=one_cell_case, last_cell_wide=last_cell_wide_case, clouds_300=clouds_300_case,
               two_chains=two_chains_case, bridge_core=bridge_core_case, bridge_border=bridge_border_case)
    for axis in "xyz":
        out[f"last_cell_{axis}"] = functools.partial(last_cell_case, axis)
    for order in CHAIN_ORDERS:
        out[f"chain_{order}"] = functools.partial(chain_case, order)
    for n in SCAN_NS:
        out[f"scan_edge_{n}"] = functools.partial(scan_edge_case, n)
    return out


BORDER_NAMES = tuple(n for n in cases() if n.startswith("border_"))
# which fixtures must fail under which wrong search (tests/test_dbscan_cases.py asserts the whole table)
REJECTED_BY = {
    "no_slack": BORDER_NAMES,
    "lt": BORDER_NAMES + ("grown_grid", "last_cell_wide", "last_cell_x", "last_cell_y", "last_cell_z"),
    "no_clamp_hi": ("last_cell_x", "last_cell_y"),
    "same_cloud_ignored": ("clouds_300",),
}
