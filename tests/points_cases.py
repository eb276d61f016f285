"""Fixtures, host models and brute-force truths for the radius-mean pooling and the 1-NN re-projection
(``autoinst_amd/csrc/ai_points.hip``) and the dense cell list under them (``autoinst_amd/csrc/ai_cells.inc``).

Plain NumPy, seeded, no GPU and no library: tests/test_points_cases.py proves on the CPU that every fixture sits in the regime
its name claims and that a list of deliberately wrong rules is rejected; tests/test_gpu_points.py feeds the device's answers to
the same `check_*` helpers.

The limits are READ from the sources (`constants`): a changed constant moves the fixtures with it, and the CPU test proves
the regime claims again.

* `grid_of` / `cells_of` restate `build_cells`' grid (bounds, growth loop, nx, ny, nz) and `pcell_of`;
* `nn1_model` restates `kp_nn1`'s ring search with a pluggable stop rule: ``"shipped"`` (the face bound with its counted slack)
  or ``"parent"`` (``sqrt(best) <= r * cell - outside``, the rule before the rounding of `pcell_of` was counted);
* `pool_model` restates `kp_radius_mean`: the +-1 ring around the clamped cell, the strict predicate, sum then one division;
* the truths are brute force: `edge_geometry.nn1_brute` (plain square, ties to the smaller index, correctly rounded sqrt) and
  `pool_brute` (the predicate over all pairs, means by ``math.fsum``).
"""
from __future__ import annotations

import functools
import math
import os
import re
from dataclasses import dataclass, field

import numpy as np

import edge_geometry as eg

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "autoinst_amd", "csrc")
EPS = float(np.finfo(np.float64).eps)      # 2^-52, the kernels' `eps`
U = 2.0 ** -53                             # the unit roundoff


# ------------------------------------------------------------------------------------------------- constants from the sources
def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _find(text, pattern, what):
    m = re.search(pattern, text, re.M)
    if not m:
        raise RuntimeError(f"{what} not found in the sources")
    return m.group(1)


def constants():
    """The kernels' limits, parsed out of ``ai_common.h``, ``ai_points.hip`` and ``ai_cells.inc``."""
    common, points, cells = _read(_CSRC, "ai_common.h"), _read(_CSRC, "ai_points.hip"), _read(_CSRC, "ai_cells.inc")
    lanes = int(_find(points, r"const int c = t \+ (\d+) \* k;", "the lanes per query of kp_radius_mean"))
    if not re.search(r"gid >> 4;", points) or not re.search(r"gid & 15\)", points) or lanes != 16:
        raise RuntimeError("kp_radius_mean no longer gives 16 lanes to a query")
    c = dict(AI_BLOCK=int(_find(common, r"^\s*#define\s+AI_BLOCK\s+(\d+)", "AI_BLOCK")), LANES=lanes,
             MAXK=int(_find(points, r"constexpr int MAXK = (\d+);", "MAXK")),
             MAX_DIM=int(_find(points, r"dim <= 0 \|\| dim > (\d+)", "the widest feature row of ai_radius_mean_pool")),
             CELL_CAP=1 << int(_find(cells, r"\(double\)\(\(int64_t\)1 << (\d+)\)\) break;", "the cell cap of build_cells")),
             GROW=float(_find(cells, r"^\s*cell \*= ([0-9.]+);", "the growth factor of build_cells")),
             EXTENT_LIMIT=float(_find(cells, r"mx\[a\] - mn\[a\] < ([0-9.e+]+)\)", "the extent limit of build_cells")),
             NN1_CELL=float(_find(points, r'build_cells\(ctx, dfm, nf, ([0-9.]+), C, "ai_nn1_project"\)', "the cell of ai_nn1_project")),
             POOL_CELL_FACTOR=1.0 + float(_find(points, r"radius \* \(1\.0 \+ ([0-9.e-]+)\), C, \"ai_radius_mean_pool\"",
                                                "the cell factor of ai_radius_mean_pool")),
             SLACK_ULPS=float(_find(points, r"const double slack = ([0-9.]+) \* eps \*", "the slack of kp_nn1's stop rule")),
             STOP_ULPS=float(_find(points, r"sqrt\(best\) \* \(1\.0 \+ ([0-9.]+) \* eps\) <= lb", "kp_nn1's stop rule")))
    if c["MAX_DIM"] != c["LANES"] * c["MAXK"]:
        raise RuntimeError("dim <= 384 is no longer 16 lanes x MAXK accumulators")
    return c


K = constants()
BLOCK = K["AI_BLOCK"]
LANES = K["LANES"]
MAX_DIM = K["MAX_DIM"]
CELL_CAP = K["CELL_CAP"]
GROW = K["GROW"]
NN1_CELL = K["NN1_CELL"]
POOL_CELL_FACTOR = K["POOL_CELL_FACTOR"]
QUERIES_PER_BLOCK = BLOCK // LANES
POOL_RADIUS = eg.POOL_RADIUS


def pool_cell(radius):
    """The cell `ai_radius_mean_pool` asks `build_cells` for."""
    return float(radius) * POOL_CELL_FACTOR


# ------------------------------------------------------------------------------------------------- the grid of build_cells
@dataclass
class Grid:
    """`build_cells`' grid of one cloud, or of T clouds at once (every field with a leading axis of T)."""
    mn: np.ndarray          # (T, 3)
    mx: np.ndarray          # (T, 3)
    cell: np.ndarray        # (T,) the grown cell
    requested: float
    n: np.ndarray           # (T, 3) int64: nx, ny, nz

    @property
    def inv(self):
        return 1.0 / self.cell

    @property
    def ncell(self):
        return self.n[:, 0] * self.n[:, 1] * self.n[:, 2]

    @property
    def grown(self):
        return self.cell > self.requested


def grid_of(sources, cell, *, grow=True, nan="reject"):
    """The host part of `build_cells` for sources (S, 3) or (T, S, 3): bounds, the extent check, the growth loop, nx, ny, nz.
    ``nan="reject"``: a coordinate that is not finite counts as +inf (the shipped `kp_bounds`) and fails the extent check with
    ``ValueError``; ``nan="drop"`` folds with fmin / fmax, which lose a NaN (a wrong rule).  ``grow=False`` is a wrong rule too."""
    s = np.asarray(sources, dtype=np.float64)
    s = s[None] if s.ndim == 2 else s
    if nan == "reject":
        s = np.where(np.isfinite(s), s, np.inf)
    mn = np.fmin(np.fmin.reduce(s, axis=1), 1e300)
    mx = np.fmax(np.fmax.reduce(s, axis=1), -1e300)
    with np.errstate(invalid="ignore"):
        if not (mn <= mx).all() or not ((mx - mn) < K["EXTENT_LIMIT"]).all():
            raise ValueError("coordinates are not finite")
    c = np.full(s.shape[0], float(cell))
    while grow:
        e = np.floor((mx - mn) / c[:, None]) + 1.0
        big = (e[:, 0] * e[:, 1]) * e[:, 2] > float(CELL_CAP)
        if not big.any():
            break
        c = np.where(big, c * GROW, c)
    n = (np.floor((mx - mn) / c[:, None]).astype(np.int64) + 1)
    return Grid(mn, mx, c, float(cell), n)


def check_grid(name, g):
    """The dense table fits: at most CELL_CAP cells, of a cell no smaller than the one asked for."""
    assert (g.ncell <= CELL_CAP).all(), f"{name}: a table of {int(g.ncell.max())} cells, above the cap of {CELL_CAP}"
    assert (g.cell >= g.requested).all() and (g.n >= 1).all(), f"{name}: cell {g.cell} below the requested {g.requested}"


def cells_of(g, pts, clamp=True):
    """`pcell_of`: floor((p - min) * inv_cell), clamped to the grid.  pts (T or 1, ..., 3) against the T grids of ``g``."""
    p = np.asarray(pts, dtype=np.float64)
    shape = (-1,) + (1,) * (p.ndim - 2)
    c = np.floor((p - g.mn.reshape(shape + (3,))) * g.inv.reshape(shape + (1,))).astype(np.int64)
    return np.clip(c, 0, g.n.reshape(shape + (3,)) - 1) if clamp else c


# ------------------------------------------------------------------------------------------------- kp_nn1, ring by ring
NN1_MUTANTS = ("ties_larger", "no_clamp")


def _stop_parent(g, q, qc, r, best, cell):
    hi = g.mn + g.n * cell[:, None]
    o = np.fmax(np.fmax(g.mn - q, q - hi), 0.0)
    outside = np.sqrt(o[:, 0] * o[:, 0] + o[:, 1] * o[:, 1] + o[:, 2] * o[:, 2])
    return np.sqrt(best) <= r * cell - outside


def stop_slack(g, q, cell):
    """`kp_nn1`'s slack: SLACK_ULPS ulps of the largest |min| + (n + 1) * cell + |q| over the axes."""
    mag = ((np.abs(g.mn) + (g.n + 1).astype(np.float64) * cell[:, None]) + np.abs(q)).max(axis=1)
    return K["SLACK_ULPS"] * EPS * mag


def _stop_shipped(g, q, qc, r, best, cell):
    c = cell[:, None]
    with np.errstate(invalid="ignore"):
        lo = np.where(qc - r - 1 >= 0, q - (g.mn + (qc - r).astype(np.float64) * c), np.inf)
        hi = np.where(qc + r + 1 <= g.n - 1, (g.mn + (qc + r + 1).astype(np.float64) * c) - q, np.inf)
    lb = np.fmin(lo, hi).min(axis=1) - stop_slack(g, q, cell)
    return np.sqrt(best) * (1.0 + K["STOP_ULPS"] * EPS) <= lb


STOP_RULES = {"parent": _stop_parent, "shipped": _stop_shipped}


def nn1_model(queries, sources, *, cell=None, stop="shipped", mutant=None, chunk=256):
    """`kp_nn1` on the CPU: (index int32, distance, rings searched) for queries (T, 3) against sources (S, 3), one cloud for all
    queries, or (T, S, 3), a cloud of its own per query.  Ring r is every source whose stored cell is at Chebyshev distance r
    from the query's clamped cell; after each ring the stop rule is asked.  ``mutant`` breaks one rule on purpose."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    s = np.asarray(sources, dtype=np.float64)
    own = s.ndim == 3
    g = grid_of(s, NN1_CELL if cell is None else cell)
    sc = cells_of(g, s if own else s[None])
    rule = STOP_RULES[stop]
    T = q.shape[0]
    idx, dist, rings = np.empty(T, np.int32), np.empty(T), np.empty(T, np.int64)
    for a in range(0, T, chunk):
        b = min(T, a + chunk)
        gg = Grid(g.mn[a:b], g.mx[a:b], g.cell[a:b], g.requested, g.n[a:b]) if own else g
        qq = q[a:b]
        qc = cells_of(gg, qq)
        ss = s[a:b] if own else s[None]
        ring = np.abs((sc[a:b] if own else sc) - qc[:, None, :]).max(axis=2)
        d2 = eg.sq_plain(qq[:, None, :], ss)
        cell_stop = np.broadcast_to(gg.cell, (b - a,))
        t = b - a
        bi, best, used = np.full(t, -1, np.int64), np.full(t, 1e300), np.zeros(t, np.int64)
        live = np.ones(t, bool)
        rmax = np.broadcast_to(gg.n.max(axis=1), (t,))
        if mutant == "no_clamp":
            live &= (cells_of(gg, qq, clamp=False) == qc).all(axis=1)          # a query outside the grid finds nothing
        r = 0
        while live.any():
            d2m = np.where(ring <= r, d2, np.inf)
            if mutant == "ties_larger":
                k = d2m.shape[1] - 1 - np.argmin(d2m[:, ::-1], axis=1)
            else:
                k = np.argmin(d2m, axis=1)
            v = d2m[np.arange(t), k]
            found = np.isfinite(v)
            bi = np.where(live & found, k, bi)
            best = np.where(live & found, v, best)
            used = np.where(live, r, used)
            with np.errstate(invalid="ignore", over="ignore"):
                done = (bi >= 0) & rule(gg, qq, qc, r, best, cell_stop)
            live &= ~done & (r < rmax)
            r += 1
        idx[a:b], dist[a:b], rings[a:b] = bi, np.where(bi >= 0, np.sqrt(best), np.nan), used
    return idx, dist, rings


# ------------------------------------------------------------------------------------------------- kp_radius_mean
POOL_MUTANTS = ("le_predicate", "no_clamp", "no_divide", "drop_tail")


def _members(q, s, radius, mutant=None, a=0, b=None):
    d2 = eg.sq_plain(q[a:b, None, :], s[None, :, :])
    return d2 <= eg.r2_of(radius) if mutant == "le_predicate" else d2 < eg.r2_of(radius)


def pool_model(queries, sources, feat, radius, mutant=None, chunk=256):
    """`kp_radius_mean` on the CPU: (mean (nq, dim) float64, count int32).  A source is a member iff its stored cell is within one
    cell of the query's clamped cell on every axis and the predicate holds; the mean is the float64 sum, then one division."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    s = np.asarray(sources, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(feat, dtype=np.float32).astype(np.float64)
    g = grid_of(s, pool_cell(radius))
    sc = cells_of(g, s[None])[0]
    out, cnt = np.zeros((q.shape[0], f.shape[1])), np.zeros(q.shape[0], np.int32)
    for a in range(0, q.shape[0], chunk):
        b = min(q.shape[0], a + chunk)
        qc = cells_of(g, q[None, a:b])[0]
        m = _members(q, s, radius, mutant, a, b) & (np.abs(sc[None] - qc[:, None]).max(axis=2) <= 1)
        if mutant == "no_clamp":
            m &= (cells_of(g, q[None, a:b], clamp=False)[0] == qc).all(axis=1)[:, None]
        cnt[a:b] = m.sum(axis=1)
        for i in np.flatnonzero(cnt[a:b]):
            tot = f[m[i]].sum(axis=0)
            out[a + i] = tot if mutant == "no_divide" else tot / float(cnt[a + i])
    if mutant == "drop_tail" and f.shape[1] % LANES:
        out[:, f.shape[1] - f.shape[1] % LANES:] = 0.0
    return out, cnt


def pool_brute(queries, sources, feat, radius):
    """The truth: dict(count, mean, abs_sum).  Members by the predicate over ALL pairs, no grid; ``mean`` = ``math.fsum`` of the
    members' features (the correctly rounded sum) / count; ``abs_sum`` = the sum of their magnitudes, for the bound."""
    q = np.asarray(queries, dtype=np.float64).reshape(-1, 3)
    s = np.asarray(sources, dtype=np.float64).reshape(-1, 3)
    f = np.asarray(feat, dtype=np.float32).astype(np.float64)
    nq, dim = q.shape[0], f.shape[1]
    cnt, mean, asum = np.zeros(nq, np.int32), np.zeros((nq, dim)), np.zeros((nq, dim))
    for a in range(0, nq, 256):
        m = _members(q, s, radius, None, a, a + 256)
        for i in range(m.shape[0]):
            rows = f[m[i]]
            c = rows.shape[0]
            cnt[a + i] = c
            if c:
                mean[a + i] = [math.fsum(col) / c for col in rows.T]
                asum[a + i] = np.abs(rows).sum(axis=0)
    return {"count": cnt, "mean": mean, "abs_sum": asum}


def pool_bound(truth):
    """Per entry: the device sums cnt float64 terms one after the other, cnt - 1 roundings of partial sums that never exceed
    sum|f|, so its sum is within (cnt - 1) * 2^-53 * sum|f| of the exact one (first order); divided by cnt, plus one rounding
    of the division, 2^-53 * |mean|.  A single member (and an empty mean) must be exact."""
    cnt = np.maximum(truth["count"], 1).astype(np.float64)[:, None]
    return (cnt - 1.0) * U * truth["abs_sum"] / cnt + U * np.abs(truth["mean"])


def check_pool(name, got_mean, got_count, truth):
    got_mean = np.asarray(got_mean)
    if got_count is not None:
        bad = np.flatnonzero(np.asarray(got_count) != truth["count"])
        assert bad.size == 0, (f"{name}: {bad.size} counts differ, first at query {bad[:1]}: {np.asarray(got_count)[bad[:1]]} "
                               f"instead of {truth['count'][bad[:1]]}")
    assert got_mean.shape == truth["mean"].shape, f"{name}: shape {got_mean.shape} instead of {truth['mean'].shape}"
    empty = truth["count"] == 0
    assert not got_mean[empty].any(), f"{name}: a query without a member has a non-zero row"
    err, tol = np.abs(got_mean - truth["mean"]), pool_bound(truth)
    bad = np.argwhere(~(err <= tol))
    assert bad.shape[0] == 0, (f"{name}: {bad.shape[0]} means beyond the bound, first at {tuple(bad[0])}: "
                               f"{got_mean[tuple(bad[0])]!r} instead of {truth['mean'][tuple(bad[0])]!r} (bound {tol[tuple(bad[0])]:.3e})")


def check_nn1(name, idx, dist, truth):
    """Index equality and byte-equal distances against (index, distance) of `edge_geometry.nn1_brute`."""
    eidx, edist = truth
    idx = np.asarray(idx)
    bad = np.flatnonzero(idx != eidx)
    assert bad.size == 0, f"{name}: {bad.size} queries took another source, first query {bad[:1]}: {idx[bad[:1]]} instead of {eidx[bad[:1]]}"
    if dist is not None:
        d = np.ascontiguousarray(dist, dtype=np.float64)
        nb = int((d.view(np.int64) != np.ascontiguousarray(edist).view(np.int64)).sum())
        assert nb == 0, f"{name}: {nb} distances differ in their bits"


# ------------------------------------------------------------------------------------------------- fixtures
@dataclass
class Nn1Case:
    name: str
    queries: np.ndarray
    sources: np.ndarray
    claims: dict = field(default_factory=dict)

    @functools.cached_property
    def truth(self):
        return eg.nn1_brute(self.queries, self.sources)


@dataclass
class PoolCase:
    name: str
    queries: np.ndarray
    sources: np.ndarray
    feat: np.ndarray
    radius: float = POOL_RADIUS
    claims: dict = field(default_factory=dict)

    @functools.cached_property
    def truth(self):
        return pool_brute(self.queries, self.sources, self.feat, self.radius)


def _feat(rng, n, dim):
    return rng.standard_normal((n, dim)).astype(np.float32)


# ---- ring stop
ISSUE_CASE = {"anchor": -32.1, "A": -1.1000000000000048, "B": 0.899999999999995, "query": -0.10000000000000475}
GROWN_EXTENT = (1000.0, 1000.0, 20.0)      # 2001 x 2001 x 41 cells of 0.5 m: above the cap, one growth step to 0.75 m


def ring_stop_search(tries, seed, *, grown=False, outside=False, keep=0):
    """The construction of the issue's case at random: on a random axis, direction ``sgn`` and ring r, a query q just below a cell
    border, a source B just below the border r cells further on, a source A at r cells from q on the other side, and the
    anchor that fixes the grid's minimum.  The two offsets below their borders are a few ulps of the coordinate, so whether
    ``fl(p - min)`` rounds a point onto its border is left to chance.  The point nearer the minimum must keep its place and
    the other must be rounded up although it lies further below its border: that needs a coarser spacing of the doubles at
    the second, so a power of two (in metres from the minimum) lies between the two borders, or on the lower one.
    ``outside``: the query sits one ulp below the cloud on another axis.
    ``grown``: a far corner (`GROWN_EXTENT`) makes `build_cells` grow the cell.

    Returns dict(tries, miss_parent, miss_shipped, cases): the number of tries in which `nn1_model` with either stop rule
    differs from brute force, and up to ``keep`` missed cases per (axis, sgn, r) as dict(axis, sgn, r, query, sources, A, B)."""
    rng = np.random.default_rng(seed)
    T = int(tries)
    axis, sgn, r = rng.integers(0, 3, T), rng.choice([-1, 1], T), rng.integers(1, 4, T)
    mn = np.where(rng.random(T) < 0.5, -np.round(rng.uniform(5.0, 60.0, T), 1), -rng.uniform(5.0, 60.0, T))
    cell = NN1_CELL * GROW if grown else NN1_CELL
    P = 2.0 ** rng.integers(3, 7, T)                          # 8 .. 64 m from the minimum the spacing of the doubles doubles
    kl = np.floor(P / cell).astype(np.int64) - rng.integers(0, 3, T) % r      # a border at or below P, within r cells of it
    ku = kl + r                                               # and the border r cells on, above P
    kq = np.where(sgn > 0, kl, ku)                            # q just below border kq, B just below border kb
    kb = np.where(sgn > 0, ku, kl)
    h = np.spacing(P)
    xq = mn + kq * cell - rng.uniform(0.0, 2.0, T) * h
    xb = mn + kb * cell - rng.uniform(0.0, 2.0, T) * h
    xa = xq - sgn * (r * cell)
    w0 = 2.0 ** -10 if outside else 0.0                       # the line's place on the other axes
    b_first = rng.random(T) < 0.5                             # B before A: an exact tie goes to B
    src = np.full((T, 4 if grown else 3, 3), w0)
    t = np.arange(T)
    src[t, 0, axis] = mn
    src[t, 1, axis] = np.where(b_first, xb, xa)
    src[t, 2, axis] = np.where(b_first, xa, xb)
    if grown:
        ext = np.array(GROWN_EXTENT)
        far = np.where((axis == 2)[:, None], ext[[2, 1, 0]], ext) + w0
        far[t, axis] += mn - w0
        src[:, 3] = far
    q = np.full((T, 3), w0)
    q[t, axis] = xq
    if outside:
        q[t, (axis + 1) % 3] = np.nextafter(w0, -1.0)
    truth = np.argmin(eg.sq_plain(q[:, None, :], src), axis=1)
    got = {rule: nn1_model(q, src, stop=rule, chunk=1 << 16)[0] for rule in STOP_RULES}
    miss = {rule: got[rule] != truth for rule in STOP_RULES}
    cases, seen = [], {}
    for i in np.flatnonzero(miss["parent"]) if keep else ():
        key = (int(axis[i]), int(sgn[i]), int(r[i]))
        if seen.get(key, 0) < keep:
            seen[key] = seen.get(key, 0) + 1
            cases.append(dict(axis=key[0], sgn=key[1], r=key[2], query=q[i], sources=src[i], A=int(got["parent"][i]), B=int(truth[i])))
    return {"tries": T, "miss_parent": int(miss["parent"].sum()), "miss_shipped": int(miss["shipped"].sum()), "cases": cases}


def _embed(case, rng, name, variant, fill=40):
    """The line of a found case inside a filler cloud that makes the grid 3-D.  The filler stays strictly inside the line's
    range on the case's axis (the grid's minimum and cell count there stay the case's) and at least 3 m from the line on the
    other axes (with ``outside`` on their upper side only, so the query stays below the cloud)."""
    ax = case["axis"]
    line = case["sources"]
    lo, hi = line[:, ax].min(), line[:, ax].max()
    f = np.empty((fill, 3))
    f[:, ax] = rng.uniform(lo + 0.01, min(hi, lo + 80.0) - 0.01, fill)
    ang = rng.uniform(0.0, 0.5 * np.pi if variant == "outside" else 2.0 * np.pi, fill)
    rad = rng.uniform(3.0, 5.0, fill)
    w0 = line[0, (ax + 1) % 3]
    f[:, (ax + 1) % 3] = w0 + rad * np.cos(ang)
    f[:, (ax + 2) % 3] = w0 + rad * np.sin(ang)
    return Nn1Case(name, case["query"][None, :].copy(), np.concatenate([line, f]),
                   dict(A=case["A"], B=case["B"], axis=ax, sgn=case["sgn"], r=case["r"], variant=variant))


def issue_case():
    """The case written out in the issue, as it stands: y = z = 0, three sources, one query."""
    src = np.array([[ISSUE_CASE["anchor"], 0, 0], [ISSUE_CASE["A"], 0, 0], [ISSUE_CASE["B"], 0, 0]])
    return Nn1Case("ring_stop_issue", np.array([[ISSUE_CASE["query"], 0, 0]]), src,
                   dict(A=1, B=2, axis=0, sgn=1, r=2, variant="plain"))


@functools.lru_cache(maxsize=None)
def ring_stop_cases():
    """A few dozen one-query clouds on which the parent's stop rule answers A although B is nearer (or tied with the smaller
    index): one per axis, direction and ring 1, 2, 3 (``plain``), some with the query one ulp outside the box on another axis
    (``outside``), some on a grown 0.75 m cell (``grown``), and the issue's own."""
    out = [issue_case()]
    rng = np.random.default_rng(606)
    for variant, tries, seed, per, limit in (("plain", 120_000, 11, 1, 18), ("outside", 60_000, 12, 1, 6), ("grown", 120_000, 13, 1, 6)):
        found = ring_stop_search(tries, seed, grown=variant == "grown", outside=variant == "outside", keep=per)["cases"]
        found.sort(key=lambda c: (c["r"], c["axis"], c["sgn"]))
        if limit < len(found):                                  # spread over rings, axes and directions
            found = found[::max(1, len(found) // limit)][:limit]
        for c in found:
            out.append(_embed(c, rng, f"ring_stop_{variant}_{'xyz'[c['axis']]}{'+' if c['sgn'] > 0 else '-'}_r{c['r']}", variant))
    return out


# ---- the growth branch
def _clusters(rng, lo, hi, n_clusters, per, sigma):
    lo, hi = np.asarray(lo, np.float64), np.asarray(hi, np.float64)
    centres = rng.uniform(lo + 5 * sigma, hi - 5 * sigma, (n_clusters, 3))
    pts = centres[:, None, :] + rng.normal(0.0, sigma, (n_clusters, per, 3))
    return np.clip(np.concatenate([[lo, hi], pts.reshape(-1, 3)]), lo, hi)


def under_cap_extent(cell):
    """The extent of a box of exactly CELL_CAP cells of ``cell``, 2^k x 2^k x the rest (2048 x 2048 x 32 at 2^27): the largest
    that `build_cells` does not grow."""
    e = CELL_CAP.bit_length() - 1
    assert CELL_CAP == 1 << e
    side = 1 << ((e + 6) // 3)
    n = np.array([side, side, CELL_CAP // (side * side)])
    return (n - 0.5) * cell


@functools.lru_cache(maxsize=None)
def growth_nn1_case():
    """3002 sources in 30 clusters in a 1000 x 1000 x 20 m box (above the cap at 0.5 m), 1000 queries each within 0.5 m of a
    source on every axis: under two cells of the grown grid."""
    rng = np.random.default_rng(2701)
    o = eg.MAP_ORIGIN
    src = _clusters(rng, o, o + np.array(GROWN_EXTENT), 30, 100, 0.4)
    src = src[rng.permutation(src.shape[0])]
    q = src[rng.integers(0, src.shape[0], 1000)] + rng.uniform(-0.5, 0.5, (1000, 3))
    return Nn1Case("growth_nn1", q, src, dict(grown=True))


@functools.lru_cache(maxsize=None)
def growth_pool_case():
    """3002 sources in 60 clusters in a 100.1 m cube (573^3 cells of 0.175 m: above the cap), 500 queries within 0.15 m of a
    source on every axis, 16 features."""
    rng = np.random.default_rng(2702)
    o = eg.MAP_ORIGIN
    src = _clusters(rng, o, o + 100.1, 60, 50, 0.1)
    src = src[rng.permutation(src.shape[0])]
    q = src[rng.integers(0, src.shape[0], 500)] + rng.uniform(-0.15, 0.15, (500, 3))
    return PoolCase("growth_pool", q, src, _feat(rng, src.shape[0], 16), POOL_RADIUS, dict(grown=True))


# ---- small clouds: widths, block edges, degenerate grids
def _small_cloud(rng, ns, nq, origin=eg.MAP_ORIGIN, side=1.0):
    src = origin + rng.uniform(0.0, side, (ns, 3))
    q = src[rng.integers(0, ns, nq)] + rng.uniform(-0.12, 0.12, (nq, 3))
    return q, src


POOL_WIDTHS = (1, LANES - 1, LANES, LANES + 1, 96, MAX_DIM - 1, MAX_DIM)
POOL_NQ = (1, QUERIES_PER_BLOCK - 1, QUERIES_PER_BLOCK, QUERIES_PER_BLOCK + 1)
NN1_NT = (BLOCK - 1, BLOCK, BLOCK + 1)
DEGENERATE = ("one_source", "identical", "coplanar", "collinear")


@functools.lru_cache(maxsize=None)
def pool_width_case(dim):
    rng = np.random.default_rng([31, dim])
    q, src = _small_cloud(rng, 400, QUERIES_PER_BLOCK + 1)
    return PoolCase(f"pool_width_{dim}", q, src, _feat(rng, 400, dim), POOL_RADIUS, dict(dim=dim, tail=dim % LANES))


@functools.lru_cache(maxsize=None)
def pool_nq_case(nq):
    rng = np.random.default_rng([32, nq])
    q, src = _small_cloud(rng, 400, nq)
    return PoolCase(f"pool_nq_{nq}", q, src, _feat(rng, 400, LANES + 1), POOL_RADIUS, dict(nq=nq))


@functools.lru_cache(maxsize=None)
def nn1_nt_case(nt):
    rng = np.random.default_rng([33, nt])
    src = eg.MAP_ORIGIN + rng.uniform(0.0, 6.0, (300, 3))
    q = eg.MAP_ORIGIN + rng.uniform(-1.0, 7.0, (nt, 3))
    return Nn1Case(f"nn1_nt_{nt}", q, src, dict(nt=nt))


def _degenerate_sources(kind, rng):
    o = eg.MAP_ORIGIN
    if kind == "one_source":
        return o[None, :] + 0.1
    if kind == "identical":
        return np.tile(o + [0.3, 0.1, 0.2], (50, 1))
    s = o + rng.uniform(0.0, 3.0, (200, 3))
    if kind == "coplanar":
        s[:, 2] = o[2]
    else:
        s[:, 1:] = o[1:]
    return s


@functools.lru_cache(maxsize=None)
def degenerate_nn1_case(kind):
    rng = np.random.default_rng([34, DEGENERATE.index(kind)])
    src = _degenerate_sources(kind, rng)
    q = np.concatenate([src[rng.integers(0, src.shape[0], 40)] + rng.uniform(-0.4, 0.4, (40, 3)), src[:3],
                        eg.MAP_ORIGIN + rng.uniform(-3.0, 6.0, (40, 3))])
    return Nn1Case(f"nn1_{kind}", q, src, dict(kind=kind))


@functools.lru_cache(maxsize=None)
def degenerate_pool_case(kind):
    rng = np.random.default_rng([35, DEGENERATE.index(kind)])
    src = _degenerate_sources(kind, rng)
    q = np.concatenate([src[rng.integers(0, src.shape[0], 40)] + rng.uniform(-0.1, 0.1, (40, 3)), src[:3],
                        eg.MAP_ORIGIN + rng.uniform(-1.0, 4.0, (20, 3))])
    return PoolCase(f"pool_{kind}", q, src, _feat(rng, src.shape[0], LANES + 1), POOL_RADIUS, dict(kind=kind))


# ---- clamped queries
def _directions():
    d = np.array([[i, j, k] for i in (-1, 0, 1) for j in (-1, 0, 1) for k in (-1, 0, 1) if (i, j, k) != (0, 0, 0)], np.float64)
    return d                                                      # 6 faces, 12 edges, 8 corners


@functools.lru_cache(maxsize=None)
def clamp_pool_case(where):
    """A 5 x 5 x 5 lattice of sources 0.5 m apart (the box is about 12 cells a side).  ``near``: per face, edge and corner of the
    box a query 0.09 m outside it on each of the direction's axes (0.156 m from the corner source at most: inside the radius);
    ``far``: 0.2 m outside on each axis (more than the radius from every source)."""
    rng = np.random.default_rng(36)
    o = eg.MAP_ORIGIN
    ijk = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    src = o + ijk * 0.5
    d = _directions()
    face = np.where(d > 0, 2.0, 0.0)                              # the source on that face / edge / corner: the lattice's own
    base = o + np.where(d == 0, 1.0, face)
    q = base + d * (0.09 if where == "near" else 0.2)
    return PoolCase(f"clamp_pool_{where}", q, src[rng.permutation(src.shape[0])], _feat(rng, src.shape[0], LANES + 1), POOL_RADIUS,
                    dict(where=where))


@functools.lru_cache(maxsize=None)
def clamp_nn1_case():
    """300 sources in a 15 m box (31 cells a side); queries 1e-3 .. 1e6 m outside it over every face, edge and corner."""
    rng = np.random.default_rng(37)
    o = eg.MAP_ORIGIN
    src = np.concatenate([o + rng.uniform(0.0, 15.0, (298, 3)), [o + 15.0, o]])
    d = _directions()
    q = []
    for dist in (1e-3, 0.3, 7.0, 1e3, 1e6):
        inside = o + rng.uniform(0.0, 15.0, (d.shape[0], 3))
        q.append(np.where(d == 0, inside, np.where(d > 0, o + 15.0 + dist, o - dist) + rng.uniform(0.0, 0.1, d.shape) * d * dist))
    return Nn1Case("clamp_nn1", np.concatenate(q), src, dict(max_cells=40))


# ---- cell borders of the pooling grid
@functools.lru_cache(maxsize=None)
def pool_border_case():
    """Cell = radius * (1 + 1e-9): neither it nor its inverse is a power of two, so `pcell_of`'s product rounds.  The sources'
    minimum is `MAP_ORIGIN`.  Per border k (several per axis): a query one ulp below it with a source one ulp above it and the
    other way round (``straddle``), and a query one ulp above it with a source 0.999999 radius below the query, most of a cell
    into the neighbouring cell (``reach``)."""
    rng = np.random.default_rng(38)
    o = eg.MAP_ORIGIN
    cell = pool_cell(POOL_RADIUS)
    q, s, kind = [], [o.copy(), o + 40 * cell], ["anchor", "anchor"]
    qkind = []
    for ax in range(3):
        for k in (1, 2, 3, 7, 16, 31, 32, 33):
            border = o[ax] + k * cell
            lo, hi = np.nextafter(border, -np.inf), np.nextafter(border, np.inf)
            for a, b, what in ((lo, hi, "straddle"), (hi, lo, "straddle"), (hi, hi - 0.999999 * POOL_RADIUS, "reach")):
                p = o + rng.uniform(1.0, 5.0, 3)
                pq, ps = p.copy(), p.copy()
                pq[ax], ps[ax] = a, b
                q.append(pq)
                s.append(ps)
                qkind.append(what)
                kind.append(what)
    s = np.array(s)
    return PoolCase("pool_border", np.array(q), s, _feat(rng, s.shape[0], LANES + 1), POOL_RADIUS, dict(qkind=qkind, skind=kind))


# ---- one crowded cell, and the predicate at the exact radius
@functools.lru_cache(maxsize=None)
def pool_crowded_case():
    """4000 sources, 800 of them copies of others, inside a ball of 0.04 m: every one of the 16 queries (inside the ball too)
    pools them all."""
    rng = np.random.default_rng(39)
    c = eg.MAP_ORIGIN + [0.3, 0.4, 0.5]
    u = rng.standard_normal((3200, 3))
    base = c + u / np.linalg.norm(u, axis=1, keepdims=True) * (0.04 * rng.random((3200, 1)) ** (1 / 3))
    src = np.concatenate([base, base[rng.integers(0, 3200, 800)]])
    src = src[rng.permutation(4000)]
    q = c + rng.uniform(-0.02, 0.02, (QUERIES_PER_BLOCK, 3))
    return PoolCase("pool_crowded", q, src, _feat(rng, 4000, LANES + 1), POOL_RADIUS, dict(members=4000))


@functools.lru_cache(maxsize=None)
def pool_exact_radius_case():
    """Radius 0.25 on dyadic coordinates: per query six sources at exactly the radius (the square equals radius * radius: out,
    the predicate is strict) and six 2^-30 nearer (in)."""
    rng = np.random.default_rng(40)
    q = np.array([[4.0, -2.5, 1.25], [6.0, -2.5, 1.25], [4.0, 1.0, 3.0]])
    s = []
    for p in q:
        for ax in range(3):
            for sg in (-1.0, 1.0):
                for d in (0.25, 0.25 - 2.0 ** -30):
                    t = p.copy()
                    t[ax] += sg * d
                    s.append(t)
    s = np.array(s)
    return PoolCase("pool_exact_radius", q, s, _feat(rng, s.shape[0], 2), 0.25, dict(at_radius=6, inside=6))


# ---- input that is not finite, arguments that are refused
NONFINITE = (np.nan, np.inf, -np.inf)


def nonfinite_sources():
    """name -> (S, 3) sources with one coordinate that is not finite, at the front, in the middle or at the end."""
    rng = np.random.default_rng(41)
    out = {}
    for v, tag in zip(NONFINITE, ("nan", "inf", "neginf")):
        for ax in range(3):
            s = eg.MAP_ORIGIN + rng.uniform(0.0, 4.0, (300, 3))
            s[(0, 150, 299)[ax], ax] = v
            out[f"source_{tag}_{'xyz'[ax]}"] = s
    s = eg.MAP_ORIGIN + rng.uniform(0.0, 4.0, (300, 3))
    s[:, 1] = np.nan
    out["source_nan_whole_axis"] = s
    return out


@functools.lru_cache(maxsize=None)
def nonfinite_query_case():
    """300 sources in a 15 m box (31 cells a side: a query that walks the whole grid is done in milliseconds); every fourth of
    the 64 queries has one coordinate that is not finite: index -1 and a NaN distance; the others are ordinary."""
    rng = np.random.default_rng(42)
    src = eg.MAP_ORIGIN + rng.uniform(0.0, 15.0, (300, 3))
    q = eg.MAP_ORIGIN + rng.uniform(-2.0, 17.0, (64, 3))
    bad = np.arange(0, 64, 4)
    for j, i in enumerate(bad):
        q[i, j % 3] = NONFINITE[(j // 3) % 3]
    return Nn1Case("nn1_nonfinite_query", q, src, dict(bad=bad, max_cells=40))


def nonfinite_query_truth(case):
    """(index, distance): brute force on the finite queries, -1 / NaN on the others."""
    bad = case.claims["bad"]
    ok = np.setdiff1d(np.arange(case.queries.shape[0]), bad)
    idx, dist = np.full(case.queries.shape[0], -1, np.int32), np.full(case.queries.shape[0], np.nan)
    idx[ok], dist[ok] = eg.nn1_brute(case.queries[ok], case.sources)
    return idx, dist


POOL_BAD_ARGS = {"dim_385": dict(dim=MAX_DIM + 1), "dim_0": dict(dim=0), "radius_0": dict(radius=0.0), "radius_negative": dict(radius=-0.175),
                 "radius_nan": dict(radius=float("nan"))}


# ---- every fixture by family
def nn1_cases():
    return (list(ring_stop_cases()) + [growth_nn1_case(), clamp_nn1_case()] + [nn1_nt_case(n) for n in NN1_NT] +
            [degenerate_nn1_case(k) for k in DEGENERATE])


def pool_cases():
    return ([pool_width_case(d) for d in POOL_WIDTHS] + [pool_nq_case(n) for n in POOL_NQ] + [degenerate_pool_case(k) for k in DEGENERATE] +
            [clamp_pool_case("near"), clamp_pool_case("far"), pool_border_case(), pool_crowded_case(), pool_exact_radius_case(),
             growth_pool_case()])
