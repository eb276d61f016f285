"""Fixtures and traced walks for hidden point removal on the device (``autoinst_amd/csrc/ai_hidden.hip``, rules H1-H6 of
``include/autoinst_hip.h``) at the limits of its kernels.

Plain NumPy, seeded, no GPU (only `skip_regime_case` needs the package, for the synthetic rig): tests/test_hpr_cases.py proves on the CPU that every fixture sits where its name says
(which re-solve falls where in `kh_local`'s walk of a cell and in `kh_global`'s walk of the tiles) and that the re-solve counts
tell a wrong skip rule from the shipped one; tests/test_gpu_hpr_cases.py compares the device with the restatement, everything
equal.  The truth is `hpr_ref` (flags and the four statistics).

The limits are READ from the sources (`constants`): a changed constant moves the fixtures with it.  The seeds in `SEEDS` were
found by `seed_search` (seeded itself): the CPU test proves the claims of every committed seed again.

* `walk` is the local and the global pass of every point as the device runs them: the local list by its 27 segments (one lane of
  `kh_local` each), the global list by tiles under a skip-rule variant of `hpr_ref.can_skip`.  It records where every re-solve
  falls, and counts them as `kh_global` would under that variant.
"""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass, field

import numpy as np

import hpr_ref
import points_cases as pc


# ------------------------------------------------------------------------------------------------- constants from the sources
def constants():
    """The limits of `ai_hidden_points`, parsed out of ``ai_hidden.hip`` and ``ai_common.h``."""
    src = pc._read(pc._CSRC, "ai_hidden.hip")
    num = lambda name, pat: pc._find(src, r"^\s*#define\s+" + name + r"\s+(" + pat + r")", name)
    c = dict(HP_GRID=int(num("HP_GRID", r"\d+")), HP_TILE=int(num("HP_TILE", r"\d+")), HP_STEP=int(num("HP_STEP", r"\d+")),
             HP_BOX=float(num("HP_BOX", r"[0-9.e+-]+")), HP_SKIP_EPS=float(num("HP_SKIP_EPS", r"[0-9.e+-]+")), AI_BLOCK=pc.K["AI_BLOCK"])
    if not re.search(r"tile\[HP_TILE \+ HP_STEP\]", src) or not re.search(r"base \+= 64;", src):
        raise RuntimeError("kh_global no longer pads its tile by HP_STEP records, or kh_local no longer walks 64 records a turn")
    return c


K = constants()
GRID, TILE, STEP, BLOCK = K["HP_GRID"], K["HP_TILE"], K["HP_STEP"], K["AI_BLOCK"]
WAVE = 64                       # records of a cell that kh_local tests per turn
HPR_RADIUS = 1000.0             # the drop-in's radius factor (autoinst_amd.config.HPR_RADIUS)
SKIP_VARIANTS = ("own_u", "no_t")


# ------------------------------------------------------------------------------------------------- the traced walks
def segments(pr, p):
    """The local list of sorted point p as `kh_local` holds it: [(lane s, start, end)] of the cells that are not empty, the
    point's own cell in lane 0, then the others in (dz, dy, dx) order."""
    skey, (cx, cy, cz) = pr["skey"], pr["cell"][p]
    out = []
    for s, (dx, dy, dz) in enumerate(hpr_ref._OFFSETS):
        xx, yy, zz = cx + dx, cy + dy, cz + dz
        if 0 <= xx < GRID and 0 <= yy < GRID and 0 <= zz < GRID:
            k = (zz * GRID + yy) * GRID + xx
            a, b = int(np.searchsorted(skey, k, "left")), int(np.searchsorted(skey, k, "right"))
            if b > a:
                out.append((s, a, b))
    return out


def walk(p_cam, radius_factor, variant="rule"):
    """Both passes of every point of a view, as the device runs them.  Returns None for a skipped view, else a dict:

    flags (input order), stats (local_hidden, resolves, max_resolves, at_camera: what `kh_global` and `kh_local` would count
    under ``variant``), local: per sorted point [(list position, lane s, position in the lane's cell)] of its local re-solves,
    glob: per sorted point the sorted positions of its global re-solves (None for a point the local pass decided), survivors,
    met / passed / unsound: the tiles the survivors met, passed over, and passed over although a constraint of the tile was
    violated at the lane's t."""
    pr = hpr_ref.prepare(p_cam, radius_factor)
    if pr is None:
        return None
    E, U, n, order = pr["E"], pr["U"], pr["n"], pr["order"]
    boxes, u_min = hpr_ref.tile_boxes(E), U.min()
    assert hpr_ref.TILE == TILE and hpr_ref.GRID == GRID
    flags = np.zeros(n, dtype=np.uint8)
    st = {"local_hidden": 0, "resolves": 0, "max_resolves": 0, "at_camera": 0}
    local, glob = [None] * n, [None] * n
    met = passed = unsound = survivors = 0
    for p in range(n):
        ex, ey, ez, u = E[p, 0], E[p, 1], E[p, 2], U[p]
        if ex == 0.0 and ey == 0.0 and ez == 0.0:
            st["at_camera"] += 1
            continue
        A0, A1, g = hpr_ref.constraints(ex, ey, ez, u, E, U)
        seg = segments(pr, p)
        loc = np.concatenate([np.arange(a, b) for _, a, b in seg])
        ends = np.cumsum([b - a for _, a, b in seg])
        tr = []
        ok, t0, t1, nres = hpr_ref.seidel(A0[loc], A1[loc], g[loc], 0.0, 0.0, trace=tr)
        which = np.searchsorted(ends, tr, "right")
        local[p] = [(k, seg[w][0], k - (int(ends[w - 1]) if w else 0)) for k, w in zip(tr, which)]
        if not ok:
            st["local_hidden"] += 1
        else:
            survivors += 1
            tr = []
            for k, a in enumerate(range(0, n, TILE)):
                b = min(a + TILE, n)
                met += 1
                if hpr_ref.can_skip(ex, ey, ez, u, t0, t1, boxes[k], u_min, variant):
                    passed += 1
                    with np.errstate(all="ignore"):
                        unsound += int(((t0 * A0[a:b] + t1 * A1[a:b]) > g[a:b]).any())
                    continue
                ok, t0, t1, _ = hpr_ref._seidel_range(A0, A1, g, t0, t1, a, b, trace=tr)
                if not ok:
                    break
            glob[p] = tr
            nres += len(tr)
        st["resolves"] += nres
        st["max_resolves"] = max(st["max_resolves"], nres)
        flags[order[p]] = 1 if ok else 0
    return dict(flags=flags, stats=st, local=local, glob=glob, survivors=survivors, met=met, passed=passed, unsound=unsound, n=n)


def stats_list(st):
    """The statistics in the order of the library's stats_out."""
    return [st["local_hidden"], st["resolves"], st["max_resolves"], st["at_camera"]]


# ------------------------------------------------------------------------------------------------- fixtures and their truth
@dataclass
class Case:
    name: str
    points: np.ndarray      # (n, 3) in the camera frame
    factor: float = HPR_RADIUS
    claims: dict = field(default_factory=dict)

    @functools.cached_property
    def truth(self):
        """(ascending visible rows or None, [local_hidden, resolves, max_resolves, at_camera] or None): `hpr_ref`."""
        st = {}
        flags = hpr_ref.visible_flags(self.points, self.factor, stats=st)
        if flags is None:
            return None, None
        return np.flatnonzero(flags).astype(np.int64), stats_list(st)

    @functools.cached_property
    def walked(self):
        return walk(self.points, self.factor)


def cell_population(c):
    """{cell key: points} of the direction grid of a fixture."""
    pr = hpr_refprepare(c)
    keys, counts = np.unique(pr["skey"], return_counts=True)
    return dict(zip(keys.tolist(), counts.tolist()))


def hpr_refprepare(c):
    return hpr_ref.prepare(c.points, c.factor)


# ---- crowded direction cells
CELL_POPULATIONS = (WAVE - 1, WAVE, WAVE + 1, 2 * WAVE - 1, 2 * WAVE, 2 * WAVE + 1, 300)
RING_OFFSETS = {"face": (1, 0, 0), "edge": (1, 1, 0), "corner": (1, 1, 1)}
HALF_WIDTH = 0.003          # of the directions' spread: a tenth of a cell (2 / HP_GRID)
QUERY_CELL_POINTS = 6


def _cell_coords(e):
    v = (np.asarray(e) + 1.0) * (GRID / 2.0)
    return np.floor(v), v - np.floor(v)


@functools.lru_cache(maxsize=None)
def _direction_table():
    """One draw of seeded random unit directions away from the grid's rim: (directions, cells, places inside the cells)."""
    e = np.random.default_rng(81).standard_normal((1_500_000, 3))
    e /= np.linalg.norm(e, axis=1)[:, None]
    c, f = _cell_coords(e)
    ok = (c >= 2).all(axis=1) & (c <= GRID - 3).all(axis=1)
    return e[ok], c[ok].astype(np.int64), f[ok]


@functools.lru_cache(maxsize=None)
def centred_directions(where):
    """(e0, e1): unit directions in neighbouring cells, e1's across a face, an edge or a corner of e0's, each 0.2 cells from the
    border between them on the axes they differ in and in the middle of its cell on the others (``own``: one direction in the
    middle of a cell): the first such pair of one seeded draw.  A near point hides a far one only within about a degree and a
    half (a cell is 1.8 degrees wide), so the two groups sit near their common border."""
    e, c, f = _direction_table()
    off = np.array(RING_OFFSETS.get(where, (0, 0, 0)), dtype=np.int64)
    tol = np.where(off == 1, 0.05, 0.2)
    first = np.flatnonzero((np.abs(f - np.where(off == 1, 0.8, 0.5)) < tol).all(axis=1))
    second = np.flatnonzero((np.abs(f - np.where(off == 1, 0.2, 0.5)) < tol).all(axis=1))
    key = lambda cells: (cells * [1, GRID, GRID * GRID]).sum(axis=1)
    k2 = key(c[second])
    order = np.argsort(k2, kind="stable")
    want = key(c[first] + off)
    at = np.minimum(np.searchsorted(k2[order], want), k2.shape[0] - 1)
    hit = np.flatnonzero(k2[order][at] == want)
    if hit.size == 0:
        raise RuntimeError(f"no pair of directions across a {where}")
    return e[first[hit[0]]], e[second[order[at[hit[0]]]]]


def _layers(rng, e0, n_near, n_far):
    """Two depth layers around one direction, all inside its cell: near points at 5, far points at 10."""
    dirs = e0 + rng.uniform(-HALF_WIDTH, HALF_WIDTH, (n_near + n_far, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dist = np.concatenate([5.0 + 0.01 * rng.standard_normal(n_near), 10.0 + 0.01 * rng.standard_normal(n_far)])
    return dirs * dist[:, None]


# The records of a cell keep their input order (the sort is stable), and at the start t = 0 a far point's first violated record is
# the first near point it meets (g = U_j - c u_i < 0 for a nearer point in almost the same direction).  So the position of the
# crowded cell's first near point IS the position of the first re-solve: placed on either side of the 64-record turns of
# kh_local's walk.  Default: the last quarter of the cell, or position 64 where that would come earlier in a cell of more than 64.
FIRST_NEAR = {(WAVE, "own"): WAVE - 1, (WAVE, "face"): WAVE - 1, (WAVE + 1, "own"): WAVE, (WAVE + 1, "face"): WAVE - 1,
              (WAVE + 1, "edge"): WAVE, (2 * WAVE, "own"): 2 * WAVE - 1, (2 * WAVE, "face"): WAVE + 1, (2 * WAVE, "edge"): WAVE,
              (2 * WAVE, "corner"): 2 * WAVE - 1, (2 * WAVE + 1, "own"): 2 * WAVE, (2 * WAVE + 1, "face"): WAVE + 1,
              (2 * WAVE + 1, "edge"): 2 * WAVE - 1, (2 * WAVE + 1, "corner"): WAVE - 1}
WHERES = ("own",) + tuple(RING_OFFSETS)


def first_near(P, where):
    x = P - P // 4
    return FIRST_NEAR.get((P, where), x if x >= WAVE or P <= WAVE else WAVE)


@functools.lru_cache(maxsize=None)
def cell_case(P, where):
    """P points in one direction cell, in two depth layers: far points, then from position `first_near` on the near points that
    hide them.  ``own``: nothing else.  Ring: six far points in the cell on the other side of a face, an edge or a corner, whose
    waves hold the crowded cell in a lane s >= 1 behind their own cell's records."""
    e0, e1 = centred_directions(where)
    rng = np.random.default_rng([82, P, WHERES.index(where)])
    x = first_near(P, where)
    near, far = _layers(rng, e1, P - x, 0), _layers(rng, e1, 0, x)
    p = np.concatenate(([] if where == "own" else [_layers(rng, e0, 0, QUERY_CELL_POINTS)]) + [far, near])
    key = lambda e: int((_cell_coords(e)[0] * [1, GRID, GRID * GRID]).sum())
    return Case(f"cell_{P}_{where}", p, HPR_RADIUS, dict(P=P, where=where, first_near=x, crowded=key(e1), query=key(e0),
                                                         lane=hpr_ref._OFFSETS.index(RING_OFFSETS.get(where, (0, 0, 0)))))


def cell_positions(c, lane):
    """The positions inside the cell held by ``lane`` at which a local re-solve of the fixture falls, over all its points."""
    out = set()
    for tr in c.walked["local"]:
        out |= {j for _, s, j in tr or () if s == lane}
    return out


# ---- shells: every point visible
SHELL_NS = (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1, 4 * BLOCK + 1)


@functools.lru_cache(maxsize=None)
def shell_case(n, hidden=False):
    """n directions spread evenly over the sphere (a spiral, jittered by a tenth of their spacing) at distance 5 +- 1 %: every
    point is visible, the global pass has n survivors.  ``hidden``: one more point straight behind another one (twice as far in
    the same direction, bit for bit), in the middle of the index: m = n + 1, the count stays n."""
    rng = np.random.default_rng([83, n])
    i = np.arange(n) + 0.5
    z, phi = 1.0 - 2.0 * i / n, i * (np.pi * (3.0 - np.sqrt(5.0)))
    d = np.stack([np.sqrt(1.0 - z * z) * np.cos(phi), np.sqrt(1.0 - z * z) * np.sin(phi), z], 1)
    d += rng.normal(0.0, 0.1 * np.sqrt(4.0 * np.pi / n) / np.sqrt(3.0), d.shape)
    d /= np.linalg.norm(d, axis=1)[:, None]
    p = (d * (5.0 * rng.uniform(0.99, 1.01, (n, 1))))[rng.permutation(n)]
    claims = dict(n=n)
    if hidden:
        at, front = n // 2, int(rng.integers(0, n // 2))
        p = np.concatenate([p[:at], 2.0 * p[front:front + 1], p[at:]])
        claims.update(hidden=at, front=front)
    return Case(f"shell_{n}" + ("_plus_hidden" if hidden else ""), p, HPR_RADIUS, claims)


# ---- tile tails of the global pass
TAILS = (0, 1, 2, 3, STEP, STEP + 1)


def build_tail_case(r, seed):
    """m = 2 * HP_TILE + r points in two depth layers, in the manner of `test_hpr_ref.two_layers`: a near grid that hides part of
    a wider far layer, under a seeded rotation (which decides the order of the sorted records)."""
    m = 2 * TILE + r
    rng = np.random.default_rng([84, r, seed])
    side = 13
    g = np.linspace(-0.3, 0.3, side)
    near = np.array([(x, y, 5.0) for x in g for y in g]) + 0.001 * rng.standard_normal((side * side, 3))
    far = np.concatenate([rng.uniform(-0.8, 0.8, (m - side * side, 2)), 10.0 + 0.01 * rng.standard_normal((m - side * side, 1))], 1)
    q, _ = np.linalg.qr(rng.standard_normal((3, 3)))
    p = np.concatenate([near, far])[rng.permutation(m)] @ q.T
    return Case(f"tail_{r}", p, HPR_RADIUS, dict(m=m, r=r, seed=seed))


def tail_case_holds(c):
    m, r = c.claims["m"], c.claims["r"]
    last_tile = (m - 1) // TILE * TILE
    hit = [k for tr in c.walked["glob"] if tr for k in tr]
    return any(k >= last_tile for k in hit) and (r % STEP == 0 or (m - 1) in hit)


# ---- the committed seeds, and the search that found them
SEEDS = {"tail_0": 0, "tail_1": 15, "tail_2": 1, "tail_3": 1, "tail_4": 5, "tail_5": 15}


def seed_search(build, holds, limit=60):
    """The first seed of 0 .. limit - 1 whose fixture shows what its name claims."""
    for seed in range(limit):
        if holds(build(seed)):
            return seed
    raise RuntimeError("no seed found")


@functools.lru_cache(maxsize=None)
def tail_case(r):
    return build_tail_case(r, SEEDS[f"tail_{r}"])


def searched():
    """name -> (build(seed), holds(case)) of every fixture whose seed was searched."""
    return {f"tail_{r}": (functools.partial(build_tail_case, r), tail_case_holds) for r in TAILS}


# ---- the skip rule where the wrong variants are unsound
SKIP_FACTORS = (2.0, 10.0)


@functools.lru_cache(maxsize=None)
def skip_regime_case(factor, n=2000):
    from test_hpr_ref import rig_subsample, shared_rig
    return Case(f"skip_regime_{factor:g}", np.ascontiguousarray(rig_subsample(shared_rig(), n=n)), factor, dict(n=n))


# ---- H6: views that are skipped, and their neighbours that are not
@functools.lru_cache(maxsize=None)
def far_cloud():
    """300 points in a box of 2 m, 50 m from the camera."""
    return np.random.default_rng(85).uniform(-1.0, 1.0, (300, 3)) + [3.0, -4.0, 50.0]


@functools.lru_cache(maxsize=None)
def h6_far_factors():
    """(skipped, kept): two radius factors three steps of the doubles apart, on either side of ``far < 2 R`` for `far_cloud`."""
    p = far_cloud()
    mn, mx = p.min(axis=0), p.max(axis=0)
    f = float(np.linalg.norm(np.maximum(np.abs(mn), np.abs(mx))) / (2.0 * np.linalg.norm(mx - mn)))
    lo = f
    for _ in range(64):
        lo = float(np.nextafter(lo, 0.0))
    while hpr_ref.prepare(p, float(np.nextafter(lo, np.inf))) is None:
        lo = float(np.nextafter(lo, np.inf))
    # lo: the largest skipped factor, one step under the first kept one
    hi = lo
    for _ in range(3):
        hi = float(np.nextafter(hi, np.inf))
    return lo, hi


def h6_cases():
    lo, hi = h6_far_factors()
    p = far_cloud()
    out = [Case("h6_far_skipped", p, lo, dict(skipped=True)), Case("h6_far_kept", p, hi, dict(skipped=False)),
           Case("h6_factor_zero", p, 0.0, dict(skipped=True)), Case("h6_factor_negative", p, -1.0, dict(skipped=True)),
           Case("h6_factor_overflows", p, 1e160, dict(skipped=True)),
           Case("h6_equal_points", np.tile(np.array([[0.3, -1.7, 2.5]]), (8, 1)), HPR_RADIUS, dict(skipped=True))]
    return {c.name: c for c in out}


def translation(t):
    T = np.eye(4)
    T[:3, 3] = t
    return T


def h6_far_views():
    """(factor, T (3, 4, 4), skipped): `far_cloud` a metre farther away, as it is, and a metre farther away again, at the kept
    factor: the sphere holds only the middle view."""
    return h6_far_factors()[1], np.stack([translation([0.0, 0.0, 1.0]), np.eye(4), translation([0.0, 0.0, 1.0])]), [True, False, True]


# ---- views of one cloud
def rigid(seed, shift):
    q, _ = np.linalg.qr(np.random.default_rng([86, seed]).standard_normal((3, 3)))
    T = np.eye(4)
    T[:3, :3], T[:3, 3] = q, shift
    return T


def order_views():
    """(cloud, T (5, 4, 4)): rigid views of `cell_129_own`'s cloud -- as it is (the crowded cell), turned, turned and moved
    away, turned and moved sideways -- and one degenerate view that sends every point to one place (skipped)."""
    flat = np.zeros((4, 4))
    flat[:, 3] = [1.0, 2.0, 3.0, 1.0]
    T = np.stack([np.eye(4), rigid(1, [0.0, 0.0, 0.0]), flat, rigid(2, [0.0, 0.0, 30.0]), rigid(3, [4.0, -3.0, 0.0])])
    return cell_case(2 * WAVE + 1, "own").points, T


# ------------------------------------------------------------------------------------------------- every fixture
def cases():
    """name -> builder of every single-view fixture."""
    out = {}
    for P in CELL_POPULATIONS:
        for where in WHERES:
            out[f"cell_{P}_{where}"] = functools.partial(cell_case, P, where)
    for n in SHELL_NS:
        out[f"shell_{n}"] = functools.partial(shell_case, n)
        out[f"shell_{n}_plus_hidden"] = functools.partial(shell_case, n, True)
    for r in TAILS:
        out[f"tail_{r}"] = functools.partial(tail_case, r)
    for f in SKIP_FACTORS:
        out[f"skip_regime_{f:g}"] = functools.partial(skip_regime_case, f)
    for name, c in h6_cases().items():
        out[name] = functools.partial(lambda c: c, c)
    return out
