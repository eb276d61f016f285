"""Fixtures, host model and high-precision reference for the affinity build (``autoinst_amd/csrc/ai_affinity.hip``).

Pure NumPy / SciPy: importable and checkable without a GPU (tests/test_affinity_cases.py); tests/test_gpu_affinity.py
feeds the device's matrices to the same `check_affinity`.

Three parts:

* `library_order` / `plan`: what the library does BEFORE it computes a weight, restated on the host -- bounds, cell
  size, cell of every point, 30-bit Morton key, stable sort, and from the reference pattern in that row order the
  tiles of `k_weights_lanes` with the branch each one takes.  Test-side only: a fixture uses it to PROVE that it sits
  on a threshold of the kernels.
* `cases()`: fixtures on those thresholds (cliques along x, neighbour-walk grids, tile tails, feature widths, SAM and
  two cameras, underflowing weights) plus one ordinary random cloud.  Every case carries `claims`: conditions on the
  plan that tests/test_affinity_cases.py asserts on the CPU.
* `reference` / `bound` / `check_affinity`: pattern by the project's float64 rule, values in ``np.longdouble``, and a
  per-entry error bound derived from the arithmetic (see `bound`), not measured on any device.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp
from scipy.spatial import cKDTree

# ---- the kernels' constants (ai_affinity.hip); a change there must be made here too, and the claims then re-proven
NB_STASH = 128            # AI_NB_STASH: hits of a row the counting walk keeps; longer rows are walked a second time
NB_LANES = 8              # AI_NB_LANES: candidates per round of the neighbour walk
ROUND = 64                # 2 * ACC: entries of a row per round of k_weights_lanes
PLANS = {16: dict(rows_per_tile=16, ecap=2048, maxd=256),     # k_weights_lanes<256, 256, 32> (the default)
         32: dict(rows_per_tile=32, ecap=4096, maxd=384)}     # k_weights_lanes<512, 384, 32> (AI_WEIGHTS_TILE=32)
HASH_SLOTS = {16: 512, 32: 1024}   # 2 * NT; no fixture here overflows the table (that needs > 2 * NT distinct columns in <= ECAP entries)

U = 2.0 ** -53            # unit roundoff of float64
TINY = 2.0 ** -1074       # spacing of the subnormals
LD = np.longdouble


# ------------------------------------------------------------------------------------------------- row order, tile plan
def _part1by2(x):
    x = x.astype(np.uint64) & np.uint64(0x3FF)
    out = np.zeros_like(x)
    for b in range(10):
        out |= ((x >> np.uint64(b)) & np.uint64(1)) << np.uint64(3 * b)
    return out


def grid_of(points, radius):
    """(min[3], inv_cell, (nx, ny, nz), cells[n, 3]) exactly as ``ai_affinity_build_sam`` and ``cell_of`` form them."""
    p = np.asarray(points, dtype=np.float64)
    mn, mx = p.min(0), p.max(0)
    cell = radius * (1.0 + 1e-9)
    inv_cell = 1.0 / cell
    dims = (np.floor((mx - mn) / cell).astype(np.int64) + 1)
    c = np.floor((p - mn) * inv_cell).astype(np.int64)
    c = np.minimum(np.maximum(c, 0), dims - 1)
    return mn, inv_cell, tuple(int(d) for d in dims), c


def morton_keys(cells):
    return _part1by2(cells[:, 0]) | (_part1by2(cells[:, 1]) << np.uint64(1)) | (_part1by2(cells[:, 2]) << np.uint64(2))


def library_order(points, radius):
    """order[p] = caller's index of library row p: Morton key of the cell (x in the lowest bit), stable."""
    _, _, _, c = grid_of(points, radius)
    return np.argsort(morton_keys(c), kind="stable")


def radius_pairs(points, radius):
    """(i, j) of every stored entry, diagonal included, sorted by (i, j): the project's predicate --
    ``sqrt((dx*dx + dy*dy) + dz*dz) <= radius`` with every operation rounded in float64."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    if n > 1:
        pr = cKDTree(p).query_pairs(radius * (1 + 1e-9) + 1e-12, output_type="ndarray")
    else:
        pr = np.zeros((0, 2), dtype=np.int64)
    i = np.concatenate([pr[:, 0], pr[:, 1], np.arange(n)]).astype(np.int64)
    j = np.concatenate([pr[:, 1], pr[:, 0], np.arange(n)]).astype(np.int64)
    d = p[i] - p[j]
    sq = d * d
    keep = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2]) <= radius
    i, j = i[keep], j[keep]
    o = np.lexsort((j, i))
    return i[o], j[o]


def plan(points, radius, rows_per_tile, ecap, maxd, pairs=None):
    """The tiles `k_weights_lanes` forms for this cloud and the branch each takes.

    Returns a dict: ``order`` (library row -> caller's index), ``pos`` (its inverse), ``rowlen`` (entries per library
    row), ``over_stash`` (per library row: more than NB_STASH entries), and per tile ``rows``, ``entries``,
    ``distinct`` (distinct columns), ``longest`` (longest row) and ``branch``: 'fallback_entries' when the tile has
    more than ``ecap`` entries, else 'fallback_distinct' when it has more than ``maxd`` distinct columns, else 'staged'."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    order = library_order(p, radius)
    pos = np.empty(n, dtype=np.int64)
    pos[order] = np.arange(n)
    i, j = radius_pairs(p, radius) if pairs is None else pairs
    pi, pj = pos[i], pos[j]
    rowlen = np.bincount(pi, minlength=n)
    ntile = (n + rows_per_tile - 1) // rows_per_tile
    tile = pi // rows_per_tile
    entries = np.bincount(tile, minlength=ntile)
    distinct = np.bincount(np.unique(tile * n + pj) // n, minlength=ntile)
    rows = np.minimum(rows_per_tile, n - np.arange(ntile) * rows_per_tile)
    longest = np.array([rowlen[t * rows_per_tile:(t + 1) * rows_per_tile].max() for t in range(ntile)])
    branch = np.where(entries > ecap, "fallback_entries", np.where(distinct > maxd, "fallback_distinct", "staged"))
    return dict(order=order, pos=pos, rowlen=rowlen, over_stash=rowlen > NB_STASH, rows=rows, entries=entries,
                distinct=distinct, longest=longest, branch=branch, rows_per_tile=rows_per_tile)


# ------------------------------------------------------------------------------------------------- reference and bound
def _ops(F):
    """Roundings a term of a squared feature distance passes through after its square: the longest of the device's
    paths.  Tiled (F % 16 == 0): a lane's chain of F / 8 fma, then a 3-level tree.  Row-wise: a chain of ceil(F / 16)
    fma, then a 4-level tree."""
    if F <= 0:
        return 0
    rowwise = -(-F // 16) + 4
    tiled = (F // 8 + 3) if F % 16 == 0 else 0
    return max(rowwise, tiled)


def _factor_err(x_abs, sq_ops):
    """Relative error of ``exp(-k * sqrt(s))``, |k sqrt(s)| = x_abs, s a sum of squares with `sq_ops` roundings."""
    eps_sq = (2 + sq_ops) * U            # difference rounded (u), squared (2 u), then the sum's roundings
    eps_arg = eps_sq / 2 + U / 2 + U     # square root, then the product with the weight
    return x_abs * eps_arg + 2 * U       # exp: argument error |x| eps, own error 1 ulp <= 2 u


@dataclass
class Reference:
    indptr: np.ndarray
    indices: np.ndarray
    data: np.ndarray          # float64: the longdouble value rounded once
    data_ld: np.ndarray       # np.longdouble
    bound: np.ndarray         # absolute bound of |device - data_ld| per entry (float64)
    rows: np.ndarray          # row of every entry


def _cams(x):
    return [] if x is None else (list(x) if isinstance(x, (list, tuple)) else [x])


def reference(points, tarl, dino, sam, alpha, beta, theta, gamma, radius):
    """Pattern by the project's float64 rule (`radius_pairs`), every stored value in ``np.longdouble``.

    ``dino`` / ``sam``: one matrix or a list with one per camera.  A falsy weight drops its factor; a pair with an
    all-zero TARL row on either side has TARL distance 0; the diagonal is exactly 1.  A weight that underflows is
    still an entry (value subnormal or 0.0), as in ``oracle.ncuts_ref.affinity_sparse``.  See `bound` for the bound."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    i, j = radius_pairs(p, radius)
    val = np.ones(i.shape[0], dtype=LD)
    rel = np.zeros(i.shape[0], dtype=np.float64)
    nfac = 0

    def fdist(F):
        F = np.asarray(F, dtype=np.float64)
        out = np.empty(i.shape[0], dtype=LD)
        blk = max(1, (1 << 22) // max(1, F.shape[1]))
        for s in range(0, i.shape[0], blk):
            d = F[i[s:s + blk]].astype(LD) - F[j[s:s + blk]].astype(LD)
            out[s:s + blk] = np.sqrt((d * d).sum(1))
        return out

    if theta:
        T = np.asarray(tarl, dtype=np.float64)
        t = fdist(T)
        no = ~T.any(1)
        t[no[i] | no[j]] = 0
        val = val * np.exp(-LD(theta) * t)
        rel += _factor_err(np.abs(theta * t.astype(np.float64)), _ops(T.shape[1]))
        nfac += 1
    if alpha:
        d = p[i].astype(LD) - p[j].astype(LD)
        dd = np.sqrt((d * d).sum(1))
        val = val * np.exp(-LD(alpha) * dd)
        # the device's distance is the float64 one of the predicate: three products, two sums (5 u with the rounded differences)
        rel += _factor_err(np.abs(alpha * dd.astype(np.float64)), 3)
        nfac += 1
    if beta:
        for S in _cams(sam):
            S = np.asarray(S)
            both = (S[i] != -1) & (S[j] != -1)
            co = both.sum(1)
            diff = (both & (S[i] != S[j])).sum(1)
            frac = np.where(co > 0, diff.astype(LD) / np.maximum(co, 1).astype(LD), LD(0))
            val = val * np.exp(-LD(beta) * frac)
            rel += np.abs(beta * frac.astype(np.float64)) * 2 * U + 2 * U   # quotient and product rounded, then exp
            nfac += 1
    if gamma:
        for D in _cams(dino):
            g = fdist(D)
            val = val * np.exp(-LD(gamma) * g)
            rel += _factor_err(np.abs(gamma * g.astype(np.float64)), _ops(np.asarray(D).shape[1]))
            nfac += 1
    rel += max(nfac - 1, 0) * U                                  # the products of the factors
    nfeat = sum(np.asarray(x).shape[1] for x in ([tarl] if theta else []) + (_cams(dino) if gamma else []))
    rel += (nfeat + 16) * 2.0 ** -64                              # this reference's own longdouble arithmetic
    diag = i == j
    val[diag] = 1
    rel[diag] = 0.0                                              # exp(-0) = 1 and 1 * 1 = 1 exactly
    absb = rel * np.abs(val).astype(np.float64) + (1 + 0.5 * max(nfac - 1, 0)) * TINY
    absb[diag] = 0.0
    indptr = np.zeros(n + 1, dtype=np.int64)
    np.cumsum(np.bincount(i, minlength=n), out=indptr[1:])
    return Reference(indptr, j.astype(np.int32), val.astype(np.float64), val, absb, i)


def bound(ref: Reference, entry=None):
    """Absolute bound on ``|device value - longdouble value|`` of an entry -- DERIVED, not measured on a device.

    u = 2^-53.  A squared feature distance over F dimensions: every difference is rounded once (u), its square is
    formed inside the fma (2 u), and the term then passes through one rounding per fma of its lane's chain and one
    per level of the reduction tree.  The longest of the device's paths (`_ops`): tiled, F / 8 fma + 3 levels;
    row-wise, ceil(F / 16) fma + 4 levels.  So the squared distance s has relative error <= (2 + chain + tree) u, its
    (correctly rounded) square root half of that plus u/2, the argument ``k * sqrt(s)`` of ``exp`` one more u, and
    ``exp`` of an argument x with relative error e has relative error <= |x| e plus its own 1 ulp <= 2 u (ROCm's
    documented accuracy of double ``exp``).  The spatial factor takes the float64 distance of the radius predicate:
    rounded differences, three products and two sums, i.e. the same expression with chain + tree = 3.  A SAM factor:
    the fraction and its product with beta are rounded (|x| 2 u), then ``exp`` (2 u).  The k factors are joined by
    k - 1 multiplications, u each; one more camera (``ai_affinity_apply_camera``) adds its factors and their
    multiplications in the same way.  The reference's own longdouble error is (F_total + 16) 2^-64.  The sum is a
    relative bound; times |value|, plus one subnormal spacing for ``exp`` and half of one per multiplication, it is
    the absolute bound returned here, which is what is compared when a weight underflows.  The diagonal is exact.

    One expression serves every path, so `check_affinity` does not need to know which branch computed an entry.  At
    F = 96 and theta * t = 5 it is about 5e-15 relative."""
    return ref.bound if entry is None else ref.bound[entry]


# ------------------------------------------------------------------------------------------------- cases
@dataclass
class Case:
    name: str
    points: np.ndarray
    tarl: np.ndarray | None = None
    dino: object = None        # matrix, or list of one matrix per camera
    sam: object = None
    alpha: float = 1.0
    beta: float = 0.0
    theta: float = 0.0
    gamma: float = 0.0
    radius: float = 1.0
    claims: list = field(default_factory=list)   # (threshold, side, plan rows or None): see `claim_holds`
    sizes: list | None = None                    # clique sizes in x order, for the clique cases
    note: str = ""
    _ref: Reference | None = None
    _plans: dict = field(default_factory=dict)
    _pairs: tuple | None = None

    @property
    def n(self):
        return self.points.shape[0]

    def kw(self):
        return dict(alpha=self.alpha, theta=self.theta, gamma=self.gamma, radius=self.radius, beta=self.beta)

    def pairs(self):
        if self._pairs is None:
            self._pairs = radius_pairs(self.points, self.radius)
        return self._pairs

    def ref(self) -> Reference:
        if self._ref is None:
            self._ref = reference(self.points, self.tarl, self.dino, self.sam, self.alpha, self.beta, self.theta,
                                  self.gamma, self.radius)
        return self._ref

    def plan(self, rows):
        if rows not in self._plans:
            self._plans[rows] = plan(self.points, self.radius, pairs=self.pairs(), **PLANS[rows])
        return self._plans[rows]

    def tiled(self):
        """Whether the default build sends this case through `k_weights_lanes` (else: wave per row)."""
        t, d = (self.tarl if self.theta else None), (self.dino if self.gamma else None)
        if isinstance(d, (list, tuple)):
            d = d[0]
        return (t is not None or d is not None) and not self.beta and all(f is None or f.shape[1] % 16 == 0 for f in (t, d))


def _grid_jitter(rng, m, steps=16):
    """m offsets on the 2^-10 grid, |component| <= steps * 2^-10: translations by multiples of 2^-10 stay exact."""
    return rng.integers(-steps, steps + 1, (m, 3)).astype(np.float64) * 2.0 ** -10


def clique_points(sizes, rng, spacing=2.0):
    """Clusters of sizes[k] points inside a ball of diameter << 1 at x = 0.5 + spacing * k: each in its own cell, in x
    order = Morton order (ny = nz = 1), so cluster k is contiguous in library order and all its rows have sizes[k] entries."""
    pts = []
    for k, m in enumerate(sizes):
        pts.append(np.array([0.5 + spacing * k, 0.0, 0.0]) + _grid_jitter(rng, m))
    pts = np.concatenate(pts)
    pts[0] = [0.25, -0.25, -0.25]   # the grid's origin: every cluster then sits a quarter cell inside its own cell
    return pts


def _features(rng, n, tdim, ddim, zero_every=9):
    tarl = rng.normal(0, 0.4, (n, tdim)) if tdim else None
    if tarl is not None and zero_every:
        tarl[3::zero_every] = 0.0          # all-zero rows inside and across clusters
    dino = rng.normal(0, 0.3, (n, ddim)) if ddim else None
    return tarl, dino


# 16-row plan.  Rows (library order): 8 | 128 | 128 | 129 | 1 | 120 | 12 | 125 | 3 | 2 | 127 | 1 | 63 | 1 | 64 | 15 | 65 | 15
#   tile 8 = last 8 rows of the first 128-clique + first 8 of the second: 2048 entries, 256 columns -> staged (both limits met exactly)
#   tiles 1..7, 9..15 = 16 rows of a 128-clique: exactly ECAP entries -> staged
#   tile 16 = 8 rows of 128 + 8 of 129: 2056 entries; tiles 17..23: 2064 -> fallback_entries; their mirrors in tile 24 are staged
#   tile 32 = last 2 rows of the 120-clique, the 12-clique, first 2 rows of the 125-clique: 634 entries, 257 columns -> fallback_distinct
SIZES16 = [8, 128, 128, 129, 1, 120, 12, 125, 3, 2, 127, 1, 63, 1, 64, 15, 65, 15]
# 32-row plan.  16 | 177 | 30 | 177 : tile 6 = last row of the first 177-clique, the 30-clique, first row of the second: 384 columns
#   ... | 31 | 178 | 30 | 177 : the same with 385 columns; | 16 | 128 | 128 | 129 | 31 ...: 32 rows of a 128-clique = 4096 entries,
#   32 rows of the 129-clique = 4128, its last row shares a (staged) tile with the 31-clique
SIZES32 = [16, 177, 30, 177, 31, 178, 30, 177, 16, 128, 128, 129, 31, 127, 1, 63, 1, 64, 31, 65, 2]


def _clique_case(name, sizes, tdim, ddim, seed, claims):
    rng = np.random.default_rng(seed)
    pts = clique_points(sizes, rng)
    tarl, dino = _features(rng, pts.shape[0], tdim, ddim)
    return Case(name, pts, tarl, dino, theta=0.5, gamma=0.1 if ddim else 0.0, claims=claims, sizes=list(sizes))


def walk_points(rng, ny, nz, flat_x=False):
    """Cells along x holding 5 | k | 5 points for k = 0, 1, 7, 8, 9, 16, 17, twice, the second time one cell further so that
    every populated home cell occurs with odd and with even cx; one such line per (cy, cz), rotated by cy + cz.  Points on
    the 2^-10 grid, never on a cell's lower face, and one point at the origin so that cell (i, j, k) is [i, i + 1) x ..."""
    seq = [5, 0, 5, 1, 5, 7, 5, 8, 5, 9, 5, 16, 5, 17, 5]
    line = seq + [0, 0] + seq
    pts = [np.zeros((1, 3))]
    for cy in range(ny):
        for cz in range(nz):
            cnt = np.roll(line, 2 * (cy + cz)) if not flat_x else [17, 8, 9][(cy + cz) % 3:][:1]
            for cx, k in enumerate(cnt):
                if k:
                    off = rng.integers(1, 1024, (k, 3)).astype(np.float64) * 2.0 ** -10
                    if ny == 1:
                        off[:, 1] *= 2.0 ** -4
                    if nz == 1:
                        off[:, 2] *= 2.0 ** -4
                    pts.append(np.array([cx, cy, cz], dtype=np.float64) + off)
    return np.concatenate(pts)


def random_mixed(rng):
    """The cloud of test_feature_factors_tiled_and_fallback_tiles_in_one_graph at a third of its size: sheet, blob, mid."""
    sheet = np.c_[rng.uniform(-7, 7, (1700, 2)), rng.normal(0, 0.05, 1700)]
    blob = rng.normal(0, 0.35, (500, 3)) + np.array([2.0, -3.0, 0.0])
    mid = rng.normal(0, 0.8, (500, 3)) + np.array([-5.0, 4.0, 0.0])
    return np.concatenate([sheet, blob, mid])


MAP_SHIFT = np.array([4e5, 5e6, 2e2])
TAIL_N = [1, 2, 15, 16, 17, 31, 32, 33, 1025, 1023]
WIDTHS = [(1, 7), (7, 16), (16, 96), (96, 384), (100, 112), (112, 400), (384, 1), (400, 100), (96, 0), (0, 384)]
_CASES = None


def cases():
    """Every fixture, built once per process.  Which fixture carries which threshold is its `claims`."""
    global _CASES
    if _CASES is not None:
        return _CASES
    out = []
    both = ("below", "at", "above")
    c16 = [("stash", s, None) for s in both] + [("tile_entries", s, 16) for s in ("at", "above")] + \
          [("distinct", s, 16) for s in ("at", "above")] + [("longest", L, 16) for L in (63, 64, 65, 128, 129)] + \
          [("mirror", "staged_vs_fallback", 16)]
    out.append(_clique_case("cliques16", SIZES16, 96, 384, 1, c16))
    c32 = [("stash", s, None) for s in both] + [("tile_entries", s, 32) for s in ("at", "above")] + \
          [("distinct", s, 32) for s in ("at", "above")] + [("longest", L, 32) for L in (63, 64, 65, 128, 129)] + \
          [("mirror", "staged_vs_fallback", 32)]
    out.append(_clique_case("cliques32", SIZES32, 32, 48, 2, c32))
    # a graph in which NO row is over the stash: the second walk is not launched at all
    out.append(_clique_case("cliques_no_row_over", [8, 128, 127, 64, 3], 16, 0, 3, [("stash", "none_over", None)]))

    rng = np.random.default_rng(4)
    for name, ny, nz in (("walk_line", 1, 1), ("walk_sheet", 3, 1), ("walk_3d", 3, 3)):
        p = walk_points(rng, ny, nz)
        t, d = _features(rng, p.shape[0], 16, 32)
        out.append(Case(name, p, t, d, theta=0.5, gamma=0.1, claims=[("walk", (ny, nz), None)]))
    p = walk_points(rng, 4, 3, flat_x=True)
    p[:, 0] *= 0.5                                  # x extent below one cell
    t, d = _features(rng, p.shape[0], 16, 0)
    out.append(Case("walk_nx1", p, t, None, theta=0.5, claims=[("grid", "nx1", None)]))
    base = out[5]                                   # walk_3d
    out.append(Case("walk_3d_negative", base.points - np.array([3000.0, 2000.0, 100.0]), base.tarl, base.dino, theta=0.5, gamma=0.1,
                    claims=[("translated", "walk_3d", None), ("grid", "negative", None)]))
    out.append(Case("walk_3d_map", base.points + MAP_SHIFT, base.tarl, base.dino, theta=0.5, gamma=0.1,
                    claims=[("translated", "walk_3d", None)]))

    for n in TAIL_N:
        rng = np.random.default_rng(100 + n)
        p = rng.normal(0, 1.2 if n > 100 else 0.6, (n, 3))
        t, d = _features(rng, n, 16, 32, zero_every=5)
        out.append(Case(f"tail_{n}", p, t, d, theta=0.5, gamma=0.1, claims=[("tail", n, None)]))

    rng = np.random.default_rng(7)
    wp = np.concatenate([rng.normal(0, 1.5, (400, 3)), clique_points([129, 65], rng) + np.array([8.0, 0, 0])])
    for tdim, ddim in WIDTHS:
        rng = np.random.default_rng(1000 + 7 * tdim + ddim)
        t, d = _features(rng, wp.shape[0], tdim, ddim)
        if tdim and tdim < 96:
            t *= np.sqrt(96.0 / tdim)               # a distance like the 96-d one, so that theta * t stays of order 3
        out.append(Case(f"width_{tdim}_{ddim}", wp, t, d, theta=0.5 if tdim else 0.0, gamma=0.1 if ddim else 0.0,
                        claims=[("width", (tdim, ddim), None)]))
    rng = np.random.default_rng(8)
    t, d = _features(rng, wp.shape[0], 96, 384)
    out.append(Case("theta0_with_features", wp, t, d, theta=0.0, gamma=0.1, claims=[("weight0", "theta", None)]))
    out.append(Case("alpha0", wp, t, d, alpha=0.0, theta=0.5, gamma=0.1, claims=[("weight0", "alpha", None)]))

    # SAM ids and a second camera (wave-per-row kernel + ai_affinity_apply_camera)
    sam1 = rng.integers(-1, 4, (wp.shape[0], 3)).astype(np.int32)
    sam2 = rng.integers(-1, 3, (wp.shape[0], 2)).astype(np.int32)
    out.append(Case("sam_one_camera", wp, t, d, sam=sam1, beta=0.7, theta=0.5, gamma=0.1, claims=[("sam", 1, None)]))
    for name, w2 in (("two_cameras_384", 384), ("two_cameras_100", 100)):
        d2 = rng.normal(0, 0.3, (wp.shape[0], w2))
        out.append(Case(name, wp, t, [d, d2], sam=[sam1, sam2], beta=0.7, theta=0.5, gamma=0.1, claims=[("sam", 2, None)]))

    # weights at the end of the range: TARL distances that make exp return a subnormal (theta t = 720) and 0.0 (theta t = 800)
    rng = np.random.default_rng(9)
    up = clique_points([6, 4], rng)
    ut = rng.normal(0, 0.01, (10, 16))
    ut[1, 0] += 1440.0
    ut[2, 0] -= 1600.0
    ut[4] = 0.0
    out.append(Case("underflow", up, ut, None, theta=0.5, claims=[("underflow", "subnormal_and_zero", None)],
                    note="rows 0-5 are one clique: (0, 1) underflows to a subnormal, (0, 2) and (1, 2) to 0.0; the entries stay"))

    # pairs exactly AT the radius (kept: the predicate is <=), one ulp inside and one ulp outside
    rng = np.random.default_rng(11)
    ap = np.array([[0, 0, 0], [1, 0, 0], [0, 0, 1], [0.5, 0, 0], [0, np.nextafter(1.0, 2.0), 0], [0, -np.nextafter(1.0, 0.0), 0], [0.6, 0.8, 0]])
    t, _ = _features(rng, ap.shape[0], 16, 0, zero_every=0)
    out.append(Case("at_radius", ap, t, None, theta=0.5, claims=[("radius", "exact", None)]))

    rng = np.random.default_rng(10)
    p = random_mixed(rng)
    t, d = _features(rng, p.shape[0], 32, 48)
    out.append(Case("random_mixed", p, t, d, theta=0.5, gamma=0.1, claims=[("ordinary", "three_regimes", None)]))
    _CASES = out
    return out


def case(name):
    return next(c for c in cases() if c.name == name)


# ------------------------------------------------------------------------------------------------- claims
def _tiles(c, rows):
    return c.plan(rows)


def claim_holds(c: Case, claim):
    """True when the fixture really sits where it says -- a condition on the host plan, not a measurement."""
    what, side, rows = claim
    if what == "stash":
        L = c.plan(16)["rowlen"]
        return {"below": (L == NB_STASH - 1).any(), "at": (L == NB_STASH).any(), "above": (L == NB_STASH + 1).any(),
                "none_over": (L == NB_STASH).any() and not (L > NB_STASH).any()}[side]
    if what == "tile_entries":
        P, ecap = c.plan(rows), PLANS[rows]["ecap"]
        if side == "at":
            return ((P["entries"] == ecap) & (P["branch"] == "staged")).any()
        return ((P["entries"] > ecap) & (P["entries"] <= ecap + 2 * rows) & (P["branch"] == "fallback_entries")).any()
    if what == "distinct":
        P, maxd = c.plan(rows), PLANS[rows]["maxd"]
        ok = P["entries"] <= PLANS[rows]["ecap"]
        if side == "at":
            return ((P["distinct"] == maxd) & ok & (P["branch"] == "staged")).any()
        return ((P["distinct"] == maxd + 1) & ok & (P["branch"] == "fallback_distinct")).any()
    if what == "longest":
        P = c.plan(rows)
        return ((P["longest"] == side) & (P["branch"] == "staged")).any()
    if what == "mirror":
        return mirror_pairs(c, rows)[0].size > 0
    if what == "walk":
        _, _, dims, cells = grid_of(c.points, c.radius)
        if (dims[1] > 1) != (side[0] > 1) or (dims[2] > 1) != (side[1] > 1):
            return False
        occ = np.zeros(dims, dtype=np.int64)
        np.add.at(occ, tuple(cells.T), 1)
        occp = np.pad(occ, ((1, 1), (0, 0), (0, 0)), constant_values=-1)
        for k in (0, 1, 7, 8, 9, 16, 17):
            for parity in (0, 1):   # a populated home cell of this parity with a cell of k points at cx + 1 and one at cx - 1
                home = (occ > 0) & ((np.arange(dims[0]) % 2 == parity)[:, None, None])
                if not ((home & (occp[2:] == k)).any() and (home & (occp[:-2] == k)).any()):
                    return False
        return occ[0].any() and occ[-1].any()
    if what == "grid":
        _, _, dims, _ = grid_of(c.points, c.radius)
        return {"nx1": dims[0] == 1 and dims[1] > 1 and dims[2] > 1, "negative": bool((c.points < 0).all())}[side]
    if what == "translated":
        b = case(side)
        bi, bj = b.pairs()
        ci, cj = c.pairs()
        d = c.points - b.points
        return np.array_equal(bi, ci) and np.array_equal(bj, cj) and (d == d[0]).all() and \
            np.array_equal(library_order(b.points, b.radius), library_order(c.points, c.radius))
    if what == "tail":
        return c.n == side and c.tiled()
    if what == "width":
        t = c.tarl.shape[1] if c.tarl is not None else 0
        d = c.dino.shape[1] if c.dino is not None else 0
        return (t, d) == side and (c.plan(16)["rowlen"] > NB_STASH).any()
    if what == "weight0":
        return (c.theta == 0.0 and c.tarl is not None) if side == "theta" else c.alpha == 0.0
    if what == "sam":
        return c.beta != 0 and len(_cams(c.sam)) == side and len(_cams(c.dino)) == side
    if what == "underflow":
        v = c.ref().data
        return ((v > 0) & (v < 2.0 ** -1022)).any() and (v == 0.0).any()
    if what == "radius":
        i, j = c.pairs()
        d = c.points[i] - c.points[j]
        dist = np.sqrt((d[:, 0] * d[:, 0] + d[:, 1] * d[:, 1]) + d[:, 2] * d[:, 2])
        return (dist == c.radius).sum() >= 4 and (dist == np.nextafter(c.radius, 0.0)).any()
    if what == "ordinary":
        L = c.plan(16)["rowlen"]
        br = set(c.plan(16)["branch"])
        return L.max() > 129 and (L < 40).sum() > 500 and br >= {"staged", "fallback_entries"}
    raise KeyError(what)


def mirror_pairs(c: Case, rows):
    """Entries (i, j) computed by a staged tile whose mirror (j, i) is computed by a fallback tile: positions into the
    reference's (= the exported matrix's) data array, as (staged entries, their mirrors)."""
    P, r = c.plan(rows), c.ref()
    staged = P["branch"][P["pos"][r.rows] // rows] == "staged"
    n = c.n
    key = r.rows * n + r.indices
    mkey = r.indices.astype(np.int64) * n + r.rows
    mpos = np.searchsorted(key, mkey)            # symmetric pattern: every mirror exists
    sel = staged & ~staged[mpos] & (r.rows != r.indices)
    return np.nonzero(sel)[0], mpos[sel]


# ------------------------------------------------------------------------------------------------- the check
def _where(c: Case, e):
    r = c.ref()
    i, j = int(r.rows[e]), int(r.indices[e])
    s = f"row {i} column {j}"
    for rows in (16, 32):
        P = c.plan(rows)
        t = int(P["pos"][i] // rows)
        s += f", tile{rows} {t} ({P['branch'][t]})"
    return s + f", row length {int(c.plan(16)['rowlen'][c.plan(16)['pos'][i]])}"


def check_affinity(c: Case, A, label="", extra_rel=0.0):
    """The one check of a device (or model) matrix ``A`` (CSR, caller's row order, sorted columns) against the reference:
    pattern equal, every value within `bound` of the longdouble value, ``A == A.T`` bit for bit, unit diagonal.
    Raises AssertionError naming the first offending (row, column, tile, predicted branch); returns the largest
    error / bound ratio overall and per predicted branch of the 16- and 32-row plans.  ``extra_rel``: relative widening
    for arithmetic the caller has added and derived (none of this module's own callers passes it)."""
    r = c.ref()
    A = sp.csr_matrix(A)
    tag = f"[{c.name}{' ' + label if label else ''}] "
    ip = np.asarray(A.indptr, dtype=np.int64)
    if not np.array_equal(ip, r.indptr) or not np.array_equal(A.indices, r.indices):
        bad = np.nonzero(np.diff(ip) != np.diff(r.indptr))[0] if ip.shape == r.indptr.shape else np.array([0])
        if bad.size == 0:
            e = int(np.nonzero(A.indices != r.indices)[0][0])
            raise AssertionError(tag + f"pattern differs: device column {int(A.indices[e])} at {_where(c, e)}")
        i = int(bad[0])
        got, want = set(A.indices[ip[i]:ip[i + 1]].tolist()), set(r.indices[r.indptr[i]:r.indptr[i + 1]].tolist())
        e = int(r.indptr[i]) if i < c.n and r.indptr[i] < r.indices.size else 0
        raise AssertionError(tag + f"pattern differs: row {i} has {len(got)} entries for {len(want)}, missing {sorted(want - got)[:4]} "
                             f"extra {sorted(got - want)[:4]}; first entry of the row at {_where(c, e)}")
    data = np.asarray(A.data, dtype=np.float64)
    err = np.abs(data.astype(LD) - r.data_ld).astype(np.float64)
    bnd = r.bound + extra_rel * np.abs(r.data)
    bad = np.nonzero(~(err <= bnd))[0]
    if bad.size:
        e = int(bad[0])
        raise AssertionError(tag + f"value {data[e]!r} for {r.data[e]!r}: error {err[e]:.3e} > bound {bnd[e]:.3e} "
                             f"({err[e] / max(bnd[e], TINY):.2f} x) at {_where(c, e)}; {bad.size} entries over")
    diag = r.rows == r.indices
    if not np.all(data[diag] == 1.0):
        e = int(np.nonzero(diag & (data != 1.0))[0][0])
        raise AssertionError(tag + f"diagonal {data[e]!r} != 1 at {_where(c, e)}")
    n = c.n
    mpos = np.searchsorted(r.rows * n + r.indices, r.indices.astype(np.int64) * n + r.rows)
    asym = np.nonzero(data.view(np.int64) != data[mpos].view(np.int64))[0]
    if asym.size:
        e = int(asym[0])
        raise AssertionError(tag + f"not symmetric bit for bit: {data[e]!r} vs mirror {data[mpos[e]]!r} at {_where(c, e)}; mirror at {_where(c, int(mpos[e]))}")
    ratio = np.where(bnd > 0, err / np.where(bnd > 0, bnd, 1.0), 0.0)
    out = {"max_ratio": float(ratio.max()) if ratio.size else 0.0}
    for rows in (16, 32):
        P = c.plan(rows)
        br = P["branch"][P["pos"][r.rows] // rows]
        for b in ("staged", "fallback_entries", "fallback_distinct"):
            m = br == b
            if m.any():
                out[f"tile{rows}_{b}"] = float(ratio[m].max())
    return out


# ------------------------------------------------------------------------------------------------- float64 model, mutants
def _sq_tree(a, b):
    """aw_sqdist_tree's order in float64 (products rounded on their own: NumPy has no fma): lane m owns dimensions
    16 s + 2 m, 16 s + 2 m + 1 over the slabs, the 8 partials are added as a balanced tree."""
    d = a - b
    sq = (d * d).reshape(d.shape[0], -1, 8, 2)
    p = np.zeros((d.shape[0], 8))
    for s in range(sq.shape[1]):
        p = (p + sq[:, s, :, 0]) + sq[:, s, :, 1]
    return ((p[:, 0] + p[:, 1]) + (p[:, 2] + p[:, 3])) + ((p[:, 4] + p[:, 5]) + (p[:, 6] + p[:, 7]))


def _sq_lanes16(a, b):
    """sqdist16's order: lane t owns dimensions t, t + 16, ... (ragged last stride), then ai_group16_sum's xor tree."""
    d = a - b
    F = d.shape[1]
    pad = (-F) % 16
    sq = np.pad(d * d, ((0, 0), (0, pad))).reshape(d.shape[0], -1, 16)
    p = np.zeros((d.shape[0], 16))
    for s in range(sq.shape[1]):
        p = p + sq[:, s]
    for o in (8, 4, 2, 1):
        p = p + p[:, np.arange(16) ^ o]
    return p[:, 0]


def model_affinity(c: Case, order="auto", *, drop_last_dim=False, zero_rule="both", strict_radius=False):
    """Plain float64 NumPy restatement of the device's arithmetic (`order`: 'tree' = tiled kernels, 'lanes16' = wave per
    row, 'auto' = what the default build picks), or a deliberately wrong one: the keyword arguments are the mutants."""
    p = np.asarray(c.points, dtype=np.float64)
    i, j = c.pairs()
    dv = p[i] - p[j]
    sq = dv * dv
    dist = np.sqrt((sq[:, 0] + sq[:, 1]) + sq[:, 2])
    if strict_radius:
        keep = (dist < c.radius) | (i == j)
        i, j, dist = i[keep], j[keep], dist[keep]
    if order == "auto":
        order = "tree" if c.tiled() else "lanes16"

    def sqd(F):
        F = np.asarray(F, dtype=np.float64)
        if drop_last_dim:
            F = np.concatenate([F[:, :-1], np.zeros((F.shape[0], 1))], axis=1)
        out = np.empty(i.shape[0])
        blk = max(1, (1 << 22) // F.shape[1])
        for s in range(0, i.shape[0], blk):
            a, b = F[i[s:s + blk]], F[j[s:s + blk]]
            out[s:s + blk] = _sq_tree(a, b) if (order == "tree" and F.shape[1] % 16 == 0) else _sq_lanes16(a, b)
        return out

    w = np.ones(i.shape[0])
    if c.theta:
        t2 = sqd(c.tarl)
        no = ~np.asarray(c.tarl).any(1)
        t2[(no[i] | no[j]) if zero_rule == "both" else no[i]] = 0.0
        w = np.exp(-c.theta * np.sqrt(t2))
    if c.alpha:
        w = w * np.exp(-c.alpha * dist)
    sams, dinos = (_cams(c.sam) if c.beta else []), (_cams(c.dino) if c.gamma else [])
    for k in range(max(len(sams), len(dinos))):          # camera by camera, as ai_affinity_apply_camera does
        if k < len(sams):
            S = np.asarray(sams[k])
            both = (S[i] != -1) & (S[j] != -1)
            co = both.sum(1)
            diff = (both & (S[i] != S[j])).sum(1).astype(np.float64)
            w = w * np.exp(-c.beta * np.where(co > 0, diff / np.maximum(co, 1), 0.0))
        if k < len(dinos):
            w = w * np.exp(-c.gamma * np.sqrt(sqd(dinos[k])))
    return sp.csr_matrix((w, (i, j)), shape=(c.n, c.n))
