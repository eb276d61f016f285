"""Seeded boundary cases for the distance predicates in front of the eigensolver, each with its truth in float64.

Every discrete decision before the cut compares a distance with a threshold: the radius graph (``d <= radius``), the TARL
pooling (``d2 < radius * radius``), the 1-NN re-projection (nearest, ties to the smaller source index) and the kNN of the
statistical outlier filter.  Random clouds never put a pair within an ulp of a threshold; the generators here do.

The rounding orders told apart:

* ``sq_plain`` -- ``((dx*dx + dy*dy) + dz*dz)``, every product and sum rounded on its own: scipy's cdist and nanoflann's
  ``L2_Adaptor`` (what open3d's KDTreeFlann runs), and what the kernels compute;
* ``sq_fused`` -- ``fma(dz, dz, fma(dy, dy, dx*dx))``: what a compiler that contracts ``a*b + c`` makes of the same line.
  Python 3.10 has no ``math.fma``, so it is restated with ``fractions.Fraction`` (``float(Fraction)`` rounds correctly).

All coordinates are generated at their final place: moving a pair changes ``p - q`` by rounding, so a pair found near the
origin is not a boundary case at 300 m.
"""
from __future__ import annotations

import math
from fractions import Fraction

import numpy as np

AFFINITY_RADIUS = 1.0      # PROXIMITY_THRESHOLD
POOL_RADIUS = 0.175        # MAJOR_VOXEL_SIZE / 2
NN1_CELL = 0.5             # ai_nn1_project's cell edge
MAP_ORIGIN = np.array([312.75, -287.5, 41.25])   # a few hundred metres from the origin, like a map's chunk centres


# --------------------------------------------------------------------------- the two orders
def sq_plain(p, q):
    """(..., 3) -> squared distance summed ``(dx*dx + dy*dy) + dz*dz``, each step rounded."""
    d = np.asarray(p, dtype=np.float64) - np.asarray(q, dtype=np.float64)
    return (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]


def _fma(a: float, b: float, c: float) -> float:
    return float(Fraction(a) * Fraction(b) + Fraction(c))


def sq_fused_one(p, q) -> float:
    dx, dy, dz = (float(p[a]) - float(q[a]) for a in range(3))
    return _fma(dz, dz, _fma(dy, dy, dx * dx))


def sq_fused(p, q):
    p = np.asarray(p, dtype=np.float64).reshape(-1, 3)
    q = np.asarray(q, dtype=np.float64).reshape(-1, 3)
    return np.array([sq_fused_one(a, b) for a, b in zip(p, q)], dtype=np.float64)


def r2_of(radius: float) -> float:
    """``radius * radius`` rounded once: the bound the pooling compares the squared distance with."""
    return float(radius) * float(radius)


def affinity_in(s, radius=AFFINITY_RADIUS):
    """The radius graph's predicate on a squared distance: ``sqrt(s) <= radius`` (ncuts_utils.py:60-61)."""
    return np.sqrt(s) <= radius


def pool_in(s, radius=POOL_RADIUS):
    """The pooling predicate on a squared distance: ``s < fl(radius * radius)`` (nanoflann's radius search)."""
    return np.asarray(s) < r2_of(radius)


# --------------------------------------------------------------------------- radius pairs
def _unit(rng, m):
    u = rng.standard_normal((m, 3))
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    keep = np.abs(u).min(axis=1) > 0.15   # general directions: three non-zero squares of different size
    return u[keep]


def anchors(count, spacing, origin, seed=0):
    """``count`` points on a square grid in the (x, y) plane with the given spacing, jittered by 10 % of it."""
    rng = np.random.default_rng(seed)
    side = int(math.ceil(math.sqrt(count)))
    ij = np.stack(np.meshgrid(np.arange(side), np.arange(side), indexing="ij"), -1).reshape(-1, 2)[:count]
    a = np.zeros((count, 3))
    a[:, :2] = ij * spacing
    a += rng.uniform(-0.1, 0.1, (count, 3)) * spacing
    return a + np.asarray(origin, dtype=np.float64)


def _near_candidates(rng, p, u, radius, m=2048, wobble=4096):
    """Points q = p + (a ux, b uy, c uz) on p's own coordinate grid (u. = the ulp of p's coordinate, so p - q is exact) near
    the direction u: a, b are u's components plus up to ``wobble`` grid steps, c is solved for ``|p - q| = radius`` and
    taken with its two neighbours.  Far from the origin the grid is coarse (2^-44 at 300 m), so ``radius * (1 + k 2^-52)``
    cannot be hit by scaling u; this lands within a few ulps of the radius in a few per cent of the tries."""
    ulp = np.maximum(np.spacing(np.abs(p)), 2.0 ** -60)
    a = np.round(radius * u[0] / ulp[0]) + rng.integers(-wobble, wobble + 1, m)
    b = np.round(radius * u[1] / ulp[1]) + rng.integers(-wobble, wobble + 1, m)
    rest = radius * radius - (a * ulp[0]) ** 2 - (b * ulp[1]) ** 2
    ok = rest > 0
    a, b = a[ok], b[ok]
    c0 = np.round(np.copysign(np.sqrt(rest[ok]), u[2]) / ulp[2])
    step = np.stack([a, b, c0], -1)
    cand = np.concatenate([step + [0, 0, dc] for dc in (-1, 0, 1)]) * ulp
    return p[None, :] + cand


def radius_pairs(kind, *, n_split, n_agree, origin=(0.0, 0.0, 0.0), spacing=4.0, seed=0):
    """``n_split + n_agree`` pairs (P[i], Q[i]), one per anchor (``anchors(..., spacing, origin)``), at ``|P - Q|`` within a
    few ulps of the radius.  The first ``n_split`` pairs are split by the two predicates of ``kind``, the rest sit as close
    to the radius but both predicates agree:

    * ``"affinity"`` (radius 1): ``affinity_in`` of the plain and of the fused square;
    * ``"pool_fused"`` (radius 0.175): ``pool_in`` of the plain and of the fused square;
    * ``"pool_sqrt"`` (radius 0.175): ``pool_in`` of the plain square and ``sqrt(plain) < radius`` (the norm test).

    Returns dict(P, Q, plain, fused, radius, kind, n_split).
    """
    radius = AFFINITY_RADIUS if kind == "affinity" else POOL_RADIUS
    rng = np.random.default_rng(seed)
    A = anchors(n_split + n_agree, spacing, origin, seed)
    r2 = r2_of(radius)

    def split_of(p, q):
        s_p = float(sq_plain(p, q))
        if kind == "affinity":
            return bool(affinity_in(s_p, radius)) != bool(affinity_in(sq_fused_one(p, q), radius))
        if kind == "pool_fused":
            return bool(pool_in(s_p, radius)) != bool(pool_in(sq_fused_one(p, q), radius))
        return bool(pool_in(s_p, radius)) != bool(math.sqrt(s_p) < radius)

    P, Q = [], []
    for i, a in enumerate(A):
        found = None
        for _ in range(400):
            u = _unit(rng, 4)
            if u.shape[0] == 0:
                continue
            p = a + rng.uniform(-0.05, 0.05, 3)
            qs = _near_candidates(rng, p, u[0], radius)
            near = np.abs(sq_plain(p[None, :], qs) - r2) <= 4 * np.spacing(r2)
            for q in qs[near][rng.permutation(int(near.sum()))[:32]]:
                if split_of(p, q) == (i < n_split):
                    found = (p, q)
                    break
            if found is not None:
                break
        if found is None:
            raise RuntimeError(f"radius_pairs({kind}): no case for anchor {i}")
        P.append(found[0])
        Q.append(found[1])
    P, Q = np.array(P), np.array(Q)
    return {"P": P, "Q": Q, "plain": sq_plain(P, Q), "fused": sq_fused(P, Q), "radius": radius, "kind": kind,
            "n_split": n_split}


# --------------------------------------------------------------------------- 1-NN near-ties
def nn1_brute(queries, sources):
    """(index, distance): the nearest source by the plain squared distance, ties to the smaller index; distance = the
    correctly rounded sqrt of that square."""
    s = sq_plain(np.asarray(queries)[:, None, :], np.asarray(sources)[None, :, :])
    idx = np.argmin(s, axis=1)            # the first minimum: the smaller index wins a tie
    return idx.astype(np.int32), np.sqrt(s[np.arange(s.shape[0]), idx])


def nn1_pair_ties(count, *, origin=MAP_ORIGIN, spacing=3.0, seed=0):
    """``count`` cases of one query and two sources whose plain squared distances to it are equal or one ulp apart, each
    case alone within ``spacing``.  Returns dict(queries (count, 3), sources (2 count, 3): the two of case i at rows
    2 i, 2 i + 1, with the nearer-by-index-rule one first in half of the cases; tie (count,) bool: exactly equal squares;
    fused_flip (count,) bool: the fused order ranks the two the other way round)."""
    rng = np.random.default_rng(seed)
    A = anchors(count, spacing, origin, seed + 1)
    queries, sources, tie, flip = [], [], [], []
    for i, a in enumerate(A):
        want_tie = i % 3 != 2
        for _ in range(10_000):
            q = a + rng.uniform(-0.2, 0.2, 3)
            v = rng.uniform(0.05, 0.3, 3) * rng.choice([-1.0, 1.0], 3)
            form = rng.integers(0, 3)
            if form == 0:
                w = -v                              # mirror image: the same squares
            elif form == 1:
                w = v[[1, 0, 2]]                    # dx, dy swapped: the same sum
            else:
                w = v[[2, 1, 0]] * [1.0, -1.0, 1.0]  # dx, dz swapped: may differ by an ulp
            a1, a2 = q + v, q + w
            s1, s2 = float(sq_plain(q, a1)), float(sq_plain(q, a2))
            if want_tie and s1 != s2:
                continue
            if not want_tie and (s1 == s2 or abs(s1 - s2) > np.spacing(max(s1, s2))):
                continue
            f1, f2 = sq_fused_one(q, a1), sq_fused_one(q, a2)
            fl = (f1 < f2) != (s1 < s2) or (f1 == f2) != (s1 == s2)
            pair = [a1, a2] if rng.random() < 0.5 else [a2, a1]
            queries.append(q)
            sources.extend(pair)
            tie.append(s1 == s2)
            flip.append(fl)
            break
        else:
            raise RuntimeError(f"nn1_pair_ties: no case for anchor {i}")
    return {"queries": np.array(queries), "sources": np.array(sources), "tie": np.array(tie), "fused_flip": np.array(flip)}


def nn1_lattice(*, origin=MAP_ORIGIN, shape=(14, 12, 6), step=NN1_CELL, hole_frac=0.35, outside=40, seed=0):
    """Sources on a ``step`` lattice (``ai_nn1_project``'s cell edge, the lattice's corner at the sources' minimum, so every
    source sits on a cell border) with ``hole_frac`` of the sites left empty; queries at cell centres, edge and face
    midpoints (8-, 2- and 4-way exact ties), at the sites themselves, and ``outside`` queries beyond the bounding box.
    Returns dict(sources, queries)."""
    rng = np.random.default_rng(seed)
    o = np.asarray(origin, dtype=np.float64)
    ijk = np.stack(np.meshgrid(*[np.arange(m) for m in shape], indexing="ij"), -1).reshape(-1, 3)
    keep = rng.random(ijk.shape[0]) >= hole_frac
    corners = np.all((ijk == 0) | (ijk == np.array(shape) - 1), axis=1)   # the bounding box stays the lattice's
    src = ijk[keep | corners].astype(np.float64)
    src = src[rng.permutation(src.shape[0])]
    half = []
    for off in ([0.5, 0.5, 0.5], [0.5, 0, 0], [0, 0.5, 0], [0, 0, 0.5], [0.5, 0.5, 0], [0, 0.5, 0.5], [0.5, 0, 0.5], [0, 0, 0]):
        base = ijk[rng.choice(ijk.shape[0], 60, replace=False)].astype(np.float64)
        half.append(np.minimum(base + off, np.array(shape) - 1))
    qs = np.concatenate(half)
    # beyond the box: up to 3 cells out on one, two or three axes, on the lattice's half-steps (ties stay exact)
    out = rng.integers(0, 2 * np.array(shape), (outside, 3)).astype(np.float64) * 0.5
    axis = rng.random((outside, 3)) < 0.5
    axis[np.arange(outside), rng.integers(0, 3, outside)] = True
    side = rng.random((outside, 3)) < 0.5
    beyond = np.where(side, -rng.integers(1, 7, (outside, 3)) * 0.5, np.array(shape) - 1 + rng.integers(1, 7, (outside, 3)) * 0.5)
    out = np.where(axis, beyond, out)
    qs = np.concatenate([qs, out])
    return {"sources": o + src * step, "queries": o + qs * step}


# --------------------------------------------------------------------------- kNN ties on the statistical filter's cells
def knn_cell(points) -> float:
    """The cell edge ``ai_statistical_inliers`` picks for this cloud (``ai_prep.hip``): the cube root of the bounding box's
    volume per point (axes thinner than 1e-3 of the widest count as that), grown by 1.5 until the (z, y) row table has at
    most 2 n + 1024 entries."""
    p = np.asarray(points, dtype=np.float64)
    n = p.shape[0]
    ext = p.max(axis=0) - p.min(axis=0)
    emax = ext.max()
    vol = 1.0
    for a in range(3):
        vol *= max(ext[a], max(1e-3 * emax, 1e-9))
    cell = float(np.cbrt(vol / n))
    while True:
        fx, fy, fz = (math.floor(e / cell) + 1 for e in ext)
        if fx < 1e9 and fy * fz <= 2.0 * n + 1024.0:
            return cell
        cell *= 1.5


def knn_lattice(*, origin=MAP_ORIGIN, side=8.0, step=0.25, cell=0.5, dup_frac=0.08, seed=0):
    """A cloud on a ``step`` lattice inside a ``side`` cube whose ``knn_cell`` is exactly ``cell`` (a multiple of ``step``):
    n = side^3 / cell^3 points, so half the lattice planes are cell borders and many points sit on them.  The eight
    corners fix the bounding box; ``dup_frac`` of the points repeat another point (distance 0, and avg == 0 for small k)."""
    rng = np.random.default_rng(seed)
    m = int(round(side / step)) + 1
    n = int(round(side ** 3 / cell ** 3))
    corners = np.array([[i, j, k] for i in (0, m - 1) for j in (0, m - 1) for k in (0, m - 1)])
    n_dup = int(dup_frac * n)
    n_site = n - 8 - n_dup
    flat = rng.choice(m ** 3, n_site, replace=False)
    sites = np.stack(np.unravel_index(flat, (m, m, m)), -1)
    base = np.concatenate([corners, sites])
    dups = base[rng.integers(8, base.shape[0], n_dup)]
    ijk = np.concatenate([base, dups])
    ijk = ijk[rng.permutation(ijk.shape[0])]
    pts = np.asarray(origin, dtype=np.float64) + ijk * step
    return pts
