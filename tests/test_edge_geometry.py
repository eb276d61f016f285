"""CPU: the boundary fixtures of tests/edge_geometry.py tell the rounding orders apart, and the oracles state the chosen
rules on them (radius graph: cdist's ``d <= 1``; pooling: the plain square ``< fl(r * r)``; 1-NN: the smallest plain
square, ties to the smaller index).  tests/test_gpu_edges.py runs the same fixtures through the kernels."""
import math

import numpy as np
import pytest
from scipy.spatial.distance import cdist

import edge_geometry as eg
import prep_ref
from oracle import ncuts_ref, points_ref

ORIGINS = {"near": (25.0, -18.0, 1.0), "map": tuple(eg.MAP_ORIGIN)}


def _pair_cdist(P, Q):
    return np.array([cdist(p[None], q[None])[0, 0] for p, q in zip(P, Q)])


@pytest.fixture(scope="module", params=sorted(ORIGINS))
def affinity_pairs(request):
    return eg.radius_pairs("affinity", n_split=120, n_agree=40, origin=ORIGINS[request.param], seed=1)


def test_plain_order_is_cdist_and_fused_is_exact(affinity_pairs):
    P, Q = affinity_pairs["P"], affinity_pairs["Q"]
    assert np.array_equal(_pair_cdist(P, Q), np.sqrt(affinity_pairs["plain"]))   # bit for bit
    for p, q, s in zip(P[:20], Q[:20], affinity_pairs["fused"][:20]):
        dx, dy, dz = (float(p[a]) - float(q[a]) for a in range(3))
        t = eg._fma(dy, dy, dx * dx)
        assert s == eg._fma(dz, dz, t)
        # a fused step is the exact value rounded once: the neighbouring doubles are further from it
        exact = eg.Fraction(dz) ** 2 + eg.Fraction(t)
        assert all(abs(exact - eg.Fraction(s)) <= abs(exact - eg.Fraction(v)) for v in (np.nextafter(s, 0), np.nextafter(s, 9)))


def test_affinity_pairs_split_the_orders(affinity_pairs):
    c = affinity_pairs
    split = eg.affinity_in(c["plain"]) != eg.affinity_in(c["fused"])
    assert split[:c["n_split"]].all() and not split[c["n_split"]:].any()
    assert split.sum() >= 100
    d = np.sqrt(c["plain"])
    assert np.all(np.abs(d - 1.0) <= 4 * 2.0 ** -52)                      # every pair is at the radius to a few ulps
    inside = eg.affinity_in(c["plain"])
    assert 0 < inside[split].sum() < split.sum()                            # the fused order errs both ways
    assert 0 < inside[~split].sum() < (~split).sum()


def test_pool_pairs_split_the_orders():
    for origin in ORIGINS.values():
        f = eg.radius_pairs("pool_fused", n_split=100, n_agree=20, origin=origin, seed=2)
        split = eg.pool_in(f["plain"]) != eg.pool_in(f["fused"])
        assert split.sum() >= 100 and not split[100:].any()
        s = eg.radius_pairs("pool_sqrt", n_split=100, n_agree=20, origin=origin, seed=3)
        by_norm = np.sqrt(s["plain"]) < eg.POOL_RADIUS
        assert (eg.pool_in(s["plain"]) != by_norm).sum() >= 100
        assert np.all(np.abs(np.sqrt(s["plain"]) - eg.POOL_RADIUS) <= 4 * np.spacing(eg.POOL_RADIUS))


def test_affinity_oracles_give_cdists_mask(affinity_pairs):
    P, Q = affinity_pairs["P"], affinity_pairs["Q"]
    m = P.shape[0]
    pts = np.empty((2 * m, 3))
    pts[0::2], pts[1::2] = P, Q
    exp = _pair_cdist(P, Q) <= 1.0
    rows = np.arange(m) * 2
    S = ncuts_ref.affinity_sparse(pts, alpha=1.0)
    D = ncuts_ref.affinity_dense(pts, alpha=1.0)
    assert np.array_equal(np.asarray(S[rows, rows + 1]).ravel() != 0, exp)
    assert np.array_equal(np.asarray(S[rows + 1, rows]).ravel() != 0, exp)
    assert np.array_equal(D[rows, rows + 1] != 0, exp)
    # the pairs are alone: nothing else is within the radius
    assert S.nnz == 2 * m + 2 * int(exp.sum()) and np.count_nonzero(D) == S.nnz


def test_pool_oracle_states_the_squared_rule():
    for kind, seed in (("pool_fused", 2), ("pool_sqrt", 3)):
        for origin in ORIGINS.values():
            c = eg.radius_pairs(kind, n_split=100, n_agree=20, origin=origin, seed=seed)
            feat = np.ones((c["Q"].shape[0], 1), np.float32)
            got = points_ref.tarl_pool(c["P"], c["Q"], feat, eg.POOL_RADIUS)[:, 0]
            exp = eg.pool_in(c["plain"])
            assert np.array_equal(got == 1.0, exp) and np.all((got == 1.0) | (got == 0.0)), (kind, origin)


def test_nn1_fixtures_hold_ties():
    t = eg.nn1_pair_ties(150, seed=2)
    assert t["tie"].sum() >= 90 and (~t["tie"]).sum() >= 40 and t["fused_flip"].sum() >= 10
    s = eg.sq_plain(t["queries"], t["sources"][0::2]), eg.sq_plain(t["queries"], t["sources"][1::2])
    assert np.array_equal(s[0] == s[1], t["tie"])
    assert np.all(np.abs(s[0] - s[1]) <= np.spacing(np.maximum(s[0], s[1])))
    lat = eg.nn1_lattice()
    S = eg.sq_plain(lat["queries"][:, None], lat["sources"][None])
    ties = (S == S.min(1, keepdims=True)).sum(1)
    assert (ties >= 2).sum() >= 100 and (ties >= 8).sum() >= 5
    lo, hi = lat["sources"].min(0), lat["sources"].max(0)
    out = np.any((lat["queries"] < lo) | (lat["queries"] > hi), axis=1)
    assert out.sum() >= 30
    # every source on a border of ai_nn1_project's cells (0.5 m from the sources' minimum)
    k = (lat["sources"] - lo) / eg.NN1_CELL
    assert np.array_equal(k, np.round(k))


def test_nn1_oracle_states_the_tie_rule():
    t = eg.nn1_pair_ties(150, seed=2)
    lat = eg.nn1_lattice()
    for q, s in ((t["queries"], t["sources"]), (lat["queries"], lat["sources"])):
        for src in (s, s[::-1].copy()):
            idx, d = points_ref.nn1_index(q, src)
            eidx, ed = eg.nn1_brute(q, src)
            assert np.array_equal(idx, eidx) and d.tobytes() == ed.tobytes()
    # per tie case: the smaller index of the two, in either order
    idx, _ = points_ref.nn1_index(t["queries"], t["sources"])
    s0, s1 = eg.sq_plain(t["queries"], t["sources"][0::2]), eg.sq_plain(t["queries"], t["sources"][1::2])
    assert np.array_equal(idx, 2 * np.arange(idx.size) + (s1 < s0))


def test_knn_lattice_sits_on_the_cell_borders():
    p = eg.knn_lattice(side=6.0)
    cell = eg.knn_cell(p)
    assert cell == 0.5 and p.shape[0] == 1728
    k = (p - p.min(0)) / cell
    on = np.any(k == np.round(k), axis=1)
    assert on.mean() > 0.5
    assert p.shape[0] - np.unique(p, axis=0).shape[0] >= 100         # duplicates
    D = np.sqrt(eg.sq_plain(p[:, None], p[None]))
    Ds = np.sort(D, axis=1)
    assert (Ds[:, 19] == Ds[:, 20]).mean() > 0.3                      # the 20th and 21st neighbour tie
    np.testing.assert_array_equal(prep_ref.knn_avg(p, 20), prep_ref.knn_avg_brute(p, 20))
    assert math.isclose(prep_ref.knn_avg_brute(p, 20).mean(), Ds[:, :20].mean(), rel_tol=1e-12)
