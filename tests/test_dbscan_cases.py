"""CPU proofs for tests/dbscan_cases.py: every fixture sits where its name says, the model of the device's search
(`search_model`) equals the truth on every fixture, and each of four deliberately wrong searches is rejected by exactly the
fixtures named for it.  No GPU, no library.  Run with ``-s`` to see the variant -> fixture table."""
import numpy as np
import pytest

import dbscan_cases as dc
import dbscan_ref
import edge_geometry as eg
import points_cases as pc


@pytest.fixture(scope="module")
def built():
    return {name: build() for name, build in dc.cases().items()}


def cloud(c):
    assert len(c.clouds) == 1
    return c.clouds[0]


# ------------------------------------------------------------------------------------------------- constants
def test_constants_are_read_from_the_sources():
    assert dc.K == dict(DB_CELL_SLACK=1e-6, AI_BLOCK=256, SCAN_TILE=2048, CELL_CAP=1 << 27, GROW=1.5, EXTENT_LIMIT=1e15, N_LIMIT=1 << 30)
    assert dc.SCAN_NS == (2047, 2048, 2049)
    assert len(dc.cases()) == 16 + 1 + 1 + 4 + 1 + 3 + 3 + 3


# ------------------------------------------------------------------------------------------------- the model is the truth
def test_the_shipped_search_equals_the_truth(built):
    for name, c in built.items():
        runs = [(c.eps, c.truth)] + ([(float(np.nextafter(c.eps, 0)), c.truth_below)] if c.below else [])
        for eps, truth in runs:
            got = dc.search_model(c.clouds, eps, c.ms)
            bad = [i for i, (g, w) in enumerate(zip(got, truth)) if not dc.same(g, w)]
            assert not bad, f"{name} at eps {eps!r}: the ring search differs from the full matrix in clouds {bad[:5]} (a design bug)"


def test_every_wrong_search_is_rejected_by_its_fixtures(built):
    table = {v: tuple(n for n, c in built.items() if dc.rejects(c, v)) for v in dc.VARIANTS}
    for v in dc.VARIANTS:
        print(f"{v:20s} rejected by {', '.join(table[v])}")
    assert set(dc.REJECTED_BY) == set(dc.VARIANTS)
    for v in dc.VARIANTS:
        assert table[v], f"{v} is accepted everywhere"
        assert set(table[v]) == set(dc.REJECTED_BY[v]), (v, sorted(set(table[v]) ^ set(dc.REJECTED_BY[v])))


# ------------------------------------------------------------------------------------------------- border pairs
def test_the_search_finds_pairs_from_the_issues_example():
    eps, a, b, k = dc.border_pair_search(100, [71, 0, False, False], big=False, mn=0.0)[0]
    assert (eps, a, b, k) == (dc.ISSUE_PAIR["eps"], dc.ISSUE_PAIR["a"], dc.ISSUE_PAIR["b"], 2)
    assert dc.border_pair_case("x", "small", "zero").eps == eps


@pytest.mark.parametrize("name", dc.BORDER_NAMES)
def test_border_pairs_are_two_cells_apart_without_the_slack(name, built):
    c = built[name]
    p, cl = cloud(c), c.claims
    a, b, ax = p[cl["a"]], p[cl["b"]], cl["axis"]
    origin = np.zeros(3) if name.endswith("zero") else eg.MAP_ORIGIN
    assert np.array_equal(p.min(axis=0), origin) and p[:, ax].max() > b[ax]
    assert (cl["k"] >= 8000) if "_big_" in name else (cl["k"] <= 40)
    # D1 holds with equality, and fails one step of the doubles below eps
    d2 = dbscan_ref.d1_sq_dist(a, b)
    below = float(np.nextafter(c.eps, 0))
    assert d2 == c.eps * c.eps and d2 > below * below
    # the cells: two apart when the cell is eps (clamped or not), at most one apart with the slack, on every axis
    for clamp in (False, True):
        bare = pc.cells_of(pc.grid_of(p, c.eps), np.stack([a, b])[None], clamp=clamp)[0]
        assert bare[1, ax] - bare[0, ax] == 2 and bare[0, ax] == cl["k"] - 1
    g = dc.device_grid(p, c.eps)
    assert not g.grown[0]
    shipped = pc.cells_of(g, np.stack([a, b])[None])[0]
    assert np.abs(shipped[1] - shipped[0]).max() <= 1
    assert shipped[1, 1] - shipped[0, 1] == (1 if "_xy_" in name else 0) or ax == 1
    # the pair is the whole evidence
    lab, k, counts, sizes = c.truth[0]
    want = np.full(p.shape[0], -1)
    want[[cl["a"], cl["b"]]] = 0
    assert k == 1 and np.array_equal(lab, want) and sizes.tolist() == [2] and counts[[cl["a"], cl["b"]]].tolist() == [2, 2]
    for gone in (cl["a"], cl["b"]):
        lab, k, _, _ = dbscan_ref.dbscan_brute(np.delete(p, gone, axis=0), c.eps, c.ms)
        assert k == 0 and (lab == -1).all()
    assert c.truth_below[0][1] == 0 and (c.truth_below[0][2] == 1).all()


# ------------------------------------------------------------------------------------------------- grids
def test_grown_grid_grew_the_cell_and_holds_threshold_pairs(built):
    c = built["grown_grid"]
    p = cloud(c)
    g = dc.device_grid(p, c.eps)
    assert g.grown[0] and g.cell[0] >= c.eps * (1.0 + dc.SLACK) * dc.K["GROW"] ** 3 and g.ncell[0] <= dc.K["CELL_CAP"]
    assert pc.grid_of(p, c.eps * (1.0 + dc.SLACK), grow=False).ncell[0] > dc.K["CELL_CAP"]
    lab, k, counts, _ = c.truth[0]
    tags = [t for t, _, _ in c.claims["pairs"]]
    assert tags.count("at") == 12 and tags.count("beyond") == 12
    for tag, i, j in c.claims["pairs"]:
        d2 = dbscan_ref.d1_sq_dist(p[i], p[j])
        if tag == "at":
            assert d2 == c.eps * c.eps and counts[i] == counts[j] == 2 and lab[i] == lab[j] >= 0
        else:
            assert d2 > c.eps * c.eps and counts[i] == counts[j] == 1 and lab[i] == lab[j] == -1
    assert k > 12


def test_one_cell(built):
    c = built["one_cell"]
    p = cloud(c)
    assert dc.device_grid(p, c.eps).n[0].tolist() == [1, 1, 1]
    lab, k, counts, _ = c.truth[0]
    assert k == 1 and counts.min() < c.ms and (counts == c.ms).any()              # the cell holds pairs that are no neighbours


@pytest.mark.parametrize("axis", "xyz")
def test_last_cell_is_the_only_cell_of_its_axis(axis, built):
    c = built[f"last_cell_{axis}"]
    p, cl = cloud(c), c.claims
    ax = cl["axis"]
    n = dc.device_grid(p, c.eps).n[0]
    assert n[ax] == 1 and n[(ax + 1) % 3] == n[(ax + 2) % 3] == 9
    assert p[cl["a"], ax] == p[:, ax].min() and p[cl["b"], ax] == p[:, ax].max()
    assert dbscan_ref.d1_sq_dist(p[cl["a"]], p[cl["b"]]) == c.eps * c.eps
    lab, k, counts, _ = c.truth[0]
    assert k == 0 and counts[[cl["a"], cl["b"]]].tolist() == [2, 2] and counts.sum() == p.shape[0] + 2


def test_last_cell_of_a_wide_axis(built):
    c = built["last_cell_wide"]
    p, cl = cloud(c), c.claims
    g = dc.device_grid(p, c.eps)
    cells = pc.cells_of(g, p[None])[0]
    assert g.n[0, 0] == 40 and cells[cl["b"], 0] == 39 and cells[cl["a"], 0] == 38 and p[cl["b"], 0] == p[:, 0].max()
    assert c.truth[0][1] == 1 and c.truth[0][0][[cl["a"], cl["b"]]].tolist() == [0, 0]


# ------------------------------------------------------------------------------------------------- many clouds
def test_the_cloud_list_has_the_stated_structure(built):
    c = built["clouds_300"]
    sizes = [x.shape[0] for x in c.clouds]
    assert len(c.clouds) == dc.N_CLOUDS == 300 > dc.BLOCK and 11_000 < c.n < 13_000    # kd_nclusters goes past its first block
    assert [i for i, s in enumerate(sizes) if s == 0] == sorted(dc.CLOUDS_EMPTY) and sizes[0] == sizes[-1] == 0
    assert all(i + 1 in dc.CLOUDS_EMPTY for i in range(100, 104))                  # a run of five
    assert [i for i, s in enumerate(sizes) if s == 1] == sorted(dc.CLOUDS_SINGLE)
    assert all(s == 40 for i, s in enumerate(sizes) if i not in dc.CLOUDS_EMPTY + dc.CLOUDS_SINGLE)
    a, b = dc.CLOUDS_EQUAL
    assert c.clouds[a].tobytes() == c.clouds[b].tobytes() and c.clouds[a] is not c.clouds[b]
    t = c.truth
    assert all(t[i][1] == 0 and t[i][0].tolist() == [-1] for i in dc.CLOUDS_SINGLE)
    first = t[dc.CLOUD_NOISE_FIRST]
    assert first[0][0] == -1 and first[2][0] == 1 and first[1] >= 2                # rank[off[c]] is not a root's rank
    assert t[dc.CLOUD_NO_CLUSTER][1] == 0 and (t[dc.CLOUD_NO_CLUSTER][0] == -1).all() and t[dc.CLOUD_AFTER_IT][1] >= 2
    assert t[dc.CLOUD_NO_CLUSTER - 1][1] >= 2
    full = [x for x in t if x[0].shape[0] == 40]
    assert sum(x[1] for x in full) > 800 and any((x[0] == -1).any() for x in full) and len({x[1] for x in full}) >= 3
    # the clouds share their cells: all 290 full clouds but the blown-up one in the cells of one of them, a handful each
    g = dc.device_grid(np.concatenate(c.clouds), c.eps)
    key = lambda x: {tuple(v) for v in pc.cells_of(g, x[None])[0]}
    cells = [key(x) for i, x in enumerate(c.clouds) if x.shape[0] == 40 and i != dc.CLOUD_NO_CLUSTER]
    assert 50 * len(set.union(*cells)) < c.n and all(len(s & cells[0]) >= 10 for s in cells)   # over 50 points a cell, 40 a cloud


# ------------------------------------------------------------------------------------------------- chains
def test_the_snake_has_the_stated_rows():
    path = dc.snake_path(400, dc.CHAIN_EPS)
    s = 0.9 * dc.CHAIN_EPS
    assert np.allclose(np.unique(np.round(path[:, 1] / s))[:8], [0, 1, 2, 3, 4, 5, 6, 7])
    rows = path[np.isclose(path[:, 1] / s % dc.GAP, 0.0) | np.isclose(path[:, 1] / s % dc.GAP, dc.GAP)]
    assert np.isclose(rows[:, 0].max(), (dc.ROW - 1) * s) and rows[:, 0].min() == 0.0
    assert np.allclose(np.linalg.norm(np.diff(path, axis=0), axis=1), s)


@pytest.mark.parametrize("order", dc.CHAIN_ORDERS)
def test_chains_are_one_cluster_of_core_points(order, built):
    c = built[f"chain_{order}"]
    p, perm = cloud(c), c.claims["perm"]
    assert p.shape[0] == dc.CHAIN_N == 20_000 and c.ms == 2
    lab, k, counts, sizes = c.truth[0]
    assert k == 1 and (lab == 0).all() and sizes.tolist() == [dc.CHAIN_N] and (counts == 2).all()
    # the neighbours of a point are the two next to it on the path, nothing else
    ii, jj = dbscan_ref.neighbour_pairs(p, c.eps)
    assert ii.shape[0] == 2 * (dc.CHAIN_N - 1) and (np.abs(perm[ii] - perm[jj]) == 1).all()
    step = np.abs(np.diff(perm))
    if order == "evens_up_odds_down":
        assert (step[:dc.CHAIN_N // 2 - 1] == 2).all() and (step[dc.CHAIN_N // 2:] == 2).all() and perm[0] == 0 and perm[-1] == 1
    else:
        assert (step == 1).all() and perm[0] == (0 if order == "ascending" else dc.CHAIN_N - 1)


def nearest(a, b):
    """The distance from every point of b to the nearest point of a."""
    from scipy.spatial import cKDTree
    return cKDTree(a).query(b)[0]


def test_two_chains_stay_two(built):
    c = built["two_chains"]
    p, cl = cloud(c), c.claims
    lab, k, counts, sizes = c.truth[0]
    assert 19_000 < p.shape[0] <= dc.CHAIN_N
    assert k == 2 and np.array_equal(lab, cl["labels"]) and sizes.tolist() == cl["sizes"] and (counts == 2).all()
    a, b = p[lab == 0], p[lab == 1]
    gap = float(nearest(a, b).min()) / c.eps
    assert 1.01 - 1e-9 < gap < 1.01 + 1e-9
    close = np.flatnonzero(nearest(a, b) <= 1.0101 * c.eps)
    assert close.size > 0.8 * b.shape[0]                                           # along nearly all of its length
    assert b[:, 2].max() > c.eps and (a[:, 2] == 0).all()                          # the second path crosses over the first


def test_bridge_core_joins_and_bridge_border_does_not(built):
    c = built["bridge_core"]
    p, cl = cloud(c), c.claims
    lab, k, counts, sizes = c.truth[0]
    assert p.shape[0] <= dc.CHAIN_N and cl["bridge"] == p.shape[0] - 1
    assert k == 1 and (lab == 0).all() and sizes.tolist() == [p.shape[0]] and (counts == 2).all()
    ii, jj = dbscan_ref.neighbour_pairs(p, c.eps)
    assert sorted(jj[ii == cl["bridge"]].tolist()) == sorted(cl["touch"])
    assert dbscan_ref.dbscan(p[:-1], c.eps, c.ms)[1] == 2                          # without it: two
    c = built["bridge_border"]
    p, cl = cloud(c), c.claims
    lab, k, counts, sizes = c.truth[0]
    assert p.shape[0] <= dc.CHAIN_N and cl["bridge"] == p.shape[0] - 1 and c.ms == 4
    ii, jj = dbscan_ref.neighbour_pairs(p, c.eps)
    assert sorted(jj[ii == cl["bridge"]].tolist()) == sorted(cl["touch"]) and counts[-1] == 3
    assert (counts[:-1] == 4).all()                                                # every path point is core
    assert k == 2 and (lab[:cl["split"]] == 0).all() and (lab[cl["split"]:-1] == 1).all() and lab[-1] == 0
    assert sizes.tolist() == [cl["split"] + 1, p.shape[0] - 1 - cl["split"]]


# ------------------------------------------------------------------------------------------------- the scan's tile edge
@pytest.mark.parametrize("n", dc.SCAN_NS)
def test_scan_edge(n, built):
    c = built[f"scan_edge_{n}"]
    p = cloud(c)
    lab, k, counts, sizes = c.truth[0]
    assert p.shape[0] == n and c.ms == 1 and (counts == 1).all()
    assert k == c.claims["k"] == n - 20 and lab[-1] == k - 1 and sizes[-1] == 1      # the last point: alone, the last root
    assert sorted(sizes.tolist()) == [1] * (k - 20) + [2] * 20


# ------------------------------------------------------------------------------------------------- refusals
def test_the_refused_arguments_are_past_the_limits():
    lo, hi = dc.REFUSED_EPS
    assert lo > 0.0 and lo * lo == 0.0 and np.isfinite(hi) and hi * hi == np.inf
    p = dc.refused_extent_cloud()
    assert np.isfinite(p).all() and (p.max(axis=0) - p.min(axis=0)).max() >= dc.K["EXTENT_LIMIT"]
    with pytest.raises(ValueError):
        pc.grid_of(p, 0.5)
    assert dc.K["N_LIMIT"] == 2 ** 30
