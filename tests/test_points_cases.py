"""CPU proofs for tests/points_cases.py: every fixture sits in the regime its name claims, the host models equal brute force
on all of them, the stop rule of `kp_nn1` before the rounding of `pcell_of` was counted misses every ring-stop case and
the shipped one misses none (also in a seeded adversarial search), and eight deliberately wrong rules are each rejected by a
named fixture.  No GPU, no library."""
import numpy as np
import pytest

import edge_geometry as eg
import points_cases as pc


def _grid(case, cell):
    return pc.grid_of(case.sources, cell)


# ------------------------------------------------------------------------------------------------- constants
def test_constants_are_read_from_the_sources():
    assert pc.K == dict(AI_BLOCK=256, LANES=16, MAXK=24, MAX_DIM=384, CELL_CAP=1 << 27, GROW=1.5, EXTENT_LIMIT=1e15, NN1_CELL=0.5,
                        POOL_CELL_FACTOR=1.0 + 1e-9, SLACK_ULPS=8.0, STOP_ULPS=4.0)
    assert pc.NN1_CELL == eg.NN1_CELL and pc.QUERIES_PER_BLOCK == 16
    assert pc.POOL_WIDTHS == (1, 15, 16, 17, 96, 383, 384) and pc.POOL_NQ == (1, 15, 16, 17) and pc.NN1_NT == (255, 256, 257)


# ------------------------------------------------------------------------------------------------- regime claims
def test_issue_case_is_what_the_issue_says():
    c = pc.issue_case()
    g = _grid(c, pc.NN1_CELL)
    assert g.n.tolist() == [[67, 1, 1]] and not g.grown[0]
    assert pc.cells_of(g, c.sources[None])[0, :, 0].tolist() == [0, 61, 66] and pc.cells_of(g, c.queries)[0, 0] == 63
    sq = eg.sq_plain(c.queries[0], c.sources)
    assert sq[1] == 1.0 and sq[2] == 0.9999999999999996
    # B lies below the border of cell 66 (33 m from the minimum): only fl(x - min) puts it there
    from fractions import Fraction
    assert Fraction(pc.ISSUE_CASE["B"]) - Fraction(pc.ISSUE_CASE["anchor"]) < 33 and pc.ISSUE_CASE["B"] - pc.ISSUE_CASE["anchor"] == 33.0
    assert c.truth[0][0] == 2
    assert pc.nn1_model(c.queries, c.sources, stop="parent")[0][0] == 1
    idx, dist, rings = pc.nn1_model(c.queries, c.sources, stop="shipped")
    assert idx[0] == 2 and rings[0] == 3 and dist[0] == c.truth[1][0]


def test_ring_stop_cases_cover_axes_directions_rings_and_variants():
    cases = pc.ring_stop_cases()
    assert 24 <= len(cases) <= 48
    plain = {(c.claims["axis"], c.claims["sgn"], c.claims["r"]) for c in cases if c.claims["variant"] == "plain"}
    assert plain == {(a, s, r) for a in range(3) for s in (-1, 1) for r in (1, 2, 3)}
    for variant in ("outside", "grown"):
        some = [c for c in cases if c.claims["variant"] == variant]
        assert len(some) >= 4 and {c.claims["r"] for c in some} == {1, 2, 3} and len({c.claims["sgn"] for c in some}) == 2
    for c in cases:
        g = _grid(c, pc.NN1_CELL)
        q = c.queries
        if c.name != "ring_stop_issue":
            assert (g.n > 1).all(), f"{c.name}: the grid is not 3-D"
        inside = (pc.cells_of(g, q, clamp=False) == pc.cells_of(g, q)).all()
        if c.claims["variant"] == "outside":
            assert not inside and (q < g.mn).any(), f"{c.name}: the query is inside the box"
        else:
            assert inside
        if c.claims["variant"] == "grown":
            assert g.grown[0] and g.cell[0] == pc.NN1_CELL * pc.GROW and np.log2(g.cell[0]) % 1 != 0 and g.ncell[0] <= pc.CELL_CAP
            assert 2 * 4 * int(g.ncell[0]) < 1e9, "the two tables of the grown grid stay under 1 GB"
        else:
            assert not g.grown[0]
        # B is the answer, A is r cells from the query, and B's stored cell is one beyond the rings that hold A
        A, B, ax, r = c.claims["A"], c.claims["B"], c.claims["axis"], c.claims["r"]
        assert c.truth[0][0] == B != A
        sc, qc = pc.cells_of(g, c.sources[None])[0], pc.cells_of(g, q)[0]
        assert np.abs(sc[B] - qc).max() == r + 1 and np.abs(sc[A] - qc).max() <= r and abs(sc[B][ax] - qc[ax]) == r + 1
        assert np.sqrt(eg.sq_plain(q[0], c.sources[A])) == r * g.cell[0]


def test_growth_fixtures_grow_and_the_extent_under_the_cap_does_not():
    for case, cell in ((pc.growth_nn1_case(), pc.NN1_CELL), (pc.growth_pool_case(), pc.pool_cell(pc.POOL_RADIUS))):
        g = _grid(case, cell)
        assert g.grown[0] and g.cell[0] > cell and g.ncell[0] <= pc.CELL_CAP < pc.grid_of(case.sources, cell, grow=False).ncell[0]
        assert 2 * 4 * int(g.ncell[0]) < 1e9, "the two tables of the grown grid stay under 1 GB"
        # every query within two cells of a source: no lane walks a sparse grid
        near = np.abs(pc.cells_of(g, case.sources[None])[0][None] - pc.cells_of(g, case.queries)[:, None]).max(axis=2).min(axis=1)
        assert near.max() <= 2
        assert 2000 <= case.sources.shape[0] <= 5000
        ext = pc.under_cap_extent(cell)
        corners = np.array([eg.MAP_ORIGIN, eg.MAP_ORIGIN + ext])
        gu = pc.grid_of(corners, cell)
        assert not gu.grown[0] and gu.ncell[0] == pc.CELL_CAP
        assert pc.grid_of(np.array([eg.MAP_ORIGIN, eg.MAP_ORIGIN + ext + [cell, 0, 0]]), cell).grown[0]


def test_block_edge_and_width_fixtures():
    for d in pc.POOL_WIDTHS:
        c = pc.pool_width_case(d)
        assert c.feat.shape == (c.sources.shape[0], d) and c.claims["tail"] == d % 16
        assert (c.truth["count"] > 1).any()
    assert {pc.pool_width_case(d).claims["tail"] for d in pc.POOL_WIDTHS} >= {0, 1, 15}
    for n in pc.POOL_NQ:
        assert pc.pool_nq_case(n).queries.shape[0] == n
    blocks = [-(-n * pc.LANES // pc.BLOCK) for n in pc.POOL_NQ]
    assert blocks == [1, 1, 1, 2]
    assert [-(-n // pc.BLOCK) for n in pc.NN1_NT] == [1, 1, 2]
    for n in pc.NN1_NT:
        assert pc.nn1_nt_case(n).queries.shape[0] == n


def test_degenerate_grids():
    want = {"one_source": [1, 1, 1], "identical": [1, 1, 1]}
    for kind in pc.DEGENERATE:
        for case, cell in ((pc.degenerate_nn1_case(kind), pc.NN1_CELL), (pc.degenerate_pool_case(kind), pc.pool_cell(pc.POOL_RADIUS))):
            n = _grid(case, cell).n[0].tolist()
            if kind in want:
                assert n == want[kind]
            elif kind == "coplanar":
                assert n[2] == 1 and n[0] > 1 and n[1] > 1
            else:
                assert n[1] == 1 and n[2] == 1 and n[0] > 1
    assert pc.degenerate_nn1_case("one_source").sources.shape[0] == 1
    assert np.unique(pc.degenerate_nn1_case("identical").sources, axis=0).shape[0] == 1
    assert (pc.degenerate_pool_case("identical").truth["count"] == 50).any()


def test_clamped_queries():
    for where in ("near", "far"):
        c = pc.clamp_pool_case(where)
        g = _grid(c, pc.pool_cell(c.radius))
        assert g.n.max() <= 40 and c.queries.shape[0] == 26
        d = np.abs(pc._directions()) > 0
        assert np.array_equal((c.queries < g.mn) | (c.queries > g.mx), d), "outside the box on exactly the axes of its face, edge or corner"
        low = pc.cells_of(g, c.queries, clamp=False) < 0
        assert np.array_equal(low, pc._directions() < 0), "below the box the cell index is clamped (above it the last cell reaches)"
        gap = np.maximum(np.maximum(g.mn - c.queries, c.queries - g.mx), 0.0)
        if where == "near":
            assert (gap[d] < c.radius).all() and (gap[d] > 0).all() and (c.truth["count"] >= 1).all()
        else:
            assert (gap[d] > c.radius).all() and (c.truth["count"] == 0).all()
    c = pc.clamp_nn1_case()
    g = _grid(c, pc.NN1_CELL)
    assert g.n.max() <= c.claims["max_cells"]
    assert ((c.queries < g.mn) | (c.queries > g.mx)).any(axis=1).all()
    assert (pc.cells_of(g, c.queries, clamp=False) != pc.cells_of(g, c.queries)).any(axis=1).sum() > 100
    far = np.maximum(g.mn - c.queries, c.queries - g.mx).max(axis=1)
    assert far.min() < 2e-3 and 1e6 <= far.max() < 1.1e6


def test_pool_border_pairs_straddle_their_borders():
    c = pc.pool_border_case()
    cell = pc.pool_cell(c.radius)
    g = _grid(c, cell)
    assert g.n.max() <= 41 and np.array_equal(g.mn[0], eg.MAP_ORIGIN)
    assert np.log2(cell) % 1 != 0 and np.log2(1.0 / cell) % 1 != 0
    qc, sc = pc.cells_of(g, c.queries), pc.cells_of(g, c.sources[None])[0][2:]
    kinds = np.array(c.claims["qkind"])
    diff = np.abs(qc - sc)
    assert (diff.sum(axis=1) == 1).all(), "query and source of a pair sit in neighbouring cells of one axis"
    ax = diff.argmax(axis=1)
    rows = np.arange(len(kinds))
    d = np.abs(c.queries[rows, ax] - c.sources[2:][rows, ax])
    st = kinds == "straddle"
    assert st.sum() == 48 and (~st).sum() == 24
    assert (d[st] <= 2 * np.spacing(np.abs(c.queries[rows, ax][st]))).all() and (d[st] > 0).all()
    assert (d[~st] > 0.99 * c.radius).all() and (d[~st] < c.radius).all()
    member = eg.pool_in(eg.sq_plain(c.queries, c.sources[2:]), c.radius)
    assert member.all() and (c.truth["count"] >= 1).all()


def test_crowded_cell_and_exact_radius():
    c = pc.pool_crowded_case()
    assert (c.truth["count"] == 4000).all() and np.unique(c.sources, axis=0).shape[0] < 3300
    g = _grid(c, pc.pool_cell(c.radius))
    assert g.n.max() == 1, "one cell holds them all"
    e = pc.pool_exact_radius_case()
    sq = eg.sq_plain(e.queries[:, None], e.sources[None])
    assert ((sq == eg.r2_of(e.radius)).sum(axis=1) == 6).all() and (e.truth["count"] == 6).all()


def test_nonfinite_fixtures():
    for name, s in pc.nonfinite_sources().items():
        assert not np.isfinite(s).all()
        with pytest.raises(ValueError, match="not finite"):
            pc.grid_of(s, pc.NN1_CELL)
        with pytest.raises(ValueError, match="not finite"):
            pc.grid_of(s, pc.pool_cell(pc.POOL_RADIUS))
    c = pc.nonfinite_query_case()
    assert _grid(c, pc.NN1_CELL).n.max() <= c.claims["max_cells"]
    idx, dist = pc.nonfinite_query_truth(c)
    bad = ~np.isfinite(c.queries).all(axis=1)
    assert bad.sum() == 16 and np.array_equal(np.flatnonzero(bad), c.claims["bad"])
    assert (idx[bad] == -1).all() and np.isnan(dist[bad]).all() and (idx[~bad] >= 0).all() and np.isfinite(dist[~bad]).all()
    v = c.queries[bad][~np.isfinite(c.queries[bad])]
    assert np.isnan(v).sum() >= 3 and (v == np.inf).sum() >= 3 and (v == -np.inf).sum() >= 3


# ------------------------------------------------------------------------------------------------- the stop rule
def test_parent_stop_rule_answers_A_on_every_ring_stop_case():
    for c in pc.ring_stop_cases():
        idx, _, rings = pc.nn1_model(c.queries, c.sources, stop="parent")
        assert idx[0] == c.claims["A"] and rings[0] == c.claims["r"], c.name


def test_models_equal_brute_force_on_every_fixture():
    for c in pc.nn1_cases():
        idx, dist, _ = pc.nn1_model(c.queries, c.sources, stop="shipped")
        pc.check_nn1(c.name, idx, dist, c.truth)
    for c in pc.pool_cases():
        mean, cnt = pc.pool_model(c.queries, c.sources, c.feat, c.radius)
        pc.check_pool(c.name, mean, cnt, c.truth)


def test_shipped_rule_costs_a_ring_only_within_the_slack():
    """The face gap is at least r * cell: the shipped rule never searches more than one ring beyond the parent's, and that one only
    when sqrt(best) is within the slack (and the 4 ulps of the comparison) of r * cell."""
    extra = 0
    for c in pc.nn1_cases():
        g = _grid(c, pc.NN1_CELL)
        _, dp, rp = pc.nn1_model(c.queries, c.sources, stop="parent")
        _, ds, rs = pc.nn1_model(c.queries, c.sources, stop="shipped")
        more = rs > rp
        assert (rs <= rp + 1).all(), c.name
        slack = pc.stop_slack(g, c.queries, np.broadcast_to(g.cell, (c.queries.shape[0],)))
        assert (dp[more] * (1.0 + 8 * pc.EPS) > rp[more] * g.cell[0] - slack[more]).all(), c.name
        extra += int(more.sum())
    assert extra >= len(pc.ring_stop_cases())


SEARCH_TRIES = {"plain": 300_000, "grown": 100_000}


def test_adversarial_search_finds_misses_of_the_parent_rule_only(capsys):
    """The construction of the ring-stop cases at random minimum, ring, axis and direction, 400 000 tries: the parent's rule
    takes the wrong source in several thousand of them (3774 as of writing), the shipped one in none."""
    total = {"tries": 0, "miss_parent": 0, "miss_shipped": 0}
    for variant, tries in SEARCH_TRIES.items():
        r = pc.ring_stop_search(tries, 2024, grown=variant == "grown")
        for k in total:
            total[k] += r[k]
        assert r["miss_parent"] > tries // 1000 and r["miss_shipped"] == 0, (variant, r["miss_parent"], r["miss_shipped"])
    with capsys.disabled():
        print(f"\nring-stop search: {total['tries']} tries, parent rule misses {total['miss_parent']}, shipped rule misses "
              f"{total['miss_shipped']}")
    assert total["tries"] == 400_000


# ------------------------------------------------------------------------------------------------- wrong rules
def _rejected(check, *args):
    with pytest.raises(AssertionError):
        check(*args)


def test_wrong_rule_le_in_the_pooling_predicate():
    c = pc.pool_exact_radius_case()
    mean, cnt = pc.pool_model(c.queries, c.sources, c.feat, c.radius, mutant="le_predicate")
    assert (cnt == 12).all()
    _rejected(pc.check_pool, c.name, mean, cnt, c.truth)


def test_wrong_rule_ties_to_the_larger_index():
    c = pc.degenerate_nn1_case("identical")
    idx, dist, _ = pc.nn1_model(c.queries, c.sources, mutant="ties_larger")
    assert (idx == c.sources.shape[0] - 1).all() and (c.truth[0] == 0).all()
    _rejected(pc.check_nn1, c.name, idx, dist, c.truth)


def test_wrong_rule_no_clamping_of_outside_queries():
    c = pc.clamp_pool_case("near")
    mean, cnt = pc.pool_model(c.queries, c.sources, c.feat, c.radius, mutant="no_clamp")
    _rejected(pc.check_pool, c.name, mean, cnt, c.truth)
    n = pc.clamp_nn1_case()
    idx, dist, _ = pc.nn1_model(n.queries, n.sources, mutant="no_clamp")
    _rejected(pc.check_nn1, n.name, idx, dist, n.truth)


def test_wrong_rule_sum_not_divided_by_the_count():
    for c in (pc.pool_crowded_case(), pc.pool_width_case(96)):
        mean, cnt = pc.pool_model(c.queries, c.sources, c.feat, c.radius, mutant="no_divide")
        _rejected(pc.check_pool, c.name, mean, cnt, c.truth)


def test_wrong_rule_feature_tail_dropped():
    for d in (1, 15, 17, 383):
        c = pc.pool_width_case(d)
        mean, cnt = pc.pool_model(c.queries, c.sources, c.feat, c.radius, mutant="drop_tail")
        _rejected(pc.check_pool, c.name, mean, cnt, c.truth)


def test_wrong_rule_cell_not_grown():
    """A cell that is too small does not change an answer (a finer grid is as exact), it asks for a table above the cap: the
    growth fixtures reject it by the table's size."""
    for c, cell in ((pc.growth_nn1_case(), pc.NN1_CELL), (pc.growth_pool_case(), pc.pool_cell(pc.POOL_RADIUS))):
        pc.check_grid(c.name, pc.grid_of(c.sources, cell))
        _rejected(pc.check_grid, c.name, pc.grid_of(c.sources, cell, grow=False))


def test_wrong_rule_the_parents_stop_rule():
    for c in pc.ring_stop_cases():
        idx, dist, _ = pc.nn1_model(c.queries, c.sources, stop="parent")
        _rejected(pc.check_nn1, c.name, idx, dist, c.truth)


def test_wrong_rule_nan_source_kept():
    kept = 0
    for name, s in pc.nonfinite_sources().items():
        try:
            g = pc.grid_of(s, pc.NN1_CELL, nan="drop")
        except ValueError:
            continue                                            # an infinity, or a whole axis of NaN, fails either way
        kept += 1
        assert "nan" in name and np.isfinite(g.mn).all() and np.isfinite(g.mx).all()
    assert kept == 3, "fmin / fmax lose a NaN coordinate on each axis: the fixture tells the two folds apart"
