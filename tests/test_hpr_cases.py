"""CPU proofs for tests/hpr_cases.py: every fixture sits where its name says -- which re-solve of `kh_local` falls behind the
first 64 records of a cell and in which lane, how many survivors `kh_global` gets, which of its re-solves fall in the last tile and
on the view's last record -- the traced walk equals the restatement on every fixture, and the re-solve statistics tell a wrong
skip rule from the shipped one.  No GPU.  Run with ``-s`` to see the figures."""
import numpy as np
import pytest

import hpr_cases as hc
import hpr_ref

W = hc.WAVE


def walked_equals_truth(c):
    w = c.walked
    rows, stats = c.truth
    assert np.array_equal(np.flatnonzero(w["flags"]), rows) and hc.stats_list(w["stats"]) == stats, c.name
    assert w["unsound"] == 0


# ------------------------------------------------------------------------------------------------- constants
def test_constants_are_read_from_the_sources():
    from autoinst_amd.config import HPR_RADIUS
    assert hc.K == dict(HP_GRID=64, HP_TILE=256, HP_STEP=4, HP_BOX=1e12, HP_SKIP_EPS=1e-9, AI_BLOCK=256)
    assert (hpr_ref.GRID, hpr_ref.TILE, hpr_ref.BOX, hpr_ref.SKIP_EPS) == (hc.GRID, hc.TILE, hc.K["HP_BOX"], hc.K["HP_SKIP_EPS"])
    assert hc.HPR_RADIUS == HPR_RADIUS
    assert hc.CELL_POPULATIONS == (63, 64, 65, 127, 128, 129, 300) and hc.SHELL_NS == (255, 256, 257, 511, 512, 513, 1025)
    assert hc.TAILS == (0, 1, 2, 3, 4, 5)
    assert len(hc.cases()) == 7 * 4 + 7 * 2 + 6 + 2 + 6


# ------------------------------------------------------------------------------------------------- crowded cells
@pytest.mark.parametrize("where", hc.WHERES)
@pytest.mark.parametrize("P", hc.CELL_POPULATIONS)
def test_cell_fixtures(P, where):
    c = hc.cell_case(P, where)
    cl = c.claims
    walked_equals_truth(c)
    pops = hc.cell_population(c)
    assert pops[cl["crowded"]] == P, "the crowded cell's population"
    if where == "own":
        assert pops == {cl["crowded"]: P} and cl["lane"] == 0
    else:
        assert pops == {cl["crowded"]: P, cl["query"]: hc.QUERY_CELL_POINTS} and cl["lane"] >= 1
        off = np.array(hc.RING_OFFSETS[where])
        assert cl["crowded"] - cl["query"] == int((off * [1, hc.GRID, hc.GRID * hc.GRID]).sum()) and off.sum() == hc.WHERES.index(where)
    got = hc.cell_positions(c, cl["lane"])
    print(c.name, "first near", cl["first_near"], "re-solves in the crowded cell at", sorted(got))
    assert cl["first_near"] in got
    if P > W:
        assert max(got) >= W, "no re-solve behind the first 64 records"
    if where != "own":
        # the walks of the query cell's points: lane 0 (their own six records) is not empty, the re-solve falls in lane s >= 1
        pr = hc.hpr_refprepare(c)
        mine = [p for p in range(pr["n"]) if int(pr["skey"][p]) == cl["query"]]
        assert len(mine) == hc.QUERY_CELL_POINTS
        assert all([s for s, _, _ in hc.segments(pr, p)] == [0, cl["lane"]] for p in mine)
        assert any(s == cl["lane"] for p in mine for _, s, _ in c.walked["local"][p])


def test_first_violations_fall_on_both_sides_of_the_64_record_turns():
    got = {}
    for P in (W, W + 1, 2 * W, 2 * W + 1):
        for where in hc.WHERES:
            c = hc.cell_case(P, where)
            for j in hc.cell_positions(c, c.claims["lane"]):
                got.setdefault(j, []).append(c.name)
    for j in (W - 1, W, W + 1):
        assert j in got, f"no first violation at position {j} of a cell"
    assert 2 * W - 1 in got and 2 * W in got
    # a re-solve whose earlier part of the cell (cnt_cur) is 64 or more, with `from` inside a later turn: one cell, two re-solves
    c = hc.cell_case(2 * W + 1, "face")
    assert any(sum(1 for _, s, j in tr if s == c.claims["lane"] and j > W) >= 2 for tr in c.walked["local"] if tr)


# ------------------------------------------------------------------------------------------------- shells
@pytest.mark.parametrize("hidden", [False, True])
@pytest.mark.parametrize("n", hc.SHELL_NS)
def test_shell_fixtures(n, hidden):
    c = hc.shell_case(n, hidden)
    walked_equals_truth(c)
    rows, stats = c.truth
    d = np.linalg.norm(c.points, axis=1)
    assert c.points.shape[0] == n + hidden and rows.size == n == c.walked["survivors"]
    if hidden:
        at, front = c.claims["hidden"], c.claims["front"]
        assert np.array_equal(rows, np.delete(np.arange(n + 1), at)) and stats[0] == 1
        e = c.points / d[:, None]
        assert np.array_equal(e[at], e[front + (front >= at)]) and d[at] > 9.0
        d = np.delete(d, at)
    else:
        assert stats == [0, 0, 0, 0]
    assert (np.abs(d / 5.0 - 1.0) <= 0.01 + 1e-12).all()


# ------------------------------------------------------------------------------------------------- tile tails
@pytest.mark.parametrize("r", hc.TAILS)
def test_tail_fixtures(r):
    c = hc.tail_case(r)
    walked_equals_truth(c)
    m = c.claims["m"]
    assert c.points.shape[0] == m == 2 * hc.TILE + r
    last_tile = (m - 1) // hc.TILE * hc.TILE
    hit = sorted(k for tr in c.walked["glob"] if tr for k in tr)
    print(c.name, "global re-solves", len(hit), "in the last tile", [k for k in hit if k >= last_tile][:8])
    assert any(k >= last_tile for k in hit), "no survivor re-solves inside the last tile"
    if r % hc.STEP:
        assert m - 1 in hit, "no survivor re-solves at the view's last record"
    assert hc.tail_case_holds(c) and 0 < c.truth[0].size < m and c.truth[1][0] > 0


def test_the_tail_seeds_are_what_the_search_finds():
    build, holds = hc.searched()["tail_2"]
    assert hc.seed_search(build, holds) == hc.SEEDS["tail_2"] and set(hc.SEEDS) == set(hc.searched())


# ------------------------------------------------------------------------------------------------- the skip rule
@pytest.fixture(scope="module")
def skip_walks():
    out = {}
    for f in hc.SKIP_FACTORS:
        c = hc.skip_regime_case(f)
        out[f] = {v: hc.walk(c.points, c.factor, v) for v in ("rule",) + hc.SKIP_VARIANTS}
    return out


@pytest.mark.parametrize("factor", hc.SKIP_FACTORS)
def test_the_rule_passes_over_no_violated_constraint_in_the_skip_regime(factor, skip_walks):
    c = hc.skip_regime_case(factor)
    w = skip_walks[factor]["rule"]
    rows, stats = c.truth
    assert c.points.shape[0] == 2000 and w["passed"] > 0 and w["unsound"] == 0
    assert np.array_equal(np.flatnonzero(w["flags"]), rows) and hc.stats_list(w["stats"]) == stats      # changed == 0


@pytest.mark.parametrize("variant", hc.SKIP_VARIANTS)
def test_the_resolve_statistics_tell_a_wrong_skip_rule_from_the_right_one(variant, skip_walks):
    """A device whose skip rule were ``variant`` would pass over violated constraints (unsound > 0) and, at one of the two
    factors at least, report other flags, another re-solve total or another largest count than the restatement."""
    seen = []
    for f in hc.SKIP_FACTORS:
        right, wrong = skip_walks[f]["rule"], skip_walks[f][variant]
        differs = (not np.array_equal(right["flags"], wrong["flags"])) or hc.stats_list(right["stats"]) != hc.stats_list(wrong["stats"])
        print(f"factor {f:g} {variant}: unsound {wrong['unsound']}, flags changed {int((right['flags'] != wrong['flags']).sum())}, "
              f"stats {hc.stats_list(wrong['stats'])} against {hc.stats_list(right['stats'])}")
        assert wrong["unsound"] > 0
        seen.append(differs)
    assert any(seen), f"{variant}: neither factor shows in the flags or in the re-solve statistics"


# ------------------------------------------------------------------------------------------------- H6
def test_h6_fixtures_are_skipped_or_kept_as_named():
    lo, hi = hc.h6_far_factors()
    steps = 0
    x = lo
    while x < hi:
        x, steps = float(np.nextafter(x, np.inf)), steps + 1
    assert steps == 3 and hpr_ref.prepare(hc.far_cloud(), float(np.nextafter(lo, np.inf))) is not None
    for name, c in hc.h6_cases().items():
        assert (hpr_ref.prepare(c.points, c.factor) is None) == c.claims["skipped"] == (c.truth[0] is None), name
    p = hc.far_cloud()
    two_R = 2.0 * (1e160 * np.linalg.norm(p.max(axis=0) - p.min(axis=0)))
    with np.errstate(over="ignore"):
        assert np.isfinite(two_R) and np.isinf(two_R * two_R)                        # S overflows, R does not
    q = hc.h6_cases()["h6_equal_points"].points
    assert q.shape == (8, 3) and (q == q[0]).all()
    kept = hc.h6_cases()["h6_far_kept"]
    walked_equals_truth(kept)
    assert 0 < kept.truth[0].size < 300
    factor, T, skipped = hc.h6_far_views()
    assert [hpr_ref.prepare(hpr_ref.transform(p, t), factor) is None for t in T] == skipped == [True, False, True]


def test_order_views():
    cloud, T = hc.order_views()
    sets = hpr_ref.visible_sets(cloud, T)
    assert [s is None for s in sets] == [False, False, True, False, False]
    assert np.array_equal(sets[0], hc.cell_case(2 * W + 1, "own").truth[0]) and len({s.tobytes() for s in sets if s is not None}) >= 3
