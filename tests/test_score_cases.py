"""CPU: every fixture of tests/score_cases.py sits on the limit its name claims, and the references agree with ``np.unique``."""
import numpy as np
import pytest

import label_cases as lc
import score_cases as sc
import score_ref as sr


def test_constants_are_read_and_sane():
    k = sc.K
    assert k["KS_MAX_ROWS"] == 64
    for name in ("KS_LDS_SLOTS", "KS_TABLE_MIN", "KS_TABLE_MAX"):
        assert k[name] & (k[name] - 1) == 0, name                       # the tables are indexed with a mask
    assert k["KS_TILE"] < 2 ** 32 and k["KS_TILE"] % 256 == 0           # a 32-bit LDS counter cannot overflow
    assert k["KS_LDS_SLOTS"] < k["KS_TILE"]                             # so a tile can have more pairs than slots
    assert k["KS_TABLE_MIN"] < k["KS_TABLE_MAX"] and k["KS_TABLE_MIN"] % 256 == 0 and k["KS_LOAD_DEN"] >= 2
    assert sc.FIT_MIN > sc.LDS_SLOTS


@pytest.mark.parametrize("name", sc.SMALL_NAMES)
def test_small_fixture_references(name):
    c = sc.small_case(name)
    tables, rem, sco = sr.ref_tables(c.preds, c.gt, c.threshold, c.min_points)
    fast = sr.ref_tables_fast(c.preds, c.gt, c.threshold, c.min_points)
    sr.check_tables(name, fast[0], tables)
    assert np.array_equal(fast[1], rem) and np.array_equal(fast[2], sco)
    for t, (pa, pb, cnt, removed, small) in enumerate(tables):
        if c.gt.size == 0:
            assert pa.size == 0
            continue
        u, n = np.unique(np.stack([c.preds[t], c.gt], 1).astype(np.int64), axis=0, return_counts=True)
        assert np.array_equal(pa, u[:, 0]) and np.array_equal(pb, u[:, 1]) and np.array_equal(cnt, n)
        assert int(cnt.sum()) == c.gt.size
        # S4: the per-point outputs are the flagged labels set to 0
        at = {int(x): i for i, x in enumerate(pa)}
        f_rem = np.array([removed[at[int(x)]] for x in c.preds[t]], bool)
        f_small = np.array([small[at[int(x)]] for x in c.preds[t]], bool)
        assert np.array_equal(rem[t], np.where(f_rem, 0, c.preds[t]))
        assert np.array_equal(sco[t], np.where(f_rem | f_small, 0, c.preds[t]))


def test_random_fixtures_show_every_kind_of_label():
    c = sc.random_case(2, sc.TILE + 1)
    for pa, pb, cnt, removed, small in sr.ref_tables(c.preds, c.gt, c.threshold, c.min_points)[0]:
        assert (removed & ~small).any() and (small & ~removed).any() and (~small & ~removed).any()
        assert cnt[(pa == pa[np.argmax(cnt)]) & (pb == 0)].size == 1


def test_tile_fixtures_are_one_tile_with_the_named_pairs():
    for c, d in zip(sc.tile_cases(), (sc.LDS_SLOTS - 1, sc.LDS_SLOTS, sc.LDS_SLOTS + 1, sc.TILE)):
        assert c.gt.size == sc.TILE and sc.distinct_per_tile(c) == [d] and sc.distinct_per_row(c) == [d] == c.claims["distinct"]


def test_table_fixtures_straddle_the_first_table():
    cases = sc.table_cases()
    assert [sc.distinct_per_row(c)[0] for c in cases] == [sc.FIT_MIN - 1, sc.FIT_MIN, sc.FIT_MIN + 1]
    for c in cases:
        assert c.gt.size > sc.TILE and max(sc.distinct_per_tile(c)) > sc.LDS_SLOTS       # more than one block, and tiles that spill


def test_fallback_fixture_straddles_the_largest_table():
    c = sc.fallback_case()
    assert sc.distinct_per_row(c) == [sc.FIT_MAX, sc.FIT_MAX + 1, 3] == c.claims["distinct"]
    tables, rem, sco = sr.ref_tables_fast(c.preds, c.gt, c.threshold, c.min_points)
    for t in range(3):
        exp = lc.ref_label_pairs(c.preds[t], c.gt)
        lc.check_label_pairs(c.name, tables[t][:3], exp)
    assert (0 in c.gt) and any(tab[3].any() for tab in tables) and any(tab[4].any() for tab in tables)


def test_extremes_fixture_has_the_all_zero_and_all_one_keys():
    c = sc.extremes_case()
    pairs = set(zip(c.preds[0].tolist(), c.gt.tolist()))
    for v in (0, -1, sc.I32_MIN, sc.I32_MAX):
        assert (v, v) in pairs
    assert len({p for p in pairs if p[0] in (sc.I32_MIN, -1, 0, 1, sc.I32_MAX) and p[1] in (sc.I32_MIN, -1, 0, 1, sc.I32_MAX)}) == 25
    assert len(pairs) > 100


def test_boundary_fixture_labels():
    c = sc.boundary_case()
    flags = sr.label_flags(c.preds[0], c.gt, c.threshold, c.min_points)
    for u, (m, z) in c.claims["labels"].items():
        assert int((c.preds[0] == u).sum()) == m and int(((c.preds[0] == u) & (c.gt == 0)).sum()) == z
    for j in range(len(sc.BOUNDARY_M)):
        assert flags[10 + 2 * j] == (False, False) and flags[11 + 2 * j] == (True, False)
    assert flags[0] == (True, False) and flags[-4] == (False, False)
    zero = sc.boundary_case(name="boundary_thr0", threshold=0.0)
    f0 = sr.label_flags(zero.preds[0], zero.gt, 0.0, 0)
    assert all(f0[u][0] == (z >= 1) for u, (m, z) in zero.claims["labels"].items())


def test_min_points_fixture_sizes():
    for c, mp in zip(sc.min_points_cases(), (0, 1, 200)):
        assert c.min_points == mp
        flags = sr.label_flags(c.preds[0], c.gt, c.threshold, mp)
        assert [flags[20 + j][1] for j in range(3)] == [199 < mp, 200 < mp, 201 < mp]
        assert flags[0][1] == (50 < mp)
        assert all(int((c.preds[0] == u).sum()) == s for u, s in c.claims["sizes"].items())
