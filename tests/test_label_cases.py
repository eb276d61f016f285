"""CPU: the fixtures of tests/label_cases.py sit where their names say, the references agree with each other and with the
oracles, and the `check_*` helpers reject a list of deliberately wrong answers.

Mutant -> a fixture that catches it (asserted in `test_*_mutants_*` below):

    drop_upper_offsets, drop_second_level_offsets,
    total_one_tile_early                      scan_{D+1}_all_heads, scan_{D+T+5}_tile_start, scan_20000000_bernoulli_half
    last_run_not_closed_with_n                scan_1_single_run, pairs_distinct_{cap-1, cap}
    unsigned_order                            pairs_extremes, scan_{T+1}_all_heads
    cube_face_exclusive                       merge_face_cube_exact, merge_face_cube_rounds
    box_face_exclusive                        merge_face_box, merge_tile_2_2
    box_tiles_from_id0                        merge_tile_{KM_BOX_TILE+2}_40
    signed_zero_two_scalars                   merge_scalar_signed_zero, merge_scalar_shared_z
    common_per_occurrence                     merge_scalar_repeat, merge_scalar_shared_z
    unique_points keeping the last of a run   unique_signed_zero, unique_ends
"""
import numpy as np
import pytest

import label_cases as lc
import prep_ref
from oracle import merge_ref
from test_labels import np_label_pairs

T, D = lc.T, lc.D


# ------------------------------------------------------------------------------------------------- constants and regimes
def test_constants_are_the_ones_the_issue_was_written_for():
    """Parsed, not assumed; the absolute lengths the done-criteria name follow from them."""
    assert (lc.K["AI_BLOCK"], lc.K["SCAN_ITEMS"], lc.K["SCAN_MAX_DIRECT_TILES"], lc.K["KM_BOX_TILE"]) == (256, 8, 4096, 256)
    assert (T, D, lc.FIRST_CAP) == (2048, 8_388_608, 65_536)


def test_scan_lengths_hit_their_regimes():
    regime = {n: lc.scan_regime(n) for n in lc.SCAN_SMALL_LENGTHS + lc.SCAN_BIG_LENGTHS}
    assert all(regime[n] == "single_tile" for n in (1, 2, lc.BLOCK - 1, lc.BLOCK, lc.BLOCK + 1, T - 1, T))
    assert all(regime[n] == "direct" for n in (T + 1, 2 * T, 2 * T + 1, D - 1, D))
    assert all(regime[n] == "recursive" for n in (D + 1, D + T + 5, lc.SCAN_BIG))
    maxd = lc.K["SCAN_MAX_DIRECT_TILES"]
    assert lc.scan_levels(T) == [1] and lc.scan_levels(T + 1) == [2] and lc.scan_levels(2 * T + 1) == [3]
    assert lc.scan_levels(D - 1) == [maxd] and lc.scan_levels(D) == [maxd]
    assert lc.scan_levels(D + 1) == [maxd + 1, 3]                      # 4097 totals: two full second-level tiles and one value
    assert lc.scan_levels(D + T + 5) == [maxd + 2, 3]
    assert lc.scan_levels(lc.SCAN_BIG) == [9766, 5]
    # the carving: every level's sums (tiles + 1) fit the workspace the library allocates
    for n in lc.SCAN_SMALL_LENGTHS + lc.SCAN_BIG_LENGTHS:
        assert sum(t + 1 for t in lc.scan_levels(n)) <= lc.scan_tmp_elems(n)
    assert lc.scan_tmp_elems(lc.SCAN_BIG) == 9767 + 6 + 2 + 8


def test_scan_fixture_sets_are_the_cross_the_issue_asks_for():
    assert len(lc.scan_names(big=False)) == 10 * 7 and len(lc.scan_names(big=True)) == 5 * 4
    assert any(lc.scan_case(n).claims["shuffled"] for n in lc.scan_names(big=False))
    assert set(lc.SCAN_SHUFFLED) <= set(lc.SCAN_BIG_PATTERNS)


def _check_scan_case(c):
    """heads are what the sorted keys show; the level-by-level model gives np.cumsum; the device-plan model of
    ai_label_pairs equals the np.unique reference."""
    n = c.claims["n"]
    sk = np.sort(lc.pack_pairs(c.a, c.b))
    head = np.ones(n, np.int8)
    head[1:] = sk[1:] != sk[:-1]
    assert np.array_equal(head, c.heads), c.name
    pos = lc.scan_model(c.heads)
    assert pos[0] == 0 and np.array_equal(pos[1:], np.cumsum(c.heads, dtype=np.int64)), c.name
    return pos


@pytest.mark.parametrize("name", lc.scan_names(big=False))
def test_small_scan_fixtures(name):
    c = lc.scan_case(name)
    _check_scan_case(c)
    exp = lc.ref_label_pairs(c.a, c.b)
    lc.check_label_pairs(name, lc.model_label_pairs(c.a, c.b)[:3], exp)
    lc.check_label_pairs(name, np_label_pairs(c.a, c.b), exp)           # packed == row-wise np.unique(axis=0)
    _, n, pattern = name.split("_", 2)
    if pattern == "tile_start":
        assert exp[0].shape[0] == lc.scan_tiles(int(n))
    if pattern == "tile_end" and int(n) >= T:
        assert exp[0].shape[0] == 1 + int(n) // T - (T == 1)
    if pattern == "last_only":
        assert exp[0].shape[0] == min(int(n), 2)


@pytest.mark.parametrize("n", lc.SCAN_BIG_LENGTHS)
def test_big_scan_fixtures(n):
    for pattern in lc.SCAN_BIG_PATTERNS:
        c = lc.scan_case(f"scan_{n}_{pattern}")
        assert c.claims["shuffled"] == (pattern in lc.SCAN_SHUFFLED)
        pos = _check_scan_case(c)
        runs = {"all_heads": n, "single_run": 1, "tile_start": lc.scan_tiles(n)}.get(pattern)
        assert runs is None or pos[n] == runs
        if pattern == "bernoulli_half":
            assert abs(int(pos[n]) - n // 2) < 5 * np.sqrt(n)


def test_scan_mutants_are_caught_by_the_recursive_fixtures():
    catches = {"drop_upper_offsets": f"scan_{D + 1}_all_heads", "drop_second_level_offsets": f"scan_{D + T + 5}_tile_start",
               "total_one_tile_early": f"scan_{lc.SCAN_BIG}_bernoulli_half"}
    for mutant, name in catches.items():
        c = lc.scan_case(name)
        exp = lc.ref_label_pairs(c.a, c.b)
        lc.check_label_pairs(name, lc.model_label_pairs(c.a, c.b)[:3], exp)
        with pytest.raises(AssertionError, match=name):
            lc.check_label_pairs(name, lc.model_label_pairs(c.a, c.b, mutant=mutant)[:3], exp)
    # and they are invisible below the boundary: only the fixtures above it can notice
    c = lc.scan_case(f"scan_{2 * T + 1}_all_heads")
    for mutant in lc.SCAN_MUTANTS:
        lc.check_label_pairs(c.name, lc.model_label_pairs(c.a, c.b, mutant=mutant)[:3], lc.ref_label_pairs(c.a, c.b))


# ------------------------------------------------------------------------------------------------- pairs_*
def test_pair_fixtures_and_capacity():
    cases = {c.name: c for c in lc.pair_cases()}
    cap = lc.FIRST_CAP
    assert {f"pairs_distinct_{k}" for k in (cap - 1, cap, cap + 1)} <= set(cases)
    for c in cases.values():
        exp = lc.ref_label_pairs(c.a, c.b)
        assert exp[0].shape[0] == c.claims["distinct"], c.name
        assert int(exp[2].sum()) == c.a.shape[0]
        lc.check_label_pairs(c.name, np_label_pairs(c.a, c.b), exp)
        lc.check_label_pairs(c.name, lc.model_label_pairs(c.a, c.b)[:3], exp)
    ext = cases["pairs_extremes"]
    assert set(np.unique(ext.a)) == set(np.unique(ext.b)) == {lc.I32_MIN, -1, 0, 1, lc.I32_MAX}
    # the entry point's cap rules, on the model: cap = 0 fills only n_pairs, 0 < cap < total gives the leading rows
    c = cases[f"pairs_distinct_{cap + 1}"]
    exp = lc.ref_label_pairs(c.a, c.b)
    assert lc.model_label_pairs(c.a, c.b, cap=0)[3] == cap + 1 and lc.model_label_pairs(c.a, c.b, cap=0)[0].shape[0] == 0
    got = lc.model_label_pairs(c.a, c.b, cap=cap)
    assert got[3] == cap + 1
    lc.check_label_pairs(c.name, got[:3], tuple(e[:cap] for e in exp))


def test_pair_mutants_are_caught():
    cap = lc.FIRST_CAP
    for name in ("scan_1_single_run", f"pairs_distinct_{cap - 1}", f"pairs_distinct_{cap}"):
        c = lc.scan_case(name) if name.startswith("scan") else lc.pair_case(name)
        with pytest.raises(AssertionError, match="count"):
            lc.check_label_pairs(name, lc.model_label_pairs(c.a, c.b, mutant="last_run_not_closed_with_n")[:3], lc.ref_label_pairs(c.a, c.b))
    for name in ("pairs_extremes", f"scan_{T + 1}_all_heads"):
        c = lc.scan_case(name) if name.startswith("scan") else lc.pair_case(name)
        with pytest.raises(AssertionError, match="pair_[ab]"):
            lc.check_label_pairs(name, lc.model_label_pairs(c.a, c.b, mutant="unsigned_order")[:3], lc.ref_label_pairs(c.a, c.b))


# ------------------------------------------------------------------------------------------------- merge_*
SMALL_MERGE = lc.merge_small_cases()


@pytest.mark.parametrize("c", SMALL_MERGE, ids=lambda c: c.name)
def test_merge_references_agree_and_fixtures_hold_their_claims(c):
    loop, vec = lc.ref_merge_associate_loop(*c.args()), lc.ref_merge_associate(*c.args())
    lc.check_merge(c.name, vec, loop)
    for key in ("inter", "n_points1", "n_scalars1", "n_scalars2", "common"):
        if key in c.claims:
            assert lc.first_difference(loop[key], np.asarray(c.claims[key], np.int32)) is None, (c.name, key)
    assert loop["inter"][0].sum() == 0 and loop["inter"][:, 0].sum() == 0 and loop["n_points1"][0] == 0
    empty = loop["n_points1"] == 0                                       # no cropped point: nothing of the instance counts
    assert not loop["inter"][empty].any() and not loop["n_scalars1"][empty].any() and not loop["common"][empty].any()


def test_merge_tile_fixtures_walk_one_two_and_three_box_tiles():
    tile = lc.BOX_TILE
    assert lc.MERGE_TILE_N1 == (2, 256, 257, 258, 512, 513, 600) and lc.MERGE_TILE_N2 == (2, 40)
    assert [lc.box_tiles(n) for n in lc.MERGE_TILE_N1] == [1, 1, 1, 2, 2, 2, 3]
    assert lc.box_tiles(tile + 1) * tile == tile and lc.box_tiles(2 * tile + 1) * tile == 2 * tile      # exactly full tiles
    for c in SMALL_MERGE:
        if not c.name.startswith("merge_tile"):
            continue
        assert c.claims["box_tiles"] == lc.box_tiles(c.n1)
        assert c.chunk_xyz.shape[0] % lc.BLOCK != 0
        live = np.flatnonzero(c.claims["n_points1"])
        assert c.claims["inter"][live].sum(1).min() >= 1 and live.max() == c.n1 - 1 - ((c.n1 - 1) % 7 == 3)
        if c.n1 > 3:
            assert (c.claims["n_points1"][1:] == 0).any()                # instances wholly outside the crop cube
        for ids, n in ((c.map_inst, c.n1), (c.chunk_inst, c.n2)):
            assert (ids == 0).any() and (ids < 0).any() and (ids == n).any()
        assert c.claims["inter"][c.n1 - 1].sum() >= 1 or (c.n1 - 1) % 7 == 3   # the last id of the last tile is counted


def test_merge_face_fixtures_sit_on_the_faces():
    for tag, centre in (("exact", lc.CENTER_EXACT), ("rounds", lc.CENTER_ROUNDS)):
        c = next(x for x in SMALL_MERGE if x.name == "merge_face_cube_" + tag)
        cen = np.asarray(centre)
        lo, hi = cen - 20.0, cen + 20.0
        exact = np.array_equal(lo + 20.0, cen) and np.array_equal(hi - 20.0, cen) and all(float(v).is_integer() for v in cen * 4)
        assert exact == (tag == "exact")
        on = ((c.map_xyz == lo) | (c.map_xyz == hi)).sum()
        off = sum(((c.map_xyz == np.nextafter(f, s)).sum()) for f, s in ((lo, -np.inf), (hi, np.inf)))
        inn = sum(((c.map_xyz == np.nextafter(f, s)).sum()) for f, s in ((lo, np.inf), (hi, -np.inf)))
        assert (on, off, inn) == (c.claims["on_face"], c.claims["ulp_outside"], c.claims["ulp_inside"]) == (6, 6, 6)
        assert c.claims["n_points1"].sum() == 12
    c = next(x for x in SMALL_MERGE if x.name == "merge_face_box")
    bl, bh = c.map_xyz.min(0), c.map_xyz.max(0)
    assert ((c.chunk_xyz == bl) | (c.chunk_xyz == bh)).sum() == 6
    assert sum((c.chunk_xyz == np.nextafter(f, s)).sum() for f, s in ((bl, -np.inf), (bh, np.inf))) == 6
    assert c.claims["inter"].sum() == 12


def test_merge_scalar_fixtures():
    by = {c.name: c for c in SMALL_MERGE}
    c = by["merge_scalar_shared_z"]
    r = lc.ref_merge_associate(*c.args())
    assert (c.n1, c.n2) == (301, 41) and c.claims["run"] == 340
    assert r["common"][1:, 1:].min() >= 1 and np.all(c.map_xyz[:, 2] == 0.0) and np.all(c.chunk_xyz[:, 2] == 0.0)
    assert np.signbit(c.chunk_xyz[:, 2]).any() and not np.signbit(c.chunk_xyz[:, 2]).all()
    assert lc.selected_counts(by["merge_scalar_empty_crop"])[0] == 0 and lc.selected_counts(by["merge_scalar_empty_crop"])[1] > 0
    assert lc.selected_counts(by["merge_scalar_all_street"]) == (0, 0)
    r = lc.ref_merge_associate(*by["merge_scalar_all_street"].args())
    assert not any(v.any() for v in r.values())
    r = lc.ref_merge_associate(*by["merge_scalar_empty_crop"].args())
    assert r["n_scalars2"].sum() > 0 and not r["inter"].any() and not r["common"].any() and not r["n_scalars1"].any()


def test_merge_scalar_cross_case_takes_the_recursive_scan():
    c = lc.merge_scalar_cross_case()
    s0, s1 = lc.selected_counts(c)
    ns = 3 * (s0 + s1)
    assert D < ns < lc.K["KM_MAX_SCALARS"] and lc.scan_regime(ns) == "recursive"
    assert lc.scan_regime(c.map_xyz.shape[0]) == "direct" and c.chunk_xyz.shape[0] % lc.BLOCK != 0


def test_merge_mutants_are_caught():
    by = {c.name: c for c in SMALL_MERGE}
    catches = {"cube_face_exclusive": ("merge_face_cube_exact", "merge_face_cube_rounds"),
               "box_face_exclusive": ("merge_face_box", "merge_tile_2_2"),
               "box_tiles_from_id0": (f"merge_tile_{lc.BOX_TILE + 2}_40", "merge_tile_2_2"),
               "signed_zero_two_scalars": ("merge_scalar_signed_zero", "merge_scalar_shared_z"),
               "common_per_occurrence": ("merge_scalar_repeat", "merge_scalar_shared_z")}
    assert set(catches) == set(lc.MERGE_MUTANTS)
    for mutant, names in catches.items():
        for name in names:
            c = by[name]
            with pytest.raises(AssertionError, match=name):
                lc.check_merge(name, lc.ref_merge_associate(*c.args(), mutant=mutant), lc.ref_merge_associate(*c.args()))


def test_merge_scalar_bound_arithmetic():
    """`ai_merge_associate` refuses 3 * (sel0 + sel1) > KM_MAX_SCALARS.  The guard cannot be run at its real size (that
    takes 716 M selected points); this is the arithmetic of the bound only."""
    m = lc.K["KM_MAX_SCALARS"]
    assert m + 1 <= lc.I32_MAX                                # head / pos hold ns + 1 int32 positions, the last the total ns
    legal = 2 ** 29 - 1                                       # the largest n_map and n_chunk the entry point admits
    assert 3 * (legal + legal) > lc.I32_MAX                   # the hazard: legal arguments, ns beyond int32
    top = m // 3                                              # the largest sel0 + sel1 that passes
    assert 3 * top <= m < 3 * (top + 1) and top == 715_827_882
    assert lc.scan_tmp_elems(m) < 2 ** 31


# ------------------------------------------------------------------------------------------------- unique_*, voxel_scan
def test_unique_reference_equals_the_oracle_and_catches_keep_last():
    cases = lc.unique_cases()
    assert {f"unique_len_{n}" for n in (1, T, T + 1)} <= set(cases) and lc.UNIQUE_BIG_LENGTHS == (D, D + 1)
    for name, p in cases.items():
        keep = lc.ref_unique_points(p)
        ep, _ = merge_ref.remove_duplicated_points(p, p)
        assert lc.first_difference(p[keep], ep) is None, name           # by bits: the oracle keeps the first row's sign too
        lc.check_unique(name, keep, keep)
    assert lc.ref_unique_points(cases["unique_identical"]).tolist() == [0]
    assert lc.ref_unique_points(cases["unique_distinct"]).shape[0] == cases["unique_distinct"].shape[0]
    assert lc.ref_unique_points(cases["unique_ends"]).shape[0] == 4999
    assert lc.ref_unique_points(cases["unique_ulp_axis"]).tolist() == [0, 1, 3, 5, 7, 9, 11]
    z = cases["unique_signed_zero"]
    kz = lc.ref_unique_points(z)
    assert kz.tolist() == [0, 2, 4, 6] and np.signbit(z[kz][1, 0]) and np.signbit(z[kz][3]).all()    # the kept row keeps its sign
    assert lc.ref_unique_points(cases["unique_denormal_negative"]).tolist() == [0, 2, 3, 5, 6, 7, 9]
    for name in ("unique_signed_zero", "unique_ends"):
        with pytest.raises(AssertionError, match=name):
            lc.check_unique(name, lc.ref_unique_points(cases[name], keep_last=True), lc.ref_unique_points(cases[name]))
    with pytest.raises(AssertionError, match="ascending"):
        lc.check_unique("order", np.array([1, 0]), np.array([0, 1]))
    p = lc.unique_len_case(200_000)
    assert 0 < lc.ref_unique_points(p).shape[0] < p.shape[0]


def test_packed_voxel_reference_equals_prep_ref():
    p = lc.voxel_scan_points(30_000, seed=4)
    got, gtr = lc.ref_voxel_down_sample_packed(p, lc.VOXEL_SIZE)
    ref, rtr = prep_ref.voxel_down_sample(p, lc.VOXEL_SIZE)
    assert got.tobytes() == ref.tobytes() and np.array_equal(gtr, rtr)
    per_voxel = np.bincount(gtr)
    assert np.mean((per_voxel >= 1) & (per_voxel <= 3)) > 0.8
    assert lc.scan_regime(D + 1) == "recursive"
    rng = np.random.default_rng(0)
    q = rng.normal(0, 3, (5000, 3))
    assert lc.ref_voxel_down_sample_packed(q, 0.35)[0].tobytes() == prep_ref.voxel_down_sample(q, 0.35)[0].tobytes()


# ------------------------------------------------------------------------------------------------- merge_iou_*
def _host_merge_on_references(monkeypatch, chunks):
    """labels_api's host association fed by the NumPy references in place of the two device calls."""
    from autoinst_amd import labels_api
    seen = []

    def assoc(mp, mi, cp, ci, center, n1, n2, side_length=40.0, **_):
        seen.append((n1, n2))
        return lc.ref_merge_associate(mp, mi, cp, ci, center, side_length, n1, n2)

    monkeypatch.setattr(labels_api, "merge_associate", assoc)
    monkeypatch.setattr(labels_api, "unique_points", lambda p, **_: lc.ref_unique_points(p))
    return labels_api.merge_chunks_unite_instances2(chunks), seen


def _has_colour(C, col):
    return bool(np.any(np.all(C == col, axis=1)))


def test_merge_iou_fixtures_through_the_host_association(monkeypatch):
    assert 1.0 / 100.0 == 0.01 and not (1.0 / 100.0 > 0.01) and 1.0 / 99.0 > 0.01
    cases = lc.merge_iou_cases()
    out = {}
    for name, (chunks, claims) in cases.items():
        (P, C), seen = _host_merge_on_references(monkeypatch, chunks)
        eP, eC = merge_ref.merge_chunks_unite_instances2(chunks)
        lc.check_points(name, P, eP)
        lc.check_points(name + " colours", C, eC)
        out[name] = (P, C, seen, claims)
    for name, merged in (("merge_iou_exactly_0.01", False), ("merge_iou_above_0.01", True)):
        P, C, seen, claims = out[name]
        chunks = cases[name][0]
        from autoinst_amd import labels_api
        t1, i1 = labels_api._color_ids(chunks[0][1])
        t2, i2 = labels_api._color_ids(chunks[1][1])
        r = lc.ref_merge_associate(chunks[0][0], i1, chunks[1][0], i2, chunks[1][0].mean(0), 40.0, t1.shape[0], t2.shape[0])
        assert r["inter"][1, 1] == 1 and r["n_scalars1"][1] + r["n_scalars2"][1] - r["common"][1, 1] == claims["union"]
        assert _has_colour(C, claims["color_c"]) == (not merged)
        assert int(np.all(C == claims["color_a"], axis=1).sum()) == 20 + (claims["n_c"] if merged else 0)
    P, C, seen, claims = out["merge_iou_tie"]
    assert not _has_colour(C, claims["color_c"])
    assert int(np.all(C == claims["color_a"], axis=1).sum()) == 7 and int(np.all(C == claims["color_b"], axis=1).sum()) == 5
    P, C, seen, claims = out["merge_iou_many_instances"]
    assert len(seen) == 2 and seen[1][0] > lc.BOX_TILE + 1 and lc.box_tiles(seen[1][0]) == 2
    assert np.unique(C, axis=0).shape[0] == claims["clusters"] + 1            # every cluster one colour, plus the street


def test_merge_reference_through_the_host_association_on_random_maps(monkeypatch):
    for i, chunks in enumerate(lc.random_small_maps()):
        (P, C), _ = _host_merge_on_references(monkeypatch, chunks)
        eP, eC = merge_ref.merge_chunks_unite_instances2(chunks)
        lc.check_points(f"random map {i}", P, eP)
        lc.check_points(f"random map {i} colours", C, eC)


def test_first_difference_names_the_index():
    assert lc.first_difference(np.arange(5), np.arange(5)) is None
    assert "first at 3" in lc.first_difference(np.array([0, 1, 2, 9, 9]), np.arange(5))
    assert "shape" in lc.first_difference(np.arange(4), np.arange(5))
    assert lc.first_difference(np.array([0.0]), np.array([-0.0])) is not None      # floats by their bits
