"""CPU: every fixture of tests/finish_cases.py sits in the regime its name claims (tile counts, k per chunk and template
instance, growth steps, the sums of cells and rows, lap counts, planted non-inliers), the host model of `ai_chunk_finish` equals
the grid-free truth on all of them, every deliberately wrong rule is rejected by the fixtures that claim to reject it (and the
one rule that must change nothing changes nothing), and no fixture leaves the GPU test anything to exclude: no fine point between
two majors and no average within the statistics bound of the threshold, but in the chunks built that way.  No GPU, no library."""
import numpy as np
import pytest

import finish_cases as fc
import finish_ref
import points_cases as pts
import prep_cases as pc


def _table(name):
    return fc.case(name).model()["table"]


# ------------------------------------------------------------------------------------------------- constants
def test_constants_are_the_ones_the_fixtures_were_built_on():
    assert (fc.BLOCK, fc.BB, fc.K["RED_BLOCKS"], fc.NSTAT, fc.LAP) == (256, 8, 256, 6, 65536)
    assert fc.KNN_LENGTHS == (20, 32, 64) and fc.MAX_CHUNKS == 65535 and fc.K["MAX_ROWS"] == 1 << 30
    assert (fc.K["CAP_TOTAL"], fc.K["CAP_FLOOR"], fc.K["NN1_CELL"], fc.K["GROW"]) == (1 << 27, 64.0, 0.5, 1.5)
    assert fc.K["NN1_STOP"] == fc.K["KNN_STOP"] == (8.0, 4.0) and fc.K["EXTENT_LIMIT"] == 1e15


def test_the_floor_of_the_cell_cap_cannot_be_reached():
    share = float(fc.K["CAP_TOTAL"]) / float(fc.MAX_CHUNKS)
    assert share > fc.K["CAP_FLOOR"], (
        f"the floor {fc.K['CAP_FLOOR']:.0f} of cell_cap is dead code: with n_chunks <= {fc.MAX_CHUNKS} a chunk's share of "
        f"{fc.K['CAP_TOTAL']} cells is at least {share:.1f}, so max({fc.K['CAP_FLOOR']:.0f}, share) is always the share")
    assert share > 2048.0
    for n in (1, 2, 4096, fc.MAX_CHUNKS):
        assert fc.cell_cap(n) == float(fc.K["CAP_TOTAL"]) / n
    assert fc.cell_cap(0) == float(fc.K["CAP_TOTAL"]) and fc.cell_cap(4096, "cap_of_one_call") == float(fc.K["CAP_TOTAL"])


def test_tile_chunk_is_the_largest_chunk_that_starts_at_or_before_the_block():
    rng = np.random.default_rng(1)
    for _ in range(200):
        nch = int(rng.integers(1, 40))
        sizes = rng.choice(fc.TILE_SIZES, nch) * (rng.random(nch) < 0.6)
        t = fc.tiles_of(sizes)
        if t[-1] == 0:
            continue
        blocks = np.arange(t[-1])
        c = fc.tile_chunk(t, nch, blocks)
        np.testing.assert_array_equal(c, np.searchsorted(t[:nch], blocks, side="right") - 1)
        assert (sizes[c] > 0).all() and ((blocks - t[c]) * fc.BLOCK < sizes[c]).all()
        assert fc.covered_rows(sizes).all()


# ------------------------------------------------------------------------------------------------- regimes
def test_tiles_sits_on_the_block_boundaries_with_runs_of_empty_chunks():
    c = fc.case("tiles")
    sizes = c.claims["sizes"]
    assert c.n_chunks == 24 and fc.TILE_SIZES == (0, 1, 255, 256, 257, 511, 512, 513)
    for kind, runs in fc.TILE_EMPTY.items():
        s = np.array(sizes[kind])
        assert set(s) == set(fc.TILE_SIZES), kind
        assert {len(r) for r in runs} <= {2, 3}
        assert runs[0][0] == 0 and runs[-1][-1] == c.n_chunks - 1 and 0 < runs[1][0] and runs[1][-1] < c.n_chunks - 1
        for run in runs:
            assert not s[list(run)].any(), (kind, run)
            if run[-1] + 1 < c.n_chunks:
                assert s[run[-1] + 1] in (fc.BLOCK - 1, fc.BLOCK, fc.BLOCK + 1), (kind, run)
    followers = [sizes[kind][run[-1] + 1] for kind, runs in fc.TILE_EMPTY.items() for run in runs if run[-1] + 1 < c.n_chunks]
    assert set(followers) == {fc.BLOCK - 1, fc.BLOCK, fc.BLOCK + 1}
    assert len({fc.TILE_EMPTY[k][1] for k in fc.TILE_EMPTY}) == 3, "the middle runs are elsewhere for every cloud"
    for place in range(3):                              # front, middle, end: a run of two and a run of three
        assert {len(fc.TILE_EMPTY[k][place]) for k in fc.TILE_EMPTY} == {2, 3}
    assert len({tuple(sizes[k]) for k in sizes}) == 3
    f, m = np.array(sizes["fine"]), np.array(sizes["major"])
    assert not (f[m == 0]).any()
    t = c.model()["table"]
    assert t["tiles"] == tuple(int(sum(-(-n // fc.BLOCK) for n in sizes[k])) for k in ("fine", "major", "ground"))
    for kind in sizes:      # the wrong tile rules leave rows untaken, the right one none
        assert fc.covered_rows(sizes[kind]).all()
        assert not fc.covered_rows(sizes[kind], "tile_floor").all() and not fc.covered_rows(sizes[kind], "tile_chunk_first").all()


@pytest.mark.parametrize("nb", fc.MIXED_NB + (100,))
def test_mixed_k_has_a_k_per_chunk_under_the_longest_instance(nb):
    c = fc.case(f"mixed_k_nb{nb}")
    t = c.model()["table"]
    sizes = c.claims["sizes"]
    assert t["k"].tolist() == [min(nb, n) for n in sizes] == list(c.claims["k"])
    assert t["k_max"] == max(c.claims["k"]) and t["instance"] == c.claims["instance"] == pc.knn_instance(t["k_max"])
    if nb <= 64:
        assert sizes == tuple(n for n in (1, 2, 12, nb - 1, nb, nb + 1, 300) if n >= 1) and t["k_max"] == nb
        if nb > 2:
            assert len(set(c.claims["k"])) >= 4                                   # 1, 2, 12 / nb - 1, nb
    else:
        assert max(sizes) == 64 and t["k"].tolist() == list(sizes) and t["instance"] == 64
    if nb > 2:          # at least one chunk alone would get a shorter instance than the batch gives it
        alone = [pc.knn_instance(k) for k in c.claims["k"]]
        assert min(alone) == 20 and (min(alone) < t["instance"] or nb <= 20)


def test_instances_of_the_mixed_batches_cover_every_switch():
    got = {nb: fc.case(f"mixed_k_nb{nb}").claims["instance"] for nb in fc.MIXED_NB + (100,)}
    assert got == {1: 20, 2: 20, 19: 20, 20: 20, 21: 32, 32: 32, 33: 64, 63: 64, 64: 64, 100: 64}


def test_many_chunks_grown_takes_zero_one_and_two_growth_steps():
    c = fc.case("many_chunks_grown")
    t = c.model()["table"]
    assert c.n_chunks == 4096 and c.occupied == list(fc.GROWN_AT) and t["cap"] == 32768.0
    steps = tuple(int(t["psteps"][a]) for a in fc.GROWN_AT)
    assert steps == c.claims["steps"] == (0, 1, 2, 2)
    one = c.model("cap_of_one_call")["table"]
    assert not one["psteps"].any() and (one["pcell"][list(fc.GROWN_AT)] == 0.5).all()
    for a in fc.GROWN_AT:
        n = t["pn"][a]
        assert n.prod() <= t["cap"] and t["pcell"][a] == 0.5 * 1.5 ** t["psteps"][a]
        if t["psteps"][a]:                                                       # the step before was too large: the loop had to run
            smaller = np.floor(np.ptp(c.major[a], axis=0) / (t["pcell"][a] / 1.5)) + 1
            assert smaller.prod() > t["cap"]
        # fine points outside the major box: their cells are clamped, on every side
        g = pts.Grid(c.major[a].min(axis=0)[None], c.major[a].max(axis=0)[None], np.array([t["pcell"][a]]), 0.5, n[None])
        raw = pts.cells_of(g, c.fine[a][None], clamp=False)[0]
        assert (raw < 0).any() and (raw > n - 1).any() and ((raw >= 0) & (raw <= n - 1)).all(axis=1).sum() >= 150
        out = np.maximum(c.major[a].min(axis=0) - c.fine[a], c.fine[a] - c.major[a].max(axis=0)).max()
        assert 50.0 < out <= 100.0


def test_chunk_limit_is_the_largest_call():
    c = fc.case("chunk_limit")
    assert c.n_chunks == fc.MAX_CHUNKS == 65535 and c.occupied == [0, 30000, 65534]
    t = c.model()["table"]
    assert t["cap"] == float(1 << 27) / 65535 and not t["psteps"].any()


@pytest.mark.parametrize("plus", (0, 1))
def test_key_bits_puts_both_sums_on_a_power_of_two(plus):
    c = fc.case(f"key_bits_plus{plus}")
    t = c.model()["table"]
    for total, bits in ((t["ncell"], t["mbits"]), (t["nrow"], t["gbits"] - 32)):
        b = pc.bits_for(total - plus)
        assert total - plus == 1 << b and b >= 9, (total, plus)               # 2^b, or 2^b + 1
        assert bits == pc.bits_for(total) == b + plus                           # 2^b + 1 entries need one bit more
    last_m = max(a for a in range(c.n_chunks) if len(c.major[a]))
    last_g = max(a for a in range(c.n_chunks) if len(c.ground[a]))
    moff, goff = np.cumsum([0] + [len(m) for m in c.major]), np.cumsum([0] + [len(g) for g in c.ground])
    assert int(t["mkey"][moff[last_m]:moff[last_m + 1]].max()) == t["ncell"] - 1, "the last chunk's last cell is occupied"
    assert int(t["gkey"][goff[last_g]:goff[last_g + 1]].max() >> np.uint64(32)) == t["nrow"] - 1, "the last chunk's last row is occupied"
    # one bit less moves exactly the keys with the top bit: they exist
    assert (t["mkey"] >> np.uint64(t["mbits"] - 1)).any() and ((t["gkey"] >> np.uint64(t["gbits"] - 1)) & np.uint64(1)).any()
    # keys that differ in the top bit alone lie in ONE major chunk, more than once per cell, their rows interleaved
    lo, hi = int(t["cellbase"][last_m]), int(t["cellbase"][last_m + 1])
    own = t["mkey"][moff[last_m]:moff[last_m + 1]].astype(np.int64)
    top = 1 << (t["mbits"] - 1)
    pairs = np.intersect1d(own[own >= top] - top, own[own < top])
    assert hi - lo > top // 2 and pairs.size >= 1 and (pairs >= lo).all(), "the last major chunk holds both cells of a pair"
    x = int(pairs[0])
    a, b = np.flatnonzero(own == x), np.flatnonzero(own == x + top)
    assert a.size + b.size >= 3 and a.min() < b.max() and b.min() < a.max(), "their rows interleave"
    short = c.model("key_bits_short")
    assert short["table"]["runs_whole"] == (False, False), "one bit short, cells and rows fall into pieces"
    bad = fc.differences(short, c.truth, c.truth["per_chunk"])
    assert {"fine_nn", "fine_dist", "fine_label", "ground_avg"} <= set(bad), bad


@pytest.mark.parametrize("name", [n for n in fc.CASE_NAMES if n.startswith("ring_stop")])
def test_ring_stop_batches_hold_every_ring_stop_cloud_beside_a_neighbour(name):
    c = fc.case(name)
    k = c.nb
    knn = [x for x in pc.ring_stop_cases() if x.nb == k]
    names = [n for n in c.claims["names"] if n is not None]
    assert [n[0] for n in names if n[0]] == [x.name for x in knn] and len(knn) in (18, 21)
    got = {n[1] for k2 in pc.RING_KS for n in fc.case(f"ring_stop_k{k2}").claims["names"] if n is not None and n[1]}
    assert got == {x.name for x in pts.ring_stop_cases()}
    occ = c.occupied
    assert len(occ) % 2 == 0
    for a, b in zip(occ[0::2], occ[1::2]):                  # the neighbour lies over the same box, with other points
        for kind in (c.major, c.ground):
            if len(kind[a]):
                assert len(kind[b]) and (kind[b].min(axis=0) >= kind[a].min(axis=0) - 1e-9).all() and \
                    (kind[b].max(axis=0) <= np.maximum(kind[a].max(axis=0), kind[a].min(axis=0) + 0.5) + 1e-9).all()
    t = c.model()["table"]
    if name.endswith("_grown"):
        assert c.n_chunks == 4096 and t["cap"] == 32768.0 and t["psteps"].max() >= 1
        plain = fc.case(name[:-6])
        assert (t["psteps"][occ] >= plain.model()["table"]["psteps"][plain.occupied]).all()
        assert (t["psteps"][occ] > plain.model()["table"]["psteps"][plain.occupied]).any()
    else:
        assert c.n_chunks == len(occ)
        # alone, the old stop rule gets these very chunks wrong: the clouds are the proven fixtures, unchanged
        for a, n in zip(occ[0::2], names):
            if n[0]:
                assert c.ground[a] is next(x for x in knn if x.name == n[0]).points


def test_degenerate_has_chunks_without_inliers_and_averages_on_the_threshold():
    c = fc.case("degenerate")
    tr = c.truth
    st = tr["ground_stats"]
    for a in c.claims["no_inlier"]:
        assert st[a, 3] == 0 and np.isnan(st[a, 4]) and np.isnan(st[a, 5]) and tr["keep_off"][a + 1] == tr["keep_off"][a]
    for a in c.on_threshold:                               # every average equals the threshold: std is exactly 0
        avg = tr["per_chunk"][a]["avg"]
        assert (avg == avg[0]).all() and st[a, 1] == 0.0 and st[a, 2] == avg[0] and avg[0] > 0
    for a, n in c.claims["zeros"].items():
        assert (tr["per_chunk"][a]["avg"] == 0).sum() == n
    for a in (4, 5, 6, 7):
        assert np.ptp(c.ground[a], axis=0).min() == 0.0 and st[a, 3] > 100      # lines and a plane: a thin axis, and inliers
    assert [len(g) for g in c.ground] == [8, 239, 2, 30, 200, 200, 200, 300]


def test_f4_lap_plants_non_inliers_in_front_of_the_lap_boundary():
    c = fc.case("f4_lap")
    assert c.claims["sizes"] == (65535, 65536, 65537, 65537, 65793) == tuple(len(g) for g in c.ground)
    tr = c.truth
    assert [-(-n // fc.LAP) for n in c.claims["sizes"]] == [1, 1, 2, 2, 2], "laps of kf_zpartial's thread 0 of block 0"
    assert c.model()["table"]["tiles"] == (0, 0, 256 + 256 + 257 + 257 + 258)
    for a in range(5):
        copies, far = c.claims["planted"][a]
        inl, avg = tr["per_chunk"][a]["inliers"], tr["per_chunk"][a]["avg"]
        assert (avg[copies] == 0).all() and not inl[copies].any() and not inl[far].any()
        assert (avg[far] > tr["ground_stats"][a, 2]).all()
        assert far[:19].max() < fc.LAP and copies.size == far.size == 20
        assert copies.min() > fc.LAP if a == 4 else copies.max() < fc.LAP
        assert inl[far[0]:fc.LAP].sum() > 60000, "inliers of the first lap behind the first planted rows"
        assert (~inl).sum() >= 40 and inl[:fc.LAP].sum() > 65000
        z = c.ground[a][:, 2]
        assert (z * 1024 != np.round(z * 1024)).mean() > 0.99, "z is off the dyadic lattice"
        right = finish_ref.f4_sum(z, inl)
        by_rank = finish_ref.f4_sum(z[inl], np.ones(int(inl.sum()), bool))
        assert np.float64(right) / inl.sum() != np.float64(by_rank) / inl.sum(), f"chunk {a}: slot by rank gives the same mean_z"
        assert c.model("slot_by_rank")["ground_stats"][a, 4] != tr["ground_stats"][a, 4]
        assert c.model()["ground_stats"][a, 4] == tr["ground_stats"][a, 4]
    far3 = c.claims["planted"][3][1]
    assert far3.max() == fc.LAP and tr["per_chunk"][2]["inliers"][fc.LAP], "second lap: a non-inlier in one chunk, an inlier in the other"
    inl4 = tr["per_chunk"][4]["inliers"][fc.LAP:]
    assert inl4.size == 257 and inl4.sum() >= 230 and (~inl4).sum() >= 20, "257 slots of the second lap, non-inliers among them"


def test_strict_z_has_a_limit_per_chunk_with_points_on_it():
    c = fc.case("strict_z")
    tr = c.truth
    st = tr["ground_stats"]
    assert tuple(st[:, 5]) == c.claims["limits"] and (st[:, 3] == 256).all()
    goff = np.cumsum([0] + [len(g) for g in c.ground])
    for a in range(3):
        z = c.ground[a][:, 2]
        # chunk 1 has a point one ulp below its limit; 4 m and 8.5 m up that ulp is rounded away and the point is ON the limit
        assert (z == st[a, 5]).sum() == (128, 127, 128)[a]
        assert (z < st[a, 5]).sum() == c.claims["kept"][a] == tr["keep_off"][a + 1] - tr["keep_off"][a]
    keep1 = tr["ground_keep"][tr["keep_off"][1]:tr["keep_off"][2]]
    assert 16 in keep1 and 1 not in keep1 and goff[-1] == 768
    assert c.ground[1][16, 2] == np.nextafter(0.125, 0.0) and c.ground[0][16, 2] == 4.125


def test_ties_go_to_the_smaller_index():
    c = fc.case("ties")
    tr = c.truth
    assert tr["per_chunk"][1]["tied"] == c.claims["tied"] == 5
    assert tr["fine_nn"][50:56].tolist() == [0, 0, 0, 2, 1, 1]


def test_refusal_cases_sit_where_their_names_say():
    cases = fc.refusal_cases()
    assert len(cases) == 3 * 5 + 4
    for name, fine, major, labels, ground, cloud, chunk in cases:
        parts = {"fine": fine, "major": major, "ground": ground}[cloud]
        bad = [(a, np.argwhere(~np.isfinite(p))) for a, p in enumerate(parts) if not np.isfinite(p).all()]
        if name.startswith("extent"):
            assert not bad and max(np.ptp(p, axis=0).max() for p in parts if len(p)) >= 1e15 and np.ptp(parts[chunk], axis=0).max() >= 1e15
            continue
        assert len(bad) == 1 and bad[0][0] == chunk and bad[0][1].shape[0] == 1, name
        row = int(bad[0][1][0, 0])
        if "last_row_of_last_chunk" in name:
            assert chunk == len(parts) - 1 == 4 and row == len(parts[chunk]) - 1
        if "row_2049" in name:
            assert row == 2049 == fc.BB * fc.BLOCK + 1 and len(parts[chunk]) == 4100      # the second trip of block 0 of kf_bounds
        if "row_4097" in name:
            assert row == 4097 == 2 * fc.BB * fc.BLOCK + 1
        if "middle" in name:
            assert 0 < chunk < len(parts) - 1 and cloud == "major"
        for other in ("fine", "major", "ground"):
            if other != cloud:
                assert all(np.isfinite(p).all() for p in {"fine": fine, "major": major, "ground": ground}[other])


# ------------------------------------------------------------------------------------------------- model, truth, mutants
@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_model_equals_the_truth(name):
    c = fc.case(name)
    tr = c.truth
    assert fc.differences(c.model(), tr, tr["per_chunk"]) == []
    assert c.model()["table"]["runs_whole"] == (True, True)


@pytest.mark.parametrize("name", fc.CASE_NAMES)
def test_nothing_is_left_to_exclude(name):
    """No fine point between two majors but in the tie chunks; no average within `stats_bound` of the threshold but in the
    chunks built on it; mean_z and z_limit are predicted bit for bit, so z needs no margin."""
    c = fc.case(name)
    for a, info in c.truth["per_chunk"].items():
        if a not in c.tie_chunks:
            assert info.get("tied", 0) == 0, (name, a)
        else:
            assert info["tied"] > 0, (name, a)
        if a not in c.on_threshold and "near" in info:
            assert info["near"].size == 0, (name, a, info["near"])
    for a in c.on_threshold:
        assert c.truth["per_chunk"][a]["near"].size > 0, (name, a)


def test_every_wrong_rule_is_rejected_by_the_fixtures_that_claim_it(capsys):
    by = {m: [] for m in fc.MUTANTS}
    for name in fc.CASE_NAMES:
        c = fc.case(name)
        tr = c.truth
        for m in c.rejects:
            bad = fc.differences(c.model(m), tr, tr["per_chunk"])
            assert bad, f"{name} does not tell {m} from the truth"
            by[m].append(f"{name} ({', '.join(sorted({b.split('[')[0] for b in bad}))})")
    with capsys.disabled():
        print()
        for m in fc.MUTANTS:
            print(f"  {m}: {'; '.join(by[m]) if by[m] else 'changes no result (asserted)'}")
    for m in fc.MUTANTS:
        assert bool(by[m]) != (m in fc.NO_OP_MUTANTS), m


def test_a_chunk_with_the_whole_cap_changes_no_result():
    """`cap_of_one_call`: grids differ (the growth steps vanish), the outputs do not."""
    for name in ("many_chunks_grown", "ring_stop_k2_grown", "ring_stop_k20_grown", "chunk_limit"):
        c = fc.case(name)
        one = c.model("cap_of_one_call")
        assert fc.differences(one, c.truth, c.truth["per_chunk"]) == [], name
        for key in fc.KEYS:
            assert fc.same_bits(one[key], c.model()[key]), (name, key)
        if name != "chunk_limit":
            assert (one["table"]["pcell"] != c.model()["table"]["pcell"]).any(), name


def test_f4_is_the_truth_only_in_its_own_order():
    """`finish_ref.f4_sum` against `math.fsum` on the f4_lap chunks: within the summation bound, and not equal to a plain
    left-to-right sum (so the bits the GPU test compares do depend on the order)."""
    import math
    c = fc.case("f4_lap")
    differs = 0
    for a in range(len(c.ground)):
        inl = c.truth["per_chunk"][a]["inliers"]
        z = c.ground[a][:, 2]
        s = finish_ref.f4_sum(z, inl)
        exact = math.fsum(z[inl])
        assert abs(s - exact) <= (pc.reduction_depth(z.size) + 1) * pc.U * math.fsum(np.abs(z[inl])) * 1.01
        differs += s != float(np.cumsum(z[inl])[-1])
    assert differs >= 1
