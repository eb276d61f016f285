"""CPU proofs for tests/camera_cases.py: every fixture sits in the regime its name claims, the model of the device's search
(`visible_model`) equals rule 2 over all pairs on every fixture, and each of nine deliberately wrong searches is rejected by the
fixtures named for it.  No GPU, no library.  Run with ``-s`` to see every claim's figures and the variant -> fixture table."""
import math

import numpy as np
import pytest

import camera_cases as cc
import camera_ref
import points_cases as pc

MAXD = cc.MAXD


@pytest.fixture(scope="module")
def built():
    return {name: build() for name, build in cc.cases().items()}


@pytest.fixture(scope="module")
def seen(built):
    return {name: cc.seen_brute(c) for name, c in built.items()}


# ------------------------------------------------------------------------------------------------- constants
def test_constants_are_read_from_the_sources():
    assert cc.K == dict(MAX_VIEWS=64, LANES=16, WAVE=64, AI_BLOCK=256, NARROW=128, WIDE=384, CELL_CAP=1 << 27, GROW=1.5, SINGULAR=1e-6,
                        SLACK_REL=1e-6, SLACK_ABS=1e-9)
    assert cc.VIEW_COUNTS == (1, 31, 32, 33, 63, 64) and cc.RUN_LENGTHS == (15, 16, 17, 32, 33)
    assert cc.QUERY_COUNTS == (1, 3, 4, 5, 15, 16, 17, 65)
    assert cc.WIDTHS == (1, 63, 64, 65, 127, 128, 129, 383, 384, 385, 768, 769)


# ------------------------------------------------------------------------------------------------- the model is the truth
def test_the_shipped_search_equals_rule_2_over_all_pairs(built, seen):
    for name, c in built.items():
        if c.refused:
            with pytest.raises(ValueError, match="nearly"):
                cc.visible_model(c)
            continue
        assert np.array_equal(cc.visible_model(c), seen[name]), f"{name}: the search of kc_visible misses rule 2 (a design bug)"
        # what the device's outputs show of it: a seen pair is projected (the fixtures keep their points inside the images)
        assert np.array_equal(c.truth["pixels"][:, :, 0] >= 0, seen[name]), f"{name}: a seen pair falls outside its image"


def test_every_wrong_search_is_rejected_by_its_fixtures(built, seen):
    table = {}
    for variant in cc.VARIANTS:
        table[variant] = [name for name, c in built.items()
                          if not c.refused and not np.array_equal(cc.visible_model(c, variant), seen[name])]
        print(f"{variant:15s} rejected by {', '.join(table[variant])}")
    live = [name for name, c in built.items() if not c.refused]
    for variant, names in cc.REJECTED_BY.items():
        assert set(names) <= set(table[variant]), f"{variant}: accepted by {sorted(set(names) - set(table[variant]))}"
        assert set(table[variant]) != set(live)
    assert set(cc.REJECTED_BY) == set(cc.VARIANTS) and all(table[v] for v in cc.VARIANTS), "a wrong search is accepted everywhere"
    # and where a wrong search must NOT show: the faults are the ones the names say
    assert not {"views_1", "views_31", "views_32"} & set(table["mask32"])
    assert set(table["all_views_zero"]) == {"views_64", "views_64_empty"}
    assert set(table["first16"]) == {"cell_runs"} and set(table["no_slack"]) == {"boundary"}
    assert not [n for n in table["plain_radius"] if n not in cc.AFFINE_CASES and n != "near_singular_above"]


# ------------------------------------------------------------------------------------------------- views_N
@pytest.mark.parametrize("empty", [False, True])
@pytest.mark.parametrize("V", cc.VIEW_COUNTS)
def test_view_count_fixtures(V, empty, built, seen):
    c = built[f"views_{V}" + ("_empty" if empty else "")]
    s, cl = seen[c.name], c.claims
    assert c.n_views == V and c.sam_images.shape[0] == V and c.feature_maps.shape[0] == V
    hollow, live = cl["hollow"], cl["live"]
    assert hollow == (sorted({0, V // 2, V - 1}) if empty else []) and all(len(c.vis[v]) == 0 for v in hollow)
    assert not s[:, hollow].any()
    if not live:
        assert not s.any()
        return
    first, last = cl["first"], cl["last"]
    only = lambda rows, v: all(s[i].sum() == 1 and s[i, v] for i in rows)
    assert only(range(0, 4), last) and only(range(4, 8), first), "queries seen by the last / the first view alone"
    assert s[8:12][:, live].all() and not s[12:16].any(), "queries seen by every view, and by none"
    assert only(range(16, 20), cl["mid"]) or V == 1
    assert len({tuple(v.tolist()) for v in c.vis if len(v)}) == len(live) or V <= 2, "every view has its own visible set"
    # lane V - 1: a pixel, a label and a feature row of the last view are part of the truth
    t = c.truth
    shown = last if not empty else V - 2
    assert (t["pixels"][:, shown, 0] >= 0).sum() >= 4 and (t["sam"][:, shown] > 0).any() and t["dino_views"].max() >= min(len(live), 2)
    if V > 2:
        assert len({tuple(t["pixels"][8, v]) for v in live}) > 1, "the views have their own pixels"
    print(f"{c.name}: {int(s.sum())} seen pairs, hollow views {hollow}, most views on one point {int(s.sum(axis=1).max())}")


# ------------------------------------------------------------------------------------------------- scaled, sheared, singular
def _check_pairs(c, s):
    for p in c.claims["pairs"]:
        T = c.T[p["view"]]
        a, b = camera_ref.transform(c.points[p["query"]], T), camera_ref.transform(c.cloud[p["point"]], T)
        d = float(camera_ref.rule_dist(a, b)[0])
        want = {"below": np.nextafter(MAXD, 0.0), "at": MAXD, "above": np.nextafter(MAXD, np.inf), "at_sq_below": MAXD}.get(p["kind"])
        if want is not None:
            assert d == want, (c.name, p)
        assert s[p["query"], p["view"]] == (p["kind"] in ("below", "pcd_above")), (c.name, p)


@pytest.mark.parametrize("name", sorted(cc.AFFINE_CASES))
def test_affine_fixtures(name, built, seen):
    c = built[name]
    _check_pairs(c, seen[name])
    sig = [cc.sigma_min_bound(T) for T in c.T]
    true = [float(np.linalg.svd(T[:3, :3], compute_uv=False)[-1]) for T in c.T]
    assert all(0 < b <= t * (1 + 1e-12) for b, t in zip(sig, true)), "the bound is a lower bound of the smallest singular value"
    assert len({round(b, 6) for b in sig}) == len(sig), "the views of one call have different sigma"
    plain = MAXD * (1 + cc.K["SLACK_REL"]) + cc.K["SLACK_ABS"]
    beyond = [p for p in c.claims["pairs"] if p["kind"] == "below" and p["pcd_dist"] > plain]
    assert beyond, "an accepted pair lies beyond the radius of a rotation in the pcd frame"
    assert max(p["pcd_dist"] for p in beyond) <= cc.search_radius(c)
    lost = cc.visible_model(c, "plain_radius")
    assert any(not lost[p["query"], p["view"]] for p in beyond), "the plain radius loses it"
    print(f"{name}: sigma bounds {[f'{b:.4g}' for b in sig]} (true {[f'{t:.4g}' for t in true]}), radius {cc.search_radius(c):.4g} m, "
          f"{len(beyond)} accepted pairs beyond {plain:.9f} m, the farthest at {max(p['pcd_dist'] for p in beyond):.4g} m")


def test_the_shear_takes_its_bound_from_the_inverse(built):
    c = built["sheared"]
    R = c.T[0][:3, :3]
    assert np.linalg.norm(R.T @ R - np.eye(3)) >= 1.0
    assert cc.sigma_min_bound(c.T[0]) == pytest.approx(1.0 / np.linalg.norm(np.linalg.inv(R)), rel=1e-12)
    rot = cc.sigma_min_bound(c.T[1])
    assert 1.0 - 1e-7 < rot <= 1.0, "tight for a rotation: sqrt(1 - ||R^T R - I||)"


def test_boundary_fixture(built, seen):
    c = built["boundary"]
    _check_pairs(c, seen["boundary"])
    kinds = {p["kind"] for p in c.claims["pairs"]}
    assert kinds == set(cc.PAIR_KINDS) | {"pcd_above"}
    above = [p for p in c.claims["pairs"] if p["kind"] == "pcd_above"]
    assert len(above) == 4 and all(MAXD < p["pcd_dist"] < MAXD * (1 + 2e-12) for p in above)
    sq = [p for p in c.claims["pairs"] if p["kind"] == "at_sq_below"]
    assert sq and not any(seen["boundary"][p["query"], p["view"]] for p in sq)
    assert all(cc.visible_model(c, "squared")[p["query"], p["view"]] for p in sq), "the square is below max_dist * max_dist there"


def test_near_singular_fixtures(built, seen):
    up, down = built["near_singular_above"], built["near_singular_below"]
    assert cc.sigma_min_bound(up.T[0]) == pytest.approx(cc.SINGULAR * 1.001, rel=1e-9) and not up.refused
    assert cc.sigma_min_bound(down.T[0]) == pytest.approx(cc.SINGULAR * 0.999, rel=1e-9) and down.refused
    assert 1.7e5 < cc.search_radius(up) < 1.8e5 and pc.grid_of(up.cloud, cc.search_radius(up)).ncell[0] == 1
    assert seen["near_singular_above"][:, 0].all() and 0 < seen["near_singular_above"][:, 1].sum() < 21
    with pytest.raises(ValueError, match=cc.REFUSAL.replace("(", r"\(").replace(")", r"\)")):
        cc.search_radius(down)


# ------------------------------------------------------------------------------------------------- the walk
def test_cell_runs_fixture(built, seen):
    c = built["cell_runs"]
    g = pc.grid_of(c.cloud, cc.search_radius(c))
    assert g.cell[0] == c.claims["cell"] and not g.grown[0]
    sc, qc = pc.cells_of(g, c.cloud[None])[0], pc.cells_of(g, c.points[None])[0]
    s = seen["cell_runs"]
    for run in c.claims["runs"]:
        L, i, members = run["L"], run["query"], run["members"]
        assert qc[i].tolist() == run["home"]
        in_last = np.flatnonzero((sc == qc[i] + 1).all(axis=1))          # the (+1, +1, +1) neighbour: the 27th cell of the walk
        assert in_last.tolist() == members and len(members) == L, "exactly L points, in index order (the sort is stable)"
        finder = members[-1]
        assert [p for p in c.vis[1] if np.abs(sc[p] - qc[i]).max() <= 1] == [finder], "one point of view 1's set in the ring: the last"
        assert (L - 1) % cc.LANES == {15: 14, 16: 15, 17: 0, 32: 15, 33: 0}[L] and (L - 1) // cc.LANES == -(-L // cc.LANES) - 1
        # view 0 is found in the first step of the walk: the first occupied ring cell holds a finder of view 0
        ring = [(dz, dy, dx) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1)]
        occupied = [(dz, dy, dx) for (dz, dy, dx) in ring if (sc == qc[i] + [dx, dy, dz]).all(axis=1).any()]
        assert occupied[0] == (-1, 0, 0) and occupied[-1] == (1, 1, 1)
        first = np.flatnonzero((sc == qc[i] + [0, 0, -1]).all(axis=1))
        assert len(first) == 1 and first[0] in c.vis[0] and cc._pair_matrix(c.points[i:i + 1], c.cloud[first])[1][0, 0] < MAXD
        assert s[i].tolist() == [True, True, False]
    print("cell_runs: run lengths", [r["L"] for r in c.claims["runs"]], "the finder of view 1 is the last point of the 27th cell")


def test_query_tails_and_clamped_fixtures(built, seen):
    assert [built[f"query_tail_{n}"].points.shape[0] for n in cc.QUERY_COUNTS] == list(cc.QUERY_COUNTS)
    assert [-(-n // cc.QUERIES_PER_BLOCK) for n in cc.QUERY_COUNTS] == [1, 1, 1, 1, 1, 1, 2, 5]          # blocks of kc_visible
    assert [-(-n // cc.WAVES_PER_BLOCK) for n in cc.QUERY_COUNTS] == [1, 1, 1, 2, 4, 4, 5, 17]          # blocks of kc_project
    assert all(seen[f"query_tail_{n}"].any() for n in cc.QUERY_COUNTS)
    c = built["clamped"]
    g = pc.grid_of(c.cloud, cc.search_radius(c))
    assert (((c.points < g.mn[0]) | (c.points > g.mx[0])).any(axis=1)).all() and (g.n[0] > 10).all(), "every query is outside the box"
    moved = (pc.cells_of(g, c.points[None], clamp=False)[0] != pc.cells_of(g, c.points[None])[0]).any(axis=1)
    low = (c.points < g.mn[0]).any(axis=1)
    assert moved[low].all() and moved.sum() >= 70, "below the box the cell index is negative; above it the clamp moves all but the nearest"
    where = np.array(c.claims["where"])
    s = seen["clamped"]
    assert s[where == "near", 1].all() and not s[where != "near"].any() and (where == "near").sum() == 26
    assert s[where == "near", 0].any()
    assert np.abs(c.points[where == "far"]).max() >= 1e6


@pytest.mark.parametrize("side", ["under", "over"])
def test_grown_grid_fixtures(side, built, seen):
    c = built[f"grown_grid_{side}"]
    cell = cc.search_radius(c)
    g, flat = pc.grid_of(c.cloud, cell), pc.grid_of(c.cloud, cell, grow=False)
    if side == "under":
        assert not g.grown[0] and int(g.ncell[0]) == cc.K["CELL_CAP"] and g.n[0].tolist() == [2048, 2048, 32]
    else:
        assert g.grown[0] and g.cell[0] == cell * cc.K["GROW"] and flat.n[0].tolist() == [2049, 2048, 32]
        assert int(flat.ncell[0]) > cc.K["CELL_CAP"] > int(g.ncell[0]) > cc.K["CELL_CAP"] // 4
    assert 2 * 4 * int(g.ncell[0]) <= 2 ** 30, "the two dense tables stay within 1 GiB"
    old = pc.cells_of(flat, c.cloud[None])[0], pc.cells_of(flat, c.points[None])[0]
    new = pc.cells_of(g, c.cloud[None])[0], pc.cells_of(g, c.points[None])[0]
    s = seen[c.name]
    for p in c.claims["placed"]:
        i = p["query"]
        assert old[0][p["seen"], 0] - old[1][i, 0] == 1 and old[0][p["refused"], 0] - old[1][i, 0] == 2
        assert abs(new[0][p["refused"], 0] - new[1][i, 0]) <= (1 if side == "over" else 2)
        assert s[i].tolist() == [True, False], "view 0 has the near point; view 1 only the one two old cells away"
        d = float(np.linalg.norm(c.cloud[p["refused"]] - c.points[i]))
        assert MAXD < cell < d < cell + 0.0021
    assert s[:120].any(axis=1).mean() > 0.5
    print(f"{c.name}: grid {g.n[0].tolist()} of {g.cell[0]:.6f} m, {int(g.ncell[0])} cells, {8 * int(g.ncell[0]) / 2 ** 30:.2f} GiB of tables")


# ------------------------------------------------------------------------------------------------- kc_project
@pytest.mark.parametrize("F", cc.WIDTHS)
def test_width_fixtures(F, built):
    c = built[f"width_{F}"]
    kinds = c.claims["kinds"]
    t = c.truth
    passes = -(-F // cc.WIDE)
    assert [k for k in kinds if k.startswith("pass_") and k != "pass_and_first"] == [f"pass_{cc.WIDE * p}" for p in range(1, passes)]
    want = {"first_column": 1, "last_column": 1, "zero": 0, "negative_zero": 0, "nan": 1, "random": 3, "random_and_zero": 2, "pass_and_first": 2}
    assert t["dino_views"].tolist() == [want.get(k, 1) for k in kinds]
    assert (t["pixels"][:, :, 0] >= 0).all() and np.isnan(t["dino"][kinds.index("nan")]).sum() == 1
    zero = [kinds.index("zero"), kinds.index("negative_zero")]
    assert not t["dino"][zero].any() and not np.signbit(t["dino"][zero]).any()
    assert t["dino"][kinds.index("first_column"), 0] == 1.5 and t["dino"][kinds.index("last_column"), F - 1] == -2.5
    if passes > 1:   # a row whose only non-zero element is in the first pass counts in the last pass too
        j = kinds.index("pass_and_first")
        assert t["dino"][j, 0] == 0.5 and t["dino"][j, (F - 1) // cc.WIDE * cc.WIDE] == 1.0 and np.count_nonzero(t["dino"][j]) == 2


def test_patch_fixtures(built):
    off = {}
    for shape in cc.PATCH_SHAPES:
        c = built["patch_%dx%d_%dx%d" % shape]
        fh, fw, ph, pw = shape
        h, w = c.image_hw
        assert (h, w) == (fh * ph, fw * pw)
        t, cl = c.truth, c.claims
        u, v = c.points[:, 0].astype(int), c.points[:, 1].astype(int)
        assert set(u) == set(range(w)) and set(v) == set(range(h)), "every row and every column is met"
        assert np.array_equal(t["dino"][:, 0], cl["rows"][v] + 1.0) and np.array_equal(t["dino"][:, 1], cl["cols"][u] + 1.0)
        assert cl["rows"].tolist() == [int(fh / h * x) for x in range(h)] and cl["cols"].tolist() == [int(fw / w * x) for x in range(w)]
        off[c.name] = (cl["off_rows"], cl["off_cols"])
        print(f"{c.name}: int(f / n * v) differs from v // patch on {cl['off_rows']} of {h} rows and {cl['off_cols']} of {w} columns")
    # For an image of f * p pixels over f cells, f / (f * p) is fl(1 / p) whatever f is.  With DINOv2's p = 14 (and 11, 13) the
    # product at a patch border v = k * p is k or just above it for every image below 2048 pixels, so int() agrees with v // p
    # there (exhaustive, below).  p = 49 is the smallest patch for which fl(1 / p) * (k * p) falls BELOW k for some k: the
    # reference's expression then puts the first pixel row of patch k into cell k - 1, and so must the device.
    assert all(off["patch_%dx%d_%dx%d" % s] == (0, 0) for s in cc.PATCH_SHAPES if s[2:] != (49, 49))
    assert off["patch_8x6_49x49"] == (6, 4), "rows 49, 98, 147, 196, 294, 343 of 392 and columns 49, 98, 147, 196 of 294"
    v = np.arange(2048)
    smallest = None
    for p in range(1, 64):
        r = 1.0 / p
        assert r == 3.0 / (3 * p) == 37.0 / (37 * p)
        if not np.array_equal((r * v).astype(np.int64), v // p):
            smallest = smallest or p
            assert p not in (11, 13, 14)
    assert smallest == 49 and int((1.0 / 49) * 49) == 0
