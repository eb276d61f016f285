"""CPU: every fixture of tests/prep_cases.py sits in the regime its name claims, the host models equal the grid-free truths on
all of them, the stop rule `kq_knn_avg` had before the rounding of `kcell_of` was counted gets an average wrong on every ring-stop
case while the shipped one misses none (also in a seeded search), a list of deliberately wrong rules is each rejected by a
fixture built for it, and no fixture but the ones built to sit on the threshold lies inside the statistics bound.  No GPU, no
library."""
import os
import re

import numpy as np
import pytest

import prep_cases as pc

SEARCH_TRIES = 100_000         # per k, seed 2025


def _by_name(cases, name):
    return next(c for c in cases if c.name == name)


def _models(c):
    """The fixtures the ring-by-ring model runs on: all but the second-lap cloud, whose n x n matrix is too large."""
    return c.n <= 4096


# ------------------------------------------------------------------------------------------------- constants
def test_the_three_ring_searches_share_one_stop_rule():
    """`kq_knn_avg` (ai_prep.hip), `kf_knn_avg`, `kf_nn1` (ai_finish.hip) and `kp_nn1` (ai_points.hip) use the same slack and the same
    ulps in the comparison, and all four call the one `face_gap` and the one `axis_mag` that exist under csrc (ai_cells.inc).

    The two kNN search bodies, and the two 1-NN search bodies, are still compared as text: written once as `__forceinline__`
    functions they gave the parent's instructions (up to exchanged operands of commutative ones) in `kq_knn_avg` alone; in
    `kf_knn_avg<20 / 32 / 64>` the same 1301 / 1822 / 3430 instructions came out in another order, and `kp_nn1` / `kf_nn1` came out
    with 496 / 507 instructions for 502 / 513 (tools/asm_identity.py), so the bodies stay in their kernels."""
    sources = {f: pc._read(pc._CSRC, f) for f in sorted(os.listdir(pc._CSRC)) if f.endswith((".hip", ".h", ".inc"))}
    for helper in ("face_gap", "axis_mag"):
        defined = [f for f, text in sources.items() for _ in re.finditer(r"^__device__ [^\n;]*\b%s\([^;{]*\) \{" % helper, text, re.M)]
        assert defined == ["ai_cells.inc"], (helper, defined)
    kernels = {name: re.search(r"void %s\(.*?\n\}" % name, sources[f], re.S).group(0)
               for name, f in (("kq_knn_avg", "ai_prep.hip"), ("kf_knn_avg", "ai_finish.hip"), ("kp_nn1", "ai_points.hip"),
                               ("kf_nn1", "ai_finish.hip"))}
    want = (pc.K["SLACK_ULPS"], pc.K["STOP_ULPS"])
    for name, body in kernels.items():
        cell, best = (r"g\.cell", "kth") if name.endswith("knn_avg") else ("cell", "best")
        assert pc.stop_constants(body, cell, best, name) == want, name
        assert body.count("axis_mag(") == 3 and body.count("face_gap(") == 3, name
    loops = [kernels[name][kernels[name].index("  double best[K];"):] for name in ("kq_knn_avg", "kf_knn_avg")]
    assert loops[0] == loops[1], "the search bodies of kq_knn_avg and kf_knn_avg differ"
    # kf_nn1 reads its chunk's slice of the cell tables (cs, ce) and speaks of major rows; nothing else may differ
    nn1 = [kernels[name][kernels[name].index("  int cx, cy, cz;"):kernels[name].index("lb) break;")] for name in ("kp_nn1", "kf_nn1")]
    nn1 = [re.sub(r"\s*//[^\n]*", "", body) for body in nn1]
    assert nn1[0] == nn1[1].replace("cs[cc]", "cstart[cc]").replace("ce[cc]", "cend[cc]"), "the search bodies of kp_nn1 and kf_nn1 differ"


def test_template_boundaries_are_fixtures():
    assert pc.KNN_LENGTHS == (20, 32, 64) and pc.LAP == 65536
    ks = {c.nb: c.claims["instance"] for c in pc.knn_cases() if c.name.startswith("knn_k") and "instance" in c.claims}
    for a, b in zip(pc.KNN_LENGTHS, pc.KNN_LENGTHS[1:]):
        assert ks[a] == a and ks[a + 1] == b
    assert ks[1] == ks[2] == ks[19] == 20 and ks[63] == ks[64] == 64
    assert [pc.knn_instance(k) for k in (1, 20, 21, 32, 33, 64)] == [20, 20, 32, 32, 64, 64]


# ------------------------------------------------------------------------------------------------- kNN
def test_ring_stop_cases_cover_axes_directions_rings_and_k():
    got = {(c.claims["k"], c.claims["axis"], c.claims["sgn"], c.claims["r"]) for c in pc.ring_stop_cases()
           if not c.name.startswith("ring_stop_issue")}
    assert got == {(k, a, s, r) for k in pc.RING_KS for a in range(3) for s in (-1, 1) for r in (1, 2, 3)}
    assert sum(c.name.startswith("ring_stop_issue") for c in pc.ring_stop_cases()) == 3


def test_parent_stop_rule_gets_an_average_wrong_on_every_ring_stop_case():
    found = [c for c in pc.ring_stop_cases() if not c.claims.get("issue")]
    for c in found:
        q = c.claims["query"]
        parent = pc.knn_model(c.points, c.nb, stop="parent")
        shipped = pc.knn_model(c.points, c.nb, stop="shipped")
        assert parent["avg"][q] != c.avg[q], c.name
        assert parent["rings"][q] == c.claims["r"] and shipped["rings"][q] > c.claims["r"], (c.name, parent["rings"][q], shipped["rings"][q])
        assert shipped["avg"].tobytes() == c.avg.tobytes(), c.name
    assert len(found) == 36


def test_the_line_of_the_issue_misses_on_the_grid_it_was_found_on():
    """With ``np.cbrt`` for the cell the parent's rule gives the two averages the issue quotes, on each axis; the shipped rule is
    exact on that grid and on the host's."""
    lines = [c for c in pc.ring_stop_cases() if c.claims.get("issue")]
    assert len(lines) == 3
    for c in lines:
        g = pc.knn_grid(c.points, cbrt=np.cbrt)
        assert (pc.knn_model(c.points, 2, stop="parent", grid=g)["avg"][2].hex(), c.avg[2].hex()) == pc.ISSUE_AVG, c.name
        for grid in (g, None):
            assert pc.knn_model(c.points, 2, grid=grid)["avg"].tobytes() == c.avg.tobytes(), c.name


def test_shipped_model_equals_the_truth_on_every_fixture():
    for c in pc.knn_cases():
        if _models(c):
            m = pc.knn_model(c.points, c.nb)
            assert m["avg"].tobytes() == c.avg.tobytes(), c.name
    big = _by_name(pc.knn_cases(), f"knn_n{pc.LAP + 1}_second_lap")
    one = np.flatnonzero(big.groups == 0)                   # the group with the extra point, on its own grid
    assert pc.knn_model(big.points[one], big.nb)["avg"].tobytes() == big.avg[one].tobytes()


def test_seeded_search_finds_misses_of_the_parent_rule_only(capsys):
    total = {"tries": 0, "miss_parent": 0, "miss_shipped": 0}
    for k in pc.RING_KS:
        r = pc.ring_stop_search(SEARCH_TRIES, 2025, k)
        for key in total:
            total[key] += r[key]
        assert r["miss_parent"] > 0 and r["miss_shipped"] == 0, (k, r["miss_parent"], r["miss_shipped"])
    with capsys.disabled():
        print(f"\nkNN ring-stop search: {total['tries']} tries, parent rule misses {total['miss_parent']}, shipped rule misses "
              f"{total['miss_shipped']}")
    assert total["tries"] == len(pc.RING_KS) * SEARCH_TRIES and total["miss_shipped"] == 0


def test_shipped_rule_costs_a_ring_only_near_the_border():
    """The face gap is at least r * cell up to its own rounding: the shipped rule never searches more than one ring beyond the
    parent's on the fixtures, and in total fewer than two per cent more."""
    more = total = 0
    for c in pc.knn_cases():
        if _models(c):
            a, b = pc.knn_model(c.points, c.nb, stop="parent")["rings"], pc.knn_model(c.points, c.nb)["rings"]
            assert (b - a <= 1).all(), c.name
            more, total = more + int((b - a).clip(min=0).sum()), total + int(a.sum())
    assert more <= 0.02 * total, (more, total)


def test_knn_regime_claims():
    cases = pc.knn_cases()
    grown = _by_name(cases, "knn_plane_yz_grown")
    g, g0 = pc.knn_grid(grown.points), pc.knn_grid(grown.points, grow=False)
    cap = pc.K["ROW_CAP"][0] * grown.n + pc.K["ROW_CAP"][1]
    assert g.steps >= 1 and g.cell == g.cell0 * pc.K["GROW"] ** g.steps and g.rows <= cap < g0.rows and g.n[0] == 1
    for c in cases:
        if _models(c) and c is not grown:
            assert pc.knn_grid(c.points).steps == 0 or c.name == "knn_two_clusters", c.name
    two = _by_name(cases, "knn_two_clusters")
    g = pc.knn_grid(two.points)
    occupied = np.unique(pc.kcells(g, two.points)[:, 1:], axis=0).shape[0]
    assert pc.knn_model(two.points, two.nb)["rings"].min() >= two.claims["min_rings"] and occupied < g.rows // 10
    corner = _by_name(cases, "knn_max_corner")          # the seeded search found one: a far corner whose index reaches nx
    g = pc.knn_grid(corner.points)
    assert (pc.kcells(g, corner.points, clamp=False) == g.n).any() and (pc.kcells(g, corner.points) <= g.n - 1).all()
    assert not _by_name(cases, "knn_identical").avg.any() and (pc.knn_grid(_by_name(cases, "knn_identical").points).n == 1).all()
    copies = _by_name(cases, "knn_k_copies")
    assert int((copies.avg == 0).sum()) == copies.claims["zeros"] == copies.k
    assert np.unique(copies.points, axis=0).shape[0] == copies.n - (copies.k - 1) - (copies.k - 2)
    for c in cases:
        if c.name.startswith("knn_nb_above_n"):
            assert c.nb > pc.MAX_K >= c.n == c.k == c.claims["k"]
    for a, name in enumerate("xyz"):
        g = pc.knn_grid(_by_name(cases, f"knn_line_{name}").points)
        assert g.n[a] > 1 and (np.delete(g.n, a) == 1).all()
    for name in ("knn_plane_xy", "knn_plane_xz"):
        assert sorted(pc.knn_grid(_by_name(cases, name).points).n)[0] == 1
    assert [c.n for c in cases if re.fullmatch(r"knn_n\d+", c.name)] == [pc.BLOCK - 1, pc.BLOCK, pc.BLOCK + 1]
    big = _by_name(cases, f"knn_n{pc.LAP + 1}_second_lap")
    assert big.n == pc.RED_BLOCKS * pc.BLOCK + 1 and pc.reduction_depth(big.n) == pc.reduction_depth(pc.LAP) + 1 == 2 + 20


def test_the_cube_sits_on_the_threshold():
    cube = _by_name(pc.knn_cases(), "knn_dyadic_cube")
    assert np.unique(cube.avg).size == 1 and cube.avg[0] > 0
    assert cube.ref["mean"] == cube.avg[0] and cube.ref["std"] == 0.0 and cube.ref["threshold"] == cube.avg[0]
    assert cube.ref["keep"].size == 0
    model = pc.stats_model(cube.avg, cube.std_ratio)
    assert (model["mean"], model["std"], model["threshold"]) == (cube.avg[0], 0.0, cube.avg[0])


def test_no_fixture_lies_inside_the_statistics_bound():
    """Except the ones built to sit on the threshold (all averages equal: the cube, and the two-point cloud), no fixture has an
    average within `stats_bound` of the threshold, so its kept set is the reference's whatever the device's rounding."""
    for c in pc.knn_cases():
        if c.claims.get("on_threshold"):
            assert c.near.size == c.n, c.name
        else:
            assert c.near.size == 0, (c.name, c.near, c.ref["threshold"], c.bound)


def test_the_bound_holds_for_the_device_order_and_is_far_below_1e_12():
    for c in pc.knn_cases():
        if c.n < 2:
            continue
        m = pc.stats_model(c.avg, c.std_ratio)
        for key in ("mean", "std", "threshold"):
            assert abs(m[key] - c.ref[key]) <= c.bound[key], (c.name, key, m[key], c.ref[key], c.bound[key])
        if c.ref["std"] > 1e-3 * c.ref["mean"]:             # a spread that is not itself a rounding error
            assert c.bound["threshold"] <= 1e-14 * c.ref["threshold"], (c.name, c.bound, c.ref)


# ------------------------------------------------------------------------------------------------- box select
def test_box_model_equals_the_truth_and_the_claims_hold():
    sizes = []
    for c in pc.box_cases():
        out, off, total = pc.box_model(c.points, c.boxes)
        assert total == c.truth[0].size and out.tobytes() == c.truth[0].tobytes() and off.tobytes() == c.truth[1].tobytes(), c.name
        if "inside" in c.claims:
            assert total == c.claims["inside"], (c.name, total)
        if "tiles" in c.claims:
            sizes.append(c.points.shape[0])
    assert tuple(sizes) == (1, 63, 64, 65, 255, 256, 257, 513)
    assert [c.claims["n_boxes"] for c in pc.box_cases() if "n_boxes" in c.claims] == [1, 2, 65536]
    faces = _by_name(pc.box_cases(), "box_faces")
    np.testing.assert_array_equal(faces.truth[0], [2, 5, 8, 9, 12, 15])      # low faces: the ulp above; high faces: the ulp below
    nested = _by_name(pc.box_cases(), "box_identical_nested_inverted")
    cnt = np.diff(nested.truth[1])
    assert cnt[0] == cnt[1] > cnt[2] > 0 and cnt[3] == 0 and cnt[4] == 300 and 0 < cnt[5] < 300
    bad = _by_name(pc.box_cases(), "box_nonfinite_points")
    assert np.diff(bad.truth[1]).tolist() == [20, 20] and bad.truth[0].max() < 20


def test_box_model_cap_protocol():
    c = _by_name(pc.box_cases(), "box_n513")
    total = c.truth[0].size
    out, off, t = pc.box_model(c.points, c.boxes, cap=total - 1)
    assert t == total and (out == -7).all() and off.tobytes() == c.truth[1].tobytes()
    assert pc.box_model(c.points, c.boxes, cap=0)[0].size == 0
    assert pc.box_model(c.points, c.boxes, cap=total)[0].tobytes() == c.truth[0].tobytes()


# ------------------------------------------------------------------------------------------------- voxels
def test_voxel_model_equals_the_truth_and_the_claims_hold():
    for c in pc.voxel_cases():
        if "refused" in c.claims:
            with pytest.raises(ValueError, match=c.claims["refused"]):
                pc.voxel_keys(c.points, c.voxel)
            continue
        keys = pc.voxel_keys(c.points, c.voxel)
        out, trace = pc.voxel_model(c.points, c.voxel)
        assert out.tobytes() == c.truth[0].tobytes() and trace.tobytes() == c.truth[1].tobytes(), c.name
        if "bits" in c.claims:
            assert tuple(keys["bits"]) == c.claims["bits"], (c.name, keys["bits"])
        if "voxels" in c.claims:
            assert out.shape[0] == c.claims["voxels"], (c.name, out.shape)
        if "found" in c.claims:
            assert c.claims["found"] >= 3, c.name
    assert sum(pc.voxel_keys(_by_name(pc.voxel_cases(), "voxel_64_key_bits").points, 1.0)["bits"]) == pc.K["MAX_KEY_BITS"]
    borders = _by_name(pc.voxel_cases(), "voxel_borders_0.35")
    assert (borders.points < 0).any() and np.unique(borders.truth[1]).size > 15


# ------------------------------------------------------------------------------------------------- wrong rules
def _stats_differ(c, mutant):
    m = pc.stats_ref(c.avg, c.std_ratio, mutant)
    beyond = any(abs(m[k] - c.ref[k]) > c.bound[k] for k in ("mean", "std", "threshold"))
    return beyond or m["keep"].tolist() != c.ref["keep"].tolist()


def test_every_wrong_rule_is_rejected_by_a_fixture_built_for_it():
    knn, box, vox = pc.knn_cases(), pc.box_cases(), pc.voxel_cases()
    # box: `<=` faces; the rank inside the wave alone
    for name in ("box_faces", "box_signed_zero"):
        c = _by_name(box, name)
        assert pc.box_model(c.points, c.boxes, mutant="le_faces")[2] > c.truth[0].size, name
    c = _by_name(box, "box_n513")
    assert pc.box_model(c.points, c.boxes, mutant="wave_rank_only")[0].tobytes() != c.truth[0].tobytes()
    # kNN: no clamp in kcell_of; the parent's stop rule (every ring-stop case: test above); the order of the sum; the divisor
    c = _by_name(knn, "knn_max_corner")
    assert pc.knn_model(c.points, c.nb, mutant="no_clamp")["avg"].tobytes() != c.avg.tobytes()
    assert all(pc.knn_model(r.points, r.nb, stop="parent")["avg"].tobytes() != r.avg.tobytes() for r in pc.ring_stop_cases()
               if not r.claims.get("issue"))
    c = _by_name(knn, "knn_k20")
    assert pc.knn_avg_exact(c.points, c.nb, mutant="sum_before_sort").tobytes() != c.avg.tobytes()
    for c in knn:
        if c.name.startswith("knn_nb_above_n") and c.n > 1:
            assert pc.knn_avg_exact(c.points, c.nb, mutant="divide_by_nb").tobytes() != c.avg.tobytes(), c.name
    # statistics: avg >= 0 kept, the mean over avg > 0 only, std with n, `<=` threshold
    copies = _by_name(knn, "knn_k_copies")
    zeros = np.flatnonzero(copies.avg == 0)
    assert np.isin(zeros, pc.stats_ref(copies.avg, 2.0, "keep_zero")["keep"]).all() and not np.isin(zeros, copies.ref["keep"]).any()
    assert _stats_differ(copies, "mean_over_positive")
    assert not _stats_differ(_by_name(knn, "knn_k20"), "mean_over_positive")      # without an avg == 0 the two means agree
    assert all(_stats_differ(_by_name(knn, name), "std_with_n") for name in ("knn_k20", "knn_n255", "knn_k_copies"))
    cube = _by_name(knn, "knn_dyadic_cube")
    assert pc.stats_ref(cube.avg, 2.0, "le_threshold")["keep"].size == 8 and cube.ref["keep"].size == 0
    # voxels: multiplication by the inverse, vmin without the half voxel, sums in sorted order
    for v in pc.VOXEL_SIZES:
        c = _by_name(vox, f"voxel_inverse_mismatch_{v}")
        assert pc.voxel_model(c.points, c.voxel, "inverse")[1].tobytes() != c.truth[1].tobytes(), c.name
        c = _by_name(vox, f"voxel_borders_{v}")
        assert pc.voxel_model(c.points, c.voxel, "no_half")[1].tobytes() != c.truth[1].tobytes(), c.name
    abc, cba = _by_name(vox, "voxel_triple_abc"), _by_name(vox, "voxel_triple_cba")
    assert abc.truth[0].tobytes() != cba.truth[0].tobytes()
    assert pc.voxel_model(cba.points, 1.0, "sorted_sum")[0].tobytes() != cba.truth[0].tobytes()
    assert pc.voxel_model(abc.points, 1.0, "sorted_sum")[0].tobytes() == abc.truth[0].tobytes()


def test_nonfinite_clouds_are_refused_by_both_grids():
    clouds = pc.nonfinite_clouds()
    assert len(clouds) == 9 and all(p.shape == (301 - 1, 3) and int((~np.isfinite(p)).sum()) == 1 for _, p in clouds)
    for name, p in clouds:
        with pytest.raises(ValueError, match="coordinates are not finite"):
            pc.knn_grid(p)
        with pytest.raises(ValueError, match="coordinates are not finite"):
            pc.voxel_keys(p, 0.35)
