"""CPU suite: the chunk-preparation restatement (tests/prep_ref.py) against brute force, every open3d rule it restates pinned by
a hand-made case, and the host-side parts of autoinst_amd.prep_api (the trajectory walk, the synthetic street)."""
import numpy as np
import pytest

import prep_ref
from autoinst_amd import prep_api, synth


def _cloud(n, seed):
    rng = np.random.default_rng(seed)
    p = rng.random((n, 3)) * [4.0, 4.0, 1.0]
    p[: n // 10] = p[n // 10: 2 * (n // 10)]       # exact duplicates
    p[-3:] += [30.0, -20.0, 9.0]                    # far outliers
    return p


@pytest.mark.parametrize("n,nb", [(1, 20), (2, 20), (7, 3), (25, 20), (300, 20), (300, 1), (300, 64), (40, 64)])
def test_knn_avg_matches_brute_force(n, nb):
    p = _cloud(n, n + nb)
    a = prep_ref.knn_avg(p, nb)
    b = prep_ref.knn_avg_brute(p, nb)
    assert a.shape == (n,)
    np.testing.assert_allclose(a, b, rtol=1e-13, atol=0.0)


def test_self_is_one_of_the_k_at_distance_zero():
    # two points 2 m apart, k = 2: each sees itself (0) and the other (2): avg = 1
    p = np.array([[0.0, 0.0, 0.0], [2.0, 0.0, 0.0]])
    np.testing.assert_array_equal(prep_ref.knn_avg_brute(p, 20), [1.0, 1.0])
    np.testing.assert_array_equal(prep_ref.knn_avg(p, 20), [1.0, 1.0])


def test_mean_counts_zero_avg_points_in_denominator():
    # 3 copies of one point (avg 0 with k = 3) and 3 points on a line: the mean divides by all 6
    p = np.array([[0.0, 0, 0]] * 3 + [[10.0, 0, 0], [11.0, 0, 0], [12.0, 0, 0]])
    idx, avg, mean, std, thr = prep_ref.statistical_inliers(p, nb_neighbors=3, std_ratio=2.0, brute=True)
    np.testing.assert_array_equal(avg[:3], 0.0)
    pos = avg[avg > 0]
    assert mean == pos.sum() / 6
    assert std == np.sqrt(((pos - mean) ** 2).sum() / 5)
    assert thr == mean + 2.0 * std
    assert set(idx.tolist()) <= {3, 4, 5}     # avg == 0 is never kept


def test_keep_rule_is_strict_and_ascending():
    rng = np.random.default_rng(3)
    avg = rng.random(50) + 0.1
    avg[[4, 9]] = 0.0
    idx, mean, std, thr = prep_ref.statistical_from_avg(avg, 1.0)
    assert np.all(np.diff(idx) > 0)
    expect = np.where((avg > 0) & (avg < thr))[0]
    np.testing.assert_array_equal(idx, expect)
    # the comparison is strict: equal averages give std = 0 and a threshold equal to every avg, so nothing is kept
    idx, mean, std, thr = prep_ref.statistical_from_avg(np.full(4, 2.0), 2.0)
    assert (mean, std, thr) == (2.0, 0.0, 2.0) and idx.size == 0
    p = np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0]])    # the same from points: avg 0.5 and 0.5
    assert prep_ref.statistical_inliers(p, brute=True)[0].size == 0


def test_edge_cases():
    with pytest.raises(ValueError):
        prep_ref.statistical_inliers(np.zeros((5, 3)), nb_neighbors=0)
    with pytest.raises(ValueError):
        prep_ref.statistical_inliers(np.zeros((5, 3)), std_ratio=0.0)
    idx, avg, *_ = prep_ref.statistical_inliers(np.zeros((0, 3)))
    assert idx.size == 0 and avg.size == 0
    idx, avg, mean, std, thr = prep_ref.statistical_inliers(np.array([[1.0, 2.0, 3.0]]))
    assert idx.size == 0 and avg[0] == 0.0 and np.isnan(thr)


def test_far_outlier_is_dropped():
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.random((400, 3)), [[40.0, 40.0, 40.0]]])
    idx, *_ = prep_ref.statistical_inliers(p, brute=True)
    assert 400 not in idx and idx.size > 300


def test_voxel_restatement_against_a_loop():
    rng = np.random.default_rng(8)
    p = rng.random((2000, 3)) * 2.0 - 1.0
    v = 0.35
    out, tr = prep_ref.voxel_down_sample(p, v)
    vmin = p.min(0) - v * 0.5
    groups = {}
    for i, q in enumerate(p):
        key = tuple(int(np.floor(x)) for x in (q - vmin) / v)
        groups.setdefault(key, []).append(i)
    keys = sorted(groups)
    assert out.shape == (len(keys), 3)
    for r, key in enumerate(keys):
        s = np.zeros(3)
        for i in groups[key]:
            s = s + p[i]
        np.testing.assert_array_equal(out[r], s / len(groups[key]))
        np.testing.assert_array_equal(tr[groups[key]], r)


def test_voxel_borders():
    # min bound 0 -> vmin = -0.5 with voxel 1: a point at 0.5 lies exactly on the border and belongs to the upper voxel; so does
    # the double just below 0.5, because p - vmin rounds up to 1.0 before the division (the rule is floor((p - vmin) / v))
    p = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.49999999999999994, 0.0, 0.0], [0.4, 0.0, 0.0], [1.5, 0.0, 0.0]])
    out, tr = prep_ref.voxel_down_sample(p, 1.0)
    np.testing.assert_array_equal(tr, [0, 1, 1, 0, 2])
    np.testing.assert_array_equal(out[:, 0], [(0.0 + 0.4) / 2, (0.5 + 0.49999999999999994) / 2, 1.5])


def test_box_select_restatement_is_strict():
    p = np.array([[0.0, 0, 0], [1.0, 0.5, 0.5], [0.5, 0.5, 0.5], [1e-300, 0.5, 0.5]])
    (a,) = prep_ref.box_select(p, [(np.zeros(3), np.ones(3))])
    np.testing.assert_array_equal(a, [2, 3])


def test_walk_matches_restatement():
    m = synth.street_map(70.0, seed=2)
    c1, i1 = prep_api.chunk_centres(m["T_pcd"], m["positions"], m["first_position"], m["indices"])
    c2, i2 = prep_ref.chunk_centres(m["T_pcd"], m["positions"], m["first_position"], m["indices"])
    assert len(c1) == len(c2) == 3 and i1 == i2
    for a, b in zip(c1, c2):
        np.testing.assert_array_equal(a, b)


def test_street_map_is_deterministic_and_has_its_features():
    a = synth.street_map(50.0, seed=4)
    b = synth.street_map(50.0, seed=4)
    for k in ("nonground", "ground", "positions", "T_pcd"):
        np.testing.assert_array_equal(a[k], b[k])
    for k, v in a["labels"].items():
        np.testing.assert_array_equal(v, b["labels"][k])
    assert a["labels"]["seg_nonground"].shape[0] == a["nonground"].shape[0]
    assert a["labels"]["seg_ground"].shape[0] == a["ground"].shape[0]
    assert not np.allclose(a["T_pcd"][:3, :3], np.eye(3))
    _, cnt = np.unique(a["nonground"], axis=0, return_counts=True)
    assert cnt.max() >= 20                            # repeated points: the avg == 0 rule fires
    assert (a["labels"]["instance_nonground"] > 0).any()
    # points exactly on the x faces of a chunk box
    c, _ = prep_api.chunk_centres(a["T_pcd"], a["positions"], a["first_position"], a["indices"])
    assert c and np.any(a["nonground"][:, 0] == c[0][0] - 12.5)
