"""CPU suite: tests/finish_ref.py (the restatement `ai_chunk_finish` is checked against on the GPU) against the reference's own
expressions, written out here line by line -- ``ncuts_utils.py:185-204`` and ``point_cloud_utils.py:331-342`` -- with NumPy's
``np.mean`` / ``np.where`` and a brute-force nearest neighbour, on small clouds; and against wrong rules, each on a case built so
that the wrong rule gives another answer."""
import warnings

import numpy as np
import pytest

import finish_ref
import prep_ref
from finish_ref import sq_dist


def reference_tail(fine, major, labels, ground, inst, seg, mean_height, nb=20, std_ratio=2.0):
    """The reference's lines on arrays (a cloud is its point array, get_subpcd is an index, + is a concatenation)."""
    nn = np.array([int(np.argmin(sq_dist(p, major))) for p in fine], dtype=np.int64)     # :186-188, search_knn_vector_3d(point, 1)
    colors = np.asarray(labels)[nn] if fine.shape[0] else np.zeros(0, np.int32)           # features_to[i] = features_from[idx[0]]
    inliers = prep_ref.statistical_inliers(ground, nb, std_ratio, brute=True)[0]          # :191
    ground_inliers = ground[inliers]                                                      # :192
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        mean_hight = np.mean(ground_inliers[:, 2])                                        # :193
        in_idcs = np.where(ground_inliers[:, 2] < (mean_hight + mean_height))[0]          # :194-196
    cut_hight = ground_inliers[in_idcs]                                                   # :197
    merged_chunk = np.concatenate([fine, cut_hight])                                      # :199
    inst_ground = inst[inliers][in_idcs]                                                  # :201
    seg_ground = seg[inliers][in_idcs]                                                    # :202
    return {"nn": nn, "colors": colors, "inliers": inliers, "in_idcs": in_idcs, "mean_hight": float(mean_hight),
            "merged_chunk": merged_chunk, "cut_hight": cut_hight, "inst_ground": inst_ground, "seg_ground": seg_ground}


def dyadic(a, bits=10):
    return np.round(np.asarray(a) * 2.0 ** bits) / 2.0 ** bits


def random_chunk(seed, nf=300, nm=40, ng=500):
    """Coordinates on a 2^-10 grid: every sum of z is exact, so np.mean and F4's order agree bit for bit."""
    rng = np.random.default_rng(seed)
    fine = dyadic(rng.random((nf, 3)) * [8.0, 8.0, 2.0])
    major = dyadic(rng.random((nm, 3)) * [8.0, 8.0, 2.0])
    ground = rng.random((ng, 3)) * [8.0, 8.0, 0.05]
    ground[: ng // 5, 2] += 0.9                       # a kerb
    ground[-6:] += [[30.0, 0, 5.0], [0, -40.0, 2.0], [25.0, 25.0, 9.0], [-30.0, 1.0, -4.0], [-30.5, 1.0, 3.0], [9.0, 50.0, 1.0]]
    ground = dyadic(ground[rng.permutation(ng)])
    labels = rng.integers(0, 7, nm).astype(np.int32)
    inst = rng.integers(0, 1000, ng).astype(np.int64)
    seg = rng.integers(0, 50, ng).astype(np.int64)
    return fine, major, labels, ground, inst, seg


def check_against_reference(got, ref, fine, ground, inst, seg):
    np.testing.assert_array_equal(got["fine_nn"], ref["nn"])
    np.testing.assert_array_equal(got["fine_label"], ref["colors"])
    np.testing.assert_array_equal(got["inliers"], ref["inliers"])
    np.testing.assert_array_equal(got["keep"], ref["inliers"][ref["in_idcs"]])     # the indices behind [inliers][in_idcs]
    assert got["merged_points"].tobytes() == ref["merged_chunk"].tobytes()
    np.testing.assert_array_equal(inst[got["keep"]], ref["inst_ground"])
    np.testing.assert_array_equal(seg[got["keep"]], ref["seg_ground"])
    nf = fine.shape[0]
    np.testing.assert_array_equal(got["merged_label"][:nf], ref["colors"] + 1)
    assert not got["merged_label"][nf:].any() and got["merged_label"].shape[0] == nf + ref["in_idcs"].size


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_restatement_equals_the_reference_lines(seed):
    fine, major, labels, ground, inst, seg = random_chunk(seed)
    ref = reference_tail(fine, major, labels, ground, inst, seg, 0.6)
    got = finish_ref.finish_chunk(fine, major, labels, ground, brute=True)
    assert got["mean_z"] == ref["mean_hight"]          # dyadic z: both orders are exact
    assert 0 < ref["in_idcs"].size < ref["inliers"].size < ground.shape[0]      # the kerb is cut, the outliers are gone
    check_against_reference(got, ref, fine, ground, inst, seg)
    np.testing.assert_array_equal(got["fine_dist"], np.sqrt(sq_dist(fine, major[ref["nn"]])))
    # the cKDTree path gives what brute force gives
    tree = finish_ref.finish_chunk(fine, major, labels, ground)
    for k in ("fine_nn", "fine_dist", "keep", "merged_label"):
        np.testing.assert_array_equal(tree[k], got[k])


def test_f4_order_is_a_sum_and_exact_on_dyadic_values():
    rng = np.random.default_rng(5)
    z = dyadic(rng.standard_normal(140_000))          # more than 65 536: a slot adds more than one member
    flag = rng.random(z.size) < 0.7
    assert finish_ref.f4_sum(z, flag) == np.sum(z[flag]) == float(sum(int(v * 1024) for v in z[flag])) / 1024.0
    y = rng.standard_normal(70_001)
    n = y.size
    assert abs(finish_ref.f4_sum(y, np.ones(n, bool)) - np.sum(y)) <= 2 * (n - 1) * 2.0 ** -53 * np.abs(y).sum()
    assert finish_ref.f4_sum(np.zeros(0), np.zeros(0, bool)) == 0.0


def test_get_corrected_ground_lines():
    """point_cloud_utils.py:331-342: the same ground tail, appended to the chunk's non-ground points."""
    fine, major, labels, ground, inst, seg = random_chunk(7)
    inliers = prep_ref.statistical_inliers(ground, 20, 2.0, brute=True)[0]                    # :332
    ground_inliers = ground[inliers]                                                          # :333
    mean_hight = np.mean(ground_inliers[:, 2])                                                # :334
    inliers_ground = np.where(ground_inliers[:, 2] < (mean_hight + 0.6))[0]                   # :335-337
    pcd_chunk_ground = ground_inliers[inliers_ground]                                         # :338
    input_pcd = np.concatenate([fine, pcd_chunk_ground])                                      # :340
    inst_ground = inst[inliers][inliers_ground]                                               # :341
    got = finish_ref.corrected_ground(ground, brute=True)
    assert np.concatenate([fine, ground[got["keep"]]]).tobytes() == input_pcd.tobytes()
    np.testing.assert_array_equal(inst[got["keep"]], inst_ground)


def test_empty_and_tiny_grounds():
    for ground in (np.zeros((0, 3)), np.array([[1.0, 2.0, 3.0]])):
        got = finish_ref.corrected_ground(ground, brute=True)
        assert got["keep"].size == 0 and np.isnan(got["mean_z"]) and got["n_inliers"] == 0
    with pytest.raises(ValueError):
        finish_ref.finish_chunk(np.zeros((2, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), np.zeros((0, 3)))
    with pytest.raises(ValueError):
        finish_ref.finish_chunk(np.array([[np.nan, 0, 0]]), np.zeros((1, 3)), np.zeros(1, np.int32), np.zeros((0, 3)))


# ------------------------------------------------------------------ wrong rules, each on a case that tells it from the right one

def grid_ground():
    """A 16 x 16 grid, z alternating 0 and 2^-3; with std_ratio 100 every point is an inlier: mean_z = 2^-4 exactly, and with
    mean_height = 2^-4 the limit is 2^-3 exactly -- half of the points sit ON the limit."""
    xx, yy = np.meshgrid(np.arange(16.0), np.arange(16.0), indexing="ij")
    z = ((xx + yy) % 2) * 0.125
    return np.stack([xx.ravel(), yy.ravel(), z.ravel()], 1)


def test_rejects_le_in_the_height_cut():
    ground = grid_ground()
    inst = np.arange(256)
    ref = reference_tail(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), ground, inst, inst, 0.0625, std_ratio=100.0)
    good = finish_ref.corrected_ground(ground, 20, 100.0, 0.0625, brute=True)
    bad = finish_ref.corrected_ground(ground, 20, 100.0, 0.0625, brute=True, variant="le")
    assert good["n_inliers"] == 256 and good["mean_z"] == 0.0625 and good["z_limit"] == 0.125
    assert np.sum(ground[:, 2] == good["z_limit"]) == 128
    np.testing.assert_array_equal(good["keep"], ref["inliers"][ref["in_idcs"]])
    assert good["keep"].size == 128 and bad["keep"].size == 256


def kerb_ground():
    """Outliers FIRST (so that inlier positions and chunk indices differ), a plane at z = 0 and a kerb at z = 0.875."""
    rng = np.random.default_rng(11)
    far = np.array([[60.0, 0, 100.0], [0, -45.0, 100.0], [20.0, 30.0, 100.0], [-80.0, 1.0, 100.0], [-80.5, 1.0, 100.0]])
    plane = np.c_[dyadic(rng.random((200, 2)) * 6.0), np.zeros(200)]
    kerb = np.c_[dyadic(rng.random((50, 2)) * [6.0, 1.0] + [0.0, 6.0]), np.full(50, 0.875)]
    return np.concatenate([far, plane, kerb])


def test_rejects_a_mean_over_all_ground_points_and_inlier_list_indices():
    ground = kerb_ground()
    inst = np.arange(ground.shape[0]) * 3
    ref = reference_tail(np.zeros((0, 3)), np.zeros((0, 3)), np.zeros(0, np.int32), ground, inst, inst, 0.6)
    good = finish_ref.corrected_ground(ground, brute=True)
    assert not np.isin(np.arange(5), good["inliers"]).any() and good["n_inliers"] == 250
    assert good["mean_z"] == ref["mean_hight"] == 50 * 0.875 / 250
    np.testing.assert_array_equal(good["keep"], ref["inliers"][ref["in_idcs"]])
    np.testing.assert_array_equal(good["keep"], np.arange(5, 205))                 # the plane: the kerb is above 0.175 + 0.6
    np.testing.assert_array_equal(inst[good["keep"]], ref["inst_ground"])
    mean_all = finish_ref.corrected_ground(ground, brute=True, variant="mean_all")
    assert mean_all["mean_z"] > 2.0 and mean_all["keep"].size == 250               # the far points lift the limit over the kerb
    shifted = finish_ref.corrected_ground(ground, brute=True, variant="keep_in_inliers")
    np.testing.assert_array_equal(shifted["keep"], np.arange(0, 200))              # positions in the inlier list, 5 too low
    assert not np.array_equal(inst[shifted["keep"]], ref["inst_ground"])


def test_rejects_a_nearest_major_of_a_neighbouring_chunk():
    rng = np.random.default_rng(13)
    fine = dyadic(rng.random((200, 3)) * 4.0)
    major0 = dyadic(rng.random((30, 3)) * 4.0)
    major = [major0, major0 + [0.25, 0.0, 0.0]]                  # overlapping chunks: the same place, other voxel means
    labels = [np.arange(30, dtype=np.int32), np.arange(30, dtype=np.int32) + 100]
    empty = np.zeros((0, 3))
    good = finish_ref.finish_chunks([fine, fine], major, labels, [empty, empty], brute=True)
    for c in range(2):
        ref = reference_tail(fine, major[c], labels[c], empty, np.zeros(0, int), np.zeros(0, int), 0.6)
        np.testing.assert_array_equal(good[c]["fine_label"], ref["colors"])
    assert (good[0]["fine_label"] < 100).all() and (good[1]["fine_label"] >= 100).all()
    bad = finish_ref.finish_chunks([fine, fine], major, labels, [empty, empty], brute=True, variant="neighbour_chunk")
    assert (bad[0]["fine_label"] >= 100).any() and (bad[1]["fine_label"] < 100).any()


def test_rejects_ties_to_the_larger_index_and_a_missing_plus_one():
    major = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 2.0, 0], [2.0, 2.0, 0], [1.0, 1.0, 4.0]])
    fine = np.array([[1.0, 0, 0], [0.0, 1.0, 0], [1.0, 1.0, 0], [1.0, 2.0, 0], [1.75, 0.25, 0.0],
                     [1.0, 1.0, 3.5]])   # midpoints, and two plain points
    labels = np.array([4, 3, 2, 1, 0], np.int32)
    good = finish_ref.finish_chunk(fine, major, labels, np.zeros((0, 3)), brute=True)
    ref = reference_tail(fine, major, labels, np.zeros((0, 3)), np.zeros(0, int), np.zeros(0, int), 0.6)
    np.testing.assert_array_equal(good["fine_nn"], [0, 0, 0, 2, 1, 4])
    np.testing.assert_array_equal(good["fine_nn"], ref["nn"])                   # np.argmin: the first of the equal minima
    np.testing.assert_array_equal(good["fine_tied"], [1, 1, 3, 1, 0, 0])
    np.testing.assert_array_equal(good["merged_label"], labels[good["fine_nn"]] + 1)
    bad = finish_ref.finish_chunk(fine, major, labels, np.zeros((0, 3)), brute=True, variant="tie_larger")
    np.testing.assert_array_equal(bad["fine_nn"], [1, 2, 3, 3, 1, 4])
    flat = finish_ref.finish_chunk(fine, major, labels, np.zeros((0, 3)), brute=True, variant="no_plus_one")
    assert (flat["merged_label"] == 0).any() and not (good["merged_label"] == 0).any()   # group 0 would turn into "no instance"
    # the tree path reports the ties as brute force does
    big = np.concatenate([major, np.random.default_rng(3).random((50, 3)) + 10.0])
    t = finish_ref.finish_chunk(fine, big, np.arange(55, dtype=np.int32), np.zeros((0, 3)))
    np.testing.assert_array_equal(t["fine_nn"], [0, 0, 0, 2, 1, 4])
    np.testing.assert_array_equal(t["fine_tied"], [1, 1, 3, 1, 0, 0])
