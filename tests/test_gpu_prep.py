"""GPU suite: the chunk preparation on the device (autoinst_amd.prep_api, csrc/ai_prep.hip) against the CPU restatement
tests/prep_ref.py on a synthetic street (synth.street_map: ~1.7 M points, 5 chunks, both clouds) and on hand-made cases.

Tolerances: box select, the voxel means and their trace are bit-equal; against cKDTree the per-point kNN averages and the
threshold agree to rel 1e-12 (the distances are formed in another order than cKDTree's) and the kept sets are equal except for
points whose oracle avg lies within 1e-12 x threshold of the threshold -- that set is asserted empty on the fixture.  The kNN
itself is exact: on the hand-made clouds the averages equal the grid-free brute force `prep_cases.knn_avg_exact` bit for bit
(tests/test_gpu_prep_cases.py does the same at the kernel limits)."""
import numpy as np
import pytest

import prep_cases
import prep_ref
from autoinst_amd import prep_api, synth

pytestmark = pytest.mark.gpu

WORKERS = 16


@pytest.fixture(scope="module")
def street():
    m = synth.street_map(120.0, seed=0)
    centres, _ = prep_api.chunk_centres(m["T_pcd"], m["positions"], m["first_position"], m["indices"])
    m["boxes"] = [(c - 12.5, c + 12.5) for c in centres]
    return m


@pytest.fixture(scope="module")
def oracle(street):
    return prep_ref.chunk_and_downsample_point_clouds(street["nonground"], street["ground"], street["T_pcd"], street["positions"],
                                                      street["first_position"], street["indices"], street["labels"],
                                                      workers=WORKERS)


def test_box_select_is_bit_equal(street, ctx):
    assert len(street["boxes"]) == 5
    for cloud in ("nonground", "ground"):
        p = street[cloud]
        got = prep_api.box_select(p, [np.concatenate(b) for b in street["boxes"]], ctx=ctx)
        ref = prep_ref.box_select(p, street["boxes"])
        on_face = 0
        for g, r, (lo, hi) in zip(got, ref, street["boxes"]):
            assert g.dtype == np.int64 and r.size > 100_000
            np.testing.assert_array_equal(g, r)
            on_face += int(np.sum((p[:, 0] == lo[0]) | (p[:, 0] == hi[0])))
        assert on_face > 0   # the fixture has points exactly on box faces (and they are out)


def test_box_select_edge_cases(ctx):
    p = np.array([[0.0, 0, 0], [1.0, 0.5, 0.5], [0.5, 0.5, 0.5], [0.25, 0.5, 0.999999], [np.nan, 0.5, 0.5]])
    boxes = [np.r_[np.zeros(3), np.ones(3)], np.r_[np.full(3, 5.0), np.full(3, 6.0)], np.r_[np.full(3, -1.0), np.full(3, 2.0)]]
    a, b, c = prep_api.box_select(p, boxes, ctx=ctx)
    np.testing.assert_array_equal(a, [2, 3])
    assert b.size == 0
    np.testing.assert_array_equal(c, [0, 1, 2, 3])
    assert [x.size for x in prep_api.box_select(np.zeros((0, 3)), boxes, ctx=ctx)] == [0, 0, 0]


def _check_inliers(got_idx, got_avg, st, ref, tag):
    r_idx, r_avg, r_mean, r_std, r_thr = ref
    np.testing.assert_allclose(got_avg, r_avg, rtol=1e-12, atol=0.0, err_msg=tag)
    assert abs(st["threshold"] - r_thr) <= 1e-12 * abs(r_thr), tag
    near = np.where((r_avg > 0) & (np.abs(r_avg - r_thr) <= 1e-12 * abs(r_thr)))[0]   # avg == 0 is never kept
    print(f"{tag}: n={r_avg.size} kept={r_idx.size} avg==0: {int(np.sum(r_avg == 0))} near-threshold: {near.size}")
    assert near.size == 0, tag
    np.testing.assert_array_equal(got_idx, r_idx, err_msg=tag)


def test_statistical_inliers_on_the_street(street, oracle, ctx):
    for cloud in ("nonground", "ground"):
        p = street[cloud]
        ids_all = prep_ref.box_select(p, street["boxes"])
        zero = 0
        for c, ids in enumerate(ids_all):
            crop = p[ids]
            idx, avg, st = prep_api.statistical_inlier_indices(crop, 20, 2.0, return_stats=True, ctx=ctx)
            ref = prep_ref.statistical_from_avg(oracle["_avg"][cloud][c], 2.0)
            _check_inliers(idx, avg, st, (ref[0], oracle["_avg"][cloud][c], *ref[1:]), f"{cloud} chunk {c}")
            np.testing.assert_array_equal(idx, oracle["_inliers"][cloud][c])
            zero += int(np.sum(avg == 0))
            if c == 0:   # reproducible bit for bit
                idx2, avg2, st2 = prep_api.statistical_inlier_indices(crop, 20, 2.0, return_stats=True, ctx=ctx)
                np.testing.assert_array_equal(idx2, idx)
                assert avg2.tobytes() == avg.tobytes() and st2 == st
        assert zero > 0   # the repeated points: the avg == 0 rule fired


@pytest.mark.parametrize("nb", [1, 3, 20, 32, 64])
def test_statistical_inliers_hand_cases(nb, ctx):
    rng = np.random.default_rng(nb)
    p = rng.random((3000, 3)) * [6.0, 6.0, 0.5]
    p[:40] = p[40]                                       # 41 copies of one point: avg == 0 for every k <= 41
    p[-5:] = [[60.0, 0, 0], [0, -45.0, 3.0], [20.0, 30.0, 40.0], [-80.0, 1.0, 1.0], [-80.5, 1.0, 1.0]]   # far outliers
    idx, avg, st = prep_api.statistical_inlier_indices(p, nb, 2.0, return_stats=True, ctx=ctx)
    ref = prep_ref.statistical_inliers(p, nb, 2.0)
    _check_inliers(idx, avg, st, ref, f"hand nb={nb}")
    assert avg.tobytes() == prep_cases.knn_avg_exact(p, nb).tobytes()   # the exact kNN: no tolerance
    assert not np.isin(np.arange(2995, 3000), idx).any()
    if nb <= 41:
        assert np.all(avg[:41] == 0) and not np.isin(np.arange(41), idx).any()


def test_statistical_inliers_edge_cases(ctx):
    f = prep_api.statistical_inlier_indices
    assert f(np.zeros((0, 3)), ctx=ctx).size == 0                       # n = 0
    idx, avg, st = f(np.array([[1.0, 2.0, 3.0]]), return_stats=True, ctx=ctx)   # n = 1: avg 0, nothing kept
    assert idx.size == 0 and avg[0] == 0.0 and np.isnan(st["threshold"])
    assert f(np.array([[0.0, 0, 0], [1.0, 0, 0]]), ctx=ctx).size == 0   # std 0: threshold == every avg, strict <
    p = np.random.default_rng(1).random((12, 3))
    for nb in (20, 100):                                                 # nb_neighbors > n: k = n
        idx, avg, st = f(p, nb, 1.0, return_stats=True, ctx=ctx)
        _check_inliers(idx, avg, st, prep_ref.statistical_inliers(p, nb, 1.0, brute=True), f"nb={nb} > n")
        assert avg.tobytes() == prep_cases.knn_avg_exact(p, nb).tobytes()
    for nb, r in ((0, 2.0), (-3, 2.0), (20, 0.0), (20, -1.0)):
        with pytest.raises(ValueError):
            f(p, nb, r, ctx=ctx)
    with pytest.raises(ValueError):
        f(np.random.default_rng(2).random((100, 3)), 65, 2.0, ctx=ctx)   # k > 64


def test_voxel_down_sample_is_bit_equal(oracle, ctx):
    for cloud in ("nonground", "ground"):
        for c, chunk in enumerate(oracle[f"pcd_{cloud}_chunks"]):
            got, tr = prep_api.voxel_down_sample(chunk, 0.35, return_trace=True, ctx=ctx)
            ref, rtr = prep_ref.voxel_down_sample(chunk, 0.35)
            assert got.shape == ref.shape and got.shape[0] > 1000
            assert got.tobytes() == ref.tobytes(), f"{cloud} chunk {c}"
            np.testing.assert_array_equal(tr, rtr)


def test_voxel_down_sample_hand_cases(ctx):
    # points exactly on voxel borders (min bound 0, voxel 1 -> vmin -0.5: borders at 0.5, 1.5, ...), on all three axes
    p = np.array([[0.0, 0.0, 0.0], [0.5, 0.0, 0.0], [0.49999999999999994, 0.0, 0.0], [0.4, 0.0, 0.0], [1.5, 0.0, 0.0],
                  [0.0, 0.5, 0.0], [0.0, 0.0, 1.5], [0.0, 0.0, 1.4999999], [2.5, 2.5, 2.5]])
    got, tr = prep_api.voxel_down_sample(p, 1.0, return_trace=True, ctx=ctx)
    ref, rtr = prep_ref.voxel_down_sample(p, 1.0)
    assert got.tobytes() == ref.tobytes()
    np.testing.assert_array_equal(tr, rtr)
    np.testing.assert_array_equal(rtr[:5], [0, 4, 4, 0, 5])   # ascending (ix, iy, iz): voxel (1,0,0) after the x = 0 ones
    assert prep_api.voxel_down_sample(np.zeros((0, 3)), 0.35, ctx=ctx).shape == (0, 3)
    one, t1 = prep_api.voxel_down_sample(np.array([[1.0, 2.0, 3.0]]), 0.35, return_trace=True, ctx=ctx)
    np.testing.assert_array_equal(one, [[1.0, 2.0, 3.0]])
    assert t1.tolist() == [0]
    with pytest.raises(ValueError):
        prep_api.voxel_down_sample(p, 0.0, ctx=ctx)
    with pytest.raises(ValueError):
        prep_api.voxel_down_sample(np.array([[0.0, 0, 0], [1e7, 0, 0]]), 1e-5, ctx=ctx)   # index beyond the int range


def _same_chunks(a, b):
    assert len(a) == len(b)
    for x, y in zip(a, b):
        x = x.cpu().numpy() if hasattr(x, "cpu") else np.asarray(x)
        assert x.tobytes() == np.ascontiguousarray(y, dtype=x.dtype).tobytes()


def _compare_dict(got, ref):
    for k in ("pcd_nonground_chunks", "pcd_ground_chunks", "pcd_nonground_chunks_major_downsampling",
              "pcd_ground_chunks_major_downsampling", "indices", "indices_ground"):
        _same_chunks(got[k], ref[k])
    for k in ("center_positions", "center_ids", "obbs"):
        _same_chunks([np.asarray(v) for v in got[k]], ref[k])
    for (a0, a1), (b0, b1) in zip(got["chunk_bounds"], ref["chunk_bounds"]):
        np.testing.assert_array_equal(a0, b0)
        np.testing.assert_array_equal(a1, b1)
    for cloud in ("nonground", "ground"):
        assert got["kitti_labels"][cloud]["panoptic"] == []
        for k in ("semantic", "instance"):
            _same_chunks(got["kitti_labels"][cloud][k], ref["kitti_labels"][cloud][k])
    assert set(got) == set(ref) - {"_inliers", "_avg"}


def test_chunk_and_downsample_matches_the_oracle(street, oracle, ctx):
    got = prep_api.chunk_and_downsample_point_clouds(street["nonground"], street["ground"], street["T_pcd"], street["positions"],
                                                     street["first_position"], street["indices"], street["labels"], ctx=ctx)
    _compare_dict(got, oracle)


def test_device_tensors_through_run_chunks(street, oracle, ctx):
    import torch
    from autoinst_amd import sharding
    from autoinst_amd.config import CONFIG_SPATIAL

    dev = torch.device("cuda", ctx.device)
    labels = {k: torch.as_tensor(v, device=dev) for k, v in street["labels"].items()}
    got = prep_api.chunk_and_downsample_point_clouds(torch.as_tensor(street["nonground"], device=dev),
                                                     torch.as_tensor(street["ground"], device=dev), street["T_pcd"],
                                                     street["positions"], street["first_position"], street["indices"], labels,
                                                     ctx=ctx)
    major = got["pcd_nonground_chunks_major_downsampling"]
    assert all(m.is_cuda for m in major) and all(x.is_cuda for x in got["kitti_labels"]["nonground"]["instance"])
    _compare_dict(got, oracle)
    cfg = dict(alpha=CONFIG_SPATIAL["alpha"], theta=0.0, gamma=0.0, T=CONFIG_SPATIAL["T"])
    lab_dev = sharding.run_chunks([(m, None) for m in major], **cfg)
    lab_ref = sharding.run_chunks([(m, None) for m in oracle["pcd_nonground_chunks_major_downsampling"]], **cfg)
    for a, b in zip(lab_dev, lab_ref):
        np.testing.assert_array_equal(np.asarray(a), np.asarray(b))
