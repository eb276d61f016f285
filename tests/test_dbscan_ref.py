"""CPU suite: the NumPy / SciPy restatement of rules D1-D5 (tests/dbscan_ref.py) against scikit-learn's own labels (the golden
tests/golden/dbscan_sklearn.npz, and live scikit-learn where it imports), against the brute-force form, and the label
post-processing of autoinst_amd.cluster_api (keep-largest, delimiter rows, ground) on hand-made labels, without a device."""
import os

import numpy as np
import pytest

import dbscan_ref
from conftest import GOLDEN


def golden_clouds():
    z = np.load(os.path.join(GOLDEN, "dbscan_sklearn.npz"))
    return [(str(z[f"name_{k}"]), z[f"points_{k}"], float(z[f"eps_{k}"]), int(z[f"min_samples_{k}"]), z[f"labels_{k}"], float(z[f"margin_{k}"]))
            for k in range(int(z["n_clouds"]))]


def test_golden_is_what_the_issue_asks_for():
    clouds = golden_clouds()
    assert len(clouds) >= 10
    assert {ms for _, _, _, ms, _, _ in clouds} == {1, 3, 20} and {eps for _, _, eps, _, _, _ in clouds} == {0.3, 0.5, 0.7}
    for name, p, eps, ms, labels, margin in clouds:
        assert p.dtype == np.float64 and p.shape[0] <= 1500 and labels.shape == (p.shape[0],)
        assert margin > 1e-9 or name.startswith("lattice")
    assert any(name.startswith("duplicates") for name, *_ in clouds)
    assert os.path.getsize(os.path.join(GOLDEN, "dbscan_sklearn.npz")) < 1 << 20


@pytest.mark.parametrize("k", range(11))
def test_restatement_equals_the_sklearn_golden(k):
    name, p, eps, ms, labels, _ = golden_clouds()[k]
    got, n_clusters, counts, sizes = dbscan_ref.dbscan(p, eps, ms)
    assert np.array_equal(got, labels), name
    assert n_clusters == labels.max() + 1
    assert np.array_equal(sizes, np.bincount(labels[labels >= 0], minlength=n_clusters))
    assert counts.max() <= ms and counts.min() >= 1


def test_golden_has_exactly_the_parametrised_clouds():
    assert len(golden_clouds()) == 11


@pytest.mark.parametrize("seed", range(6))
def test_restatement_equals_brute_force(seed):
    rng = np.random.default_rng(seed)
    n = int(rng.integers(1, 400))
    p = rng.normal(0, 1.0, (n, 3)) + rng.integers(0, 3, (n, 1)) * 2.0
    if seed % 2:
        p = np.concatenate([p, p[: n // 5]])
    for eps, ms in ((0.3, 1), (0.5, 3), (0.7, 20), (0.5, p.shape[0] + 1)):
        a, b = dbscan_ref.dbscan(p, eps, ms), dbscan_ref.dbscan_brute(p, eps, ms)
        assert a[1] == b[1]
        for x, y in zip((a[0], a[2], a[3]), (b[0], b[2], b[3])):
            assert x.dtype == y.dtype and np.array_equal(x, y)


def test_restatement_on_the_exact_eps_lattice_is_inclusive():
    """Neighbours at exactly eps count (D1); one ulp less and they do not."""
    g = np.stack(np.meshgrid(np.arange(4), np.arange(4), np.arange(2), indexing="ij"), -1).reshape(-1, 3) * 0.5
    lab, k, counts, _ = dbscan_ref.dbscan(g, 0.5, 4)
    assert k == 1 and (lab == 0).all() and (counts == 4).all()
    lab, k, counts, _ = dbscan_ref.dbscan(g, np.nextafter(0.5, 0), 2)
    assert k == 0 and (lab == -1).all() and (counts == 1).all()
    for eps in (0.5, np.nextafter(0.5, 0), np.nextafter(0.5, np.inf)):
        assert np.array_equal(dbscan_ref.dbscan(g, eps, 4)[0], dbscan_ref.dbscan_brute(g, eps, 4)[0])


def test_restatement_empty_and_single():
    lab, k, counts, sizes = dbscan_ref.dbscan(np.zeros((0, 3)), 0.5, 1)
    assert lab.shape == (0,) and k == 0 and counts.shape == (0,) and sizes.shape == (0,)
    lab, k, counts, sizes = dbscan_ref.dbscan(np.zeros((1, 3)), 0.5, 1)
    assert lab.tolist() == [0] and k == 1 and counts.tolist() == [1] and sizes.tolist() == [1]


@pytest.mark.parametrize("seed", range(4))
def test_restatement_equals_live_sklearn(seed):
    cluster = pytest.importorskip("sklearn.cluster")
    rng = np.random.default_rng(100 + seed)
    n = int(rng.integers(200, 1500))
    c = rng.uniform(-6, 6, (6, 3))
    p = c[rng.integers(0, 6, n)] + rng.normal(0, rng.uniform(0.2, 1.0), (n, 3))
    if seed == 0:
        p = np.concatenate([p, p[:100]])
    for eps, ms in ((0.3, 2), (0.5, 5), (0.7, 20)):
        d2 = dbscan_ref.d1_sq_dist(p[:, None, :], p[None, :, :])
        assert np.abs(d2 - eps * eps).min() > 1e-9 * eps * eps    # nobody's rounding decides
        assert np.array_equal(dbscan_ref.dbscan(p, eps, ms)[0], cluster.DBSCAN(eps=eps, min_samples=ms).fit(p).labels_)


# ----------------------------------------------------------------------------- the wrappers' label post-processing, no device
def test_keep_largest_ranks_by_size_then_label():
    from autoinst_amd import cluster_api
    labels = np.array([0, 0, 1, 1, 2, 2, 2, 3, -1, 4, 4], dtype=np.int32)
    sizes = np.array([2, 2, 3, 1, 2], dtype=np.int32)
    # ranking: 2 (3 points), then 0, 1, 4 (2 points each, label ascending), then 3
    for k, kept in ((0, []), (1, [2]), (2, [2, 0]), (3, [2, 0, 1]), (4, [2, 0, 1, 4]), (5, [0, 1, 2, 3, 4]), (9, [0, 1, 2, 3, 4])):
        got = cluster_api.keep_largest_labels(labels, sizes, k)
        want = np.where(np.isin(labels, kept), labels, -1)
        assert got.dtype == np.int32 and np.array_equal(got, want), k
        assert np.array_equal(got, dbscan_ref.keep_largest(labels, sizes, k))
    assert labels[7] == 3   # the input is not modified
    with pytest.raises(ValueError):
        cluster_api.keep_largest_labels(labels, sizes, -1)


def test_keep_largest_without_noise_keeps_cluster_zero():
    """The reference's lbls[1:] drops cluster 0 when no point is noise; this project does not."""
    from autoinst_amd import cluster_api
    labels = np.array([0, 0, 0, 1, 1], dtype=np.int32)
    assert np.array_equal(cluster_api.keep_largest_labels(labels, np.array([3, 2]), 1), [0, 0, 0, -1, -1])


def test_torch_stable_descending_sort_is_the_ranking():
    """The device branch of keep_largest_labels ranks with torch's stable descending sort: the same order as the host's."""
    torch = pytest.importorskip("torch")
    from autoinst_amd import cluster_api
    rng = np.random.default_rng(3)
    sizes = rng.integers(1, 4, 40)
    labels = np.repeat(np.arange(40), sizes)
    labels = np.concatenate([labels, -np.ones(7, dtype=labels.dtype)])[rng.permutation(labels.size + 7)].astype(np.int32)
    for k in (0, 1, 5, 17, 40, 50):
        want = dbscan_ref.keep_largest(labels, sizes, k)
        order = torch.sort(torch.as_tensor(sizes.astype(np.int32)), descending=True, stable=True).indices
        assert np.array_equal(order.numpy(), np.argsort(-sizes, kind="stable"))
        assert np.array_equal(cluster_api.keep_largest_labels(labels, sizes, k), want)


def _fake_cluster(calls):
    def cluster(p):
        calls.append(np.array(p))
        return np.arange(p.shape[0]) % 3 - 1
    return cluster


def test_delimiter_rows_keep_minus_inf_and_are_not_clustered():
    from autoinst_amd import cluster_api
    ps = np.arange(24, dtype=np.float64).reshape(6, 4)
    ps[1] = -np.inf
    ps[4] = -np.inf
    ps[5, 0] = -np.inf     # not a delimiter: only one entry
    calls = []
    got = cluster_api.delimited_labels(ps, _fake_cluster(calls))
    assert got.dtype == np.float64 and got.shape == (6,)
    assert np.array_equal(got, [-1.0, -np.inf, 0.0, 1.0, -np.inf, -1.0])
    assert len(calls) == 1 and np.array_equal(calls[0], ps[[0, 2, 3, 5], :3])
    with pytest.raises(ValueError):
        cluster_api.delimited_labels(np.zeros((4, 2)), _fake_cluster([]))


def test_ground_points_get_minus_ten():
    from autoinst_amd import cluster_api
    pts = np.arange(21, dtype=np.float64).reshape(7, 3)
    ground = np.array([[-10], [0], [-10], [1], [0], [-10], [5]])
    calls = []
    got = cluster_api.ground_labels(pts, ground, _fake_cluster(calls))
    assert got.dtype == np.float64 and got.shape == (7, 1)
    assert np.array_equal(got.reshape(-1), [-10.0, -1.0, -10.0, 0.0, 1.0, -10.0, -1.0])
    assert np.array_equal(calls[0], pts[[1, 3, 4, 6]])
    with pytest.raises(ValueError):
        cluster_api.ground_labels(pts, ground[:3], _fake_cluster([]))


def test_reference_wrappers_of_the_restatement_compose():
    rng = np.random.default_rng(5)
    p = np.concatenate([rng.normal(0, 0.2, (60, 3)), rng.normal(4, 0.2, (40, 3)), rng.uniform(-9, 9, (10, 3))])
    ps = np.concatenate([p[:50], np.full((1, 3), -np.inf), p[50:]])
    lab = dbscan_ref.clusters_dbscan(ps, 1, 0.7, 5)
    assert lab[50] == -np.inf and set(np.unique(lab[np.isfinite(lab)])) == {-1.0, 0.0}
    ground = np.zeros(ps.shape[0])
    ground[:5] = -10
    full = dbscan_ref.clusterize_pcd(ps, ground, 2, 0.7, 5)
    assert full.shape == (ps.shape[0], 1) and (full[:5] == -10).all() and full[50, 0] == -np.inf


def test_the_binding_keeps_the_rules_of_the_other_bindings():
    """cluster_api is a package (autoinst_amd/cluster_api/), so tests/test_buffers.py's walk over the *_api.py files does not see
    it: the same structure rules, applied here -- buffers, pointers and the wait for torch come from _buffers alone."""
    import re
    from conftest import ROOT
    src = open(os.path.join(ROOT, "autoinst_amd", "cluster_api", "__init__.py")).read()
    for pattern in (r"data_ptr\(", r"current_stream\(", r"\.synchronize\(", r"\.ctypes\.data_as", r"AI_MEM_(HOST|DEVICE)"):
        assert not re.search(pattern, src), pattern
    for helper in ("is_device_tensor", "place_of", "points_f64", "rows", "concat", "segmented", "offsets_of", "cat_int32", "grow"):
        assert not re.search(rf"^def {helper}\(", src, re.M), helper
    assert re.search(r"^from \.\._buffers import ", src, re.M) and "place.sync()" in src
