"""GPU suite: the camera projection on the device (autoinst_amd.camera_api, csrc/ai_camera.hip) against the CPU restatement
tests/camera_ref.py.  Pixels, SAM labels, the DINOv2 means and their view counts are bit-equal everywhere: on the synthetic
rig (synth.camera_rig: ~33 k points and 200 k points, 29 views), on hand-made cases with an identity transform and a diagonal
K, on a sweep over every pixel, and through the drop-in image_based_features_per_patch against the reference's control flow."""
import numpy as np
import pytest

import camera_ref
import prep_ref
from autoinst_amd import camera_api, ncuts_api, prep_api, synth

pytestmark = pytest.mark.gpu

MAXD = camera_ref.MAX_DIST


def bits_equal(a, b):
    a, b = np.asarray(a), np.asarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return np.array_equal(a, b)
    nan = np.isnan(a)
    return np.array_equal(nan, np.isnan(b)) and np.array_equal(a[~nan].view(np.uint64), b[~nan].view(np.uint64))


def assert_same(got, ref, V):
    assert bits_equal(got["pixels"], ref["pixels"])
    for k in ("sam", "dino_views"):
        if ref[k] is not None:
            assert bits_equal(got[k], ref[k].astype(np.int32)), k
    if ref["dino"] is not None:
        assert bits_equal(got["dino"], ref["dino"])


@pytest.fixture(scope="module")
def rig():
    return synth.camera_rig(n_views=29, seed=0)


def _rig_inputs(rig):
    cloud = rig["pcd"][rig["chunk_indices"]]
    vis = [np.where(m[rig["chunk_indices"]])[0] for m in rig["hpr_masks"]]
    return cloud, vis


def test_rig_chunk_29_views(rig, ctx):
    cloud, vis = _rig_inputs(rig)
    pts = rig["points"]
    assert pts.shape[0] > 25_000 and len(vis) == 29
    args = (pts, cloud, vis, rig["T_pcd2cam"], rig["K"], rig["image_hw"])
    got = camera_api.camera_features(*args, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"], return_pixels=True, ctx=ctx)
    ref = camera_ref.camera_features(*args, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"], check_mean_rows=2000)
    assert_same(got, ref, 29)
    has = ref["pixels"][:, :, 0] >= 0
    assert has.any(axis=1).mean() > 0.5 and has.sum() > 100_000
    assert (ref["dino_views"] < has.sum(axis=1)).any()   # zero and -0.0 rows stayed out of the mean
    # without maps / without SAM: the same pixels, and the other outputs are None
    only = camera_api.camera_features(*args, return_pixels=True, ctx=ctx)
    assert only["dino"] is None and only["sam"] is None and bits_equal(only["pixels"], ref["pixels"])


def test_rig_200k_queries_29_views(rig, ctx):
    cloud, vis = _rig_inputs(rig)
    rng = np.random.default_rng(7)
    q = cloud[rng.choice(cloud.shape[0], 200_000, replace=False)] + rng.normal(0.0, 0.05, (200_000, 3))
    args = (q, cloud, vis, rig["T_pcd2cam"], rig["K"], rig["image_hw"])
    got = camera_api.camera_features(*args, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"], return_pixels=True, ctx=ctx)
    ref = camera_ref.camera_features(*args, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"])
    assert_same(got, ref, 29)
    assert (ref["pixels"][:, :, 0] >= 0).any(axis=1).mean() > 0.5


def test_device_tensors_give_the_same_result(rig, ctx):
    import torch
    cloud, vis = _rig_inputs(rig)
    dev = torch.device("cuda", ctx.device)
    args = (rig["points"], cloud, vis, rig["T_pcd2cam"], rig["K"], rig["image_hw"])
    host = camera_api.camera_features(*args, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"], return_pixels=True, ctx=ctx)
    d = camera_api.camera_features(torch.as_tensor(rig["points"], device=dev), torch.as_tensor(cloud, device=dev),
                                   [torch.as_tensor(v, device=dev) for v in vis], rig["T_pcd2cam"], rig["K"], rig["image_hw"],
                                   feature_maps=torch.as_tensor(rig["feature_maps"], device=dev),
                                   sam_images=torch.as_tensor(rig["sam_images"], device=dev), return_pixels=True, ctx=ctx)
    for k in ("dino", "dino_views", "sam", "pixels"):
        assert d[k].is_cuda and bits_equal(d[k].cpu().numpy(), host[k]), k


def test_non_contiguous_and_per_view_device_maps(rig, ctx):
    """Maps handed over as views of other device tensors (a channel-first DINOv2 output permuted to channel-last, transposed SAM
    images) and as lists of per-view device tensors: the copies that make them contiguous are queued on torch's stream, and the
    library must read them only once they are done.  Bit-equal to the host inputs' result."""
    import torch
    cloud, vis = _rig_inputs(rig)
    dev = torch.device("cuda", ctx.device)
    fixed = (rig["T_pcd2cam"], rig["K"], rig["image_hw"])
    host = camera_api.camera_features(rig["points"], cloud, vis, *fixed, feature_maps=rig["feature_maps"], sam_images=rig["sam_images"],
                                      return_pixels=True, ctx=ctx)
    q_d, c_d = torch.as_tensor(rig["points"], device=dev), torch.as_tensor(cloud, device=dev)
    fm_cf = torch.as_tensor(np.ascontiguousarray(rig["feature_maps"].transpose(0, 3, 1, 2)), device=dev)   # (V, F, fh, fw)
    sam_t = torch.as_tensor(np.ascontiguousarray(rig["sam_images"].transpose(0, 2, 1)), device=dev)       # (V, w, h)
    fm, sm = fm_cf.permute(0, 2, 3, 1), sam_t.transpose(1, 2)
    assert not fm.is_contiguous() and not sm.is_contiguous()
    for maps, sams in ((fm, sm), (list(fm.unbind(0)), list(sm.unbind(0)))):
        d = camera_api.camera_features(q_d, c_d, vis, *fixed, feature_maps=maps, sam_images=sams, return_pixels=True, ctx=ctx)
        for k in ("dino", "dino_views", "sam", "pixels"):
            assert bits_equal(d[k].cpu().numpy(), host[k]), k
    with pytest.raises(ValueError):   # device maps with host points
        camera_api.camera_features(rig["points"], cloud, vis, *fixed, feature_maps=fm, ctx=ctx)
    with pytest.raises(ValueError):   # a list mixing host and device maps
        camera_api.camera_features(q_d, c_d, vis, *fixed, feature_maps=[rig["feature_maps"][0]] + list(fm.unbind(0))[1:], ctx=ctx)


def _ident(V):
    return np.repeat(np.eye(4)[None], V, 0)


def test_half_pixel_ties_and_w(ctx):
    """Identity transform, K = I, a 10 x 10 image: u = rint(x / z)."""
    pts = np.array([[2.5, 0.0, 1.0], [3.5, 0.0, 1.0], [-0.4, 0.0, 1.0], [-0.6, 0.0, 1.0], [9.5, 0.5, 1.0], [8.5, 1.5, 1.0],
                    [-0.5, 2.5, 1.0], [1.0, 1.0, 0.0], [1.0, 1.0, -1.0], [4.0, 4.0, 4.0], [-4.0, -4.0, -4.0]])
    K = np.eye(3)
    r = camera_api.camera_features(pts, pts, [np.arange(len(pts))], _ident(1), K, (10, 10), return_pixels=True, ctx=ctx)
    ref = camera_ref.camera_features(pts, pts, [np.arange(len(pts))], _ident(1), K, (10, 10))
    assert bits_equal(r["pixels"], ref["pixels"])
    px = r["pixels"][:6, 0].tolist()
    assert px == [[2, 0], [4, 0], [0, 0], [-1, -1], [-1, -1], [8, 2]]
    # a 9-wide image keeps u = rint(8.5) = 8 and drops rint(9.5) = 10; w' = 0 and w' < 0 are dropped
    r9 = camera_api.camera_features(pts[:6], pts[:6], [np.arange(6)], _ident(1), K, (10, 9), return_pixels=True, ctx=ctx)
    assert r9["pixels"][:, 0].tolist() == [[2, 0], [4, 0], [0, 0], [-1, -1], [-1, -1], [8, 2]]
    zw = np.array([[1.0, 1.0, 0.0], [1.0, 1.0, -1.0], [0.0, 0.0, -0.0]])
    rz = camera_api.camera_features(zw, zw, [np.arange(3)], _ident(1), K, (10, 10), return_pixels=True, ctx=ctx)
    assert (rz["pixels"] == -1).all()


def test_distance_one_ulp_from_max_dist(ctx):
    """A cloud point at distance nextafter(max_dist, 0) sees the query; at max_dist and one ulp above it does not."""
    q = np.array([[0.0, 0.5, 2.0]])
    ds = [np.nextafter(MAXD, 0.0), MAXD, np.nextafter(MAXD, 1.0)]
    cloud = np.array([[d, 0.5, 2.0] for d in ds] + [[-d, 0.5, 2.0] for d in ds] + [[0.0, 0.5, 2.0 + d] for d in ds])
    vis = [np.array([k]) for k in range(9)]
    K = np.diag([100.0, 100.0, 1.0])
    r = camera_api.camera_features(q, cloud, vis, _ident(9), K, (200, 200), return_pixels=True, ctx=ctx)
    ref = camera_ref.camera_features(q, cloud, vis, _ident(9), K, (200, 200))
    assert bits_equal(r["pixels"], ref["pixels"])
    # along x the difference is d itself (q.x = 0); along z, 2 + d is rounded first, so only the restatement decides there
    assert (r["pixels"][0, :6, 0] >= 0).tolist() == [True, False, False] * 2
    # the same at a large offset: the pcd-frame search radius must cover the camera-frame rounding
    T = _ident(9)
    T[:, :3, 3] = [1234.5, -987.25, 3.0]
    r2 = camera_api.camera_features(q, cloud, vis, T, K, (200, 200), return_pixels=True, ctx=ctx)
    ref2 = camera_ref.camera_features(q, cloud, vis, T, K, (200, 200))
    assert bits_equal(r2["pixels"], ref2["pixels"])


def _feature_case(fdim, rng):
    """5 x 7 map per view over a 50 x 70 image (K = I: pixel = (x, y)); cells: zero, -0.0, one NaN, random."""
    V, fh, fw = 3, 5, 7
    maps = rng.standard_normal((V, fh, fw, fdim)).astype(np.float32)
    maps[0, 0, 0] = 0.0
    maps[1, 0, 0] = -0.0
    maps[2, 0, 0, fdim - 1] = np.nan
    maps[:, 1, 1] = 0.0
    maps[0, 1, 1, fdim // 2] = -0.0
    maps[1, 1, 1, fdim - 1] = 1e-30
    sam = rng.integers(0, 4, (V, 50, 70)).astype(np.int32)
    px = np.array([[1, 1], [15, 15], [69, 49], [0, 0], [30, 20], [12, 12], [55, 5]], dtype=np.float64)
    pts = np.stack([px[:, 0], px[:, 1], np.ones(len(px))], 1)
    return pts, maps, sam


@pytest.mark.parametrize("fdim", [100, 384, 500])
def test_feature_rows_zero_negzero_nan(fdim, ctx):
    rng = np.random.default_rng(fdim)
    pts, maps, sam = _feature_case(fdim, rng)
    vis = [np.arange(len(pts)), np.arange(len(pts)), np.arange(len(pts))]
    args = (pts, pts, vis, _ident(3), np.eye(3), (50, 70))
    got = camera_api.camera_features(*args, feature_maps=maps, sam_images=sam, return_pixels=True, ctx=ctx)
    ref = camera_ref.camera_features(*args, feature_maps=maps, sam_images=sam, check_mean_rows=len(pts))
    assert_same(got, ref, 3)
    # cell (0, 0): zero in view 0, -0.0 in view 1, a NaN in view 2; cell (1, 1): zero, -0.0 and one 1e-30 element
    assert got["dino_views"].tolist()[:4] == [1, 1, 3, 1]
    assert np.isnan(got["dino"][:, fdim - 1]).sum() == 2   # the NaN of view 2's cell (0, 0) entered the means of the points on it
    assert (got["sam"] == -1).any() and (got["sam"] > 0).any()


def test_empty_views_and_sizes(ctx):
    rng = np.random.default_rng(9)
    pts, maps, sam = _feature_case(64, rng)
    n = len(pts)
    empty = np.zeros(0, np.int64)
    for vis in ([np.arange(n), empty, np.arange(n)], [empty, empty, empty]):
        args = (pts, pts, vis, _ident(3), np.eye(3), (50, 70))
        got = camera_api.camera_features(*args, feature_maps=maps, sam_images=sam, return_pixels=True, ctx=ctx)
        ref = camera_ref.camera_features(*args, feature_maps=maps, sam_images=sam)
        assert_same(got, ref, 3)
        assert (got["pixels"][:, 1] == -1).all() and (got["sam"][:, 1] == -1).all()
    assert (got["dino"] == 0).all() and not np.signbit(got["dino"]).any() and (got["dino_views"] == 0).all()
    # an empty cloud, N = 0, V = 1
    got = camera_api.camera_features(pts, np.zeros((0, 3)), [empty] * 3, _ident(3), np.eye(3), (50, 70), feature_maps=maps,
                                     sam_images=sam, return_pixels=True, ctx=ctx)
    assert (got["pixels"] == -1).all() and (got["dino_views"] == 0).all()
    got = camera_api.camera_features(np.zeros((0, 3)), pts, vis, _ident(3), np.eye(3), (50, 70), feature_maps=maps, sam_images=sam,
                                     return_pixels=True, ctx=ctx)
    assert got["dino"].shape == (0, 64) and got["sam"].shape == (0, 3) and got["pixels"].shape == (0, 3, 2)
    args = (pts, pts, [np.arange(n)], _ident(1), np.eye(3), (50, 70))
    got = camera_api.camera_features(*args, feature_maps=maps[:1], sam_images=sam[:1], return_pixels=True, ctx=ctx)
    assert_same(got, camera_ref.camera_features(*args, feature_maps=maps[:1], sam_images=sam[:1]), 1)
    with pytest.raises(ValueError):
        camera_api.camera_features(pts, pts, [np.arange(n)] * 65, _ident(65), np.eye(3), (50, 70), ctx=ctx)
    with pytest.raises(ValueError):
        camera_api.camera_features(*args, sam_images=sam[:1, :40], ctx=ctx)
    with pytest.raises(ValueError):
        camera_api.camera_features(pts, pts, [np.arange(n)] * 2, _ident(2), np.eye(3), (50, 70), feature_maps=[maps[0], maps[1, :4]],
                                   ctx=ctx)


def test_feature_cell_out_of_range_raises(ctx):
    pts = np.array([[1.0, 1.0, 1.0]])
    maps = np.zeros((1, 0, 5, 8), np.float32)
    with pytest.raises(IndexError):
        camera_api.camera_features(pts, pts, [np.array([0])], _ident(1), np.eye(3), (4, 4), feature_maps=maps, ctx=ctx)
    with pytest.raises(IndexError):
        camera_ref.camera_features(pts, pts, [np.array([0])], _ident(1), np.eye(3), (4, 4), feature_maps=maps)
    # not projected: nothing is read, nothing raises
    r = camera_api.camera_features(pts, pts, [np.array([0])], _ident(1), np.eye(3), (1, 1), feature_maps=maps, ctx=ctx)
    assert r["dino_views"].tolist() == [0]


def test_pixel_sweep_feature_cells(ctx):
    """One point on every pixel of a 376 x 1241 image (K = I, z = 1); each cell's row holds (row + 1, column + 1): the cell the
    device reads is (int(27 / 376 * v), int(88 / 1241 * u)) for every row v and column u."""
    h, w, fh, fw = 376, 1241, 27, 88
    vv, uu = np.meshgrid(np.arange(h), np.arange(w), indexing="ij")
    pts = np.stack([uu.ravel(), vv.ravel(), np.ones(h * w)], 1).astype(np.float64)
    maps = np.zeros((1, fh, fw, 2), np.float32)
    maps[0, :, :, 0] = np.arange(1, fh + 1)[:, None]
    maps[0, :, :, 1] = np.arange(1, fw + 1)[None, :]
    r = camera_api.camera_features(pts, pts, [np.arange(h * w)], _ident(1), np.eye(3), (h, w), feature_maps=maps, return_pixels=True,
                                   ctx=ctx)
    assert (r["dino_views"] == 1).all()
    assert np.array_equal(r["pixels"][:, 0, 0], uu.ravel()) and np.array_equal(r["pixels"][:, 0, 1], vv.ravel())
    f0, f1 = fh / h, fw / w
    rows = np.array([int(f0 * v) for v in range(h)])
    cols = np.array([int(f1 * u) for u in range(w)])
    assert np.array_equal(r["dino"][:, 0].reshape(h, w), np.repeat(rows[:, None] + 1.0, w, 1))
    assert np.array_equal(r["dino"][:, 1].reshape(h, w), np.repeat(cols[None, :] + 1.0, h, 0))


@pytest.fixture(scope="module")
def small_rig():
    return synth.camera_rig(n_views=4, seed=3, query_voxel=0.35)


def _dropin_ref(rig, dataset, inliers, cam_indices, hpr_masks, sam, dino, hpr=None):
    return camera_ref.image_based_features_per_patch(dataset, rig["pcd"], rig["chunk_indices"], rig["points"], rig["T_pcd2world"],
                                                     cam_indices, hpr_masks=hpr_masks, sam=sam, dino=dino, inliers=inliers, hpr=hpr)


def test_dropin_return_forms_with_given_hpr(small_rig, ctx):
    rig = small_rig
    ds = camera_ref.RigDataset(rig)
    chunk = rig["pcd"][rig["chunk_indices"]]
    inl = prep_ref.statistical_inliers(chunk, workers=16)[0]
    assert np.array_equal(np.asarray(prep_api.statistical_inlier_indices(chunk, ctx=ctx)), inl)
    base = (ds, rig["pcd"], rig["chunk_indices"], rig["points"], rig["T_pcd2world"], rig["cam_indices"])
    masks = rig["hpr_masks"].copy()
    masks[2] = False   # an "out of view skip"
    s_ref, d_ref = _dropin_ref(rig, ds, inl, rig["cam_indices"], masks, True, True)
    s, d = camera_api.image_based_features_per_patch(*base, hpr_masks=masks, ctx=ctx)
    assert len(s) == len(d) == 1 and s[0].dtype == s_ref[0].dtype and np.array_equal(s[0], s_ref[0])
    assert d[0].shape == (len(rig["points"]), 4, 384) and bits_equal(d[0], d_ref[0])
    assert (s[0][:, 2] == -1).all() and (d[0][:, 2] == 0).all() and (s[0] > 0).any()
    s_only = camera_api.image_based_features_per_patch(*base, hpr_masks=masks, sam=True, dino=False, ctx=ctx)
    assert np.array_equal(s_only[0], s_ref[0])
    d_only, vis = camera_api.image_based_features_per_patch(*base, hpr_masks=masks, sam=False, dino=True, ctx=ctx)
    assert bits_equal(d_only[0], d_ref[0]) and (vis == 0).all() and vis.shape == (len(rig["points"]),)
    s_m, d_m = camera_api.image_based_features_per_patch(*base, hpr_masks=masks, dino_mean=True, ctx=ctx)
    assert bits_equal(d_m[0], camera_ref.dinov2_mean(d_ref[0])) and np.array_equal(s_m[0], s_ref[0])
    with pytest.raises(NotImplementedError):
        camera_api.image_based_features_per_patch(*base, hpr_masks=masks, rm_perp=0.1, ctx=ctx)
    with pytest.raises(NotImplementedError):
        camera_api.image_based_features_per_patch(*base, hpr_masks=masks, vis=True, ctx=ctx)


def test_dropin_with_computed_hpr(small_rig, ctx):
    rig = small_rig
    ds = camera_ref.RigDataset(rig)
    cams = rig["cam_indices"][:2]
    chunk = rig["pcd"][rig["chunk_indices"]]
    inl = np.asarray(prep_api.statistical_inlier_indices(chunk, ctx=ctx))
    s_ref, d_ref = _dropin_ref(rig, ds, inl, cams, None, True, True, hpr=camera_api.hidden_point_removal)
    s, d = camera_api.image_based_features_per_patch(ds, rig["pcd"], rig["chunk_indices"], rig["points"], rig["T_pcd2world"], cams,
                                                     ctx=ctx)
    assert np.array_equal(s[0], s_ref[0]) and bits_equal(d[0], d_ref[0])
    assert (s[0] != -1).any() and (d[0] != 0).any()


def test_affinity_on_projected_features(rig, ctx):
    """build_affinity with the tri-modal weights on the device's means gives the graph it gives on the restatement's."""
    cloud, vis = _rig_inputs(rig)
    args = (rig["points"], cloud, vis, rig["T_pcd2cam"], rig["K"], rig["image_hw"])
    got = camera_api.camera_features(*args, feature_maps=rig["feature_maps"], ctx=ctx)
    ref = camera_ref.camera_features(*args, feature_maps=rig["feature_maps"])
    tarl = synth.surrogate_features(np.arange(len(rig["points"])) // 50, 96, 0)
    graphs = []
    for dino in (got["dino"], ref["dino"]):
        g = ncuts_api.build_affinity(rig["points"], tarl, dino, alpha=1.0, theta=0.5, gamma=0.1, ctx=ctx)
        try:
            graphs.append(g.to_scipy())
        finally:
            g.free()
    a, b = graphs
    assert a.nnz > 0 and np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices)
    assert np.array_equal(a.data.view(np.uint64), b.data.view(np.uint64))
