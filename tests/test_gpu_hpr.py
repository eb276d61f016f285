"""GPU suite: hidden point removal on the device (camera_api.visible_sets / hidden_point_removal_device, csrc/ai_hidden.hip)
against its NumPy restatement tests/hpr_ref.py -- equal sets everywhere, equal re-solve counts too -- and against the host
function over qhull where qhull defines a result."""
import numpy as np
import pytest

import camera_ref
import hpr_ref
from autoinst_amd import camera_api, synth
from autoinst_amd.config import CAM_IDS, HPR_RADIUS
from test_gpu_camera import bits_equal
from test_hpr_ref import around_camera, full_view_sample, rig_subsample, rig_view, shared_rig, two_layers, wall_and_plate

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def rig():
    return shared_rig()


@pytest.fixture(scope="module")
def subsample(rig):
    """3 000 points of the rig's chunk in the pcd frame (rows of the crop), and the restatement's sets for the rig's four views."""
    cloud = rig["pcd"][rig["chunk_indices"]]
    sel = np.random.default_rng(0).choice(cloud.shape[0], 3000, replace=False)
    return cloud[sel], hpr_ref.visible_sets(cloud[sel], rig["T_pcd2cam"])


def device_set(p, ctx, radius_factor=HPR_RADIUS, camera=(0.0, 0.0, 0.0)):
    return camera_api.hidden_point_removal_device(p, camera=camera, radius_factor=radius_factor, ctx=ctx)


def check_against_ref(p, ctx, radius_factor=HPR_RADIUS, qhull=True):
    """The device's set and statistics equal the restatement's; the set equals qhull's where qhull gives one."""
    st = {}
    ref = hpr_ref.hidden_point_removal(p, radius_factor=radius_factor, stats=st)
    T = np.eye(4)[None]
    sets, stats = camera_api.visible_sets(p, T, radius_factor=radius_factor, return_stats=True, ctx=ctx)
    assert sets[0].dtype == np.int64 and np.array_equal(sets[0], ref)
    assert stats[0].tolist() == [st["local_hidden"], st["resolves"], st["max_resolves"], st["at_camera"]]
    if qhull:
        try:
            hull = camera_api.hidden_point_removal(p, radius_factor=radius_factor)
        except Exception:   # noqa: BLE001 -- qhull defines nothing there
            return ref
        assert np.array_equal(ref, hull)
    return ref


@pytest.mark.parametrize("n", [4, 5, 63, 64, 65, 129, 300])
def test_small_clouds_around_the_camera(n, ctx):
    for seed in (0, 1):
        check_against_ref(around_camera(n, seed), ctx)


def test_occlusion_and_the_degenerate_cases(ctx):
    wall, plate = wall_and_plate()
    for factor in (2.0, 10.0, 1000.0):
        check_against_ref(np.concatenate([wall, plate]), ctx, radius_factor=factor)
    p = two_layers()
    ref = check_against_ref(p, ctx)
    assert 100 < ref.size < 310
    i, hidden = int(ref[0]), int(np.setdiff1d(np.arange(310), ref)[0])
    for extra in (p[i], p[hidden], 2.0 * p[i], 0.5 * p[i], np.zeros(3)):   # equal points, one direction, a point at the camera
        check_against_ref(np.concatenate([p, extra[None]]), ctx, qhull=False)
    cam = np.array([0.5, -0.25, 2.0])
    assert np.array_equal(device_set(p + cam, ctx, camera=cam), hpr_ref.hidden_point_removal(p + cam, camera=cam))
    perm = np.random.default_rng(1).permutation(310)
    assert np.array_equal(np.sort(perm[device_set(p[perm], ctx)]), ref)


def _cluster(direction, seed, spread=0.03, n_near=60, n_far=140):
    """Two depth layers around one direction, wider than a direction cell (1 / 32), the first point exactly on the direction:
    the near layer's points lie in the cells around the far points' cells."""
    rng = np.random.default_rng(seed)
    e0 = np.asarray(direction, dtype=np.float64)
    dirs = e0 + rng.uniform(-spread, spread, (n_near + n_far, 3))
    dirs /= np.linalg.norm(dirs, axis=1)[:, None]
    dist = np.concatenate([5.0 + 0.01 * rng.standard_normal(n_near), 10.0 + 0.01 * rng.standard_normal(n_far)])
    p = dirs * dist[:, None]
    p[0] = 5.0 * e0 / np.linalg.norm(e0)
    return p


def _on_cell_borders():
    """Directions on a face of the direction grid (one component a multiple of 1 / 32), on an edge (two components), and the six
    poles: the grid's corners on the sphere, where the tangent basis changes its axis."""
    out = []
    b, c = 0.25, 0.5   # (b + 1) * 32 = 40 and (c + 1) * 32 = 48: cell borders
    for axis in range(3):
        face = np.full(3, np.sqrt((1.0 - b * b) / 2.0))
        face[axis] = b
        out.append(("face%d" % axis, face))
        edge = np.full(3, np.sqrt(1.0 - b * b - c * c))
        edge[(axis + 1) % 3], edge[(axis + 2) % 3] = b, c
        out.append(("edge%d" % axis, edge))
        for sign in (1.0, -1.0):
            pole = np.zeros(3)
            pole[axis] = sign
            out.append(("pole%d%+d" % (axis, sign), pole))
    return out


@pytest.mark.parametrize("name,direction", _on_cell_borders(), ids=[n for n, _ in _on_cell_borders()])
def test_constraints_in_the_cells_around_the_query(name, direction, ctx):
    p = _cluster(direction, seed=len(name))
    cells = hpr_ref._cell(p / np.linalg.norm(p, axis=1)[:, None])
    assert len({tuple(c) for c in cells}) >= (4 if name.startswith("edge") or name.startswith("pole") else 2)
    ref = check_against_ref(p, ctx)
    assert 0 < ref.size < 200 and (ref >= 60).sum() < 140   # near points hide far ones
    behind = check_against_ref(np.concatenate([p, 2.0 * p[:1]]), ctx, qhull=False)   # straight behind the point on the direction
    assert np.array_equal(behind, ref)


def test_rig_subsample(rig, ctx):
    sub = rig_subsample(rig)
    ref = check_against_ref(sub, ctx)
    assert ref.size == 2513
    check_against_ref(sub, ctx, radius_factor=100.0)


@pytest.fixture(scope="module")
def full_view(ctx):
    """One full view (358 123 points) in the camera frame, the device's set of it and the restatement's flags of 400 sampled rows."""
    pc, rows, flags, _ = full_view_sample()
    return pc, device_set(pc, ctx), rows, flags


def test_full_rig_view_sample_equals_the_restatement(full_view):
    """At full density (local lists of thousands of constraints, the loop of kh_local over cells of more than 64 points, long
    chains of re-solves) the device's flags of 400 sampled rows are the restatement's, every one."""
    pc, got, rows, flags = full_view
    on_device = np.zeros(pc.shape[0], dtype=np.uint8)
    on_device[got] = 1
    differ = rows[on_device[rows] != flags]
    assert differ.size == 0, f"rows {differ.tolist()} differ from the restatement"
    assert 100 < flags.sum() < 300


def test_full_rig_view_against_qhull(full_view):
    """One full view (358 123 points) against qhull, at most 3 differences (1e-5 of n).  The comparison is per distinct location:
    this view holds 17 groups of 24 bit-equal points, qhull lists one vertex per location (which of the 24 is its own affair)
    and the rule makes equal points visible together (0 <= 0), so a visible group is 24 points here and 1 point there -- 184 raw
    differences in 8 visible groups, none of them a disagreement about a location.  Measured: 0 locations differ.
    `test_full_rig_view_without_duplicates_against_qhull` counts raw points."""
    pc, got = full_view[:2]
    assert pc.shape[0] == 358_123
    hull = camera_api.hidden_point_removal(pc, radius_factor=HPR_RADIUS)
    _, loc, size = np.unique(pc, axis=0, return_inverse=True, return_counts=True)
    loc = loc.reshape(-1)
    on_device, on_host = np.bincount(loc[got], minlength=size.shape[0]), np.bincount(loc[hull], minlength=size.shape[0])
    assert ((on_device == 0) | (on_device == size)).all()   # equal points are visible together
    assert (on_host <= 1).all()
    differ = np.flatnonzero((on_device > 0) != (on_host > 0))
    rows = np.flatnonzero(np.isin(loc, differ))
    print("full view: device", got.size, "qhull", hull.size, "raw differences", np.setxor1d(got, hull).size, "locations", differ.size)
    assert differ.size <= 3, f"{differ.size} locations differ from qhull, rows {rows.tolist()[:50]}"
    assert np.array_equal(np.setdiff1d(hull, got), []) and got.size - hull.size == int((size - 1)[on_host > 0].sum())
    assert 100_000 < got.size < 250_000


def test_full_rig_view_without_duplicates_against_qhull(full_view, ctx):
    """The same view with one point per distinct location (the first of each group of bit-equal points, in input order): there
    qhull defines every point's flag, and at most 3 raw points (1e-5 of n) may differ."""
    pc = full_view[0]
    first = np.sort(np.unique(pc, axis=0, return_index=True)[1])
    assert pc.shape[0] - 17 * 23 == first.size
    p = pc[first]
    got = device_set(p, ctx)
    hull = camera_api.hidden_point_removal(p, radius_factor=HPR_RADIUS)
    differ = np.setxor1d(got, hull)
    print("full view without duplicates: device", got.size, "qhull", hull.size, "differences", differ.size)
    assert differ.size <= 3, f"{differ.size} points differ from qhull: rows {differ.tolist()[:50]}"
    assert 100_000 < got.size < 250_000


@pytest.mark.parametrize("V", [1, 2, 4])
def test_views_in_one_call_equal_single_view_calls(V, rig, subsample, ctx):
    cloud, ref = subsample
    T = rig["T_pcd2cam"][:V]
    together = camera_api.visible_sets(cloud, T, ctx=ctx)
    assert len(together) == V
    for v in range(V):
        alone = camera_api.visible_sets(cloud, T[v:v + 1], ctx=ctx)[0]
        assert np.array_equal(together[v], alone) and np.array_equal(alone, ref[v])
        assert 0 < alone.size < 3000


def test_subset_equals_the_same_points_as_a_cloud(rig, subsample, ctx):
    cloud = rig["pcd"][rig["chunk_indices"]][:50_000]
    sel = np.sort(np.random.default_rng(3).choice(50_000, 2000, replace=False))
    T = rig["T_pcd2cam"][:2]
    with_subset = camera_api.visible_sets(cloud, T, subset=sel, ctx=ctx)
    as_cloud = camera_api.visible_sets(cloud[sel], T, ctx=ctx)
    for a, b in zip(with_subset, as_cloud):
        assert np.array_equal(a, sel[b]) and 0 < b.size < 2000
    unsorted = np.random.default_rng(4).permutation(sel)   # the rows come back ascending in the subset's order
    for a, b in zip(camera_api.visible_sets(cloud, T, subset=unsorted, ctx=ctx), as_cloud):
        assert np.array_equal(np.sort(a), sel[b])
    with pytest.raises(IndexError):
        camera_api.visible_sets(cloud, T, subset=np.array([0, 1, 2, 50_000]), ctx=ctx)
    assert np.array_equal(camera_api.visible_sets(cloud[sel], T, ctx=ctx)[1], as_cloud[1])   # the context is still usable


def test_skipped_views(rig, subsample, ctx):
    cloud, ref = subsample
    flat = np.zeros((4, 4))
    flat[:3, 3] = [1.0, 2.0, 3.0]
    flat[3, 3] = 1.0   # every point goes to (1, 2, 3): no extent
    T = np.stack([rig["T_pcd2cam"][0], flat, rig["T_pcd2cam"][1]])
    sets = camera_api.visible_sets(cloud, T, ctx=ctx)
    assert sets[1] is None and np.array_equal(sets[0], ref[0]) and np.array_equal(sets[2], ref[1])
    assert camera_api.visible_sets(cloud[:3], T, ctx=ctx) == [None, None, None]
    assert camera_api.visible_sets(np.zeros((0, 3)), T[:1], ctx=ctx) == [None]
    bad = cloud[:100].copy()
    bad[7, 1] = np.nan
    assert camera_api.visible_sets(bad, T[:1], ctx=ctx) == [None]
    with pytest.raises(ValueError):
        camera_api.hidden_point_removal_device(cloud[:3], ctx=ctx)
    tilted = rig["T_pcd2cam"][:1].copy()
    tilted[0, 3, 0] = 1e-3
    with pytest.raises(ValueError):   # a projective last row is refused, as ai_scan_pool refuses it
        camera_api.visible_sets(cloud, tilted, ctx=ctx)
    assert np.array_equal(camera_api.visible_sets(cloud, T[:1], ctx=ctx)[0], ref[0])


def test_device_tensors_give_the_same_indices(rig, subsample, ctx):
    import torch
    cloud, ref = subsample
    dev = torch.device("cuda", ctx.device)
    T = rig["T_pcd2cam"][:2]
    sets = camera_api.visible_sets(torch.as_tensor(cloud, device=dev), T, ctx=ctx)
    for v in range(2):
        assert sets[v].is_cuda and sets[v].dtype == torch.int64 and np.array_equal(sets[v].cpu().numpy(), ref[v])
    sel = np.arange(0, 3000, 2)
    host = camera_api.visible_sets(cloud, T, subset=sel, ctx=ctx)
    for sub in (torch.as_tensor(sel, device=dev), sel):
        got = camera_api.visible_sets(torch.as_tensor(cloud, device=dev), T, subset=sub, ctx=ctx)
        for v in range(2):
            assert np.array_equal(got[v].cpu().numpy(), host[v])
    one = camera_api.hidden_point_removal_device(torch.as_tensor(camera_api.transform_points(cloud, T[0]), device=dev), ctx=ctx)
    assert one.is_cuda and np.array_equal(one.cpu().numpy(), ref[0])


def test_dropin_with_the_device_removal(ctx):
    """image_based_features_per_patch(hpr="device") equals hpr="qhull" in all three return forms."""
    rig = synth.camera_rig(n_views=4, seed=3, query_voxel=0.35)
    ds = camera_ref.RigDataset(rig)
    cams = rig["cam_indices"][:2]
    base = (ds, rig["pcd"], rig["chunk_indices"], rig["points"], rig["T_pcd2world"], cams)
    kw = dict(cam_ids=CAM_IDS[:1], ctx=ctx)
    s_q, d_q = camera_api.image_based_features_per_patch(*base, hpr="qhull", **kw)
    s_d, d_d = camera_api.image_based_features_per_patch(*base, hpr="device", **kw)
    assert len(s_d) == len(d_d) == 1 and np.array_equal(s_d[0], s_q[0]) and bits_equal(d_d[0], d_q[0])
    assert (s_q[0] != -1).any() and (d_q[0] != 0).any()
    s_only = camera_api.image_based_features_per_patch(*base, sam=True, dino=False, hpr="device", **kw)
    assert np.array_equal(s_only[0], s_q[0])
    d_only, mask = camera_api.image_based_features_per_patch(*base, sam=False, dino=True, hpr="device", **kw)
    assert bits_equal(d_only[0], d_q[0]) and (mask == 0).all() and mask.shape == (len(rig["points"]),)
    with pytest.raises(ValueError):
        camera_api.image_based_features_per_patch(*base, hpr="open3d", **kw)
