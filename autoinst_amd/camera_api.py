"""The camera projection of the tri-modal configuration: ``image_based_features_per_patch`` and ``dinov2_mean``
(``pipeline/utils/image/image_utils.py:89-371``, with ``point_to_pixel`` of ``point_to_pixels.py:6-35``) on the device.

* `camera_features` -- the array-level, fused path: for every chunk point and view, whether a visible point of the view lies
  within ``max_dist`` of it in the camera frame, its pixel, its SAM label, and the mean DINOv2 feature over the views
  (``csrc/ai_camera.hip``; rules in DESIGN.md section 12).  No (N, V, F) block is formed;
* `image_based_features_per_patch` -- the reference's function with its positional arguments and its three return forms; the
  per-view host steps (poses, hidden point removal, the crop and the inlier intersection) stay in Python, the per-point search,
  projection and gathers run in one `camera_features` call per camera;
* `hidden_point_removal` -- open3d 0.17 ``PointCloud::HiddenPointRemoval`` restated on the host over scipy's qhull;
* `hidden_point_removal_device`, `visible_sets` -- the same visible sets on the device, one linear program in two unknowns per
  point instead of a hull (``csrc/ai_hidden.hip``; rules H1-H6 in ``include/autoinst_hip.h``), all views of
  a chunk in one call;
* `masks_to_image` -- ``image_utils.py:44-52``.

Inputs are NumPy arrays; `camera_features` also takes float64 torch tensors on the context's GPU (then every array input and
every output is a device tensor).  There is no CPU fallback.
"""
from __future__ import annotations

import numpy as np

from . import _ffi
from .config import CAM_IDS, HPR_RADIUS, MAJOR_VOXEL_SIZE, NUM_DINO_FEATURES
from ._buffers import cat_int32, place_of, points_f64
from .ncuts_api import Context, _is_device_tensor, default_context

MAX_VIEWS = 64
_CAMS = ("cam2", "cam3")   # image_utils.py:103


def transform_points(points, T):
    """open3d ``PointCloud.transform`` in a fixed order: row r of the result is ``((T[r,0]*x + T[r,1]*y) + T[r,2]*z) + T[r,3]``,
    divided by row 3 -- element-wise, each step rounded on its own (the order the device uses)."""
    # rounds differently from `points_api._transform_points` (a matrix product) on purpose: the two stay two functions
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    T = np.asarray(T, dtype=np.float64)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    rows = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(4)]
    return np.stack([rows[0] / rows[3], rows[1] / rows[3], rows[2] / rows[3]], 1)


def masks_to_image(masks):
    """``masks_to_image`` (``image_utils.py:44-52``): a label per pixel, ``i + 1`` for mask i, the last mask winning, 0 where none."""
    image_labels = np.zeros(np.asarray(masks[0]["segmentation"]).shape)
    for i, mask in enumerate(masks):
        image_labels[np.asarray(mask["segmentation"], dtype=bool)] = i + 1
    return image_labels


def hidden_point_removal(points, camera=(0.0, 0.0, 0.0), radius_factor=HPR_RADIUS):
    """Ascending indices of the points visible from ``camera``: open3d 0.17 ``HiddenPointRemoval`` as its source is written,
    called the way ``hidden_point_removal_o3d`` (``pipeline/utils/image/hidden_points_removal.py:6-24``) calls it.

    ``radius = radius_factor * ||max_bound - min_bound||``; every point p (relative to the camera) is flipped to
    ``p + 2 (radius - |p|) p / |p|`` (``|p| = 0`` counts as 1e-4); the origin is appended; the visible points are the vertices of
    the convex hull of that set (qhull with "Qt", through ``scipy.spatial.ConvexHull``) other than the origin.  open3d lists them
    in hull order; the reference only intersects them with a set, so they are sorted here.  Raises what qhull raises (too few
    or degenerate points), as open3d does.

    Not checked against open3d: open3d is not installed where this project is tested.  tests/test_camera_ref.py checks it
    against a brute-force hull-vertex test (a linear program per point) instead.
    """
    from scipy.spatial import ConvexHull
    p = np.asarray(points, dtype=np.float64).reshape(-1, 3)
    if p.shape[0] == 0:
        raise ValueError("hidden_point_removal: no points")
    diameter = np.linalg.norm(p.max(axis=0) - p.min(axis=0))
    radius = diameter * radius_factor
    if not radius > 0:
        raise ValueError("hidden_point_removal: radius must be positive")
    rel = p - np.asarray(camera, dtype=np.float64)
    norm = np.sqrt(np.einsum("ij,ij->i", rel, rel))
    norm[norm == 0] = 0.0001
    flipped = rel + (2 * (radius - norm))[:, None] * rel / norm[:, None]
    hull = ConvexHull(np.concatenate([flipped, np.zeros((1, 3))]), qhull_options="Qt")
    v = np.unique(hull.vertices)
    return v[v != p.shape[0]].astype(np.int64)


def visible_sets(cloud, T_pcd2cam, *, subset=None, radius_factor=HPR_RADIUS, return_stats=False, ctx: Context | None = None):
    """The points of ``cloud`` visible from the camera of each of V views, on the device (`ai_hidden_points`): per view the
    ascending int64 rows of ``cloud``, or None for a view the removal skips (fewer than 4 points, all points equal, a
    coordinate that is not finite, or a sphere that does not hold the points: where `hidden_point_removal` raises, the
    reference's "hpr skip").  One library call serves all views.

    cloud (M, 3): points in the pcd frame, a NumPy array or a float64 tensor on the context's GPU (then the index arrays are
    device tensors too); T_pcd2cam: V 4x4 transforms (last row 0 0 0 1); subset: rows of ``cloud`` the removal is run on (the
    reference's ``bound_indices``), all rows when None.  With ``return_stats`` the result is ``(sets, stats)``, ``stats`` (V, 4)
    int64: points the local pass proved hidden, re-solves summed over the points, most re-solves of one point, points at the camera.
    """
    ctx = ctx or default_context()
    c = points_f64(cloud, "cloud")
    place = place_of(c)
    T = np.ascontiguousarray(np.asarray(T_pcd2cam, dtype=np.float64).reshape(-1, 4, 4))
    V, M = int(T.shape[0]), int(c.shape[0])
    sub = None
    if subset is not None:
        on_dev = _is_device_tensor(subset)
        if on_dev and place.device is None:
            raise ValueError("subset on the device needs the cloud on the device too")
        sub64 = subset.reshape(-1) if on_dev else np.asarray(subset).reshape(-1)
        if int(sub64.shape[0]) and (int(sub64.min()) < 0 or int(sub64.max()) >= M):
            raise IndexError("subset holds a row outside the cloud")
        sub = cat_int32([sub64], place)
    m = M if sub is None else int(sub.shape[0])
    flags = place.new((V, m), np.uint8)
    counts, status, stats = np.zeros(V, dtype=np.int64), np.zeros(V, dtype=np.int32), np.zeros((V, 4), dtype=np.int64)
    mem = place.mem
    place.sync()
    code = _ffi.load().ai_hidden_points(ctx._h, place.addr_or_null(c), M, place.addr_or_null(sub), m, T.ctypes.data, V, float(radius_factor),
                                        mem, place.addr_or_null(flags), counts.ctypes.data, status.ctypes.data, stats.ctypes.data)
    _ffi.check(code, "ai_hidden_points")
    sets = []
    for v in range(V):
        if status[v]:
            sets.append(None)
            continue
        if place.device is None:
            local = np.flatnonzero(flags[v]).astype(np.int64)
            sets.append(local if sub is None else sub[local].astype(np.int64))
        else:
            local = flags[v].nonzero().reshape(-1)
            sets.append(local if sub is None else place.index64(sub[local]))
        if int(sets[-1].shape[0]) != int(counts[v]):
            raise RuntimeError(f"ai_hidden_points: view {v} has {int(sets[-1].shape[0])} flags set, its count says {int(counts[v])}")
    return (sets, stats) if return_stats else sets


def hidden_point_removal_device(points, camera=(0.0, 0.0, 0.0), radius_factor=HPR_RADIUS, *, ctx: Context | None = None):
    """`hidden_point_removal` on the device: the ascending int64 indices of the points visible from ``camera`` (a NumPy array
    for a NumPy array, a device tensor for a float64 device tensor).  Raises ValueError where the removal skips the cloud
    (`visible_sets`), as the host function raises there."""
    T = np.eye(4)
    T[:3, 3] = -np.asarray(camera, dtype=np.float64).reshape(3)   # row r of the fixed-order transform: (1 * x + 0 + 0) - camera_r
    visible = visible_sets(points, T[None], radius_factor=radius_factor, ctx=ctx)[0]
    if visible is None:
        raise ValueError("hidden_point_removal_device: fewer than 4 points, no extent, a coordinate that is not finite, or a "
                         "sphere that does not hold the points")
    return visible


def _stack_maps(maps, n_views, dtype, name, on_device):
    """(V, ...) contiguous array from a stacked array / tensor or a list of per-view arrays / tensors, all of one shape.  Host
    maps are checked to fit ``dtype`` exactly and converted; device maps (allowed only with device points) must have it.  A
    device result may come from a copy queued on torch's current stream: the caller synchronises before the library reads it."""
    if isinstance(maps, np.ndarray) or _is_device_tensor(maps):
        out = maps
    else:
        maps = list(maps)
        on_dev = [_is_device_tensor(m) for m in maps]
        if any(on_dev) and not all(on_dev):
            raise ValueError(f"{name}: the per-view maps must all be host arrays or all device tensors")
        if not all(on_dev):
            maps = [np.asarray(m) for m in maps]
        shapes = {tuple(m.shape) for m in maps}
        if len(shapes) > 1:
            raise ValueError(f"{name}: every view's map must have the same shape, got {sorted(shapes)}")
        if not maps:
            out = None
        elif all(on_dev):
            import torch
            out = torch.stack(maps)
        else:
            out = np.stack(maps)
    if out is None or out.shape[0] != n_views:
        raise ValueError(f"{name}: one map per view expected ({n_views})")
    if _is_device_tensor(out):
        import torch
        if not on_device:
            raise ValueError(f"{name} on the device need points and cloud on the device too")
        want = torch.float32 if dtype == np.float32 else torch.int32
        if out.dtype != want:
            raise ValueError(f"{name} on the device must be {want}")
        return out.contiguous()
    a = np.asarray(out)
    if a.dtype != dtype:
        b = a.astype(dtype)
        if not np.array_equal(b, a, equal_nan=np.issubdtype(a.dtype, np.floating)):
            raise ValueError(f"{name}: values do not fit {np.dtype(dtype).name}")
        a = b
    return np.ascontiguousarray(a)


def camera_features(points, cloud, visible_indices, T_pcd2cam, K, image_hw, *, feature_maps=None, sam_images=None,
                    max_dist=MAJOR_VOXEL_SIZE / 2.0, return_pixels=False, ctx: Context | None = None):
    """Per-point camera features of one chunk over V views (``image_utils.py:146-348`` and ``dinov2_mean``), on the device.

    points (N, 3): the chunk's major-voxel points; cloud (M, 3): the points the visible sets index into (both in the pcd frame);
    visible_indices: V integer arrays of rows of ``cloud``; T_pcd2cam: V 4x4 transforms (last row 0 0 0 1); K: 3x3 intrinsics;
    image_hw: (h, w) of the images; feature_maps: V float32 maps of one shape (fh, fw, F), or a (V, fh, fw, F) array;
    sam_images: V int label images (h, w) (``masks_to_image`` output), or a (V, h, w) array.

    Returns a dict: ``dino`` (N, F) float64 -- the mean over the views of the feature rows under the point's pixels that hold a
    non-zero element (0 where none), ``dino_views`` (N,) int32 -- how many views entered that mean, ``sam`` (N, V) int32 -- the
    SAM label under the pixel, -1 where the point is not projected or the label is 0, and with ``return_pixels`` ``pixels``
    (N, V, 2) int32 -- (u, v), -1 where not projected.  Entries whose input is not given are None.  A projected pixel whose
    feature cell lies outside the map raises IndexError, as the reference does.
    """
    ctx = ctx or default_context()
    dev = _is_device_tensor(points)
    q = points_f64(points, "points")
    c = points_f64(cloud, "cloud")
    if dev != _is_device_tensor(c):
        raise ValueError("points and cloud must both be host arrays or both device tensors")
    place = place_of(q)
    vis = list(visible_indices)
    V = len(vis)
    if V > MAX_VIEWS:
        raise ValueError(f"at most {MAX_VIEWS} views per call, got {V}")
    T = np.ascontiguousarray(np.asarray(T_pcd2cam, dtype=np.float64).reshape(-1, 4, 4))
    if T.shape[0] != V:
        raise ValueError(f"T_pcd2cam: one 4x4 transform per view expected ({V}), got {T.shape[0]}")
    Kh = np.ascontiguousarray(np.asarray(K, dtype=np.float64).reshape(3, 3))
    h, w = (int(image_hw[0]), int(image_hw[1]))
    if h <= 0 or w <= 0:
        raise ValueError("image_hw must be positive")
    N, M = int(q.shape[0]), int(c.shape[0])
    off = np.zeros(V + 1, dtype=np.int64)
    for v, ix in enumerate(vis):
        off[v + 1] = off[v] + (int(ix.numel()) if _is_device_tensor(ix) else int(np.asarray(ix).size))
    if dev:
        import torch
        device = place.device
        vi = (torch.cat([torch.as_tensor(np.asarray(x) if not _is_device_tensor(x) else x, device=device).reshape(-1).to(torch.int32)
                         for x in vis]) if off[-1] > 0 else torch.zeros(1, dtype=torch.int32, device=device))
        if off[-1] > 0 and (int(vi.min()) < 0 or int(vi.max()) >= M):
            raise IndexError("visible_indices hold a row outside the cloud")
    else:
        vi = np.concatenate([np.asarray(x, dtype=np.int64).reshape(-1) for x in vis]) if off[-1] > 0 else np.zeros(0, np.int64)
        if vi.size and (vi.min() < 0 or vi.max() >= M):
            raise IndexError("visible_indices hold a row outside the cloud")
        vi = np.ascontiguousarray(vi.astype(np.int32))
    feat = fh = fw = F = None
    if feature_maps is not None:
        feat = _stack_maps(feature_maps, V, np.float32, "feature_maps", dev) if V else None
        if feat is None:
            shape = tuple(feature_maps.shape) if hasattr(feature_maps, "shape") else np.shape(feature_maps)
            F = int(shape[-1]) if len(shape) == 4 else None
            if F is None:
                raise ValueError("feature_maps: no view given, so the feature width is unknown; pass a (0, fh, fw, F) array")
            fh = fw = 0
        else:
            if feat.ndim != 4:
                raise ValueError("feature_maps must be (fh, fw, F) per view")
            fh, fw, F = (int(s) for s in feat.shape[1:])
        if F <= 0:
            raise ValueError("feature_maps: F must be positive")
    sam = None
    if sam_images is not None:
        sam = _stack_maps(sam_images, V, np.int32, "sam_images", dev) if V else None
        if sam is not None and tuple(sam.shape[1:]) != (h, w):
            raise ValueError(f"sam_images must be {h} x {w}, got {tuple(sam.shape[1:])}")
    if dev:
        import torch
        if feat is not None and not _is_device_tensor(feat):
            feat = torch.as_tensor(feat, device=device)
        if sam is not None and not _is_device_tensor(sam):
            sam = torch.as_tensor(sam, device=device)
    i32, f64 = np.int32, np.float64
    if N == 0:   # nothing to compute (a device tensor of no elements has no address to pass)
        return {"dino": place.new((0, F), f64) if feature_maps is not None else None,
                "dino_views": place.new((0,), i32) if feature_maps is not None else None,
                "sam": place.new((0, V), i32) if sam_images is not None else None,
                "pixels": place.new((0, V, 2), i32) if return_pixels else None}
    pix = place.new((N, V, 2), i32) if return_pixels else None
    sam_out = place.new((N, V), i32) if sam_images is not None else None
    mean = place.new((N, F), f64) if feature_maps is not None else None
    views = place.new((N,), i32) if feature_maps is not None else None
    feat_p = place.addr(feat if feat is not None else mean)   # a non-NULL map with V = 0: never read
    sam_p = place.addr(sam if sam is not None else sam_out)
    # every device input above (index concatenation, stacking, .contiguous() copies, uploads) was queued on torch's current stream
    place.sync()
    status = _ffi.load().ai_camera_project(
        ctx._h, place.addr(q), N, place.addr(c), M, place.addr(vi), off.ctypes.data, V, T.ctypes.data, Kh.ctypes.data, h, w, float(max_dist),
        feat_p, fh or 0, fw or 0, F or 0, sam_p, place.mem, place.addr(pix), place.addr(sam_out), place.addr(mean), place.addr(views))
    if status == -1 and "feature cell out of range" in _ffi.load().ai_last_error().decode("utf-8", "replace"):
        raise IndexError(_ffi.load().ai_last_error().decode("utf-8", "replace"))
    _ffi.check(status, "ai_camera_project")
    return {"dino": mean, "dino_views": views, "sam": sam_out, "pixels": pix}


def image_based_features_per_patch(dataset, pcd, chunk_indices, chunk_nc, T_pcd2world, cam_indices, hpr_masks=None, sam=True,
                                   dino=True, rm_perp=0.0, pcd_chunk=None, vis=False, *, cam_ids=CAM_IDS, dino_mean=False,
                                   hpr="qhull", ctx: Context | None = None):
    """Drop-in for ``image_based_features_per_patch`` (``image_utils.py:89-360``): the same positional arguments and return forms
    -- ``(point2sam_list, point2dino_list)``, ``point2sam_list``, or ``(point2dino_list, visibility_mask)`` for sam and dino /
    sam only / dino only -- with ``point2sam`` (N, V) int64 (-1: no label) and ``point2dino`` (N, V, F) float64 per camera.
    With ``dino_mean`` each ``point2dino`` is ``dinov2_mean`` of it instead, (N, F), formed on the device without the block.

    The host keeps the reference's control flow: ``pcd_chunk`` is recomputed from ``chunk_indices`` (:109, the argument is
    ignored as there); the inliers of the chunk come from `prep_api.statistical_inlier_indices`; ``T_pcd2cam = (T_lidar2cam @
    inv(pose_i)) @ T_pcd2world``; without ``hpr_masks`` the visible points are `hidden_point_removal` of the map points whose
    ``get_pose(0)``-transformed coordinates lie strictly inside the chunk's bounds (:158-179, formed once, not per view); a view
    is skipped when the removal raises ("hpr skip") or when no visible point is a chunk inlier ("out of view skip").  The
    visibility mask is all zeros, as with ``vis=False``.  ``rm_perp`` and ``vis=True`` are not implemented.
    ``hpr`` chooses the removal when ``hpr_masks`` is None: "qhull" (the default) is `hidden_point_removal` on the host, view by
    view; "device" is one `visible_sets` call per camera with ``bound_indices`` as its subset, a skipped view being an "hpr skip".
    ``dataset`` needs ``get_image(cam, 0).size``, ``get_pose``, ``get_calibration_matrices``, ``get_sam_mask`` and
    ``get_dinov2_features``; ``pcd`` / ``chunk_nc`` are arrays or objects with ``.points``.
    """
    if rm_perp:
        raise NotImplementedError("rm_perp != 0 is not implemented")
    if vis:
        raise NotImplementedError("vis=True is not implemented")
    if not sam and not dino:
        raise ValueError("Either sam or dino must be True")
    if hpr not in ("qhull", "device"):
        raise ValueError('hpr must be "qhull" or "device"')
    from .prep_api import statistical_inlier_indices
    ctx = ctx or default_context()
    pts = points_f64(pcd, "pcd")
    nc_pts = points_f64(chunk_nc, "chunk_nc")
    N = nc_pts.shape[0]
    V = len(cam_indices)
    chunk_indices = np.asarray(chunk_indices, dtype=np.int64).reshape(-1)
    pcd_chunk = pts[chunk_indices]                                                            # :109
    inliers = np.asarray(statistical_inlier_indices(pcd_chunk, ctx=ctx), dtype=np.int64)      # :110
    chunk_and_inlier = chunk_indices[inliers]                                                 # :111
    cai_order = np.argsort(chunk_and_inlier, kind="stable")
    cai_sorted = chunk_and_inlier[cai_order]
    visibility_mask = np.zeros(N)
    if hpr_masks is not None:
        assert len(cam_indices) == hpr_masks.shape[0]
    else:
        min_bound, max_bound = pcd_chunk.min(axis=0), pcd_chunk.max(axis=0)                  # :153-157
        world0 = transform_points(pts, dataset.get_pose(0))                                  # :148
        bound_indices = np.where(np.all(world0 > min_bound, axis=1) & np.all(world0 < max_bound, axis=1))[0]   # :162-173
    point2sam_list, point2dino_list = [], []
    F = NUM_DINO_FEATURES                                                                       # :122-124
    for cam_id in cam_ids:
        cam = _CAMS[cam_id]
        width, height = dataset.get_image(cam, 0).size
        kept, Ts, rows, Ks = [], [], [], []

        def view(points_index):
            T_lidar2world = np.asarray(dataset.get_pose(points_index), dtype=np.float64)
            T_lidar2cam, K = dataset.get_calibration_matrices(cam)
            return (np.asarray(T_lidar2cam, dtype=np.float64) @ np.linalg.inv(T_lidar2world)) @ np.asarray(T_pcd2world,
                                                                                                           dtype=np.float64), K

        device_sets = None
        if hpr_masks is None and hpr == "device" and V:   # one call needs every view's transform; the host paths ask view by view
            views = [view(points_index) for points_index in cam_indices]
            device_sets = visible_sets(pts, np.array([T for T, _ in views]), subset=bound_indices, radius_factor=HPR_RADIUS, ctx=ctx)
        for i, points_index in enumerate(cam_indices):
            T_pcd2cam, K = views[i] if device_sets is not None else view(points_index)
            if device_sets is not None:
                if device_sets[i] is None:   # "hpr skip"
                    continue
                visible = np.asarray(device_sets[i])
            elif hpr_masks is None:
                try:
                    local = hidden_point_removal(transform_points(pts[bound_indices], T_pcd2cam), camera=(0, 0, 0),
                                                 radius_factor=HPR_RADIUS)
                except Exception:   # noqa: BLE001 -- the reference's bare except: "hpr skip"
                    continue
                visible = bound_indices[local]
            else:
                visible = np.where(hpr_masks[i])[0]
            frame = np.intersect1d(visible, chunk_and_inlier)                                  # :204
            if frame.size == 0:                                                                 # "out of view skip"
                continue
            kept.append((i, points_index))
            Ts.append(T_pcd2cam)
            Ks.append(np.asarray(K, dtype=np.float64))
            rows.append(cai_order[np.searchsorted(cai_sorted, frame)])
        if len(kept) > MAX_VIEWS:
            raise ValueError(f"at most {MAX_VIEWS} views with visible points per camera, got {len(kept)}")
        sam_imgs = [masks_to_image(dataset.get_sam_mask(cam, pi)) for _, pi in kept] if sam else None
        maps = [np.asarray(dataset.get_dinov2_features(cam, pi)) for _, pi in kept] if dino else None
        if dino and any(m.ndim != 3 or m.shape[2] != F for m in maps):
            raise ValueError(f"the drop-in takes {F}-wide feature maps (NUM_DINO_FEATURES; the UMAP branch is not implemented)")
        Kc = Ks[0] if Ks else np.eye(3)
        # the means come from the device only when they are what is returned; the blocks are filled on the host from the
        # device's pixels, so the maps are not uploaded for them
        want_mean = dino and dino_mean
        res = camera_features(nc_pts, pts[chunk_and_inlier], rows, np.array(Ts).reshape(-1, 4, 4), Kc, (height, width),
                              feature_maps=(maps if maps else np.zeros((0, 1, 1, F), np.float32)) if want_mean else None,
                              sam_images=(sam_imgs if sam_imgs else (np.zeros((0, height, width), np.int32) if sam else None)),
                              return_pixels=dino and not dino_mean, ctx=ctx)
        if sam:
            p2s = np.full((N, V), -1, dtype=np.int64)
            for k, (i, _) in enumerate(kept):
                p2s[:, i] = res["sam"][:, k]
            point2sam_list.append(p2s)
        if dino:
            if dino_mean:
                point2dino_list.append(res["dino"])
            else:
                p2d = np.zeros((N, V, F))
                for k, (i, _) in enumerate(kept):
                    pix = res["pixels"][:, k]
                    on = np.where(pix[:, 0] >= 0)[0]
                    fmap = maps[k]
                    f0, f1 = fmap.shape[0] / height, fmap.shape[1] / width                     # :259-260
                    # a cell past the map raises IndexError here, as the reference's indexing does
                    p2d[on, i, :] = fmap[(f0 * pix[on, 1]).astype(np.int64), (f1 * pix[on, 0]).astype(np.int64), :]   # :342-346
                point2dino_list.append(p2d)
    if sam and dino:
        return point2sam_list, point2dino_list
    if sam:
        return point2sam_list
    return point2dino_list, visibility_mask

