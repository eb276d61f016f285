"""Seeded synthetic "surface chunk" generator.

The reference ships no data and its sample map is not reachable offline, so every
benchmark and parity test runs on chunks made here.  A chunk imitates what
``chunk_generation.chunks_from_pointcloud`` hands to ``ncuts_chunk``
(reference ``pipeline/utils/point_cloud/chunk_generation.py:96-180``): points of
object surfaces, voxel-downsampled at ``MAJOR_VOXEL_SIZE`` = 0.35 m
(``pipeline/config.py:56``), so that the 1.0 m radius graph
(``PROXIMITY_THRESHOLD``, ``pipeline/config.py:65``) has ~28-37 neighbours per point.

Recipe: boxes with centre ~U(-X/2, X/2)^2 x U(0, 2) m, size ~U(0.5, 4)^3 m, 200-3000
points on the 6 faces; first point per 0.35 m voxel kept, truncated to N.  The box
index (+1) is the ground-truth instance id used by the AP / S_assoc scorer.
"""
from __future__ import annotations

import numpy as np

VOXEL = 0.35

# extent (metres) that keeps the neighbour count of real 0.35 m chunks, per N
_EXTENTS = {10_000: 25.0, 50_000: 60.0, 200_000: 120.0, 1_000_000: 270.0}


def extent_for(n: int) -> float:
    """Square side X for an N-point chunk (25 m @10k ... 270 m @1M)."""
    if n in _EXTENTS:
        return _EXTENTS[n]
    # same areal density as the 10k / 25 m chunk
    return float(25.0 * np.sqrt(n / 10_000.0))


def _box_surface_points(rng, centre, size, m):
    """m points uniformly on the 6 faces of an axis-aligned box."""
    face = rng.integers(0, 6, size=m)
    u = rng.random((m, 3)) - 0.5
    axis = face // 2
    side = (face % 2).astype(np.float64) - 0.5
    u[np.arange(m), axis] = side
    return centre[None, :] + u * size[None, :]


def surface_chunk(n: int, seed: int = 0, extent: float | None = None):
    """Return (points[n,3] f64, gt_instance[n] int64).

    Deterministic for (n, seed, extent).  Points keep generation order after the
    voxel de-duplication, i.e. they are NOT spatially sorted (like open3d's
    voxel_down_sample output, which is hash-ordered).
    """
    rng = np.random.default_rng(seed)
    X = extent_for(n) if extent is None else float(extent)
    pts_l, ids_l = [], []
    seen = np.zeros(0, dtype=np.int64)
    total = 0
    box = 0
    target = int(1.05 * n) + 1
    while total < target:
        # a batch of boxes per round keeps the python overhead negligible at 1M
        nb = max(8, (target - total) // 400)
        bp, bi = [], []
        for _ in range(nb):
            box += 1
            centre = np.array([rng.uniform(-X / 2, X / 2), rng.uniform(-X / 2, X / 2), rng.uniform(0.0, 2.0)])
            size = rng.uniform(0.5, 4.0, size=3)
            m = int(rng.integers(200, 3001))
            bp.append(_box_surface_points(rng, centre, size, m))
            bi.append(np.full(m, box, dtype=np.int64))
        p = np.concatenate(bp)
        i = np.concatenate(bi)
        key = _voxel_key(p)
        # first occurrence inside this batch, in generation order
        _, first = np.unique(key, return_index=True)
        first.sort()
        p, i, key = p[first], i[first], key[first]
        # drop voxels already occupied by earlier batches
        fresh = ~np.isin(key, seen, assume_unique=False)
        p, i, key = p[fresh], i[fresh], key[fresh]
        seen = np.concatenate([seen, key])
        pts_l.append(p)
        ids_l.append(i)
        total += p.shape[0]
    pts = np.concatenate(pts_l)[:n]
    ids = np.concatenate(ids_l)[:n]
    return np.ascontiguousarray(pts, dtype=np.float64), ids


def _voxel_key(p):
    v = np.floor(p / VOXEL).astype(np.int64)
    v -= np.array([-(1 << 19), -(1 << 19), -(1 << 19)])
    return (v[:, 0] << 42) | (v[:, 1] << 21) | v[:, 2]


def surrogate_features(gt_ids, dim: int, seed: int = 0, zero_frac: float = 0.05, noise: float = 0.3):
    """TARL / DINO surrogate: f = noise*N(0,1)^dim + one-hot-ish box code.

    Stored the way the reference holds pooled features: float64, an all-zero row
    meaning "no feature for this point" (``chunk_generation.py:243-256`` yields a
    zero row when the 0.175 m radius search finds nothing).  Values are first rounded
    to float32, because the on-disk TARL / DINO features are float32
    (``kitti_odometry_dataset.py:251-281``).
    """
    rng = np.random.default_rng(seed + 7919 * dim)
    n = gt_ids.shape[0]
    f = noise * rng.standard_normal((n, dim)).astype(np.float32)
    code = (gt_ids * 2654435761 % dim).astype(np.int64)
    f[np.arange(n), code] += 1.0
    f[np.arange(n), (code * 7 + 3) % dim] += 1.0
    zero = rng.random(n) < zero_frac
    f[zero] = 0.0
    return f.astype(np.float64)


def synthetic_chunk(n: int, seed: int = 0, tarl: bool = True, dino: bool = False, extent: float | None = None):
    """Convenience: dict(points, gt, tarl|None, dino|None) for a cfg-named workload."""
    pts, gt = surface_chunk(n, seed, extent)
    out = {"points": pts, "gt": gt, "tarl": None, "dino": None}
    if tarl:
        out["tarl"] = surrogate_features(gt, 96, seed)
    if dino:
        out["dino"] = surrogate_features(gt, 384, seed + 1, zero_frac=0.05)
    return out


def _jittered_grid(rng, u0, u1, v0, v1, step):
    """One point per step x step cell of the rectangle [u0, u1) x [v0, v1), uniform inside its cell (a minor-voxel surface)."""
    u = np.arange(u0, u1, step)
    v = np.arange(v0, v1, step)
    uu, vv = np.meshgrid(u, v, indexing="ij")
    uu = uu.ravel() + rng.random(uu.size) * step
    vv = vv.ravel() + rng.random(vv.size) * step
    return uu, vv


def street_map(length: float = 120.0, seed: int = 0, *, step: float = 0.05, width: float = 16.0, facade_height: float = 8.0,
               n_objects: int | None = None, outlier_frac: float = 0.01):
    """A deterministic street in the shape of the minor-voxel maps ``chunk_and_downsample_point_clouds`` takes
    (``dataset_utils.py:489``): one point per ``step`` (0.05 m, ``MINOR_VOXEL_SIZE``) cell of every surface.

    In the map's frame the street runs along x over [0, length]: a ground plane |y| <= width / 2 (the ground cloud), two
    facades at y = +-width / 2 up to ``facade_height`` and box-shaped objects on the road (the non-ground cloud), plus
    ``outlier_frac`` uniform outliers in the box [0, length] x [-width, width] x [-2, 3 facade_height] (some metres from
    everything) and a few points repeated 24 times each (so that the outlier filter's ``avg == 0`` rule fires).  Both clouds
    are shuffled, as a hash-ordered voxel map is.  The trajectory runs along the street centre at 1.7 m in the world frame
    ``T_pcd`` (a rotation about z and a tilt, then a shift); points on the chunk boxes' x faces (exactly) test the strict crop.

    Returns a dict: ``nonground``, ``ground`` (n, 3) float64; ``labels`` with ``seg_nonground``, ``instance_nonground``,
    ``seg_ground``, ``instance_ground`` (int32: semantic 40 road, 50 building, 10 object, 0 outlier; instance = object
    number from 1, else 0); ``T_pcd`` (4, 4); ``positions`` (P, 3) world; ``first_position``; ``indices`` (P,) int64.
    """
    rng = np.random.default_rng(seed)
    half = width / 2.0
    # ground
    gx, gy = _jittered_grid(rng, 0.0, length, -half, half, step)
    gz = 0.02 * np.sin(gx * 0.3) + 0.01 * rng.standard_normal(gx.size)
    ground = np.stack([gx, gy, gz], 1)
    # facades
    parts, sem, inst = [], [], []
    for side in (-1.0, 1.0):
        fx, fz = _jittered_grid(rng, 0.0, length, 0.0, facade_height, step)
        fy = side * half + 0.01 * rng.standard_normal(fx.size)
        parts.append(np.stack([fx, fy, fz], 1))
        sem.append(np.full(fx.size, 50, np.int32))
        inst.append(np.zeros(fx.size, np.int32))
    # objects: boxes on the road, their 5 visible faces sampled at the same density
    n_objects = int(length / 6.0) if n_objects is None else n_objects
    for o in range(n_objects):
        c = np.array([rng.uniform(2.0, length - 2.0), rng.uniform(-half + 2.0, half - 2.0), 0.0])
        s = np.array([rng.uniform(1.5, 4.5), rng.uniform(1.2, 2.0), rng.uniform(1.0, 2.2)])
        lo = c - np.array([s[0] / 2, s[1] / 2, 0.0])
        faces = []
        for axis in range(3):
            a, b = [d for d in range(3) if d != axis]
            for end in ((0, 1) if axis < 2 else (1,)):
                u, v = _jittered_grid(rng, 0.0, s[a], 0.0, s[b], step)
                f = np.empty((u.size, 3))
                f[:, a] = lo[a] + u
                f[:, b] = lo[b] + v
                f[:, axis] = lo[axis] + end * s[axis]
                faces.append(f)
        f = np.concatenate(faces)
        parts.append(f)
        sem.append(np.full(f.shape[0], 10, np.int32))
        inst.append(np.full(f.shape[0], o + 1, np.int32))
    nonground = np.concatenate(parts)
    seg_ng, inst_ng = np.concatenate(sem), np.concatenate(inst)
    # uniform outliers
    n_out = int(outlier_frac * (nonground.shape[0] + ground.shape[0]))
    out = np.stack([rng.uniform(0.0, length, n_out), rng.uniform(-width, width, n_out),
                    rng.uniform(-2.0, 3.0 * facade_height, n_out)], 1)
    nonground = np.concatenate([nonground, out])
    seg_ng = np.concatenate([seg_ng, np.zeros(n_out, np.int32)])
    inst_ng = np.concatenate([inst_ng, np.zeros(n_out, np.int32)])
    seg_g = np.full(ground.shape[0], 40, np.int32)
    inst_g = np.zeros(ground.shape[0], np.int32)
    # trajectory: one position per metre along the centre line (with a little lateral noise), in the world frame
    ang, tilt = 0.6, 0.02
    Rz = np.array([[np.cos(ang), -np.sin(ang), 0.0], [np.sin(ang), np.cos(ang), 0.0], [0.0, 0.0, 1.0]])
    Rx = np.array([[1.0, 0.0, 0.0], [0.0, np.cos(tilt), -np.sin(tilt)], [0.0, np.sin(tilt), np.cos(tilt)]])
    T_pcd = np.eye(4)
    T_pcd[:3, :3] = Rz @ Rx
    T_pcd[:3, 3] = [351.25, -72.5, 3.0]
    s_path = np.arange(0.0, length, 1.0)
    p_map = np.stack([s_path, 0.05 * rng.standard_normal(s_path.size), np.full(s_path.size, 1.7)], 1)
    positions = p_map @ T_pcd[:3, :3].T + T_pcd[:3, 3]
    first_position = T_pcd[:3, 3].copy()
    indices = np.arange(s_path.size, dtype=np.int64) * 5

    # points exactly on the x faces of the chunk boxes (the crop is strict: they belong to no box through that face)
    from .prep_api import chunk_centres
    from .config import CHUNK_SIZE
    centres, _ = chunk_centres(T_pcd, positions, first_position, indices)
    extra_ng, extra_g = [], []
    for c in centres:
        for xf in (c[0] - 0.5 * CHUNK_SIZE[0], c[0] + 0.5 * CHUNK_SIZE[0]):
            for cloud, extra in ((nonground, extra_ng), (ground, extra_g)):
                near = cloud[np.abs(cloud[:, 0] - xf) < 0.5]
                pick = near[rng.choice(near.shape[0], size=min(40, near.shape[0]), replace=False)].copy()
                pick[:, 0] = xf
                extra.append(pick)
    if extra_ng:
        e = np.concatenate(extra_ng)
        nonground = np.concatenate([nonground, e])
        seg_ng = np.concatenate([seg_ng, np.full(e.shape[0], 50, np.int32)])
        inst_ng = np.concatenate([inst_ng, np.zeros(e.shape[0], np.int32)])
        e = np.concatenate(extra_g)
        ground = np.concatenate([ground, e])
        seg_g = np.concatenate([seg_g, np.full(e.shape[0], 40, np.int32)])
        inst_g = np.concatenate([inst_g, np.zeros(e.shape[0], np.int32)])

    def dup_and_shuffle(p, s_, i_):
        d = rng.choice(p.shape[0], size=max(1, p.shape[0] // 20000), replace=False)
        rep = np.repeat(d, 23)   # each picked point 24 times in all
        p, s_, i_ = np.concatenate([p, p[rep]]), np.concatenate([s_, s_[rep]]), np.concatenate([i_, i_[rep]])
        perm = rng.permutation(p.shape[0])
        return np.ascontiguousarray(p[perm]), s_[perm], i_[perm]

    nonground, seg_ng, inst_ng = dup_and_shuffle(nonground, seg_ng, inst_ng)
    ground, seg_g, inst_g = dup_and_shuffle(ground, seg_g, inst_g)
    labels = {"seg_nonground": seg_ng, "instance_nonground": inst_ng, "seg_ground": seg_g, "instance_ground": inst_g}
    return {"nonground": nonground, "ground": ground, "labels": labels, "T_pcd": T_pcd, "positions": positions,
            "first_position": first_position, "indices": indices}


def _rotation(axis, angle):
    """Rotation matrix about a unit axis (Rodrigues)."""
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0.0, -a[2], a[1]], [a[2], 0.0, -a[0]], [-a[1], a[0], 0.0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


def camera_rig(n_views: int = 29, seed: int = 0, *, length: float = 48.0, query_voxel: float = 0.17, fh: int = 27, fw: int = 88,
               fdim: int = 384, image_hw=(376, 1241), n_masks: int = 12, keep_frac: float = 0.8):
    """A seeded KITTI-like camera rig along `street_map`'s trajectory, enough to drive ``camera_api``.

    The map is the street's two clouds (``pcd``, in the pcd frame); the chunk is the 25 m box around the street's middle
    (``chunk_indices``, strict crop) and ``points`` its points averaged over ``query_voxel`` voxels (0.17 m: about 30 k points;
    the pipeline's 0.35 m gives a quarter of that on this street).  The scans are numbered from 1 at one metre apart along the
    centre line, the first views ~20 m before the chunk's centre, looking down the street; scan 0 has the identity pose (the
    reference crops the map for its hidden point removal by ``get_pose(0)``).  The pcd-to-world transform is the street's
    ``T_pcd``.  Per view: ``T_pcd2cam = (T_lidar2cam @ inv(pose)) @ T_pcd2world``.

    ``T_lidar2cam`` maps x forward / z up to z forward / y down (with a small seeded tilt and KITTI's lever arm), ``K`` has
    fx = fy = 718.856, cx = 607.1928, cy = 185.2157 and the image is 376 x 1241.  ``feature_maps`` (V, fh, fw, fdim) float32 with
    fh / h and fw / w inexact (27 / 376, 88 / 1241), about 5 % all-zero and 3 % all-(-0.0) cells; ``sam_masks[v]``: rectangles
    (row0, row1, col0, col1) of the view's SAM masks (``sam_images`` their ``masks_to_image`` labels, int32, 0 where no mask).
    ``hpr_masks`` (V, len(pcd)) bool stands in for the hidden point removal: the points in front of the camera that project into
    the image, a seeded ``keep_frac`` of them.
    """
    rng = np.random.default_rng(seed + 4242)
    m = street_map(length, seed)
    pcd = np.ascontiguousarray(np.concatenate([m["nonground"], m["ground"]]))
    centre = np.array([length / 2.0, 0.0, 4.0])
    lo, hi = centre - 12.5, centre + 12.5
    chunk_indices = np.where(np.all(pcd > lo, axis=1) & np.all(pcd < hi, axis=1))[0]
    chunk = pcd[chunk_indices]
    key = np.floor((chunk - chunk.min(axis=0)) / query_voxel).astype(np.int64)
    _, inv, cnt = np.unique(key, axis=0, return_inverse=True, return_counts=True)
    inv = inv.reshape(-1)
    points = np.stack([np.bincount(inv, weights=chunk[:, a]) for a in range(3)], 1) / cnt[:, None]
    T_pcd2world = m["T_pcd"]
    h, w = int(image_hw[0]), int(image_hw[1])
    K = np.array([[718.856, 0.0, 607.1928], [0.0, 718.856, 185.2157], [0.0, 0.0, 1.0]])
    T_lidar2cam = np.eye(4)
    T_lidar2cam[:3, :3] = _rotation(rng.standard_normal(3), 0.01) @ np.array([[0.0, -1.0, 0.0], [0.0, 0.0, -1.0], [1.0, 0.0, 0.0]])
    T_lidar2cam[:3, 3] = [0.06, -0.08, -0.27]
    poses = {0: np.eye(4)}
    cam_indices = list(range(1, n_views + 1))
    x0 = centre[0] - 20.0
    T_pcd2cam = np.empty((n_views, 4, 4))
    for k, idx in enumerate(cam_indices):
        local = np.eye(4)
        local[:3, :3] = _rotation([0.0, 0.0, 1.0], 0.03 * rng.standard_normal())
        local[:3, 3] = [x0 + k, 0.3 * rng.standard_normal(), 1.7]
        poses[idx] = T_pcd2world @ local
        T_pcd2cam[k] = (T_lidar2cam @ np.linalg.inv(poses[idx])) @ T_pcd2world
    feature_maps = rng.standard_normal((n_views, fh, fw, fdim), dtype=np.float32)
    cell = rng.random((n_views, fh, fw))
    feature_maps[cell < 0.05] = 0.0
    feature_maps[(cell >= 0.05) & (cell < 0.08)] = -0.0
    sam_masks, sam_images = [], np.zeros((n_views, h, w), dtype=np.int32)
    for v in range(n_views):
        rects = []
        for i in range(n_masks):
            r0, c0 = int(rng.integers(0, h - 20)), int(rng.integers(0, w - 40))
            r1, c1 = r0 + int(rng.integers(10, h // 2)), c0 + int(rng.integers(20, w // 3))
            rects.append((r0, min(r1, h), c0, min(c1, w)))
            sam_images[v, r0:r1, c0:c1] = i + 1
        sam_masks.append(rects)
    hpr_masks = np.zeros((n_views, pcd.shape[0]), dtype=bool)
    x, y, z = pcd[:, 0], pcd[:, 1], pcd[:, 2]
    for v in range(n_views):
        T = T_pcd2cam[v]
        cx, cy, cz = (T[r, 0] * x + T[r, 1] * y + T[r, 2] * z + T[r, 3] for r in range(3))
        with np.errstate(divide="ignore", invalid="ignore"):
            u, vv = (K[0, 0] * cx + K[0, 2] * cz) / cz, (K[1, 1] * cy + K[1, 2] * cz) / cz
        hpr_masks[v] = (cz > 0.5) & (cz < 60.0) & (u > -1) & (u < w) & (vv > -1) & (vv < h) & (rng.random(pcd.shape[0]) < keep_frac)
    return {"pcd": pcd, "chunk_indices": chunk_indices, "points": np.ascontiguousarray(points), "T_pcd2world": T_pcd2world,
            "poses": poses, "cam_indices": cam_indices, "T_lidar2cam": T_lidar2cam, "K": K, "image_hw": (h, w),
            "T_pcd2cam": T_pcd2cam, "feature_maps": feature_maps, "sam_masks": sam_masks, "sam_images": sam_images,
            "hpr_masks": hpr_masks}


def rig_sam_masks(rig, view: int):
    """The SAM masks of one view of `camera_rig` as the dataset hands them out: a list of {"segmentation": bool (h, w)}."""
    h, w = rig["image_hw"]
    out = []
    for r0, r1, c0, c1 in rig["sam_masks"][view]:
        seg = np.zeros((h, w), dtype=bool)
        seg[r0:r1, c0:c1] = True
        out.append({"segmentation": seg})
    return out


def labelled_scans(n_scans: int = 20, points_per_scan: int = 10_000, seed: int = 0, *, spacing: float = 1.5, width: float = 16.0,
                   reach: float = 40.0, facade_height: float = 8.0, moving_frac: float = 0.03):
    """A deterministic street as the scans ``aggregate_pointcloud`` reads (``aggregate_pointcloud.py:99-107``): per scan float32
    points in the sensor frame, raw ``.label`` words, a ground mask (what a ground segmentation would return) and the pose.

    The sensor drives along x, ``spacing`` metres per scan, 1.7 m above the road, with a slow yaw and a little roll; scan lengths
    vary by a few per cent around ``points_per_scan``.  In the sensor frame a scan sees the road (|x| <= ``reach``, |y| <=
    ``width`` / 2; semantic 40, flagged ground), the two facades (semantic 50) and box-shaped objects (semantic 10 with an
    instance number in the upper half of the word; ``moving_frac`` of the points carry a moving class, 252 upwards).  The map
    frame is the world frame: ``T_pcd`` is the identity and ``first_position`` the origin.

    Returns a dict: ``scans``, ``labels`` (uint32), ``ground`` (bool) -- lists per scan; ``poses`` (n_scans, 4, 4);
    ``T_pcd``, ``positions``, ``first_position``, ``indices`` for `prep_api.chunk_and_downsample_point_clouds`.
    """
    rng = np.random.default_rng(seed)
    half = np.float32(width / 2.0)
    scans, labels, ground = [], [], []
    poses = np.zeros((n_scans, 4, 4))
    for s in range(n_scans):
        n = int(points_per_scan * (0.97 + 0.06 * rng.random()))
        u = rng.random((n, 3), dtype=np.float32)
        kind = rng.random(n, dtype=np.float32)
        p = np.empty((n, 3), dtype=np.float32)
        p[:, 0] = (u[:, 0] * 2 - 1) * np.float32(reach)
        road, left = kind < 0.45, (kind >= 0.45) & (kind < 0.68)
        right = (kind >= 0.68) & (kind < 0.91)
        p[:, 1] = (u[:, 1] * 2 - 1) * half
        p[:, 2] = np.float32(-1.7) + np.float32(0.02) * (u[:, 2] - np.float32(0.5))
        for side, m in ((-1.0, left), (1.0, right)):
            p[m, 1] = np.float32(side) * half + np.float32(0.02) * (u[m, 1] - np.float32(0.5))
            p[m, 2] = np.float32(-1.7) + u[m, 2] * np.float32(facade_height)
        obj = ~(road | left | right)
        number = (np.floor((p[:, 0] + np.float32(reach)) / np.float32(6.0)).astype(np.uint32) + np.uint32(s // 4 + 1)) & np.uint32(0xFFFF)
        p[obj, 1] *= np.float32(0.6)
        p[obj, 2] = np.float32(-1.7) + u[obj, 2] * np.float32(1.8)
        sem = np.where(road, 40, np.where(obj, 10, 50)).astype(np.uint32)
        moving = obj & (rng.random(n, dtype=np.float32) < moving_frac / 0.09)
        sem[moving] = np.uint32(252) + (number[moving] % np.uint32(8))
        words = sem | np.where(obj, number << np.uint32(16), np.uint32(0))
        yaw, roll = 0.002 * s, 0.01 * np.sin(0.3 * s)
        T = np.eye(4)
        T[:3, :3] = _rotation((0.0, 0.0, 1.0), yaw) @ _rotation((1.0, 0.0, 0.0), roll)
        T[:3, 3] = [spacing * s, 0.05 * np.sin(0.7 * s), 1.7]
        poses[s] = T
        scans.append(p)
        labels.append(words.astype(np.uint32))
        ground.append(road)
    positions = poses[:, :3, 3].copy()
    return {"scans": scans, "labels": labels, "ground": ground, "poses": poses, "T_pcd": np.eye(4), "positions": positions,
            "first_position": np.zeros(3), "indices": np.arange(n_scans, dtype=np.int64)}
