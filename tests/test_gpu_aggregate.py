"""GPU suite: ai_aggregate_scans / prep_api.aggregate_scans / prep_api.aggregate_pointcloud (csrc/ai_aggregate.hip) against the
NumPy restatement tests/aggregate_ref.py (rules A1-A6 of include/autoinst_hip.h).

Every comparison is an equality, the coordinates bit for bit: both maps' points, all six label arrays, the source positions, the
per-scan offsets and the counts.  The shapes are those of aggregate_ref.cases(): one scan of 1 .. 2049 points around the pass
(256), the tile (1024) and two tiles; scans whose boundaries disagree with the tiles'; empty scans; no scans; one class only;
alternating classes; the one-ulp range cases; the special label words; each filter off; the three kinds of pose.

The shared scan's recursive path cannot be reached: it starts above SCAN_MAX_DIRECT_TILES * SCAN_TILE = 4096 * 2048 scanned
elements, and the scanned elements are the counts of 1024-point tiles, so that is above 2^33 points while M < 2^31 - 256.  The
boundary a call does cross is the scan's second block, above 2048 tile counts: aggregate_ref.big_case() has 2 098 177 points
(2050 tile counts)."""
import ctypes as C
import os
import re

import numpy as np
import pytest

import aggregate_ref as R
from autoinst_amd import _ffi, prep_api, synth
from conftest import ROOT

pytestmark = pytest.mark.gpu

CASES = R.cases()
KEYS = [f"{k}_{c}" for k in R.KINDS for c in R.CLOUDS]


def _host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


def check(got, exp, what, labelled=True):
    """got: (pcd_ground, pcd_nonground, dict) of prep_api.aggregate_scans(..., return_source=True); exp: aggregate_ref.aggregate."""
    g, n, d = got
    for cloud, pts in (("ground", g), ("nonground", n)):
        pts = _host(pts)
        assert pts.dtype == np.float64 and pts.shape == exp[f"xyz_{cloud}"].shape, (what, cloud, pts.shape, exp[f"xyz_{cloud}"].shape)
        assert pts.tobytes() == exp[f"xyz_{cloud}"].tobytes(), (what, cloud)
        src = _host(d[f"source_{cloud}"])
        assert src.dtype == np.int64
        np.testing.assert_array_equal(src, exp[f"source_{cloud}"], err_msg=f"{what} source_{cloud}")
        off = d[f"offsets_{cloud}"]
        assert isinstance(off, np.ndarray) and off.dtype == np.int64
        np.testing.assert_array_equal(off, exp[f"offsets_{cloud}"], err_msg=f"{what} offsets_{cloud}")
        assert off[-1] == pts.shape[0]
    assert all((k in d) == labelled for k in KEYS), what
    if labelled:
        for k in KEYS:
            a = _host(d[k])
            assert a.ndim == 1 and a.dtype == (np.int64 if hasattr(d[k], "is_cuda") else np.uint32), (what, k, a.dtype)
            np.testing.assert_array_equal(a.astype(np.uint32), exp[k], err_msg=f"{what} {k}")
            assert int(a.min(initial=0)) >= 0


def on_device(c, dev):
    """The case as resident tensors: one (M, 3) tensor with offsets, int64 label words, one (M,) mask."""
    import torch
    off = np.cumsum([0] + [s.shape[0] for s in c["scans"]]).astype(np.int64)
    xyz = np.concatenate(c["scans"]) if c["scans"] else np.zeros((0, 3), np.float32)
    kw = {k: c[k] for k in ("moving_index", "range_min", "range_max")}
    kw["labels"] = None if c["labels"] is None else torch.as_tensor(
        (np.concatenate(c["labels"]) if c["labels"] else np.zeros(0, np.uint32)).astype(np.int64), device=dev)
    kw["ground"] = None if c["ground"] is None else torch.as_tensor(
        np.concatenate(c["ground"]) if c["ground"] else np.zeros(0, bool), device=dev)
    return (torch.as_tensor(xyz, device=dev), c["poses"]), dict(kw, scan_offsets=off)


@pytest.fixture(scope="module")
def expected():
    return {name: R.aggregate(**c) for name, c in CASES.items()}


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_restatement(name, expected, ctx):
    import torch
    c = CASES[name]
    kw = {k: c[k] for k in ("labels", "ground", "moving_index", "range_min", "range_max")}
    got = prep_api.aggregate_scans(c["scans"], c["poses"], return_source=True, ctx=ctx, **kw)
    check(got, expected[name], name, labelled=c["labels"] is not None)
    again = prep_api.aggregate_scans(c["scans"], c["poses"], return_source=True, ctx=ctx, **kw)
    for a, b in zip(got[:2], again[:2]):
        assert a.tobytes() == b.tobytes()                                   # two calls: bit-identical
    assert all(np.array_equal(got[2][k], again[2][k]) for k in got[2])
    args, dkw = on_device(c, torch.device("cuda", ctx.device))
    dev = prep_api.aggregate_scans(*args, return_source=True, ctx=ctx, **dkw)
    assert dev[0].is_cuda and dev[1].is_cuda and all(v.is_cuda for k, v in dev[2].items() if not k.startswith("offsets"))
    check(dev, expected[name], name + " (device)", labelled=c["labels"] is not None)   # NumPy inputs and device tensors: the same bits


def test_the_scan_of_the_tile_counts_takes_its_second_block(ctx):
    """2 098 177 points = 2050 tiles of 1024: the shared scan needs two of its 2048-element blocks (the module docstring says why
    no call can reach SCAN_MAX_DIRECT_TILES)."""
    src = open(os.path.join(ROOT, "autoinst_amd", "csrc", "ai_scan.hip")).read()
    agg = open(os.path.join(ROOT, "autoinst_amd", "csrc", "ai_aggregate.hip")).read()
    assert int(re.search(r"#define SCAN_MAX_DIRECT_TILES (\d+)", src).group(1)) == R.SCAN_MAX_DIRECT_TILES
    assert int(re.search(r"#define SCAN_ITEMS (\d+)", src).group(1)) * 256 == R.SCAN_TILE
    assert int(re.search(r"#define AG_ITEMS (\d+)", agg).group(1)) * 256 == R.TILE
    assert R.SCAN_MAX_DIRECT_TILES * R.SCAN_TILE * R.TILE >= 2 ** 31 and -(-R.BIG_POINTS // R.TILE) > R.SCAN_TILE
    import torch
    c = R.big_case()
    exp = R.aggregate(**c)
    args, dkw = on_device(c, torch.device("cuda", ctx.device))
    check(prep_api.aggregate_scans(*args, return_source=True, ctx=ctx, **dkw), exp, "big")
    # everything kept, one class: every tile is full and the bases run to the point count
    flat = dict(dkw, moving_index=None, range_min=None, range_max=None, ground=None)
    g, n, d = prep_api.aggregate_scans(*args, return_source=True, ctx=ctx, **flat)
    assert g.shape[0] == 0 and n.shape[0] == R.BIG_POINTS
    assert torch.equal(d["source_nonground"], torch.arange(R.BIG_POINTS, device=n.device))
    full = R.aggregate(c["scans"], c["poses"], c["labels"])
    assert n.cpu().numpy().tobytes() == full["xyz_nonground"].tobytes()
    np.testing.assert_array_equal(d["instance_nonground"].cpu().numpy().astype(np.uint32), full["instance_nonground"])


def test_a_scan_alone_and_among_others(expected, ctx):
    c = CASES["three_scans_2047_2048_2049"]
    exp = expected["three_scans_2047_2048_2049"]
    kw = {k: c[k] for k in ("moving_index", "range_min", "range_max")}
    for s in range(3):
        g, n, d = prep_api.aggregate_scans([c["scans"][s]], c["poses"][s:s + 1], labels=[c["labels"][s]], ground=[c["ground"][s]],
                                           return_source=True, ctx=ctx, **kw)
        for cloud, pts in (("ground", g), ("nonground", n)):
            a, b = exp[f"offsets_{cloud}"][s], exp[f"offsets_{cloud}"][s + 1]
            assert pts.tobytes() == exp[f"xyz_{cloud}"][a:b].tobytes(), (s, cloud)
            for kind in R.KINDS:
                np.testing.assert_array_equal(d[f"{kind}_{cloud}"], exp[f"{kind}_{cloud}"][a:b])


def test_input_forms(expected, ctx):
    """(n, 4) scans with an intensity column, ground as index lists in any order, labels of another integer dtype, labels and
    source outputs left out: the same maps."""
    c, exp = CASES["three_scans_1023_1024_1025"], expected["three_scans_1023_1024_1025"]
    rng = np.random.default_rng(3)
    scans4 = [np.concatenate([s, rng.random((s.shape[0], 1), dtype=np.float32)], 1) for s in c["scans"]]
    idx = [rng.permutation(np.flatnonzero(g)) for g in c["ground"]]
    kw = {k: c[k] for k in ("moving_index", "range_min", "range_max")}
    got = prep_api.aggregate_scans(scans4, c["poses"], labels=[w.astype(np.int64) for w in c["labels"]], ground=idx, return_source=True,
                                   ctx=ctx, **kw)
    check(got, exp, "forms")
    g, n, d = prep_api.aggregate_scans(scans4, c["poses"], labels=c["labels"], ground=idx, ctx=ctx, **kw)
    assert sorted(d) == sorted(KEYS) and g.tobytes() == exp["xyz_ground"].tobytes() and n.tobytes() == exp["xyz_nonground"].tobytes()
    g, n, d = prep_api.aggregate_scans(scans4, c["poses"], ground=idx, range_min=3.0, range_max=25.0, ctx=ctx)
    assert d == {}
    plain = R.aggregate(c["scans"], c["poses"], None, c["ground"], None, 3.0, 25.0)
    assert g.tobytes() == plain["xyz_ground"].tobytes() and n.tobytes() == plain["xyz_nonground"].tobytes()
    for bad in ([np.array([0, 5, 5])] + idx[1:], [np.array([0, 1023])] + idx[1:], [np.array([-1])] + idx[1:], idx[:2]):
        with pytest.raises(ValueError):
            prep_api.aggregate_scans(c["scans"], c["poses"], ground=bad, ctx=ctx)          # duplicate, out of range, too few
    with pytest.raises(ValueError):
        prep_api.aggregate_scans(c["scans"], c["poses"], labels=[np.full(w.shape, -1) for w in c["labels"]], ctx=ctx)
    with pytest.raises(ValueError):
        prep_api.aggregate_scans([s.astype(np.float64) for s in c["scans"]], c["poses"], ctx=ctx)


# ----------------------------------------------------------------------------- errors leave the outputs unwritten

FILL = 0xAB


def fresh_outputs(M, n_off, label_outputs=True):
    """Host output buffers of ai_aggregate_scans, every one filled with a value no call writes."""
    M = max(int(M), 1)
    bufs = {"xyz_g": np.full((M, 3), np.nan), "xyz_n": np.full((M, 3), np.nan)}
    for k in ("seg_g", "seg_n", "inst_g", "inst_n", "pan_g", "pan_n"):
        bufs[k] = np.full(M, FILL, np.uint32) if label_outputs else None
    bufs["src_g"], bufs["src_n"] = np.full(M, -FILL, np.int32), np.full(M, -FILL, np.int32)
    bufs["class_off"] = np.full(2 * n_off, -FILL, np.int64)
    return bufs


def raw_call(ctx, xyz, off, poses, words, flags, moving, rmin, rmax, label_outputs=True):
    """ai_aggregate_scans on fresh host buffers: (status, every output buffer, the two counts)."""
    bufs = fresh_outputs(xyz.shape[0], off.shape[0], label_outputs)
    ng, nn = C.c_int64(-FILL), C.c_int64(-FILL)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    st = _ffi.load().ai_aggregate_scans(
        ctx._h, ptr(xyz), ptr(off), off.shape[0] - 1, ptr(poses), ptr(words), ptr(flags), moving, rmin, rmax, _ffi.AI_MEM_HOST,
        *[ptr(bufs[k]) for k in ("xyz_g", "xyz_n", "seg_g", "seg_n", "inst_g", "inst_n", "pan_g", "pan_n", "src_g", "src_n", "class_off")],
        C.byref(ng), C.byref(nn))
    bufs["ng"], bufs["nn"] = np.array([ng.value]), np.array([nn.value])
    return st, bufs


def test_errors_leave_the_outputs_unwritten(ctx):
    rng = np.random.default_rng(9)
    p, w, g = R.make_scan(rng, 1500)
    off = np.array([0, 700, 1500], dtype=np.int64)
    poses = np.ascontiguousarray(np.stack([R.pose("rotation", 1), R.pose("translation")]).reshape(2, 16))
    flags = g.astype(np.uint8)
    st, clean = raw_call(ctx, p, off, poses, w, flags, 251, 3.0, 25.0)
    assert st == 0 and clean["ng"][0] + clean["nn"][0] > 100
    exp = R.aggregate([p[:700], p[700:]], poses.reshape(2, 4, 4), [w[:700], w[700:]], [g[:700], g[700:]], 251, 3.0, 25.0)
    assert clean["xyz_g"][:clean["ng"][0]].tobytes() == exp["xyz_ground"].tobytes()
    np.testing.assert_array_equal(clean["class_off"], np.concatenate([exp["offsets_ground"], exp["offsets_nonground"]]))

    def bad_pose(r, c, v):
        q = poses.copy().reshape(2, 4, 4)
        q[1, r, c] = v
        return np.ascontiguousarray(q.reshape(2, 16))
    last_row = poses.copy().reshape(2, 4, 4)
    last_row[0, 3] = np.array([0.0, 0.0, 0.0, 1.0]) + 1e-16        # (1e-16, 1e-16, 1e-16, 1): the 1 absorbs it, the zeros do not
    assert last_row[0, 3, 3] == 1.0 and last_row[0, 3, 0] != 0.0
    bad = {
        "offsets start at 1": dict(off=np.array([1, 700, 1500], dtype=np.int64)),
        "offsets decrease": dict(off=np.array([0, 900, 800], dtype=np.int64)),
        "last pose row + 1e-16": dict(poses=np.ascontiguousarray(last_row.reshape(2, 16))),
        "last pose row 0 0 0 2": dict(poses=bad_pose(3, 3, 2.0)),
        "NaN in a pose": dict(poses=bad_pose(1, 2, np.nan)),
        "inf in a pose": dict(poses=bad_pose(0, 3, np.inf)),
        "range_min > range_max": dict(rmin=25.0, rmax=3.0),
        "NaN range_min": dict(rmin=float("nan"), rmax=3.0),
        "moving filter without words": dict(words=None, label_outputs=False),
        "label outputs without words": dict(words=None, moving=-1),
    }
    for what, change in bad.items():
        a = dict(xyz=p, off=off, poses=poses, words=w, flags=flags, moving=251, rmin=3.0, rmax=25.0)
        a.update(change)
        st, bufs = raw_call(ctx, **a)
        assert st == -1, what
        assert _ffi.load().ai_last_error().decode().startswith("ai_aggregate_scans:"), what
        untouched = fresh_outputs(p.shape[0], a["off"].shape[0], a.get("label_outputs", True))
        untouched["ng"] = untouched["nn"] = np.array([-FILL])
        for k, v in bufs.items():
            assert v is None or v.tobytes() == untouched[k].tobytes(), (what, k)
    # the same through the wrapper
    scans, labels = [p[:700], p[700:]], [w[:700], w[700:]]
    for kw in (dict(range_min=25.0, range_max=3.0), dict(moving_index=251), dict(poses=last_row), dict(poses=bad_pose(1, 2, np.nan))):
        with pytest.raises(ValueError):
            prep_api.aggregate_scans(scans, kw.pop("poses", poses), labels=None if "moving_index" in kw else labels, ctx=ctx, **kw)
    with pytest.raises(ValueError):
        prep_api.aggregate_scans(scans, poses, ground=[np.array([3, 3]), np.array([], dtype=np.int64)], ctx=ctx)   # duplicate ground index
    # not errors
    st, z = raw_call(ctx, p[:0], np.array([0], dtype=np.int64), None, None, None, -1, 0.0, -1.0, label_outputs=False)
    assert st == 0 and z["ng"][0] == z["nn"][0] == 0 and z["class_off"].tolist() == [0, 0]
    lib = _ffi.load()
    n1, n2 = C.c_int64(7), C.c_int64(7)
    big = np.array([0, 2 ** 31 - 256], dtype=np.int64)
    assert lib.ai_aggregate_scans(ctx._h, p.ctypes.data, big.ctypes.data, 1, poses.ctypes.data, None, None, -1, 0.0, -1.0, _ffi.AI_MEM_HOST,
                                  p.ctypes.data, p.ctypes.data, None, None, None, None, None, None, None, None, None, C.byref(n1),
                                  C.byref(n2)) == -1                                      # ai_box_select's bound on M
    assert n1.value == n2.value == 7


# ----------------------------------------------------------------------------- hand-over and the drop-in

def test_hand_over_to_the_map_and_chunk_preparation(ctx):
    """aggregate_scans -> downsample_map -> chunk_and_downsample_point_clouds on a ~200 k-point street, resident from the scans
    on: the minor maps and the chunks equal those of the restatement's clouds fed to the same functions."""
    import torch
    dev = torch.device("cuda", ctx.device)
    m = synth.labelled_scans(20, 10_000, seed=4)
    assert 190_000 < sum(s.shape[0] for s in m["scans"]) < 210_000
    filt = dict(moving_index=251, range_min=3.0, range_max=35.0)
    c = dict(scans=m["scans"], poses=m["poses"], labels=m["labels"], ground=m["ground"], **filt)
    exp = R.aggregate(**c)
    assert exp["xyz_ground"].shape[0] > 50_000 and exp["xyz_nonground"].shape[0] > 50_000
    assert exp["xyz_ground"].shape[0] + exp["xyz_nonground"].shape[0] < 0.97 * sum(s.shape[0] for s in m["scans"])
    args, dkw = on_device(c, dev)
    g, ng, labels = prep_api.aggregate_scans(*args, ctx=ctx, **dkw)
    assert g.is_cuda and ng.is_cuda and all(v.is_cuda and v.dtype == torch.int64 for v in labels.values())
    g_minor, ng_minor, kitti = prep_api.downsample_map(ng, g, labels, ctx=ctx)
    assert g_minor.is_cuda and ng_minor.is_cuda and all(v.is_cuda for v in kitti.values())
    ref_labels = {k: exp[k] for k in KEYS}
    rg_minor, rng_minor, rkitti = prep_api.downsample_map(exp["xyz_nonground"], exp["xyz_ground"], ref_labels, ctx=ctx)
    assert isinstance(rg_minor, np.ndarray) and rkitti["seg_ground"].dtype == np.uint32        # both label forms pass the integer test
    assert g_minor.cpu().numpy().tobytes() == rg_minor.tobytes() and ng_minor.cpu().numpy().tobytes() == rng_minor.tobytes()
    assert 10_000 < rg_minor.shape[0] <= exp["xyz_ground"].shape[0]
    for k in prep_api.LABEL_KEYS:
        np.testing.assert_array_equal(kitti[k].cpu().numpy().astype(np.uint32), rkitti[k], err_msg=k)
    walk = (m["T_pcd"], m["positions"], m["first_position"], m["indices"])
    d = prep_api.chunk_and_downsample_point_clouds(ng_minor, g_minor, *walk, kitti_labels=kitti, ctx=ctx)
    assert len(d["pcd_nonground_chunks"]) >= 1 and all(x.is_cuda for x in d["pcd_nonground_chunks"] + d["pcd_ground_chunks"])
    ref = prep_api.chunk_and_downsample_point_clouds(rng_minor, rg_minor, *walk, kitti_labels=rkitti, ctx=ctx)
    assert ref["pcd_nonground_chunks"][0].shape[0] > 5_000
    for key in ("pcd_nonground_chunks", "pcd_ground_chunks", "pcd_nonground_chunks_major_downsampling",
                "pcd_ground_chunks_major_downsampling", "indices", "indices_ground"):
        assert len(d[key]) == len(ref[key])
        for a, b in zip(d[key], ref[key]):
            assert a.cpu().numpy().tobytes() == np.asarray(b).tobytes(), key
    for cloud in ("nonground", "ground"):
        for kind in ("semantic", "instance"):
            for a, b in zip(d["kitti_labels"][cloud][kind], ref["kitti_labels"][cloud][kind]):
                np.testing.assert_array_equal(a.cpu().numpy().astype(np.uint32), b)


class _Entry:
    def __init__(self, points, intensity, words):
        seg, inst, pan = R.decode_labels(words)
        self.point_cloud, self.intensity = points, intensity
        self.semantic_labels, self.instance_labels, self.panoptic_labels = seg.reshape(-1, 1), inst.reshape(-1, 1), pan.reshape(-1, 1)


class _Dataset:
    """What aggregate_pointcloud reads of a dataset: entries with point_cloud, intensity and the three label arrays; get_pose."""

    def __init__(self, m):
        rng = np.random.default_rng(0)
        self.entries = [_Entry(p, rng.random(p.shape[0], dtype=np.float32), w) for p, w in zip(m["scans"], m["labels"])]
        self.poses = m["poses"]

    def __getitem__(self, i):
        return self.entries[i]

    def get_pose(self, i):
        return self.poses[i]


def test_aggregate_pointcloud_gives_the_reference_tuples(ctx):
    m = synth.labelled_scans(6, 1500, seed=2)
    ds = _Dataset(m)
    seen = []

    def segmenter(points, intensity):
        assert points.shape == (intensity.shape[0], 3) and points.dtype == np.float32
        seen.append(points.shape[0])
        return np.flatnonzero(points[:, 2] < -1.6)[::-1]            # an index list in descending order

    first, last = 1, 5
    sub = range(first, last)
    ground = [m["scans"][i][:, 2] < -1.6 for i in sub]
    exp = R.aggregate([m["scans"][i] for i in sub], m["poses"][first:last], [m["labels"][i] for i in sub], ground)
    g, ng, poses, world, labels = prep_api.aggregate_pointcloud(ds, first, last, ground_segmentation=segmenter, ctx=ctx)
    assert seen == [m["scans"][i].shape[0] for i in sub]
    assert g.tobytes() == exp["xyz_ground"].tobytes() and ng.tobytes() == exp["xyz_nonground"].tobytes() and g.shape[0] > 500
    assert len(poses) == 4 and all(np.array_equal(a, m["poses"][i]) for a, i in zip(poses, sub)) and np.array_equal(world, np.eye(4))
    assert sorted(labels) == sorted(KEYS)
    for k in KEYS:
        assert labels[k].shape == (exp[k].shape[0], 1) and labels[k].dtype == np.uint32
        np.testing.assert_array_equal(labels[k][:, 0], exp[k], err_msg=k)
    out = prep_api.aggregate_pointcloud(ds, first, last, ctx=ctx)
    assert len(out) == 2 and len(out[1]) == 4
    every = R.aggregate([m["scans"][i] for i in sub], m["poses"][first:last])
    assert out[0].tobytes() == every["xyz_nonground"].tobytes() and out[0].shape[0] == sum(seen)
    with pytest.raises(NotImplementedError, match="RANSAC"):
        prep_api.aggregate_pointcloud(ds, first, last, ground_segmentation="open3d", ctx=ctx)
    with pytest.raises(NotImplementedError, match="ICP"):
        prep_api.aggregate_pointcloud(ds, first, last, ground_segmentation=segmenter, icp=True, ctx=ctx)
    try:
        import pypatchworkpp  # noqa: F401
    except ImportError:
        with pytest.raises(ImportError, match="pypatchworkpp"):
            prep_api.aggregate_pointcloud(ds, first, last, ground_segmentation="patchwork", ctx=ctx)
