"""GPU suite: ai_ground_planes / prep_api.ground_planes / aggregate_scans(ground="ransac") / aggregate_pointcloud(
ground_segmentation="ransac") (csrc/ai_ground.hip) against the NumPy restatement tests/ground_ref.py (rules G1-G7 of
include/autoinst_hip.h).

Every comparison is an equality: the flags, best_hyp, best_count, the counts of every hypothesis and the planes bit for bit, from
NumPy inputs and from resident tensors.  The shapes are those of ground_ref.cases(): scans of 0 .. 4 kept points; one scan of one
slab (1024 input points) - 1, +- 0, + 1 and of two slabs + 1; scans whose boundaries disagree with the slabs'; no scans; 1, 255,
256, 257 and 4096 hypotheses (a scoring block holds 256); collinear points, duplicates, two parallel planes with equal
populations, points one float32 from the threshold, NaN and infinite coordinates, each filter on."""
import ctypes as C

import numpy as np
import pytest

import aggregate_ref as R
import ground_ref as G
from autoinst_amd import _ffi, prep_api, synth

pytestmark = pytest.mark.gpu

CASES = G.cases()
OUTPUTS = ("flags", "planes", "best_hyp", "best_count", "hyp_count")


def _host(a):
    return a.cpu().numpy() if hasattr(a, "is_cuda") else np.asarray(a)


@pytest.fixture(scope="module")
def expected():
    return {name: G.ground_planes(**c) for name, c in CASES.items()}


def check(got, exp, what):
    """got: the 5-tuple of prep_api.ground_planes(..., return_counts=True); exp: ground_ref.ground_planes."""
    got = dict(zip(OUTPUTS, (_host(a) for a in got)))
    assert got["flags"].dtype == np.bool_ and got["planes"].dtype == np.float64
    assert got["best_hyp"].dtype == got["best_count"].dtype == got["hyp_count"].dtype == np.int32
    for k in OUTPUTS:
        assert got[k].shape == exp[k].shape, (what, k, got[k].shape, exp[k].shape)
    np.testing.assert_array_equal(got["hyp_count"], exp["hyp_count"], err_msg=f"{what} hyp_count")
    np.testing.assert_array_equal(got["best_hyp"], exp["best_hyp"], err_msg=f"{what} best_hyp")
    np.testing.assert_array_equal(got["best_count"], exp["best_count"], err_msg=f"{what} best_count")
    assert got["planes"].tobytes() == exp["planes"].tobytes(), (what, got["planes"], exp["planes"])
    np.testing.assert_array_equal(got["flags"], exp["flags"], err_msg=f"{what} flags")


def on_device(c, dev):
    """The case as resident tensors: one (M, 3) tensor with offsets, int64 label words."""
    import torch
    off = np.cumsum([0] + [s.shape[0] for s in c["scans"]]).astype(np.int64)
    xyz = np.concatenate(c["scans"]) if c["scans"] else np.zeros((0, 3), np.float32)
    kw = {k: v for k, v in c.items() if k not in ("scans", "labels")}
    kw["labels"] = None if c["labels"] is None else torch.as_tensor(np.concatenate(c["labels"]).astype(np.int64), device=dev)
    return torch.as_tensor(xyz, device=dev), dict(kw, scan_offsets=off)


@pytest.mark.parametrize("name", sorted(CASES))
def test_every_output_equals_the_restatement(name, expected, ctx):
    import torch
    c = CASES[name]
    kw = {k: v for k, v in c.items() if k != "scans"}
    got = prep_api.ground_planes(c["scans"], return_counts=True, ctx=ctx, **kw)
    check(got, expected[name], name)
    again = prep_api.ground_planes(c["scans"], return_counts=True, ctx=ctx, **kw)
    assert all(a.tobytes() == b.tobytes() for a, b in zip(got, again))                      # two calls: bit-identical
    off = np.cumsum([0] + [s.shape[0] for s in c["scans"]])
    for s in range(len(c["scans"])):
        assert got[0][off[s]:off[s + 1]].sum() == got[3][s]                                 # a scan's flags sum to its best count
    xyz, dkw = on_device(c, torch.device("cuda", ctx.device))
    dev = prep_api.ground_planes(xyz, return_counts=True, ctx=ctx, **dkw)
    assert all(a.is_cuda for a in dev) and dev[0].dtype == torch.bool
    check(dev, expected[name], name + " (device)")
    short = prep_api.ground_planes(xyz, ctx=ctx, **dkw)                                     # without the counts: the same four
    assert len(short) == 4 and all(torch.equal(a, b) for a, b in zip(short, dev[:4]))


def test_the_scan_of_the_kept_flags_takes_its_recursive_path(ctx):
    """The kept flags go through the shared scan one element per POINT, so unlike ai_aggregate_scans (one element per tile) this
    entry reaches the scan's recursive path, above 4096 x 2048 = 8 388 608 points.  Three scans of 8 390 657 points, range filter
    on, two hypotheses: a wrong prefix would move every rank of the later scans."""
    import torch
    n = R.SCAN_MAX_DIRECT_TILES * R.SCAN_TILE + 2049
    sizes = [n // 2, 1000, n - n // 2 - 1000]
    rng = np.random.default_rng(6)
    xyz = np.empty((n, 3), dtype=np.float32)
    xyz[:, :2] = rng.uniform(-30.0, 30.0, (n, 2))
    xyz[:, 2] = np.float32(-1.7) + np.float32(0.5) * rng.standard_normal(n, dtype=np.float32)
    off = np.cumsum([0] + sizes).astype(np.int64)
    kw = dict(range_min=3.0, range_max=25.0, distance_threshold=0.4, num_iterations=2, seed=1)
    exp = G.ground_planes([xyz[off[s]:off[s + 1]] for s in range(3)], **kw)
    assert (exp["best_count"] > 100).all() and (exp["best_hyp"] >= 0).all()
    got = prep_api.ground_planes(torch.as_tensor(xyz, device=torch.device("cuda", ctx.device)), scan_offsets=off, return_counts=True,
                                 ctx=ctx, **kw)
    check(got, exp, "recursive scan")


def test_a_scan_alone_with_its_key_equals_its_rows_in_the_map(expected, ctx):
    for name in ("boundaries_disagree", "both_filters"):
        c, exp = CASES[name], expected[name]
        kw = {k: v for k, v in c.items() if k not in ("scans", "labels", "scan_base")}
        off = np.cumsum([0] + [s.shape[0] for s in c["scans"]])
        for s, scan in enumerate(c["scans"]):
            labels = None if c["labels"] is None else [c["labels"][s]]
            one = prep_api.ground_planes([scan], labels=labels, scan_base=c["scan_base"] + s, return_counts=True, ctx=ctx, **kw)
            check(one, {k: (exp[k][off[s]:off[s + 1]] if k == "flags" else exp[k][s:s + 1]) for k in OUTPUTS}, f"{name} scan {s} alone")


def test_the_one_ulp_points(ctx):
    c = CASES["threshold_ulps"]
    flags, planes, best_hyp, best_count = prep_api.ground_planes(c["scans"], distance_threshold=c["distance_threshold"],
                                                                 num_iterations=c["num_iterations"], ctx=ctx)
    assert abs(planes[0, 2]) == 1.0 and not planes[0, [0, 1, 3]].any()                      # the plane z = 0 exactly: dist = |z|
    assert flags[G.ULP_ROWS].tolist() == G.ULP_FLAGS                                        # below: in; at and above: out (strict)
    assert best_count[0] == 202 and flags.sum() == 202


def test_aggregate_scans_with_ransac(ctx):
    """aggregate_scans(ground="ransac") = aggregate_scans(ground=<the flags of ground_planes>) = the restatement of the aggregation
    fed the restatement's flags, bit for bit, from NumPy lists and from resident tensors."""
    import torch
    m = synth.labelled_scans(5, 1400, seed=3)
    filt = dict(moving_index=251, range_min=3.0, range_max=35.0)
    opts = dict(distance_threshold=0.3, num_iterations=300, seed=9, scan_base=4)
    ref = G.ground_planes(m["scans"], labels=m["labels"], **filt, **opts)
    off = np.cumsum([0] + [s.shape[0] for s in m["scans"]])
    masks = [ref["flags"][off[s]:off[s + 1]] for s in range(5)]
    assert all(0.2 < k.mean() < 0.7 for k in masks)                                        # the road is 45 % of a scan
    exp = R.aggregate(m["scans"], m["poses"], m["labels"], masks, **filt)
    flags = prep_api.ground_planes(m["scans"], labels=m["labels"], ctx=ctx, **filt, **opts)[0]
    np.testing.assert_array_equal(flags, ref["flags"])
    for ground, go in (("ransac", opts), (flags, None)):
        g, n, d = prep_api.aggregate_scans(m["scans"], m["poses"], labels=m["labels"], ground=ground, ground_options=go,
                                           return_source=True, ctx=ctx, **filt)
        assert g.tobytes() == exp["xyz_ground"].tobytes() and n.tobytes() == exp["xyz_nonground"].tobytes()
        for k in exp:
            if not k.startswith("xyz"):
                np.testing.assert_array_equal(d[k], exp[k], err_msg=k)
    dev = torch.device("cuda", ctx.device)
    xyz = torch.as_tensor(np.concatenate(m["scans"]), device=dev)
    words = torch.as_tensor(np.concatenate(m["labels"]).astype(np.int64), device=dev)
    g, n, d = prep_api.aggregate_scans(xyz, m["poses"], labels=words, ground="ransac", ground_options=opts, return_source=True,
                                       scan_offsets=off, ctx=ctx, **filt)
    assert g.is_cuda and g.cpu().numpy().tobytes() == exp["xyz_ground"].tobytes() and n.cpu().numpy().tobytes() == exp["xyz_nonground"].tobytes()
    np.testing.assert_array_equal(d["source_ground"].cpu().numpy(), exp["source_ground"])
    with pytest.raises(ValueError):
        prep_api.aggregate_scans(m["scans"], m["poses"], ground="patchwork", ctx=ctx)
    with pytest.raises(ValueError):
        prep_api.aggregate_scans(m["scans"], m["poses"], ground="ransac", ground_options={"iterations": 5}, ctx=ctx)
    with pytest.raises(ValueError):
        prep_api.aggregate_scans(m["scans"], m["poses"], ground=masks, ground_options=opts, ctx=ctx)


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


def test_aggregate_pointcloud_with_ransac_gives_the_reference_tuple(ctx):
    m = synth.labelled_scans(6, 1500, seed=2)
    ds = _Dataset(m)
    first, last = 1, 5
    sub = list(range(first, last))
    scans = [m["scans"][i] for i in sub]
    keys = [f"{k}_{c}" for k in R.KINDS for c in R.CLOUDS]
    for opts in (None, dict(distance_threshold=0.25, num_iterations=128, seed=3)):
        ref = G.ground_planes(scans, **(opts or {}))                         # the scan key is the position in the range
        off = np.cumsum([0] + [s.shape[0] for s in scans])
        masks = [ref["flags"][off[s]:off[s + 1]] for s in range(len(sub))]
        exp = R.aggregate(scans, m["poses"][first:last], [m["labels"][i] for i in sub], masks)
        g, ng, poses, world, labels = prep_api.aggregate_pointcloud(ds, first, last, ground_segmentation="ransac", ground_options=opts,
                                                                    ctx=ctx)
        assert g.tobytes() == exp["xyz_ground"].tobytes() and ng.tobytes() == exp["xyz_nonground"].tobytes() and g.shape[0] > 2000
        assert len(poses) == 4 and all(np.array_equal(a, m["poses"][i]) for a, i in zip(poses, sub)) and np.array_equal(world, np.eye(4))
        assert sorted(labels) == sorted(keys)
        for k in keys:
            assert labels[k].shape == (exp[k].shape[0], 1) and labels[k].dtype == np.uint32
            np.testing.assert_array_equal(labels[k][:, 0], exp[k], err_msg=k)
    with pytest.raises(NotImplementedError, match="RANSAC"):
        prep_api.aggregate_pointcloud(ds, first, last, ground_segmentation="open3d", ctx=ctx)
    with pytest.raises(ValueError):
        prep_api.aggregate_pointcloud(ds, first, last, ground_segmentation=lambda p, i: np.zeros(0, np.int64), ground_options={}, ctx=ctx)


# ----------------------------------------------------------------------------- errors leave the outputs unwritten

FILL = 0xAB


def fresh_outputs(M, n_scans, n_hyp):
    return {"flag": np.full(max(M, 1), FILL, np.uint8), "plane": np.full((max(n_scans, 1), 4), np.nan),
            "best_hyp": np.full(max(n_scans, 1), -FILL, np.int32), "best_count": np.full(max(n_scans, 1), -FILL, np.int32),
            "hyp_count": np.full((max(n_scans, 1), max(min(n_hyp, 8192), 1)), -FILL, np.int32)}


def raw_call(ctx, xyz, off, words=None, moving=-1, rmin=0.0, rmax=-1.0, thr=0.4, n_hyp=32, seed=0, base=0, mem=_ffi.AI_MEM_HOST):
    bufs = fresh_outputs(xyz.shape[0], off.shape[0] - 1, n_hyp)
    ptr = lambda a: None if a is None else a.ctypes.data   # noqa: E731
    st = _ffi.load().ai_ground_planes(ctx._h, ptr(xyz), ptr(off), off.shape[0] - 1, ptr(words), moving, rmin, rmax, thr, n_hyp, seed, base,
                                      mem, *[ptr(bufs[k]) for k in ("flag", "plane", "best_hyp", "best_count", "hyp_count")])
    return st, bufs


def test_errors_leave_the_outputs_unwritten(ctx):
    rng = np.random.default_rng(4)
    p, w = G.make_scan(rng, 1500)
    off = np.array([0, 700, 1500], dtype=np.int64)
    st, clean = raw_call(ctx, p, off, w, 251, 3.0, 25.0)
    exp = G.ground_planes([p[:700], p[700:]], [w[:700], w[700:]], 251, 3.0, 25.0, 0.4, 32)
    assert st == 0 and clean["plane"].tobytes() == exp["planes"].tobytes()
    np.testing.assert_array_equal(clean["flag"], exp["flags"].astype(np.uint8))
    np.testing.assert_array_equal(clean["hyp_count"], exp["hyp_count"])
    bad = {
        "threshold 0": dict(thr=0.0), "threshold < 0": dict(thr=-0.4), "threshold NaN": dict(thr=float("nan")),
        "threshold inf": dict(thr=float("inf")), "no hypotheses": dict(n_hyp=0), "negative n_hyp": dict(n_hyp=-1),
        "4097 hypotheses": dict(n_hyp=4097), "negative scan_base": dict(base=-1), "a key of 2^48": dict(base=(1 << 48) - 1),
        "offsets start at 1": dict(off=np.array([1, 700, 1500], dtype=np.int64)),
        "offsets decrease": dict(off=np.array([0, 900, 800], dtype=np.int64)),
        "range_min > range_max": dict(rmin=25.0, rmax=3.0), "NaN range_min": dict(rmin=float("nan"), rmax=3.0),
        "moving filter without words": dict(words=None), "mem_kind": dict(mem=7),
    }
    for what, change in bad.items():
        a = dict(xyz=p, off=off, words=w, moving=251, rmin=3.0, rmax=25.0)
        a.update(change)
        st, bufs = raw_call(ctx, **a)
        assert st == -1, what
        assert _ffi.load().ai_last_error().decode().startswith("ai_ground_planes:"), what
        untouched = fresh_outputs(p.shape[0], 2, a.get("n_hyp", 32))
        for k, v in bufs.items():
            assert v.tobytes() == untouched[k].tobytes(), (what, k)
    for kw in (dict(distance_threshold=0.0), dict(distance_threshold=float("nan")), dict(num_iterations=0), dict(num_iterations=4097),
               dict(scan_base=-1), dict(range_min=25.0, range_max=3.0), dict(moving_index=251)):
        with pytest.raises(ValueError):
            prep_api.ground_planes([p[:700], p[700:]], ctx=ctx, **kw)
    big = np.array([0, 2 ** 31 - 256], dtype=np.int64)
    st, bufs = raw_call(ctx, p, big)                                                        # ai_aggregate_scans' bound on M
    assert st == -1 and bufs["flag"][0] == FILL
    # not errors: no scans, and the key just below 2^48
    st, z = raw_call(ctx, p[:0], np.array([0], dtype=np.int64))
    assert st == 0 and z["best_hyp"][0] == -FILL
    st, z = raw_call(ctx, p, off, base=(1 << 48) - 2)
    assert st == 0 and (z["best_hyp"] >= 0).all()
