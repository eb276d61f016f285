"""CPU suite: tests/aggregate_ref.py (the restatement of ai_aggregate_scans, rules A1-A6) against the reference's own expressions
where they can be evaluated without open3d and pykitti -- the three label decodes (kitti_odometry_dataset.py:73-104) and the two
filter predicates (kitti_gt_mo_filter.py:40-51, range_filter.py:23-29), written out on arrays -- and against a plain per-scan loop
of mask, index, transform and np.concatenate.  Then: each of five wrong rules is rejected by at least one shared case."""
import numpy as np
import pytest

import aggregate_ref as R
from autoinst_amd import camera_api

CASES = R.cases()


def reference_label_decodes(labels_orig):
    """The three decodes as the reference writes them, `& 0xFFFF + 10` included."""
    semantic = (labels_orig & 0xFFFF).reshape((-1, 1))
    panoptic = (labels_orig & 0xFFFF0000).reshape((-1, 1))
    zero = np.where(panoptic == 0)
    panoptic[zero] = semantic[zero]
    instance = (labels_orig & 0xFFFF0000).reshape((-1, 1)) * (labels_orig & 0xFFFF + 10).reshape((-1, 1))
    return semantic, instance, panoptic


def test_label_decodes_equal_the_reference_expressions():
    rng = np.random.default_rng(0)
    words = np.concatenate([R.special_words(), R.make_scan(rng, 5000)[1], rng.integers(0, 1 << 32, 5000, dtype=np.uint64).astype(np.uint32)])
    seg, inst, pan = R.decode_labels(words)
    rs, ri, rp = reference_label_decodes(words.copy())
    assert rs.dtype == ri.dtype == rp.dtype == np.uint32 and rs.shape == (words.shape[0], 1)
    np.testing.assert_array_equal(seg, rs[:, 0])
    np.testing.assert_array_equal(inst, ri[:, 0])
    np.testing.assert_array_equal(pan, rp[:, 0])
    assert (0xFFFF + 10) == 0x10009
    exact = (words & np.uint32(0xFFFF0000)).astype(np.uint64) * (words & np.uint32(0x10009)).astype(np.uint64)
    assert np.any(exact >= 1 << 32) and np.any((exact < 1 << 32) & (exact > 0))       # wrapping and non-wrapping products


def test_filter_predicates_equal_the_reference_expressions():
    rng = np.random.default_rng(1)
    pts = np.concatenate([R.ulp_points(), R.make_scan(rng, 20000)[0]])
    words = np.concatenate([R.special_words(), R.make_scan(rng, pts.shape[0] - R.special_words().shape[0])[1]])
    for min_range, max_range in ((3.0, 25.0), (0.1, 12.3), (0.0, 1e30)):
        norm = np.linalg.norm(pts, axis=1)
        assert norm.dtype == np.float32
        expected = np.logical_and(norm <= max_range, norm >= min_range)
        np.testing.assert_array_equal(R.keep_mask(pts, range_min=min_range, range_max=max_range), expected)
    np.testing.assert_array_equal(R.range_norm(pts), np.linalg.norm(pts, axis=1))
    for moving in (251, 0, 1, 0x10000):
        np.testing.assert_array_equal(R.keep_mask(pts, words, moving_index=moving), (words & (2 ** 16 - 1)) < moving)
    r = R.range_norm(R.ulp_points())
    for edge in (3.0, 25.0):       # the fixture sits on both edges and one ulp to either side
        e = np.float32(edge)
        assert np.any(r == e) and np.any(r == np.nextafter(e, np.float32(0))) and np.any(r == np.nextafter(e, np.float32(99)))
    assert R.range_norm(np.array([[15, 20, 0]], np.float32))[0] == np.float32(25)


def loop_aggregate(scans, poses, labels=None, ground=None, moving_index=None, range_min=None, range_max=None):
    """The reference's loop shape: per scan mask, index, transform, then np.concatenate per map."""
    parts = {c: {k: [] for k in ("xyz", "source") + R.KINDS} for c in R.CLOUDS}
    offsets = {c: [0] for c in R.CLOUDS}
    start = 0
    for s, pts in enumerate(scans):
        pts = np.asarray(pts, dtype=np.float32)[:, :3]
        w = None if labels is None else np.asarray(labels[s], dtype=np.uint32)
        keep = np.ones(pts.shape[0], dtype=bool)
        if moving_index is not None:
            keep &= (w & 0xFFFF) < moving_index
        if range_min is not None or range_max is not None:
            norm = np.linalg.norm(pts, axis=1)
            keep &= np.logical_and(norm <= (np.inf if range_max is None else range_max), norm >= (0.0 if range_min is None else range_min))
        g = np.zeros(pts.shape[0], dtype=bool) if ground is None else np.asarray(ground[s], dtype=bool)
        for cloud, idx in (("ground", np.flatnonzero(keep & g)), ("nonground", np.flatnonzero(keep & ~g))):
            with np.errstate(invalid="ignore"):
                parts[cloud]["xyz"].append(camera_api.transform_points(pts[idx].astype(np.float64), poses[s]))
            parts[cloud]["source"].append(idx + start)
            offsets[cloud].append(offsets[cloud][-1] + idx.shape[0])
            if w is not None:
                for kind, a in zip(R.KINDS, R.decode_labels(w[idx])):
                    parts[cloud][kind].append(a)
        start += pts.shape[0]
    out = {}
    for c in R.CLOUDS:
        out[f"xyz_{c}"] = np.concatenate(parts[c]["xyz"]) if scans else np.zeros((0, 3))
        out[f"source_{c}"] = np.concatenate(parts[c]["source"]) if scans else np.zeros(0, np.int64)
        out[f"offsets_{c}"] = np.array(offsets[c], dtype=np.int64)
        if labels is not None:
            for kind in R.KINDS:
                out[f"{kind}_{c}"] = np.concatenate(parts[c][kind]) if scans else np.zeros(0, np.uint32)
    return out


def assert_same(got, exp, what=""):
    assert sorted(got) == sorted(exp), what
    for k in exp:
        assert got[k].shape == exp[k].shape, (what, k)
        assert got[k].dtype == exp[k].dtype, (what, k)
        assert got[k].tobytes() == exp[k].tobytes(), (what, k)


@pytest.mark.parametrize("name", sorted(CASES))
def test_restatement_equals_the_per_scan_loop(name):
    assert_same(R.aggregate(**CASES[name]), loop_aggregate(**CASES[name]), name)


def test_the_cases_cover_both_classes_and_the_drops():
    kept = {n: R.aggregate(**c) for n, c in CASES.items()}
    assert kept["all_ground"]["xyz_nonground"].shape[0] == 0 < kept["all_ground"]["xyz_ground"].shape[0]
    assert kept["all_nonground"]["xyz_ground"].shape[0] == 0 < kept["all_nonground"]["xyz_nonground"].shape[0]
    assert kept["all_dropped"]["xyz_ground"].shape[0] == kept["all_dropped"]["xyz_nonground"].shape[0] == 0
    assert kept["nan_is_dropped"]["source_nonground"].tolist() == [3]
    total = sum(s.shape[0] for s in CASES["both_filters_off"]["scans"])
    assert kept["both_filters_off"]["xyz_ground"].shape[0] + kept["both_filters_off"]["xyz_nonground"].shape[0] == total


# ----------------------------------------------------------------------------- wrong rules

def _differs(a, b):
    return any(a[k].shape != b[k].shape or a[k].tobytes() != b[k].tobytes() for k in b)


def _rejected(wrong):
    """The names of the shared cases on which `wrong(case, right result)` gives another result than the restatement."""
    return [n for n, c in CASES.items() if _differs(wrong(c, R.aggregate(**c)), R.aggregate(**c))]


def _with_instance(c, right, fn):
    out = dict(right)
    if c["labels"] is not None:
        words = np.concatenate(c["labels"]) if c["labels"] else np.zeros(0, np.uint32)
        for cloud in R.CLOUDS:
            out[f"instance_{cloud}"] = fn(words[right[f"source_{cloud}"]])
    return out


def test_instance_mask_0xffff_is_rejected():
    wrong = lambda c, r: _with_instance(c, r, lambda w: (w & np.uint32(0xFFFF0000)) * (w & np.uint32(0xFFFF)))   # noqa: E731
    assert "special_words_unfiltered" in _rejected(wrong)


def test_uint64_product_is_rejected():
    def wide(w):
        return ((w & np.uint32(0xFFFF0000)).astype(np.uint64) * (w & np.uint32(0x10009)).astype(np.uint64))
    bad = _rejected(lambda c, r: _with_instance(c, r, wide))
    assert "special_words_unfiltered" in bad
    # and not by the dtype alone: the values differ where the product wraps
    w = R.special_words()
    assert np.any(wide(w) != R.decode_labels(w)[1].astype(np.uint64))


def _with_keep(c, keep_fn):
    """The restatement with another range predicate: keep_fn(float32 points) -> bool."""
    off = np.cumsum([0] + [s.shape[0] for s in c["scans"]])
    xyz = np.concatenate(c["scans"])
    mask = keep_fn(xyz)
    # feed the wrong predicate's survivors to the restatement with the range filter off
    scans = [xyz[off[s]:off[s + 1]][mask[off[s]:off[s + 1]]] for s in range(len(c["scans"]))]
    ground = None if c["ground"] is None else [np.asarray(c["ground"][s])[mask[off[s]:off[s + 1]]] for s in range(len(scans))]
    return R.aggregate(scans, c["poses"], None, ground, None, None, None)


def test_exclusive_range_ends_are_rejected():
    c = CASES["range_ulps"]
    right = R.aggregate(**c)
    r = R.range_norm(np.concatenate(c["scans"]))
    wrong = _with_keep(c, lambda p: (R.range_norm(p) > np.float32(3)) & (R.range_norm(p) < np.float32(25)))
    assert int(np.sum(r == np.float32(3))) >= 2 and int(np.sum(r == np.float32(25))) >= 2
    assert wrong["xyz_ground"].shape[0] + wrong["xyz_nonground"].shape[0] < right["xyz_ground"].shape[0] + right["xyz_nonground"].shape[0]


def test_float64_norm_is_rejected():
    c = CASES["range_ulps"]
    right = R.aggregate(**c)

    def norm64(p):
        q = p.astype(np.float64)
        r = np.sqrt((q[:, 0] * q[:, 0] + q[:, 1] * q[:, 1]) + q[:, 2] * q[:, 2])
        return (r >= 3.0) & (r <= 25.0)
    wrong = _with_keep(c, norm64)
    n_right = right["xyz_ground"].shape[0] + right["xyz_nonground"].shape[0]
    n_wrong = wrong["xyz_ground"].shape[0] + wrong["xyz_nonground"].shape[0]
    print(f"kept by the float32 rule: {n_right}, by a float64 norm: {n_wrong}")
    assert n_wrong != n_right


def test_ground_before_nonground_order_is_rejected():
    """One map that lists a scan's ground points in front of its non-ground points (what concatenating get_subpcd results would
    give) is not in ascending input position."""
    c = CASES["ground_none"]
    right = R.aggregate(**c)
    flags = [R.make_scan(np.random.default_rng(5), s.shape[0])[2] for s in c["scans"]]
    off = np.cumsum([0] + [s.shape[0] for s in c["scans"]])
    order = np.concatenate([np.concatenate([np.flatnonzero(f), np.flatnonzero(~f)]) + off[s] for s, f in enumerate(flags)])
    keep = R.keep_mask(np.concatenate(c["scans"]), np.concatenate(c["labels"]), c["moving_index"], c["range_min"], c["range_max"])
    wrong_source = order[keep[order]]
    assert sorted(wrong_source.tolist()) == right["source_nonground"].tolist()
    assert wrong_source.tolist() != right["source_nonground"].tolist()
    assert np.all(np.diff(right["source_nonground"]) > 0) and np.all(np.diff(right["source_ground"]) > 0)


def test_big_case_crosses_the_scan_block_boundary():
    assert R.BIG_POINTS == 2_098_177 and -(-R.BIG_POINTS // R.TILE) == 2050 > R.SCAN_TILE
    assert R.SCAN_MAX_DIRECT_TILES * R.SCAN_TILE * R.TILE > 2 ** 31       # the recursive scan path is beyond the limit on M
