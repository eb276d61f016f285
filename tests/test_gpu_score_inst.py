"""GPU: `ai_label_scores` (rules Q1-Q8 of ``include/autoinst_hip.h``) -- the greedy matching at every overlap and S_assoc per row on
the device -- against the pair-list restatement of tests/score_inst_ref.py, the dense host path (`score_sweep(...,
instance_level="host")`) and ``oracle/metrics_ref.score``.  Every comparison is exact: ``==``, or both NaN."""
import os

import numpy as np
import pytest

import score_cases as sc
import score_inst_ref as si
import score_ref as sr
from conftest import GOLDEN
from oracle import metrics_ref

pytestmark = pytest.mark.gpu

GUARD_I32, GUARD_I64, GUARD_U8, GUARD_F64 = -123456789, -987654321987, 0xA5, -7.25
NO = len(si.OVERLAPS)


def device_rows(ctx, preds, gt, threshold=0.8, min_points=200, remove=True, device=False):
    """`labels_api._device_scores` as `score_inst_ref.ref_row`'s dicts."""
    from autoinst_amd import labels_api
    if device:
        import torch
        preds = torch.as_tensor(np.ascontiguousarray(preds), device="cuda")
        gt = torch.as_tensor(np.ascontiguousarray(gt), device="cuda")
    rows = labels_api._device_scores(preds, gt, threshold, min_points, remove, ctx)
    return [{"hits": h, "n_pred": n_pred, "n_gt_labels": n_gt, "gt_zero": zero, "tp05": tps, "s_assoc": s}
            for h, n_pred, n_gt, zero, tps, s in rows]


def check_rows(got, exp, what):
    assert len(got) == len(exp), what
    for t, (g, e) in enumerate(zip(got, exp)):
        assert g["n_pred"] == e["n_pred"] and g["n_gt_labels"] == e["n_gt_labels"] and g["gt_zero"] == e["gt_zero"], (what, t, g, e)
        assert g["hits"].shape == e["hits"].shape and g["hits"].dtype == np.uint8, (what, t)
        bad = np.argwhere(g["hits"] != e["hits"])
        assert bad.size == 0, (what, t, "first differing (overlap, label rank)", bad[0])
        assert g["tp05"] == int(e["tp"][si.OVERLAPS.index(0.5)]), (what, t)
        assert si.same_value(g["s_assoc"], e["s_assoc"]), (what, t, g["s_assoc"], e["s_assoc"])


def check_case(ctx, preds, gt, threshold=0.8, min_points=200, remove=True, host=True, device=False, what=""):
    """The device's rows equal the restatement's; the dicts of `label_scores` equal the restatement's and (``host``) the dense host
    path's.  Returns the restatement's rows."""
    from autoinst_amd import labels_api
    preds = np.ascontiguousarray(np.asarray(preds, np.int32).reshape(len(preds), -1))
    exp = si.ref_rows(preds, gt, threshold, min_points, remove)
    check_rows(device_rows(ctx, preds, gt, threshold, min_points, remove, device), exp, what)
    got = labels_api.label_scores(preds, gt, threshold=threshold, min_points=min_points, remove=remove, ctx=ctx)
    for t, row in enumerate(exp):
        si.same_dict(got[t], si.ref_dict(row), (what, t))
    if host:
        dense = labels_api.score_sweep(preds, gt, min_points, remove=remove, threshold=threshold, instance_level="host", ctx=ctx)
        for t in range(len(exp)):
            si.same_dict(got[t], dense[t], (what, t, "host"))
    return exp


# ------------------------------------------------------------------------------------------------- Q4: the boundary
def test_iou_boundary_through_the_device(ctx):
    """For every overlap p / q a label with intersection p c and union q c is a hit at that overlap (c = 1, 7, 99 991), and one with
    intersection 1000 p c - 1 and union 1000 q c is a miss there and a hit at the overlap before (c = 1, 7)."""
    pairs, what = si.boundary_pairs()
    pred, gt = si.points_of(pairs)
    row = device_rows(ctx, pred[None, :], gt, 0.8, 0, False)[0]
    labels = sorted(what)
    assert row["n_pred"] == len(labels) and row["n_gt_labels"] == len(labels) and not row["gt_zero"]
    for r, u in enumerate(labels):
        j, hit = what[u]
        assert row["hits"][j, r] == int(hit), (u, si.OVERLAPS[j], hit)
        assert (row["hits"][:j, r] == 1).all() and (row["hits"][j + 1:, r] == 0).all(), (u, row["hits"][:, r])
    none = np.zeros(len(pairs), bool)
    check_rows([row], [si.ref_row(*si.sorted_pair_arrays(pairs), none, none, 0, False)], "boundary")


# ------------------------------------------------------------------------------------------------- Q5: the order
GREEDY_PAIRS = [(0, 0, 3),
                (5, 1, 2), (6, 1, 2),              # IoU 2 / (2 + 4 - 2) = 0.5 each: the smaller label takes gt 1
                (7, 2, 3),                         # 3 / (3 + 5 - 3) = 0.6
                (8, 2, 2), (8, 3, 2),              # 2 / (4 + 5 - 2) = 2/7 and 2 / (4 + 4 - 2) = 1/3: gt 2 is label 7's, so gt 3
                (9, 3, 2)]                         # 2 / (2 + 4 - 2) = 0.5: at 0.25 gt 3 is taken, at 0.5 it is free
GREEDY_HITS = {0.25: [1, 0, 1, 1, 0], 0.5: [1, 0, 1, 0, 1], 0.55: [0, 0, 1, 0, 0], 0.6: [0, 0, 1, 0, 0], 0.65: [0, 0, 0, 0, 0]}


def test_greedy_order_by_hand(ctx):
    pred, gt = si.shuffled_points(GREEDY_PAIRS)
    row = device_rows(ctx, pred[None, :], gt, 0.8, 0, False)[0]
    assert row["n_pred"] == 5 and row["n_gt_labels"] == 3 and row["gt_zero"]
    for j, o in enumerate(si.OVERLAPS):
        assert row["hits"][j].tolist() == GREEDY_HITS.get(o, [0] * 5), o
    assert row["tp05"] == 3
    check_case(ctx, pred[None, :], gt, 0.8, 0, False, what="greedy")


# ------------------------------------------------------------------------------------------------- the 64-pair reads
def straddle_pairs(fillers):
    """``fillers`` one-pair labels on gt 0, then label 1000 with the pairs (1000, 0), (1000, 1), (1000, 2) at positions
    fillers .. fillers + 2 and label 1001 on gt 2.  IoU(1000, 1) = 10 / 21, IoU(1000, 2) = 10 / 31, IoU(1001, 2) = 0.5: at 0.25 label
    1000 takes gt 1 and must leave gt 2 to label 1001, wherever a read ends."""
    return [(1 + i, 0, 1) for i in range(fillers)] + [(1000, 0, 1), (1000, 1, 10), (1000, 2, 10), (1001, 2, 10)]


@pytest.mark.parametrize("fillers", [si.WAVE - 3, si.WAVE - 2, si.WAVE - 1, 2 * si.WAVE - 2])
def test_a_label_across_two_reads_is_matched_once(ctx, fillers):
    pairs = straddle_pairs(fillers)
    pred, gt = si.shuffled_points(pairs)
    row = device_rows(ctx, pred[None, :], gt, 0.8, 0, False)[0]
    assert row["n_pred"] == fillers + 2
    expect = np.zeros((NO, fillers + 2), np.uint8)
    expect[0, fillers:] = 1                       # 0.25: both; 0.5: label 1001 alone
    expect[1, fillers + 1] = 1
    assert np.array_equal(row["hits"], expect)
    check_case(ctx, pred[None, :], gt, 0.8, 0, False, what=("straddle", fillers))


@pytest.mark.parametrize("d", [si.WAVE - 1, si.WAVE, si.WAVE + 1, 3 * si.WAVE + 5])
def test_rows_around_one_read(ctx, d):
    pred, gt = si.shuffled_points(si.pair_row(d, 20))
    for remove in (False, True):
        check_case(ctx, pred[None, :], gt, 0.3, 3, remove, what=("read", d, remove))


def test_a_label_with_more_than_one_read_of_pairs(ctx):
    """Label 7 meets 70 gts with one point each and the last of them, gt 170, with 200: its candidate is its 70th pair.  Label 8
    shares gt 170 and comes too late at 0.25."""
    pairs = [(3, 0, 5)] + [(7, 101 + i, 1) for i in range(69)] + [(7, 170, 200), (8, 170, 150)]
    pred, gt = si.shuffled_points(pairs)
    row = device_rows(ctx, pred[None, :], gt, 0.8, 0, False)[0]
    assert row["n_pred"] == 3 and row["hits"][0].tolist() == [0, 1, 0] and row["hits"][1].tolist() == [0, 0, 0]
    check_case(ctx, pred[None, :], gt, 0.8, 0, False, what="long label")


@pytest.mark.parametrize("n_gt", [si.TAKEN_LDS - 1, si.TAKEN_LDS, si.TAKEN_LDS + 1])
def test_taken_flags_around_the_lds_capacity(ctx, n_gt):
    pred, gt = si.shuffled_points(si.pair_row(3 * si.TAKEN_LDS, n_gt))
    exp = check_case(ctx, pred[None, :], gt, 0.8, 3, True, what=("taken", n_gt))
    assert exp[0]["n_gt_labels"] == n_gt and 0 < exp[0]["tp"][0] < exp[0]["n_pred"]


# ------------------------------------------------------------------------------------------------- labels
@pytest.mark.parametrize("seed", range(4))
def test_negative_labels_and_maps_without_ground(ctx, seed):
    pred, gt = si.random_points(seed, negative=True, gt_zero=seed % 2 == 0)
    assert (pred == -1).any() and (pred < -1).any() and (gt < 0).any()
    for min_points in (0, 1, 200):
        exp = check_case(ctx, pred[None, :], gt, 0.5, min_points, seed < 2, what=("negative", seed, min_points))
    if seed % 2:
        from autoinst_amd import labels_api
        d = labels_api.label_scores(pred[None, :], gt, min_points=1, ctx=ctx)[0]
        assert d["n_gt"] == 0 and np.isnan(d["r"]) and not exp[0]["gt_zero"]


def test_only_ground_raises_as_the_host_path(ctx):
    from autoinst_amd import labels_api
    pred, gt = si.random_points(2, gt_labels=False)
    row = device_rows(ctx, pred[None, :], gt, 0.8, 1, False)[0]
    check_rows([row], si.ref_rows(pred[None, :], gt, 0.8, 1, False), "only ground")
    assert row["n_pred"] > 0 and row["n_gt_labels"] == 0 and row["gt_zero"] and np.isnan(row["s_assoc"])
    for level in ("device", "host"):
        with pytest.raises(ZeroDivisionError):
            labels_api.score_sweep(pred[None, :], gt, 1, remove=False, instance_level=level, ctx=ctx)
    # no scored label: nothing is divided
    exp = check_case(ctx, pred[None, :], gt, 0.8, 10 ** 6, False, what="no scored label")
    assert exp[0]["n_pred"] == 0 and exp[0]["hits"].shape == (NO, 0)


def test_sizes_around_min_points(ctx):
    """min_points 20: labels of 19, 20 and 21 points (19 is small), gts of 19, 20 and 21 points (only 21 is kept: S_assoc is
    21 * (21 / 21) / 21 / 1)."""
    pairs = [(0, 0, 30), (30, 42, 19), (31, 40, 20), (32, 41, 21)]
    pred, gt = si.shuffled_points(pairs)
    row = device_rows(ctx, pred[None, :], gt, 0.8, 20, True)[0]
    assert row["n_pred"] == 2 and row["hits"].tolist() == [[1, 1]] * NO and row["s_assoc"] == 1.0
    check_case(ctx, pred[None, :], gt, 0.8, 20, True, what="min_points")
    for mp in (19, 21):
        check_case(ctx, pred[None, :], gt, 0.8, mp, True, what=("min_points", mp))


# ------------------------------------------------------------------------------------------------- calls
@pytest.mark.parametrize("k", [1, 2, sc.MAX_ROWS])
def test_row_counts(ctx, k):
    c = sc.random_case(k, sc.TILE + 1)
    check_case(ctx, c.preds, c.gt, c.threshold, c.min_points, True, device=k == 2, what=c.name)


def test_remove_on_and_off(ctx):
    """Label 50 has 6 of its 10 points on gt 0 (removed at 0.5) and IoU 4 / 12 with gt 7; label 51 has IoU 2 / 6 with gt 7.  Without
    the removal 50 takes gt 7 at 0.25, with it 51 does."""
    pairs = [(0, 0, 9), (50, 0, 6), (50, 7, 4), (51, 7, 2), (52, 8, 5)]
    pred, gt = si.shuffled_points(pairs)
    off = check_case(ctx, pred[None, :], gt, 0.5, 0, False, what="remove off")[0]
    on = check_case(ctx, pred[None, :], gt, 0.5, 0, True, what="remove on")[0]
    assert off["hits"][0].tolist() == [1, 0, 1] and on["hits"][0].tolist() == [1, 1]
    assert off["s_assoc"] == on["s_assoc"]                      # the association does not see the removal


def test_second_table_beside_three_pairs(ctx):
    d = (sc.FIT_MIN + 300) // 3 * 3
    preds, gt = si.big_rows(d)
    assert sc.FIT_MIN < d <= sc.FIT_MAX
    exp = check_case(ctx, preds, gt, 0.8, 3, True, what="second table")
    assert exp[0]["n_pred"] == d // 3 and exp[0]["tp"][1] == 2 and exp[1]["n_pred"] == 1 and exp[1]["tp"][0] == 1


def test_sort_path_by_the_restatement_alone(ctx):
    """A row of 70 002 distinct pairs (`ai_label_tables` sorts it) at min_points 1, beside a 3-pair row.  The dense host path is not
    run here.  Its (labels x gts) tables would be affordable only because this fixture has three gts -- on a map with thousands of
    gts 23 334 labels allocate gigabytes -- and its `_greedy` makes one NumPy pass per label and overlap, a quarter of a million of
    them for this row: too slow for a test that runs with every suite.  The restatement walks the pairs alone and is proven equal
    to the dense path in tests/test_score_inst_ref.py."""
    d = 70_002
    preds, gt = si.big_rows(d)
    assert d > sc.FIT_MAX
    exp = check_case(ctx, preds, gt, 0.8, 1, True, host=False, what="sort path")
    assert exp[0]["n_pred"] == d // 3 and exp[0]["tp"][1] == 2 and exp[1]["n_pred"] == 1


# ------------------------------------------------------------------------------------------------- the entry itself
def raw_scores(ctx, preds, gt, k=None, n=None, threshold=0.8, min_points=3, mem=None, remove=1, overlaps=si.OVERLAPS, n_overlaps=None,
               cap=1 << 16, null=(), device=False, slack=64):
    """The C entry with guarded outputs: (status, dict of the output arrays)."""
    from autoinst_amd import _ffi
    preds = np.ascontiguousarray(preds, np.int32)
    gt = np.ascontiguousarray(gt, np.int32)
    k = preds.shape[0] if k is None else k
    n = gt.shape[0] if n is None else n
    ov = np.ascontiguousarray(overlaps, np.float64)
    no = ov.size if n_overlaps is None else n_overlaps
    rows = max(preds.shape[0], 1)
    out = {"hits": np.full(max(cap, 0) + slack, GUARD_U8, np.uint8), "hit_off": np.full(rows + 1 + slack, GUARD_I64, np.int64),
           "row_counts": np.full(3 * rows + slack, GUARD_I32, np.int32), "tp": np.full(rows * max(ov.size, 1) + slack, GUARD_I32, np.int32),
           "s_assoc": np.full(rows + slack, GUARD_F64, np.float64)}
    keep = []
    if device:
        import torch
        tp_, tg_ = torch.as_tensor(preds, device="cuda"), torch.as_tensor(gt, device="cuda")
        torch.cuda.synchronize()
        keep += [tp_, tg_]
        p_addr, g_addr, mem_kind = tp_.data_ptr(), tg_.data_ptr(), _ffi.AI_MEM_DEVICE
    else:
        p_addr, g_addr, mem_kind = preds.ctypes.data, gt.ctypes.data, _ffi.AI_MEM_HOST
    addr = {name: (None if name in null else a.ctypes.data) for name, a in out.items()}
    status = _ffi.load().ai_label_scores(
        None if "ctx" in null else ctx._h, None if "pred" in null else p_addr, None if "gt" in null else g_addr, k, n, float(threshold),
        int(min_points), mem_kind if mem is None else mem, remove, None if "overlaps" in null else ov.ctypes.data, no, cap, addr["hits"],
        addr["hit_off"], addr["row_counts"], addr["tp"], addr["s_assoc"])
    return status, out


def untouched(out):
    return ((out["hits"] == GUARD_U8).all() and (out["hit_off"] == GUARD_I64).all() and (out["row_counts"] == GUARD_I32).all()
            and (out["tp"] == GUARD_I32).all() and (out["s_assoc"] == GUARD_F64).all())


@pytest.fixture(scope="module")
def small():
    c = sc.random_case(2, sc.TILE + 1)
    return c.preds, c.gt


def test_host_and_device_inputs_and_two_runs_agree_in_bytes(ctx, small):
    preds, gt = small
    runs = [raw_scores(ctx, preds, gt, min_points=40, device=dev) for dev in (False, True, True)]
    assert all(status == 0 for status, _ in runs)
    assert int(runs[0][1]["hit_off"][2]) > 0
    for _, out in runs[1:]:
        for name, a in out.items():
            assert a.tobytes() == runs[0][1][name].tobytes(), name


def test_capacity_rule(ctx, small):
    preds, gt = small
    status, full = raw_scores(ctx, preds, gt, min_points=40)
    total = int(full["hit_off"][2]) * NO
    assert status == 0 and 0 < total < 1 << 16
    assert (full["hits"][total:] == GUARD_U8).all() and set(np.unique(full["hits"][:total])) <= {0, 1}
    assert full["hit_off"][0] == 0 and (full["hit_off"][3:] == GUARD_I64).all() and (full["row_counts"][6:] == GUARD_I32).all()
    assert (full["tp"][2 * NO:] == GUARD_I32).all() and (full["s_assoc"][2:] == GUARD_F64).all()
    for cap in (0, 1, total - 1, total):
        status, out = raw_scores(ctx, preds, gt, min_points=40, cap=cap, null=("hits",) if cap == 0 else ())
        assert status == 0
        assert np.array_equal(out["hits"][:cap], full["hits"][:cap]) and (out["hits"][cap:] == GUARD_U8).all(), cap
        for name in ("hit_off", "row_counts", "tp", "s_assoc"):
            assert out[name].tobytes() == full[name].tobytes(), (cap, name)


def test_no_points_is_no_error(ctx):
    status, out = raw_scores(ctx, np.zeros((3, 0), np.int32), np.zeros(0, np.int32), null=("pred", "gt"))
    assert status == 0
    assert (out["hit_off"][:4] == 0).all() and (out["row_counts"][:9] == 0).all() and (out["tp"][:3 * NO] == 0).all()
    assert np.isnan(out["s_assoc"][:3]).all() and (out["hits"] == GUARD_U8).all()
    assert (out["hit_off"][4:] == GUARD_I64).all() and (out["row_counts"][9:] == GUARD_I32).all() and (out["s_assoc"][3:] == GUARD_F64).all()
    from autoinst_amd import labels_api
    d = labels_api.label_scores(np.zeros((1, 0), np.int32), np.zeros(0, np.int32), ctx=ctx)[0]
    assert d["ap"] == 0.0 and d["n_pred"] == 0 and np.isnan(d["S_assoc"]) and np.isnan(d["p"])


BAD = {
    "k = 0": dict(k=0), "k = 65": dict(k=sc.MAX_ROWS + 1), "n < 0": dict(n=-1), "n = 2^31 - 1": dict(n=2 ** 31 - 1),
    "threshold NaN": dict(threshold=float("nan")), "threshold inf": dict(threshold=float("inf")), "threshold < 0": dict(threshold=-0.5),
    "min_points < 0": dict(min_points=-1), "mem_kind": dict(mem=7), "no overlaps": dict(n_overlaps=0),
    "17 overlaps": dict(overlaps=[0.5] * (si.MAX_OVERLAPS + 1)), "overlap 0": dict(overlaps=[0.5, 0.0]),
    "overlap < 0": dict(overlaps=[-0.25]), "overlap > 1": dict(overlaps=[0.5, 1.0000000000000002]), "overlap NaN": dict(overlaps=[float("nan")]),
    "overlap inf": dict(overlaps=[float("inf")]), "null overlaps": dict(null=("overlaps",)), "null ctx": dict(null=("ctx",)),
    "null pred": dict(null=("pred",)), "null gt": dict(null=("gt",)), "null hits": dict(null=("hits",)), "null hit_off": dict(null=("hit_off",)),
    "null row_counts": dict(null=("row_counts",)), "null tp": dict(null=("tp",)), "null s_assoc": dict(null=("s_assoc",)), "cap < 0": dict(cap=-1),
}


@pytest.mark.parametrize("what", sorted(BAD))
def test_bad_arguments_leave_every_output_untouched(ctx, small, what):
    from autoinst_amd import _ffi
    status, out = raw_scores(ctx, *small, **BAD[what])
    assert status == -1 and untouched(out), what                # AI_ERR_BAD_ARG
    assert _ffi.load().ai_last_error().decode().startswith("ai_label_scores:")


def test_the_limits_themselves_are_accepted(ctx, small):
    """16 overlaps, among them 1.0 and the smallest float64 above 0 (every stored pair with gt != 0 is a candidate), threshold 0 and
    min_points 0."""
    overlaps = [1.0, 5e-324] + [0.5] * (si.MAX_OVERLAPS - 2)
    preds, gt = small
    status, out = raw_scores(ctx, preds, gt, overlaps=overlaps, threshold=0.0, min_points=0)
    assert status == 0 and int(out["hit_off"][2]) > 0
    exp = si.ref_rows(preds, gt, 0.0, 0, True, overlaps)
    for t in range(2):
        a, b = int(out["hit_off"][t]) * si.MAX_OVERLAPS, int(out["hit_off"][t + 1]) * si.MAX_OVERLAPS
        assert np.array_equal(out["hits"][a:b].reshape(si.MAX_OVERLAPS, -1), exp[t]["hits"]), t
        assert np.array_equal(out["tp"][t * si.MAX_OVERLAPS:(t + 1) * si.MAX_OVERLAPS], exp[t]["tp"])
    assert exp[0]["tp"][1] > exp[0]["tp"][2]


# ------------------------------------------------------------------------------------------------- end to end
@pytest.fixture(scope="module")
def stacked():
    """tests/test_gpu_score.py's rows: scorer_a / scorer_b, each with two relabelled copies and one row whose instances lie on the
    ground."""
    out = {}
    for name in ("scorer_a", "scorer_b"):
        z = np.load(os.path.join(GOLDEN, name + ".npz"))
        pred, gt = z["pred"].astype(np.int32), z["gt"].astype(np.int32)
        rng = np.random.default_rng(len(name) + pred.size)
        rows = [pred]
        top = int(pred.max()) + 1
        for _ in range(2):
            m = np.concatenate([[0], 1 + rng.permutation(top + 5)])[: top + 1]
            rows.append(np.where(pred >= 0, m[np.maximum(pred, 0)], pred).astype(np.int32))
        rows.append(np.where((gt == 0) & (rng.random(gt.size) < 0.9), top + 7 + (np.arange(gt.size) % 3), pred).astype(np.int32))
        out[name] = (np.stack(rows), gt)
    return out


@pytest.mark.parametrize("name", ["scorer_a", "scorer_b"])
@pytest.mark.parametrize("remove", [False, True])
def test_score_sweep_device_equals_host_and_the_oracle(ctx, stacked, name, remove):
    import torch
    from autoinst_amd import labels_api
    preds, gt = stacked[name]
    p, g = torch.as_tensor(preds, device="cuda"), torch.as_tensor(gt, device="cuda")
    dev = labels_api.score_sweep(p, g, 200, remove=remove, ctx=ctx)                       # the default is the device
    host = labels_api.score_sweep(p, g, 200, remove=remove, instance_level="host", ctx=ctx)
    from_host_arrays = labels_api.score_sweep(preds, gt, 200, remove=remove, instance_level="device", ctx=ctx)
    for t in range(preds.shape[0]):
        si.same_dict(dev[t], host[t], (name, t))
        si.same_dict(dev[t], from_host_arrays[t], (name, t, "host arrays"))
        oracle = metrics_ref.score(preds[t], sr.remove_semantics(gt, preds[t], 0.8) if remove else preds[t], gt, 200)
        assert all(si.same_value(dev[t][key], v) for key, v in oracle.items()), (name, t, dev[t], oracle)
    with pytest.raises(ValueError):
        labels_api.score_sweep(p, g, 200, instance_level="dense", ctx=ctx)


def test_score_sweep_of_a_cut_tree_left_on_the_device(ctx):
    import torch
    from autoinst_amd import labels_api, ncuts_api, synth
    ch = synth.synthetic_chunk(20_000, 11, tarl=True)
    g = ncuts_api.build_affinity(ch["points"], ch["tarl"], alpha=1.0, theta=0.5, gamma=0.0, ctx=ctx)
    tree = ncuts_api.ncuts_tree(g, 20_000, 0.03)
    g.free()
    labels, _ = ncuts_api.relabel([tree], [0.005, 0.01, 0.02, 0.03], device=torch.device("cuda"), ctx=ctx)
    gt = ch["gt"].copy()
    gt[::97] = 0
    rows = [labels[t][0] + 1 for t in range(4)]
    tg = torch.as_tensor(gt, device="cuda")
    for remove in (False, True):
        dev = labels_api.score_sweep(rows, tg, 200, remove=remove, instance_level="device", ctx=ctx)
        host = labels_api.score_sweep(rows, tg, 200, remove=remove, instance_level="host", ctx=ctx)
        for t in range(4):
            si.same_dict(dev[t], host[t], (remove, t))
            p = rows[t].cpu().numpy()
            oracle = metrics_ref.score(p, sr.remove_semantics(gt, p, 0.8) if remove else p, gt, 200)
            assert all(si.same_value(dev[t][key], v) for key, v in oracle.items()), (remove, t)


def test_metrics_update_stats_on_tensors_over_two_updates(ctx, stacked):
    import torch
    from autoinst_amd import labels_api
    preds, gt = stacked["scorer_b"]
    removed = sr.remove_semantics(gt, preds[3], 0.8)
    assert (removed != preds[3]).any()
    host, dev = labels_api.Metrics("h", min_points=200, ctx=ctx), labels_api.Metrics("d", min_points=200, ctx=ctx)
    tg = torch.as_tensor(gt, device="cuda")
    for alll, pred in ((preds[2], preds[2]), (preds[3], removed)):
        a = host.update_stats(alll, pred, gt)
        ta = torch.as_tensor(alll, device="cuda")
        b = dev.update_stats(ta, ta if pred is alll else torch.as_tensor(pred, device="cuda"), tg)
        assert a == b
    assert host.sequence_metrics == dev.sequence_metrics
    s = labels_api.score(torch.as_tensor(preds[3], device="cuda"), torch.as_tensor(removed, device="cuda"), tg, 200, ctx=ctx)
    assert all(si.same_value(s[key], v) for key, v in metrics_ref.score(preds[3], removed, gt, 200).items())
