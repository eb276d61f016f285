"""CPU: the pair-list restatement of rules Q2-Q7 (tests/score_inst_ref.py) against the dense host path `labels_api._score_tables` and
``oracle/metrics_ref.score``, bit for bit; the host finish from hit flags against `_average_precision`; the fixtures' claims; and the
new entry point is declared, bound and exported."""
import os
import re

import numpy as np
import pytest

import score_inst_ref as si
import score_ref as sr
from conftest import GOLDEN, ROOT
from oracle import metrics_ref


def host_dicts(preds, gt, threshold, min_points, remove):
    from autoinst_amd import labels_api
    tables, _, _ = sr.ref_tables_fast(preds, gt, threshold, min_points)
    tables = [(pa, pb, cnt, rem, sm) for pa, pb, cnt, rem, sm in tables]
    return labels_api._sweep_scores(tables, min_points, remove)


@pytest.mark.parametrize("seed", range(12))
@pytest.mark.parametrize("min_points", [0, 1, 200])
def test_restatement_equals_the_dense_host_path(seed, min_points):
    pred, gt = si.random_points(seed, negative=seed % 2 == 0, gt_zero=seed % 3 != 0)
    threshold = (0.8, 0.5, 0.3)[seed % 3]
    for remove in (False, True):
        exp = host_dicts([pred], gt, threshold, min_points, remove)[0]
        got = si.ref_dict(si.ref_rows([pred], gt, threshold, min_points, remove)[0])
        si.same_dict(got, exp, (seed, min_points, remove))
        assert all(type(got[key]) is type(exp[key]) for key in exp), (got, exp)
    if seed % 3 == 0:
        assert got["n_gt"] == 0 and np.isnan(got["r"])


def test_the_removal_changes_a_random_score():
    """The fixtures above are no no-ops: in one of them a removed label would have matched."""
    differ = 0
    for seed in range(12):
        pred, gt = si.random_points(seed)
        rows = [si.ref_rows([pred], gt, 0.3, 1, remove)[0] for remove in (False, True)]
        differ += int(rows[0]["n_pred"] != rows[1]["n_pred"]) + 2 * int(rows[0]["tp"][0] != rows[1]["tp"][0])
    assert differ >= 3


def test_no_ground_truth_label_raises_as_the_host_path():
    from autoinst_amd import labels_api
    pred, gt = si.random_points(2, gt_labels=False)
    with pytest.raises(ZeroDivisionError):
        host_dicts([pred], gt, 0.8, 1, False)
    row = si.ref_rows([pred], gt, 0.8, 1, False)[0]
    assert row["n_pred"] > 0 and row["n_gt_labels"] == 0 and np.isnan(row["s_assoc"])
    with pytest.raises(ZeroDivisionError):
        si.ref_dict(row)
    with pytest.raises(ZeroDivisionError):
        labels_api._score_from_hits(row["hits"], row["n_pred"], 0, True, 0, row["s_assoc"])
    # with no scored label either there is nothing to divide: AP 0.0 on both paths
    exp = host_dicts([pred], gt, 0.8, 10 ** 6, False)[0]
    row = si.ref_rows([pred], gt, 0.8, 10 ** 6, False)[0]
    assert row["n_pred"] == 0
    si.same_dict(si.ref_dict(row), exp)
    si.same_dict(labels_api._score_from_hits(row["hits"], 0, 0, True, 0, row["s_assoc"]), exp)


@pytest.mark.parametrize("name", ["scorer_a", "scorer_b"])
def test_restatement_equals_the_oracle_on_the_goldens(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    pred, gt = z["pred"].astype(np.int32), z["gt"].astype(np.int32)
    exp = metrics_ref.score(pred, pred, gt, 200)
    got = si.ref_dict(si.ref_rows([pred], gt, 0.8, 200, False)[0])
    assert all(si.same_value(got[key], v) for key, v in exp.items()), (got, exp)
    removed = sr.remove_semantics(gt, pred, 0.8)
    exp = metrics_ref.score(pred, removed, gt, 200)
    got = si.ref_dict(si.ref_rows([pred], gt, 0.8, 200, True)[0])
    assert all(si.same_value(got[key], v) for key, v in exp.items()), (got, exp)


@pytest.mark.parametrize("n_pred", [0, 1, 7, 8, 9, 128, 129, 1000])
def test_host_finish_equals_average_precision(n_pred):
    """`_ap_from_hits` on arrays against `_average_precision` on the dense table that has exactly these hits: label 1 + i lies on
    its own gt 1 + i (IoU 1) where it hits and on gt 0 where it misses; 5 further gts are never met."""
    from autoinst_amd import labels_api
    rng = np.random.default_rng(n_pred)
    hits = (rng.random(n_pred) < 0.6).astype(np.uint8)
    pa = np.arange(1, n_pred + 1)
    pb = np.where(hits, pa, 0)
    extra = np.arange(n_pred + 1, n_pred + 6)                        # pred 0 on gts nobody else has, and on gt 0
    pa, pb = np.concatenate([[0], pa, np.zeros(5, np.int64)]), np.concatenate([[0], pb, extra])
    order = np.lexsort((pb, pa))
    table = labels_api._Table(pa[order].astype(np.int32), pb[order].astype(np.int32), np.full(pa.size, 10, np.int64))
    n_gt_labels = int((table.cols != 0).sum())
    assert n_gt_labels == int(hits.sum()) + 5
    for o in (0.25, 0.5, 0.95):
        assert labels_api._greedy(table, labels_api._iou(table), o) == [bool(h) for h in hits]
        exp = labels_api._average_precision(table, labels_api._iou(table), o)
        assert labels_api._ap_from_hits(hits, n_gt_labels) == exp
        assert si.ap_by_the_loop(hits, n_gt_labels) == exp
    if n_pred == 0:
        assert labels_api._ap_from_hits(hits, n_gt_labels) == 0.0 and labels_api._ap_from_hits(hits, 0) == 0.0


@pytest.mark.parametrize("pq", si.OVERLAP_FRACTIONS)
def test_the_boundary_quotients_are_the_literals(pq):
    """Rule Q4 at the boundary: (p c) / (q c) is the float64 literal of the overlap for the fixture's scales and up to c = 2^31 - 1,
    and one point less at 1000 times the scale is below it."""
    p, q = pq
    for c in si.BOUNDARY_SCALES + (2 ** 31 - 1, 2 ** 31 - 1 - 12345, 2 ** 30 + 1):
        assert si.quotient_is_the_literal(p, q, c), (p, q, c)


def test_the_boundary_fixture_by_the_restatement():
    pairs, what = si.boundary_pairs()
    assert sum(c for _, _, c in pairs) < 14_000_000
    assert len(what) == len(si.OVERLAPS) * (len(si.BOUNDARY_SCALES) + len(si.BOUNDARY_MISS_SCALES))
    pa, pb, cnt = si.sorted_pair_arrays(pairs)                             # the fixture is large: its pairs are given, not counted
    none = np.zeros(pa.size, bool)
    row = si.ref_row(pa, pb, cnt, none, none, 0, False)
    labels = sorted(what)
    for r, u in enumerate(labels):
        j, hit = what[u]
        assert row["hits"][j, r] == int(hit), (u, j, hit)
        if not hit and j > 0:
            assert row["hits"][j - 1, r] == 1                               # just below this overlap is above the one before


@pytest.mark.parametrize("d,n_gt", [(63, 20), (64, 20), (65, 20)] + [(3 * si.TAKEN_LDS, si.TAKEN_LDS + e) for e in (-1, 0, 1)])
def test_pair_row_has_what_it_claims(d, n_gt):
    """Exactly d pairs and n_gt non-zero gts, and a contest: at 0.25 some label misses although it has a candidate."""
    import label_cases as lc
    pairs = si.pair_row(d, n_gt)
    pred, gt = si.shuffled_points(pairs)
    pa, pb, cnt = lc.ref_label_pairs(pred, gt)
    exp = si.sorted_pair_arrays(pairs)
    assert pa.size == d and np.unique(pb[pb != 0]).size == n_gt and all(np.array_equal(a, b) for a, b in zip((pa, pb, cnt), exp))
    none = np.zeros(d, bool)
    row = si.ref_row(pa, pb, cnt, none, none, 0, False)
    ap = np.bincount(np.unique(pa, return_inverse=True)[1].reshape(-1), weights=cnt)
    gts, gi = np.unique(pb, return_inverse=True)
    ag = np.bincount(gi.reshape(-1), weights=cnt)
    iou = cnt / (ap[np.searchsorted(np.unique(pa), pa)] + ag[gi.reshape(-1)] - cnt)
    with_candidate = np.unique(pa[(pa != 0) & (pb != 0) & (iou >= 0.25)]).size
    assert 0 < row["tp"][0] < with_candidate and row["tp"][-1] < row["tp"][0]


def test_the_entry_point_is_declared_bound_and_exported():
    from autoinst_amd import _ffi
    assert "ai_label_scores" in _ffi.SYMBOLS
    with open(os.path.join(ROOT, "include", "autoinst_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int ai_label_scores\(ai_ctx\* ctx, const int32_t\* pred, const int32_t\* gt, int32_t k, int64_t n,", header, re.M)
    assert header.index("int ai_label_tables(") < header.index("int ai_label_scores(")
    for rule in ("Q1  Tables and flags", "Q2  Labels", "Q3  Areas", "Q4  IoU of a stored pair", "Q5  Greedy match", "Q6  Integers per row",
                 "Q7  S_assoc per row", "Q8  Limits and errors"):
        assert rule in header, rule
    assert "#define AI_ABI_VERSION 6" in header
    lib = _ffi.load()
    assert hasattr(lib, "ai_label_scores") and lib.ai_label_scores.argtypes is not None and len(lib.ai_label_scores.argtypes) == 17
    import autoinst_amd
    from autoinst_amd import labels_api
    assert callable(autoinst_amd.label_scores) and autoinst_amd.label_scores is labels_api.label_scores
    assert labels_api.OVERLAPS == si.OVERLAPS and len(si.OVERLAPS) <= si.MAX_OVERLAPS
    import inspect
    assert inspect.signature(labels_api.score_sweep).parameters["instance_level"].default == "device"
