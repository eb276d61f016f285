"""CPU: the NumPy yardstick of `ai_label_tables` (tests/score_ref.py) against hand-computed cases, the boundary of rule S2 and the
argument of rule S3; and the new entry point is declared, bound and exported."""
import os
import re

import numpy as np
import pytest

import score_cases as sc
import score_ref as sr
from conftest import ROOT


def test_remove_semantics_by_hand():
    #             label 1: 3 of 4 on ground   label 2: 1 of 2    label 0: 2 of 2    label -7: 0 of 1
    gt = np.array([0, 0, 0, 9, 0, 4, 0, 0, 3])
    pred = np.array([1, 1, 1, 1, 2, 2, 0, 0, -7])
    assert np.array_equal(sr.remove_semantics(gt, pred, 0.8), pred)                       # 3 > 3.2 is false
    assert np.array_equal(sr.remove_semantics(gt, pred, 0.7), [0, 0, 0, 0, 2, 2, 0, 0, -7])   # 3 > 2.8; 1 > 1.4 is false
    assert np.array_equal(sr.remove_semantics(gt, pred, 0.5), [0, 0, 0, 0, 2, 2, 0, 0, -7])   # 1 > 1.0 is false: strict
    assert np.array_equal(sr.remove_semantics(gt, pred, 0.49), [0, 0, 0, 0, 0, 0, 0, 0, -7])
    out = sr.remove_semantics(gt, pred.astype(np.int64), 0.7)
    assert out.dtype == np.int64 and out is not pred
    assert sr.label_flags(pred, gt, 0.7, 3) == {1: (True, False), 2: (False, True), 0: (True, True), -7: (False, True)}


def test_filter_labels_by_hand():
    lab = np.array([5, 5, 5, 6, 6, 0, -1])
    assert np.array_equal(sr.filter_labels(lab, 3), [5, 5, 5, 0, 0, 0, 0])
    assert np.array_equal(sr.filter_labels(lab, 2), [5, 5, 5, 6, 6, 0, 0])
    assert np.array_equal(sr.filter_labels(lab, 0), lab) and np.array_equal(sr.filter_labels(lab, 1), lab)


def test_ref_tables_by_hand():
    gt = np.array([0, 0, 0, 9, 0, 4, 0, 0, 3])
    pred = np.array([1, 1, 1, 1, 2, 2, 0, 0, -7])
    (tab,), rem, sco = sr.ref_tables([pred], gt, 0.7, 2)
    assert np.array_equal(tab[0], [-7, 0, 1, 1, 2, 2]) and np.array_equal(tab[1], [3, 0, 0, 9, 0, 4])
    assert np.array_equal(tab[2], [1, 2, 3, 1, 1, 1]) and tab[2].dtype == np.int64
    assert np.array_equal(tab[3], [False, True, True, True, False, False])
    assert np.array_equal(tab[4], [True, False, False, False, False, False])
    assert np.array_equal(rem[0], [0, 0, 0, 0, 2, 2, 0, 0, -7]) and np.array_equal(sco[0], [0, 0, 0, 0, 2, 2, 0, 0, 0])


@pytest.mark.parametrize("m", sc.BOUNDARY_M + (sc.BOUNDARY_BIG_M,))
def test_the_boundary_of_the_removal(m):
    """At threshold 0.8 a label with exactly 4 m / 5 points on the ground is kept and one with one more is removed: 0.8 * m in float64
    is not below 4 m / 5 for these m, and is below 4 m / 5 + 1."""
    z = 4 * m // 5
    assert 5 * z == 4 * m
    assert not np.float64(z) > np.float64(0.8) * np.float64(m)
    assert np.float64(z + 1) > np.float64(0.8) * np.float64(m)
    pred, gt, what = sc.boundary_labels((m,))
    out = sr.remove_semantics(gt, pred, 0.8)
    assert what == {10: (m, z), 11: (m, z + 1)}
    assert np.array_equal(out, np.where(pred == 11, 0, pred))
    flags = sr.label_flags(pred, gt, 0.8, 0)
    assert flags == {10: (False, False), 11: (True, False)}


def test_threshold_zero_removes_every_label_that_touches_the_ground():
    rng = np.random.default_rng(4)
    gt = np.where(rng.random(5000) < 0.02, 0, rng.integers(1, 9, 5000))
    pred = rng.integers(-5, 120, 5000)
    out = sr.remove_semantics(gt, pred, 0.0)
    touched = np.unique(pred[gt == 0])
    assert 0 < touched.size < np.unique(pred).size
    assert np.array_equal(out, np.where(np.isin(pred, touched), 0, pred))


@pytest.mark.parametrize("seed", range(6))
def test_small_after_the_removal_iff_small_before(seed):
    """Rule S3: the flags decided on the labels as given reproduce filter_labels(remove_semantics(...)), the scorer's order."""
    rng = np.random.default_rng(seed)
    n = 4000
    gt = np.where(rng.random(n) < 0.4, 0, rng.integers(1, 12, n))
    pred = np.where(gt == 0, rng.integers(0, 6, n), rng.integers(0, 40, n))        # labels 0 .. 5 lie mostly on the ground
    thr, mp = (0.8, 0.5, 0.3)[seed % 3], (55, 60, 65)[seed // 2]          # the labels off the ground have about 60 points
    flags = sr.label_flags(pred, gt, thr, mp)
    removed = np.array([flags[int(u)][0] for u in pred])
    small = np.array([flags[int(u)][1] for u in pred])
    two_step = sr.filter_labels(sr.remove_semantics(gt, pred, thr), mp)
    assert removed.any() and small.any() and not (removed | small).all()
    assert np.array_equal(np.where(removed | small, 0, pred), two_step)
    # and label 0 itself: it grows by the removal, which can only turn it from small to not small -- either way its points are 0
    assert np.all(two_step[pred == 0] == 0)


def test_the_entry_point_is_declared_bound_and_exported():
    from autoinst_amd import _ffi
    assert "ai_label_tables" in _ffi.SYMBOLS
    with open(os.path.join(ROOT, "include", "autoinst_hip.h")) as f:
        header = f.read()
    assert re.search(r"^int ai_label_tables\(ai_ctx\* ctx, const int32_t\* pred, const int32_t\* gt, int32_t k, int64_t n,", header, re.M)
    for rule in ("S1  Tables", "S2  Removal", "S3  Small labels", "S4  What the scorer sees", "S5  Limits and errors"):
        assert rule in header, rule
    lib = _ffi.load()
    assert hasattr(lib, "ai_label_tables") and lib.ai_label_tables.restype is not None
    import autoinst_amd
    for name in ("label_tables", "remove_semantics", "score_sweep"):
        assert callable(getattr(autoinst_amd, name))
