"""GPU: `ai_label_tables` on the fixtures of tests/score_cases.py, every answer compared exactly with tests/score_ref.py."""
import ctypes as C

import numpy as np
import pytest

import label_cases as lc
import score_cases as sc
import score_ref as sr

pytestmark = pytest.mark.gpu

GUARD_I32, GUARD_I64, GUARD_U8 = -123456789, -987654321987, 0xA5


def tables_of(ctx, c, *, device=False, labels=True):
    from autoinst_amd import labels_api
    preds, gt = c.preds, c.gt
    if device:
        import torch
        preds, gt = torch.as_tensor(preds, device="cuda"), torch.as_tensor(gt, device="cuda")
    out = labels_api.label_tables(preds, gt, threshold=c.threshold, min_points=c.min_points, return_labels=labels, ctx=ctx)
    if not labels:
        return out, None, None
    tabs, rem, sco = out
    if device:
        assert rem.is_cuda and sco.is_cuda
        rem, sco = rem.cpu().numpy(), sco.cpu().numpy()
    return tabs, rem, sco


def check_case(ctx, c, ref=sr.ref_tables, **kw):
    exp_t, exp_r, exp_s = ref(c.preds, c.gt, c.threshold, c.min_points)
    tabs, rem, sco = tables_of(ctx, c, **kw)
    sr.check_tables(c.name, tabs, exp_t)
    assert rem.dtype == np.int32 and sco.dtype == np.int32
    assert lc.first_difference(rem, exp_r) is None, c.name + " pred_removed: " + str(lc.first_difference(rem, exp_r))
    assert lc.first_difference(sco, exp_s) is None, c.name + " pred_scored: " + str(lc.first_difference(sco, exp_s))
    return tabs, rem, sco


def raw_call(ctx, preds, gt, k, n, threshold, min_points, cap, total_cap, want_labels=True):
    """The C entry point on host arrays with guarded outputs: (status, pa, pb, cnt, flags, row_off, rem, sco)."""
    from autoinst_amd import _ffi
    pa, pb = np.full(total_cap, GUARD_I32, np.int32), np.full(total_cap, GUARD_I32, np.int32)
    cnt, fl = np.full(total_cap, GUARD_I64, np.int64), np.full(total_cap, GUARD_U8, np.uint8)
    off = np.full(max(k, 0) + 2, GUARD_I64, np.int64)
    size = max(k, 1) * max(n, 1) if 0 <= n < 2 ** 24 else 16         # a refused call writes nothing: no need for the room
    rem, sco = np.full(size, GUARD_I32, np.int32), np.full(size, GUARD_I32, np.int32)
    status = _ffi.load().ai_label_tables(ctx._h, preds.ctypes.data, gt.ctypes.data, k, n, float(threshold), int(min_points), _ffi.AI_MEM_HOST,
                                         cap, pa.ctypes.data, pb.ctypes.data, cnt.ctypes.data, fl.ctypes.data, off.ctypes.data,
                                         rem.ctypes.data if want_labels else None, sco.ctypes.data if want_labels else None)
    return status, pa, pb, cnt, fl, off, rem, sco


@pytest.mark.parametrize("name", sc.SMALL_NAMES)
def test_small_fixtures(ctx, name):
    """Lengths around one tile, 1 to 64 rows, tiles around the LDS table's slots and with a pair per point, the extreme labels and
    keys, the S2 boundary (label 0 flagged, its points unchanged) and the label sizes around min_points."""
    c = sc.small_case(name)
    tabs, rem, sco = check_case(ctx, c)
    if name == "boundary":
        (pa, pb, cnt, removed, small), = tabs
        assert removed[pa == 0].all() and np.array_equal(rem[0][c.preds[0] == 0], np.zeros(12, np.int32))
        assert not removed[pa == 10].any() and removed[pa == 11].all()


def test_threshold_zero(ctx):
    c = sc.boundary_case(name="boundary_thr0", threshold=0.0)
    (tab,), rem, _ = check_case(ctx, c)
    assert all(bool(tab[3][tab[0] == u][0]) == (z >= 1) for u, (m, z) in c.claims["labels"].items())


def test_the_boundary_at_five_million_points(ctx):
    c = sc.boundary_case(ms=(sc.BOUNDARY_BIG_M,), name="boundary_big")
    (tab,), rem, _ = check_case(ctx, c, ref=sr.ref_tables_fast)
    pa, _, _, removed, _ = tab
    assert not removed[pa == 10].any() and removed[pa == 11].all()


@pytest.mark.parametrize("which", range(3))
def test_rows_around_the_first_table(ctx, which):
    check_case(ctx, sc.table_cases()[which], ref=sr.ref_tables_fast)


def test_rows_around_the_largest_table_side_by_side(ctx):
    """One row that fits the largest table, one that is sorted and one with three pairs in one call: each equals ref_label_pairs."""
    c = sc.fallback_case()
    tabs, _, _ = check_case(ctx, c, ref=sr.ref_tables_fast)
    for t in range(3):
        lc.check_label_pairs(f"{c.name} row {t}", tabs[t][:3], lc.ref_label_pairs(c.preds[t], c.gt))
    assert [tab[0].size for tab in tabs] == c.claims["distinct"]


def test_eight_million_points_of_one_pair(ctx):
    c = sc.one_pair_case()
    (tab,), rem, sco = tables_of(ctx, c, device=True)
    assert [x.tolist() for x in tab] == [[3], [0], [sc.ONE_PAIR_POINTS], [True], [False]]
    assert not rem.any() and not sco.any()


@pytest.mark.parametrize("name", ["random_k16_n%d" % (sc.TILE + 1), "extremes", "tile_every_point_a_pair"])
def test_device_inputs_give_the_same_bytes(ctx, name):
    c = sc.small_case(name)
    host = tables_of(ctx, c)
    dev = check_case(ctx, c, device=True)
    for h, d in zip(host[0], dev[0]):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(h, d))
    assert host[1].tobytes() == dev[1].tobytes() and host[2].tobytes() == dev[2].tobytes()


def test_two_runs_give_the_same_bytes(ctx):
    c = sc.table_cases()[2]
    one, two = tables_of(ctx, c, device=True), tables_of(ctx, c, device=True)
    for h, d in zip(one[0], two[0]):
        assert all(a.tobytes() == b.tobytes() for a, b in zip(h, d))
    assert one[1].tobytes() == two[1].tobytes() and one[2].tobytes() == two[2].tobytes()


def test_the_tables_alone(ctx):
    c = sc.small_case("random_k2_n%d" % (sc.TILE + 1))
    tabs, _, _ = tables_of(ctx, c, labels=False)
    sr.check_tables(c.name, tabs, sr.ref_tables(c.preds, c.gt, c.threshold, c.min_points)[0])


def test_capacity_rules(ctx):
    """cap = 0, 1, total - 1, total, total + 3: row_off always full, exactly the leading cap pairs written, the per-point outputs
    complete."""
    c = sc.small_case("random_k2_n%d" % (sc.TILE + 1))
    k, n = c.preds.shape
    exp_t, exp_r, exp_s = sr.ref_tables(c.preds, c.gt, c.threshold, c.min_points)
    cat = [np.concatenate([t[j] for t in exp_t]) for j in range(3)]
    fl = np.concatenate([t[3].astype(np.uint8) | (t[4].astype(np.uint8) << 1) for t in exp_t])
    total = cat[0].size
    offs = np.concatenate([[0], np.cumsum([t[0].size for t in exp_t])])
    for cap in (0, 1, total - 1, total, total + 3):
        st, pa, pb, cnt, flg, off, rem, sco = raw_call(ctx, c.preds, c.gt, k, n, c.threshold, c.min_points, cap, total + 8)
        m = min(cap, total)
        assert st == 0 and np.array_equal(off[:k + 1], offs) and off[k + 1] == GUARD_I64, cap
        assert np.array_equal(pa[:m], cat[0][:m]) and np.array_equal(pb[:m], cat[1][:m]) and np.array_equal(cnt[:m], cat[2][:m]), cap
        assert np.array_equal(flg[:m], fl[:m]), cap
        assert np.all(pa[m:] == GUARD_I32) and np.all(pb[m:] == GUARD_I32) and np.all(cnt[m:] == GUARD_I64) and np.all(flg[m:] == GUARD_U8), cap
        assert np.array_equal(rem.reshape(k, n), exp_r) and np.array_equal(sco.reshape(k, n), exp_s), cap


def test_no_points_is_not_an_error(ctx):
    st, pa, pb, cnt, flg, off, rem, sco = raw_call(ctx, np.zeros(1, np.int32), np.zeros(1, np.int32), 3, 0, 0.8, 200, 4, 4)
    assert st == 0 and np.array_equal(off[:4], [0, 0, 0, 0]) and off[4] == GUARD_I64
    assert np.all(pa == GUARD_I32) and np.all(rem == GUARD_I32)


@pytest.mark.parametrize("what", ["k0", "k65", "threshold_nan", "threshold_inf", "threshold_negative", "min_points_negative", "n_negative",
                                  "n_too_large", "cap_negative"])
def test_bad_arguments_leave_every_output_untouched(ctx, what):
    n = 100
    args = dict(k=2, n=n, threshold=0.8, min_points=200, cap=16)
    args.update({"k0": dict(k=0), "k65": dict(k=sc.MAX_ROWS + 1), "threshold_nan": dict(threshold=float("nan")),
                 "threshold_inf": dict(threshold=float("inf")), "threshold_negative": dict(threshold=-0.25),
                 "min_points_negative": dict(min_points=-1), "n_negative": dict(n=-1), "n_too_large": dict(n=2 ** 31 - 1),
                 "cap_negative": dict(cap=-1)}[what])
    preds, gt = np.ones((sc.MAX_ROWS + 1) * n, np.int32), np.zeros(n, np.int32)
    st, pa, pb, cnt, flg, off, rem, sco = raw_call(ctx, preds, gt, args["k"], args["n"], args["threshold"], args["min_points"], args["cap"], 16)
    assert st == -1
    assert np.all(pa == GUARD_I32) and np.all(pb == GUARD_I32) and np.all(cnt == GUARD_I64) and np.all(flg == GUARD_U8)
    assert np.all(off == GUARD_I64) and np.all(rem == GUARD_I32) and np.all(sco == GUARD_I32)


def test_binding_refuses_no_rows_and_too_many(ctx):
    from autoinst_amd import labels_api
    gt = np.zeros(10, np.int32)
    with pytest.raises(ValueError):
        labels_api.label_tables([], gt, ctx=ctx)
    with pytest.raises(ValueError):
        labels_api.label_tables(np.zeros((sc.MAX_ROWS + 1, 10), np.int32), gt, ctx=ctx)
    with pytest.raises(ValueError):
        labels_api.label_tables([np.zeros(9, np.int32)], gt, ctx=ctx)
