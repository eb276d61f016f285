"""GPU: `ai_box_select`, `ai_statistical_inliers` and `ai_voxel_down_sample` (ai_prep.hip) at their kernel limits.  Fixtures, models
and truths: tests/prep_cases.py (proven on the CPU by tests/test_prep_cases.py).

* Box select: indices and `box_offsets` equal to NumPy's crop; the ``cap`` protocol; the limits of ``n_boxes``.
* Statistical inliers: ``avg`` equal BIT FOR BIT to the grid-free truth `prep_cases.knn_avg_exact` (the kNN is exact: no
  tolerance, no exclusion set); the kept set equal to ``where((avg > 0) & (avg < threshold))`` formed on the host from the
  device's own outputs; mean, std and threshold within the DERIVED bound of the ``math.fsum`` reference; the kept set equal to the
  reference's on every fixture that tests/test_prep_cases.py proves clear of that bound (all but the two built to sit on the
  threshold, which keep nothing).
* Voxels: means and trace byte-equal to `prep_ref.voxel_down_sample`.
* Every fixture goes through the C entry from host memory, with the optional outputs NULL in turn, from device memory, and
  twice; all byte-identical; and through `prep_api`.
* Input that is not finite is refused by status and text with every output untouched.

The statistics bound (`prep_cases.stats_bound`), with u = 2^-53.  `kq_partial` gives thread t of block b the averages b * 256 + t,
+ 65536, ...: ceil(n / 65536) laps, added one after the other.  `ai_block_sum_first` adds the 64 lanes of a wave in a pairwise tree
(6 steps) and the block's 4 waves one after the other; `kq_finish` sends the 256 block sums through the same tree and waves once
more.  The longest chain of rounded additions from one average to the total is D = laps + 2 * (6 + 4): 21 for n <= 65536, 22 for
the second-lap cloud.  All terms are non-negative, so the total is within D u / (1 - D u) of the exact sum, relatively.
  mean: D u for the sum, u for the division by n, and 2 u for the reference's own two roundings: (D + 3) u |mean| = 24 u |mean|.
  std: the squares are taken around the device's mean, which moves the total by at most 2 dm |sum (v - m)| + P dm^2 (dm = the
  bound above, P = the number of positive averages); each square carries 3 roundings (the difference, twice, and the product), the
  sum D more, the reference's terms 4: (D + 7) u sum (|v - m| + dm)^2; the division by n - 1 and the root add 2 u on either side.
  threshold = mean + std_ratio * std: both bounds, and 2 u on either side for the product and the sum.
For a cloud whose averages spread by more than a thousandth of their mean that is below 1e-14 of the threshold (asserted in
tests/test_prep_cases.py), where tests/test_gpu_prep.py allows 1e-12 against cKDTree.
"""
import ctypes as C

import numpy as np
import pytest

import prep_cases as pc
from autoinst_amd import prep_api

pytestmark = pytest.mark.gpu

BAD_ARG = -1
POISON = -7


def _lib():
    from autoinst_amd import _ffi
    return _ffi.load(), _ffi


def _last_error():
    return _lib()[0].ai_last_error().decode("utf-8", "replace")


def _dev(a):
    import torch
    return torch.from_numpy(np.ascontiguousarray(a)).to("cuda:0")


def _ptr(t):
    return C.c_void_p(t.data_ptr())


def _same(name, what, a, b):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{name}: {what} is not byte-identical"


def _buffers(device, *specs):
    """Poisoned output buffers (shape, dtype) in host or device memory: (arrays, pointers, to_host)."""
    if device:
        import torch
        dt = {np.int32: torch.int32, np.float64: torch.float64}
        arrs = [torch.full(shape, POISON, dtype=dt[d], device="cuda:0") for shape, d in specs]
        torch.cuda.synchronize()                       # the fills ran on torch's stream, the library writes on its own
        return arrs, [_ptr(a) for a in arrs], lambda a: a.cpu().numpy()
    arrs = [np.full(shape, POISON, dtype=d) for shape, d in specs]
    return arrs, [a.ctypes.data for a in arrs], lambda a: a


def _points(points, device):
    p = np.ascontiguousarray(points, dtype=np.float64).reshape(-1, 3)
    if device:
        t = _dev(p)
        import torch
        torch.cuda.synchronize()
        return t, _ptr(t), p.shape[0]
    return p, p.ctypes.data, p.shape[0]


def box_entry(ctx, points, boxes, cap, *, device=False, out_null=False, n_boxes=None):
    """`ai_box_select` called directly: (status, out_index (cap, poisoned), box_offsets (poisoned), n_total)."""
    lib, ffi = _lib()
    hold, pptr, n = _points(points, device)
    b = np.ascontiguousarray(boxes, dtype=np.float64).reshape(-1, 6)
    nb = b.shape[0] if n_boxes is None else n_boxes
    (out,), (optr,), host = _buffers(device, ((max(cap, 1),), np.int32))
    off = np.full(b.shape[0] + 1, POISON, np.int64)
    total = C.c_int64(POISON)
    rc = lib.ai_box_select(ctx._h, pptr, n, b.ctypes.data, nb, ffi.AI_MEM_DEVICE if device else ffi.AI_MEM_HOST, cap,
                           None if out_null else optr, off.ctypes.data, C.byref(total))
    return rc, host(out)[:cap], off, total.value


def inliers_entry(ctx, points, nb, std_ratio, *, device=False, want_avg=True, want_stats=True):
    """`ai_statistical_inliers` called directly: (status, keep_index (n, poisoned), n_keep, avg or None, stats or None)."""
    lib, ffi = _lib()
    hold, pptr, n = _points(points, device)
    (keep, avg), (kptr, aptr), host = _buffers(device, ((max(n, 1),), np.int32), ((max(n, 1),), np.float64))
    stats = np.full(3, float(POISON))
    nk = C.c_int64(POISON)
    rc = lib.ai_statistical_inliers(ctx._h, pptr, n, int(nb), float(std_ratio), ffi.AI_MEM_DEVICE if device else ffi.AI_MEM_HOST, kptr,
                                    C.byref(nk), aptr if want_avg else None, stats.ctypes.data if want_stats else None)
    return rc, host(keep)[:n], nk.value, host(avg)[:n] if want_avg else None, stats if want_stats else None


def voxel_entry(ctx, points, voxel, *, device=False, want_trace=True, nearest=False):
    """`ai_voxel_down_sample` (or `_nearest`) called directly: (status, out (n, 3), n_out, trace or None, nearest index, distance)."""
    lib, ffi = _lib()
    hold, pptr, n = _points(points, device)
    (out, trace, nn, dist), (optr, tptr, nptr, dptr), host = _buffers(
        device, ((max(n, 1), 3), np.float64), ((max(n, 1),), np.int32), ((max(n, 1),), np.int32), ((max(n, 1),), np.float64))
    m = C.c_int64(POISON)
    mem = ffi.AI_MEM_DEVICE if device else ffi.AI_MEM_HOST
    if nearest:
        rc = lib.ai_voxel_down_sample_nearest(ctx._h, pptr, n, float(voxel), mem, optr, C.byref(m), tptr if want_trace else None, nptr, dptr)
    else:
        rc = lib.ai_voxel_down_sample(ctx._h, pptr, n, float(voxel), mem, optr, C.byref(m), tptr if want_trace else None)
    return rc, host(out), m.value, host(trace)[:n] if want_trace else None, host(nn), host(dist)


def _collect(cases, run):
    failed = []
    for c in cases:
        try:
            run(c)
        except AssertionError as e:
            failed.append(str(e).splitlines()[0] if str(e) else repr(e))
    assert not failed, f"{len(failed)} of {len(cases)} fixtures:\n" + "\n".join(failed)


# ------------------------------------------------------------------------------------------------- box select
def _run_box(ctx, c):
    want, woff = c.truth
    total = want.size
    rc, out, off, t = box_entry(ctx, c.points, c.boxes, 0, out_null=True)       # cap 0, no buffer: the total and the offsets
    assert rc == 0, f"{c.name}: status {rc}: {_last_error()}"
    assert t == total, f"{c.name}: n_total {t} instead of {total}"
    _same(c.name, "box_offsets of the sizing call", off, woff)
    if total > 0:
        rc, out, off, t = box_entry(ctx, c.points, c.boxes, total - 1)          # one too small: nothing is written
        assert rc == 0 and t == total, f"{c.name}: cap = total - 1: status {rc}, n_total {t}"
        assert (out == POISON).all(), f"{c.name}: cap = total - 1 wrote to out_index"
    rc, out, off, t = box_entry(ctx, c.points, c.boxes, total)
    assert rc == 0 and t == total, f"{c.name}: status {rc}: {_last_error()}"
    _same(c.name, "out_index", out, want)
    _same(c.name, "box_offsets", off, woff)
    rc, out_d, off_d, t = box_entry(ctx, c.points, c.boxes, total + 3, device=True)
    assert rc == 0 and t == total, f"{c.name}: device memory: status {rc}: {_last_error()}"
    _same(c.name, "out_index from device memory", out_d[:total], want)
    assert (out_d[total:] == POISON).all(), f"{c.name}: device memory: wrote beyond the total"
    _same(c.name, "box_offsets from device memory", off_d, woff)
    rc, out2, off2, _ = box_entry(ctx, c.points, c.boxes, total)
    assert rc == 0
    _same(c.name, "the second run's out_index", out2, out)
    _same(c.name, "the second run's box_offsets", off2, off)


def test_box_select_fixtures(ctx):
    _collect(pc.box_cases(), lambda c: _run_box(ctx, c))


def test_box_select_through_prep_api(ctx):
    for c in pc.box_cases():
        if c.boxes.shape[0] <= 8:
            got = prep_api.box_select(c.points, c.boxes, ctx=ctx)
            for b, g in enumerate(got):
                np.testing.assert_array_equal(g, c.truth[0][c.truth[1][b]:c.truth[1][b + 1]], err_msg=c.name)
            dev = prep_api.box_select(_dev(c.points), c.boxes, ctx=ctx)
            assert all(d.is_cuda for d in dev)
            np.testing.assert_array_equal(np.concatenate([d.cpu().numpy() for d in dev]), c.truth[0], err_msg=c.name)


def test_box_select_limits_of_n_boxes(ctx):
    c = next(x for x in pc.box_cases() if x.name == "box_n257")
    one = np.tile(c.boxes[:1], (pc.MAX_BOXES + 1, 1))
    for nb in (0, pc.MAX_BOXES + 1, -1):
        rc, out, off, t = box_entry(ctx, c.points, one, 16, n_boxes=nb)
        assert rc == BAD_ARG and "ai_box_select" in _last_error(), (nb, rc)
        assert (out == POISON).all() and (off == POISON).all() and t == POISON, f"n_boxes = {nb}: an output was written"
    rc, out, off, t = box_entry(ctx, c.points, one[:pc.MAX_BOXES], 0, out_null=True)
    assert rc == 0 and t == pc.MAX_BOXES * c.truth[1][1]


# ------------------------------------------------------------------------------------------------- statistical inliers
def _check_inliers(c, keep, nk, avg, stats, tag=""):
    name = c.name + tag
    bad = np.flatnonzero(np.ascontiguousarray(avg).view(np.int64) != c.avg.view(np.int64))
    assert bad.size == 0, (f"{name}: {bad.size} averages differ from the exact kNN in their bits, first at point {bad[0]}: "
                           f"{float(avg[bad[0]]).hex()} instead of {float(c.avg[bad[0]]).hex()}")
    print(f"{name}: n={c.n} k={c.k} mean {stats[0]!r} (ref {c.ref['mean']!r}, bound {c.bound['mean']:.3e}) std {stats[1]!r} "
          f"(ref {c.ref['std']!r}, bound {c.bound['std']:.3e}) threshold {stats[2]!r} (ref {c.ref['threshold']!r}, bound "
          f"{c.bound['threshold']:.3e}) kept {nk}")
    own = pc.keep_from(avg, stats[2])
    assert nk == own.size and np.array_equal(keep[:nk], own), f"{name}: the kept set is not where((avg > 0) & (avg < threshold))"
    assert (keep[nk:] == POISON).all(), f"{name}: keep_index was written beyond n_keep"
    if c.n >= 2:
        for i, key in enumerate(("mean", "std", "threshold")):
            assert abs(stats[i] - c.ref[key]) <= c.bound[key], (f"{name}: {key} {stats[i]!r} is {abs(stats[i] - c.ref[key]):.3e} from "
                                                                f"the fsum reference {c.ref[key]!r}, bound {c.bound[key]:.3e}")
    else:
        assert stats[0] == 0.0 and np.isnan(stats[1]) and np.isnan(stats[2]), f"{name}: statistics of one point: {stats}"
    if c.claims.get("on_threshold"):
        assert nk == 0 and stats[1] == 0.0 and stats[0] == c.avg[0] == stats[2], f"{name}: {nk} kept on the threshold, stats {stats}"
    else:
        assert c.near.size == 0
        assert np.array_equal(keep[:nk], c.ref["keep"]), f"{name}: the kept set differs from the reference's"


def _run_inliers(ctx, c):
    rc, keep, nk, avg, stats = inliers_entry(ctx, c.points, c.nb, c.std_ratio)
    assert rc == 0, f"{c.name}: status {rc}: {_last_error()}"
    _check_inliers(c, keep, nk, avg, stats)
    rc, keep_a, nk_a, none, stats_a = inliers_entry(ctx, c.points, c.nb, c.std_ratio, want_avg=False)
    assert rc == 0 and none is None and nk_a == nk
    _same(c.name, "keep_index with avg_out NULL", keep_a, keep)
    _same(c.name, "stats_out with avg_out NULL", stats_a, stats)
    rc, keep_s, nk_s, avg_s, none = inliers_entry(ctx, c.points, c.nb, c.std_ratio, want_stats=False)
    assert rc == 0 and none is None and nk_s == nk
    _same(c.name, "keep_index with stats_out NULL", keep_s, keep)
    _same(c.name, "avg_out with stats_out NULL", avg_s, avg)
    rc, keep_d, nk_d, avg_d, stats_d = inliers_entry(ctx, c.points, c.nb, c.std_ratio, device=True)
    assert rc == 0 and nk_d == nk, f"{c.name}: device memory: status {rc}: {_last_error()}"
    _same(c.name, "keep_index from device memory", keep_d, keep)
    _same(c.name, "avg_out from device memory", avg_d, avg)
    _same(c.name, "stats_out from device memory", stats_d, stats)
    rc, keep_n, nk_n, _, _ = inliers_entry(ctx, c.points, c.nb, c.std_ratio, device=True, want_avg=False, want_stats=False)
    assert rc == 0 and nk_n == nk
    _same(c.name, "keep_index from device memory with both optional outputs NULL", keep_n, keep)
    rc, keep2, nk2, avg2, stats2 = inliers_entry(ctx, c.points, c.nb, c.std_ratio)
    assert rc == 0 and nk2 == nk
    _same(c.name, "the second run's keep_index", keep2, keep)
    _same(c.name, "the second run's avg_out", avg2, avg)
    _same(c.name, "the second run's stats_out", stats2, stats)
    idx, avg_p, st = prep_api.statistical_inlier_indices(c.points, c.nb, c.std_ratio, return_stats=True, ctx=ctx)
    assert idx.dtype == np.int64 and np.array_equal(idx, keep[:nk]), f"{c.name}: prep_api keeps another set"
    _same(c.name, "prep_api's avg", avg_p, avg)
    _same(c.name, "prep_api's statistics", np.array([st["mean"], st["std"], st["threshold"]]), stats)


def _small(c):
    return c.n <= 4096


def test_knn_ring_stop_cases(ctx):
    """Every case on which ``sqrt(kth) <= r * cell`` ends the query's search a ring early: the averages are the exact ones."""
    _collect(pc.ring_stop_cases(), lambda c: _run_inliers(ctx, c))


def test_statistical_inliers_fixtures(ctx):
    ring = {c.name for c in pc.ring_stop_cases()}
    _collect([c for c in pc.knn_cases() if c.name not in ring and _small(c)], lambda c: _run_inliers(ctx, c))


def test_statistical_inliers_second_lap(ctx):
    """RED_BLOCKS * AI_BLOCK + 1 points: the last one is the second term of thread 0 of block 0 in `kq_partial`."""
    (c,) = [x for x in pc.knn_cases() if not _small(x)]
    assert c.n == pc.LAP + 1
    rc, keep, nk, avg, stats = inliers_entry(ctx, c.points, c.nb, c.std_ratio)
    assert rc == 0, f"{c.name}: status {rc}: {_last_error()}"
    _check_inliers(c, keep, nk, avg, stats)
    rc, keep_d, nk_d, avg_d, stats_d = inliers_entry(ctx, c.points, c.nb, c.std_ratio, device=True)
    assert rc == 0 and nk_d == nk
    _same(c.name, "keep_index from device memory", keep_d, keep)
    _same(c.name, "avg_out from device memory", avg_d, avg)
    _same(c.name, "stats_out from device memory", stats_d, stats)
    dropped = c.avg.copy()
    dropped[-1] = 0.0                                   # a reduction that forgot the second lap would report this mean
    assert abs(pc.stats_ref(dropped, c.std_ratio)["mean"] - c.ref["mean"]) > 100 * c.bound["mean"]


def test_statistical_inliers_largest_k(ctx):
    rng = np.random.default_rng(65)
    p = rng.uniform(-1.0, 1.0, (pc.MAX_K + 1, 3))
    rc, keep, nk, avg, stats = inliers_entry(ctx, p, pc.MAX_K + 1, 2.0)             # k = 65 = n: no instance serves it
    assert rc == BAD_ARG and "nb_neighbors > 64 is not supported" in _last_error()
    assert (keep == POISON).all() and nk == POISON and (avg == POISON).all() and (stats == POISON).all()
    with pytest.raises(ValueError):
        prep_api.statistical_inlier_indices(p, pc.MAX_K + 1, 2.0, ctx=ctx)
    c = pc.KnnCase("k65_n64", p[:pc.MAX_K], pc.MAX_K + 1)                            # the same nb_neighbors, k = n = 64: served
    rc, keep, nk, avg, stats = inliers_entry(ctx, c.points, c.nb, c.std_ratio)
    assert rc == 0, _last_error()
    _check_inliers(c, keep, nk, avg, stats)


# ------------------------------------------------------------------------------------------------- voxels
def _run_voxel(ctx, c):
    if "refused" in c.claims:
        for nearest in (False, True):
            rc, out, m, trace, nn, dist = voxel_entry(ctx, c.points, c.voxel, nearest=nearest)
            assert rc == BAD_ARG and c.claims["refused"] in _last_error(), f"{c.name}: status {rc}: {_last_error()}"
            assert (out == POISON).all() and (trace == POISON).all() and (nn == POISON).all() and (dist == POISON).all(), \
                f"{c.name}: a refused call wrote an output"
        with pytest.raises(ValueError, match=c.claims["refused"]):
            prep_api.voxel_down_sample(c.points, c.voxel, ctx=ctx)
        return
    want, wtrace = c.truth
    rc, out, m, trace, _, _ = voxel_entry(ctx, c.points, c.voxel)
    assert rc == 0, f"{c.name}: status {rc}: {_last_error()}"
    assert m == want.shape[0], f"{c.name}: {m} voxels instead of {want.shape[0]}"
    _same(c.name, "the means", out[:m], want)
    _same(c.name, "the trace", trace, wtrace)
    assert (out[m:] == POISON).all(), f"{c.name}: out_xyz was written beyond n_out"
    rc, out0, m0, none, _, _ = voxel_entry(ctx, c.points, c.voxel, want_trace=False)
    assert rc == 0 and none is None and m0 == m
    _same(c.name, "the means with trace NULL", out0, out)
    rc, out_d, m_d, trace_d, _, _ = voxel_entry(ctx, c.points, c.voxel, device=True)
    assert rc == 0 and m_d == m, f"{c.name}: device memory: status {rc}: {_last_error()}"
    _same(c.name, "the means from device memory", out_d, out)
    _same(c.name, "the trace from device memory", trace_d, trace)
    rc, out_n, m_n, trace_n, nn, dist = voxel_entry(ctx, c.points, c.voxel, nearest=True)
    assert rc == 0 and m_n == m
    _same(c.name, "the means of ai_voxel_down_sample_nearest", out_n, out)
    _same(c.name, "the trace of ai_voxel_down_sample_nearest", trace_n, trace)
    rc, out2, m2, trace2, _, _ = voxel_entry(ctx, c.points, c.voxel)
    assert rc == 0 and m2 == m
    _same(c.name, "the second run's means", out2, out)
    _same(c.name, "the second run's trace", trace2, trace)
    got, tr = prep_api.voxel_down_sample(c.points, c.voxel, return_trace=True, ctx=ctx)
    _same(c.name, "prep_api's means", got, want)
    _same(c.name, "prep_api's trace", tr, wtrace)


def test_voxel_down_sample_fixtures(ctx):
    _collect(pc.voxel_cases(), lambda c: _run_voxel(ctx, c))


# ------------------------------------------------------------------------------------------------- input that is not finite
def _refused(ctx, name, p):
    for device in (False, True):
        where = f"{name}, {'device' if device else 'host'} memory"
        rc, keep, nk, avg, stats = inliers_entry(ctx, p, 20, 2.0, device=device)
        assert rc == BAD_ARG and "ai_statistical_inliers: coordinates are not finite" in _last_error(), f"{where}: status {rc}: {_last_error()}"
        assert (keep == POISON).all() and (avg == POISON).all() and (stats == POISON).all(), f"{where}: ai_statistical_inliers wrote an output"
        for nearest, entry in ((False, "ai_voxel_down_sample"), (True, "ai_voxel_down_sample_nearest")):
            rc, out, m, trace, nn, dist = voxel_entry(ctx, p, 0.35, device=device, nearest=nearest)
            assert rc == BAD_ARG and f"{entry}: coordinates are not finite" in _last_error(), f"{where}: {entry}: status {rc}: {_last_error()}"
            assert (out == POISON).all() and (trace == POISON).all() and (nn == POISON).all() and (dist == POISON).all(), \
                f"{where}: {entry} wrote an output"
    for call in (lambda: prep_api.statistical_inlier_indices(p, 20, 2.0, ctx=ctx), lambda: prep_api.voxel_down_sample(p, 0.35, ctx=ctx),
                 lambda: prep_api.voxel_down_sample_nearest(p, 0.35, ctx=ctx)):
        with pytest.raises(ValueError, match="coordinates are not finite"):
            call()


def test_nan_coordinate_is_refused(ctx):
    """One NaN among 300 finite points, on each axis: fmin / fmax would drop it from the bounds."""
    clouds = [(name, p) for name, p in pc.nonfinite_clouds() if name.startswith("nan")]
    assert len(clouds) == 3
    _collect(clouds, lambda c: _refused(ctx, *c))


def test_infinite_coordinate_is_refused(ctx):
    clouds = [(name, p) for name, p in pc.nonfinite_clouds() if not name.startswith("nan")]
    assert len(clouds) == 6
    _collect(clouds, lambda c: _refused(ctx, *c))
