"""GPU: `ai_nn1_project` and `ai_radius_mean_pool` (ai_points.hip) and the cell list under them (ai_cells.inc) at their limits.
Fixtures, truths and checks: tests/points_cases.py (proven on the CPU by tests/test_points_cases.py).

* 1-NN: index equality and byte-equal distances against brute force (plain square, ties to the smaller index, correctly
  rounded sqrt) on every fixture: the ring-stop cases, the grown grid, block edges, degenerate grids, clamped queries.
* Pooling: equal counts, zero rows where there is no member, and every mean within the DERIVED bound of the ``math.fsum`` mean
  (`points_cases.pool_bound`): ``(cnt - 1) * 2^-53 * sum|f| / cnt`` for the device's sequential float64 sum, plus one rounding
  ``2^-53 * |mean|`` for its division.
* Every fixture goes through the C entry four ways: host memory, host memory with the optional output NULL, device memory on
  torch tensors (what tools/run_map.py does), and host memory again; all byte-identical.
* Errors by return code and `ai_last_error` text; input that is not finite.
"""
import ctypes as C

import numpy as np
import pytest

import points_cases as pc

pytestmark = pytest.mark.gpu

BAD_ARG = -1


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


def nn1_entry(ctx, queries, sources, *, device=False, want_dist=True):
    """`ai_nn1_project` called directly: (status, index, distance or None)."""
    lib, ffi = _lib()
    q = np.ascontiguousarray(queries, dtype=np.float64)
    s = np.ascontiguousarray(sources, dtype=np.float64)
    if device:
        import torch
        tq, ts = _dev(q), _dev(s)
        idx = torch.full((q.shape[0],), -7, dtype=torch.int32, device="cuda:0")
        dist = torch.full((q.shape[0],), -7.0, dtype=torch.float64, device="cuda:0")
        torch.cuda.synchronize()                       # the uploads ran on torch's stream, the library reads on its own
        rc = lib.ai_nn1_project(ctx._h, _ptr(tq), q.shape[0], _ptr(ts), s.shape[0], ffi.AI_MEM_DEVICE, _ptr(idx),
                                _ptr(dist) if want_dist else None)
        return rc, idx.cpu().numpy(), dist.cpu().numpy() if want_dist else None
    idx, dist = np.full(q.shape[0], -7, np.int32), np.full(q.shape[0], -7.0)
    rc = lib.ai_nn1_project(ctx._h, q.ctypes.data, q.shape[0], s.ctypes.data, s.shape[0], ffi.AI_MEM_HOST, idx.ctypes.data,
                            dist.ctypes.data if want_dist else None)
    return rc, idx, dist if want_dist else None


def pool_entry(ctx, queries, sources, feat, radius, *, device=False, want_count=True, dim=None):
    """`ai_radius_mean_pool` called directly: (status, mean, count or None).  ``dim`` overrides the width handed over."""
    lib, ffi = _lib()
    q = np.ascontiguousarray(queries, dtype=np.float64)
    s = np.ascontiguousarray(sources, dtype=np.float64)
    f = np.ascontiguousarray(feat, dtype=np.float32)
    d = f.shape[1] if dim is None else dim
    if device:
        import torch
        tq, ts, tf = _dev(q), _dev(s), _dev(f)
        out = torch.full((q.shape[0], f.shape[1]), -7.0, dtype=torch.float64, device="cuda:0")
        cnt = torch.full((q.shape[0],), -7, dtype=torch.int32, device="cuda:0")
        torch.cuda.synchronize()
        rc = lib.ai_radius_mean_pool(ctx._h, _ptr(tq), q.shape[0], _ptr(ts), s.shape[0], _ptr(tf), d, float(radius), ffi.AI_MEM_DEVICE,
                                     _ptr(out), _ptr(cnt) if want_count else None)
        return rc, out.cpu().numpy(), cnt.cpu().numpy() if want_count else None
    out, cnt = np.full((q.shape[0], f.shape[1]), -7.0), np.full(q.shape[0], -7, np.int32)
    rc = lib.ai_radius_mean_pool(ctx._h, q.ctypes.data, q.shape[0], s.ctypes.data, s.shape[0], f.ctypes.data, d, float(radius),
                                 ffi.AI_MEM_HOST, out.ctypes.data, cnt.ctypes.data if want_count else None)
    return rc, out, cnt if want_count else None


def _same(name, what, a, b):
    assert np.ascontiguousarray(a).tobytes() == np.ascontiguousarray(b).tobytes(), f"{name}: {what} is not byte-identical"


def _run_nn1(ctx, c, truth=None):
    """One fixture through the four calls; the first failure's sentence, or None."""
    try:
        rc, idx, dist = nn1_entry(ctx, c.queries, c.sources)
        assert rc == 0, f"{c.name}: status {rc}: {_last_error()}"
        pc.check_nn1(c.name, idx, dist, c.truth if truth is None else truth)
        rc, idx0, none = nn1_entry(ctx, c.queries, c.sources, want_dist=False)
        assert rc == 0 and none is None
        _same(c.name, "the index with nn_dist NULL", idx0, idx)
        rc, idx_d, dist_d = nn1_entry(ctx, c.queries, c.sources, device=True)
        assert rc == 0, f"{c.name}: device memory: status {rc}: {_last_error()}"
        _same(c.name, "the index from device memory", idx_d, idx)
        _same(c.name, "the distance from device memory", dist_d, dist)
        rc, idx_n, _ = nn1_entry(ctx, c.queries, c.sources, device=True, want_dist=False)
        assert rc == 0
        _same(c.name, "the index from device memory with nn_dist NULL", idx_n, idx)
        rc, idx2, dist2 = nn1_entry(ctx, c.queries, c.sources)
        assert rc == 0
        _same(c.name, "the second run's index", idx2, idx)
        _same(c.name, "the second run's distance", dist2, dist)
    except AssertionError as e:
        return str(e)
    return None


def _run_pool(ctx, c):
    rc, mean, cnt = pool_entry(ctx, c.queries, c.sources, c.feat, c.radius)
    assert rc == 0, f"{c.name}: status {rc}: {_last_error()}"
    pc.check_pool(c.name, mean, cnt, c.truth)
    rc, mean0, none = pool_entry(ctx, c.queries, c.sources, c.feat, c.radius, want_count=False)
    assert rc == 0 and none is None
    _same(c.name, "the mean with count_out NULL", mean0, mean)
    rc, mean_d, cnt_d = pool_entry(ctx, c.queries, c.sources, c.feat, c.radius, device=True)
    assert rc == 0, f"{c.name}: device memory: status {rc}: {_last_error()}"
    _same(c.name, "the mean from device memory", mean_d, mean)
    _same(c.name, "the count from device memory", cnt_d, cnt)
    rc, mean_n, _ = pool_entry(ctx, c.queries, c.sources, c.feat, c.radius, device=True, want_count=False)
    assert rc == 0
    _same(c.name, "the mean from device memory with count_out NULL", mean_n, mean)
    rc, mean2, cnt2 = pool_entry(ctx, c.queries, c.sources, c.feat, c.radius)
    assert rc == 0
    _same(c.name, "the second run's mean", mean2, mean)
    _same(c.name, "the second run's count", cnt2, cnt)


# ------------------------------------------------------------------------------------------------- 1-NN
def test_nn1_ring_stop_cases(ctx):
    """Every case on which the stop rule before the rounding of `pcell_of` was counted answers A; B is nearer."""
    failed = [m for m in (_run_nn1(ctx, c) for c in pc.ring_stop_cases()) if m]
    assert not failed, f"{len(failed)} of {len(pc.ring_stop_cases())} ring-stop cases:\n" + "\n".join(failed)


NN1_FAMILIES = {
    "growth": lambda: [pc.growth_nn1_case()],
    "block_edges": lambda: [pc.nn1_nt_case(n) for n in pc.NN1_NT],
    "degenerate": lambda: [pc.degenerate_nn1_case(k) for k in pc.DEGENERATE],
    "clamped": lambda: [pc.clamp_nn1_case()],
}


@pytest.mark.parametrize("family", sorted(NN1_FAMILIES))
def test_nn1_fixtures(family, ctx):
    failed = [m for m in (_run_nn1(ctx, c) for c in NN1_FAMILIES[family]()) if m]
    assert not failed, "\n".join(failed)


def test_nn1_through_points_api(ctx):
    """`points_api.nn1_index` / `nn1_reproject` on a ring-stop case and the clamped queries: the label of the nearest source."""
    from autoinst_amd import points_api
    for c in (pc.ring_stop_cases()[0], pc.clamp_nn1_case()):
        idx, dist = points_api.nn1_index(c.queries, c.sources, ctx=ctx)
        pc.check_nn1(c.name, idx, dist, c.truth)
        lab = np.arange(c.sources.shape[0] * 2, dtype=np.float64).reshape(-1, 2)
        got = points_api.nn1_reproject(np.zeros((c.queries.shape[0], 2)), c.queries, lab, c.sources, ctx=ctx)
        assert np.array_equal(got, lab[c.truth[0]])


# ------------------------------------------------------------------------------------------------- pooling
POOL_FAMILIES = {
    "widths": lambda: [pc.pool_width_case(d) for d in pc.POOL_WIDTHS],
    "block_edges": lambda: [pc.pool_nq_case(n) for n in pc.POOL_NQ],
    "degenerate": lambda: [pc.degenerate_pool_case(k) for k in pc.DEGENERATE],
    "clamped": lambda: [pc.clamp_pool_case("near"), pc.clamp_pool_case("far")],
    "borders": lambda: [pc.pool_border_case()],
    "crowded": lambda: [pc.pool_crowded_case()],
    "exact_radius": lambda: [pc.pool_exact_radius_case()],
    "growth": lambda: [pc.growth_pool_case()],
}


@pytest.mark.parametrize("family", sorted(POOL_FAMILIES))
def test_pool_fixtures(family, ctx):
    for c in POOL_FAMILIES[family]():
        _run_pool(ctx, c)


def test_pool_through_points_api(ctx):
    from autoinst_amd import points_api
    c = pc.clamp_pool_case("near")
    mean, cnt = points_api.tarl_pool(c.queries, c.sources, c.feat, radius=c.radius, return_count=True, ctx=ctx)
    pc.check_pool(c.name, mean, cnt, c.truth)


# ------------------------------------------------------------------------------------------------- errors
def test_pool_argument_errors(ctx):
    from autoinst_amd import points_api
    c = pc.pool_width_case(16)
    wide = np.zeros((c.sources.shape[0], pc.MAX_DIM + 1), np.float32)
    text = "ai_radius_mean_pool: bad argument"
    for name, kw in pc.POOL_BAD_ARGS.items():
        feat = wide if kw.get("dim", 0) > pc.MAX_DIM else c.feat
        rc, _, _ = pool_entry(ctx, c.queries, c.sources, feat, kw.get("radius", c.radius), dim=kw.get("dim"))
        assert rc == BAD_ARG and text in _last_error(), f"{name}: status {rc}, {_last_error()!r}"
    with pytest.raises(ValueError, match=text):
        points_api.tarl_pool(c.queries, c.sources, wide, ctx=ctx)
    for r in (0.0, -1.0, float("nan")):
        with pytest.raises(ValueError, match=text):
            points_api.tarl_pool(c.queries, c.sources, c.feat, radius=r, ctx=ctx)
    lib, ffi = _lib()
    q, s, f = c.queries, c.sources, c.feat
    out, cnt = np.zeros((q.shape[0], 16)), np.zeros(q.shape[0], np.int32)
    good = [ctx._h, q.ctypes.data, q.shape[0], s.ctypes.data, s.shape[0], f.ctypes.data, 16, c.radius, ffi.AI_MEM_HOST, out.ctypes.data,
            cnt.ctypes.data]
    for pos, bad in ((0, None), (1, None), (2, 0), (2, -1), (2, 1 << 30), (3, None), (4, 0), (4, 1 << 30), (5, None), (9, None)):
        args = list(good)
        args[pos] = bad
        rc = lib.ai_radius_mean_pool(*args)
        assert rc == BAD_ARG and text in _last_error(), f"argument {pos} = {bad}: status {rc}, {_last_error()!r}"
    assert lib.ai_radius_mean_pool(*good) == 0


def test_nn1_argument_errors(ctx):
    lib, ffi = _lib()
    c = pc.nn1_nt_case(pc.BLOCK)
    q, s = c.queries, c.sources
    idx, dist = np.zeros(q.shape[0], np.int32), np.zeros(q.shape[0])
    good = [ctx._h, q.ctypes.data, q.shape[0], s.ctypes.data, s.shape[0], ffi.AI_MEM_HOST, idx.ctypes.data, dist.ctypes.data]
    for pos, bad in ((0, None), (1, None), (2, 0), (2, -1), (2, 1 << 30), (3, None), (4, 0), (4, 1 << 30), (6, None)):
        args = list(good)
        args[pos] = bad
        rc = lib.ai_nn1_project(*args)
        assert rc == BAD_ARG and "ai_nn1_project: bad argument" in _last_error(), f"argument {pos} = {bad}: status {rc}, {_last_error()!r}"
    assert lib.ai_nn1_project(*good) == 0


# ------------------------------------------------------------------------------------------------- input that is not finite
def test_source_that_is_not_finite_is_refused_by_both_entries(ctx):
    from autoinst_amd import points_api
    failed = []
    q = pc.nn1_nt_case(pc.BLOCK).queries[:20]
    for name, s in pc.nonfinite_sources().items():
        feat = np.ones((s.shape[0], 3), np.float32)
        for device in (False, True):
            rc, _, _ = nn1_entry(ctx, q, s, device=device)
            if rc != BAD_ARG or "ai_nn1_project: coordinates are not finite" not in _last_error():
                failed.append(f"{name} (device memory {device}): ai_nn1_project status {rc}")
            rc, _, _ = pool_entry(ctx, q, s, feat, pc.POOL_RADIUS, device=device)
            if rc != BAD_ARG or "ai_radius_mean_pool: coordinates are not finite" not in _last_error():
                failed.append(f"{name} (device memory {device}): ai_radius_mean_pool status {rc}")
    assert not failed, "\n".join(failed)
    s = pc.nonfinite_sources()["source_nan_x"]
    with pytest.raises(ValueError, match="not finite"):
        points_api.nn1_index(q, s, ctx=ctx)
    with pytest.raises(ValueError, match="not finite"):
        points_api.tarl_pool(q, s, np.ones((s.shape[0], 3), np.float32), ctx=ctx)


def test_query_that_is_not_finite_has_no_nearest_source(ctx):
    from autoinst_amd import points_api
    c = pc.nonfinite_query_case()
    truth = pc.nonfinite_query_truth(c)
    bad = c.claims["bad"]
    msg = _run_nn1(ctx, c, truth)                       # index -1 and the NaN's bits on the bad rows, brute force on the others
    assert msg is None, msg
    rc, idx, dist = nn1_entry(ctx, c.queries, c.sources)
    assert rc == 0 and (idx[bad] == -1).all() and np.isnan(dist[bad]).all()
    lab = np.arange(c.sources.shape[0], dtype=np.float64)[:, None]
    with pytest.raises(ValueError, match="NaN or infinite"):
        points_api.nn1_index(c.queries, c.sources, ctx=ctx)
    with pytest.raises(ValueError, match="NaN or infinite"):
        points_api.nn1_reproject(np.zeros((c.queries.shape[0], 1)), c.queries, lab, c.sources, ctx=ctx)
    ok = np.setdiff1d(np.arange(c.queries.shape[0]), bad)
    got = points_api.nn1_reproject(np.zeros((ok.size, 1)), c.queries[ok], lab, c.sources, ctx=ctx)
    assert np.array_equal(got[:, 0], truth[0][ok])
