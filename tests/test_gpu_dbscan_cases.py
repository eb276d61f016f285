"""GPU: `ai_dbscan` (csrc/ai_dbscan.hip) at its kernel limits.  Fixtures and truth: tests/dbscan_cases.py, proven on the CPU by
tests/test_dbscan_cases.py (which also shows which fixture fails for which wrong search).

Every fixture goes through `cluster_api.dbscan(..., return_counts=True, return_sizes=True)` from NumPy arrays, twice (the union
is a race by design: two runs must agree), and from resident tensors.  Labels, cluster counts, saturated neighbour counts and
sizes equal the truth of every cloud alone.  The pairs at a cell border are compared at eps and one step of the doubles below
it.  What the entry refuses is refused with its outputs unwritten, and the context computes afterwards.
"""
import ctypes as C

import numpy as np
import pytest

import dbscan_cases as dc

pytestmark = pytest.mark.gpu


def device(clouds, eps, ms, ctx, resident=False):
    """Per cloud (labels, n_clusters, counts, sizes) as NumPy arrays: one cloud as an array, several as a list."""
    import torch
    from autoinst_amd import cluster_api
    dev = torch.device("cuda", ctx.device)
    arg = [torch.as_tensor(np.ascontiguousarray(c), device=dev) if resident else c for c in clouds]
    many = len(arg) > 1
    lab, k, counts, sizes = cluster_api.dbscan(arg if many else arg[0], eps, ms, return_counts=True, return_sizes=True, ctx=ctx)
    if not many:
        lab, k, counts, sizes = [lab], [k], [counts], [sizes]
    out = []
    for i in range(len(arg)):
        if resident:
            assert all(x[i].is_cuda and x[i].dtype == torch.int32 for x in (lab, counts, sizes))
        host = [x[i].cpu().numpy() if resident else x[i] for x in (lab, counts, sizes)]
        assert all(h.dtype == np.int32 for h in host)
        out.append((host[0], int(k[i]), host[1], host[2]))
    return out


def assert_truth(name, got, truth):
    assert len(got) == len(truth)
    for i, (g, w) in enumerate(zip(got, truth)):
        if dc.same(g, w):
            continue
        what = [f for f, a, b in zip(("labels", "n_clusters", "counts", "sizes"), g, w) if not np.array_equal(a, b)]
        bad = np.flatnonzero(g[0] != w[0]) if g[0].shape == w[0].shape else []
        raise AssertionError(f"{name}: cloud {i} differs from the truth in {what}: {g[1]} clusters instead of {w[1]}, {len(bad)} labels, "
                             f"first at {bad[:1]}: {g[0][bad[:1]]} instead of {w[0][bad[:1]]}")


def assert_equal_runs(name, a, b, what):
    assert all(dc.same(x, y) for x, y in zip(a, b)), f"{name}: {what}"


@pytest.mark.parametrize("name", sorted(dc.cases()))
def test_fixture_equals_the_truth(name, ctx):
    c = dc.cases()[name]()
    runs = [(c.eps, c.truth)] + ([(float(np.nextafter(c.eps, 0)), c.truth_below)] if c.below else [])
    for eps, truth in runs:
        host = device(c.clouds, eps, c.ms, ctx)
        assert_truth(f"{name} at eps {eps!r}", host, truth)
        assert_equal_runs(name, device(c.clouds, eps, c.ms, ctx), host, "two calls differ")
        assert_equal_runs(name, device(c.clouds, eps, c.ms, ctx, resident=True), host, "resident tensors give another answer")


def test_clouds_in_reversed_order(ctx):
    c = dc.clouds_300_case()
    got = device(c.clouds[::-1], c.eps, c.ms, ctx)
    assert_truth("clouds_300 reversed", got, c.truth[::-1])
    assert got[0][0].shape == (0,) and got[-1][0].shape == (0,)


def _entry(ctx, xyz, off, eps, ms):
    """`ai_dbscan` itself on outputs filled beforehand: (return code, message, outputs)."""
    from autoinst_amd import _ffi
    lib = _ffi.load()
    xyz, off = np.ascontiguousarray(xyz, dtype=np.float64), np.asarray(off, dtype=np.int64)
    n = xyz.shape[0]
    lab, cnt, siz, found = (np.full(m, -7, np.int32) for m in (n, n, n, off.shape[0] - 1))
    code = lib.ai_dbscan(ctx._h, xyz.ctypes.data, off.ctypes.data, off.shape[0] - 1, C.c_double(eps), ms, _ffi.AI_MEM_HOST, lab.ctypes.data,
                         found.ctypes.data, cnt.ctypes.data, siz.ctypes.data)
    return code, lib.ai_last_error().decode("utf-8", "replace"), (lab, cnt, siz, found)


def _valid_call_computes(ctx):
    c = dc.last_cell_wide_case()
    assert_truth("after a refusal", device(c.clouds, c.eps, c.ms, ctx), c.truth)


def test_too_many_points_are_refused_before_anything_is_read(ctx):
    """off = [0, 2^30] over a 4-point array: the entry returns on the count alone."""
    p = np.random.default_rng(0).normal(0.0, 1.0, (4, 3))
    code, msg, outs = _entry(ctx, p, [0, dc.K["N_LIMIT"]], 0.5, 2)
    assert code == -1 and "2^30" in msg
    assert all((o == -7).all() for o in outs)
    _valid_call_computes(ctx)


@pytest.mark.parametrize("eps", dc.REFUSED_EPS)
def test_eps_whose_square_is_not_a_positive_number_is_refused(eps, ctx):
    from autoinst_amd import cluster_api
    p = np.random.default_rng(1).normal(0.0, 1.0, (50, 3))
    with pytest.raises(ValueError, match=r"eps \* eps"):
        cluster_api.dbscan(p, eps, 3, ctx=ctx)
    code, msg, outs = _entry(ctx, p, [0, 20, 50], eps, 3)
    assert code == -1 and "eps * eps" in msg and all((o == -7).all() for o in outs)
    _valid_call_computes(ctx)


def test_an_extent_at_the_limit_is_refused(ctx):
    from autoinst_amd import cluster_api
    p = dc.refused_extent_cloud()
    with pytest.raises(ValueError, match="not finite"):
        cluster_api.dbscan(p, 0.5, 3, ctx=ctx)
    code, msg, outs = _entry(ctx, p, [0, 50], 0.5, 3)
    assert code == -1 and "not finite" in msg and all((o == -7).all() for o in outs)
    _valid_call_computes(ctx)
