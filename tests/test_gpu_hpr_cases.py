"""GPU: `ai_hidden_points` (csrc/ai_hidden.hip) at its kernel limits.  Fixtures: tests/hpr_cases.py, proven on the CPU by
tests/test_hpr_cases.py (which re-solve falls where, and that the statistics tell a wrong skip rule from the shipped one).

Every fixture goes through `camera_api.visible_sets(..., return_stats=True)` from a NumPy array, twice, and from a resident tensor.
The set and the four statistics equal the restatement's (`hpr_ref`); a skipped view is None exactly where `hpr_ref.prepare` says.
"""
import numpy as np
import pytest

import hpr_cases as hc
import hpr_ref

pytestmark = pytest.mark.gpu

EYE = np.eye(4)[None]


def device(points, T, factor, ctx, resident=False):
    """(sets, stats) of `visible_sets` with the sets as NumPy arrays (None for a skipped view) and the stats as lists."""
    import torch
    from autoinst_amd import camera_api
    cloud = torch.as_tensor(np.ascontiguousarray(points), device=torch.device("cuda", ctx.device)) if resident else points
    sets, stats = camera_api.visible_sets(cloud, T, radius_factor=factor, return_stats=True, ctx=ctx)
    out = []
    for s in sets:
        if s is not None and resident:
            assert s.is_cuda and s.dtype == torch.int64
            s = s.cpu().numpy()
        assert s is None or s.dtype == np.int64
        out.append(s)
    return out, [row.tolist() for row in np.asarray(stats)]


def same_set(a, b):
    return (a is None and b is None) or (a is not None and b is not None and np.array_equal(a, b))


def assert_truth(name, got, rows, stats):
    s, st = got
    assert (s is None) == (rows is None), f"{name}: {'skipped' if s is None else 'computed'} against the restatement"
    if rows is None:
        assert st == [0, 0, 0, 0], name
        return
    differ = np.setxor1d(s, rows)
    assert differ.size == 0, f"{name}: {differ.size} flags differ from the restatement, rows {differ[:10].tolist()}"
    assert st == stats, f"{name}: statistics {st} instead of {stats} (local_hidden, resolves, max_resolves, at_camera)"


@pytest.mark.parametrize("name", sorted(hc.cases()))
def test_fixture_equals_the_restatement(name, ctx):
    c = hc.cases()[name]()
    rows, stats = c.truth
    sets, st = device(c.points, EYE, c.factor, ctx)
    assert_truth(name, (sets[0], st[0]), rows, stats)
    again = device(c.points, EYE, c.factor, ctx)
    assert same_set(again[0][0], sets[0]) and again[1] == st, f"{name}: two calls differ"
    res = device(c.points, EYE, c.factor, ctx, resident=True)
    assert same_set(res[0][0], sets[0]) and res[1] == st, f"{name}: a resident tensor gives another answer"


def test_views_on_both_sides_of_the_sphere_limit_in_one_call(ctx):
    """far < 2 R fails for the first and the third view (the cloud a metre farther away) and holds for the second."""
    factor, T, skipped = hc.h6_far_views()
    p = hc.far_cloud()
    sets, st = device(p, T, factor, ctx)
    assert [s is None for s in sets] == skipped
    kept = hc.h6_cases()["h6_far_kept"]
    assert_truth("the view inside the sphere", (sets[1], st[1]), *kept.truth)
    assert st[0] == st[2] == [0, 0, 0, 0]
    for name in ("h6_factor_zero", "h6_factor_negative", "h6_factor_overflows"):     # the factor is the call's: every view is skipped
        c = hc.h6_cases()[name]
        assert device(p, T, c.factor, ctx)[0] == [None, None, None], name
    assert_truth("afterwards", tuple(x[0] for x in device(p, EYE, factor, ctx)), *kept.truth)


def test_views_are_independent_of_their_order(ctx):
    cloud, T = hc.order_views()
    ref = hpr_ref.visible_sets(cloud, T)
    assert [r is None for r in ref] == [False, False, True, False, False]
    alone = [device(cloud, T[v:v + 1], hc.HPR_RADIUS, ctx) for v in range(T.shape[0])]
    for v in range(T.shape[0]):
        assert same_set(alone[v][0][0], ref[v]), f"view {v} alone differs from the restatement"
    for order in (list(range(T.shape[0])), list(range(T.shape[0]))[::-1]):
        for resident in (False, True):
            sets, st = device(cloud, T[order], hc.HPR_RADIUS, ctx, resident=resident)
            for slot, v in enumerate(order):
                assert same_set(sets[slot], alone[v][0][0]) and st[slot] == alone[v][1][0], f"view {v} in slot {slot} (order {order})"
