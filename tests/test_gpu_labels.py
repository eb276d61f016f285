"""GPU: label pairs, chunk merge, duplicate removal and the shared scan at their kernel thresholds (fixtures and exact
references: tests/label_cases.py, proven on the CPU by tests/test_label_cases.py).

Every fixture goes through the public entry point and must EQUAL its reference: integers and bit patterns, no tolerance.
The ``scan_*`` lengths lie on both sides of one tile (2048), of the direct path (8 388 608) and at 20 M (five second-level
tiles); ``merge_tile_*`` walk one, two and three box tiles; ``pairs_distinct_*`` sit on the first-call capacity.  One
fixture of each family runs a second time in the same process and must return the same bytes.

Not run at its real size: the refusal of ``3 * (sel0 + sel1) > KM_MAX_SCALARS`` in `ai_merge_associate` (716 M selected
points); test_label_cases.test_merge_scalar_bound_arithmetic checks the arithmetic of the bound."""
import numpy as np
import pytest

import label_cases as lc
import prep_ref
from oracle import merge_ref

pytestmark = pytest.mark.gpu

T, D = lc.T, lc.D
# run twice, identical bytes: one of each family
REPEAT = {f"scan_{D + 1}_bernoulli_half", f"pairs_distinct_{lc.FIRST_CAP + 1}", f"merge_tile_{2 * lc.BOX_TILE + 88}_40", "merge_face_box",
          "merge_scalar_shared_z", "unique_ends", "merge_iou_many_instances"}


@pytest.fixture(scope="module")
def api(ctx):
    from autoinst_amd import labels_api
    return labels_api


def _same_bytes(a, b):
    return all(np.asarray(x).tobytes() == np.asarray(y).tobytes() for x, y in zip(a, b))


# ------------------------------------------------------------------------------------------------- scan_* and pairs_*
def _run_pairs(api, ctx, c):
    got = api.label_pairs(c.a, c.b, ctx=ctx)
    assert got[0].dtype == np.int32 and got[1].dtype == np.int32 and got[2].dtype == np.int64
    lc.check_label_pairs(c.name, got, lc.ref_label_pairs(c.a, c.b))
    assert int(got[2].sum()) == c.a.shape[0]
    if c.name in REPEAT:
        assert _same_bytes(got, api.label_pairs(c.a, c.b, ctx=ctx)), f"{c.name}: a second run gave other bytes"
    return got


@pytest.mark.parametrize("name", lc.scan_names(big=False))
def test_scan_through_label_pairs_small(api, ctx, name):
    _run_pairs(api, ctx, lc.scan_case(name))


@pytest.mark.parametrize("name", lc.scan_names(big=True))
def test_scan_through_label_pairs_big(api, ctx, name):
    """D - 1 and D: the last lengths of the direct path; D + 1, D + T + 5 and 20 M: the recursive path."""
    c = lc.scan_case(name)
    got = _run_pairs(api, ctx, c)
    assert got[0].shape[0] == int(c.heads.sum(dtype=np.int64))


@pytest.mark.parametrize("name", [c.name for c in lc.pair_cases()])
def test_label_pairs_extremes_and_first_capacity(api, ctx, name):
    c = lc.pair_case(name)
    got = _run_pairs(api, ctx, c)
    assert got[0].shape[0] == c.claims["distinct"]


def test_label_pairs_refuses_bad_input(api, ctx):
    ok = np.zeros(4, np.int64)
    for bad in (np.array([0, 1, 2 ** 31, 3]), np.array([0, -2 ** 31 - 1, 2, 3])):
        with pytest.raises(ValueError):
            api.label_pairs(bad, ok, ctx=ctx)
        with pytest.raises(ValueError):
            api.label_pairs(ok, bad, ctx=ctx)
    with pytest.raises(ValueError):
        api.label_pairs(np.zeros(4, np.int32), np.zeros(5, np.int32), ctx=ctx)
    edge = np.array([-2 ** 31, 2 ** 31 - 1, 0, -2 ** 31], np.int64)                    # the extremes themselves are legal
    lc.check_label_pairs("int64 extremes", api.label_pairs(edge, edge[::-1].copy(), ctx=ctx), lc.ref_label_pairs(edge, edge[::-1]))


_GUARD = 5
_UNTOUCHED = -123456789


def _ffi_label_pairs(ctx, a, b, cap):
    """`ai_label_pairs` itself; the output arrays are _GUARD rows longer than ``cap`` and come back whole."""
    from autoinst_amd import _ffi
    a, b = np.ascontiguousarray(a, np.int32), np.ascontiguousarray(b, np.int32)
    pa, pb = np.full(cap + _GUARD, _UNTOUCHED, np.int32), np.full(cap + _GUARD, _UNTOUCHED, np.int32)
    cnt = np.full(cap + _GUARD, _UNTOUCHED, np.int64)
    total = _ffi.C.c_int64(-1)
    ptr = (lambda x: x.ctypes.data) if cap else (lambda x: None)
    _ffi.check(_ffi.load().ai_label_pairs(ctx._h, a.ctypes.data, b.ctypes.data, a.shape[0], _ffi.AI_MEM_HOST, cap, ptr(pa), ptr(pb), ptr(cnt),
                                          _ffi.C.byref(total)), "ai_label_pairs")
    return pa, pb, cnt, int(total.value)


def test_ffi_label_pairs_cap_zero_fills_only_the_total(ctx):
    c = lc.pair_case(f"pairs_distinct_{lc.FIRST_CAP + 1}")
    pa, pb, cnt, total = _ffi_label_pairs(ctx, c.a, c.b, 0)
    assert total == lc.FIRST_CAP + 1
    assert np.all(pa == _UNTOUCHED) and np.all(pb == _UNTOUCHED) and np.all(cnt == _UNTOUCHED)


@pytest.mark.parametrize("cap", [1, 1000, lc.FIRST_CAP, "total-1", "total", "total+3"])
def test_ffi_label_pairs_partial_capacity(ctx, cap):
    """0 < cap < total: exactly ``cap`` correct leading rows, the count of row cap - 1 (from start[cap]) included;
    cap >= total: every row, the last run closed with n."""
    c = lc.pair_case(f"pairs_distinct_{lc.FIRST_CAP + 1}")
    exp = lc.ref_label_pairs(c.a, c.b)
    n_exp = exp[0].shape[0]
    cap = {"total-1": n_exp - 1, "total": n_exp, "total+3": n_exp + 3}.get(cap, cap)
    pa, pb, cnt, total = _ffi_label_pairs(ctx, c.a, c.b, cap)
    m = min(cap, n_exp)
    assert total == n_exp
    lc.check_label_pairs(f"cap {cap}", (pa[:m], pb[:m], cnt[:m]), tuple(e[:m] for e in exp))
    assert np.all(pa[m:] == _UNTOUCHED) and np.all(pb[m:] == _UNTOUCHED) and np.all(cnt[m:] == _UNTOUCHED), "rows beyond min(cap, total) written"


# ------------------------------------------------------------------------------------------------- merge_associate
def _run_merge(api, ctx, c):
    def run():
        return api.merge_associate(c.map_xyz, c.map_inst, c.chunk_xyz, c.chunk_inst, c.center, c.n1, c.n2, c.side, ctx=ctx)
    got = run()
    lc.check_merge(c.name, got, lc.ref_merge_associate(*c.args()))
    for key in ("inter", "n_points1", "n_scalars1", "n_scalars2", "common"):
        if key in c.claims:
            assert lc.first_difference(got[key], np.asarray(c.claims[key], np.int32)) is None, (c.name, key)
    if c.name in REPEAT:
        again = run()
        assert all(got[k].tobytes() == again[k].tobytes() for k in got), f"{c.name}: a second run gave other bytes"
    return got


@pytest.mark.parametrize("c", lc.merge_small_cases(), ids=lambda c: c.name)
def test_merge_associate_at_its_thresholds(api, ctx, c):
    got = _run_merge(api, ctx, c)
    if c.name == "merge_scalar_shared_z":
        assert got["common"][1:, 1:].min() >= 1


def test_merge_associate_own_scan_crosses_the_direct_path(api, ctx):
    c = lc.merge_scalar_cross_case()
    s0, s1 = lc.selected_counts(c)
    assert 3 * (s0 + s1) > D
    got = _run_merge(api, ctx, c)
    assert int(got["n_points1"].sum()) == s0


# ------------------------------------------------------------------------------------------------- unique_points
@pytest.mark.parametrize("name", sorted(lc.unique_cases()))
def test_unique_points_small(api, ctx, name):
    p = lc.unique_cases()[name]
    keep = api.unique_points(p, ctx=ctx)
    lc.check_unique(name, keep, lc.ref_unique_points(p))
    ep, _ = merge_ref.remove_duplicated_points(p, p)
    lc.check_points(name, p[keep], ep)                                  # by bits: the kept row keeps its own sign of zero
    if name in REPEAT:
        assert keep.tobytes() == api.unique_points(p, ctx=ctx).tobytes()


@pytest.mark.parametrize("n", lc.UNIQUE_BIG_LENGTHS)
def test_unique_points_across_the_direct_path(api, ctx, n):
    p = lc.unique_len_case(n)
    keep = api.unique_points(p, ctx=ctx)
    exp = lc.ref_unique_points(p)
    assert 0 < exp.shape[0] < n
    lc.check_unique(f"unique_len_{n}", keep, exp)


# ------------------------------------------------------------------------------------------------- voxel_scan
def test_voxel_down_sample_above_the_direct_path(ctx):
    from autoinst_amd import prep_api
    p = lc.voxel_scan_points()
    assert p.shape[0] == D + 1
    got, tr = prep_api.voxel_down_sample(p, lc.VOXEL_SIZE, return_trace=True, ctx=ctx)
    ref, rtr = lc.ref_voxel_down_sample_packed(p, lc.VOXEL_SIZE)
    lc.check_points("voxel_scan", got, ref)
    assert lc.first_difference(tr, rtr) is None
    small = p[:30_000]                                                   # the packed reference is prep_ref's on a small cloud
    assert lc.ref_voxel_down_sample_packed(small, lc.VOXEL_SIZE)[0].tobytes() == prep_ref.voxel_down_sample(small, lc.VOXEL_SIZE)[0].tobytes()


# ------------------------------------------------------------------------------------------------- merge_iou_*
@pytest.mark.parametrize("name", sorted(lc.merge_iou_cases()))
def test_merge_iou_rule_end_to_end(api, ctx, name):
    chunks, claims = lc.merge_iou_cases()[name]
    P, C = api.merge_chunks_unite_instances2(chunks, ctx=ctx)
    eP, eC = merge_ref.merge_chunks_unite_instances2(chunks)
    lc.check_points(name, P, eP)
    lc.check_points(name + " colours", C, eC)
    if name == "merge_iou_exactly_0.01":
        assert np.any(np.all(C == claims["color_c"], axis=1)), "a pair with IoU exactly 0.01 was merged"
    if name == "merge_iou_above_0.01":
        assert not np.any(np.all(C == claims["color_c"], axis=1)), "a pair with IoU 1/99 was not merged"
    if name == "merge_iou_tie":
        assert int(np.all(C == claims["color_a"], axis=1).sum()) == 7
    if name in REPEAT:
        P2, C2 = api.merge_chunks_unite_instances2(chunks, ctx=ctx)
        assert P.tobytes() == P2.tobytes() and C.tobytes() == C2.tobytes()
