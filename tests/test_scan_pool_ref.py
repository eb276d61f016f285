"""CPU: the restatement tests/scan_pool_ref.py agrees with an O(N M) brute force, its hand-made cases sit where their names say,
and each deliberately wrong rule is rejected by the case made for it.

Wrong answer -> what catches it (asserted below):

    ignoring the window            window_last (the scan at position `last` is 1 mm from every query), the base fixture
    a non-strict box               box_face (a source exactly on a face)
    <= at the radius               radius_pairs needs no equality; `closed_radius_case`: a pair at exactly fl(r * r)
    a BLAS-order (fused) transform blas_one_ulp (the two transforms put the source on different sides of the radius)
"""
import numpy as np
import pytest

import edge_geometry as eg
import scan_pool_ref as sp


def _counts(res):
    return np.concatenate([r["count"] for r in res])


def test_restatement_equals_brute_force():
    case = sp.base_case(per_scan=300, per_chunk=120, seed=1)
    a, b = sp.pool(case), sp.pool(case, brute=True)
    assert _counts(a).sum() > 50
    for x, y in zip(a, b):
        assert np.array_equal(x["count"], y["count"]) and np.array_equal(x["mean"], y["mean"]) and np.array_equal(x["fmax"], y["fmax"])


def test_base_fixture_discriminates():
    d = sp.discrimination(sp.base_case(per_scan=600, per_chunk=300, seed=1))
    assert all(v > 0 for v in d.values()), d


def test_ignoring_the_window_is_rejected():
    case = sp.case_window_last()
    assert np.array_equal(_counts(sp.pool(case)), case["expect"])
    assert np.array_equal(_counts(sp.pool(case, wrong="ignore_window")), case["expect"] + 1)
    # and the scan at `last` really is the nearest: 1 mm
    w = sp.transform_points(case["scans"][2], case["T"][2])
    assert np.all(np.abs(np.sqrt(eg.sq_plain(w, case["chunks"][0])) - 0.001) < 1e-9)


def test_a_closed_box_is_rejected():
    case = sp.case_box_face()
    w = sp.transform_points(case["scans"][0], case["T"][0])
    assert w[0, 0] == case["boxes"][0][3] and w[2, 1] == case["boxes"][0][1]           # exactly on the faces
    assert np.array_equal(_counts(sp.pool(case)), case["expect"])
    assert np.array_equal(_counts(sp.pool(case, wrong="closed_box")), [1, 1, 1, 1])


def closed_radius_case():
    """A pair whose plain square is exactly fl(radius * radius): dx = radius on an axis where the subtraction is exact."""
    q = np.array([[0.0, 0.0, 0.0]])
    src = q + [sp.RADIUS, 0.0, 0.0]            # at the origin the difference is the radius itself
    d = src[0, 0] - q[0, 0]
    case = sp._case([sp.to_scan_frame(src)], [np.ones((1, 8), np.float32)], [sp.ROT90], [q], [sp._big_box(q, src)], [[0, 1]])
    return case, d


def test_closed_radius_is_rejected():
    case, d = closed_radius_case()
    assert d * d == eg.r2_of(sp.RADIUS)
    assert _counts(sp.pool(case)).tolist() == [0] and _counts(sp.pool(case, wrong="closed_radius")).tolist() == [1]
    # the seeded pairs: each within 4 ulps of the bound, members on both sides; the first 40 are split by plain vs fused
    rp = sp.case_radius_pairs()
    r2 = eg.r2_of(sp.RADIUS)
    assert np.all(np.abs(rp["plain"] - r2) <= 4 * np.spacing(r2))
    member = eg.pool_in(rp["plain"])
    assert 0 < member.sum() < member.size and np.all(member[:40] != eg.pool_in(rp["fused"])[:40])
    assert np.array_equal(sp.transform_points(rp["scans"][0], rp["T"][0]), rp["world"])   # the transform moves nothing by an ulp
    assert np.array_equal(_counts(sp.pool(rp)), member.astype(np.int32))                  # 4 m apart: each query sees its own source


def test_a_fused_transform_is_rejected():
    case = sp.case_blas_one_ulp()
    right, wrong = _counts(sp.pool(case)), _counts(sp.pool(case, wrong="blas_transform"))
    assert np.all(right != wrong) and set(right.tolist()) <= {0, 1} and 0 < right.sum() < right.size


def test_cell_border_case_sits_on_borders():
    case = sp.case_cell_borders()
    w = sp.transform_points(case["scans"][0], case["T"][0])
    for pts in (w, case["chunks"][0]):
        lower = sp.cell_of(np.nextafter(pts, -np.inf))
        upper = sp.cell_of(np.nextafter(pts, np.inf))
        assert np.all((lower != sp.cell_of(pts)) | (upper != sp.cell_of(pts)))             # one ulp away is another cell
        assert sp.cell_of(pts).min() == -4 and sp.cell_of(pts).max() == 3
    res = sp.pool(case)
    assert np.array_equal(res[0]["count"], sp.pool(case, brute=True)[0]["count"]) and res[0]["count"].max() >= 4


@pytest.mark.parametrize("layers", [1, 2])
def test_iz_row_case_would_double_count(layers):
    case = sp.case_iz_rows(layers)
    w = sp.transform_points(case["scans"][0], case["T"][0])
    q = case["chunks"][0]
    cw, cq = sp.cell_of(w), sp.cell_of(q)
    lo, hi = case["boxes"][0][:3], case["boxes"][0][3:]
    assert sp.cell_of(lo[2]) == cq[:, 2].min() == cq[:, 2].max() and sp.cell_of(hi[2]) - sp.cell_of(lo[2]) == layers - 1
    # the top cell of the previous (ix, iy - 1) row holds a member of some query: an aliased run would add it a second time
    member = eg.pool_in(eg.sq_plain(q[:, None], w[None]))
    prev_top = (cw[None, :, 0] == cq[:, None, 0]) & (cw[None, :, 1] == cq[:, None, 1] - 1) & (cw[None, :, 2] == cw[:, 2].max())
    assert np.sum(member & prev_top) > 20
    assert np.array_equal(sp.pool(case)[0]["count"], member.sum(1))


def test_near_origin_radius_pairs_survive_their_transform():
    rp = sp.case_radius_pairs(origin=(25.0, -18.0, 1.0), seed=4, translation=(32.0, 0.0, 1.0))
    assert np.array_equal(sp.transform_points(rp["scans"][0], rp["T"][0]), rp["world"])
    member = eg.pool_in(rp["plain"])
    assert 0 < member.sum() < member.size and np.array_equal(_counts(sp.pool(rp)), member.astype(np.int32))


def test_remaining_hand_made_cases():
    for case in (sp.case_neighbours_only(), sp.case_repeated()):
        assert np.array_equal(_counts(sp.pool(case)), case["expect"])
        assert np.array_equal(_counts(sp.pool(case, brute=True)), case["expect"])
