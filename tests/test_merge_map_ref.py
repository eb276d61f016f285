"""The NumPy restatement of ``ai_merge_map``'s rules (``tests/merge_map_ref.py``) against the line-by-line restatement of the
reference's merge (``oracle/merge_ref.py``).  No GPU.

M11: colour global id g as (g, 0, 0), black for 0.  np.unique(colours, axis=0) then orders instances by id, "the same colour" is
"the same id", and the colour-identified reference must give the id-identified merge's points bit for bit and colour(out_inst).

Centres: the reference computes np.mean of the new chunk itself (:397-403).  The restatement is handed exactly those values as
explicit centres, so both crop with the same cube and the comparison does not depend on how a mean is summed; M4's own sum is
checked separately (it differs from np.mean by rounding only, and no point of these maps lies within 1e-6 of a cube face, which
is asserted, so even that difference could not move a point across a face).
"""
import numpy as np
import pytest

import merge_map_cases as mc
import merge_map_ref as ref

N_RANDOM = 300


def _equal_to_oracle(points, instances, res):
    p, g = mc.oracle(points, instances)
    return (p.shape == res["points"].shape and p.tobytes() == np.ascontiguousarray(res["points"]).tobytes()
            and np.array_equal(g, res["inst"]))


def test_m11_random_maps_equal_the_reference():
    seen = dict(chunks=set(), street=0, dup=0, relabelled=0, dropped=0)
    for k, (points, instances) in enumerate(mc.random_maps(N_RANDOM)):
        centers = mc.mean_centers(points)
        assert mc.face_distance(points, centers) > 1e-6, k
        res = ref.merge_map(points, instances, centers=centers)
        assert _equal_to_oracle(points, instances, res), k
        # the source is what carries any per-point value into the merged order
        assert np.array_equal(np.concatenate(points)[res["src"]].tobytes(), res["points"].tobytes())
        seen["chunks"].add(len(points))
        seen["street"] += any(not i.any() for i in instances)
        seen["dup"] += any(np.unique(p, axis=0).shape[0] < p.shape[0] for p in points)
        seen["relabelled"] += int(res["stats"][:, 3].sum() > 0)
        seen["dropped"] += int(res["src"].size < sum(p.shape[0] for p in points))
    assert seen["chunks"] == {1, 2, 3, 4, 5}
    assert min(seen["street"], seen["dup"], seen["relabelled"], seen["dropped"]) >= 20, seen


def test_m11_with_the_restatements_own_centres():
    """Without explicit centres the restatement sums in M4's order; np.mean differs by rounding only, far less than the distance
    of any point to a face, so the result is still the reference's."""
    for k, (points, instances) in enumerate(mc.random_maps(40, seed=5)):
        assert mc.face_distance(points, mc.mean_centers(points)) > 1e-6, k
        assert _equal_to_oracle(points, instances, ref.merge_map(points, instances)), k


@pytest.mark.parametrize("n", [1, 2, 255, 256, 257, 1025, ref.SLOTS + 3])
def test_m4_sum_is_a_float64_sum(n):
    x = np.random.default_rng(n).normal(100.0, 30.0, n)
    got = ref.f4_sum(x) / n
    assert abs(got - np.mean(x)) <= n * 2.0 ** -52 * np.abs(x).max()
    assert ref.f4_sum(np.full(n, 0.5)) == 0.5 * n                     # exact sums stay exact in any order


@pytest.mark.parametrize("name", sorted(mc.hand_cases()))
def test_hand_made_case(name):
    case = mc.hand_cases()[name]
    res = ref.merge_map(case["points"], case["instances"], centers=case["centers"])
    assert res["inst"].tolist() == list(case["inst"])
    assert res["src"].tolist() == list(case["src"])
    assert res["points"].tobytes() == np.concatenate(case["points"])[case["src"]].tobytes()
    assert _equal_to_oracle(case["points"], case["instances"], res)      # the reference's own lines give the same


def test_hand_made_ious_are_the_stated_doubles():
    assert 1.0 / 50.0 == 2.0 / 100.0 and 1.0 / 100.0 == 0.01 and not (1.0 / 100.0 > 0.01)
    cases = mc.hand_cases()
    tie = cases["iou_tie_keeps_smaller_id"]
    res = ref.merge_map(tie["points"], tie["instances"], centers=tie["centers"])
    assert res["stats"][1].tolist() == [len(tie["points"][0]), 2, 2, 1]   # every map point cropped, 2 instances, 2 pairs, 1 id
    edge = cases["iou_exactly_iou_min"]
    assert ref.merge_map(edge["points"], edge["instances"], centers=edge["centers"])["stats"][1].tolist()[1:] == [1, 0, 0]


@pytest.mark.parametrize("variant", ref.VARIANTS)
def test_wrong_rule_is_told_apart(variant):
    """Each plausible wrong rule differs from the reference on at least one hand-made case."""
    differs = []
    for name, case in mc.hand_cases().items():
        res = ref.merge_map(case["points"], case["instances"], centers=case["centers"], variant=variant)
        if not _equal_to_oracle(case["points"], case["instances"], res):
            differs.append(name)
    assert differs, variant


def test_errors_of_m10():
    p, i = [np.zeros((2, 3))], [np.array([1, 1])]
    for bad_p, bad_i, kw, text in (
            ([np.array([[0.0, np.nan, 0.0]])], [np.array([1])], {}, "not finite"),
            (p, [np.array([1, -1])], {}, "negative"),
            (p, i, dict(centers=[[0.0, np.inf, 0.0]]), "centre"),
            (p, i, dict(side_length=0.0), "side_length"),
            (p, i, dict(iou_min=float("nan")), "iou_min")):
        with pytest.raises(ValueError, match=text):
            ref.merge_map(bad_p, bad_i, **kw)
    empty = ref.merge_map([], [])
    assert empty["points"].shape == (0, 3) and empty["src"].size == 0
