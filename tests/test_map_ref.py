"""CPU: the restatement tests/map_ref.py agrees with an O(n m) brute force, rejects a list of deliberately wrong answers, and
its hand-made edge cases sit where their names say.

Wrong answer -> what catches it (asserted below):

    nearest member of the OWN voxel           the street (voxels whose nearest raw point is a neighbour's), neighbour_one_ulp_nearer,
                                              diagonal_neighbours_only
    first member of the voxel                 the street, tie_neighbour_first
    ties to the LARGER index                  the street's repeated points, tie_own_first, tie_neighbour_first
    dx*dx + (dy*dy + dz*dz)                   `association_case`: two pairs of points one ulp apart whose order that sum swaps
"""
import numpy as np
import pytest

import map_ref
import prep_ref
from autoinst_amd import synth


@pytest.fixture(scope="module")
def small():
    """A raw-density street short enough for the brute force: both clouds, <= 20 k points each."""
    m = synth.street_map(2.0, seed=3, step=0.02, width=2.0, facade_height=1.0, n_objects=0)
    assert 5_000 < m["ground"].shape[0] <= 20_000 and 5_000 < m["nonground"].shape[0] <= 20_000
    return m


def _members(trace, m):
    order = np.argsort(trace, kind="stable")
    start = np.searchsorted(trace[order], np.arange(m + 1))
    return order, start


def wrong_own_voxel(points, voxel):
    """Nearest member of the voxel itself."""
    out, trace = prep_ref.voxel_down_sample(points, voxel)
    order, start = _members(trace, out.shape[0])
    idx = np.empty(out.shape[0], np.int64)
    for v in range(out.shape[0]):
        mem = order[start[v]:start[v + 1]]
        idx[v] = mem[np.argmin(map_ref.sq_dist(out[v], points[mem]))]
    return idx


def wrong_first_member(points, voxel):
    out, trace = prep_ref.voxel_down_sample(points, voxel)
    order, start = _members(trace, out.shape[0])
    return order[start[:-1]]


def wrong_larger_index(points, voxel):
    out, _ = prep_ref.voxel_down_sample(points, voxel)
    n = points.shape[0]
    return np.concatenate([n - 1 - np.argmin(map_ref.sq_dist(out[s:s + 256, None, :], points[None, ::-1, :]), axis=1)
                           for s in range(0, out.shape[0], 256)])


def wrong_association(points, voxel):
    out, _ = prep_ref.voxel_down_sample(points, voxel)
    d = out[:, None, :] - points[None, :, :]
    return np.argmin(d[..., 0] * d[..., 0] + (d[..., 1] * d[..., 1] + d[..., 2] * d[..., 2]), axis=1)


def _rejected(name, points, voxel, wrong_idx):
    exp = map_ref.voxel_down_sample_nearest(points, voxel, brute=True)
    with pytest.raises(AssertionError):
        map_ref.check_nearest(name, (exp[0], wrong_idx, None, None), exp)


@pytest.mark.parametrize("cloud", ["ground", "nonground"])
def test_restatement_equals_brute_force(small, cloud):
    p = small[cloud]
    a = map_ref.voxel_down_sample_nearest(p, 0.05)
    b = map_ref.voxel_down_sample_nearest(p, 0.05, brute=True)
    map_ref.check_nearest(cloud, a, b)
    own = a[2][a[1]] == np.arange(a[0].shape[0])
    d2 = map_ref.nearest_raw_brute(a[0], p)[1]
    ties = np.concatenate([(map_ref.sq_dist(a[0][s:s + 256, None, :], p[None, :, :]) == d2[s:s + 256, None]).sum(1)
                           for s in range(0, d2.size, 256)])
    print(f"{cloud}: n={p.shape[0]} voxels={a[0].shape[0]} nearest in another voxel: {int((~own).sum())} tied: {int((ties > 1).sum())}")
    assert (~own).sum() > 0 and (ties > 1).sum() > 0           # the small street discriminates too
    for k in (1, 2, 50):                                        # the ball-query branch: every k-th neighbour is a candidate
        i2, e2 = map_ref.nearest_raw(a[0], p, k=k)
        assert np.array_equal(i2, b[1]) and np.array_equal(e2, d2)


def test_wrong_answers_are_rejected_on_the_street(small):
    p = small["ground"]
    for wrong in (wrong_own_voxel, wrong_first_member, wrong_larger_index):
        _rejected(wrong.__name__, p, 0.05, wrong(p, 0.05))
    exp = map_ref.voxel_down_sample_nearest(p, 0.05, brute=True)
    map_ref.check_nearest("right", (exp[0], exp[1].copy(), exp[2], exp[3].copy()), exp)
    for field, bad in ((0, np.nextafter(exp[0], np.inf)), (3, np.nextafter(exp[3], np.inf)), (2, exp[2][::-1])):
        got = list(exp)
        got[field] = bad
        with pytest.raises(AssertionError):
            map_ref.check_nearest("mutated", tuple(got), exp)
    with pytest.raises(AssertionError):
        map_ref.check_nearest("int32", (exp[0], exp[1].astype(np.int32), None, None), exp)


def association_case():
    """Two point pairs, C +- (a, b, c) and C +- (c, b, a), in one voxel whose mean is exactly C: under the rule their squares are
    (a2 + b2) + c2 and (c2 + b2) + a2, one ulp apart; a2 + (b2 + c2) gives the same two numbers the other way round."""
    rng = np.random.default_rng(11)
    C = np.array([2.0, 2.0, 2.0])
    while True:
        o = np.round(rng.uniform(0.05, 0.45, 3) * 2.0 ** 49) * 2.0 ** -49
        a2, b2, c2 = o * o
        if (a2 + b2) + c2 != (c2 + b2) + a2:
            break
    p = np.array([[0.0, 0.0, 0.0], C + o, C - o, C + o[::-1], C - o[::-1]])
    return p, ((a2 + b2) + c2, (c2 + b2) + a2)


def test_association_order_is_pinned():
    p, (d_first, d_second) = association_case()
    out, idx, trace, dist = map_ref.voxel_down_sample_nearest(p, 1.0, brute=True)
    v = trace[1]
    assert np.all(trace[1:] == v) and np.array_equal(out[v], [2.0, 2.0, 2.0])     # the mean is exact
    assert np.nextafter(min(d_first, d_second), np.inf) == max(d_first, d_second)  # one ulp
    assert idx[v] == (1 if d_first < d_second else 3) and dist[v] == np.sqrt(min(d_first, d_second))
    w = wrong_association(p, 1.0)
    assert w[v] == (3 if d_first < d_second else 1)
    _rejected("association", p, 1.0, w)
    map_ref.check_nearest("kd-tree path", map_ref.voxel_down_sample_nearest(p, 1.0), (out, idx, trace, dist))


def test_edge_cases_sit_where_their_names_say():
    cases = map_ref.edge_cases()
    for name, c in cases.items():
        p, voxel, claims = c["points"], c["voxel"], c["claims"]
        out, idx, trace, dist = map_ref.voxel_down_sample_nearest(p, voxel, brute=True)
        map_ref.check_nearest(name, map_ref.voxel_down_sample_nearest(p, voxel), (out, idx, trace, dist))
        if "expect_all" in claims:
            assert idx.tolist() == claims["expect_all"], name
        if "member" not in claims:
            continue
        v = trace[claims["member"]]
        if "expect" in claims:
            assert idx[v] == claims["expect"], name
        if "ulps" in claims:                                    # own members vs the neighbour-voxel point, in ulps of the square
            members = np.where(trace == v)[0]
            other = [i for i in range(1, p.shape[0]) if trace[i] != v]
            assert len(other) == 1 and trace[other[0]] != v, name
            d_own = map_ref.sq_dist(out[v], p[members]).min()
            d_nb = map_ref.sq_dist(out[v], p[other[0]])
            steps = {-1: np.nextafter(d_own, 0.0), 0: d_own, 1: np.nextafter(d_own, np.inf)}
            assert d_nb == steps[claims["ulps"]], (name, d_own, d_nb)
            if claims["ulps"] == 0:                              # labels differ across the tie, and the order decides
                assert idx[v] == min(members.min(), other[0]), name
    # what each wrong answer gets wrong on them
    for name, wrong in (("neighbour_one_ulp_nearer", wrong_own_voxel), ("diagonal_neighbours_only", wrong_own_voxel),
                        ("tie_neighbour_first", wrong_first_member), ("tie_own_first", wrong_larger_index),
                        ("tie_neighbour_first", wrong_larger_index), ("lattice_on_borders", wrong_larger_index)):
        c = cases[name]
        _rejected(name, c["points"], c["voxel"], wrong(c["points"], c["voxel"]))
    c = cases["point_on_a_face"]
    _, _, trace, _ = map_ref.voxel_down_sample_nearest(c["points"], 1.0, brute=True)
    assert trace[1] == trace[2] != trace[3]                      # x = 1.5 belongs to the voxel above the face
    lat = cases["lattice_on_borders"]["points"][1:]
    assert np.all((lat[:, 0] + 0.5) % 1.0 == 0.0)
    d = cases["diagonal_neighbours_only"]
    vox = np.floor(d["points"] + 0.5).astype(int)
    rel = np.abs(vox[4:] - vox[1])
    assert np.all(vox[1:4] == vox[1]) and np.all(rel == 1) and len({tuple(r) for r in (vox[4:] - vox[1])}) == 8
