"""CPU checks of tests/affinity_cases.py: the host model of the build's row order and tile plan, the fixtures' claims
(every threshold of the kernels hit on both sides, for the 16-row and the 32-row plan), the longdouble reference
against the dense oracle, and the teeth of `check_affinity` (the function tests/test_gpu_affinity.py calls)."""
import numpy as np
import pytest
import scipy.sparse as sp
from scipy.spatial.distance import cdist

import affinity_cases as ac
from oracle import ncuts_ref

# every row of the thresholds table, for both tile plans where the threshold belongs to a plan
REQUIRED = [("stash", s, None) for s in ("below", "at", "above", "none_over")] + \
    [(w, s, r) for r in (16, 32) for w in ("tile_entries", "distinct") for s in ("at", "above")] + \
    [("longest", L, r) for r in (16, 32) for L in (63, 64, 65, 128, 129)] + \
    [("mirror", "staged_vs_fallback", r) for r in (16, 32)] + \
    [("tail", n, None) for n in (1, 2, 15, 16, 17, 31, 32, 33, 1025, 1023)] + \
    [("walk", g, None) for g in ((1, 1), (3, 1), (3, 3))] + [("grid", "nx1", None), ("grid", "negative", None)] + \
    [("translated", "walk_3d", None)] + [("width", w, None) for w in ac.WIDTHS] + \
    [("weight0", "theta", None), ("weight0", "alpha", None), ("sam", 1, None), ("sam", 2, None),
     ("underflow", "subnormal_and_zero", None), ("radius", "exact", None), ("ordinary", "three_regimes", None)]


# --------------------------------------------------------------------------------------------- the plan model
@pytest.mark.parametrize("seed,n,scale", [(0, 1, 1.0), (1, 40, 0.7), (2, 300, 1.5), (3, 500, 0.6), (4, 257, 4.0)])
def test_plan_matches_brute_force(seed, n, scale):
    rng = np.random.default_rng(seed)
    p = rng.normal(0, scale, (n, 3)) + rng.uniform(-50, 50, 3)
    p[n // 2:] = np.round(p[n // 2:] * 4) / 4          # shared cells, duplicate points, pairs on cell faces
    d = p[:, None, :] - p[None, :, :]
    sq = d * d
    adj = np.sqrt((sq[..., 0] + sq[..., 1]) + sq[..., 2]) <= 1.0
    i, j = ac.radius_pairs(p, 1.0)
    assert np.array_equal(np.c_[i, j], np.argwhere(adj))
    for rows, kw in ac.PLANS.items():
        P = ac.plan(p, 1.0, **kw)
        order = P["order"]
        adj_lib = adj[order][:, order]
        assert np.array_equal(P["rowlen"], adj_lib.sum(1)) and np.array_equal(P["over_stash"], adj_lib.sum(1) > 128)
        for t in range((n + rows - 1) // rows):
            blk = adj_lib[t * rows:(t + 1) * rows]
            assert P["rows"][t] == blk.shape[0] and P["entries"][t] == blk.sum()
            assert P["distinct"][t] == blk.any(0).sum() and P["longest"][t] == blk.sum(1).max()
            want = "fallback_entries" if blk.sum() > kw["ecap"] else "fallback_distinct" if blk.any(0).sum() > kw["maxd"] else "staged"
            assert P["branch"][t] == want


@pytest.mark.parametrize("seed", [0, 1, 2])
def test_library_order_is_the_stable_morton_order(seed):
    rng = np.random.default_rng(seed)
    p = np.round(rng.uniform(-6, 9, (700, 3)) * 2) / 2
    mn, inv, dims, c = ac.grid_of(p, 1.0)
    assert np.array_equal(mn, p.min(0)) and inv == 1.0 / (1.0 * (1.0 + 1e-9))
    assert (c >= 0).all() and (c < np.array(dims)).all() and (c.max(0) == np.array(dims) - 1).all()
    # bit b of x is bit 3 b of the key, of y bit 3 b + 1, of z bit 3 b + 2: sort by the bits from the top one down
    bits = [(c[:, a] >> b) & 1 for b in range(10) for a in range(3)]      # least significant key first for lexsort
    want = np.lexsort(tuple(bits))                                        # lexsort is stable: ties keep the caller's order
    assert np.array_equal(ac.library_order(p, 1.0), want)
    key = ac.morton_keys(c)
    assert np.array_equal(key, sum(((c[:, a] >> b) & 1).astype(np.uint64) << np.uint64(3 * b + a) for b in range(10) for a in range(3)))


def test_clique_layout_is_contiguous_in_library_order():
    for name in ("cliques16", "cliques32", "cliques_no_row_over"):
        c = ac.case(name)
        P = c.plan(16)
        assert np.array_equal(P["order"], np.arange(c.n))                 # x order = Morton order = caller's order
        assert np.array_equal(P["rowlen"], np.repeat(c.sizes, c.sizes))   # every row of a cluster has its size in entries
        assert ac.grid_of(c.points, 1.0)[2][1:] == (1, 1)


# --------------------------------------------------------------------------------------------- the fixtures' claims
def _all_claims():
    return [(c.name, cl) for c in ac.cases() for cl in c.claims]


@pytest.mark.parametrize("name,claim", _all_claims(), ids=lambda v: v if isinstance(v, str) else "-".join(map(str, v)).replace(" ", ""))
def test_fixture_sits_on_its_threshold(name, claim):
    assert ac.claim_holds(ac.case(name), claim), f"{name} no longer hits {claim}"


def test_every_threshold_is_claimed_and_by_one_fixture_where_it_matters():
    claimed = {}
    for c in ac.cases():
        for cl in c.claims:
            claimed.setdefault(cl, []).append(c.name)
    missing = [r for r in REQUIRED if r not in claimed]
    assert not missing, missing
    # removing a fixture must make this test fail: the plan thresholds have exactly one carrier each ...
    for cl, names in claimed.items():
        if cl[0] in ("tile_entries", "distinct", "longest", "mirror", "tail", "width", "walk", "grid", "underflow", "radius", "ordinary"):
            assert len(names) == 1, (cl, names)
    # ... and every fixture carries something
    assert all(c.claims for c in ac.cases())
    assert all(c.n <= 12000 for c in ac.cases())


def test_translated_chunks_have_the_pattern_of_the_untranslated_one():
    b = ac.case("walk_3d")
    for name in ("walk_3d_map", "walk_3d_negative"):
        c = ac.case(name)
        assert np.array_equal(c.ref().indptr, b.ref().indptr) and np.array_equal(c.ref().indices, b.ref().indices)
        assert np.array_equal(c.ref().data, b.ref().data)       # the translation is exact, so every distance is the same number
    assert np.array_equal(ac.case("walk_3d_map").points - b.points, np.broadcast_to(ac.MAP_SHIFT, b.points.shape))


def test_underflowing_weights_stay_entries():
    c = ac.case("underflow")
    r = c.ref()
    A = sp.csr_matrix((r.data, r.indices, r.indptr), shape=(c.n, c.n))
    assert 0.0 < A[0, 1] < 2.0 ** -1022 and A[0, 2] == 0.0 and A[1, 2] == 0.0
    assert r.indptr[1] - r.indptr[0] == 6                        # the clique's row keeps all six entries, two of them ~0
    B = ncuts_ref.affinity_sparse(c.points, c.tarl, None, **{k: v for k, v in c.kw().items() if k != "beta"})
    assert np.array_equal(B.indptr, r.indptr) and np.array_equal(B.indices, r.indices)   # affinity_sparse keeps them too
    assert abs(B[0, 1] - A[0, 1]) <= ac.bound(r)[1] and B[0, 2] == 0.0


# --------------------------------------------------------------------------------------------- reference vs the dense oracle
SMALL = ["tail_2", "tail_17", "tail_33", "tail_1023", "walk_line", "walk_sheet", "walk_nx1", "underflow", "at_radius",
         "width_1_7", "width_100_112", "width_96_384", "alpha0", "theta0_with_features", "sam_one_camera", "two_cameras_100",
         "two_cameras_384", "cliques_no_row_over"]


@pytest.mark.parametrize("name", SMALL)
def test_reference_agrees_with_dense_oracle(name):
    c = ac.case(name)
    D = ncuts_ref.affinity_dense(c.points, c.tarl, c.dino, sam=c.sam, **c.kw())
    mask = cdist(c.points, c.points) <= c.radius
    r = c.ref()
    pat = sp.csr_matrix((np.ones(r.indices.size), r.indices, r.indptr), shape=(c.n, c.n)).toarray() > 0
    assert np.array_equal(pat, mask)
    assert not D[~mask].any()
    A = sp.csr_matrix((D[r.rows, r.indices], r.indices, r.indptr), shape=(c.n, c.n))
    m = ac.check_affinity(c, A, "dense oracle")
    assert m["max_ratio"] <= 1.0


# --------------------------------------------------------------------------------------------- teeth
MODEL_CASES = ["cliques16", "cliques32", "walk_3d", "tail_1025", "width_1_7", "width_100_112", "width_112_400", "width_400_100",
               "sam_one_camera", "two_cameras_100", "underflow", "at_radius", "random_mixed"]


@pytest.mark.parametrize("name", MODEL_CASES)
@pytest.mark.parametrize("order", ["tree", "lanes16"])
def test_float64_model_of_the_device_orders_passes(name, order):
    c = ac.case(name)
    m = ac.check_affinity(c, ac.model_affinity(c, order), order)
    print(f"\n[model {name} {order}] error / bound {m['max_ratio']:.3f}")
    assert m["max_ratio"] <= 1.0


def _rejected(c, A, *needles):
    with pytest.raises(AssertionError) as e:
        ac.check_affinity(c, A, "mutant")
    msg = str(e.value)
    for s in ("row ", "column ", "tile16 ", "tile32 ") + needles:
        assert s in msg, msg
    assert any(b in msg for b in ("staged", "fallback_entries", "fallback_distinct")), msg
    return msg


def test_mutant_last_dimension_dropped():
    for name in ("width_96_384", "width_1_7", "cliques32"):
        c = ac.case(name)
        _rejected(c, ac.model_affinity(c, drop_last_dim=True), "error")


def test_mutant_zero_row_exemption_for_i_only():
    c = ac.case("cliques16")
    _rejected(c, ac.model_affinity(c, zero_rule="i_only"))


def test_mutant_strict_radius():
    c = ac.case("at_radius")
    msg = _rejected(c, ac.model_affinity(c, strict_radius=True), "pattern differs")
    assert "row 0" in msg and "missing [1, 2, 6]" in msg


def _row_of_length(c, L):
    r = c.ref()
    rows = np.nonzero(np.diff(r.indptr) == L)[0]
    return int(rows[len(rows) // 2])


def test_mutant_entry_of_a_129_row_taken_from_its_neighbour():
    c = ac.case("cliques16")
    A = ac.model_affinity(c)
    i = _row_of_length(c, 129)
    e = A.indptr[i] + 128 if A.indices[A.indptr[i] + 128] != i else A.indptr[i] + 127      # the entry past the stash
    A.data[e] = A.data[e - 1]
    msg = _rejected(c, A)
    assert f"row {i} " in msg and "row length 129" in msg


@pytest.mark.parametrize("ulps,what", [(64, "error"), (1, "not symmetric bit for bit")])
def test_mutant_value_off_by_ulps(ulps, what):
    c = ac.case("cliques32")
    A = ac.model_affinity(c)
    i = _row_of_length(c, 65)
    e = A.indptr[i] + (1 if A.indices[A.indptr[i]] == i else 0)
    j = A.indices[e]
    pairs = [e] if ulps == 1 else [e, A.indptr[j] + int(np.searchsorted(A.indices[A.indptr[j]:A.indptr[j + 1]], i))]
    for k in pairs:
        A.data[k] = (A.data[k:k + 1].view(np.int64) + ulps).view(np.float64)[0]
    _rejected(c, A, what)


def test_mutant_diagonal():
    c = ac.case("tail_33")
    A = ac.model_affinity(c)
    A.data[A.indptr[5] + int(np.searchsorted(A.indices[A.indptr[5]:A.indptr[6]], 5))] = np.nextafter(1.0, 0.0)
    _rejected(c, A, "error")     # the diagonal's bound is 0: the value check names it
