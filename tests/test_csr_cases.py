"""CPU suite: the hand-built CSR fixtures of tests/csr_cases.py sit where they claim to sit, their input forms have one value, and the
dense float64 reference and the NumPy model of the device algorithm agree on them with margins that keep the GPU tests
(tests/test_gpu_csr_cases.py, tests/test_gpu_flow_values.py) from resting on a coin toss."""
import numpy as np
import pytest
import scipy.sparse as sp

import csr_cases as cc
import gpu_model

LIMIT_REFS = [("limit", name, None) for name in cc.LIMIT_CASES]
SMALL_REFS = [("small", "canonical", d) for d in cc.SMALL_DIAGONALS] + [("small", "zero_bridges", 1.0)]


def test_band_has_the_claimed_rows():
    w = cc.limit_case("band")
    L = cc.row_lengths(w)
    assert w.shape == (1764, 1764) and w.nnz == 214146 and L.max() == 401
    assert {15, 16, 17, 63, 64, 65} <= set(L.tolist())
    assert w.has_sorted_indices and (w != w.T).nnz == 0 and np.all(w.diagonal() == 1.0)
    # one bridge between consecutive blocks and nothing else
    off = np.concatenate([[0], np.cumsum(cc.BAND["sizes"])])
    for k, b in enumerate(cc.BAND["bridges"]):
        blk = w[off[k]:off[k + 1]][:, off[k + 1]:]
        assert blk.nnz == 1 and w[off[k + 1] - 1, off[k + 1]] == b == w[off[k + 1], off[k + 1] - 1]


def test_band128_tasks_sit_on_the_entry_limit_and_the_twin_one_above():
    """Interior rows (64..447) hold 128 entries, so the root tasks 2..13 hold exactly 4096 = AI_ENC_MAXNNZ; the twin's one stored
    diagonal entry at row 200 gives task 6 4097 and leaves the others."""
    w, twin = cc.limit_case("band128"), cc.limit_case("band128_diag")
    L = cc.row_lengths(w)
    assert w.shape == (812, 812) and np.all(L[64:448] == 128) and L.max() == 128 and np.all(w.diagonal() == 0)
    nnz, cols = cc.task_counts(w)
    assert np.flatnonzero(nnz == 4096).tolist() == list(range(2, 14)) and nnz.max() == 4096 and cols.max() < 1024
    nnz2, _ = cc.task_counts(twin)
    assert twin.nnz == w.nnz + 1 and twin[cc.BAND128_DIAG_ROW, cc.BAND128_DIAG_ROW] == 1.0 and twin.diagonal().sum() == 1.0
    assert nnz2[cc.BAND128_DIAG_ROW // 32] == 4097 and np.array_equal(np.delete(nnz2, 6), np.delete(nnz, 6))
    assert (twin != twin.T).nnz == 0 and twin.has_sorted_indices


def test_stride_blocks_sit_on_the_distinct_column_limit():
    """Root task 17 (rows 544..575): 1024 entries in 1024 distinct columns = AI_ENC_XCAP; 1056 of each with a unit diagonal."""
    w, wd = cc.limit_case("stride"), cc.limit_case("stride_diag")
    assert w.shape == (2300, 2300) and np.all(w.diagonal() == 0) and np.all(wd.diagonal() == 1.0)
    from scipy.sparse.csgraph import connected_components
    assert connected_components(w, directed=False)[0] == 1
    nnz, cols = cc.task_counts(w)
    assert (nnz[17], cols[17]) == (1024, 1024) and cols.max() == 1024 and nnz.max() == 1024
    nnz, cols = cc.task_counts(wd)
    assert (nnz[17], cols[17]) == (1056, 1056) and cols.max() == 1056
    assert w[1099, 1100] == 2e-3 == w[1100, 1099] and w[:1100][:, 1100:].nnz == 1
    assert (w != w.T).nnz == 0 and (wd != wd.T).nnz == 0


@pytest.mark.parametrize("diagonal", cc.SMALL_DIAGONALS)
def test_every_form_of_small_has_the_value_of_the_canonical_form(diagonal):
    can = cc.small("canonical", diagonal)
    assert can.has_sorted_indices and (can != can.T).nnz == 0 and not np.any(can.data == 0)
    assert np.all(can.diagonal() == (diagonal or 0.0))
    assert np.array_equal(can.data.astype(np.float32).astype(np.float64), can.data)
    dense = can.toarray()
    for form in cc.SMALL_FORMS:
        w = cc.small(form, diagonal)
        if form == "zero_bridges":
            diff = np.argwhere(w.toarray() != dense)
            off = np.cumsum(cc.SMALL["sizes"])[:-1]
            assert sorted(map(tuple, diff)) == sorted([(o - 1, o) for o in off] + [(o, o - 1) for o in off])
            assert (w.data == 0).sum() == 8 and w.nnz == can.nnz
            continue
        assert np.array_equal(w.toarray(), dense), form
        v = cc.by_value(w)
        assert np.array_equal(v.indptr, can.indptr) and np.array_equal(v.indices, can.indices), form
        assert np.array_equal(v.data.view(np.int64), can.data.view(np.int64)), form
    assert not cc.small("shuffled", diagonal).has_sorted_indices
    assert cc.small("split", diagonal).nnz > can.nnz and cc.small("zeros", diagonal).nnz > can.nnz
    assert cc.small("float32", diagonal).dtype == np.float32 and sp.issparse(cc.small("coo", diagonal))
    # the diagonal forms differ on the diagonal alone
    base = cc.small("canonical", None).toarray()
    assert np.array_equal(dense - np.diag(np.diag(dense)), base)


def test_the_api_detects_duplicates_without_touching_the_matrix():
    from autoinst_amd import ncuts_api as api
    for form, dup in (("canonical", False), ("shuffled", False), ("zeros", False), ("split", True)):
        w = sp.csr_matrix(cc.small(form))
        before = (w.indptr.copy(), w.indices.copy(), w.data.copy())
        assert api._has_duplicates(w) is dup, form
        assert all(np.array_equal(a, b) for a, b in zip(before, (w.indptr, w.indices, w.data)))
    empty = sp.csr_matrix((4, 4))
    assert api._has_duplicates(empty) is False
    two = sp.csr_matrix((np.array([1.0, 1.0]), np.array([1, 1], dtype=np.int32), np.array([0, 0, 2, 2])), shape=(3, 3))
    assert api._has_duplicates(two) is True
    # the same column at the end of one row and the start of the next is no duplicate
    edge = sp.csr_matrix((np.array([1.0, 1.0]), np.array([1, 1], dtype=np.int32), np.array([0, 1, 2, 2])), shape=(3, 3))
    assert api._has_duplicates(edge) is False


@pytest.mark.parametrize("key", LIMIT_REFS + SMALL_REFS, ids=lambda k: "-".join(str(x) for x in k))
def test_dense_reference_and_model_agree_with_margins(key):
    """Same groups in the same order; every cost that is cut lies below T / 10 and every cost that is refused above 2 T; no solved
    segment has two different masks within `flow_dump.COST_RTOL` of each other -- except the 3-row block, whose two one-against-two
    masks are mirror images of each other (the block is symmetric under reversal) and cost the same: both lie far above 2 T, the
    block stays whole whichever wins, and no GPU test asks which one did."""
    dense, model, ds, ms = cc.reference(*key)
    assert cc.same_groups(dense, model)
    assert ds.get("null", 0) == ms.get("null", 0) and len(ds["segments"]) == ms["lanczos"]
    assert sorted(ds["segments"]) == sorted(n for n, _, _, _ in ms["iters"])
    assert max(ds.get("cut", [0.0])) < cc.T / 10 and min(ds["refused"]) > 2 * cc.T
    assert set(ds.get("near_ties", [])) <= {3}
    n = sum(len(g) for g in dense)
    assert np.array_equal(np.sort(np.concatenate(dense)), np.arange(n))


def test_band_reference_numbers():
    """num_points_orig = 100: the nine blocks in the order below, the 3-row block solved too (m = n - 1 = 2), segments on both sides
    of 32, 64 and 512 rows, Krylov sizes on both sides of 32 (AI_SLAB_VECS) and 64 (FK_CHECK_WIDE_M)."""
    dense, model, ds, ms = cc.reference("limit", "band")
    assert [len(g) for g in model] == [64, 32, 511, 33, 31, 512, 65, 3, 513]
    off = np.concatenate([[0], np.cumsum(cc.BAND["sizes"])])
    blocks = {(int(a), int(b)) for a, b in zip(off[:-1], off[1:])}
    assert {(int(g.min()), int(g.max()) + 1) for g in model} == blocks and all(len(g) == g.max() - g.min() + 1 for g in model)
    solved = {n: m for n, m, _, _ in ms["iters"]}
    assert {3, 31, 32, 33, 64, 65, 511, 512, 513, 1764} <= set(solved)
    assert solved[3] == 2
    ms_ = sorted(m for _, m, _, _ in ms["iters"])
    assert ms_[0] < 32 < ms_[-1] and any(m < 32 for m in ms_) and any(32 < m < 64 for m in ms_) and any(m > 64 for m in ms_)
    assert max(ds["cut"]) <= 2.0e-4 and min(ds["refused"]) >= 1.44e-2


def test_stride_and_band128_reference_numbers():
    for name, root, leaf in (("stride", 2.7e-7, 5.7e-2), ("stride_diag", 2.5e-7, 5.3e-2)):
        dense, model, ds, ms = cc.reference("limit", name)
        assert [len(g) for g in model] == [1100, 1200]
        assert ds["cut"] == pytest.approx([root], rel=0.03) and min(ds["refused"]) == pytest.approx(leaf, rel=0.03)
    for name in ("band128", "band128_diag"):
        dense, model, ds, ms = cc.reference("limit", name)
        assert [len(g) for g in model] == [300, 512] and ms["lanczos"] == 3


def test_stored_zero_bridges_follow_the_value_not_the_pattern():
    """The finding that closed the door: a model that follows STORED entries (connected_components does) sees the five blocks of
    SMALL as one component when their bridges are stored zeros, and emits them in another order, after more solves, than on the same
    matrix with the zeros eliminated.  By value the graph is five components: one component split, then one solve per block."""
    w = sp.csr_matrix(cc.small("zero_bridges", 1.0))
    ids = np.arange(w.shape[0])
    st_stored, st_value = {}, {}
    stored = gpu_model.normalized_cut_model(w, cc.N_ORIG, ids, T=cc.T, split_lim=cc.SPLIT_LIM, stats=st_stored)
    value = gpu_model.normalized_cut_model(cc.by_value(w), cc.N_ORIG, ids, T=cc.T, split_lim=cc.SPLIT_LIM, stats=st_value)
    assert np.array_equal(w.toarray(), cc.by_value(w).toarray())
    assert [len(g) for g in value] == [33, 65, 31, 3, 64] and st_value["null"] == 1 and st_value["lanczos"] == 5
    assert [len(g) for g in stored] != [len(g) for g in value] and st_stored["lanczos"] > 5
    dense, model, ds, _ = cc.reference("small", "zero_bridges", 1.0)
    assert cc.same_groups(dense, value) and cc.same_groups(model, value) and ds["null"] == 1
