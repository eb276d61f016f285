"""GPU suite (-m gpu): the contract of a caller-built CSR (ai_csr_from_host, DeviceGraph.from_scipy) and the shipped cut (ai_ncut,
ai_ncut_batch, ai_ncut_tree) on the hand-built graphs of tests/csr_cases.py, whose rows, 32-row tasks and segments sit exactly on the
thresholds of the fk_* kernels.  The yardsticks are the dense float64 restatement of the reference (`csr_cases.dense_reference`) and
the NumPy model of the device algorithm (`gpu_model`); every tolerance is one of tests/test_gpu_tree.py's."""
import ctypes as C

import numpy as np
import pytest
import scipy.sparse as sp

import csr_cases as cc

pytestmark = pytest.mark.gpu

SENTINEL = 0x5A5A5A5A


@pytest.fixture(scope="module")
def api():
    from autoinst_amd import ncuts_api
    ncuts_api.default_context()
    return ncuts_api


@pytest.fixture(scope="module")
def ctx(api):
    """A context of this module's own: its workspace and graph cache come and go with these tests, and the session's default context
    reaches the later test files as it would without them."""
    own = api.Context()
    yield own
    own.close()


@pytest.fixture(scope="module")
def cut(api, ctx):
    """key -> (graph, labels, n_groups, stats) of the solo `ncuts_labels` call; each graph is uploaded and cut once per module."""
    done = {}

    def get(kind, name, diagonal=None):
        key = (kind, name, diagonal)
        if key not in done:
            w = cc.limit_case(name) if kind == "limit" else cc.small(name, diagonal)
            g = api.DeviceGraph.from_scipy(w, ctx)
            lab, ng, st = api.ncuts_labels(g, cc.N_ORIG, cc.T, cc.SPLIT_LIM)
            done[key] = (g, lab, ng, st)
        return done[key]

    yield get
    for g, _, _, _ in done.values():
        g.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _arrays(w):
    w = sp.csr_matrix(w)
    return (np.ascontiguousarray(w.indptr, dtype=np.int64), np.ascontiguousarray(w.indices, dtype=np.int32),
            np.ascontiguousarray(w.data, dtype=np.float64))


def _from_host(ctx, indptr, indices, data):
    from autoinst_amd import _ffi
    h = C.c_void_p(SENTINEL)
    st = _ffi.load().ai_csr_from_host(ctx._h, indptr.shape[0] - 1, indptr.ctypes.data, indices.ctypes.data, data.ctypes.data, C.byref(h))
    return st, h, _ffi.load().ai_last_error().decode()


def _entry(indptr, indices, i, j):
    e = indptr[i] + int(np.flatnonzero(indices[indptr[i]:indptr[i + 1]] == j)[0])
    assert indices[e] == j
    return e


def _without(indptr, indices, data, e):
    ip = indptr.copy()
    ip[np.searchsorted(indptr, e, side="right"):] -= 1
    return ip, np.delete(indices, e), np.delete(data, e)


def _with_duplicate(indptr, indices, data, e):
    """Entry e stored once more, at the end of its row."""
    i = int(np.searchsorted(indptr, e, side="right")) - 1
    ip = indptr.copy()
    ip[i + 1:] += 1
    at = indptr[i + 1]
    return ip, np.insert(indices, at, indices[e]), np.insert(data, at, data[e])


def _set(data, e, v):
    d = data.copy()
    d[e] = v
    return d


ROW, COL = 40, 45      # an edge inside the 65-row block of SMALL (rows 33..97, band 16)


def _refused_inputs():
    indptr, indices, data = _arrays(cc.small("canonical", 1.0))
    e = _entry(indptr, indices, ROW, COL)
    v = data[e]
    s_indptr, s_indices, s_data = _arrays(cc.small("shuffled", 1.0))      # rows the host has to sort before it can judge them
    return {
        "mirror_missing_unsorted": _without(s_indptr, s_indices, s_data, _entry(s_indptr, s_indices, COL, ROW)),
        "mirror_one_ulp_unsorted": (s_indptr, s_indices, _set(s_data, _entry(s_indptr, s_indices, COL, ROW), np.nextafter(v, 1.0))),
        "nan": (indptr, indices, _set(data, e, np.nan)),
        "inf": (indptr, indices, _set(data, e, np.inf)),
        "negative": (indptr, indices, _set(data, e, -v)),
        "zero": (indptr, indices, _set(data, e, 0.0)),
        "negative_zero": (indptr, indices, _set(data, e, -0.0)),
        "duplicate": _with_duplicate(indptr, indices, data, e),
        "mirror_missing": _without(indptr, indices, data, _entry(indptr, indices, COL, ROW)),
        "mirror_one_ulp": (indptr, indices, _set(data, _entry(indptr, indices, COL, ROW), np.nextafter(v, 1.0))),
    }


@pytest.mark.parametrize("rule", ["nan", "inf", "negative", "zero", "negative_zero", "duplicate", "mirror_missing", "mirror_one_ulp",
                                  "mirror_missing_unsorted", "mirror_one_ulp_unsorted"])
def test_the_door_refuses_what_the_contract_excludes(api, ctx, cut, rule):
    """AI_ERR_BAD_ARG, a message that starts with the entry's name and names the offending row and column, the handle unwritten, no
    graph memory taken -- and the context goes on: a valid upload and cut right afterwards give the canonical labels.  Only uploads
    happen with the refused arrays: none of them reaches a kernel."""
    _, lab_ref, ng_ref, _ = cut("small", "canonical", 1.0)
    live = ctx.mem_info()["graphs_live"]
    st, h, msg = _from_host(ctx, *_refused_inputs()[rule])
    assert st == -1 and h.value == SENTINEL
    assert msg.startswith("ai_csr_from_host:") and f"row {ROW}" in msg and f"column {COL}" in msg, msg
    assert ctx.mem_info()["graphs_live"] == live
    st, h, _ = _from_host(ctx, *_arrays(cc.small("canonical", 1.0)))
    assert st == 0 and h.value not in (None, SENTINEL)
    g = api.DeviceGraph(ctx, h)
    lab, ng, _ = api.ncuts_labels(g, cc.N_ORIG, cc.T, cc.SPLIT_LIM)
    g.free()
    assert ng == ng_ref and np.array_equal(lab, lab_ref)
    assert ctx.mem_info()["graphs_live"] == live


@pytest.mark.parametrize("rule", ["nan", "inf", "negative", "mirror_missing", "mirror_one_ulp"])
def test_from_scipy_raises_value_error_with_the_library_message(api, ctx, rule):
    indptr, indices, data = _refused_inputs()[rule]
    n = indptr.shape[0] - 1
    live = ctx.mem_info()["graphs_live"]
    with pytest.raises(ValueError, match=f"ai_csr_from_host: .*row {ROW}.*column {COL}"):
        api.DeviceGraph.from_scipy(sp.csr_matrix((data, indices, indptr), shape=(n, n)), ctx)
    assert ctx.mem_info()["graphs_live"] == live


def test_accepted_exactly_as_stored(api, ctx):
    """Any column order, a partial diagonal with any positive value, empty rows: the device holds the arrays as they were passed (the
    export of an uploaded graph returns them bit for bit, unsorted columns included).  Once with shuffled rows, which the host judges,
    once sorted, where the mirrors are looked up on the device."""
    import eig_cases
    w = cc.small("canonical", None).tolil()
    w[0, 0], w[7, 7], w[100, 100] = 3.5, 1e-300, 0.25
    w = sp.bmat([[sp.csr_matrix(w), None], [None, sp.csr_matrix((3, 3))]], format="csr")     # three empty rows at the end
    w.sort_indices()
    assert np.diff(w.indptr)[-3:].sum() == 0 and np.count_nonzero(w.diagonal()) == 3
    for m in (eig_cases.shuffle_columns(w, 9), w):
        indptr, indices, data = _arrays(m)
        assert m.has_sorted_indices == (m is w)
        st, h, msg = _from_host(ctx, indptr, indices, data)
        assert st == 0, msg
        g = api.DeviceGraph(ctx, h)
        back = g.to_scipy()
        g.free()
        assert np.array_equal(back.indptr, indptr) and np.array_equal(back.indices, indices)
        assert np.array_equal(_bits(back.data), _bits(data))


# ------------------------------------------------------------------------------------------------------------ equal by value
@pytest.mark.parametrize("form,diagonal", [("split", 1.0), ("zeros", 1.0), ("zeros", None)])
def test_duplicates_and_stored_zeros_are_the_canonical_matrix(api, cut, form, diagonal):
    """`from_scipy` sums duplicates and drops stored zeros: the device holds the canonical arrays, and labels, group count and the
    tree's heights and leaf costs are bit-equal to the canonical form's."""
    g0, lab0, ng0, _ = cut("small", "canonical", diagonal)
    g, lab, ng, _ = cut("small", form, diagonal)
    a, b = g.to_scipy(), g0.to_scipy()
    assert np.array_equal(a.indptr, b.indptr) and np.array_equal(a.indices, b.indices) and np.array_equal(_bits(a.data), _bits(b.data))
    assert ng == ng0 and np.array_equal(lab, lab0)
    t, t0 = api.ncuts_tree(g, cc.N_ORIG, cc.T), api.ncuts_tree(g0, cc.N_ORIG, cc.T)
    assert t.n_groups == t0.n_groups == ng0 and np.array_equal(t.labels, t0.labels) and np.array_equal(t.labels, lab0)
    assert np.array_equal(_bits(t.cut_height), _bits(t0.cut_height)) and np.array_equal(_bits(t.leaf_cost), _bits(t0.leaf_cost))


def test_bridges_stored_as_zeros_are_no_bridges(api, ctx, cut):
    """By value the five blocks are five components: one component split, the groups of the eliminated matrix and of the model, in
    the order [33, 65, 31, 3, 64]."""
    g, lab, ng, st = cut("small", "zero_bridges", 1.0)
    _, model, _, ms = cc.reference("small", "zero_bridges", 1.0)
    assert [len(x) for x in model] == [33, 65, 31, 3, 64]
    assert ng == 5 and np.array_equal(lab, cc.labels_of(model, g.n))
    assert st["null_solves"] == 1 == ms["null"] and st["unconverged"] == 0
    ge = api.DeviceGraph.from_scipy(cc.by_value(cc.small("zero_bridges", 1.0)), ctx)
    lab_e, ng_e, st_e = api.ncuts_labels(ge, cc.N_ORIG, cc.T, cc.SPLIT_LIM)
    ge.free()
    assert ng_e == ng and np.array_equal(lab_e, lab) and st_e["null_solves"] == 1


@pytest.mark.parametrize("form", ["shuffled", "csc", "coo", "float32"])
def test_other_storage_of_the_same_value_gives_the_same_groups(api, cut, form):
    """Same groups in the same order; cut_height has its -inf and 0.0 entries at the same places and agrees elsewhere within rel
    1e-10 (the bound of tests/test_gpu_tree.py against the model)."""
    g0, lab0, ng0, _ = cut("small", "canonical", 1.0)
    g, lab, ng, st = cut("small", form, 1.0)
    assert ng == ng0 and np.array_equal(lab, lab0) and st["unconverged"] == 0
    h, h0 = api.ncuts_tree(g, cc.N_ORIG, cc.T).cut_height, api.ncuts_tree(g0, cc.N_ORIG, cc.T).cut_height
    assert h.shape == h0.shape and np.array_equal(np.isneginf(h), np.isneginf(h0)) and np.array_equal(h == 0.0, h0 == 0.0)
    pos = h0 > 0.0
    print("cut_height: largest relative difference", np.max(np.abs(h[pos] - h0[pos]) / h0[pos], initial=0.0))
    assert np.all(np.abs(h[pos] - h0[pos]) <= 1e-10 * h0[pos])


# ------------------------------------------------------------------------------------------------------------ against references
def _against_references(api, cut, key):
    from oracle import ncuts_ref
    g, lab, ng, st = cut(*key)
    dense, model, ds, ms = cc.reference(*key)
    print(f"{key}: groups {ng} (dense {len(dense)}, model {len(model)}); lanczos {st['lanczos_solves']} (model {ms.get('lanczos', 0)}); "
          f"null {st['null_solves']} (model {ms.get('null', 0)}); unconverged {st['unconverged']}")
    assert ncuts_ref.partitions_equal(lab, cc.labels_of(dense, g.n))
    assert ng == len(model) and np.array_equal(lab, cc.labels_of(model, g.n))
    assert st["unconverged"] == 0
    return g, lab, ng, st, ms


@pytest.mark.parametrize("diagonal", cc.SMALL_DIAGONALS)
def test_diagonal_forms_of_small_match_the_dense_reference_and_the_model(api, cut, diagonal):
    _against_references(api, cut, ("small", "canonical", diagonal))


@pytest.mark.parametrize("name", cc.LIMIT_CASES)
def test_the_cut_at_its_row_and_task_limits(api, cut, name):
    """The partition of the dense reference, the model's groups in the model's order, as many Lanczos solves and component splits as
    the model made, nothing unconverged; the tree call gives the same labels."""
    g, lab, ng, st, ms = _against_references(api, cut, ("limit", name, None))
    assert st["lanczos_solves"] == ms.get("lanczos", 0) and st["null_solves"] == ms.get("null", 0)
    tree = api.ncuts_tree(g, cc.N_ORIG, cc.T)
    assert api.last_stats()["unconverged"] == 0
    assert tree.n_groups == ng and np.array_equal(tree.labels, lab)


def test_batch_of_all_fixtures_equals_the_solo_calls(api, cut):
    """Every fixture in ONE ai_ncut_batch call, and once more with window_rows = 1 (one chunk at a time): labels bit-equal to the
    solo calls."""
    keys = [("limit", n, None) for n in cc.LIMIT_CASES] + [("small", "canonical", d) for d in cc.SMALL_DIAGONALS]
    keys += [("small", f, 1.0) for f in ("shuffled", "zero_bridges")]
    solo = [cut(*k) for k in keys]
    graphs = [s[0] for s in solo]
    for kw in ({}, {"window_rows": 1}):
        labs, ngs, st = api.ncuts_labels_batch(graphs, [cc.N_ORIG] * len(graphs), cc.T, cc.SPLIT_LIM, **kw)
        assert st["unconverged"] == 0
        assert ngs == [s[2] for s in solo]
        for k, a, s in zip(keys, labs, solo):
            assert np.array_equal(a, s[1]), (k, kw)
