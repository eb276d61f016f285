"""GPU suite (-m gpu): the cut tree of a chunk (ai_ncut_tree, ai_ncut_tree_batch, ai_ncut_relabel).

The yardstick for labels derived from a tree is the device's own direct cut at the same threshold (`ncuts_labels`), bit for bit,
and the CPU model (`tree_ref.tree_model`) -- never the goldens' labels at another T, which are not nested."""
import ctypes as C
import json
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import ROOT
import tree_ref

pytestmark = pytest.mark.gpu

FIXTURES = [("g1_blob_pair_spatial", 0.5), ("g2_multicomp_spatial", 0.3), ("g5_surface3k_T003", 0.3)]


@pytest.fixture(scope="module")
def api():
    from autoinst_amd import ncuts_api
    ncuts_api.default_context()
    return ncuts_api


@pytest.fixture(scope="module")
def cut(api):
    """name -> (graph, tree at the fixture's T_max), cut once for the module."""
    out = {}
    for name, T_max in FIXTURES:
        g = api.DeviceGraph.from_scipy(tree_ref.load_graph(name))
        out[name] = (g, api.ncuts_tree(g, g.n, T_max))
        assert api.last_stats()["unconverged"] == 0
    yield out
    for g, _ in out.values():
        g.free()


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same_tree(a, b):
    assert a.n_groups == b.n_groups and np.array_equal(a.labels, b.labels)
    assert np.array_equal(_bits(a.cut_height), _bits(b.cut_height))
    assert np.array_equal(_bits(a.leaf_cost), _bits(b.leaf_cost))


@pytest.mark.parametrize("name,T_max", FIXTURES)
def test_derived_labels_equal_the_direct_cut_at_the_threshold(api, cut, name, T_max):
    """At every distinct height h and at the next float above it (g5: the three configuration values and 20 heights), at 0 and at
    T_max: labels and group counts from the tree equal `ncuts_labels` at that T bit for bit.  At T_max that is also the statement
    that the tree call leaves the plain cut's labels unchanged."""
    g, tree = cut[name]
    lab, ng, _ = api.ncuts_labels(g, g.n, T_max)
    assert tree.n_groups == ng and np.array_equal(tree.labels, lab) and tree.labels.dtype == np.int32
    ts = tree_ref.sweep_thresholds(tree.cut_height, T_max, limit=20 if name.startswith("g5") else None)
    if name.startswith("g5"):
        ts += [0.005, 0.03, 0.075]
    derived, counts = api.relabel([tree], ts)
    changes = 0
    for t, T in enumerate(ts):
        lab, ng, _ = api.ncuts_labels(g, g.n, T)
        assert int(counts[t, 0]) == ng == tree.n_groups_at(T), (T, int(counts[t, 0]), ng)
        assert np.array_equal(derived[t][0], lab), T
        changes += ng != tree.n_groups
    assert changes >= len(ts) // 2      # the thresholds do move the partition
    assert np.array_equal(tree.labels_at(ts[2]), derived[2][0])
    groups = tree.groups_at(ts[3], ids=np.arange(g.n) + 10)
    assert len(groups) == int(counts[3, 0]) and np.array_equal(np.sort(np.concatenate(groups)), np.arange(g.n) + 10)


@pytest.mark.parametrize("name,T_max", FIXTURES)
def test_tree_equals_the_model(cut, name, T_max):
    """Same partition in the same order as `tree_ref.tree_model`; the -inf / 0.0 entries of cut_height at the same places exactly,
    the others (and the finite leaf costs) within rel 1e-10 -- the bound tests/test_gpu_flow_values.py applies to mcut."""
    g, tree = cut[name]
    with tree_ref.cached_solver():
        tm = tree_ref.tree_model(tree_ref.load_graph(name), g.n, T_max)
    assert tree.n_groups == tm.cut_height.shape[0] and np.array_equal(tree.labels, tm.labels)
    h, hm = tree.cut_height, tm.cut_height
    assert h[0] == -np.inf and np.array_equal(np.isneginf(h), np.isneginf(hm)) and np.array_equal(h == 0.0, hm == 0.0)
    pos = hm > 0.0
    print("cut_height: largest relative difference", np.max(np.abs(h[pos] - hm[pos]) / hm[pos], initial=0.0))
    assert np.all(np.abs(h[pos] - hm[pos]) <= 1e-10 * hm[pos])
    assert np.all(h[1:] < T_max)
    c, cm = tree.leaf_cost, tm.leaf_cost
    assert np.array_equal(np.isnan(c), np.isnan(cm))
    fin = np.isfinite(c) & np.isfinite(cm)
    assert fin.any() and np.all(np.abs(c[fin] - cm[fin]) <= 1e-10 * cm[fin])
    assert np.all(c[~np.isnan(c)] >= T_max)


@pytest.mark.parametrize("name,T_max", FIXTURES)
def test_smallest_leaf_cost_is_where_the_partition_changes_next(api, cut, name, T_max):
    g, tree = cut[name]
    m = float(np.min(tree.leaf_cost[np.isfinite(tree.leaf_cost)]))
    assert m >= T_max
    lab, ng, _ = api.ncuts_labels(g, g.n, m)
    assert ng == tree.n_groups and np.array_equal(lab, tree.labels)
    _, ng_next, _ = api.ncuts_labels(g, g.n, float(np.nextafter(m, np.inf)))
    assert ng_next > tree.n_groups


def test_batch_equals_separate_calls(api):
    """Four fixtures, a chunk too small to split and a 2-point chunk: one window, and window_rows at its minimum (one chunk at a
    time); labels, heights and leaf costs bit-equal to the per-chunk calls."""
    mats = [tree_ref.load_graph(n) for n in ("g1_blob_pair_spatial", "g2_multicomp_spatial", "g5_surface3k_T003", "g6_connected_tarl")]
    rng = np.random.default_rng(3)
    small = sp.csr_matrix(np.triu(rng.uniform(0.2, 1.0, (5, 5)), 1))
    mats += [small + small.T, sp.csr_matrix(np.array([[0.0, 0.5], [0.5, 0.0]]))]
    norig = [m.shape[0] for m in mats]
    norig[4] = 1000      # 5 rows of a 1000-point chunk: below split_lim
    graphs = [api.DeviceGraph.from_scipy(m) for m in mats]
    T_max = 0.075
    single = [api.ncuts_tree(g, no, T_max) for g, no in zip(graphs, norig)]
    assert [t.n_groups for t in single[4:]] == [1, 1] and all(np.isnan(t.leaf_cost[0]) for t in single[4:])
    assert all(t.n_groups > 1 for t in single[:4])
    for kw in ({}, {"window_rows": 1}):
        batch = api.ncuts_tree_batch(graphs, norig, T_max, **kw)
        assert api.last_stats()["unconverged"] == 0
        for a, b in zip(batch, single):
            _same_tree(a, b)
    labs, ngs, _ = api.ncuts_labels_batch(graphs, norig, T_max)
    assert ngs == [t.n_groups for t in single] and all(np.array_equal(a, t.labels) for a, t in zip(labs, single))
    for g in graphs:
        g.free()


def test_leaf_cost_and_the_optional_arguments_may_be_null(api, cut):
    """The C entry with leaf_cost, opts and stats all NULL fills labels and heights as the full call does."""
    from autoinst_amd import _ffi
    g, tree = cut["g2_multicomp_spatial"]
    lab = np.full(g.n, -1, dtype=np.int32)
    hgt = np.full(g.n, 7.0)
    ng = C.c_int32(-1)
    st = _ffi.load().ai_ncut_tree(g.ctx._h, g._h, g.n, 0.3, 0.01, None, lab.ctypes.data, C.byref(ng), hgt.ctypes.data, None, None)
    assert st == 0 and ng.value == tree.n_groups and np.array_equal(lab, tree.labels)
    assert np.array_equal(_bits(hgt[:ng.value]), _bits(tree.cut_height)) and np.all(hgt[ng.value:] == 7.0)
    assert _ffi.load().ai_ncut_tree(g.ctx._h, g._h, g.n, 0.3, 0.01, None, lab.ctypes.data, C.byref(ng), None, None, None) == -1


def test_normalized_cut_sweep_and_run_chunks_with_trees(api):
    """The two callers on top: `normalized_cut_sweep` returns `normalized_cut` at every T; `sharding.run_chunks(tree=True)` returns
    trees whose labels are the plain call's, and whose labels at a smaller T are those of a run at that T."""
    from autoinst_amd import sharding, synth
    A = tree_ref.load_graph("g2_multicomp_spatial")
    n = A.shape[0]
    ids = np.arange(n) * 3 + 1
    Ts = [0.03, 0.3, 0.005, 0.075]
    by_T = api.normalized_cut_sweep(A, n, ids, Ts)
    assert sorted(by_T) == sorted(Ts)
    for T in Ts:
        direct = api.normalized_cut(A, n, ids, T=T)
        assert len(by_T[T]) == len(direct) and all(np.array_equal(a, b) for a, b in zip(by_T[T], direct)), T
    chunks = [(synth.synthetic_chunk(m, seed=s, tarl=False, extent=14.0)["points"], None) for s, m in enumerate((3000, 2500, 3200))]
    kw = dict(threads=2, batch=2, alpha=1.0, theta=0.0, gamma=0.0)
    trees = sharding.run_chunks(chunks, T=0.075, tree=True, **kw)
    plain = sharding.run_chunks(chunks, T=0.075, **kw)
    lower = sharding.run_chunks(chunks, T=0.03, **kw)
    assert all(isinstance(t, api.CutTree) and t.T_max == 0.075 for t in trees)
    assert all(np.array_equal(t.labels, p) for t, p in zip(trees, plain))
    labs, counts = api.relabel(trees, [0.03])
    assert all(np.array_equal(a, b) for a, b in zip(labs[0], lower))
    assert [int(x) for x in counts[0]] == [int(l.max()) + 1 for l in lower]
    assert any(int(a.max()) < int(b.max()) for a, b in zip(lower, plain))     # the two thresholds do differ on these chunks


# ---------------------------------------------------------------------------------------------- the relabel kernels at their limits
T_TOP = 0.25
SHAPES = [(0, 0), (1, 1), (255, 2), (256, 256), (257, 257), (6000, 70000), (0, 0), (300, 1), (0, 3)]   # (points, groups) per chunk


@pytest.fixture(scope="module")
def synthetic(api):
    """Chunks of 0 / 1 / 255 / 256 / 257 points with 1 / 2 / 256 / 257 / 70 000 groups (one block of the kernels is 256 threads, one
    tile of the scan 256 x its items), heights drawn from 40 values so that thresholds hit them exactly; no cut is needed."""
    rng = np.random.default_rng(17)
    values = np.concatenate([[0.0], np.sort(rng.uniform(1e-3, T_TOP * (1 - 1e-9), 39))])
    trees = []
    for n, G in SHAPES:
        h = rng.choice(values, G)
        if G:
            h[0] = -np.inf
        lab = rng.integers(0, max(G, 1), n).astype(np.int32)
        if n >= G > 0:
            lab[:G] = np.arange(G)
        trees.append(api.CutTree(lab, G, h, None, T_TOP))
    return trees, values


def _thresholds(values, k):
    h = float(values[20])
    base = [h, float(np.nextafter(h, np.inf)), T_TOP, float(np.nextafter(h, -np.inf)), -1.0, 0.0, float(np.nextafter(0.0, 1.0)),
            float(values[1]), float(values[-1]), float(np.nextafter(values[-1], np.inf))]
    base += [float(v) for v in values[2:9]]
    return base[:k]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("k", [1, 2, 17])
def test_relabel_equals_the_restatement(api, synthetic, k, where):
    import torch
    trees, values = synthetic
    ts = _thresholds(values, k)
    assert len(ts) == k
    labs, counts = api.relabel(trees, ts, device=torch.device("cuda", 0) if where == "device" else None)
    ref_labs, ref_counts = tree_ref.relabel_chunks_ref([t.labels for t in trees], [t.cut_height for t in trees], ts)
    assert counts.shape == (k, len(trees)) and np.array_equal(counts, ref_counts)
    for t in range(k):
        for c in range(len(trees)):
            got = labs[t][c].cpu().numpy() if where == "device" else labs[t][c]
            assert got.dtype == np.int32 and np.array_equal(got, ref_labs[t][c]), (t, c)


@pytest.mark.parametrize("where", ["host", "device"])
def test_relabel_refuses_bad_input_and_writes_nothing(api, ctx, where):
    """Each refused input of the C ABI: AI_ERR_BAD_ARG, labels_out / n_groups_out untouched, and the next call works."""
    import torch
    from autoinst_amd import _ffi
    lib = _ffi.load()
    dev = where == "device"
    lab = np.array([0, 1, 2, 0, 1, 0], dtype=np.int32)
    hgt = np.array([-np.inf, 0.01, 0.02, -np.inf, 0.03, -np.inf])
    off = np.array([0, 3, 5, 5, 6], dtype=np.int64)       # four chunks, the third without points
    goff = np.array([0, 3, 5, 5, 6], dtype=np.int64)

    def call(lab=lab, hgt=hgt, thr=(0.015, 0.05), k=None, T_max=0.05):
        thr = np.array(thr, dtype=np.float64)
        k = thr.shape[0] if k is None else k
        n = lab.shape[0]
        out = np.full((max(k, 1), n), -7, dtype=np.int32)
        counts = np.full((max(k, 1), 4), -7, dtype=np.int32)
        if dev:
            d_lab, d_hgt, d_out = (torch.as_tensor(a, device="cuda:0") for a in (lab, hgt, out))
            torch.cuda.synchronize()
            ptr = [C.c_void_p(a.data_ptr()) for a in (d_lab, d_hgt, d_out)]
        else:
            ptr = [a.ctypes.data for a in (lab, hgt, out)]
        st = lib.ai_ncut_relabel(ctx._h, ptr[0], off.ctypes.data, 4, ptr[1], goff.ctypes.data, float(T_max), thr.ctypes.data, int(k),
                                 _ffi.AI_MEM_DEVICE if dev else _ffi.AI_MEM_HOST, ptr[2], counts.ctypes.data)
        return st, (d_out.cpu().numpy() if dev else out), counts

    def bad(a, i, v):
        b = a.copy()
        b[i] = v
        return b

    refused = [dict(thr=(0.015, np.nan)), dict(thr=(np.inf, 0.015)), dict(thr=(-np.inf,)), dict(thr=(0.015, np.nextafter(0.05, 1.0))),
               dict(hgt=bad(hgt, 3, 0.0)), dict(hgt=bad(hgt, 0, np.nan)), dict(lab=bad(lab, 4, 2)), dict(lab=bad(lab, 1, -1)),
               dict(lab=bad(lab, 5, 1)), dict(k=0), dict(k=-3)]
    for kw in refused:
        st, out, counts = call(**kw)
        assert st == -1, kw
        assert np.all(out == -7) and np.all(counts == -7), kw
        assert lib.ai_last_error().decode().startswith("ai_ncut_relabel")
        st, out, counts = call()       # the context is usable afterwards
        assert st == 0
        assert out.tolist() == [[0, 1, 1, 0, 0, 0], [0, 1, 2, 0, 1, 0]]
        assert counts.tolist() == [[2, 1, 0, 1], [3, 2, 0, 1]]


# ---------------------------------------------------------------------------------------------- test-only build, tool
def _child(args, env=None, timeout=300):
    r = subprocess.run([sys.executable] + args, env=dict(os.environ, **(env or {})), timeout=timeout, capture_output=True, text=True, cwd=ROOT)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    return r.stdout


@pytest.mark.parametrize("case", ["slots", "repeats", "lockstep"])
def test_tree_survives_the_hooks_of_the_test_only_build(case):
    """tests/tree_cases.py: children that wait for a slot and segments that are solved twice keep their heights (the tree of g5 equals
    the undisturbed one bit for bit); under AI_NCUT_LOCKSTEP=1 the tree entries return AI_ERR_BAD_ARG."""
    locklib = os.path.join(ROOT, "autoinst_amd", "libautoinst_hip_lockstep.so")
    assert os.path.exists(locklib), "libautoinst_hip_lockstep.so is not built (make -C autoinst_amd/csrc lockstep)"
    env = {"AUTOINST_HIP_LIB": locklib}
    if case == "lockstep":
        env["AI_NCUT_LOCKSTEP"] = "1"
    out = _child([os.path.join(ROOT, "tests", "tree_cases.py"), case], env)
    assert f"tree case {case}: ok" in out, out[-2000:]


def test_tsweep_tool_runs(tmp_path):
    """tools/run_tsweep.py at 2 chunks of 30 000 points: it asserts itself that the tree's labels equal 16 direct batched cuts."""
    line = tmp_path / "line.json"
    _child([os.path.join(ROOT, "tools", "run_tsweep.py"), "--chunks", "2", "--points", "30000", "--reps", "2", "--out", str(line)])
    r = json.loads(line.read_text())
    assert r["chunks"] == 2 and r["points"] == 30000 and r["k"] == 16 and r["labels_equal"] is True
    for key in ("tree_relabel_ms", "direct_sweep_ms", "single_cut_ms"):
        assert r[key] > 0.0
