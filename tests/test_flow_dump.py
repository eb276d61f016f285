"""tests/flow_dump.py on the CPU: the dump reader, the per-segment float64 reference and the tree audit accept records built from exact
dense eigenpairs, and reject records with one subtle defect each -- the bounds are tight enough to matter."""
import math
import os

import numpy as np
import pytest
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import flow_dump as fd

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


T = 0.5


def _graph(seed=0):
    """Three blobs (one of them far away: the root has 2 components), Gaussian affinity within radius 1, diagonal 1 like the
    library's affinity."""
    rng = np.random.default_rng(seed)
    pts = np.concatenate([rng.normal(0, 0.35, (130, 2)), rng.normal(0, 0.35, (120, 2)) + [1.4, 0.2],
                          rng.normal(0, 0.3, (90, 2)) + [9.0, 9.0]])
    d2 = ((pts[:, None, :] - pts[None, :, :]) ** 2).sum(-1)
    w = np.where(d2 <= 1.0, np.exp(-d2), 0.0)
    return sp.csr_matrix(w)


def _dense_M(w, ids):
    ws, d = fd.subgraph(w, ids)
    W = ws.toarray() + np.eye(len(ids))
    s = 1.0 / np.sqrt(d)
    return W, d, s[:, None] * W * s[None, :]


def _record(w, ids, T, ev=None, theta=None, rtrue=None):
    """An L record as the device would write it, from the exact dense eigenpair (or a given vector)."""
    W, d, M = _dense_M(w, ids)
    if ev is None:
        vals, vecs = np.linalg.eigh(M)
        theta, ev = vals[-2], 0.8 * vecs[:, -2]      # (raw vector: not of unit norm)
    a = np.abs(ev)
    top = np.flatnonzero(a == a.max())
    j = top[np.argmin(ids[top])]
    sc = (1.0 / math.sqrt(math.fsum(ev * ev))) * (1.0 if ev[j] > 0 else -1.0)
    e = ev * sc
    thr, flat = fd.thresholds(e)
    masks = e[None, :] > thr[:, None]
    costs = np.empty(fd.NUM_CUTS)
    for k, m in enumerate(masks):
        cut = W[np.ix_(m, ~m)].sum()
        costs[k] = cut / d[m].sum() + cut / d[~m].sum()
    ks = int(np.argmin(costs))
    r = float(np.linalg.norm(M @ ev - theta * ev) / np.linalg.norm(ev))
    return dict(kind="L", chunk=0, n=len(ids), m=len(ids) - 1, restarts=0, nosplit=int(flat), kstar=ks, split=int(costs[ks] < T),
                ntrue=int(masks[ks].sum()), theta=theta, resid=r, rtrue=r if rtrue is None else rtrue, scale=sc, mcut=costs[ks],
                thr=thr, costs=costs, ids=np.asarray(ids, np.int32), ev=ev)


def _recursion(w, T, n_orig):
    """The whole recursion of one chunk, segment by segment, as the library runs it: records and labels."""
    recs, leaves, todo = [], [], [np.random.default_rng(1).permutation(w.shape[0])]
    while todo:
        ids = todo.pop()
        ws, _ = fd.subgraph(w, ids)
        nc, comp = connected_components(ws, directed=False)
        if nc > 1:
            recs.append(dict(kind="C", chunk=0, n=len(ids), ids=np.asarray(ids, np.int32), comp=comp.astype(np.int32) * 7 + 3))
            parts = [ids[comp == k] for k in range(nc)]
        else:
            r = _record(w, ids, T)
            recs.append(r)
            if not r["split"]:
                leaves.append(ids)
                continue
            m = r["ev"] * r["scale"] > r["thr"][r["kstar"]]
            parts = [ids[m], ids[~m]]
        for p in parts:
            (todo if fd.eligible(len(p), n_orig, fd.SPLIT_LIM_CHILD) else leaves).append(p)
    lab = np.empty(w.shape[0], np.int64)
    for g, ids in enumerate(leaves):
        lab[ids] = g
    return recs, lab


@pytest.fixture(scope="module")
def tree():
    w = _graph()
    recs, lab = _recursion(w, T, w.shape[0])
    assert sum(r["kind"] == "C" for r in recs) >= 1 and sum(r["kind"] == "L" and r["split"] for r in recs) >= 1
    return w, recs, lab


def test_reader_round_trips_the_documented_layout(tree, tmp_path):
    _, recs, _ = tree
    path = tmp_path / "dump.bin"
    with open(path, "wb") as f:
        for r in recs:
            fd.write_record(f, r)
    # the header by hand, once: 9 int64 + 25 double, little-endian
    raw = open(path, "rb").read()
    assert int.from_bytes(raw[0:8], "little") == ord(recs[0]["kind"]) and int.from_bytes(raw[16:24], "little") == recs[0]["n"]
    back = fd.read_dump(str(path))
    assert len(back) == len(recs)
    for a, b in zip(back, recs):
        assert a["kind"] == b["kind"] and a["n"] == b["n"] and np.array_equal(a["ids"], b["ids"])
        if a["kind"] == "L":
            assert np.array_equal(a["ev"], b["ev"]) and np.array_equal(a["costs"], b["costs"]) and np.array_equal(a["thr"], b["thr"])
            assert a["theta"] == b["theta"] and a["kstar"] == b["kstar"] and a["scale"] == b["scale"]
        else:
            assert np.array_equal(a["comp"], b["comp"])


def test_checker_accepts_exact_records(tree):
    w, recs, lab = tree
    s = fd.check_call(recs, [w], [w.shape[0]], [lab], 0.01, T)
    assert s["lanczos"] >= 4 and s["components"] >= 1 and s["eig_checked"] == s["lanczos"]
    assert s["cost_rel"] <= 1e-13 and s["near_ties"] == 0 and s["dk_ratio"] < 1.0


def _split_rec(tree):
    w, recs, _ = tree
    return w, next(r for r in recs if r["kind"] == "L" and r["split"] and r["n"] > 200)


def test_rejects_ge_instead_of_gt_in_the_bin_rule(tree):
    w, r = _split_rec(tree)
    W, d, _ = _dense_M(w, r["ids"])
    e = r["ev"] * r["scale"]
    bad = dict(r, costs=r["costs"].copy())
    for k in range(fd.NUM_CUTS):
        m = e >= r["thr"][k]
        cut = W[np.ix_(m, ~m)].sum()
        with np.errstate(divide="ignore", invalid="ignore"):
            bad["costs"][k] = cut / d[m].sum() + cut / d[~m].sum()
    with pytest.raises(AssertionError, match="costs"):
        fd.check_lanczos(bad, w, T)


def test_rejects_one_cost_off_by_1e9(tree):
    w, r = _split_rec(tree)
    bad = dict(r, costs=r["costs"].copy())
    bad["costs"][(r["kstar"] + 3) % fd.NUM_CUTS] *= 1.0 + 1e-9
    with pytest.raises(AssertionError, match="costs"):
        fd.check_lanczos(bad, w, T)


def test_rejects_a_stripe_dropped_from_a_volume(tree):
    """fk_sweep_final sums the fine tasks' partials (32 rows each) in 6 stripes; one stripe lost from vol(A)."""
    w, r = _split_rec(tree)
    W, d, _ = _dense_M(w, r["ids"])
    e = r["ev"] * r["scale"]
    stripe0 = (np.arange(r["n"]) // 32) % 6 == 0
    bad = dict(r, costs=r["costs"].copy())
    for k in range(fd.NUM_CUTS):
        m = e > r["thr"][k]
        cut = W[np.ix_(m, ~m)].sum()
        bad["costs"][k] = cut / d[m & ~stripe0].sum() + cut / d[~m].sum()
    with pytest.raises(AssertionError, match="costs"):
        fd.check_lanczos(bad, w, T)


def test_rejects_a_threshold_off_by_one_ulp(tree):
    w, r = _split_rec(tree)
    bad = dict(r, thr=r["thr"].copy())
    bad["thr"][4] = np.nextafter(bad["thr"][4], np.inf)
    with pytest.raises(AssertionError, match="thresholds"):
        fd.check_lanczos(bad, w, T)


def test_rejects_a_vector_rotated_past_the_davis_kahan_bound(tree):
    """The vector turned towards the third eigenvector by 1e-6 rad, everything derived from it consistent, the residual as dumped:
    only the angle can tell."""
    w, r = _split_rec(tree)
    _, _, M = _dense_M(w, r["ids"])
    vals, vecs = np.linalg.eigh(M)
    phi = 1e-6
    ev = np.cos(phi) * vecs[:, -2] + np.sin(phi) * vecs[:, -3]
    bad = _record(w, r["ids"], T, ev=ev, theta=vals[-2], rtrue=r["rtrue"])
    with pytest.raises(AssertionError, match="Davis-Kahan"):
        fd.check_lanczos(bad, w, T)


def test_rejects_a_wrong_sign(tree):
    w, r = _split_rec(tree)
    with pytest.raises(AssertionError, match="sign"):
        fd.check_lanczos(dict(r, scale=-r["scale"]), w, T)


def test_rejects_a_child_that_is_not_a_mask_side(tree):
    """One row moved from a split's first child to its second: both are still connected segments, but neither is a mask side."""
    w, recs, lab = tree
    r = _split_rec(tree)[1]
    m = r["ev"] * r["scale"] > r["thr"][r["kstar"]]
    sa, sb = set(r["ids"][m].tolist()), set(r["ids"][~m].tolist())
    ia = next(i for i, q in enumerate(recs) if set(q["ids"].tolist()) == sa)
    ib = next(i for i, q in enumerate(recs) if set(q["ids"].tolist()) == sb)
    bad = list(recs)
    mv = recs[ia]["ids"][0]
    bad[ia] = dict(recs[ia], ids=recs[ia]["ids"][1:], n=recs[ia]["n"] - 1)
    bad[ib] = dict(recs[ib], ids=np.append(recs[ib]["ids"], mv), n=recs[ib]["n"] + 1)
    with pytest.raises(AssertionError, match="never dumped"):
        fd.audit_tree(bad, [w.shape[0]], [w.shape[0]], [lab], 0.01, T)


def test_rejects_wrong_component_labels(tree):
    w, recs, _ = tree
    r = next(q for q in recs if q["kind"] == "C")
    comp = r["comp"].copy()
    comp[0] = comp[-1] if comp[-1] != comp[0] else comp[0] + 1
    with pytest.raises(AssertionError, match="component"):
        fd.check_components(dict(r, comp=comp), w)


def test_dump_hook_exists_in_the_test_only_build_alone():
    """AI_FLOW_DUMP is compiled into libautoinst_hip_lockstep.so (-DAI_TEST_HOOKS) and nowhere into the shipped library."""
    lib = os.path.join(ROOT, "autoinst_amd", "libautoinst_hip.so")
    lock = os.path.join(ROOT, "autoinst_amd", "libautoinst_hip_lockstep.so")
    if not (os.path.exists(lib) and os.path.exists(lock)):
        pytest.skip("libraries not built")
    assert b"AI_FLOW_DUMP" not in open(lib, "rb").read()
    assert b"AI_FLOW_DUMP" in open(lock, "rb").read()
