"""GPU suite (-m gpu): every cut of the shipped NCut path (ncut_flow, the fk_* kernels) against a float64 reference, segment by segment.

A child process runs the calls with the test-only build (libautoinst_hip_lockstep.so) and AI_FLOW_DUMP set (tests/flow_cases.py);
here each dumped segment is checked on its own subgraph by tests/flow_dump.py: scale and sign, thresholds bit for bit, the 10 costs
to rel 1e-11 against fsum, the decision, the eigenpair against eigsh with a Davis-Kahan bound on the vector, and the recursion tree
against the call's labels."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

from conftest import GOLDEN, golden_names
import flow_dump as fd

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CONNECTED = ["g1_blob_pair_spatial", "g6_connected_tarl", "g6_connected_spatial"]
FIXTURES = ["goldens", "c1_10k_tarl", "c1_10k_spatial", "headline", "dense", "band", "band128", "band128_diag", "stride", "stride_diag"]


@pytest.fixture(scope="module")
def dumps(tmp_path_factory):
    locklib = os.path.join(ROOT, "autoinst_amd", "libautoinst_hip_lockstep.so")
    if not os.path.exists(locklib):
        pytest.skip("libautoinst_hip_lockstep.so is not built (make -C autoinst_amd/csrc lockstep)")
    out = str(tmp_path_factory.mktemp("flow_dump"))
    env = dict(os.environ, AUTOINST_HIP_LIB=locklib)
    env.pop("AI_FLOW_DUMP", None)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "flow_cases.py"), out], env=env, timeout=900, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "flow cases: ok" in r.stdout, r.stdout[-2000:]
    return out


def load(out, name):
    z = np.load(os.path.join(out, name + ".npz"))
    k = int(z["k"])
    graphs, labels = [], []
    for i in range(k):
        ip = z[f"indptr{i}"]
        graphs.append(sp.csr_matrix((z[f"data{i}"], z[f"indices{i}"], ip), shape=(len(ip) - 1, len(ip) - 1)))
        labels.append(z[f"labels{i}"])
    return fd.read_dump(os.path.join(out, name + ".bin")), graphs, labels, z


def _check(out, name):
    recs, graphs, labels, z = load(out, name)
    s = fd.check_call(recs, graphs, [int(x) for x in z["n_orig"]], labels, float(z["split_lim"]), float(z["T"]),
                      accepted_above_limit=int(z["accepted_above_limit"]))
    print(f"[flow values] {name}: {s['records']} records ({s['lanczos']} Lanczos, {s['components']} component splits, "
          f"{s['eig_checked']} with eigsh); max rel cost error {s['cost_rel']:.2e}; max rel lambda2 error {s['lam_err']:.2e}; "
          f"max sin/bound {s['dk_ratio']:.2e}; near-ties {s['near_ties']}; above the limit {s['above_limit']}")
    return s


@pytest.mark.parametrize("fixture", FIXTURES)
def test_every_segment_matches_the_float64_reference(dumps, fixture):
    """Every dumped segment of the fixture against `flow_dump.check_call`, without near-ties.

    `band` and `band128` are the fixtures that found the cancelling start norm (fk_lz_project): their blocks are
    cut off along weak bridges, so a child's warm vector is all but parallel to its u1.  Before that kernel the 31-row block of `band`
    ended at m = n - 1 with a true residual of 1.87e-06 and the 512-row block of `band128` at 1.28e-08 behind an estimate of 2.8e-12;
    now the largest true residual of the two calls is 5.7e-11."""
    names = golden_names() if fixture == "goldens" else [fixture]
    for name in names:
        s = _check(dumps, name)
        assert s["lanczos"] >= 1 and s["near_ties"] == 0
    if fixture == "headline":
        assert s["lanczos"] >= 40 and s["eig_checked"] >= 30
    if fixture in ("c1_10k_tarl", "c1_10k_spatial"):
        assert s["components"] >= 1   # a disconnected root, then Lanczos children
    if fixture == "band":
        # the segments the CPU check of the fixture lists (tests/test_csr_cases.py): on both sides of 32, 64 and 512 rows
        recs = load(dumps, "band")[0]
        assert {31, 32, 33, 64, 65, 511, 512, 513, 1764} <= {r["n"] for r in recs} and s["components"] == 0
        ms = [r["m"] for r in recs]
        assert min(ms) < 32 and any(32 < m < 64 for m in ms) and max(ms) > 64
    if fixture == "dense":
        d = np.diff(load(dumps, "dense")[1][0].indptr)
        assert d.max() > 400 and (d > 64).sum() > 500


@pytest.mark.parametrize("name", CONNECTED)
def test_root_of_a_connected_golden_matches_the_imported_reference(dumps, name):
    """The root segment's numbers against what the reference itself computed (the golden): lambda2, |fiedler|, the mask, mcut and
    the 10 costs."""
    recs, graphs, labels, _ = load(dumps, name)
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = graphs[0].shape[0]
    root = [r for r in recs if r["n"] == n]
    assert len(root) == 1 and root[0]["kind"] == "L"
    r = root[0]
    o = np.argsort(r["ids"])          # back to original order
    e = (r["ev"] * r["scale"])[o]
    thr = r["thr"]
    # the golden's own vector keeps clear of every one of its thresholds, so that its masks and the device's are comparable (the
    # minimum itself IS threshold 0: the strict > puts it on the same side in both)
    fz = z["fiedler"] * np.sign(z["fiedler"][np.argmax(np.abs(z["fiedler"]))])
    dist = np.abs(fz[:, None] - np.linspace(fz.min(), fz.max(), 10, endpoint=False)[None, :])
    dist[np.argmin(fz), 0] = np.inf
    assert dist.min() >= 1e-6
    assert 1.0 - r["theta"] == pytest.approx(float(z["eigvals"][1]), rel=1e-8)
    assert np.abs(np.abs(e) - z["fiedler_abs"]).max() <= 1e-7
    if z["fiedler"][np.argmax(np.abs(z["fiedler"]))] < 0:
        # eigsh returned the other sign: the reference's mask, mcut and costs are those of -e, not comparable to the device's (whose
        # own costs tests/flow_dump.py checks against the float64 reference above)
        return
    assert np.array_equal(e > thr[r["kstar"]], z["top_mask"])
    assert r["mcut"] == pytest.approx(float(z["top_mcut"]), rel=1e-10)
    ref = z["costs"]
    big = np.abs(ref) > 1e-9
    assert np.allclose(r["costs"][big], ref[big], rtol=1e-10, atol=0)
    assert np.abs(r["costs"][~big] - ref[~big]).max(initial=0.0) <= 1e-9


@pytest.mark.parametrize("name", CONNECTED)
def test_the_solver_sweeps_the_root_vector_of_the_frontier_to_the_same_bits(dumps, name):
    """The contract of csrc/ai_ncut_shared.h across the two solvers: the level-synchronous Solver (ai_sweep: k_minmax .. k_sweep_final)
    given the frontier's own root vector ev * scale forms the frontier's ten costs, its mcut and its mask (fk_minmax ..
    fk_sweep_final) bit for bit.  The root's rows are in caller order in both, so tasks and stripes hold the same rows."""
    import flow_cases
    from autoinst_amd import ncuts_api as api
    recs = load(dumps, name)[0]
    graphs = flow_cases.build(name)[0]
    n = graphs[0].n
    root = [r for r in recs if r["n"] == n]
    assert len(root) == 1 and root[0]["kind"] == "L" and not root[0]["nosplit"]
    r = root[0]
    o = np.argsort(r["ids"])          # back to original order
    e = (r["ev"] * r["scale"])[o]
    costs, mask, mcut = api.sweep(graphs[0], e)
    graphs[0].free()
    assert costs.tobytes() == r["costs"].tobytes(), (costs, r["costs"])
    assert np.float64(mcut).tobytes() == np.float64(r["mcut"]).tobytes()
    assert np.array_equal(mask, e > r["thr"][r["kstar"]])     # bin > kstar: the thresholds strictly below e number more than kstar


def test_batch_equals_solo_bit_for_bit_per_segment(dumps):
    """ai_ncut_batch promises the results of separate ai_ncut calls: per segment m, theta, ev, scale, thr, costs and kstar are
    byte-equal to the solo call's, in one pool and with a window that serialises admission."""
    solo = []
    for i in range(3):
        recs, _, labels, _ = load(dumps, f"solo{i}")
        solo.append(({tuple(np.sort(r["ids"])): r for r in recs}, labels[0]))
    for name in ("batch", "batch_window"):
        recs, graphs, labels, _ = load(dumps, name)
        seen = [0, 0, 0]
        for r in recs:
            c = r["chunk"]
            key = tuple(np.sort(r["ids"]))
            assert key in solo[c][0], f"{name}: a segment of chunk {c} ({r['n']} rows) that its solo call does not have"
            q = solo[c][0][key]
            seen[c] += 1
            assert q["kind"] == r["kind"] and np.array_equal(q["ids"], r["ids"])
            if r["kind"] == "C":
                continue
            for f in ("m", "kstar", "nosplit", "split", "ntrue"):
                assert q[f] == r[f], (name, c, r["n"], f, q[f], r[f])
            for f in ("theta", "scale", "mcut", "rtrue"):
                assert np.float64(q[f]).tobytes() == np.float64(r[f]).tobytes(), (name, c, r["n"], f, q[f], r[f])
            for f in ("ev", "thr", "costs"):
                assert q[f].tobytes() == r[f].tobytes(), (name, c, r["n"], f)
        assert seen == [len(s[0]) for s in solo], (name, seen)
        for c in range(3):
            assert np.array_equal(labels[c], solo[c][1])


def test_labels_unchanged_and_the_shipped_library_writes_no_dump(dumps, tmp_path, monkeypatch):
    """The dump changes nothing: the shipped library gives the same labels for the same graphs, and with AI_FLOW_DUMP set it writes
    no file (the hook is not compiled into it)."""
    import flow_cases
    from autoinst_amd import ncuts_api as api
    api.default_context()
    path = str(tmp_path / "never.bin")
    monkeypatch.setenv("AI_FLOW_DUMP", path)
    for case in flow_cases.CASES:
        graphs, n_orig, T, split_lim = flow_cases.build(case)
        lab, _, _ = api.ncuts_labels(graphs[0], n_orig[0], T, split_lim)
        assert np.array_equal(lab, load(dumps, case)[2][0]), case
        for g in graphs:
            g.free()
    graphs, n_orig, T, split_lim = flow_cases.build_batch()
    labs, _, _ = api.ncuts_labels_batch(graphs, n_orig, T, split_lim)
    for c, lab in enumerate(labs):
        assert np.array_equal(lab, load(dumps, "batch")[2][c])
    for g in graphs:
        g.free()
    assert not os.path.exists(path)
