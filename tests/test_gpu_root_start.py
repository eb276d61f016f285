"""The principal-axis start of ancestor-less segments (fk_pca_moments / fk_pca_axis / fk_pca_fill, csrc/ai_flow_kernels.inc).

A segment without a solved ancestor whose graph kept its points (build_affinity) starts its Lanczos solve from u1 * (coordinate along
the principal axis of its own points) instead of the hash vector.  Another start vector, the same eigenvector: every label is the
hash start's (AI_FLOW_WARM=0, read per call), with fewer rows x steps.  The bound on rows x steps comes from the CPU study
(tests/tools/root_start_study.py -> profiles/root_start_study.jsonl) on the same fixtures.
"""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

from oracle import ncuts_ref
from root_start_cases import small_chunks

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

FIXTURES = [(20000, 3, "tarl", 0.03), (20000, 2, "tri", 0.005), (30000, 21, "tarl", 0.03)]
BATCH = (0, 2)   # the two fixtures that share T = 0.03 are also cut in one batched call

# spmv_rows of the PARENT library (the commit before the principal-axis start) for the 20k tarl seed-3 graph exported with to_scipy() and
# re-imported with DeviceGraph.from_scipy (no coordinates): measured once with that library on an MI355X
PARENT_SPMV_ROWS_REIMPORTED_20K_TARL_3 = 5143668


@pytest.fixture(scope="module")
def api():
    from autoinst_amd import ncuts_api
    ncuts_api.default_context()
    return ncuts_api


class _HashStart:
    def __enter__(self):
        os.environ["AI_FLOW_WARM"] = "0"

    def __exit__(self, *a):
        os.environ.pop("AI_FLOW_WARM", None)


@pytest.fixture(scope="module")
def cut(api):
    """The three fixtures and the batch of two, cut with the default start and with the hash start, once for the module."""
    from autoinst_amd import synth
    graphs = []
    for n, seed, mode, T in FIXTURES:
        ch = synth.synthetic_chunk(n, seed, tarl=True, dino=mode == "tri")
        graphs.append(api.build_affinity(ch["points"], ch["tarl"], ch["dino"] if mode == "tri" else None, alpha=1.0, theta=0.5,
                                         gamma=0.1 if mode == "tri" else 0.0))
    new = [api.ncuts_labels(g, g.n, f[3]) for g, f in zip(graphs, FIXTURES)]
    new_b = api.ncuts_labels_batch([graphs[i] for i in BATCH], None, 0.03)
    with _HashStart():
        old = [api.ncuts_labels(g, g.n, f[3]) for g, f in zip(graphs, FIXTURES)]
        old_b = api.ncuts_labels_batch([graphs[i] for i in BATCH], None, 0.03)
    yield {"graphs": graphs, "new": new, "new_b": new_b, "old": old, "old_b": old_b}
    for g in graphs:
        g.free()


def _study_row_steps():
    """rows x steps of the CPU model per fixture: {(n, mode, seed): (hash start, principal-axis start)}."""
    out = {}
    with open(os.path.join(ROOT, "profiles", "root_start_study.jsonl")) as f:
        for line in f:
            d = json.loads(line)
            out[(d["n"], d["mode"], d["seed"])] = (d["hash"]["row_steps"], d["root_start"]["row_steps"])
    return out


@pytest.mark.gpu
def test_labels_and_stats_against_the_hash_start(cut):
    """Labels, group counts and solve counts equal the hash start's on every fixture and in the batch; every pair that is cut has a
    true residual <= 2e-10 both ways; rows x steps summed over the fixtures and the batch are below the hash start's by the CPU
    study's ratio on the same fixtures plus 0.02 (the check schedule lands a few steps past the model's every-step test).
    Measured on an MI355X: 50 357 100 against 58 342 828, ratio 0.8631; the CPU study gives 0.8676 (profiles/root_start_ab.txt)."""
    rows_new = rows_old = 0
    for (lab1, ng1, st1), (lab0, ng0, st0) in zip(cut["new"], cut["old"]):
        assert ng1 == ng0 and np.array_equal(lab1, lab0)
        assert st1["lanczos_solves"] == st0["lanczos_solves"]
        assert st1["unconverged"] == 0 and st0["unconverged"] == 0
        assert st1["max_true_resid"] <= 2e-10 and st0["max_true_resid"] <= 2e-10
        rows_new += st1["spmv_rows"]
        rows_old += st0["spmv_rows"]
    (labs1, ngs1, stb1), (labs0, ngs0, stb0) = cut["new_b"], cut["old_b"]
    assert ngs1 == ngs0 and all(np.array_equal(a, b) for a, b in zip(labs1, labs0))
    assert stb1["lanczos_solves"] == stb0["lanczos_solves"] and stb1["unconverged"] == 0 and stb0["unconverged"] == 0
    assert stb1["max_true_resid"] <= 2e-10 and stb0["max_true_resid"] <= 2e-10
    rows_new += stb1["spmv_rows"]
    rows_old += stb0["spmv_rows"]
    study = _study_row_steps()
    keys = [(n, mode, seed) for n, seed, mode, _ in FIXTURES]
    keys += [keys[i] for i in BATCH]
    model = sum(study[k][1] for k in keys) / sum(study[k][0] for k in keys)
    print(f"rows x steps: principal-axis start {rows_new}, hash start {rows_old}, ratio {rows_new / rows_old:.4f}; CPU study {model:.4f}")
    assert rows_new < (model + 0.02) * rows_old, (rows_new, rows_old, rows_new / rows_old, model)


@pytest.mark.gpu
def test_a_chunk_cut_in_a_batch_equals_the_chunk_cut_alone(api):
    """The moment sums depend on a segment's own rows and tasks only: three chunks cut alone and as one batch give identical labels and
    group counts, and two repeats of the batch the same rows x steps."""
    from autoinst_amd import synth
    chunks = [synth.synthetic_chunk(n, 40 + i, tarl=False) for i, n in enumerate((9000, 14000, 5000))]
    gs = [api.build_affinity(c["points"], None, alpha=1.0, theta=0.0, gamma=0.0) for c in chunks]
    alone = [api.ncuts_labels(g, g.n, 0.05) for g in gs]
    labs1, ngs1, st1 = api.ncuts_labels_batch(gs, None, 0.05)
    labs2, ngs2, st2 = api.ncuts_labels_batch(gs, None, 0.05)
    for g in gs:
        g.free()
    for (lab, ng, _), l1, n1, l2, n2 in zip(alone, labs1, ngs1, labs2, ngs2):
        assert ng == n1 == n2 and np.array_equal(lab, l1) and np.array_equal(lab, l2)
    assert st1["spmv_rows"] == st2["spmv_rows"]
    assert st1["unconverged"] == 0


@pytest.mark.gpu
def test_a_graph_without_coordinates_is_cut_as_before(api, cut):
    """A graph made any other way than by build_affinity has no points: exported with to_scipy() and re-imported with from_scipy, the 20k
    tarl fixture gives the same partition, and exactly the rows x steps the parent library reports for that re-imported graph."""
    g = cut["graphs"][0]
    g2 = api.DeviceGraph.from_scipy(g.to_scipy())
    lab2, ng2, st2 = api.ncuts_labels(g2, g2.n, 0.03)
    g2.free()
    lab, ng, _ = cut["new"][0]
    assert ng2 == ng and ncuts_ref.partitions_equal(lab2, lab)
    assert st2["unconverged"] == 0
    print(f"spmv_rows of the re-imported graph: {st2['spmv_rows']}")
    assert st2["spmv_rows"] == PARENT_SPMV_ROWS_REIMPORTED_20K_TARL_3


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(small_chunks()))
def test_smallest_shapes(api, name):
    """A component below one coarse task, one of a coarse task plus one row, points on a line (rank-1 covariance), points in a plane,
    a component of one point repeated (sigma = 0: it keeps the hash start): the labels are the hash start's."""
    pts = small_chunks()[name]
    g = api.build_affinity(pts, None, alpha=1.0, theta=0.0, gamma=0.0)
    lab1, ng1, st1 = api.ncuts_labels(g, g.n, 0.075)
    with _HashStart():
        lab0, ng0, st0 = api.ncuts_labels(g, g.n, 0.075)
    g.free()
    assert ng1 == ng0 and np.array_equal(lab1, lab0)
    assert st1["lanczos_solves"] == st0["lanczos_solves"] and st1["unconverged"] == 0 and st0["unconverged"] == 0
    if name == "duplicates_alone":   # the fall-back is the hash start itself: the same steps, not only the same labels
        assert st1["spmv_rows"] == st0["spmv_rows"] and st1["lanczos_steps"] == st0["lanczos_steps"]
    else:
        assert st1["spmv_rows"] != st0["spmv_rows"]   # (the other chunks do start from another vector)


@pytest.mark.gpu
def test_a_spoiled_pair_of_an_ancestor_less_segment_is_solved_again_from_the_same_vector():
    """The true-residual test sends a segment back; an ancestor-less one gets its principal-axis vector again (recomputed from the same
    sums), so the labels are the undisturbed call's and restarted_solves == 1.  AI_FLOW_INJECT exists in the test-only build alone:
    tests/root_start_cases.py `restart` runs in a child process that loads it."""
    locklib = os.path.join(ROOT, "autoinst_amd", "libautoinst_hip_lockstep.so")
    assert os.path.exists(locklib), "libautoinst_hip_lockstep.so is not built (make -C autoinst_amd/csrc lockstep)"
    env = dict(os.environ, AUTOINST_HIP_LIB=locklib)
    r = subprocess.run([sys.executable, os.path.join(ROOT, "tests", "root_start_cases.py"), "restart"], env=env, timeout=300, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert "root start case restart: ok" in r.stdout, r.stdout[-2000:]
