"""Hand-made chunks for tests/test_gpu_root_start.py (the smallest shapes at which the principal-axis start of an ancestor-less segment
can go wrong), and the one case of that file that needs the fault-injection hook of the TEST-ONLY build: run as a child process with
AUTOINST_HIP_LIB pointing at libautoinst_hip_lockstep.so.

    python tests/root_start_cases.py restart
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

COARSE_ROWS = 512   # AI_COARSE_ROWS (csrc/ai_ncut_params.h): rows of one coarse task


def _box(rng, n, lo, size):
    return np.asarray(lo, dtype=np.float64) + rng.random((n, 3)) * np.asarray(size, dtype=np.float64)


def small_chunks():
    """name -> points (float64, n x 3).  Components lie more than the graph's radius (1 m) apart."""
    rng = np.random.default_rng(7)
    body = _box(rng, 2500, (0.0, 0.0, 0.0), (12.0, 3.0, 1.0))
    out = {}
    # a component below one coarse task, and one of exactly one coarse task plus one row, beside a body of several tasks
    out["below_one_task"] = np.concatenate([body, _box(rng, 300, (0.0, 6.0, 0.0), (5.0, 1.0, 0.5))])
    out["one_task_plus_one"] = np.concatenate([body, _box(rng, COARSE_ROWS + 1, (0.0, 6.0, 0.0), (7.0, 1.0, 0.5))])
    # rank-1 covariance: every point on one line (not an axis of the frame)
    s = np.cumsum(rng.uniform(0.02, 0.08, 2000))
    out["line"] = np.outer(s, np.array([0.6, 0.0, 0.8])) + np.array([1.0, 2.0, 3.0])
    # rank-2 covariance: a jittered grid in the plane z = 0.5
    u, v = np.meshgrid(np.arange(80) * 0.12, np.arange(30) * 0.12, indexing="ij")
    out["plane"] = np.stack([u.ravel() + rng.random(u.size) * 0.1, v.ravel() + rng.random(u.size) * 0.1, np.full(u.size, 0.5)], 1)
    # a component of ONE point repeated 600 times (sigma = 0: it keeps the hash start) beside the body, and that component alone
    dup = np.tile(np.array([[3.0, 8.0, 0.25]]), (600, 1))
    out["duplicates_and_body"] = np.concatenate([dup, body])
    out["duplicates_alone"] = dup
    return out


def restart():
    """AI_FLOW_INJECT=0 spoils the Ritz pair of the FIRST harvested segment of the call -- nothing is solved before it, so it has no solved
    ancestor and started from its principal-axis vector: it is solved again from the same vector and the labels are the undisturbed call's."""
    from autoinst_amd import ncuts_api as api, synth
    ch = synth.synthetic_chunk(20000, 3, tarl=True)
    g = api.build_affinity(ch["points"], ch["tarl"], alpha=1.0, theta=0.5, gamma=0.0)
    lab0, ng0, st0 = api.ncuts_labels(g, g.n, 0.03)
    assert st0["restarted_solves"] == 0 and st0["unconverged"] == 0
    os.environ["AI_FLOW_INJECT"] = "0"
    try:
        lab, ng, st = api.ncuts_labels(g, g.n, 0.03)
    finally:
        os.environ.pop("AI_FLOW_INJECT", None)
    assert st["restarted_solves"] == 1, st
    assert ng == ng0 and np.array_equal(lab, lab0)
    assert st["lanczos_solves"] == st0["lanczos_solves"] and st["unconverged"] == 0
    assert st["max_true_resid"] <= 2e-10
    g.free()


if __name__ == "__main__":
    {"restart": restart}[sys.argv[1]]()
    print(f"root start case {sys.argv[1]}: ok")
