"""Cases of the cut-tree suite that need the hooks of the TEST-ONLY build (libautoinst_hip_lockstep.so, -DAI_TEST_HOOKS): run as a
child process by tests/test_gpu_tree.py with AUTOINST_HIP_LIB pointing at that build.

    python tests/tree_cases.py slots | repeats | lockstep

The tree is recorded by the host side of the frontier, on paths the hooks reroute: a child that waits for a Lanczos slot comes back
as a root of a later wave (AI_FLOW_SMAX), a segment whose Ritz pair is rejected is solved again (AI_FLOW_TRUE_LIMIT).  Both must
carry the heights they inherited: the tree of g5 equals the undisturbed one bit for bit.
"""
import os
import re
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)
from autoinst_amd import ncuts_api as api  # noqa: E402
from hook_cases import _Env, _capture_stderr  # noqa: E402
import tree_ref  # noqa: E402

T_MAX = 0.3


def _same(a, b):
    assert a.n_groups == b.n_groups and np.array_equal(a.labels, b.labels)
    assert np.array_equal(a.cut_height.view(np.int64), b.cut_height.view(np.int64))
    assert np.array_equal(a.leaf_cost.view(np.int64), b.leaf_cost.view(np.int64))


def _g5():
    A = tree_ref.load_graph("g5_surface3k_T003")
    g = api.DeviceGraph.from_scipy(A)
    t0 = api.ncuts_tree(g, g.n, T_MAX)
    st0 = api.last_stats()
    assert st0["unconverged"] == 0 and st0["restarted_solves"] == 0 and t0.n_groups > 20
    return g, t0, st0


def slots():
    g, t0, _ = _g5()
    with _Env(AI_FLOW_SMAX=16, AI_NCUT_PHASES=1):
        t1, err = _capture_stderr(lambda: api.ncuts_tree(g, g.n, T_MAX))
    waited = int(re.search(r"children that waited for a slot (\d+)", err).group(1))
    assert waited > 0, err
    _same(t1, t0)
    g.free()


def repeats():
    g, t0, st0 = _g5()
    with _Env(AI_FLOW_TRUE_LIMIT="1e-300"):
        t1 = api.ncuts_tree(g, g.n, T_MAX)
    st1 = api.last_stats()
    assert st1["restarted_solves"] >= 0.9 * st0["lanczos_solves"] - 2 and st1["lanczos_solves"] == st0["lanczos_solves"], (st1, st0)
    _same(t1, t0)
    g.free()


def lockstep():
    """AI_NCUT_LOCKSTEP=1 (read once per process): the level-synchronous driver records no tree, the tree entries refuse."""
    assert os.environ.get("AI_NCUT_LOCKSTEP") == "1"
    A = tree_ref.load_graph("g1_blob_pair_spatial")
    g = api.DeviceGraph.from_scipy(A)
    lab, ng, _ = api.ncuts_labels(g, g.n, 0.5)          # the plain cut runs on that driver
    assert ng > 1
    for call in (lambda: api.ncuts_tree(g, g.n, 0.5), lambda: api.ncuts_tree_batch([g, g], None, 0.5)):
        try:
            call()
        except ValueError as e:
            assert "cut tree" in str(e)
        else:
            raise AssertionError("the tree entry did not refuse")
    lab2, ng2, _ = api.ncuts_labels(g, g.n, 0.5)         # the context is usable afterwards
    assert ng2 == ng and np.array_equal(lab2, lab)
    g.free()


if __name__ == "__main__":
    case = sys.argv[1]
    {"slots": slots, "repeats": repeats, "lockstep": lockstep}[case]()
    print(f"tree case {case}: ok")
