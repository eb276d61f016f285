"""GPU: ``ai_eigs_smallest`` against the dense float64 spectrum on every solver path (fixtures: tests/eig_cases.py).

Every (case, k) runs at the default tolerance and `eig_cases.check_eigs` compares it with ``numpy.linalg.eigh`` of
``ncuts_ref.laplacian_sym(w)``: exact zero pairs on distinct components, true residuals, orthonormality, the eigenvalue
SET, and every eigenspace inside the first k spanned.  The branches: Lanczos (one pair per component), the dense host
solve (components of <= 256 rows), ChFSI with blocks of 64 and 128 (grouped and plain SpMM, float32 and float64 filter).
The solver switches are read once per process, so the block cases run again in child processes with them set."""
import os
import subprocess
import sys

import numpy as np
import pytest

import eig_cases as ec

pytestmark = pytest.mark.gpu

FAMILIES = ["ring", "torus", "complete", "star", "twin", "bridge", "surface", "mixture", "variant"]
_REFS: dict = {}


@pytest.fixture(scope="module")
def api():
    from autoinst_amd import ncuts_api
    ncuts_api.default_context()
    return ncuts_api


@pytest.fixture(scope="module")
def all_cases():
    return {c.name: c for c in ec.cases() + ec.variants()}


def _ref(c):
    if c.name not in _REFS:
        _REFS[c.name] = ec.reference(c.w)
    return _REFS[c.name]


def _run(api, c, ks, **kw):
    """(failures, per-pair measurements) of every k of case c."""
    fails, got = [], []
    g = api.DeviceGraph.from_scipy(c.w)
    try:
        for k in ks:
            try:
                evals, V, steps, resid = api.eigs_smallest(g, k, **kw)
                m = ec.check_eigs(c.w, k, evals, V, resid, ref=_ref(c))
                got.append((c.name, k, m))
            except Exception as e:  # every pair is reported, not only the first failure
                fails.append(f"{c.name} k={k} {sorted(ec.branches(c.w, k))}: {type(e).__name__}: {e}")
    finally:
        g.free()
    return fails, got


@pytest.mark.parametrize("family", FAMILIES)
def test_family_matches_dense_eigh(api, all_cases, family):
    cs = [c for c in all_cases.values() if c.family == family]
    assert cs
    fails, got = [], []
    for c in cs:
        f, m = _run(api, c, c.ks)
        fails += f
        got += m
    if got:
        e = max(m["eig_err"] for _, _, m in got)
        r = max(m["resid"] for _, _, m in got)
        s = max(m["sin_frac"] for _, _, m in got)
        print(f"\n[eigs {family}] {len(got)} pairs: largest eigenvalue error {e:.3e}, true residual {r:.3e}, sin theta / bound {s:.3e}")
    assert not fails, "\n".join(fails)


@pytest.mark.parametrize("name,k", [("torus16x16", 9), ("ring200", 2), ("surface1023_tarl", 8), ("surface1023_tarl", 63),
                                    ("mixture", 20), ("torus33x34_shuffled", 5)])
def test_second_call_is_bit_identical(api, all_cases, name, k):
    c = all_cases[name]
    g = api.DeviceGraph.from_scipy(c.w)
    a = api.eigs_smallest(g, k)
    b = api.eigs_smallest(g, k)
    g.free()
    assert np.array_equal(a[0], b[0]) and np.array_equal(a[1], b[1]) and a[2:] == b[2:]


@pytest.mark.parametrize("name,ks", [("surface1023_tarl", (3, 34)), ("mixture", (3, 20, 64)), ("star40", (40,))])
def test_row_permutation_passes_the_same_checks(api, all_cases, name, ks):
    c = ec.variant(all_cases[name], "perm", seed=23)
    fails, _ = _run(api, c, ks)
    assert not fails, "\n".join(fails)


def test_lanczos_without_convergence_raises(api, all_cases):
    """One pair of a 257-row graph goes to Lanczos; 3 steps cannot reach 1e-10: the documented NoConvergence."""
    from autoinst_amd._ffi import NoConvergence
    c = all_cases["surface257"]
    assert ec.branches(c.w, 2) == {"lanczos"}
    g = api.DeviceGraph.from_scipy(c.w)
    try:
        with pytest.raises(NoConvergence, match="tolerance"):
            api.eigs_smallest(g, 2, max_iter=3)
    finally:
        g.free()


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import eig_cases as ec
from autoinst_amd import ncuts_api as api
api.default_context()
only = sys.argv[2]
fails, n = [], 0
for c in ec.chfsi_cases():
    # weights 1e-10 .. 1: the block solver's convergence there depends on the filter settings (see eig_cases.cases)
    if (only and c.family != only) or c.name.endswith("_steep"):
        continue
    g = api.DeviceGraph.from_scipy(c.w)
    for k in c.ks:
        if k < 3:
            continue
        try:
            evals, V, steps, resid = api.eigs_smallest(g, k)
            ec.check_eigs(c.w, k, evals, V, resid)
            n += 1
        except Exception as e:
            fails.append(f"{c.name} k={k}: {type(e).__name__}: {e}")
    g.free()
print("\n".join(fails))
print(f"EIGS_CHILD {n} ok {len(fails)} failed")
"""


@pytest.mark.parametrize("setting,only", [("AI_EIGS_F32_FILTER=0", ""), ("AI_EIGS_PLAIN_SPMM=1", ""),
                                          # single-vector Lanczos is only a valid answer on simple spectra
                                          ("AI_EIGS_LANCZOS=1", "surface")])
def test_block_cases_with_other_solver_settings(setting, only):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    key, val = setting.split("=")
    env = dict(os.environ, **{key: val})
    r = subprocess.run([sys.executable, "-c", _CHILD, root, only], env=env, timeout=900, capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-3000:] + r.stderr[-3000:]
    assert " 0 failed" in r.stdout and "EIGS_CHILD 0 ok" not in r.stdout, r.stdout[-3000:]
