"""Calls of the NCut path with the per-segment dump on (AI_FLOW_DUMP, a hook of the TEST-ONLY build libautoinst_hip_lockstep.so):
run as a child process by tests/test_gpu_flow_values.py with AUTOINST_HIP_LIB pointing at that build.  The fixture builders are
imported by the parent too, which runs the same graphs through the shipped library.

    python tests/flow_cases.py OUTDIR

writes OUTDIR/<case>.bin (the dump of one call) and OUTDIR/<case>.npz (the CSR of every chunk as cut, labels, parameters, stats).
"""
import os
import sys

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)
from autoinst_amd import ncuts_api as api, synth  # noqa: E402

HEADLINE = dict(alpha=1.0, theta=0.5, gamma=0.0, T=0.03)   # bench.py's configuration; its chunk: synthetic_chunk(200000, 0, tarl=True)
SPLIT_LIM = 0.01


def golden_names():
    return sorted(f[:-4] for f in os.listdir(GOLDEN) if f.startswith("g") and f.endswith(".npz"))


def build(case):
    """(graphs, n_orig, T, split_lim) of a single-chunk case."""
    if case.startswith("g"):
        z = np.load(os.path.join(GOLDEN, case + ".npz"))
        n = z["points"].shape[0]
        A = sp.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=(n, n))
        return [api.DeviceGraph.from_scipy(A)], [n], float(z["T"]), float(z["split_lim"])
    if case.startswith("c1_"):
        z = np.load(os.path.join(GOLDEN, case + ".npz"))
        tarl = z["tarl"].astype(np.float64) if float(z["theta"]) > 0 else None
        g = api.build_affinity(z["points"], tarl, alpha=float(z["alpha"]), theta=float(z["theta"]), gamma=float(z["gamma"]))
        return [g], [g.n], float(z["T"]), float(z["split_lim"])
    if case == "headline":
        ch = synth.synthetic_chunk(200000, 0, tarl=True)
        g = api.build_affinity(ch["points"], ch["tarl"], alpha=HEADLINE["alpha"], theta=HEADLINE["theta"], gamma=HEADLINE["gamma"])
        return [g], [g.n], HEADLINE["T"], SPLIT_LIM
    if case == "dense":
        # the sheet / dense blob layout of test_feature_factors_tiled_and_fallback_tiles_in_one_graph: rows of more than 64 and of
        # more than 400 entries (the second entry loop of fk_sweep), segments that span many fine tasks
        rng = np.random.default_rng(196)
        sheet = np.c_[rng.uniform(-12, 12, (5000, 2)), rng.normal(0, 0.05, 5000)]
        blob = rng.normal(0, 0.35, (1500, 3)) + np.array([2.0, -3.0, 0.0])
        mid = rng.normal(0, 0.8, (1500, 3)) + np.array([-5.0, 4.0, 0.0])
        pts = np.concatenate([sheet, blob, mid])
        tarl = rng.normal(0, 0.4, (pts.shape[0], 96))
        tarl[::9] = 0.0
        g = api.build_affinity(pts, tarl, alpha=1.0, theta=0.5, gamma=0.0)
        return [g], [g.n], 0.03, SPLIT_LIM
    if case in CSR_CASES:
        # hand-built graphs whose rows, 32-row tasks and segments sit on the kernels' thresholds (tests/csr_cases.py).  `band` runs with
        # num_points_orig = n and a root split_lim of 0.001: its 3-row block then stays unsolved, and that block is the one segment of
        # these graphs with two mirror-image masks of equal cost (tests/test_csr_cases.py), which the per-record checks count as a near-tie
        import csr_cases
        w = csr_cases.limit_case(case)
        n_orig, lim = (w.shape[0], 0.001) if case == "band" else (csr_cases.N_ORIG, csr_cases.SPLIT_LIM)
        return [api.DeviceGraph.from_scipy(w)], [n_orig], csr_cases.T, lim
    raise ValueError(case)


BATCH_SIZES = ((30000, 3), (12000, 4), (50000, 5))


def build_batch():
    gs = []
    for n, seed in BATCH_SIZES:
        ch = synth.synthetic_chunk(n, seed, tarl=True)
        gs.append(api.build_affinity(ch["points"], ch["tarl"], alpha=1.0, theta=0.5, gamma=0.0))
    return gs, [g.n for g in gs], HEADLINE["T"], SPLIT_LIM


CSR_CASES = ("band", "band128", "band128_diag", "stride", "stride_diag")
CASES = golden_names() + ["c1_10k_tarl", "c1_10k_spatial", "headline", "dense"] + list(CSR_CASES)


def _save(out, name, graphs, n_orig, T, split_lim, labs, st):
    csr = {}
    for i, g in enumerate(graphs):
        A = g.to_scipy()
        csr.update({f"indptr{i}": A.indptr, f"indices{i}": A.indices, f"data{i}": A.data, f"labels{i}": labs[i]})
    np.savez(os.path.join(out, name + ".npz"), k=len(graphs), n_orig=np.asarray(n_orig), T=T, split_lim=split_lim,
             accepted_above_limit=st["accepted_above_limit"], max_true_resid=st["max_true_resid"], **csr)


def _dumped(out, name, fn):
    path = os.path.join(out, name + ".bin")
    if os.path.exists(path):
        os.remove(path)
    os.environ["AI_FLOW_DUMP"] = path
    try:
        return fn()
    finally:
        os.environ.pop("AI_FLOW_DUMP")


def main(out):
    for case in CASES:
        graphs, n_orig, T, split_lim = build(case)
        lab, ng, st = _dumped(out, case, lambda: api.ncuts_labels(graphs[0], n_orig[0], T, split_lim))
        _save(out, case, graphs, n_orig, T, split_lim, [lab], st)
        for g in graphs:
            g.free()
    graphs, n_orig, T, split_lim = build_batch()
    for i, g in enumerate(graphs):
        lab, ng, st = _dumped(out, f"solo{i}", lambda: api.ncuts_labels(g, n_orig[i], T, split_lim))
        _save(out, f"solo{i}", [g], n_orig[i:i + 1], T, split_lim, [lab], st)
    # all three in one pool; then a window of 55 000 rows, so that admission serialises them
    for name, win in (("batch", None), ("batch_window", 55000)):
        labs, ngs, st = _dumped(out, name, lambda: api.ncuts_labels_batch(graphs, n_orig, T, split_lim, window_rows=win))
        _save(out, name, graphs, n_orig, T, split_lim, labs, st)
    print("flow cases: ok")


if __name__ == "__main__":
    main(sys.argv[1])
