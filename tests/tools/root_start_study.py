"""CPU study: do the ANCESTOR-LESS solves get shorter when they start from the principal-axis coordinate of their own points?

The warm start (tests/tools/warmstart_study.py, DESIGN_EXPERIMENTS G1) reaches segments with a solved ancestor only; the connected
components a chunk falls into first have none and start from the hash vector.  Here those segments start from

    R_0 = (u1 * t) * (sqrt(n) / sigma) * sqrt(n) + 1e-3 * hash        u1 = sqrt(d / vol),  d = degree + 1

where t is the points' coordinate along the leading eigenvector of the 3 x 3 covariance of the segment's own points (centred) and
sigma its standard deviation: the form the device computes (fk_pca_moments / fk_pca_axis / fk_pca_fill write warm = u1 t sqrt(n) / sigma,
a vector of unit root-mean-square up to the correlation of degree and coordinate, and fk_lz_init multiplies a warm vector by the
square root of SegRec.pad0 = n).  sigma not above zero (duplicated points): the hash start.  Children start as the shipped library's:
ev2|child * sqrt(n_parent) + 1e-3 * hash, inherited through component splits.

The recursion, the Lanczos iteration and the every-step convergence test are warmstart_study's (tests/gpu_model.py underneath).

    python tests/tools/root_start_study.py [N MODE SEED ...]     default: the seven fixtures below
        -> one JSON line per fixture, printed and appended to profiles/root_start_study.jsonl
"""
import json
import os
import sys
import time

import numpy as np
from scipy.sparse.csgraph import connected_components

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import warmstart_study as ws  # noqa: E402
from warmstart_study import ROOT, MODES, chunk_for, gm, ncuts_ref  # noqa: E402

FIXTURES = [(200000, "tarl", 0), (200000, "tarl", 1), (50000, "tarl", 0), (50000, "spatial", 0), (30000, "tarl", 21), (20000, "tarl", 3),
            (20000, "tri", 2)]
EPS = 1e-3


def principal_axis(pts):
    """Mean, leading eigenvector of the covariance (sign: its largest component in magnitude is positive) and sigma of the coordinate along it."""
    mean = pts.mean(axis=0)
    x = pts - mean
    lam, U = np.linalg.eigh(x.T @ x / len(pts))
    e = U[:, -1]
    if e[np.argmax(np.abs(e))] < 0:
        e = -e
    t = x @ e
    return t, float(np.sqrt(max(np.mean(t * t), 0.0)))


def root_start(w, pts, ids):
    """The device's start of an ancestor-less segment, or None (the hash start)."""
    n = w.shape[0]
    t, sigma = principal_axis(pts)
    if not (sigma > 0.0 and np.isfinite(sigma)):
        return None
    d = np.asarray(w.sum(axis=0)).ravel() + 1.0
    u1 = np.sqrt(d / d.sum())
    warm = u1 * t * (np.sqrt(n) / sigma)
    return warm * np.sqrt(n) + EPS * gm.start_vector(ids)


def run(A, pts, n, T, rule):
    """rule: "hash" (every solve starts from the hash vector: AI_FLOW_WARM=0), "shipped" (warm children), "root" (warm children + this study's roots)."""
    st = {"solves": 0, "root_solves": 0, "pca_solves": 0, "steps": 0, "row_steps": 0, "root_row_steps": 0}
    groups = []

    def rec(w, lab, warm):
        nn = w.shape[0]
        if not gm._eligible(nn, n, 0.01):
            groups.append(lab)
            return
        ncomp, comp = connected_components(w, directed=False)
        if ncomp > 1:
            if not (0.0 < T):
                groups.append(lab)
                return
            for idx in gm.split_components(ncomp, comp):
                rec(w[idx][:, idx], lab[idx], None if warm is None else warm[idx])
            return
        start = warm
        if warm is None:
            st["root_solves"] += 1
            if rule == "root":
                start = root_start(w, pts[lab], lab)
                st["pca_solves"] += start is not None
        ev, m, resid, d, fied, extra = ws.lanczos(w, lab, start=start, n_extra=1)
        st["solves"] += 1
        st["steps"] += m
        st["row_steps"] += nn * m
        if warm is None:
            st["root_row_steps"] += nn * m
        mask, mcut, _ = gm.sweep(ev, d, w)
        if not (mcut < T):
            groups.append(lab)
            return
        wv = None
        if extra and rule != "hash":
            wv = extra[0][1] * np.sqrt(nn) + EPS * gm.start_vector(lab)
        rec(w[mask][:, mask], lab[mask], None if wv is None else wv[mask])
        rec(w[~mask][:, ~mask], lab[~mask], None if wv is None else wv[~mask])

    sys.setrecursionlimit(10000)
    rec(A, np.arange(n), None)
    st["groups"] = len(groups)
    return st, ncuts_ref.groups_to_labels(groups, n)


def study(n, mode, seed):
    cfg = MODES[mode]
    ch = chunk_for(n, mode, seed)
    pts = np.asarray(ch["points"], dtype=np.float64)
    A = ncuts_ref.affinity_sparse(ch["points"], ch["tarl"], ch["dino"], alpha=cfg["alpha"], theta=cfg["theta"], gamma=cfg["gamma"])
    t0 = time.time()
    hsh, labh = run(A, pts, n, cfg["T"], "hash")
    base, lab0 = run(A, pts, n, cfg["T"], "shipped")
    new, lab1 = run(A, pts, n, cfg["T"], "root")
    return {"n": n, "mode": mode, "seed": seed, "hash": hsh, "shipped": base, "root_start": new,
            "row_steps_vs_hash": round(new["row_steps"] / hsh["row_steps"], 4),
            "root_share_of_row_steps": round(base["root_row_steps"] / base["row_steps"], 4),
            "row_steps_vs_shipped": round(new["row_steps"] / base["row_steps"], 4),
            "partition_equal": bool(ncuts_ref.partitions_equal(lab0, lab1) and ncuts_ref.partitions_equal(labh, lab1)), "seconds": round(time.time() - t0, 1)}


def main(argv):
    fx = [(int(argv[i]), argv[i + 1], int(argv[i + 2])) for i in range(0, len(argv) - 2, 3)] or FIXTURES
    out = os.path.join(ROOT, "profiles", "root_start_study.jsonl")
    for n, mode, seed in fx:
        line = json.dumps(study(n, mode, seed))
        print(line, flush=True)
        with open(out, "a") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main(sys.argv[1:])
