"""Reader of the per-segment dump of the shipped NCut path and its float64 reference (CPU only: imports no GPU code).

The test-only build (libautoinst_hip_lockstep.so, -DAI_TEST_HOOKS) appends one record per segment of every wave to the file named by
AI_FLOW_DUMP (Flow::dump_seg in autoinst_amd/csrc/ai_flow.inc).  Layout, little-endian:

    int64  kind ('L' = 76 harvested Lanczos segment | 'C' = 67 split into its connected components), chunk, n, m, restarts, nosplit,
           kstar, split, ntrue
    double theta, resid (estimate), rtrue (true residual), scale, mcut, thr[10], costs[10]
    int32  ids[n]        chunk-local original ids of the segment's rows, in position order
    L: double ev[n]      the raw Ritz vector at those positions | C: int32 comp[n], the device's component label per row

`check_lanczos` restates normalized_cut.py:13-53 in float64 on the record's own subgraph w[ids][:, ids]; `check_components` and
`audit_tree` check the rest of the recursion.  Every check raises AssertionError with a message naming what failed.
"""
from __future__ import annotations

import math

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

NUM_CUTS = 10
HEAD = np.dtype([("kind", "<i8"), ("chunk", "<i8"), ("n", "<i8"), ("m", "<i8"), ("restarts", "<i8"), ("nosplit", "<i8"),
                 ("kstar", "<i8"), ("split", "<i8"), ("ntrue", "<i8"), ("theta", "<f8"), ("resid", "<f8"), ("rtrue", "<f8"),
                 ("scale", "<f8"), ("mcut", "<f8"), ("thr", "<f8", (NUM_CUTS,)), ("costs", "<f8", (NUM_CUTS,))])
assert HEAD.itemsize == 272

COST_RTOL = 1e-11       # device costs against the fsum reference
EIG_N_MAX = 20000       # segments up to this size get the eigsh reference
RESID_MAX = 2e-10       # true residual of a healthy pair (tol = 1e-10, as max_true_resid)
TRUE_RESID_LIMIT = 1e-6  # the library's limit: pairs above it were accepted only because a repeated solve reproduced them bit for bit
SPLIT_LIM_CHILD = 0.01  # children of a cut / components: the library's fixed 1 % rule (normalized_cut.py:39-40 at its default)


# ----------------------------------------------------------------------------------------------------------------- file format
def read_dump(path):
    """Records of a dump file as dicts: the header fields, 'kind' as 'L' / 'C', 'ids' and 'ev' (L) or 'comp' (C)."""
    raw = open(path, "rb").read()
    out, p = [], 0
    while p < len(raw):
        h = np.frombuffer(raw, HEAD, 1, p)[0]
        p += HEAD.itemsize
        n = int(h["n"])
        rec = {k: (h[k].copy() if k in ("thr", "costs") else h[k].item()) for k in HEAD.names}
        rec["kind"] = chr(rec["kind"])
        assert rec["kind"] in "LC", f"bad record kind {rec['kind']!r} at byte {p - HEAD.itemsize}"
        rec["ids"] = np.frombuffer(raw, "<i4", n, p).copy()
        p += 4 * n
        if rec["kind"] == "L":
            rec["ev"] = np.frombuffer(raw, "<f8", n, p).copy()
            p += 8 * n
        else:
            rec["comp"] = np.frombuffer(raw, "<i4", n, p).copy()
            p += 4 * n
        out.append(rec)
    assert p == len(raw), "trailing bytes in the dump"
    return out


def write_record(f, rec):
    """The inverse of read_dump for one record (tests build files with it)."""
    h = np.zeros(1, HEAD)
    for k in HEAD.names:
        if k == "kind":
            h[k] = ord(rec["kind"])
        elif k == "n":
            h[k] = len(rec["ids"])
        elif k in rec:
            h[k] = rec[k]
    f.write(h.tobytes())
    f.write(np.asarray(rec["ids"], "<i4").tobytes())
    f.write(np.asarray(rec["ev"], "<f8").tobytes() if rec["kind"] == "L" else np.asarray(rec["comp"], "<i4").tobytes())


# ----------------------------------------------------------------------------------------------------------------- reference
def subgraph(w, ids):
    """w[ids][:, ids], W = w_s + I and d = colsum(W) (normalized_cut.py:38-45)."""
    ws = sp.csr_matrix(w)[ids][:, ids].tocsr()
    W = ws + sp.identity(ws.shape[0], format="csr")
    d = np.asarray(W.sum(axis=0)).ravel()
    return ws, d


def thresholds(e):
    mn, mx = e.min(), e.max()
    return np.linspace(mn, mx, NUM_CUTS, endpoint=False), bool(np.allclose(mn, mx))


def reference_costs(ws, d, masks):
    """cut(A, B) / vol(A) + cut(A, B) / vol(B) per mask, every sum with math.fsum.  The cut is taken edge by edge over the entries
    (i in A, j not in A) -- not as sum(W) - sum(W_AA) - sum(W_BB), which cancels."""
    coo = ws.tocoo()
    cross = masks[:, coo.row] & ~masks[:, coo.col]
    out = np.empty(len(masks))
    for k, m in enumerate(masks):
        cut = math.fsum(coo.data[cross[k]])
        va, vb = math.fsum(d[m]), math.fsum(d[~m])
        out[k] = cut / va + cut / vb
    return out


def _sin_angle(v, u):
    v = v / np.linalg.norm(v)
    u = u / np.linalg.norm(u)
    return float(np.linalg.norm(v - (v @ u) * u))


def check_lanczos(rec, w, T, *, eig=True, resid_max=RESID_MAX):
    """Checks 1-6 of one L record against its own subgraph; returns what was measured.

    Costs: every term of a cut and of a volume is positive, so a sum formed in any order has a relative forward error of at most
    (L - 1) u for a serial chain of length L (u = 2^-53).  The device's longest chain is 32 rows of a fine task + ceil(tasks / 6) tasks
    of a stripe + 6 stripes: about 1100 for a 200 000-row segment, 1.2e-13; the degrees inside the volumes add ~(row length) u, and a
    cost adds two divisions and a sum.  So COST_RTOL = 1e-11 holds with two orders of magnitude to spare, and a single cost off by
    1e-9 or a lost stripe (a sixth of a volume) is far outside it."""
    ids, ev = rec["ids"], rec["ev"]
    n = len(ids)
    assert n == rec["n"] and len(np.unique(ids)) == n, "ids are not a set"
    # 1. subgraph
    ws, d = subgraph(w, ids)
    ncomp, _ = connected_components(ws, directed=False)
    assert ncomp == 1, f"a Lanczos segment of {n} rows has {ncomp} components"
    # 2. scale and sign (mm_merge: the entry of largest magnitude, the smallest original id on a tie)
    sc = rec["scale"]
    nrm = math.sqrt(math.fsum(ev * ev))
    assert abs(abs(sc) * nrm - 1.0) <= 1e-14, f"|scale| * ||ev|| = {abs(sc) * nrm!r}"
    a = np.abs(ev)
    top = np.flatnonzero(a == a.max())
    j = top[np.argmin(ids[top])]
    assert ev[j] * sc > 0, "sign: the entry of largest magnitude of ev * scale is not positive"
    e = ev * sc
    # 3. thresholds, bit for bit
    thr_ref, flat = thresholds(e)
    assert np.array_equal(rec["thr"].view(np.int64), thr_ref.view(np.int64)), f"thresholds differ: {rec['thr']!r} vs {thr_ref!r}"
    assert bool(rec["nosplit"]) == flat, "nosplit differs from np.allclose(min, max)"
    out = dict(n=n, cost_rel=0.0, near_tie=0, lam_err=0.0, dk_ratio=0.0, above_limit=int(rec["rtrue"] > TRUE_RESID_LIMIT), eig=False)
    if flat:
        assert rec["split"] == 0 and rec["kstar"] == 0 and rec["ntrue"] == 0 and rec["mcut"] == np.inf and np.all(rec["costs"] == np.inf)
    else:
        # 4. costs from the device's own vector; the strict > puts the minimum itself on the B side at k = 0
        masks = e[None, :] > rec["thr"][:, None]
        ref = reference_costs(ws, d, masks)
        dev = rec["costs"]
        rel = np.abs(dev - ref) / np.abs(ref)
        out["cost_rel"] = float(rel.max())
        assert rel.max() <= COST_RTOL, f"costs differ from the fsum reference by rel {rel.max():.3g}: {dev!r} vs {ref!r}"
        # 5. decision
        ks = int(np.argmin(dev))
        assert rec["kstar"] == ks, f"kstar {rec['kstar']} is not the first minimum {ks}"
        assert rec["mcut"] == dev[ks], "mcut is not costs[kstar]"
        assert bool(rec["split"]) == bool(rec["mcut"] < T), "split != (mcut < T)"
        assert rec["ntrue"] == masks[ks].sum(), "ntrue is not the size of mask kstar"
        kr = int(np.argmin(ref))
        tie = any(not np.array_equal(masks[k], masks[kr]) and abs(ref[k] - ref[kr]) <= COST_RTOL * ref[kr] for k in range(NUM_CUTS))
        out["near_tie"] = int(tie)
        if not tie:
            assert np.array_equal(masks[ks], masks[kr]), f"the device's mask {ks} is not the reference's argmin {kr}"
    # 6. eigenpair
    if eig and n <= EIG_N_MAX and n > 3:
        import scipy.sparse.linalg as spla
        from oracle import ncuts_ref
        L, _ = ncuts_ref.laplacian_sym(ws)
        vals, vecs = spla.eigsh(L, 3, sigma=1e-10, which="LM")
        o = np.argsort(vals)
        l2, l3, v2 = vals[o[1]], vals[o[2]], vecs[:, o[1]]
        lam = 1.0 - rec["theta"]   # the flow iterates on M = D^-1/2 W D^-1/2 = I - L_sym
        out["lam_err"] = abs(lam - l2) / max(l2, 1e-300)
        assert abs(lam - l2) <= 1e-12 + 1e-8 * l2, f"lambda2 {lam!r} vs eigsh {l2!r}"
        r_dump = rec["rtrue"]
        delta = min(l2, l3 - l2)
        bound = 2.0 * r_dump / delta + 1e-10
        s = _sin_angle(ev, v2)
        out["dk_ratio"] = s / bound
        assert s <= bound, f"Davis-Kahan: sin angle {s:.3g} > 2 r / delta + 1e-10 = {bound:.3g}"
        r = float(np.linalg.norm(L @ ev - lam * ev) / np.linalg.norm(ev))
        assert abs(r - r_dump) <= max(1e-13, 1e-6 * r), f"true residual {r_dump!r} vs CPU {r!r}"
        out["eig"] = True
    # the 2e-10 bar: not for pairs above the library's limit, nor where T reached the segment's own dimension (the library accepts
    # those whatever the estimate, Flow::wave_s3) -- both still had to match the CPU residual and the Davis-Kahan bound above
    if not out["above_limit"] and rec["m"] < n - 1:
        assert rec["rtrue"] <= resid_max, f"true residual {rec['rtrue']:.3g} > {resid_max:g} (n {n}, m {rec['m']}, estimate {rec['resid']:.3g})"
    return out


def check_components(rec, w):
    """A C record: the device's component labels are scipy's connected components, as partitions, and there are at least 2."""
    from oracle import ncuts_ref
    ws, _ = subgraph(w, rec["ids"])
    ncomp, comp = connected_components(ws, directed=False)
    assert ncomp >= 2, "a component split of a connected segment"
    assert ncuts_ref.partitions_equal(rec["comp"], comp), "component labels differ from connected_components"
    return ncomp


def eligible(n, n_orig, split_lim):
    """normalized_cut.py:39-40."""
    return n > 2 and n / (n_orig + 1e-8) > split_lim


def audit_tree(recs, sizes, n_orig, labels, split_lim, T):
    """Check 7 over one call: roots, children of every split (the two mask sides) and of every component split, each eligible one
    dumped exactly once and nothing else dumped; the leaves give the call's labels as a set partition.  sizes / n_orig / labels
    per chunk."""
    from oracle import ncuts_ref
    seen = {}
    for r in recs:
        key = (r["chunk"], tuple(np.sort(r["ids"])))
        assert key not in seen, f"segment of {len(key[1])} rows in chunk {key[0]} dumped twice"
        seen[key] = r
    expected, leaves = set(), [[] for _ in sizes]

    def child(c, ids, lim):
        if eligible(len(ids), n_orig[c], lim):
            expected.add((c, tuple(np.sort(ids))))
        else:
            leaves[c].append(ids)

    for c, n in enumerate(sizes):
        child(c, np.arange(n), split_lim)
    for (c, _), r in seen.items():
        if r["kind"] == "C":
            for k in np.unique(r["comp"]):
                child(c, r["ids"][r["comp"] == k], SPLIT_LIM_CHILD)
        elif r["split"]:
            mask = r["ev"] * r["scale"] > r["thr"][r["kstar"]]
            child(c, r["ids"][mask], SPLIT_LIM_CHILD)
            child(c, r["ids"][~mask], SPLIT_LIM_CHILD)
        else:
            leaves[c].append(r["ids"])
    missing, extra = expected - set(seen), set(seen) - expected
    assert not missing, f"{len(missing)} eligible segment(s) never dumped"
    assert not extra, f"{len(extra)} dumped segment(s) that are no child of anything"
    for c, n in enumerate(sizes):
        lab = np.full(n, -1)
        for g, ids in enumerate(leaves[c]):
            assert np.all(lab[ids] == -1), "leaves overlap"
            lab[ids] = g
        assert np.all(lab >= 0), "leaves do not cover the chunk"
        assert ncuts_ref.partitions_equal(lab, labels[c]), f"leaves of chunk {c} are not the call's labels"


def check_call(recs, graphs, n_orig, labels, split_lim, T, *, accepted_above_limit=0, eig=True):
    """Every record of one call (checks 1-7) plus the count of pairs above the library's limit; returns a summary per call."""
    summ = dict(records=len(recs), lanczos=0, components=0, eig_checked=0, cost_rel=0.0, lam_err=0.0, dk_ratio=0.0, near_ties=0,
                above_limit=0)
    for r in recs:
        w = graphs[r["chunk"]]
        if r["kind"] == "C":
            check_components(r, w)
            summ["components"] += 1
            continue
        o = check_lanczos(r, w, T, eig=eig)
        summ["lanczos"] += 1
        summ["eig_checked"] += int(o["eig"])
        summ["cost_rel"] = max(summ["cost_rel"], o["cost_rel"])
        summ["lam_err"] = max(summ["lam_err"], o["lam_err"])
        summ["dk_ratio"] = max(summ["dk_ratio"], o["dk_ratio"])
        summ["near_ties"] += o["near_tie"]
        summ["above_limit"] += o["above_limit"]
    assert summ["above_limit"] == accepted_above_limit, f"{summ['above_limit']} pairs above the limit, the call reported {accepted_above_limit}"
    audit_tree(recs, [g.shape[0] for g in graphs], n_orig, labels, split_lim, T)
    return summ
