"""CPU restatement of the cut tree (ai_ncut_tree / ai_ncut_relabel), built from `gpu_model`'s functions.

`tree_model` runs the recursion of `gpu_model.normalized_cut_model` once at ``T_max`` and records, per group, the height of the
boundary in front of it and the cost of the cut the group itself was refused; `relabel_ref` is the rule that turns those into the
labels at a smaller threshold.  The tests compare both with direct cuts (`gpu_model.normalized_cut_model` on the CPU, `ncuts_labels`
on the device) at the thresholds where the answer changes.
"""
import os
from collections import namedtuple

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import gpu_model
from conftest import GOLDEN

TreeModel = namedtuple("TreeModel", "labels cut_height leaf_cost n_cheaper masked")
# labels[i]: group of row i at T_max (emission order); cut_height / leaf_cost: per group, as the device defines them;
# n_cheaper: cuts whose own cost is below the largest cost among their ancestors; masked[g]: the boundary in front of group g was
# made by such a cut, so its height is an ancestor's cost and not its own


def load_graph(name):
    z = np.load(os.path.join(GOLDEN, name + ".npz"))
    n = z["points"].shape[0]
    return sp.csr_matrix((z["data"], z["indices"], z["indptr"]), shape=(n, n))


def tree_model(w, n_orig, T_max, split_lim=0.01):
    n = w.shape[0]
    leaves = []   # (rows, front, cost, masked) in emission order
    cheaper = [0]

    def rec(w, rows, front, front_masked, path, lim):
        m = w.shape[0]
        if not gpu_model._eligible(m, n_orig, lim):
            leaves.append((rows, front, np.nan, front_masked))
            return
        ncomp, comp = connected_components(w, directed=False)
        if ncomp > 1:
            if not (0.0 < T_max):
                leaves.append((rows, front, np.nan, front_masked))
                return
            p = max(path, 0.0)
            low = 0.0 < path
            cheaper[0] += int(low)
            for j, idx in enumerate(gpu_model.split_components(ncomp, comp)):
                rec(w[idx][:, idx], rows[idx], front if j == 0 else p, front_masked if j == 0 else low, p, 0.01)
            return
        d = np.asarray(w.sum(axis=0)).ravel() + 1.0
        _, ev, _, _ = gpu_model.lanczos_fiedler(w, rows)
        mask, mcut, _ = gpu_model.sweep(ev, d, w)
        if not (mcut < T_max):
            leaves.append((rows, front, mcut, front_masked))
            return
        p = max(path, mcut)
        low = mcut < path
        cheaper[0] += int(low)
        rec(w[mask][:, mask], rows[mask], front, front_masked, p, 0.01)
        rec(w[~mask][:, ~mask], rows[~mask], p, low, p, 0.01)

    rec(sp.csr_matrix(w), np.arange(n), -np.inf, False, -np.inf, split_lim)
    labels = np.empty(n, dtype=np.int32)
    for g, (rows, _, _, _) in enumerate(leaves):
        labels[rows] = g
    return TreeModel(labels, np.array([l[1] for l in leaves], dtype=np.float64), np.array([l[2] for l in leaves], dtype=np.float64),
                     cheaper[0], np.array([l[3] for l in leaves], dtype=bool))


def relabel_ref(labels, cut_height, T):
    """Labels and group count of ONE chunk at threshold T: the boundary in front of group g >= 1 exists iff cut_height[g] < T."""
    labels = np.asarray(labels)
    h = np.asarray(cut_height, dtype=np.float64)
    if h.shape[0] == 0:
        return np.zeros(0, dtype=np.int32), 0
    exists = h < T
    exists[0] = False
    new_id = np.cumsum(exists)
    return new_id[labels].astype(np.int32), int(new_id[-1]) + 1


def relabel_chunks_ref(labels, cut_heights, thresholds):
    """`relabel_ref` for lists of chunks and thresholds: (labels[t][c], n_groups[t, c])."""
    out = [[relabel_ref(l, h, T) for l, h in zip(labels, cut_heights)] for T in thresholds]
    return [[x[0] for x in row] for row in out], np.array([[x[1] for x in row] for row in out], dtype=np.int32).reshape(len(thresholds), len(labels))


def labels_of_groups(groups, n):
    """groups (list of row-index arrays in emission order) -> label per row."""
    lab = np.full(n, -1, dtype=np.int32)
    for g, idx in enumerate(groups):
        lab[idx] = g
    return lab


def sweep_thresholds(cut_height, T_max, limit=None):
    """Where the partition changes: every distinct finite height and the next float above it (capped at T_max), plus 0 and T_max;
    ``limit``: at most that many heights, spread evenly over the sorted distinct ones."""
    hs = np.unique(cut_height[np.isfinite(cut_height)])
    if limit is not None and hs.shape[0] > limit:
        hs = hs[np.unique(np.linspace(0, hs.shape[0] - 1, limit).round().astype(int))]
    ts = [0.0, float(T_max)]
    for h in hs:
        ts += [float(h), float(min(np.nextafter(h, np.inf), T_max))]
    return ts


class cached_solver:
    """While active, `gpu_model.lanczos_fiedler` remembers its results by (graph, ids): a direct cut at T' solves a subset of the
    segments the cut at T_max solved, with identical inputs, and the model's solver is a pure function of them.  Nothing of the
    recursion's own decisions (eligibility, components, sweep, the comparison with T) is cached."""

    def __enter__(self):
        self.orig = gpu_model.lanczos_fiedler
        memo = {}

        def solver(w, ids, *a, **kw):
            w = sp.csr_matrix(w)
            key = (np.asarray(ids).tobytes(), w.indptr.tobytes(), w.indices.tobytes(), w.data.tobytes(), a, tuple(sorted(kw.items())))
            if key not in memo:
                memo[key] = self.orig(w, ids, *a, **kw)
            return memo[key]

        gpu_model.lanczos_fiedler = solver
        return self

    def __exit__(self, *exc):
        gpu_model.lanczos_fiedler = self.orig
