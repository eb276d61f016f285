"""Hand-built symmetric CSR graphs that put a row, a 32-row task or a segment of the shipped cut (the fk_* kernels of
autoinst_amd/csrc/ai_flow_kernels.inc) exactly on a threshold, the input forms a caller's SciPy matrix can take, and a dense float64
restatement of the reference's recursion.  NumPy / SciPy only: importable without a GPU.

The thresholds ("The caller's CSR at the door"): 16 lanes x 4 rounds = 64 entries of a row loaded at once, 32 rows per
fine task and 512 per coarse one, AI_ENC_MAXNNZ = 4096 entries and AI_ENC_XCAP = 1024 distinct columns of a task, FK_CHECK_WIDE_M = 64
rows of T, AI_SLAB_VECS = 32 Lanczos vectors per slab, SWF_STRIPES = 6, and a Krylov space exhausted at m = n - 1.
"""
from __future__ import annotations

import functools

import numpy as np
import scipy.linalg
import scipy.sparse as sp
from scipy.sparse.csgraph import connected_components

import flow_dump
import gpu_model

N_ORIG = 100          # num_points_orig of every case: a 3-row block is 3 % of the "chunk" and is solved, with m = n - 1 = 2
SPLIT_LIM = 0.01
T = 0.004
TASK_ROWS = 32
DENSE_N_MAX = 2400


# ----------------------------------------------------------------------------------------------------------------- builders
def _assemble(n, rows, cols, vals, diagonal):
    if diagonal:
        rows.append(np.arange(n))
        cols.append(np.arange(n))
        vals.append(np.full(n, float(diagonal)))
    w = sp.csr_matrix((np.concatenate(vals), (np.concatenate(rows), np.concatenate(cols))), shape=(n, n))
    w.sum_duplicates()     # nothing is stored twice: this only sorts
    w.sort_indices()
    assert w.nnz == sum(len(v) for v in vals)
    return w


def _bridge(offsets, bridges, rows, cols, vals):
    for k, b in enumerate(bridges):
        i, j = offsets[k + 1] - 1, offsets[k + 1]       # last row of block k, first row of block k + 1
        rows += [np.array([i, j])]
        cols += [np.array([j, i])]
        vals += [np.array([b, b], dtype=np.float64)]


def band_blocks(sizes, bands, bridges, decay=0.05, diagonal=1.0):
    """Blocks of banded rows: inside block k, w_ij = exp(-decay |i - j|) for 1 <= |i - j| <= bands[k]; a constant diagonal
    (None / 0: not stored); one edge of weight bridges[k] between the last row of block k and the first of block k + 1.  Sorted
    columns; both copies of an edge come from one computed value, so the matrix is symmetric to the bit."""
    assert len(bands) == len(sizes) and len(bridges) == len(sizes) - 1
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows, cols, vals = [], [], []
    for k, (m, b) in enumerate(zip(sizes, bands)):
        for s in range(1, min(b, m - 1) + 1):
            i = np.arange(off[k], off[k] + m - s)
            v = np.full(i.shape[0], np.exp(-decay * s))
            rows += [i, i + s]
            cols += [i + s, i]
            vals += [v, v]
    _bridge(off, bridges, rows, cols, vals)
    return _assemble(int(off[-1]), rows, cols, vals, diagonal)


def stride_blocks(sizes=(1100, 1200), bridges=(2e-3,), diagonal=None):
    """Per block, entries at |i - j| = 32 k + 1 for k = 1..16 with weight 0.9^k: the 32 rows of a task reach 32 x 32 = 1024 distinct
    columns with 1024 entries (AI_ENC_XCAP exactly; 1056 of each with a stored diagonal)."""
    off = np.concatenate([[0], np.cumsum(sizes)])
    rows, cols, vals = [], [], []
    for b, m in enumerate(sizes):
        for k in range(1, 17):
            s = 32 * k + 1
            i = np.arange(off[b], off[b] + m - s)
            v = np.full(i.shape[0], 0.9 ** k)
            rows += [i, i + s]
            cols += [i + s, i]
            vals += [v, v]
    _bridge(off, bridges, rows, cols, vals)
    return _assemble(int(off[-1]), rows, cols, vals, diagonal)


BAND = dict(sizes=[33, 512, 31, 513, 3, 65, 511, 32, 64], bands=[7, 8, 31, 32, 2, 64, 200, 31, 16],
            bridges=[1e-3 * x for x in (1.0, 1.7, 0.6, 2.3, 1.3, 0.8, 1.9, 1.1)])
BAND128 = dict(sizes=[512, 300], bands=[64, 16], bridges=[1e-3], diagonal=None)
BAND128_DIAG_ROW = 200
SMALL = dict(sizes=[33, 65, 31, 3, 64], bands=[7, 16, 31, 2, 8], bridges=[1e-3 * x for x in (1.0, 1.7, 0.6, 2.3)])
SMALL_DIAGONALS = (None, 1.0, 0.25)
SMALL_FORMS = ("canonical", "shuffled", "split", "zeros", "zero_bridges", "csc", "coo", "float32")


def band128(diag_entry=False):
    """A 512-row block of band 64 without diagonal (interior rows hold 128 entries, a task of them 4096 = AI_ENC_MAXNNZ) bridged to a
    300-row block of band 16; ``diag_entry``: the twin with ONE stored diagonal entry, 1.0 at row 200, whose task then holds 4097."""
    w = band_blocks(**BAND128)
    if diag_entry:
        w = w.tolil()
        w[BAND128_DIAG_ROW, BAND128_DIAG_ROW] = 1.0
        w = w.tocsr()
        w.sort_indices()
    return w


def limit_case(name):
    """The graphs of the limits tests: band | band128 | band128_diag | stride | stride_diag."""
    if name == "band":
        return band_blocks(**BAND)
    if name == "band128":
        return band128()
    if name == "band128_diag":
        return band128(True)
    if name == "stride":
        return stride_blocks()
    if name == "stride_diag":
        return stride_blocks(diagonal=1.0)
    raise ValueError(name)


LIMIT_CASES = ("band", "band128", "band128_diag", "stride", "stride_diag")


def _block_offsets(sizes):
    return np.concatenate([[0], np.cumsum(sizes)])


def small(form="canonical", diagonal=1.0):
    """One input form of SMALL.  Its weights are rounded to float32 (kept as float64), so that the float32 form has the same value;
    every form has the `toarray()` of the canonical form with the same diagonal, except ``zero_bridges``, whose bridges ARE zero."""
    w = band_blocks(diagonal=diagonal, **SMALL)
    w.data = w.data.astype(np.float32).astype(np.float64)
    n = w.shape[0]
    off = _block_offsets(SMALL["sizes"])
    if form == "canonical":
        return w
    if form == "shuffled":
        import eig_cases
        return eig_cases.shuffle_columns(w, 5)
    if form == "split":
        # every third entry as two exact halves, the second half stored at the end of its row
        coo = w.tocoo()
        pick = np.arange(coo.nnz) % 3 == 0
        data = np.where(pick, coo.data / 2, coo.data)
        assert np.all(data[pick] + data[pick] == coo.data[pick])
        rows = np.concatenate([coo.row, coo.row[pick]])
        cols = np.concatenate([coo.col, coo.col[pick]])
        vals = np.concatenate([data, data[pick]])
        o = np.argsort(rows, kind="stable")
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows, minlength=n))])
        out = sp.csr_matrix((vals[o], cols[o].astype(np.int32), indptr), shape=(n, n))
        assert out.nnz == w.nnz + int(pick.sum())
        return out
    if form in ("zeros", "zero_bridges"):
        lil_r, lil_c = [], []
        if form == "zeros":
            # inside a block beyond its band, between blocks (both neighbours and distant ones), and on free diagonal places
            pairs = [(off[0], off[0] + 20), (off[1] + 1, off[1] + 40), (off[4] + 2, off[4] + 50),
                     (off[1] - 1, off[1] + 1), (off[2] - 2, off[2]), (off[0] + 3, off[4] + 3), (off[3], off[4] + 10)]
            for i, j in pairs:
                assert w[i, j] == 0
                lil_r += [i, j]
                lil_c += [j, i]
            if not diagonal:
                lil_r += [0, 40, n - 1]
                lil_c += [0, 40, n - 1]
            coo = w.tocoo()
            rows = np.concatenate([coo.row, lil_r])
            cols = np.concatenate([coo.col, lil_c])
            vals = np.concatenate([coo.data, np.zeros(len(lil_r))])
        else:
            coo = w.tocoo()
            rows, cols, vals = coo.row, coo.col, coo.data.copy()
            for k in range(len(SMALL["bridges"])):
                i, j = off[k + 1] - 1, off[k + 1]
                hit = ((rows == i) & (cols == j)) | ((rows == j) & (cols == i))
                assert hit.sum() == 2
                vals[hit] = 0.0
        o = np.lexsort((cols, rows))
        indptr = np.concatenate([[0], np.cumsum(np.bincount(rows.astype(np.int64), minlength=n))])
        out = sp.csr_matrix((vals[o], cols[o].astype(np.int32), indptr), shape=(n, n))
        assert out.nnz == len(vals) and (out.data == 0).sum() == (len(lil_r) if form == "zeros" else 2 * len(SMALL["bridges"]))
        return out
    if form == "csc":
        return w.tocsc()
    if form == "coo":
        return w.tocoo()
    if form == "float32":
        out = w.astype(np.float32)
        assert np.array_equal(out.data.astype(np.float64), w.data)
        return out
    raise ValueError(form)


def by_value(w):
    """The matrix as SciPy defines it by value: CSR, duplicates summed, stored zeros dropped, sorted."""
    w = sp.csr_matrix(w, dtype=np.float64, copy=True)
    w.sum_duplicates()
    w.eliminate_zeros()
    w.sort_indices()
    return w


# ----------------------------------------------------------------------------------------------------------------- counts
def row_lengths(w):
    return np.diff(sp.csr_matrix(w).indptr)


def task_counts(w):
    """(entries, distinct columns) of every 32-row task of the root segment."""
    w = sp.csr_matrix(w)
    n = w.shape[0]
    nnz, cols = [], []
    for r in range(0, n, TASK_ROWS):
        a, b = w.indptr[r], w.indptr[min(r + TASK_ROWS, n)]
        nnz.append(int(b - a))
        cols.append(int(np.unique(w.indices[a:b]).shape[0]))
    return np.array(nnz), np.array(cols)


# ----------------------------------------------------------------------------------------------------------------- reference
def dense_reference(w, n_orig, ids, T, split_lim, stats=None):
    """normalized_cut.py:37-62 with `scipy.linalg.eigh` on the dense L_sym (connected segments of <= 2400 rows), `gpu_model.sweep` for
    :13-34, children at the default 0.01, the device's sign rule (`gpu_model.fix_sign`); a disconnected segment follows
    `gpu_model.split_components` on the matrix's VALUE (after `eliminate_zeros`).  Groups in the device's order.

    ``stats`` collects, per solved segment: its size in 'segments', the cost in 'cut' or 'refused', and in 'near_ties' the segments
    where two different masks cost within `flow_dump.COST_RTOL` of each other (the criterion of `flow_dump.check_lanczos`, on the
    reference's own vector); 'null' counts the component splits."""
    w = by_value(w)
    ids = np.asarray(ids)
    n = w.shape[0]
    if not gpu_model._eligible(n, n_orig, split_lim):
        return [ids]
    ncomp, comp = connected_components(w, directed=False)
    if ncomp > 1:
        if stats is not None:
            stats["null"] = stats.get("null", 0) + 1
        if not (0.0 < T):
            return [ids]
        out = []
        for idx in gpu_model.split_components(ncomp, comp):
            out += dense_reference(w[idx][:, idx], n_orig, ids[idx], T, 0.01, stats)
        return out
    assert n <= DENSE_N_MAX, n
    W = w.toarray() + np.eye(n)                       # :38
    d = W.sum(axis=0)                                 # :42
    d2 = 1.0 / np.sqrt(d)
    A = d2[:, None] * (np.diag(d) - W) * d2[None, :]  # :47
    vals, vecs = scipy.linalg.eigh(A)
    ev = gpu_model.fix_sign(vecs[:, 1])
    mask, mcut, _ = gpu_model.sweep(ev, d, w)
    if stats is not None:
        stats.setdefault("segments", []).append(n)
        stats.setdefault("gaps", []).append((n, float(vals[1]), float(vals[2] - vals[1]) if n > 2 else np.inf))
        thr, flat = flow_dump.thresholds(ev)
        if not flat:
            masks = ev[None, :] > thr[:, None]
            ref = flow_dump.reference_costs(w, d, masks)
            kr = int(np.argmin(ref))
            tie = any(not np.array_equal(masks[k], masks[kr]) and abs(ref[k] - ref[kr]) <= flow_dump.COST_RTOL * ref[kr]
                      for k in range(flow_dump.NUM_CUTS))
            if tie:
                stats.setdefault("near_ties", []).append(n)
        stats.setdefault("cut" if mcut < T else "refused", []).append(float(mcut))
    if mcut < T:
        return (dense_reference(w[mask][:, mask], n_orig, ids[mask], T, 0.01, stats) +
                dense_reference(w[~mask][:, ~mask], n_orig, ids[~mask], T, 0.01, stats))
    return [ids]


@functools.lru_cache(maxsize=None)
def _reference_of(key):
    kind, a, b = key
    w = limit_case(a) if kind == "limit" else small(a, b)
    n = w.shape[0]
    ids = np.arange(n)
    ds, ms = {}, {}
    dense = dense_reference(w, N_ORIG, ids, T, SPLIT_LIM, ds)
    model = gpu_model.normalized_cut_model(by_value(w), N_ORIG, ids, T=T, split_lim=SPLIT_LIM, stats=ms)
    return dense, model, ds, ms


def reference(kind, name, diagonal=None):
    """(groups of `dense_reference`, groups of `gpu_model.normalized_cut_model` on the matrix's value, their two stats dicts) of
    ('limit', name) or ('small', form, diagonal); computed once per process and shared by the tests, which leave it unchanged."""
    return _reference_of((kind, name, diagonal))


def labels_of(groups, n):
    lab = np.full(n, -1, dtype=np.int32)
    for g, idx in enumerate(groups):
        lab[idx] = g
    assert (lab >= 0).all()
    return lab


def same_groups(a, b):
    """Same groups in the same order (members as sets)."""
    return len(a) == len(b) and all(np.array_equal(np.sort(x), np.sort(y)) for x, y in zip(a, b))
