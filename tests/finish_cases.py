"""Fixtures, a host model and a grid-free truth for the batched chunk finish (``autoinst_amd/csrc/ai_finish.hip``:
`ai_chunk_finish`, rules F1-F7 of ``include/autoinst_hip.h``) at its kernel limits.

Plain NumPy, seeded, no GPU and no library: tests/test_finish_cases.py proves on the CPU that every fixture sits in the regime
its name claims, that the model equals the truth on all of them and that a list of deliberately wrong rules (`MUTANTS`) is each
rejected by the fixtures that claim to; tests/test_gpu_finish_cases.py feeds the device's answers to the same truth.

The limits are READ from the sources (`constants`): a changed constant moves the fixtures with it, and the CPU test proves the
regime claims again.  A pattern that no longer matches raises.

A call is four lists of per-chunk arrays (fine, major, labels, ground).  Model and truth both return the outputs of
`ai_chunk_finish` as one dict of flat arrays (`KEYS`), the shape `test_gpu_finish.c_finish` returns.

* `finish_model` restates the device path: the three tile tables and `tile_chunk`, the chunk table (each chunk's 1-NN grid grown
  under the CALL's cell cap, its kNN grid, `cellbase` / `rowbase`), the two key arrays and a stable sort on the bits `bits_for`
  gives, the runs per cell and per row, the ring searches (`points_cases.nn1_model`, `prep_cases.knn_model` on the chunk's grid),
  `prep_cases.stats_model`, `finish_ref.f4_sum`, the flags, the scan, `keep_off` and the merged layout.
* `finish_truth` has no grid: `finish_ref.nearest_brute`, `prep_cases.knn_avg_exact`, `prep_cases.stats_ref`, `f4_sum` over the
  truth's inliers divided once, one addition for `z_limit`, indexing for F5 / F6.
"""
from __future__ import annotations

import functools
import re
from dataclasses import dataclass, field

import numpy as np

import finish_ref
import points_cases as pts
import prep_cases as pc

EMPTY = np.zeros((0, 3))
NOLABEL = np.zeros(0, np.int32)
KEYS = ("fine_nn", "fine_dist", "fine_label", "ground_avg", "ground_keep", "keep_off", "ground_stats", "merged_xyz", "merged_label",
        "merged_off")
FILL_I, FILL_D = -9, np.nan            # what the model leaves in a row no thread wrote
MODEL_MAX = 4096                       # the ring-by-ring kNN model forms an n x n matrix: larger chunks take `avg_of`


# ------------------------------------------------------------------------------------------------- constants from the sources
def constants():
    """The limits of `ai_chunk_finish`, parsed out of ``ai_common.h`` and ``ai_finish.hip``."""
    common, fin = pc._read(pc._CSRC, "ai_common.h"), pc._read(pc._CSRC, "ai_finish.hip")
    ka, kb, kc, kd, ke = pc._groups(fin, r"if \(k_max <= (\d+)\)\s*hipLaunchKernelGGL\(kf_knn_avg<(\d+)>, KF_ARGS\);\s*else if \(k_max <= (\d+)\)\s*"
                                    r"hipLaunchKernelGGL\(kf_knn_avg<(\d+)>, KF_ARGS\);\s*else\s*hipLaunchKernelGGL\(kf_knn_avg<(\d+)>",
                                    "the template instances of kf_knn_avg and their k_max switch")
    if ka != kb or kc != kd:
        raise RuntimeError("an instance of kf_knn_avg no longer serves k_max up to its own length")
    if not re.search(r"ch\.k = \(int32_t\)std::min<int64_t>\(nb_neighbors, ch\.ng\);\s*k_max = std::max\(k_max, ch\.k\);", fin):
        raise RuntimeError("the chunk's k is no longer min(nb_neighbors, ng), k_max its maximum")
    kmax, nmax = pc._groups(fin, r"nb_neighbors > (\d+) && ng_max > (\d+)", "the largest k of ai_chunk_finish")
    if not (int(kmax) == int(nmax) == int(ke)):
        raise RuntimeError("the largest k is no longer the longest instance of kf_knn_avg")
    floor_, cap_bits = pc._groups(fin, r"cell_cap = std::max\(([0-9.]+), \(double\)\(\(int64_t\)1 << (\d+)\) / \(double\)std::max\(nch, 1\)\);",
                                  "the per-chunk cell cap")
    grows = re.findall(r"^\s*cell \*= ([0-9.]+);", fin, re.M)
    if len(grows) != 2:
        raise RuntimeError("ai_chunk_finish no longer has one growth loop per grid")
    fin_s = re.search(r"void kf_nn1\(.*?\n\}", fin, re.S)
    knn_s = re.search(r"void kf_knn_avg\(.*?\n\}", fin, re.S)
    if not fin_s or not knn_s:
        raise RuntimeError("kf_nn1 / kf_knn_avg not found in the sources")
    c = dict(AI_BLOCK=int(pc._find(common, r"^\s*#define\s+AI_BLOCK\s+(\d+)", "AI_BLOCK")),
             BB=int(pc._find(fin, r"constexpr int BB = (\d+);", "BB")),
             RED_BLOCKS=int(pc._find(fin, r"constexpr int RED_BLOCKS = (\d+);", "RED_BLOCKS")),
             NSTAT=int(pc._find(fin, r"constexpr int NSTAT = (\d+);", "NSTAT")),
             KNN_LENGTHS=(int(ka), int(kc), int(ke)),
             CAP_FLOOR=float(floor_), CAP_TOTAL=1 << int(cap_bits),
             NN1_CELL=float(pc._find(fin, r"double cell = ([0-9.]+);\s*for \(;;\) \{\s*const double ex", "the first cell of the 1-NN grid")),
             GROW=float(grows[0]), KNN_GROW=float(grows[1]),
             MAX_CHUNKS=int(pc._find(fin, r"n_chunks < 0 \|\| n_chunks > (\d+)\)", "the chunk limit")),
             MAX_ROWS=1 << int(pc._find(fin, r"off\[n\] >= \(\(int64_t\)1 << (\d+)\)\)", "the row limit")),
             EXTENT_LIMIT=float(pc._find(fin, r"mx\[a\] - mn\[a\] < ([0-9.e+]+)\)", "the extent limit of chunk_bounds")),
             NN1_STOP=pc.stop_constants(fin_s.group(0), "cell", "best", "kf_nn1"),
             KNN_STOP=pc.stop_constants(knn_s.group(0), r"g\.cell", "kth", "kf_knn_avg"))
    if c["AI_BLOCK"] % 64 or c["RED_BLOCKS"] != c["AI_BLOCK"]:
        raise RuntimeError("kf_finish no longer takes one partial per thread of a block of whole waves")
    if c["KNN_LENGTHS"] != pc.KNN_LENGTHS or c["KNN_GROW"] != pc.K["GROW"] or c["KNN_STOP"] != (pc.K["SLACK_ULPS"], pc.K["STOP_ULPS"]):
        raise RuntimeError("kf_knn_avg no longer has kq_knn_avg's instances, growth factor and stop rule (prep_cases models them)")
    if c["NN1_CELL"] != pts.NN1_CELL or c["GROW"] != pts.GROW or c["NN1_STOP"] != (pts.K["SLACK_ULPS"], pts.K["STOP_ULPS"]):
        raise RuntimeError("kf_nn1 no longer has kp_nn1's cell, growth factor and stop rule (points_cases models them)")
    if c["RED_BLOCKS"] * c["AI_BLOCK"] != 65536:
        raise RuntimeError("a lap of kf_zpartial is no longer the 65536 rows finish_ref.f4_sum restates")
    return c


K = constants()
BLOCK = K["AI_BLOCK"]
BB = K["BB"]
NSTAT = K["NSTAT"]
LAP = K["RED_BLOCKS"] * BLOCK
MAX_CHUNKS = K["MAX_CHUNKS"]
KNN_LENGTHS = K["KNN_LENGTHS"]


def cell_cap(n_chunks, mutant=None):
    """Dense cells a chunk's 1-NN grid may take in a call of ``n_chunks``."""
    return max(K["CAP_FLOOR"], float(K["CAP_TOTAL"]) / float(max(1 if mutant == "cap_of_one_call" else n_chunks, 1)))


# ------------------------------------------------------------------------------------------------- tiles
def tiles_of(sizes, mutant=None):
    """`tiles_of`: tstart[c + 1] = tstart[c] + ceil(n_c / AI_BLOCK).  ``tile_floor`` forgets the partial tile."""
    n = np.asarray(sizes, np.int64)
    per = n // BLOCK if mutant == "tile_floor" else (n + BLOCK - 1) // BLOCK
    return np.concatenate([[0], np.cumsum(per)]).astype(np.int64)


def tile_chunk(tstart, nch, blocks, mutant=None):
    """`tile_chunk`'s binary search for every block at once: the largest c in [0, nch) with tstart[c] <= block.
    ``tile_chunk_first`` answers the FIRST chunk that starts at that tile: an empty chunk in front of the right one."""
    blocks = np.asarray(blocks, np.int64)
    a, b = np.zeros_like(blocks), np.full_like(blocks, nch)
    while ((b - a) > 1).any():
        m = (a + b) >> 1
        go = (b - a) > 1
        le = tstart[m] <= blocks
        a, b = np.where(go & le, m, a), np.where(go & ~le, m, b)
    if mutant == "tile_chunk_first":
        a = np.searchsorted(tstart[:nch], tstart[a], side="left")
    return a


def covered_rows(sizes, mutant=None):
    """bool per row of the concatenated cloud: some thread of a tile-mapped kernel takes it (with its own chunk's record; under
    both wrong rules a row is either taken by its own chunk or by none)."""
    sizes = np.asarray(sizes, np.int64)
    nch = sizes.shape[0]
    off = np.concatenate([[0], np.cumsum(sizes)])
    t = tiles_of(sizes, mutant)
    out = np.zeros(int(off[-1]), bool)
    if nch == 0 or t[-1] == 0:
        return out
    blocks = np.arange(int(t[-1]), dtype=np.int64)
    c = tile_chunk(t, nch, blocks, mutant)
    local = (blocks - t[c])[:, None] * BLOCK + np.arange(BLOCK)[None, :]
    ok = local < sizes[c][:, None]
    out[(off[c][:, None] + local)[ok]] = True
    return out


# ------------------------------------------------------------------------------------------------- the chunk table
def nn1_cell(major, cap):
    """(cell, steps, (nx, ny, nz)) of a chunk's 1-NN grid: NN1_CELL, grown by GROW until the dense table fits ``cap``."""
    mn, mx = major.min(axis=0), major.max(axis=0)
    cell, steps = K["NN1_CELL"], 0
    while True:
        e = np.floor((mx - mn) / cell) + 1.0
        if (e[0] * e[1]) * e[2] <= cap:
            break
        cell *= K["GROW"]
        steps += 1
    return cell, steps, (np.floor((mx - mn) / cell).astype(np.int64) + 1)


def _sorted_runs(key, bits, shift=0):
    """A stable sort on the low ``bits`` bits (the keys come out whole, as the radix sort returns them) and the runs the gather
    kernels write, one per value of ``key >> shift`` (a cell; a row): (order, sorted keys, the values whose entries do NOT lie in
    one piece -- the gather kernels take a run's start and end from the changes of the sorted keys, so such a cell or row loses
    entries)."""
    key = np.asarray(key, np.uint64)
    mask = np.uint64((1 << bits) - 1)
    order = np.argsort(key & mask, kind="stable")
    skey = key[order]
    run = skey >> np.uint64(shift)
    starts = np.concatenate([[0], np.flatnonzero(run[1:] != run[:-1]) + 1]) if run.size else np.zeros(0, np.int64)
    values, pieces = np.unique(run[starts], return_counts=True)
    return order, skey, values[pieces > 1]


MUTANTS = ("tile_floor", "tile_chunk_first", "k_is_kmax", "k_is_nb", "cap_of_one_call", "key_bits_short", "slot_by_rank",
           "keep_global_index", "ground_first", "mean_all", "le", "keep_in_inliers", "tie_larger", "no_plus_one", "neighbour_chunk")
NO_OP_MUTANTS = ("cap_of_one_call",)       # must change no result: a coarser 1-NN grid gives the same nearest point


def _sizes(parts):
    return np.array([np.asarray(a).reshape(-1, 3).shape[0] for a in parts], np.int64)


def _cat(parts, width, dtype):
    parts = [np.asarray(a, dtype=dtype).reshape((-1, width) if width else -1) for a in parts if np.asarray(a).size]
    return np.concatenate(parts) if parts else np.zeros((0, width) if width else 0, dtype)


def finish_model(fine, major, labels, ground, nb, std_ratio, mean_height, mutant=None, *, avg_of=None):
    """`ai_chunk_finish` on the CPU, step for step (module docstring): the dict of `KEYS`, and under ``"table"`` what the CPU test
    reads the regime claims from (tiles, k, instance, cap, growth steps, cell and row sums, key bits).
    ``avg_of``: {chunk: avg} for ground chunks above `MODEL_MAX` rows, whose n x n ring model would not fit: the kNN is exact
    (proven by the model on every smaller fixture), so there the grid-free averages stand in for the search.
    ``mutant``: one of `MUTANTS`.  Where a wrong rule lets a thread read another chunk's rows or leaves rows unwritten the model
    does not follow the garbage: the rows keep `FILL_I` / `FILL_D`, which no truth holds."""
    nch = len(ground)
    nf, nm, ng = _sizes(fine), _sizes(major), _sizes(ground)
    foff, moff, goff = (np.concatenate([[0], np.cumsum(s)]).astype(np.int64) for s in (nf, nm, ng))
    Nf, Nm, Ng = int(foff[-1]), int(moff[-1]), int(goff[-1])
    F, M, G = _cat(fine, 3, np.float64), _cat(major, 3, np.float64), _cat(ground, 3, np.float64)
    L = _cat(labels, 0, np.int32)
    if ((nf > 0) & (nm == 0)).any():
        raise ValueError("a chunk with fine points and no major points")
    cov_f, cov_m, cov_g = (covered_rows(s, mutant) for s in (nf, nm, ng))
    # ---- the chunk table
    k = np.minimum(nb, ng)
    k_max = int(k.max()) if nch else 0
    if int(nb) > KNN_LENGTHS[-1] and ng.max(initial=0) > KNN_LENGTHS[-1]:
        raise ValueError("nb_neighbors > 64 is not supported")
    instance = pc.knn_instance(max(k_max, 1))
    if mutant == "k_is_kmax":
        k = np.where(ng > 0, k_max, 0)
    elif mutant == "k_is_nb":
        k = np.where(ng > 0, nb, 0)
    cap = cell_cap(nch, mutant)
    pcell, psteps, pn = np.zeros(nch), np.zeros(nch, np.int64), np.zeros((nch, 3), np.int64)
    cellbase, rowbase = np.zeros(nch + 1, np.int64), np.zeros(nch + 1, np.int64)
    kgrid = {}
    some_m, some_g, some_f = np.flatnonzero(nm), np.flatnonzero(ng), np.flatnonzero(nf)
    ncells, nrows = np.zeros(nch, np.int64), np.zeros(nch, np.int64)
    for c in some_m:
        pcell[c], psteps[c], pn[c] = nn1_cell(M[moff[c]:moff[c + 1]], cap)
        ncells[c] = int(pn[c].prod())
    for c in some_g:
        kgrid[c] = pc.knn_grid(G[goff[c]:goff[c + 1]])
        nrows[c] = kgrid[c].rows
    cellbase[1:], rowbase[1:] = np.cumsum(ncells), np.cumsum(nrows)
    ncell, nrow = int(cellbase[-1]), int(rowbase[-1])
    short = 1 if mutant == "key_bits_short" else 0
    mbits = max(1, pc.bits_for(ncell)) - short
    gbits = 32 + max(1, pc.bits_for(nrow)) - short
    # ---- F2: keys, sort, runs, search
    fine_nn, fine_dist, fine_label = np.full(Nf, FILL_I, np.int32), np.full(Nf, FILL_D), np.full(Nf, FILL_I, np.int32)
    mkey = np.zeros(Nm, np.uint64)
    for c in some_m:
        g = pts.Grid(M[moff[c]:moff[c + 1]].min(axis=0)[None], M[moff[c]:moff[c + 1]].max(axis=0)[None], np.array([pcell[c]]),
                     K["NN1_CELL"], pn[c][None])
        cc = pts.cells_of(g, M[moff[c]:moff[c + 1]][None])[0]
        mkey[moff[c]:moff[c + 1]] = cellbase[c] + (cc[:, 2] * pn[c][1] + cc[:, 1]) * pn[c][0] + cc[:, 0]
    morder, mskey, m_split = _sorted_runs(mkey[cov_m], mbits)
    mrows = np.flatnonzero(cov_m)[morder]                 # the major row behind every sorted entry
    for c in some_f:
        # a cell's run is found through the WHOLE key: while every cell's entries lie in one piece the chunk's cells hold the chunk's
        # covered rows, whatever the sort order; a chunk with a cell in pieces is not followed (its rows keep the fill value)
        if ((m_split >= np.uint64(cellbase[c])) & (m_split < np.uint64(cellbase[c + 1]))).any():
            continue
        own = mrows[(mskey >= np.uint64(cellbase[c])) & (mskey < np.uint64(cellbase[c + 1]))]
        own = np.sort(own)
        rows = np.flatnonzero(cov_f[foff[c]:foff[c + 1]]) + foff[c]
        if not rows.size or not own.size:
            continue
        if mutant == "neighbour_chunk":
            idx, dist, _ = finish_ref.nearest_brute(F[rows], M)
            fine_nn[rows], fine_dist[rows], fine_label[rows] = idx - moff[c], dist, L[idx]
            continue
        if own.size == nm[c]:
            idx, dist, _ = pts.nn1_model(F[rows], M[own], cell=pcell[c], mutant="ties_larger" if mutant == "tie_larger" else None)
        else:                                             # rows a wrong tile table left out of the cell list: the rest, exactly
            idx, dist, _ = finish_ref.nearest_brute(F[rows], M[own], mutant == "tie_larger")
        fine_nn[rows], fine_dist[rows], fine_label[rows] = own[idx] - moff[c], dist, L[own[idx]]
    # ---- F3: keys, sort, runs, search
    avg = np.full(Ng, FILL_D)
    gkey = np.zeros(Ng, np.uint64)
    for c in some_g:
        g = kgrid[c]
        cc = pc.kcells(g, G[goff[c]:goff[c + 1]])
        gkey[goff[c]:goff[c + 1]] = ((rowbase[c] + cc[:, 2] * g.n[1] + cc[:, 1]).astype(np.uint64) << np.uint64(32)) | cc[:, 0].astype(np.uint64)
    gorder, gskey, g_split = _sorted_runs(gkey, gbits, 32)    # uncovered rows hold no key of their own; they are found out below
    for c in some_g:
        # thread p of the chunk serves the sorted entry goff + p: the chunk's own rows, if the keys kept the chunks apart
        served = gorder[goff[c]:goff[c + 1]]
        if not (cov_g[goff[c]:goff[c + 1]].all() and np.array_equal(np.sort(served), np.arange(goff[c], goff[c + 1]))):
            continue
        if k[c] > ng[c]:
            avg[goff[c]:goff[c + 1]] = np.inf             # the list never fills: the sum holds an empty slot
        elif avg_of is not None and c in avg_of and k[c] == min(nb, ng[c]):
            avg[goff[c]:goff[c + 1]] = avg_of[c]
        elif ng[c] > MODEL_MAX:
            raise ValueError(f"chunk {c}: {ng[c]} ground rows are too many for the ring model; pass avg_of")
        else:
            avg[goff[c]:goff[c + 1]] = pc.knn_model(G[goff[c]:goff[c + 1]], int(k[c]), grid=kgrid[c])["avg"]
    # ---- statistics, F4, F5
    stats = np.full((nch, NSTAT), np.nan)
    stats[:, 3] = 0.0
    flag = np.zeros(Ng, bool)
    with np.errstate(invalid="ignore", divide="ignore"):
        for c in some_g:
            a, z = avg[goff[c]:goff[c + 1]], G[goff[c]:goff[c + 1], 2]
            st = pc.stats_model(a, std_ratio)
            inl = (a > 0) & (a < st["threshold"])
            cnt = float(inl.sum())
            if mutant == "mean_all":
                mz = np.float64(finish_ref.f4_sum(z, np.ones(z.size, bool))) / np.float64(z.size)
            elif mutant == "slot_by_rank":
                mz = np.float64(finish_ref.f4_sum(z[inl], np.ones(int(cnt), bool))) / np.float64(cnt)
            else:
                mz = np.float64(finish_ref.f4_sum(z, inl)) / np.float64(cnt)
            lim = mz + np.float64(mean_height)
            stats[c] = st["mean"], st["std"], st["threshold"], cnt, mz, lim
            below = (z <= lim) if mutant == "le" else (z < lim)
            if mutant == "keep_in_inliers":
                kept = np.zeros(z.size, bool)
                kept[np.flatnonzero(below[inl])] = True
            else:
                kept = inl & below
            flag[goff[c]:goff[c + 1]] = kept & cov_g[goff[c]:goff[c + 1]]
    # ---- the scan, F5 / F6
    pos = np.concatenate([[0], np.cumsum(flag)]).astype(np.int64)
    keep_off = pos[goff]
    rows = np.flatnonzero(flag)
    chunk_of = np.searchsorted(goff, rows, side="right") - 1
    ground_keep = (rows if mutant == "keep_global_index" else rows - goff[chunk_of]).astype(np.int32)
    merged_off = foff + keep_off
    mx, ml = np.full((Nf + rows.size, 3), FILL_D), np.full(Nf + rows.size, FILL_I, np.int32)
    frow = np.flatnonzero(cov_f)
    fchunk = np.searchsorted(foff, frow, side="right") - 1
    if mutant == "ground_first":
        fd = frow + keep_off[fchunk + 1]
        gd = foff[chunk_of] + np.arange(rows.size)
    else:
        fd = frow + keep_off[fchunk]
        gd = foff[chunk_of] + nf[chunk_of] + np.arange(rows.size)
    mx[fd], ml[fd] = F[frow], fine_label[frow] + (0 if mutant == "no_plus_one" else 1)
    mx[gd], ml[gd] = G[rows], 0
    table = dict(tiles=tuple(int(tiles_of(s)[-1]) for s in (nf, nm, ng)), k=k, k_max=k_max, instance=instance, cap=cap, pcell=pcell,
                 psteps=psteps, pn=pn, ncell=ncell, nrow=nrow, mbits=mbits, gbits=gbits, cellbase=cellbase, rowbase=rowbase,
                 kgrid=kgrid, mkey=mkey, gkey=gkey, runs_whole=(m_split.size == 0, g_split.size == 0))
    return {"fine_nn": fine_nn, "fine_dist": fine_dist, "fine_label": fine_label, "ground_avg": avg, "ground_keep": ground_keep,
            "keep_off": keep_off, "ground_stats": stats, "merged_xyz": mx, "merged_label": ml, "merged_off": merged_off, "table": table}


def finish_truth(fine, major, labels, ground, nb, std_ratio, mean_height, *, groups=None):
    """The grid-free truth (module docstring): the dict of `KEYS`; ``ground_stats`` holds `stats_ref`'s mean, std and threshold
    (to be met within `prep_cases.stats_bound`) and the exact n_inliers, mean_z and z_limit.  Under ``"per_chunk"``, for every
    chunk with rows: tied (fine points with two nearest majors), near (averages within the bound of the threshold), inliers.
    ``groups``: {chunk: group ids} for `knn_avg_exact`."""
    nch = len(ground)
    nf, ng = _sizes(fine), _sizes(ground)
    foff, goff = (np.concatenate([[0], np.cumsum(s)]).astype(np.int64) for s in (nf, ng))
    nn, dist, lab, avg, keep, mxyz, mlab = [], [], [], [], [], [], []
    stats = np.full((nch, NSTAT), np.nan)
    stats[:, 3] = 0.0
    keep_n = np.zeros(nch, np.int64)
    per = {}
    for c in np.flatnonzero((nf > 0) | (ng > 0)):
        f, m, g = (np.asarray(a, np.float64).reshape(-1, 3) for a in (fine[c], major[c], ground[c]))
        info = per.setdefault(int(c), {})
        lc = np.zeros(0, np.int32)
        if f.shape[0]:
            i, d, tied = finish_ref.nearest_brute(f, m)
            lc = np.asarray(labels[c], np.int32).reshape(-1)[i]
            nn.append(i.astype(np.int32)), dist.append(d), lab.append(lc)
            info["tied"] = int((tied > 0).sum())
        mxyz.append(f), mlab.append(lc + 1)
        if g.shape[0]:
            a = pc.knn_avg_exact(g, nb, None if groups is None else groups.get(int(c)))
            ref = pc.stats_ref(a, std_ratio)
            inl = np.zeros(g.shape[0], bool)
            inl[ref["keep"]] = True
            with np.errstate(invalid="ignore", divide="ignore"):
                mz = np.float64(finish_ref.f4_sum(g[:, 2], inl)) / np.float64(inl.sum())
                lim = mz + np.float64(mean_height)
                kc = np.flatnonzero(inl & (g[:, 2] < lim))
            stats[c] = ref["mean"], ref["std"], ref["threshold"], float(inl.sum()), mz, lim
            avg.append(a), keep.append(kc.astype(np.int32)), mxyz.append(g[kc]), mlab.append(np.zeros(kc.size, np.int32))
            keep_n[c] = kc.size
            info.update(avg=a, inliers=inl, near=pc.near_threshold(a, std_ratio) if g.shape[0] > 1 else np.zeros(0, np.int64),
                        bound=pc.stats_bound(a, std_ratio))
    keep_off = np.concatenate([[0], np.cumsum(keep_n)]).astype(np.int64)

    def cat(parts, width, dtype):
        return np.concatenate(parts).astype(dtype) if parts else np.zeros((0, width) if width else 0, dtype)
    return {"fine_nn": cat(nn, 0, np.int32), "fine_dist": cat(dist, 0, np.float64), "fine_label": cat(lab, 0, np.int32),
            "ground_avg": cat(avg, 0, np.float64), "ground_keep": cat(keep, 0, np.int32), "keep_off": keep_off, "ground_stats": stats,
            "merged_xyz": cat(mxyz, 3, np.float64), "merged_label": cat(mlab, 0, np.int32), "merged_off": foff + keep_off, "per_chunk": per}


# ------------------------------------------------------------------------------------------------- comparing
def same_bits(a, b):
    """Equal shape and equal bits; two NaN count as equal whatever their sign and payload (0 / 0 has the sign bit set on the
    device and not in NumPy)."""
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    if a.shape != b.shape or a.dtype != b.dtype:
        return False
    if a.dtype.kind != "f":
        return bool((a == b).all())
    nan = np.isnan(a) & np.isnan(b)
    return bool((nan | (a.view(np.int64) == b.view(np.int64))).all())


def differences(got, truth, per_chunk, *, stats_exact=False, keys=KEYS):
    """The list of `KEYS` in which ``got`` (a model's or the device's dict) is not the truth: every array bit for bit, but mean,
    std and threshold (columns 0-2 of ground_stats) within `prep_cases.stats_bound` of the ``math.fsum`` reference."""
    bad = []
    for key in keys:
        if key not in got:
            bad.append(f"{key} (missing)")
            continue
        if key != "ground_stats":
            if not same_bits(got[key], truth[key]):
                bad.append(key)
            continue
        g, t = np.asarray(got[key]), np.asarray(truth[key])
        if g.shape != t.shape or not same_bits(g[:, 3:], t[:, 3:]):
            bad.append(key)
            continue
        for c in range(g.shape[0]):
            bound = per_chunk.get(c, {}).get("bound")
            for j, name in enumerate(("mean", "std", "threshold")):
                x, y = g[c, j], t[c, j]
                if np.isnan(y) or np.isnan(x):
                    ok = np.isnan(x) and np.isnan(y)
                else:
                    ok = bound is not None and abs(x - y) <= bound[name]
                if not ok:
                    bad.append(f"{key}[{c}].{name}")
    return bad


# ------------------------------------------------------------------------------------------------- fixtures
@dataclass
class FinishCase:
    name: str
    fine: list
    major: list
    labels: list
    ground: list
    nb: int = 20
    std_ratio: float = 2.0
    mean_height: float = 0.6
    rejects: tuple = ()                       # the mutants of the model this fixture tells from the truth
    claims: dict = field(default_factory=dict)
    groups: dict | None = None                # {chunk: group ids} of `knn_avg_exact`
    on_threshold: tuple = ()                  # chunks BUILT with averages on the threshold
    tie_chunks: tuple = ()                    # chunks BUILT with fine points between two majors

    @property
    def n_chunks(self):
        return len(self.ground)

    @property
    def args(self):
        return self.fine, self.major, self.labels, self.ground

    @functools.cached_property
    def occupied(self):
        return [int(c) for c in np.flatnonzero((_sizes(self.fine) > 0) | (_sizes(self.major) > 0) | (_sizes(self.ground) > 0))]

    @functools.cached_property
    def truth(self):
        return finish_truth(*self.args, self.nb, self.std_ratio, self.mean_height, groups=self.groups)

    def avg_of(self):
        """The truth's averages of the chunks the ring model cannot hold."""
        goff = np.concatenate([[0], np.cumsum(_sizes(self.ground))])
        return {c: self.truth["ground_avg"][goff[c]:goff[c + 1]] for c in range(self.n_chunks) if goff[c + 1] - goff[c] > MODEL_MAX}

    @functools.lru_cache(maxsize=None)
    def model(self, mutant=None):
        return finish_model(*self.args, self.nb, self.std_ratio, self.mean_height, mutant, avg_of=self.avg_of())

    def __hash__(self):
        return hash(self.name)

    def __eq__(self, other):
        return self is other


def _labels(rng, major):
    return [rng.integers(0, 50, np.asarray(m).reshape(-1, 3).shape[0]).astype(np.int32) for m in major]


def _cloud(rng, n, lo=(0.0, 0.0, 0.0), side=(6.0, 6.0, 1.5)):
    return np.asarray(lo) + rng.random((n, 3)) * np.asarray(side)


def _ground(rng, n, lo=(0.0, 0.0, 0.0), side=None):
    """A patch of ground with a step: a tenth of the points 0.9 m up (the height cut has something to cut) and a few far above
    (the outlier filter has something to remove)."""
    s = max(np.sqrt(n) * 0.1, 0.5) if side is None else side
    p = np.asarray(lo) + rng.random((n, 3)) * [s, s, 0.04]
    p[: n // 10, 2] += 0.9
    p[n // 10: n // 10 + n // 50, 2] += rng.uniform(2.0, 6.0, n // 50)
    return p[rng.permutation(n)]


TILE_SIZES = (0, 1, BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK - 1, 2 * BLOCK, 2 * BLOCK + 1)
TILE_EMPTY = {"fine": ((0, 1, 2), (9, 10, 11), (21, 22, 23)), "major": ((0, 1), (10, 11), (22, 23)),
              "ground": ((0, 1), (5, 6, 7), (21, 22, 23))}


@functools.lru_cache(maxsize=None)
def tiles_case():
    """24 chunks whose three sizes are drawn independently from `TILE_SIZES`; runs of two and three empty chunks at the front, in
    the middle and at the end, elsewhere for each cloud (`TILE_EMPTY`); the chunk behind every empty run has 255, 256 or 257 rows
    in turn.  A chunk with fine points has major points."""
    rng = np.random.default_rng(5201)
    nch = 24
    size = {kind: rng.choice(TILE_SIZES[1:], nch) for kind in ("fine", "major", "ground")}
    turn = 0
    for kind, runs in TILE_EMPTY.items():
        for run in runs:
            size[kind][list(run)] = 0
            if run[-1] + 1 < nch:
                size[kind][run[-1] + 1] = (BLOCK - 1, BLOCK, BLOCK + 1)[turn % 3]
                turn += 1
    for kind, runs in TILE_EMPTY.items():            # a follower of one cloud's run must not fill another cloud's run
        for run in runs:
            size[kind][list(run)] = 0
    size["fine"][size["major"] == 0] = 0
    followers = {run[-1] + 1 for runs in TILE_EMPTY.values() for run in runs}
    for kind in ("major", "ground", "fine"):          # every size of the set occurs in every cloud: a size drawn twice makes room
        for s in TILE_SIZES:
            if s in size[kind]:
                continue
            free = [c for c in range(nch) if size[kind][c] > 0 and c not in followers and (size[kind] == size[kind][c]).sum() > 1
                    and (kind != "fine" or size["major"][c] > 0)]
            size[kind][free[0]] = s
        assert not [s for s in TILE_SIZES if s not in size[kind]], kind
    fine = [_cloud(rng, n, (c * 3.0, 0.0, 0.0)) for c, n in enumerate(size["fine"])]
    major = [_cloud(rng, n, (c * 3.0, 0.0, 0.0)) for c, n in enumerate(size["major"])]      # chunks overlap by half (F1)
    ground = [_ground(rng, n, (c * 3.0, 0.0, -1.0), side=6.0) for c, n in enumerate(size["ground"])]
    return FinishCase("tiles", fine, major, _labels(rng, major), ground,
                      rejects=("tile_floor", "tile_chunk_first", "keep_global_index", "ground_first", "no_plus_one", "neighbour_chunk",
                               "k_is_nb", "mean_all", "keep_in_inliers"),
                      claims=dict(sizes={k: tuple(int(x) for x in v) for k, v in size.items()}))


MIXED_NB = (1, 2, KNN_LENGTHS[0] - 1, KNN_LENGTHS[0], KNN_LENGTHS[0] + 1, KNN_LENGTHS[1], KNN_LENGTHS[1] + 1, KNN_LENGTHS[2] - 1,
            KNN_LENGTHS[2])


@functools.lru_cache(maxsize=None)
def mixed_k_case(nb):
    """Ground chunks of 1, 2, 12, nb - 1, nb, nb + 1 and 300 points in one call (sizes below 1 dropped, doubles kept): k differs
    per chunk and the instance is the one the longest k needs.  ``nb = 100``: every chunk has at most 64 points, k = n."""
    rng = np.random.default_rng(5300 + nb)
    sizes = [1, 2, 12, nb - 1, nb, nb + 1, 300] if nb <= KNN_LENGTHS[-1] else [1, 2, 12, 33, 63, 64]
    sizes = [n for n in sizes if n >= 1]
    ground = [_ground(rng, n, (c * 2.0, 0.0, 0.0), side=4.0) for c, n in enumerate(sizes)]
    major = [_cloud(rng, 40, (c * 2.0, 0.0, 0.5)) for c in range(len(sizes))]
    fine = [_cloud(rng, 70, (c * 2.0, 0.0, 0.5)) for c in range(len(sizes))]
    rejects = ("k_is_kmax", "k_is_nb") if nb > 2 else ("k_is_nb",) if nb == 2 else ()       # nb = 1: every average is 0
    return FinishCase(f"mixed_k_nb{nb}", fine, major, _labels(rng, major), ground, nb=nb, rejects=rejects,
                      on_threshold=tuple(c for c, n in enumerate(sizes) if n == 2 and nb >= 2),     # two points: two equal averages, std 0
                      claims=dict(sizes=tuple(sizes), k=tuple(min(nb, n) for n in sizes),
                                  instance=pc.knn_instance(min(nb, max(sizes)))))


GROWN_CHUNKS = 4096
GROWN_SIDES = ((15.0, 15.0, 15.0), (22.0, 22.0, 22.0), (34.0, 34.0, 34.0), (100.0, 100.0, 0.9))     # growth steps 0, 1, 2, 2
GROWN_AT = (7, 1000, 2047, 4095)


def _sparse(nch, at, parts, empty):
    out = [empty] * nch
    for c, a in zip(at, parts):
        out[c] = a
    return out


@functools.lru_cache(maxsize=None)
def many_chunks_grown_case():
    """4096 chunks, four with points: under the cap 2^27 / 4096 = 32768 cells their major boxes (`GROWN_SIDES`) take 0, 1, 2 and
    2 growth steps where each alone keeps 0.5 m cells.  200 majors each (the box corners among them), 300 fine points inside
    the box and up to 100 m outside it (their cells are clamped), 150 ground points."""
    rng = np.random.default_rng(5401)
    major, fine, ground = [], [], []
    for j, side in enumerate(GROWN_SIDES):
        lo = np.array([j * 10.0, -5.0, 1.0])
        m = _cloud(rng, 200, lo, side)
        m[0], m[1] = lo, lo + side
        major.append(m)
        f = _cloud(rng, 300, lo, side)
        f[150:] = lo + rng.uniform(-100.0, 100.0 + np.asarray(side), (150, 3))
        fine.append(f)
        ground.append(_ground(rng, 150, lo))
    return FinishCase("many_chunks_grown", _sparse(GROWN_CHUNKS, GROWN_AT, fine, EMPTY), _sparse(GROWN_CHUNKS, GROWN_AT, major, EMPTY),
                      _sparse(GROWN_CHUNKS, GROWN_AT, _labels(rng, major), NOLABEL), _sparse(GROWN_CHUNKS, GROWN_AT, ground, EMPTY),
                      rejects=("tile_chunk_first", "keep_global_index", "neighbour_chunk"), claims=dict(steps=(0, 1, 2, 2)))


def _limit_case(name, nch, at, seed):
    rng = np.random.default_rng(seed)
    major = [_cloud(rng, n, (j * 2.0, 0.0, 0.0)) for j, n in enumerate((30, 257, 12))]
    fine = [_cloud(rng, n, (j * 2.0, 0.0, 0.0)) for j, n in enumerate((100, 300, 257))]
    ground = [_ground(rng, n, (j * 2.0, 0.0, -1.0), side=4.0) for j, n in enumerate((257, 40, 300))]
    return FinishCase(name, _sparse(nch, at, fine, EMPTY), _sparse(nch, at, major, EMPTY), _sparse(nch, at, _labels(rng, major), NOLABEL),
                      _sparse(nch, at, ground, EMPTY), rejects=("tile_chunk_first", "keep_global_index"), claims=dict(at=tuple(at)))


@functools.lru_cache(maxsize=None)
def chunk_limit_case():
    """n_chunks = 65535, the y limit of a grid (`kf_bounds`, `kf_partial`, `kf_zpartial`): three small chunks at 0, 30000, 65534."""
    return _limit_case("chunk_limit", MAX_CHUNKS, (0, 30000, MAX_CHUNKS - 1), 5501)


def _box_points(rng, n, counts, cell):
    """n points inside a box of exactly ``counts`` cells of ``cell`` with both corners present: the last cell is occupied."""
    ext = (np.asarray(counts, np.float64) - 0.5) * cell
    p = rng.random((n, 3)) * ext
    p[0], p[-1] = 0.0, ext
    return p


@functools.lru_cache(maxsize=None)
def key_bits_case(plus):
    """Σ cells = 2^b + plus and Σ rows = 2^b' + plus (plus 0 or 1), the last chunk's last cell and last row occupied (by its last
    point), and keys that differ only in the top bit INSIDE one chunk, their rows interleaved: sorted one bit short, such cells
    fall into pieces.  plus = 0: major boxes of 8 x 8 x 4 and 16 x 16 x 3 cells of 0.5 m, 256 + 768 = 2^10, the last one with more
    than half of all cells and 2500 points in random order.  plus = 1: one box of 5 x 5 x 41 = 2^10 + 1 cells in the last chunk
    (only keys 0 and 2^10 differ in the top bit alone, so one chunk must hold both), rows 0 and 2 in its first cell, row 1 and the
    last row in its last cell.  The ground grids come out of `knn_grid`, so the last-but-one ground chunk is sought: a line along
    z of as many rows as are missing."""
    rng = np.random.default_rng(5601 + plus)
    if plus:
        box = _box_points(rng, 400, (5, 5, 41), 0.5)
        box[2], box[1] = box[0] + 0.1, box[-1] - 0.1
        major = [EMPTY, EMPTY, EMPTY, box + [0.5, 0.5, 0.5]]
    else:
        major = [_box_points(rng, 60, (8, 8, 4), 0.5), _box_points(rng, 2500, (16, 16, 3), 0.5) + [1.0, 0.5, 0.0]]
    nch = len(major)
    fine = [_cloud(rng, 80, m.min(axis=0) - 0.5, np.ptp(m, axis=0) + 1.0) if len(m) else EMPTY for m in major]
    ground = [_ground(rng, 120, (0.0, 0.0, 0.0), side=5.0), _ground(rng, 150, (1.0, 1.0, 0.0), side=5.0)]
    rows = sum(pc.knn_grid(g).rows for g in ground)
    line = None
    for b in range(pc.bits_for(rows) + 1, 16):                                            # a z line of n points has some 2 n rows
        want = (1 << b) + plus - rows - (1 if plus else 0)                                # plus: a one-row chunk comes last
        for n, step in ((n, step) for n in range(40, 1500) for step in (0.25, 0.3, 0.37, 0.41)):
            p = np.zeros((n, 3))
            p[:, 2] = np.arange(n) * step
            p[:, :2] = [2.0, 2.0]
            if pc.knn_grid(p).rows == want:
                line = p
                break
        if line is not None:
            break
    if line is None:
        raise RuntimeError("no z line with the wanted number of rows")
    ground.append(line)
    if plus:
        ground.append(np.array([[1.0, 1.0, 0.25], [1.0, 1.0, 0.25], [1.0, 1.0, 0.25]]))    # identical points: one row, the last
    while len(ground) < nch:
        ground.append(EMPTY)
    while len(ground) > nch:
        major.append(EMPTY), fine.append(EMPTY)
        nch += 1
    return FinishCase(f"key_bits_plus{plus}", fine, major, _labels(rng, major), ground, rejects=("key_bits_short",), claims=dict(plus=plus))


def _neighbour(rng, cloud, n):
    """An unrelated cloud over the same box (F1: the chunks overlap in space)."""
    c = np.asarray(cloud, np.float64).reshape(-1, 3)
    lo, hi = c.min(axis=0), c.max(axis=0)
    return lo + rng.random((n, 3)) * np.maximum(hi - lo, 0.5)


@functools.lru_cache(maxsize=None)
def ring_stop_case(k, n_chunks=None):
    """The ring-stop clouds of `prep_cases.ring_stop_cases()` with this k as ground, and a share of
    `points_cases.ring_stop_cases()` as fine / major, one chunk each, every one followed by an unrelated chunk over the same box.
    ``n_chunks``: the chunks are spread over a call of that many (the grown variant: `many_chunks_grown`'s cap)."""
    rng = np.random.default_rng(5700 + k)
    knn = [c for c in pc.ring_stop_cases() if c.nb == k]
    nn1 = list(pts.ring_stop_cases())
    nn1 = nn1[: len(nn1) // 2] if k == pc.RING_KS[0] else nn1[len(nn1) // 2:]
    fine, major, ground, names = [], [], [], []
    for j in range(max(len(knn), len(nn1))):
        g = knn[j].points if j < len(knn) else EMPTY
        f, m = (nn1[j].queries, nn1[j].sources) if j < len(nn1) else (EMPTY, EMPTY)
        fine += [f, _neighbour(rng, f, 5) if len(f) else EMPTY]
        major += [m, _neighbour(rng, m, 30) if len(m) else EMPTY]
        ground += [g, _neighbour(rng, g, 40) if len(g) else EMPTY]
        names += [(knn[j].name if j < len(knn) else None, nn1[j].name if j < len(nn1) else None), None]
    name = f"ring_stop_k{k}"
    labels = _labels(rng, major)
    at = None
    if n_chunks is not None:
        at = np.sort(rng.choice(n_chunks, len(ground), replace=False))
        fine, major, labels, ground = (_sparse(n_chunks, at, parts, e) for parts, e in ((fine, EMPTY), (major, EMPTY), (labels, NOLABEL),
                                                                                        (ground, EMPTY)))
        name += "_grown"
    # the 1-NN cases in which B and A are EXACTLY as far from the query: the smaller index decides there
    ties = tuple(int(2 * j if at is None else at[2 * j]) for j, x in enumerate(nn1)
                 if finish_ref.nearest_brute(x.queries, x.sources)[2].any())
    return FinishCase(name, fine, major, labels, ground, nb=k, rejects=("neighbour_chunk",), tie_chunks=ties,
                      claims=dict(names=names, at=None if n_chunks is None else tuple(int(c) for c in at)))


@functools.lru_cache(maxsize=None)
def degenerate_case():
    """Degenerate ground clouds as chunks of one batch (nb = 20): the dyadic cube (8 equal averages: all ON the threshold, no
    inlier, mean_z NaN), k copies of a point, two points (two equal averages), 30 identical points, lines along x, y, z, a plane."""
    rng = np.random.default_rng(5801)
    by = {c.name: c for c in pc.knn_cases()}
    ground = [by["knn_dyadic_cube"].points, by["knn_k_copies"].points, rng.uniform(-1.0, 1.0, (2, 3)),
              np.tile(np.array([[1.5, -2.25, 3.0]]), (30, 1)), by["knn_line_x"].points, by["knn_line_y"].points, by["knn_line_z"].points,
              by["knn_plane_xy"].points]
    assert by["knn_dyadic_cube"].nb == 8 == ground[0].shape[0] and by["knn_k_copies"].nb == 20
    major = [_cloud(rng, 20, g.min(axis=0)) for g in ground]
    fine = [_cloud(rng, 33, g.min(axis=0)) for g in ground]
    return FinishCase("degenerate", fine, major, _labels(rng, major), ground, on_threshold=(0, 2), rejects=("k_is_nb",),
                      claims=dict(no_inlier=(0, 2, 3), zeros={1: 20, 3: 30}))


F4_SIZES = (LAP - 1, LAP, LAP + 1, LAP + 1, LAP + 1 + pc.CLUSTER)


def _plant(p, groups, up, down, extra=()):
    """Non-inliers: the first 20 members (by index) of cluster ``up`` become copies of one point (avg == 0); ``extra`` and the
    first members of cluster ``down``, 20 rows in all, become a line 2 m apart far from everything (a group of its own; avg far
    above the threshold)."""
    p, groups = p.copy(), groups.copy()
    mem = np.flatnonzero(groups == up)
    copies = mem[:20]
    far = np.concatenate([np.flatnonzero(groups == down)[:20 - len(extra)], np.asarray(extra, np.int64)])
    p[copies] = p[mem[100]]
    p[far] = np.stack([np.arange(20) * 2.0, np.full(20, 181.3), np.full(20, 0.37)], 1)
    groups[far] = groups.max() + 1
    return p, groups, np.sort(copies), np.sort(far)


@functools.lru_cache(maxsize=None)
def f4_lap_case():
    """Ground chunks of 65535, 65536 and 65537 rows cut from `prep_cases.second_lap_cloud()`, and that cloud itself.  Every other
    cluster is lifted by 1024 m, the others lowered by 1024 m, and every z leaves the dyadic lattice: neighbouring slots of F4
    hold values of both signs, the partial sums round at 2^-42 and coarser from the first step of the tree on and cancel on
    the way up, so mean_z (a sum of a few thousand, with an ulp far below those roundings) shows which rows shared a wave.
    Non-inliers are planted by `_plant`, as many up as down, at indices all over the first lap; in chunk 3 at index 65536 as
    well, where chunk 2 has an inlier.  Chunk 4 goes 257 rows into the second lap: the cloud's first cluster once more, 128 m
    further on (a cluster of its own, so the truth stays cheap), with the copies planted in IT, at indices above 65536, and the
    far line taken from rows below.  No fine points."""
    rng = np.random.default_rng(5901)
    base, groups = pc.second_lap_cloud()
    again = np.flatnonzero(groups[:LAP] == 0)
    assert again.size == pc.CLUSTER
    base = np.concatenate([base, base[again] + [128.0, 0.0, 0.0]])
    groups = np.concatenate([groups, np.full(again.size, groups.max() + 2)])       # an odd id: lifted
    ground, grp, planted = [], {}, {}
    for c, n in enumerate(F4_SIZES):
        p = base[:n].copy()
        p[:, 2] += np.where(groups[:n] % 2 == 1, 1024.0, -1024.0) + rng.uniform(-0.025, 0.025, n) - 0.487
        p, g, copies, far = _plant(p, groups[:n], groups[-1] if c == 4 else 2 * (100 + c) + 1, 2 * c, (LAP,) if c == 3 else ())
        ground.append(p), grp.update({c: g}), planted.update({c: (copies, far)})
    nch = len(ground)
    return FinishCase("f4_lap", [EMPTY] * nch, [EMPTY] * nch, [NOLABEL] * nch, ground, groups=grp, rejects=("slot_by_rank", "mean_all"),
                      claims=dict(sizes=F4_SIZES, planted=planted))


@functools.lru_cache(maxsize=None)
def strict_z_case():
    """`test_dyadic_limit_is_strict`'s cloud (z in {0, 2^-3} on a 16 x 16 lattice, one point an ulp below 2^-3; std_ratio 100,
    mean_height 2^-4: half of the points sit ON z_limit) as the second of three chunks; the same cloud 4 m and 8.5 m up in the
    other two, so that each chunk has a limit of its own."""
    xx, yy = np.meshgrid(np.arange(16.0), np.arange(16.0), indexing="ij")
    g = np.stack([xx.ravel(), yy.ravel(), ((xx + yy) % 2).ravel() * 0.125], 1)
    g[16, 2] = np.nextafter(0.125, 0.0)
    ground = [g + [0.0, 0.0, 4.0], g, g + [0.0, 0.0, 8.5]]
    return FinishCase("strict_z", [EMPTY] * 3, [EMPTY] * 3, [NOLABEL] * 3, ground, std_ratio=100.0, mean_height=0.0625, rejects=("le",),
                      claims=dict(limits=(4.125, 0.125, 8.625), kept=(128, 129, 128)))


@functools.lru_cache(maxsize=None)
def ties_case():
    """Exact midpoints of two and four majors on dyadic coordinates, as the middle of three chunks: the smaller index wins."""
    rng = np.random.default_rng(6001)
    maj = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 2.0, 0], [2.0, 2.0, 0], [1.0, 1.0, 4.0], [0.0, 0.0, 0.0]]) + [3.0, -5.0, 0.5]
    fin = np.array([[1.0, 0, 0], [0.0, 1.0, 0], [1.0, 1.0, 0], [1.0, 2.0, 0], [1.75, 0.25, 0.0], [2.0, 1.0, 0.0]]) + [3.0, -5.0, 0.5]
    major = [_cloud(rng, 30), maj, _cloud(rng, 30)]
    fine = [_cloud(rng, 50), fin, _cloud(rng, 50)]
    ground = [_ground(rng, 100), _ground(rng, 100), EMPTY]
    return FinishCase("ties", fine, major, [np.arange(len(m), dtype=np.int32) * 7 for m in major], ground,
                      tie_chunks=(1,), rejects=("tie_larger",), claims=dict(tied=5))


_BUILDERS = {"tiles": tiles_case}
_BUILDERS.update({f"mixed_k_nb{nb}": functools.partial(mixed_k_case, nb) for nb in MIXED_NB + (100,)})
_BUILDERS.update({"many_chunks_grown": many_chunks_grown_case, "chunk_limit": chunk_limit_case,
                  "key_bits_plus0": functools.partial(key_bits_case, 0), "key_bits_plus1": functools.partial(key_bits_case, 1)})
_BUILDERS.update({f"ring_stop_k{k}": functools.partial(ring_stop_case, k) for k in pc.RING_KS})
_BUILDERS.update({f"ring_stop_k{k}_grown": functools.partial(ring_stop_case, k, GROWN_CHUNKS) for k in pc.RING_KS})
_BUILDERS.update({"degenerate": degenerate_case, "f4_lap": f4_lap_case, "strict_z": strict_z_case, "ties": ties_case})
CASE_NAMES = tuple(_BUILDERS)


def case(name):
    c = _BUILDERS[name]()
    assert c.name == name, (c.name, name)
    return c


def all_cases():
    return [case(name) for name in CASE_NAMES]


# ---- refusals
NONFINITE = (("nan", np.nan), ("pinf", np.inf), ("ninf", -np.inf))


def refusal_cases():
    """(name, fine, major, labels, ground, cloud, chunk): calls `ai_chunk_finish` must refuse with "the <cloud> coordinates of
    chunk <chunk> are not finite" and every output untouched."""
    rng = np.random.default_rng(6101)
    sizes_f, sizes_m, sizes_g = (40, 0, 300, 4100, 77), (9, 0, 12, 50, 257), (100, 257, 0, 4100, 513)
    fine = [_cloud(rng, n) for n in sizes_f]
    major = [_cloud(rng, n) for n in sizes_m]
    ground = [_ground(rng, n, side=4.0) for n in sizes_g]
    labels = _labels(rng, major)
    out = []

    def with_value(parts, c, row, axis, v):
        parts = list(parts)
        parts[c] = parts[c].copy()
        parts[c][row, axis] = v
        return parts
    for j, (tag, v) in enumerate(NONFINITE):
        a = j % 3
        out.append((f"{tag}_last_row_of_last_chunk_ground", fine, major, labels, with_value(ground, 4, sizes_g[4] - 1, a, v), "ground", 4))
        out.append((f"{tag}_last_row_of_last_chunk_fine", with_value(fine, 4, sizes_f[4] - 1, a, v), major, labels, ground, "fine", 4))
        out.append((f"{tag}_row_2049_ground", fine, major, labels, with_value(ground, 3, BB * BLOCK + 1, a, v), "ground", 3))
        out.append((f"{tag}_row_4097_fine", with_value(fine, 3, 2 * BB * BLOCK + 1, a, v), major, labels, ground, "fine", 3))
        out.append((f"{tag}_middle_chunk_major", fine, with_value(major, 2, 7, a, v), labels, ground, "major", 2))
    for e, tag in ((K["EXTENT_LIMIT"], "1e15"), (4.0 * K["EXTENT_LIMIT"], "4e15")):      # all coordinates are >= 0: from 0.0 to e exactly
        wide = with_value(with_value(ground, 3, 4098, 1, 0.0), 3, 4099, 1, e)
        out.append((f"extent_{tag}_ground", fine, major, labels, wide, "ground", 3))
        widem = with_value(with_value(major, 2, 10, 0, 0.0), 2, 11, 0, e)
        out.append((f"extent_{tag}_major", fine, widem, labels, ground, "major", 2))
    return out
