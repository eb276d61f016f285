"""Fixtures, host models and exact references for the label bookkeeping (``autoinst_amd/csrc/ai_labels.hip``) and the shared
exclusive scan under it (``autoinst_amd/csrc/ai_scan.hip``).

Pure NumPy / SciPy, no GPU and no library: tests/test_label_cases.py proves on the CPU that every fixture sits on the kernel
limit its name claims and that every `check_*` helper rejects a list of deliberately wrong answers; tests/test_gpu_labels.py
feeds the device's answers to the same helpers.  Everything here is integers or exact bit patterns, so every check is an
equality.  Inputs are finite: NaN and +-inf are out of scope.

The limits are READ from the sources (`constants`), and the fixtures are derived from them: a changed constant moves the
fixtures with it, and the regime claims are then re-proven by the CPU test.

* ``scan_*``: `ai_exclusive_scan_i32` seen through `ai_label_pairs`, whose head flags can be set freely after position 0
  (`pairs_from_heads`).  Lengths on both sides of one tile, of the direct path (`SCAN_MAX_DIRECT_TILES` tiles) and one with
  five second-level tiles; `scan_model` restates the two- and three-level plan, `tmp` carving included.
* ``pairs_*``: label extremes, the first-call capacity of `labels_api.label_pairs`, the `cap` rules of the C entry point.
* ``merge_tile_* / merge_face_* / merge_scalar_*``: `ai_merge_associate` on the box tiles of `km_inside`, the inclusive faces
  of cube and boxes, and the scalar bit patterns and run walk of `km_common`.
* ``unique_*``: `ai_unique_points`.  ``voxel_scan``: one `ai_voxel_down_sample` above the direct path.
* ``merge_iou_*``: the host rule ``iou > 0.01`` and the association, end to end against `oracle.merge_ref`.

`ai_statistical_inliers` also scans at map size, but its oracle is a kd-tree query of 8.4 M points; its scan input is a 0/1
flag array of the very form the ``scan_*`` fixtures cover, so it is left out at that size.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np
import scipy.sparse as sp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_CSRC = os.path.join(ROOT, "autoinst_amd", "csrc")

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


# ------------------------------------------------------------------------------------------------- constants from the sources
def _read(*parts):
    with open(os.path.join(*parts)) as f:
        return f.read()


def _define(text, name):
    m = re.search(r"^\s*#define\s+" + name + r"\s+\(?(\d+)\)?\s*(?://.*)?$", text, re.M)
    if not m:
        raise RuntimeError(f"#define {name} <integer> not found")
    return int(m.group(1))


def constants():
    """The kernels' limits, parsed out of the ``.hip`` / ``.h`` / ``.py`` sources."""
    scan, labels = _read(_CSRC, "ai_scan.hip"), _read(_CSRC, "ai_labels.hip")
    common, api = _read(_CSRC, "ai_common.h"), _read(ROOT, "autoinst_amd", "labels_api.py")
    if not re.search(r"#define\s+SCAN_TILE\s+\(AI_BLOCK\s*\*\s*SCAN_ITEMS\)", scan):
        raise RuntimeError("SCAN_TILE is no longer AI_BLOCK * SCAN_ITEMS")
    cap = re.search(r"^\s*cap\s*=\s*1\s*<<\s*(\d+)\s*$", api, re.M)
    if not cap:
        raise RuntimeError("the first-call capacity `cap = 1 << k` of labels_api.label_pairs was not found")
    c = dict(AI_BLOCK=_define(common, "AI_BLOCK"), SCAN_ITEMS=_define(scan, "SCAN_ITEMS"),
             SCAN_MAX_DIRECT_TILES=_define(scan, "SCAN_MAX_DIRECT_TILES"), KM_BOX_TILE=_define(labels, "KM_BOX_TILE"),
             KM_MAX_SCALARS=_define(labels, "KM_MAX_SCALARS"), FIRST_CAP=1 << int(cap.group(1)))
    c["SCAN_TILE"] = c["AI_BLOCK"] * c["SCAN_ITEMS"]
    c["SCAN_DIRECT"] = c["SCAN_TILE"] * c["SCAN_MAX_DIRECT_TILES"]
    return c


K = constants()
T = K["SCAN_TILE"]                # elements per tile (2048)
D = K["SCAN_DIRECT"]              # the longest input of the direct path (8 388 608)
BLOCK = K["AI_BLOCK"]
BOX_TILE = K["KM_BOX_TILE"]
FIRST_CAP = K["FIRST_CAP"]
SCAN_BIG = 20_000_000             # about 9766 first-level and 5 second-level tiles


# ------------------------------------------------------------------------------------------------- comparing
def first_difference(got, exp):
    """None when equal, else a sentence naming the first differing index.  Floats are compared by their bits."""
    got, exp = np.asarray(got), np.asarray(exp)
    if got.shape != exp.shape:
        return f"shape {got.shape} instead of {exp.shape}"
    if exp.dtype.kind == "f":
        g, e = np.ascontiguousarray(got, np.float64).view(np.int64), np.ascontiguousarray(exp, np.float64).view(np.int64)
    else:
        g, e = got.astype(np.int64), exp.astype(np.int64)
    bad = np.flatnonzero((g != e).reshape(-1))
    if bad.size == 0:
        return None
    i = np.unravel_index(int(bad[0]), exp.shape)
    i = i[0] if len(i) == 1 else i
    return f"{bad.size} of {exp.size} differ, first at {i}: {got[i]!r} instead of {exp[i]!r}"


def _check(what, got, exp):
    d = first_difference(got, exp)
    assert d is None, f"{what}: {d}"


def check_label_pairs(name, got, exp):
    for what, g, e in zip(("pair_a", "pair_b", "count"), got, exp):
        _check(f"{name} {what}", g, e)


def check_merge(name, got, exp):
    for key in ("n_points1", "n_scalars1", "n_scalars2", "inter", "common"):
        _check(f"{name} {key}", got[key], exp[key])


def check_unique(name, got, exp):
    got = np.asarray(got)
    assert got.size == 0 or np.all(np.diff(got.astype(np.int64)) > 0), f"{name}: kept indices are not strictly ascending"
    _check(f"{name} keep_index", got, exp)


def check_points(name, got, exp):
    _check(f"{name} points", got, exp)


# ------------------------------------------------------------------------------------------------- label pairs: references
_BIAS = np.int64(2 ** 31)


def pack_pairs(a, b):
    """One uint64 per row whose unsigned order is the signed order of (a, b)."""
    a, b = np.asarray(a).astype(np.int64), np.asarray(b).astype(np.int64)
    return ((a + _BIAS).astype(np.uint64) << np.uint64(32)) | (b + _BIAS).astype(np.uint64)


def unpack_pairs(key):
    a = (key >> np.uint64(32)).astype(np.int64) - _BIAS
    b = (key & np.uint64(0xFFFFFFFF)).astype(np.int64) - _BIAS
    return a.astype(np.int32), b.astype(np.int32)


def ref_label_pairs(a, b):
    """Distinct (a[i], b[i]) in ascending signed order with their counts: ``np.unique`` of one packed key."""
    if np.asarray(a).size == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64)
    u, c = np.unique(pack_pairs(a, b), return_counts=True)
    pa, pb = unpack_pairs(u)
    return pa, pb, c.astype(np.int64)


# ------------------------------------------------------------------------------------------------- the scan, as the source plans it
def scan_tiles(n):
    return (n + T - 1) // T


def scan_levels(n):
    """Tile counts per level, e.g. [9766, 5] for 20 M: the direct path ends the list."""
    out, m = [], n
    while True:
        m = scan_tiles(max(m, 1))
        out.append(m)
        if m <= K["SCAN_MAX_DIRECT_TILES"]:
            return out


def scan_regime(n):
    nt = scan_tiles(n)
    return "single_tile" if nt == 1 else "direct" if nt <= K["SCAN_MAX_DIRECT_TILES"] else "recursive"


def scan_tmp_elems(n):
    """`ai_scan_tmp_elems`."""
    tot, m = 0, n
    while True:
        m = scan_tiles(max(m, 1))
        tot += m + 1
        if m <= 1:
            return tot + 8


SCAN_MUTANTS = ("drop_upper_offsets", "drop_second_level_offsets", "total_one_tile_early")


def _scan_level(inp, out, n, tmp, off, mutant, level):
    nt = scan_tiles(n)
    assert off + nt + 1 <= tmp.shape[0], "the level's sums leave ai_scan_tmp_elems"
    sums = tmp[off:off + nt + 1]
    pad = np.zeros(nt * T, np.int64)                                   # k_scan_tiles (in and out may be one array)
    pad[:n] = inp[:n]
    inc = np.cumsum(pad.reshape(nt, T), axis=1)
    sums[:nt] = inc[:, -1]
    out[:n] = (inc - pad.reshape(nt, T)).reshape(-1)[:n]
    if nt <= K["SCAN_MAX_DIRECT_TILES"]:                               # k_scan_add_direct
        offs = np.cumsum(sums[:nt]) - sums[:nt]
        if not (mutant == "drop_second_level_offsets" and level > 0):
            out[:n] += np.repeat(offs, T)[:n]
        out[n] = offs[-1] + sums[nt - 1]
        return
    _scan_level(sums, sums, nt, tmp, off + nt + 1, mutant, level + 1)   # in place, the next sums behind this level's nt + 1
    if mutant != "drop_upper_offsets":                                 # k_scan_add
        out[:n] += np.repeat(sums[:nt], T)[:n]
    out[n] = sums[nt - 1] if mutant == "total_one_tile_early" else sums[nt]


def scan_model(x, mutant=None):
    """`ai_exclusive_scan_i32` restated level by level: n + 1 values, the last the grand total.  ``mutant`` breaks it on
    purpose (test_label_cases.py shows that the fixtures notice)."""
    x = np.asarray(x)
    n = x.shape[0]
    out = np.zeros(n + 1, np.int64)
    if n > 0:
        _scan_level(x, out, n, np.full(scan_tmp_elems(n), -(2 ** 40), np.int64), 0, mutant, 0)
    return out


PAIR_MUTANTS = ("last_run_not_closed_with_n", "unsigned_order")


def model_label_pairs(a, b, cap=None, mutant=None):
    """`ai_label_pairs` by the device's plan: biased keys, sort, head flags, `scan_model`, one emit per head, counts from
    the run starts.  Returns (pair_a, pair_b, count, n_pairs) with min(n_pairs, cap) rows."""
    a, b = np.asarray(a, np.int32), np.asarray(b, np.int32)
    n = a.shape[0]
    if n == 0:
        return np.zeros(0, np.int32), np.zeros(0, np.int32), np.zeros(0, np.int64), 0
    if mutant == "unsigned_order":
        key = (a.view(np.uint32).astype(np.uint64) << np.uint64(32)) | b.view(np.uint32).astype(np.uint64)
    else:
        key = pack_pairs(a, b)
    sk = np.sort(key)
    head = np.ones(n, np.int64)
    head[1:] = sk[1:] != sk[:-1]
    pos = scan_model(head, mutant if mutant in SCAN_MUTANTS else None)
    total = max(int(pos[n]), 0)
    m = total if cap is None else min(total, cap)
    okey, start = np.zeros(total, np.uint64), np.zeros(total, np.int64)
    i = np.flatnonzero(pos[1:] != pos[:-1])
    r = pos[i]
    ok = (r >= 0) & (r < total)                                        # a wrong scan would write outside: the model drops it
    okey[r[ok]], start[r[ok]] = sk[i[ok]], i[ok]
    hs = np.zeros(m + 1, np.int64)
    ncopy = min(m + 1, total)
    hs[:ncopy] = start[:ncopy]
    if ncopy == m and m > 0:
        hs[m] = hs[m - 1] if mutant == "last_run_not_closed_with_n" else n
    if mutant == "unsigned_order":
        pa = (okey >> np.uint64(32)).astype(np.uint32).view(np.int32)
        pb = (okey & np.uint64(0xFFFFFFFF)).astype(np.uint32).view(np.int32)
    else:
        pa, pb = unpack_pairs(okey)
    return pa[:m], pb[:m], np.diff(hs), total


# ------------------------------------------------------------------------------------------------- scan_* fixtures
SCAN_PATTERNS = ("all_heads", "single_run", "tile_start", "tile_end", "last_only", "bernoulli_half", "bernoulli_1e-4")
SCAN_BIG_PATTERNS = ("all_heads", "single_run", "tile_start", "bernoulli_half")
SCAN_SMALL_LENGTHS = (1, 2, BLOCK - 1, BLOCK, BLOCK + 1, T - 1, T, T + 1, 2 * T, 2 * T + 1)
SCAN_BIG_LENGTHS = (D - 1, D, D + 1, D + T + 5, SCAN_BIG)
SCAN_SHUFFLED = ("bernoulli_half",)          # big lengths: the rows of these patterns are shuffled, so the sort is real


def scan_heads(n, pattern, seed=0):
    """Head flags of the SORTED rows; position 0 is a head by definition."""
    h = np.zeros(n, np.int8)
    rng = np.random.default_rng([seed, n])
    if pattern == "all_heads":
        h[:] = 1
    elif pattern == "tile_start":
        h[::T] = 1
    elif pattern == "tile_end":
        h[T - 1::T] = 1
    elif pattern == "last_only":
        h[n - 1] = 1
    elif pattern == "bernoulli_half":
        h[:] = rng.random(n) < 0.5
    elif pattern == "bernoulli_1e-4":
        h[:] = rng.random(n) < 1e-4
    elif pattern != "single_run":
        raise KeyError(pattern)
    h[0] = 1
    return h


def pairs_from_heads(heads, shuffle_seed=None):
    """Label columns whose sorted pair keys have exactly these head flags: run r is the pair ((r >> 10) - 4096,
    (r & 1023) - 512), both columns crossing zero."""
    run = np.cumsum(heads, dtype=np.int64) - 1
    a = ((run >> 10) - 4096).astype(np.int32)
    b = ((run & 1023) - 512).astype(np.int32)
    if shuffle_seed is not None:
        p = np.random.default_rng(shuffle_seed).permutation(a.shape[0])
        a, b = a[p], b[p]
    return a, b


@dataclass
class PairCase:
    name: str
    a: np.ndarray
    b: np.ndarray
    heads: np.ndarray | None = None
    claims: dict = field(default_factory=dict)


def scan_names(big):
    if big:
        return [f"scan_{n}_{p}" for n in SCAN_BIG_LENGTHS for p in SCAN_BIG_PATTERNS]
    return [f"scan_{n}_{p}" for n in SCAN_SMALL_LENGTHS for p in SCAN_PATTERNS]


def scan_case(name):
    _, n, pattern = name.split("_", 2)
    n = int(n)
    h = scan_heads(n, pattern)
    big = n > 2 * T + 1
    shuffled = (big and pattern in SCAN_SHUFFLED) or (not big and n % 2 == 1)
    a, b = pairs_from_heads(h, shuffle_seed=n if shuffled else None)
    return PairCase(name, a, b, h, dict(n=n, tiles=scan_levels(n), regime=scan_regime(n), shuffled=shuffled))


# ------------------------------------------------------------------------------------------------- pairs_* fixtures
def _distinct_pairs(k, extra, seed):
    i = np.arange(k, dtype=np.int64)
    rng = np.random.default_rng(seed)
    i = np.concatenate([i, rng.integers(0, k, extra)])
    rng.shuffle(i)
    return ((i >> 8) - 100).astype(np.int32), ((i & 255) - 128).astype(np.int32)


def pair_cases():
    out = []
    rng = np.random.default_rng(41)
    ext = np.array([I32_MIN, -1, 0, 1, I32_MAX], np.int64)
    grid = np.stack(np.meshgrid(ext, ext, indexing="ij"), -1).reshape(-1, 2)
    rows = np.concatenate([grid, grid[rng.integers(0, 25, 5000)]])
    rng.shuffle(rows)
    out.append(PairCase("pairs_extremes", rows[:, 0].astype(np.int32), rows[:, 1].astype(np.int32), claims=dict(distinct=25)))
    for k in (FIRST_CAP - 1, FIRST_CAP, FIRST_CAP + 1):
        a, b = _distinct_pairs(k, 1000, k)
        out.append(PairCase(f"pairs_distinct_{k}", a, b, claims=dict(distinct=k)))
    out.append(PairCase("pairs_empty", np.zeros(0, np.int32), np.zeros(0, np.int32), claims=dict(distinct=0)))
    return out


def pair_case(name):
    return next(c for c in pair_cases() if c.name == name)


# ------------------------------------------------------------------------------------------------- merge: references
def _cube(center, side):
    """The same double expression as the entry point: half = side / 2, lo = center - half, hi = center + half."""
    c = np.asarray(center, np.float64)
    half = np.float64(side) / np.float64(2.0)
    return c - half, c + half


def ref_merge_associate_loop(map_xyz, map_inst, chunk_xyz, chunk_inst, center, side, n1, n2):
    """One iteration's counts, instance by instance, from the definitions: inclusive crop, ``np.unique`` of the flattened
    coordinates, min / max box, inclusive compare (the loop of test_labels.test_merge_counts_equal_brute_force)."""
    mp, cp = np.asarray(map_xyz, np.float64).reshape(-1, 3), np.asarray(chunk_xyz, np.float64).reshape(-1, 3)
    mi, ci = np.asarray(map_inst), np.asarray(chunk_inst)
    lo, hi = _cube(center, side)
    crop = np.all(mp >= lo, 1) & np.all(mp <= hi, 1)
    r = dict(inter=np.zeros((n1, n2), np.int32), common=np.zeros((n1, n2), np.int32), n_scalars1=np.zeros(n1, np.int32),
             n_scalars2=np.zeros(n2, np.int32), n_points1=np.zeros(n1, np.int32))
    p2s = {id2: cp[ci == id2] for id2 in range(1, n2)}
    for id2, p2 in p2s.items():
        r["n_scalars2"][id2] = np.unique(p2).shape[0]
    for id1 in range(1, n1):
        p1 = mp[crop & (mi == id1)]
        r["n_points1"][id1] = p1.shape[0]
        r["n_scalars1"][id1] = np.unique(p1).shape[0]
        for id2, p2 in p2s.items():
            if p1.shape[0]:
                r["inter"][id1, id2] = int((np.all(p2 >= p1.min(0), 1) & np.all(p2 <= p1.max(0), 1)).sum())
            union = np.unique(np.concatenate((p1, p2))).shape[0]
            r["common"][id1, id2] = r["n_scalars1"][id1] + r["n_scalars2"][id2] - union
    return r


MERGE_MUTANTS = ("cube_face_exclusive", "box_face_exclusive", "box_tiles_from_id0", "signed_zero_two_scalars",
                 "common_per_occurrence")


def _scalar_entries(p, ids, fold):
    vals = p.reshape(-1)
    bits = np.ascontiguousarray(vals + 0.0 if fold else vals).view(np.int64)        # + 0.0 turns -0.0 into +0.0
    return np.repeat(ids.astype(np.int64), 3), bits


def _distinct_entries(ids, bits):
    o = np.lexsort((bits, ids))
    ids, bits = ids[o], bits[o]
    keep = np.ones(ids.shape[0], bool)
    keep[1:] = (ids[1:] != ids[:-1]) | (bits[1:] != bits[:-1])
    return ids[keep], bits[keep]


def ref_merge_associate(map_xyz, map_inst, chunk_xyz, chunk_inst, center, side, n1, n2, mutant=None):
    """The vectorised form of `ref_merge_associate_loop` (proven equal on every small fixture).  Sets of scalars become
    0/1 rows of an (instance x distinct value) matrix, so ``common`` = |S1 & S2| is one sparse product.  ``mutant``
    breaks one rule on purpose."""
    mp, cp = np.asarray(map_xyz, np.float64).reshape(-1, 3), np.asarray(chunk_xyz, np.float64).reshape(-1, 3)
    mi, ci = np.asarray(map_inst).astype(np.int64), np.asarray(chunk_inst).astype(np.int64)
    lo, hi = _cube(center, side)
    if mutant == "cube_face_exclusive":
        crop = np.all(mp > lo, 1) & np.all(mp < hi, 1)
    else:
        crop = np.all(mp >= lo, 1) & np.all(mp <= hi, 1)
    v1, v2 = crop & (mi > 0) & (mi < n1), (ci > 0) & (ci < n2)
    p1, i1, p2, i2 = mp[v1], mi[v1], cp[v2], ci[v2]
    fold = mutant != "signed_zero_two_scalars"
    e1, e2 = _scalar_entries(p1, i1, fold), _scalar_entries(p2, i2, fold)
    d1, d2 = _distinct_entries(*e1), _distinct_entries(*e2)
    r = dict(n_points1=np.bincount(i1, minlength=n1).astype(np.int32), n_scalars1=np.bincount(d1[0], minlength=n1).astype(np.int32),
             n_scalars2=np.bincount(d2[0], minlength=n2).astype(np.int32))
    if mutant == "common_per_occurrence":
        d1, d2 = e1, e2
    vals = np.unique(np.concatenate([d1[1], d2[1]]))
    if vals.size:
        m1 = sp.coo_matrix((np.ones(d1[0].size, np.int64), (d1[0], np.searchsorted(vals, d1[1]))), shape=(n1, vals.size)).tocsr()
        m2 = sp.coo_matrix((np.ones(d2[0].size, np.int64), (d2[0], np.searchsorted(vals, d2[1]))), shape=(n2, vals.size)).tocsr()
        r["common"] = np.asarray((m1 @ m2.T).todense()).astype(np.int32)
    else:
        r["common"] = np.zeros((n1, n2), np.int32)
    bmin, bmax = np.full((n1, 3), np.inf), np.full((n1, 3), -np.inf)
    np.minimum.at(bmin, i1, p1)
    np.maximum.at(bmax, i1, p1)
    inter = np.zeros((n1, n2), np.int32)
    for id1 in np.flatnonzero(r["n_points1"]):
        if mutant == "box_face_exclusive":
            inside = np.all(p2 > bmin[id1], 1) & np.all(p2 < bmax[id1], 1)
        else:
            inside = np.all(p2 >= bmin[id1], 1) & np.all(p2 <= bmax[id1], 1)
        inter[id1] = np.bincount(i2[inside], minlength=n2)
    if mutant == "box_tiles_from_id0":          # boxes walked from id 0 while the rows are still numbered from 1
        inter = np.concatenate([np.zeros((1, n2), np.int32), inter[:-1]])
    r["inter"] = inter
    return r


# ------------------------------------------------------------------------------------------------- merge_* fixtures
@dataclass
class MergeCase:
    name: str
    map_xyz: np.ndarray
    map_inst: np.ndarray
    chunk_xyz: np.ndarray
    chunk_inst: np.ndarray
    center: np.ndarray
    n1: int
    n2: int
    side: float = 40.0
    claims: dict = field(default_factory=dict)

    def args(self):
        return (self.map_xyz, self.map_inst, self.chunk_xyz, self.chunk_inst, self.center, self.side, self.n1, self.n2)


def _mc(name, mp, mi, cp, ci, center, n1, n2, **claims):
    return MergeCase(name, np.ascontiguousarray(mp, np.float64).reshape(-1, 3), np.asarray(mi, np.int32),
                     np.ascontiguousarray(cp, np.float64).reshape(-1, 3), np.asarray(ci, np.int32), np.asarray(center, np.float64),
                     int(n1), int(n2), claims=claims)


def box_tiles(n1):
    """Tiles `km_inside` walks: ids 1 .. n1 - 1 in tiles of KM_BOX_TILE."""
    return (max(n1 - 1, 0) + BOX_TILE - 1) // BOX_TILE


MERGE_TILE_N1 = (2, BOX_TILE, BOX_TILE + 1, BOX_TILE + 2, 2 * BOX_TILE, 2 * BOX_TILE + 1, 2 * BOX_TILE + 88)
MERGE_TILE_N2 = (2, 40)


def merge_tile_case(n1, n2):
    """Map instance id sits in its own lattice cell with the box [corner, corner + 1]; 1 + id % 3 chunk points of instance
    1 + id % (n2 - 1) lie in it, faces included.  Every 7th id lies wholly outside the crop cube.  Ids <= 0 and ids
    == n_inst (and beyond) on both sides sit inside live boxes and count for nothing."""
    rng = np.random.default_rng([n1, n2])
    mp, mi, cp, ci = [], [], [], []
    expect = np.zeros((n1, n2), np.int32)
    npts = np.zeros(n1, np.int32)
    for id1 in range(1, n1):
        k = id1 - 1
        corner = np.array([-14.0 + 3 * (k % 10), -14.0 + 3 * ((k // 10) % 10), -8.0 + 3 * (k // 100)])
        outside = id1 % 7 == 3
        pts = np.concatenate([[np.zeros(3), np.ones(3)], rng.integers(0, 9, (2, 3)) / 8.0]) + corner
        mp.append(pts + (np.array([100.0, 0, 0]) if outside else 0.0))
        mi += [id1] * 4
        kk, id2 = 1 + id1 % 3, 1 + id1 % (n2 - 1)
        inside = corner + rng.integers(0, 9, (kk, 3)) / 8.0
        inside[0, id1 % 3] = corner[id1 % 3] + id1 % 2                                        # one of them on a face for certain
        cp.append(inside)
        ci += [id2] * kk
        if not outside:
            expect[id1, id2], npts[id1] = kk, 4
        mp.append(corner + np.array([[0.5, 0.5, 0.5], [1.5, 0.5, 0.5], [-0.5, 0.5, 0.5], [0.5, 1.5, 0.5]]))   # would widen the box
        mi += [0, -1 - id1, n1, n1 + 1 + (id1 % 2)]
        cp.append(corner + np.array([[0.5, 0.5, 0.5]] * 4))
        ci += [0, -id1, n2, n2 + 1 + (id1 % 3)]
    mp, cp = np.concatenate(mp), np.concatenate(cp)
    if cp.shape[0] % BLOCK == 0:
        cp, ci = np.concatenate([cp, [[0.25, 0.25, 0.25]]]), ci + [0]
    return _mc(f"merge_tile_{n1}_{n2}", mp, mi, cp, ci, [0.0, 0.0, 0.0], n1, n2, box_tiles=box_tiles(n1), inter=expect, n_points1=npts)


CENTER_EXACT = (1.5, -2.25, 0.5)            # center +- 20 is exact
CENTER_ROUNDS = (0.1, 1.0 / 3.0, 0.007)     # center +- 20 rounds on every axis


def merge_face_cube_case(tag, center):
    """Per cube face three map instances of one point each: on the face, one ulp outside it, one ulp inside it."""
    c = np.asarray(center, np.float64)
    lo, hi = _cube(c, 40.0)
    mp, kept = [], []
    for a in range(3):
        for face, away in ((lo[a], -np.inf), (hi[a], np.inf)):
            for v, k in ((face, 1), (np.nextafter(face, away), 0), (np.nextafter(face, -away), 1)):
                p = c.copy()
                p[a] = v
                mp.append(p)
                kept.append(k)
    n1 = len(mp) + 1
    cp = np.array([c, c + 0.5])
    return _mc(f"merge_face_cube_{tag}", mp, np.arange(1, n1), cp, [1, 1], c, n1, 2,
               n_points1=np.array([0] + kept, np.int32), on_face=6, ulp_outside=6, ulp_inside=6)


def merge_face_box_case():
    """One map instance with the box [bl, bh]; per box face three chunk instances of one point each: on, outside, inside."""
    bl, bh = np.array([-1.25, 0.1, 1.0 / 3.0]), np.array([0.7, 2.2, 1.1])
    mid = (bl + bh) / 2
    cp, inside = [], []
    for a in range(3):
        for face, away in ((bl[a], -np.inf), (bh[a], np.inf)):
            for v, k in ((face, 1), (np.nextafter(face, away), 0), (np.nextafter(face, -away), 1)):
                p = mid.copy()
                p[a] = v
                cp.append(p)
                inside.append(k)
    n2 = len(cp) + 1
    expect = np.zeros((2, n2), np.int32)
    expect[1, 1:] = inside
    return _mc("merge_face_box", [bl, bh, mid], [1, 1, 1], cp, np.arange(1, n2), [0.0, 1.0, 0.5], 2, n2, inter=expect,
               on_face=6, ulp_outside=6, ulp_inside=6)


DEN = 5e-324                                   # the smallest denormal
DEN_MAX = float(np.nextafter(np.finfo(np.float64).tiny, 0.0))


def merge_scalar_cases():
    up, dn = float(np.nextafter(1.0, 2.0)), float(np.nextafter(1.0, 0.0))
    tiny = float(np.finfo(np.float64).tiny)
    out = [
        _mc("merge_scalar_signed_zero", [[0.0, 1, 2], [-0.0, 3, 4]], [1, 1], [[-0.0, 5, 6], [0.0, -0.0, 5]], [1, 1], [0, 0, 0], 2, 2,
            n_scalars1=[0, 5], n_scalars2=[0, 3], common=[[0, 0], [0, 1]]),
        _mc("merge_scalar_ulp", [[1.0, up, dn]], [1], [[1.0, up, 7.0]], [1], [0, 0, 0], 2, 2,
            n_scalars1=[0, 3], n_scalars2=[0, 3], common=[[0, 0], [0, 2]]),
        _mc("merge_scalar_denormal", [[DEN, -DEN, 0.0], [tiny, DEN_MAX, 1.0]], [1, 1], [[DEN, 0.0, -0.0], [-DEN, DEN_MAX, 2.0]], [1, 1],
            [0, 0, 0], 2, 2, n_scalars1=[0, 6], n_scalars2=[0, 5], common=[[0, 0], [0, 4]]),
        _mc("merge_scalar_negative", [[-1, -2, -3], [float(np.nextafter(-1.0, -2.0)), -2, 5]], [1, 1],
            [[-3, -1, float(np.nextafter(-2.0, -3.0))]], [1], [0, 0, 0], 2, 2,
            n_scalars1=[0, 5], n_scalars2=[0, 3], common=[[0, 0], [0, 2]]),
        _mc("merge_scalar_repeat", [[2.5, 2.5, 2.5], [2.5, 1, 1]], [1, 1], [[2.5, 2.5, 1.0], [1.0, 1.0, 2.5]], [1, 1], [0, 0, 0], 2, 2,
            n_scalars1=[0, 2], n_scalars2=[0, 2], common=[[0, 0], [0, 2]]),
    ]
    # z = 0.0 shared by 300 map and 40 chunk instances: one run of 340 entries for km_common to walk
    n1, n2 = 301, 41
    i1, i2 = np.arange(1, n1), np.arange(1, n2)
    mp = np.stack([-15.0 + i1 * 0.0625, 3.0 + i1 * 0.03125, np.zeros(n1 - 1)], 1)
    cp = np.stack([-15.5 - i2 * 0.0625, -3.0 - i2 * 0.03125, np.where(i2 % 2 == 0, -0.0, 0.0)], 1)
    out.append(_mc("merge_scalar_shared_z", np.concatenate([mp, mp + [0.0078125, 0.0078125, 0]]), np.concatenate([i1, i1]), cp, i2,
                   [0, 0, 0], n1, n2, run=n1 - 1 + n2 - 1, common_min=1))
    rng = np.random.default_rng(9)
    live = rng.integers(-40, 41, (300, 3)) / 4.0
    out.append(_mc("merge_scalar_empty_crop", live + [100.0, 0, 0], rng.integers(1, 4, 300), live, rng.integers(0, 4, 300), [0, 0, 0], 4, 4,
                   sel0=0))
    out.append(_mc("merge_scalar_all_street", live, np.zeros(300), live[::-1], np.zeros(300), [0, 0, 0], 3, 5, sel0=0, sel1=0))
    return out


def merge_scalar_cross_case():
    """3 * (selected map + selected chunk points) > D: the merge's own scan of (value, instance) heads takes the recursive
    path.  Coarse 0.25 m grid, so the distinct entries stay few."""
    rng = np.random.default_rng(2024)
    nm, nc = 1_500_000, 1_400_001
    mp = rng.integers(-72, 73, (nm, 3)) / 4.0
    cp = rng.integers(-72, 73, (nc, 3)) / 4.0
    mi = np.where(rng.random(nm) < 0.01, 0, rng.integers(1, 6, nm))
    ci = np.where(rng.random(nc) < 0.01, 0, rng.integers(1, 5, nc))
    mp[:50, 0] += 40.0                                                                  # a few outside the crop
    return _mc("merge_scalar_cross_direct", mp, mi, cp, ci, [0, 0, 0], 6, 5)


def selected_counts(c):
    lo, hi = _cube(c.center, c.side)
    crop = np.all(c.map_xyz >= lo, 1) & np.all(c.map_xyz <= hi, 1)
    return int((crop & (c.map_inst > 0) & (c.map_inst < c.n1)).sum()), int(((c.chunk_inst > 0) & (c.chunk_inst < c.n2)).sum())


def merge_small_cases():
    out = [merge_tile_case(n1, n2) for n1 in MERGE_TILE_N1 for n2 in MERGE_TILE_N2]
    out += [merge_face_cube_case("exact", CENTER_EXACT), merge_face_cube_case("rounds", CENTER_ROUNDS), merge_face_box_case()]
    return out + merge_scalar_cases()


# ------------------------------------------------------------------------------------------------- unique points
def ref_unique_points(xyz, keep_last=False):
    """Ascending indices of the first row of every distinct triple; -0.0 equals +0.0.  (``keep_last``: a mutant.)"""
    p = np.ascontiguousarray(xyz, np.float64).reshape(-1, 3)
    n = p.shape[0]
    if n == 0:
        return np.zeros(0, np.int32)
    bits = (p + 0.0).view(np.int64)                                   # finite values: equal bits <=> equal values
    o = np.lexsort((bits[:, 2], bits[:, 1], bits[:, 0]))             # stable: a run keeps its rows in index order
    s = bits[o]
    first = np.ones(n, bool)
    first[1:] = np.any(s[1:] != s[:-1], axis=1)
    pick = np.append(first[1:], True) if keep_last else first
    return np.sort(o[pick]).astype(np.int32)


def unique_cases():
    """name -> (n, 3) float64."""
    rng = np.random.default_rng(77)
    base = np.array([1.0, -2.0, 3.5])
    rows = [base]
    for a in range(3):
        for to in (np.inf, -np.inf):
            q = base.copy()
            q[a] = np.nextafter(q[a], to)
            rows += [q, q]
    ulp = np.array(rows + [base])
    zero = np.array([[0.0, 1, 1], [-0.0, 1, 1], [-0.0, -0.0, 2], [0.0, 0.0, 2], [1, -0.0, 0.0], [1, 0.0, -0.0], [-0.0, -0.0, -0.0],
                     [0.0, 0.0, 0.0], [0.0, -0.0, 0.0]])
    ends = rng.normal(0, 5, (5000, 3))
    ends[-1] = ends[0]
    tiny = float(np.finfo(np.float64).tiny)
    den = np.array([[DEN, -DEN, 0.0], [DEN, -DEN, -0.0], [-DEN, DEN, 0.0], [DEN_MAX, tiny, -1.0], [DEN_MAX, tiny, -1.0],
                    [tiny, DEN_MAX, -1.0], [-1.0, -2.0, -3.0], [-1.0, -2.0, float(np.nextafter(-3.0, -4.0))], [-1.0, -2.0, -3.0],
                    [2 * DEN, -DEN, 0.0]])
    out = {"unique_ulp_axis": ulp, "unique_signed_zero": zero, "unique_ends": ends, "unique_identical": np.tile([0.1, -0.2, 0.3], (3000, 1)),
           "unique_distinct": rng.permutation(2 * T + 1)[:, None] * np.array([0.5, -0.25, 0.125]), "unique_denormal_negative": den}
    for n in (1, T, T + 1):
        out[f"unique_len_{n}"] = unique_len_case(n)
    return out


UNIQUE_BIG_LENGTHS = (D, D + 1)


def unique_len_case(n):
    """Points on a 0.25 m grid of 400^3 cells: about one point in eight at D repeats an earlier one."""
    return np.random.default_rng([5, n]).integers(-200, 200, (n, 3)) / 4.0


# ------------------------------------------------------------------------------------------------- voxel_scan
VOXEL_SIZE = 0.35


def voxel_scan_points(n=D + 1, seed=3):
    """Jittered lattice with about two points per occupied voxel."""
    g = int(np.ceil((n / 2.0) ** (1.0 / 3.0)))
    rng = np.random.default_rng(seed)
    cell = rng.integers(0, g, (n, 3))
    return (cell + 0.5 + (rng.random((n, 3)) - 0.5) * 0.8) * VOXEL_SIZE


def ref_voxel_down_sample_packed(points, voxel_size):
    """`prep_ref.voxel_down_sample` with ``np.unique`` of one packed int64 key in place of ``np.unique(axis=0)`` (proven
    equal on a small cloud in test_label_cases.py): means by ``np.add.at``, i.e. summed in input order."""
    p = np.asarray(points, np.float64).reshape(-1, 3)
    vmin = p.min(axis=0) - voxel_size * 0.5
    vox = np.floor((p - vmin) / voxel_size).astype(np.int64)
    dims = vox.max(axis=0) + 1
    assert float(dims[0]) * float(dims[1]) * float(dims[2]) < 2.0 ** 62
    key = (vox[:, 0] * dims[1] + vox[:, 1]) * dims[2] + vox[:, 2]
    _, inv = np.unique(key, return_inverse=True)
    inv = inv.reshape(-1)
    m = int(inv.max()) + 1
    out = np.zeros((m, 3))
    np.add.at(out, inv, p)
    return out / np.bincount(inv, minlength=m).astype(np.float64)[:, None], inv


# ------------------------------------------------------------------------------------------------- merge_iou_* (host rule, end to end)
def _vals(k0, k):
    """k distinct values on a 1/16 grid from 0.25 + k0 / 16."""
    return 0.25 + 0.0625 * np.arange(k0, k0 + k)


def _street(seed, n=40):
    rng = np.random.default_rng(seed)
    return np.stack([rng.integers(0, 80, n) / 8.0, rng.integers(0, 80, n) / 8.0, np.full(n, -1.0)], 1)


def merge_iou_pair_chunks(union):
    """Map instance A: 20 points, 60 distinct scalars.  Chunk instance C: one point inside A's box and 12 outside it with 39
    scalars shared with nobody; ``union`` = 100 adds a point (w, w, w), one scalar more.  inter = 1 either way."""
    assert union in (99, 100)
    a = _vals(0, 60).reshape(20, 3)
    inside = _vals(30, 3)[None] + 0.03125
    outside = (6.0 + 0.0625 * np.arange(36)).reshape(12, 3) + 0.015625
    c = np.concatenate([inside, outside] + ([[[9.5078125] * 3]] if union == 100 else []))
    s0, s1 = _street(1), _street(2)
    s1[:10] = s0[:10]                                                   # coincident street points: removed as duplicates
    ca, cc = np.array([0.2, 0.3, 0.4]), np.array([0.7, 0.1, 0.6])
    chunk0 = (np.concatenate([a, s0]), np.concatenate([np.tile(ca, (20, 1)), np.zeros((40, 3))]))
    chunk1 = (np.concatenate([c, s1]), np.concatenate([np.tile(cc, (c.shape[0], 1)), np.zeros((40, 3))]))
    return [chunk0, chunk1], dict(color_a=ca, color_c=cc, n_c=c.shape[0], union=union, inter=1)


def merge_iou_tie_chunks():
    """Map instances A and B with the same IoU against chunk instance C.  B's points come first in the arrays, A's colour
    comes first in colour order: A wins."""
    a, b = _vals(0, 15).reshape(5, 3), _vals(100, 15).reshape(5, 3)
    c = np.array([_vals(6, 3) + 0.03125, _vals(106, 3) + 0.03125])
    ca, cb, cc = np.array([0.1, 0.9, 0.9]), np.array([0.8, 0.1, 0.1]), np.array([0.5, 0.5, 0.5])
    chunk0 = (np.concatenate([b, a, _street(3)]), np.concatenate([np.tile(cb, (5, 1)), np.tile(ca, (5, 1)), np.zeros((40, 3))]))
    chunk1 = (np.concatenate([c, _street(4)]), np.concatenate([np.tile(cc, (2, 1)), np.zeros((40, 3))]))
    return [chunk0, chunk1], dict(color_a=ca, color_b=cb, color_c=cc)


def merge_iou_many_chunks():
    """Three chunks over one lattice of 331 clusters (0 .. 149, 100 .. 279, 200 .. 330), every chunk with colours of its
    own: after two chunks the merged cloud has more than KM_BOX_TILE instances, so the third walks two box tiles."""
    rng = np.random.default_rng(12)
    k = np.arange(331)
    centres = np.stack([-12.25 + 3.5 * (k % 8), -12.25 + 3.5 * ((k // 8) % 8), -7.0 + 2.5 * (k // 64)], 1)
    pts = centres[:, None, :] + rng.integers(-4, 5, (331, 6, 3)) / 8.0
    chunks = []
    for ci, (lo, hi) in enumerate(((0, 150), (100, 280), (200, 331))):
        pal = np.round(np.random.default_rng(500 + ci).random((hi - lo, 3)), 4) * 0.9 + 0.05
        P = np.concatenate([pts[lo:hi].reshape(-1, 3), _street(20 + ci)])
        C = np.concatenate([np.repeat(pal, 6, axis=0), np.zeros((40, 3))])
        chunks.append((P, C))
    return chunks, dict(clusters=331)


def merge_iou_cases():
    return {"merge_iou_exactly_0.01": merge_iou_pair_chunks(100), "merge_iou_above_0.01": merge_iou_pair_chunks(99),
            "merge_iou_tie": merge_iou_tie_chunks(), "merge_iou_many_instances": merge_iou_many_chunks()}


def random_small_maps(seed=77, count=12):
    """The maps of test_labels.test_merge_equals_oracle_on_random_small_maps (same recipe, a CPU-sized number of them)."""
    rng = np.random.default_rng(seed)
    out = []
    for case in range(count):
        base = np.round(rng.normal(0, 6, (int(rng.integers(30, 400)), 3)) * 4) / 4
        base[rng.random(base.shape) < 0.02] *= -0.0
        chunks = []
        for c in range(int(rng.integers(2, 4))):
            sel = rng.random(base.shape[0]) < 0.7
            pts = base[sel] + (0.0 if rng.random() < 0.6 else np.round(rng.normal(0, 0.5, 3) * 4) / 4)
            k = int(rng.integers(1, 6))
            pal = np.concatenate([np.zeros((1, 3)), np.round(np.random.default_rng(1000 * case + c).random((k, 3)), 3) * 0.9 + 0.05])
            chunks.append((pts, pal[rng.integers(0, k + 1, pts.shape[0])]))
        out.append(chunks)
    return out
