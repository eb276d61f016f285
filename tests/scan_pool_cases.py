"""Fixtures and a host model for `ai_scan_pool` (``autoinst_amd/csrc/ai_scanpool.hip``) at the kernel limits
that tests/scan_pool_ref.py's hand-made cases leave open: the LDS tiles of the chunk table, the feature widths of the two
`ks_pool` instances, the width of the 64-bit key, query counts around a group of 16 and empty scans at the ends of the list.

Plain NumPy, seeded, no GPU and no library.  The truth of every fixture is `scan_pool_ref.pool(case, brute=True)`; means are
compared within `scan_pool_ref.bound`, counts exactly.  The limits are READ from the sources (`constants`).

* `key_layout` restates the host's bias / bits rule of the key;
* `flag_model` restates `ks_flag`'s walk over the chunk table, wave by wave and tile by tile, with its early stop;
* `pool_model` pools with those flags -- or with one of `WRONG_RULES`.
"""
from __future__ import annotations

import functools
import re

import numpy as np

import edge_geometry as eg
import points_cases as pc
import scan_pool_ref as sp
from autoinst_amd.camera_api import transform_points


# ------------------------------------------------------------------------------------------------- constants from the sources
def constants():
    src = pc._read(pc._CSRC, "ai_scanpool.hip")
    f = pc._find
    lanes = int(f(src, r"const int c = t \+ (\d+) \* k;", "the lanes per query of ks_pool"))
    if not re.search(r"gid >> 4;", src) or not re.search(r"gid & 15\)", src) or lanes != 16:
        raise RuntimeError("ks_pool no longer gives 16 lanes to a query")
    narrow_k = int(f(src, r"if \(dim <= \d+\)\s*hipLaunchKernelGGL\(ks_pool<(\d+)>", "the narrow ks_pool"))
    wide_k = int(f(src, r"else\s*hipLaunchKernelGGL\(ks_pool<(\d+)>", "the wide ks_pool"))
    c = dict(SP_TILE=int(f(src, r"^\s*#define\s+SP_TILE\s+(\d+)", "SP_TILE")), LANES=lanes, WAVE=64, AI_BLOCK=pc.K["AI_BLOCK"],
             NARROW=int(f(src, r"if \(dim <= (\d+)\)\s*hipLaunchKernelGGL", "the width limit of the narrow ks_pool")),
             WIDE=int(f(src, r"dim < 1 \|\| dim > (\d+)", "the widest row of ai_scan_pool")),
             AXIS_BITS=int(f(src, r"if \(bits\[a\] > (\d+)\)", "the bits of one axis of the key")),
             KEY_BITS=int(f(src, r"bits\[0\] \+ bits\[1\] \+ bits\[2\] > (\d+)\)", "the bits of the key")),
             MAX_INDEX=float(f(src, r"^\s*#define\s+SP_MAX_INDEX\s+([0-9.]+)", "SP_MAX_INDEX")))
    if c["NARROW"] != lanes * narrow_k or c["WIDE"] != lanes * wide_k or c["MAX_INDEX"] != 2.0 ** c["AXIS_BITS"]:
        raise RuntimeError("the ks_pool widths are no longer 16 lanes x MAXK, or the index limit is no longer 2^30")
    return c


K = constants()
TILE = K["SP_TILE"]
LANES = K["LANES"]
NARROW, WIDE = K["NARROW"], K["WIDE"]
KEY_REFUSAL = "do not fit a 64-bit key"


# ------------------------------------------------------------------------------------------------- the key
def bits_for(count):
    """`bits_for` of ai_entry.h: the bits that hold 0 .. count - 1."""
    b = 0
    while b < 63 and (1 << b) < count:
        b += 1
    return b


def key_layout(case):
    """The host's rule: per axis bias = floor(min lo * inv_cell) and bits = bits_for(floor(max hi * inv_cell) - bias + 1).
    dict(bias, bits, total, refused): refused names the entry's reason, or is None."""
    cell = case["radius"] * (1.0 + 1e-9)
    inv = 1.0 / cell
    lo, hi = case["boxes"][:, :3].min(axis=0), case["boxes"][:, 3:].max(axis=0)
    i0, i1 = np.floor(lo * inv), np.floor(hi * inv)
    refused = None
    if not (np.abs(i0) < K["MAX_INDEX"]).all() or not (np.abs(i1) < K["MAX_INDEX"]).all():
        refused = "index"
    bits = [bits_for(max(int(b) - int(a) + 1, 1)) for a, b in zip(i0, i1)]
    if refused is None and max(bits) > K["AXIS_BITS"]:
        refused = "axis"
    if refused is None and sum(bits) > K["KEY_BITS"]:
        refused = "key"
    return dict(bias=[int(a) for a in i0], bits=bits, total=sum(bits), refused=refused)


# ------------------------------------------------------------------------------------------------- ks_flag and the pooling
WRONG_RULES = ("first_tile", "stop_any", "cut16")
"""first_tile  only the first SP_TILE chunks of the table are examined;
stop_any    a wave leaves the table as soon as any of its points is placed (not: all of them);
cut16       the feature columns are cut at a multiple of 16 (the last, partial lane step is dropped)."""


def _sources(case):
    """Every scan point in the pcd frame (R1) with its scan position, in scan_xyz order."""
    pts = [transform_points(s, T) if s.shape[0] else np.zeros((0, 3)) for s, T in zip(case["scans"], case["T"])]
    pos = [np.full(s.shape[0], k, np.int64) for k, s in enumerate(case["scans"])]
    return (np.concatenate(pts) if pts else np.zeros((0, 3))), (np.concatenate(pos) if pos else np.zeros(0, np.int64))


def _inside(case, c, x, s):
    lo, hi = case["boxes"][c][:3], case["boxes"][c][3:]
    return (s >= case["wins"][c][0]) & (s < case["wins"][c][1]) & sp.crop_mask(x, lo, hi)


def flag_model(case, rule=None):
    """`ks_flag` on the CPU: keep (M,) bool.  A wave is 64 consecutive source points; the chunk table comes in tiles of SP_TILE; before
    every chunk the wave asks whether all its points are placed and leaves if so."""
    x, s = _sources(case)
    M, C = x.shape[0], len(case["chunks"])
    keep = np.zeros(M, dtype=bool)
    for w0 in range(0, M, K["WAVE"]):
        w = slice(w0, min(M, w0 + K["WAVE"]))
        placed = np.zeros(w.stop - w.start, dtype=bool)
        for base in range(0, C, TILE):
            if rule == "first_tile" and base:
                break
            for b in range(base, min(C, base + TILE)):
                if placed.all() or (rule == "stop_any" and placed.any()):
                    break
                placed |= _inside(case, b, x[w], s[w])
        keep[w] = placed
    return keep


def pool_model(case, rule=None):
    """Per chunk dict(mean, count): R2 over all pairs among the sources `flag_model` keeps, R3."""
    x, s = _sources(case)
    keep = flag_model(case, rule)
    feat = np.concatenate([np.asarray(f, np.float32).reshape(-1, case["dim"]) for f in case["feats"]] or [np.zeros((0, case["dim"]), np.float32)])
    f64 = feat.astype(np.float64)
    r2 = float(case["radius"]) * float(case["radius"])
    out = []
    for c, q in enumerate(case["chunks"]):
        ok = keep & _inside(case, c, x, s)
        mean, count = np.zeros((q.shape[0], case["dim"])), np.zeros(q.shape[0], np.int32)
        idx = np.flatnonzero(ok)
        for i in range(q.shape[0]):
            m = idx[eg.sq_plain(q[i], x[idx]) < r2] if idx.size else idx
            if m.size:
                mean[i], count[i] = f64[m].sum(axis=0) / m.size, m.size
        if rule == "cut16" and case["dim"] % LANES:
            mean[:, case["dim"] - case["dim"] % LANES:] = 0.0
        out.append({"mean": mean, "count": count})
    return out


def agrees(got, truth):
    """Counts equal, means within `scan_pool_ref.bound`, zero rows without members: what the GPU test asks of the device."""
    for g, r in zip(got, truth):
        if not np.array_equal(g["count"], r["count"]) or not np.all(np.abs(g["mean"] - r["mean"]) <= sp.bound(r)) or g["mean"][r["count"] == 0].any():
            return False
    return len(got) == len(truth)


# ------------------------------------------------------------------------------------------------- fixtures
def _scan_of(world, T):
    """Scan-frame points whose transform by the rigid T lands within rounding of ``world`` (the rounding is the data's)."""
    Ti = np.linalg.inv(T)
    return world @ Ti[:3, :3].T + Ti[:3, 3]


TILE_COUNTS = (TILE - 1, TILE, TILE + 1, 2 * TILE + 1)


@functools.lru_cache(maxsize=None)
def chunk_tiles_case(n_chunks):
    """``n_chunks`` disjoint unit boxes 2 m apart along x, every window [0, 2).  Chunk c has two queries and, in each of the two
    scans, two sources within 0.1 m of them and 0.2 m or more inside the box -- inside chunk c only.  The first scan's points are
    ordered so that its first wave of 64 holds 63 points of chunk 0's box next to one of the LAST chunk's (placed only by the last
    record of the last tile), and its second wave 32 points of chunk 0 next to 32 of chunk min(SP_TILE, last) -- the first record
    of the second tile where there is one."""
    rng = np.random.default_rng([71, n_chunks])
    last = n_chunks - 1
    boxes = np.array([[2.0 * c, 0.0, 0.0, 2.0 * c + 1.0, 1.0, 1.0] for c in range(n_chunks)]) + np.tile(eg.MAP_ORIGIN, 2)
    q = [boxes[c, :3] + rng.uniform(0.3, 0.7, (2, 3)) for c in range(n_chunks)]
    T = [sp.pose(0.4, 0.02, -0.01, eg.MAP_ORIGIN + [50.0, 3.0, 1.0]), sp.pose(-0.8, 0.01, 0.03, eg.MAP_ORIGIN + [500.0, -4.0, 1.5])]
    near = lambda c, n: q[c][np.arange(n) % 2] + rng.uniform(-0.06, 0.06, (n, 3))       # the queries in turn
    other = min(TILE, last)
    head = np.concatenate([near(0, 63), near(last, 1), near(0, 32), near(other, 32)])
    owner = [0] * 63 + [last] + [0] * 32 + [other] * 32
    rest = [c for c in range(1, n_chunks) for _ in range(2)]
    world0 = np.concatenate([head] + [near(c, 1) for c in rest])
    world1 = np.concatenate([near(c, 2) for c in range(n_chunks)])
    scans = [_scan_of(world0, T[0]), _scan_of(world1, T[1])]
    feats = [sp._feats(rng, s.shape[0], 17) for s in scans]
    return sp._case(scans, feats, T, q, boxes, [[0, 2]] * n_chunks, owner0=np.array(owner + rest), name=f"chunk_tiles_{n_chunks}")


DIMS = (1, LANES - 1, LANES, LANES + 1, NARROW - 1, NARROW, NARROW + 1, WIDE - 1, WIDE)


def _blob(rng, n_src, n_q, dim, n_chunks=1, split=None):
    """``n_chunks`` boxes of 1.5 m, 3 m apart, each with ``n_src`` sources in two scans and its share of ``n_q`` queries."""
    T = [sp.pose(0.3, 0.01, 0.02, eg.MAP_ORIGIN + [1.0, 2.0, 0.5]), sp.pose(1.1, -0.02, 0.0, eg.MAP_ORIGIN + [4.0, -1.0, 0.7])]
    split = split or [n_q // n_chunks + (1 if c < n_q % n_chunks else 0) for c in range(n_chunks)]
    boxes, qs, world = [], [], [[], []]
    for c in range(n_chunks):
        lo = eg.MAP_ORIGIN + [3.0 * c, 0.0, 0.0]
        boxes.append(np.concatenate([lo, lo + 1.5]))
        src = lo + rng.uniform(0.05, 1.45, (n_src, 3))
        world[0].append(src[: n_src // 2])
        world[1].append(src[n_src // 2:])
        qs.append(src[rng.integers(0, n_src, split[c])] + rng.uniform(-0.1, 0.1, (split[c], 3)))
    scans = [_scan_of(np.concatenate(w), t) for w, t in zip(world, T)]
    return sp._case(scans, [sp._feats(rng, s.shape[0], dim) for s in scans], T, qs, boxes, [[0, 2]] * n_chunks)


@functools.lru_cache(maxsize=None)
def dim_case(dim):
    """One chunk, 300 sources in a 1.5 m box, 17 queries, ``dim`` feature columns."""
    case = _blob(np.random.default_rng([72, dim]), 300, LANES + 1, dim)
    case["name"] = f"dim_{dim}"
    return case


QUERY_TOTALS = (1, LANES - 1, LANES, LANES + 1)


@functools.lru_cache(maxsize=None)
def query_tail_case(total, n_chunks):
    """``total`` queries in all, over one chunk or three (1 query over three chunks: the middle one has it)."""
    split = [0, 1, 0] if (total, n_chunks) == (1, 3) else None
    case = _blob(np.random.default_rng([73, total, n_chunks]), 200, total, 20, n_chunks, split)
    case["name"] = f"query_tail_{total}_over_{n_chunks}"
    return case


@functools.lru_cache(maxsize=None)
def empty_end_scans_case():
    """Five scans, the first and the last without a point; four chunks on the same box with the windows [0, 5) (both empty scans
    inside), [1, 4) (both outside), [0, 2) and [3, 5) (one inside, at either end of the window)."""
    rng = np.random.default_rng(74)
    lo = eg.MAP_ORIGIN.copy()
    src = lo + rng.uniform(0.05, 1.45, (300, 3))
    T = [sp.pose(0.2 * k, 0.01, -0.01 * k, eg.MAP_ORIGIN + [1.0 * k, 0.5, 0.2]) for k in range(5)]
    parts = [src[:0], src[:100], src[100:200], src[200:], src[:0]]
    scans = [_scan_of(p, t) for p, t in zip(parts, T)]
    feats = [sp._feats(rng, p.shape[0], 24) for p in parts]
    qs = [src[rng.integers(0, 300, 20)] + rng.uniform(-0.1, 0.1, (20, 3)) for _ in range(4)]
    box = np.concatenate([lo, lo + 1.5])
    return sp._case(scans, feats, T, qs, [box] * 4, [[0, 5], [1, 4], [0, 2], [3, 5]], name="empty_end_scans")


def _span_boxes(bits, negative=True):
    """Two 1.5 m boxes at opposite corners of a block whose cell range needs ``bits[a]`` key bits on axis a: the low corner box
    starts at cell -(2^(b - 1)) + 8 (``negative``) and the high corner box ends 2^b - 16 cells further on."""
    cell = sp.CELL
    lo_idx = np.array([-(1 << (b - 1)) + 8 if negative else 8 for b in bits], dtype=np.float64)
    hi_idx = lo_idx + np.array([(1 << b) - 16 for b in bits], dtype=np.float64)
    a = lo_idx * cell
    b = hi_idx * cell
    return np.array([np.concatenate([a, a + 1.5]), np.concatenate([b - 1.5, b])])


@functools.lru_cache(maxsize=None)
def key_bits_case(bits=(21, 21, 21)):
    """Two chunks at the far corners of a block of 2^21 x 2^21 x 2^21 cells (367 km a side; negative indices at one corner,
    positive at the other): the key needs 21 + 21 + 21 = 63 bits, the most the entry takes.  40 sources and 12 queries per corner,
    identity transform.  With ``bits`` = (22, 21, 21) every axis still fits its 30 bits but the key would need 64: refused."""
    rng = np.random.default_rng([75, sum(bits)])
    boxes = _span_boxes(bits)
    src = [b[:3] + rng.uniform(0.05, 1.45, (40, 3)) for b in boxes]
    qs = [s[rng.integers(0, 40, 12)] + rng.uniform(-0.1, 0.1, (12, 3)) for s in src]
    return sp._case([np.concatenate(src)], [sp._feats(rng, 80, 20)], [np.eye(4)], qs, boxes, [[0, 1], [0, 1]], name="key_%d_bits" % sum(bits))


def cases():
    """name -> builder of every fixture that the entry computes."""
    out = {f"chunk_tiles_{n}": functools.partial(chunk_tiles_case, n) for n in TILE_COUNTS}
    out.update({f"dim_{d}": functools.partial(dim_case, d) for d in DIMS})
    out.update({f"query_tail_{t}_over_{c}": functools.partial(query_tail_case, t, c) for t in QUERY_TOTALS for c in (1, 3)})
    out["empty_end_scans"] = empty_end_scans_case
    out["key_63_bits"] = key_bits_case
    return out


REJECTED_BY = {
    "first_tile": ("chunk_tiles_%d" % (TILE + 1), "chunk_tiles_%d" % (2 * TILE + 1)),
    "stop_any": tuple("chunk_tiles_%d" % n for n in TILE_COUNTS),
    "cut16": tuple(f"dim_{d}" for d in DIMS if d % LANES),
}
