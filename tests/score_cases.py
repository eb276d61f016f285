"""Fixtures of `ai_label_tables` (``autoinst_amd/csrc/ai_score.hip``, rules S1-S5), each on the kernel limit its name claims.

Pure NumPy, no GPU and no library: tests/test_score_cases.py proves the claims on the CPU (distinct pairs per row and per tile against
``np.unique``, the S2 boundary, the label sizes around ``min_points``), tests/test_gpu_score_cases.py feeds the device's answers to
`score_ref.check_tables`.  The limits are READ from the source (`constants`), the fixtures are derived from them.  Everything is
integers and flags: every check is an equality.
"""
from __future__ import annotations

import os
import re
from dataclasses import dataclass, field

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
_SRC = os.path.join(ROOT, "autoinst_amd", "csrc", "ai_score.hip")

I32_MIN, I32_MAX = -2 ** 31, 2 ** 31 - 1


def constants():
    with open(_SRC) as f:
        text = f.read()
    out = {}
    for name in ("KS_TILE", "KS_LDS_SLOTS", "KS_LDS_PROBES", "KS_TABLE_MIN", "KS_TABLE_MAX", "KS_LOAD_DEN", "KS_MAX_ROWS"):
        m = re.search(r"^\s*#define\s+" + name + r"\s+(\d+)\s*(?://.*)?$", text, re.M)
        if not m:
            raise RuntimeError(f"#define {name} <integer> not found in ai_score.hip")
        out[name] = int(m.group(1))
    return out


K = constants()
TILE = K["KS_TILE"]
LDS_SLOTS = K["KS_LDS_SLOTS"]
FIT_MIN = K["KS_TABLE_MIN"] // K["KS_LOAD_DEN"]      # the most distinct pairs a row's first table takes
FIT_MAX = K["KS_TABLE_MAX"] // K["KS_LOAD_DEN"]      # the most its second one takes: one more and the row is sorted
MAX_ROWS = K["KS_MAX_ROWS"]

LENGTHS = (0, 1, TILE - 1, TILE, TILE + 1, 3 * TILE + 5)
ROW_COUNTS = (1, 2, 16, MAX_ROWS)
BOUNDARY_M = (5, 10, 15, 35, 1000)
BOUNDARY_BIG_M = 5 * 2 ** 20
SIZES_AROUND_MIN = (199, 200, 201)
ONE_PAIR_POINTS = 8 * 2 ** 20


@dataclass
class ScoreCase:
    name: str
    preds: np.ndarray            # (k, n) int32
    gt: np.ndarray               # n int32
    threshold: float = 0.8
    min_points: int = 200
    claims: dict = field(default_factory=dict)


def _case(name, preds, gt, threshold=0.8, min_points=200, **claims):
    preds = np.ascontiguousarray(np.asarray(preds, np.int32).reshape(len(preds), -1))
    return ScoreCase(name, preds, np.ascontiguousarray(gt, dtype=np.int32), float(threshold), int(min_points), claims)


def distinct_per_row(c):
    key = (c.preds.astype(np.int64) << 32) | (c.gt.astype(np.int64)[None, :] & 0xFFFFFFFF)
    return [int(np.unique(r).size) for r in key]


def distinct_per_tile(c, row=0):
    key = (c.preds[row].astype(np.int64) << 32) | (c.gt.astype(np.int64) & 0xFFFFFFFF)
    return [int(np.unique(key[a:a + TILE]).size) for a in range(0, key.size, TILE)]


# ------------------------------------------------------------------------------------------------- shapes
def random_case(k, n, seed=0):
    """k rows over one ground truth with a ground (gt 0) that holds about half the points; row t unites the truth's instances
    under its own map and scatters some noise, so labels are removed, small and ordinary in every row."""
    rng = np.random.default_rng([seed, k, n])
    gt = np.where(rng.random(n) < 0.5, 0, rng.integers(1, 40, n)).astype(np.int32)
    preds = np.empty((k, n), np.int32)
    for t in range(k):
        maps = rng.integers(-2, 12 + t, 40)
        p = maps[gt]
        noise = rng.random(n) < 0.1
        p[noise] = rng.integers(-3, 60, int(noise.sum()))
        preds[t] = p
    return _case(f"random_k{k}_n{n}", preds, gt, 0.8, max(1, n // 100), k=k, n=n)


N_GT = 3


def distinct_case(name, n, d, extra_rows=(), seed=0):
    """Row 0 has exactly d distinct pairs in n >= d points, the further rows ``extra_rows`` of them, over one ground truth with the
    values 0, 1, 2 (so at least 3 per row).  Before the shuffle point i has gt = i % 3; in a row with e pairs point i < e carries
    pair number i, (i // 3 - 40, i % 3), and every later point repeats one of the pairs that have its gt."""
    counts = (d,) + tuple(extra_rows)
    assert all(N_GT <= e <= n for e in counts)
    rng = np.random.default_rng([seed, n, d])
    i = np.arange(n, dtype=np.int64)
    g = i % N_GT
    preds = np.empty((len(counts), n), np.int32)
    for t, e in enumerate(counts):
        with_gt = (e - g + N_GT - 1) // N_GT                      # pairs among the first e that have this gt: >= 1
        preds[t] = np.where(i < e, i // N_GT, rng.integers(0, 2 ** 31, n) % with_gt) - 40
    perm = rng.permutation(n)
    return _case(name, preds[:, perm], g[perm], 0.8, 3, distinct=list(counts))


def tile_cases():
    out = [distinct_case(f"tile_{d}_pairs", TILE, d) for d in (LDS_SLOTS - 1, LDS_SLOTS, LDS_SLOTS + 1)]
    out.append(distinct_case("tile_every_point_a_pair", TILE, TILE))
    return out


def table_cases():
    return [distinct_case(f"table_{d}_pairs", d + TILE + 7, d) for d in (FIT_MIN - 1, FIT_MIN, FIT_MIN + 1)]


def fallback_case():
    """One row that just fits the largest table, one that is sorted, one with three pairs: side by side in one call."""
    return distinct_case("fallback_side_by_side", FIT_MAX + 1 + 2 * TILE + 11, FIT_MAX, extra_rows=(FIT_MAX + 1, 3))


def extremes_case():
    """The pairs whose packed key is all zeros and all ones -- as raw bits (0, 0) / (-1, -1) and in the sort's biased form
    (INT32_MIN, INT32_MIN) / (INT32_MAX, INT32_MAX) -- and the extreme labels in every combination, beside ordinary pairs."""
    rng = np.random.default_rng(41)
    ext = np.array([I32_MIN, -1, 0, 1, I32_MAX], np.int64)
    grid = np.stack(np.meshgrid(ext, ext, indexing="ij"), -1).reshape(-1, 2)
    ordinary = np.stack([rng.integers(2, 30, 6000), rng.integers(0, 9, 6000)], 1)
    rows = np.concatenate([grid, grid[rng.integers(0, 25, 3000)], ordinary])
    rng.shuffle(rows)
    return _case("extremes", [rows[:, 0]], rows[:, 1], 0.5, 150, distinct_extreme=25)


def one_pair_case():
    return _case("one_pair_8M", [np.full(ONE_PAIR_POINTS, 3, np.int32)], np.zeros(ONE_PAIR_POINTS, np.int32), 0.8, 200, pairs=1)


# ------------------------------------------------------------------------------------------------- S2, S3
def boundary_labels(ms, first_label=10):
    """Per m two labels: ``first_label + 2 j`` with z = 4 m / 5 points on gt 0 and ``first_label + 2 j + 1`` with one more; the other
    points of a label have gt 7.  Returns (pred, gt, {label: (m, z)})."""
    pred, gt, what = [], [], {}
    for j, m in enumerate(ms):
        assert m % 5 == 0
        for extra in (0, 1):
            u, z = first_label + 2 * j + extra, 4 * m // 5 + extra
            pred.append(np.full(m, u, np.int32))
            g = np.full(m, 7, np.int32)
            g[:z] = 0
            gt.append(g)
            what[u] = (m, z)
    return np.concatenate(pred), np.concatenate(gt), what


def boundary_case(ms=BOUNDARY_M, name="boundary", threshold=0.8, seed=3):
    """The labels of `boundary_labels`, label 0 with 10 of its 12 points on gt 0 (removed by the rule, unchanged by the removal) and
    label -4 with no point there, shuffled."""
    p, g, what = boundary_labels(ms)
    p = np.concatenate([p, np.zeros(12, np.int32), np.full(9, -4, np.int32)])
    g = np.concatenate([g, np.array([0] * 10 + [5, 6], np.int32), np.arange(1, 10, dtype=np.int32)])
    what[0], what[-4] = (12, 10), (9, 0)
    perm = np.random.default_rng(seed).permutation(p.size)
    return _case(name, [p[perm]], g[perm], threshold, 0, labels=what)


def min_points_cases():
    """Labels of exactly 199, 200 and 201 points (and label 0 with 50), at min_points 0, 1 and 200."""
    rng = np.random.default_rng(8)
    p = np.concatenate([np.full(s, 20 + j, np.int32) for j, s in enumerate(SIZES_AROUND_MIN)] + [np.zeros(50, np.int32)])
    g = rng.integers(0, 4, p.size).astype(np.int32)
    perm = rng.permutation(p.size)
    return [_case(f"min_points_{mp}", [p[perm]], g[perm], 0.8, mp, sizes={20 + j: s for j, s in enumerate(SIZES_AROUND_MIN)})
            for mp in (0, 1, 200)]


def small_cases():
    """Every fixture a per-label NumPy pass can check in well under a second."""
    out = [random_case(1, n) for n in LENGTHS] + [random_case(k, TILE + 1) for k in ROW_COUNTS[1:]]
    return out + tile_cases() + [extremes_case(), boundary_case()] + min_points_cases()


def small_case(name):
    return next(c for c in small_cases() if c.name == name)


SMALL_NAMES = [c.name for c in small_cases()]
