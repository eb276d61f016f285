"""Fixtures and host model for the grid limits of both affinity builds and for the groups of the batched one
(``autoinst_amd/csrc/ai_affinity.hip``: `affinity_grid`; ``ai_affinity_batch.inc``: `affinity_groups`, `k_b_bounds`, the split).

NumPy only.  tests/test_affinity_batch_cases.py proves on the CPU that every fixture sits where its name says;
tests/test_gpu_affinity_batch_cases.py sends the same fixtures through the device.

Two parts:

* the host model -- `affinity_grid` (`affinity_cases.grid_of` plus the refusals), `affinity_groups` (budget, ``cap - 1``, the
  chunk cap), the split recursion (lower half first, ``mid = lo + (hi - lo) // 2``), the blocks `k_b_bounds` gives a chunk and
  the rows each of its threads reads, and the group's sort on ``chunk << 30 | Morton key``.  `group_plan` returns what a call
  builds, in order, and what it tried and split.  `VARIANTS` are deliberately wrong models: each changes the plan or the
  expected result of the fixtures in `REJECTED_BY`, which is how the fixtures are shown to discriminate.
* `calls()`: the fixtures.  A `Call` is the chunks of one batched call with its weights, its ``group_rows`` and the plan it
  claims (`built`, `split`, `error`, `blocks`).

The model covers the half of the split condition that a few points can reach (more than 2^28 cells in a group); a group of
2^31 entries is not modelled."""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

import affinity_cases as ac

# ---- the sources' constants; a change there must be made here too, and the claims then re-proven
AI_BLOCK = 256
BOUNDS_ROWS = 16 * AI_BLOCK          # rows of the longest chunk per block of k_b_bounds
BOUNDS_MAX_BLOCKS = 256              # ... and the most blocks a chunk gets
KEY_BITS = 30                        # AI_KEY_BITS: the Morton key, 10 bits per axis
AXIS_LIMIT = 1023.0                  # extent / cell of an axis stays below this
CELL_LIMIT = 1 << 28                 # cells of one chunk, and of one group of several chunks
DEFAULT_GROUP_ROWS = 1 << 21         # AB_DEFAULT_GROUP_ROWS
MAX_ROWS = 1 << 30                   # AI_MAX_ROWS
MAX_GROUP_CHUNKS = 65535             # AB_MAX_GROUP_CHUNKS: gridDim.y of k_b_bounds
EXTENT_LIMIT = 1e15
OK, NOT_FINITE, AXIS, CELLS = 0, 1, 2, 3
MESSAGE = {NOT_FINITE: "not finite", AXIS: "1023 cells per axis", CELLS: "dense cell-table limit"}
RADIUS = 1.0
G = 2.0 ** -10                       # the coordinate grid of the fixtures


def bits_for(count):
    """ai_entry.h: bits that hold 0 .. count - 1."""
    b = 0
    while b < 63 and (1 << b) < count:
        b += 1
    return b


# ------------------------------------------------------------------------------------------------- the grid of one cloud
def affinity_grid(mn, mx, radius=RADIUS):
    """`affinity_grid` of ai_affinity.hip on a bounding box: (why, (nx, ny, nz) or None, cells)."""
    mn, mx = np.asarray(mn, dtype=np.float64), np.asarray(mx, dtype=np.float64)
    with np.errstate(invalid="ignore"):
        if not ((mn <= mx).all() and (mx - mn < EXTENT_LIMIT).all()):
            return NOT_FINITE, None, 0
    cell = radius * (1.0 + 1e-9)
    ext = (mx - mn) / cell
    if (ext >= AXIS_LIMIT).any():
        return AXIS, None, 0
    dims = tuple(int(d) for d in np.floor(ext).astype(np.int64) + 1)
    ncell = dims[0] * dims[1] * dims[2]
    return (CELLS if ncell > CELL_LIMIT else OK), dims, ncell


def single_grid(points, radius=RADIUS):
    """What ``ai_affinity_build`` makes of a cloud: `k_bounds` (fmin / fmax pass a NaN by), then `affinity_grid`."""
    p = np.asarray(points, dtype=np.float64)
    return affinity_grid(np.fmin(np.fmin.reduce(p, axis=0), 1e300), np.fmax(np.fmax.reduce(p, axis=0), -1e300), radius)


def axis_limit(mn, radius=RADIUS):
    """The largest double ``mx`` with ``(mx - mn) / cell < 1023`` in the float64 expression of `affinity_grid`."""
    cell = radius * (1.0 + 1e-9)
    mx = np.float64(mn) + AXIS_LIMIT * cell
    while (mx - mn) / cell >= AXIS_LIMIT:
        mx = np.nextafter(mx, -np.inf)
    while (np.nextafter(mx, np.inf) - mn) / cell < AXIS_LIMIT:
        mx = np.nextafter(mx, np.inf)
    return float(mx)


def cell_ids(points, radius=RADIUS):
    """``(cz * ny + cy) * nx + cx`` of every point, and the cell count."""
    _, _, dims, c = ac.grid_of(points, radius)
    return (c[:, 2] * dims[1] + c[:, 1]) * dims[0] + c[:, 0], dims[0] * dims[1] * dims[2]


# ------------------------------------------------------------------------------------------------- k_b_bounds
def bounds_blocks(longest):
    """S: the blocks every chunk of a group gets, from the group's longest chunk."""
    return int(min(BOUNDS_MAX_BLOCKS, max(1, -(-int(longest) // BOUNDS_ROWS))))


def bounds_rows(n, S, s, t):
    """Local rows of a chunk of n rows that thread t of block s reads, trip by trip: ``i = r0 + s * 256 + t``, step ``S * 256``."""
    return list(range(s * AI_BLOCK + t, n, S * AI_BLOCK))


def extreme_rows(n):
    """(row of the minimum, row of the maximum) of a bounds fixture of n rows: the last rows that thread 0 and thread 255 of the
    LAST block read -- rows no other block sees, on that thread's last trip."""
    S = bounds_blocks(n)
    return bounds_rows(n, S, S - 1, 0)[-1], bounds_rows(n, S, S - 1, AI_BLOCK - 1)[-1]


def group_boxes(xyz, off, lo, hi, radius=RADIUS, first_trip_only=False):
    """Per chunk of the group lo .. hi: (S, why[nc], cells[nc], dims[nc, 3]) as `k_b_bounds`, the fold over the S records and `affinity_grid`
    give them.  ``first_trip_only``: the wrong kernel whose threads stop after their first row."""
    rows = np.asarray(off[lo:hi + 1], dtype=np.int64)
    n = np.diff(rows)
    S = bounds_blocks(n.max())
    seg = np.array(xyz[rows[0]:rows[-1]], dtype=np.float64)
    start = rows[:-1] - rows[0]
    seen = np.ones(seg.shape[0], dtype=bool)
    if first_trip_only:
        seen = (np.arange(seg.shape[0]) - np.repeat(start, n)) < S * AI_BLOCK
    bad = np.add.reduceat((~np.isfinite(seg).all(1) & seen).astype(np.int64), start) > 0
    seg[~seen] = np.nan                                        # fmin / fmax pass a NaN by, as the device's do
    mn = np.fmin(np.fmin.reduceat(seg, start, axis=0), 1e300)
    mx = np.fmax(np.fmax.reduceat(seg, start, axis=0), -1e300)
    why = np.zeros(n.size, dtype=np.int64)
    cell = radius * (1.0 + 1e-9)
    with np.errstate(invalid="ignore", over="ignore"):
        d = mx - mn
        notfin = bad | ~((mn <= mx).all(1) & (d < EXTENT_LIMIT).all(1))
        ext = d / cell
        axis = (ext >= AXIS_LIMIT).any(1)
        dims = np.where((notfin | axis)[:, None], 1, np.floor(np.where(np.isfinite(ext), ext, 0.0)).astype(np.int64) + 1)
    cells = dims[:, 0] * dims[:, 1] * dims[:, 2]
    why[cells > CELL_LIMIT] = CELLS
    why[axis] = AXIS
    why[notfin] = NOT_FINITE
    cells[why == NOT_FINITE] = 0
    cells[why == AXIS] = 0
    return S, why, cells, dims


# ------------------------------------------------------------------------------------------------- groups and the split
def affinity_groups(off, budget, widest, chunk_cap=MAX_GROUP_CHUNKS):
    """`affinity_groups` of ai_affinity_batch.inc: the cuts.  ``chunk_cap=None``: the grouping without the chunk cap."""
    n_chunks = len(off) - 1
    cap = min(MAX_ROWS, ((1 << 33) + widest - 1) // widest if widest > 0 else MAX_ROWS)
    lim = min(budget, cap - 1)
    cut = [0]
    for c in range(n_chunks):
        if c > cut[-1] and (off[c + 1] - off[cut[-1]] > lim or (chunk_cap is not None and c - cut[-1] >= chunk_cap)):
            cut.append(c)
    cut.append(n_chunks)
    return cut


@dataclass
class Plan:
    groups: list            # (lo, hi) as `affinity_groups` cuts the call
    built: list             # (lo, hi) of every group that is built, in order
    split: list             # (lo, hi) of every group that was tried and halved
    error: tuple | None     # (chunk, why) that ends the call, or None
    blocks: dict            # (lo, hi) -> S of every group tried
    cells: dict             # (lo, hi) -> cells of every group tried (0 for one that is refused)

    def key(self):
        return (tuple(self.groups), tuple(self.built), tuple(self.split), self.error)


def group_plan(offsets, clouds, radius=RADIUS, group_rows=None, widest=0, *, split_ge=False, mid_up=False, chunk_cap=MAX_GROUP_CHUNKS,
               first_trip_only=False):
    """What ``ai_affinity_build_batch`` does with the chunks ``offsets`` of ``clouds`` (a list of per-chunk arrays, or the
    concatenated rows): see `Plan`.  The keyword arguments after ``widest`` are the wrong variants."""
    off = [int(o) for o in offsets]
    xyz = np.concatenate([np.asarray(c, dtype=np.float64).reshape(-1, 3) for c in clouds]) if isinstance(clouds, (list, tuple)) \
        else np.asarray(clouds, dtype=np.float64)
    assert xyz.shape[0] == off[-1] and off[0] == 0
    cut = affinity_groups(off, group_rows if group_rows and group_rows > 0 else DEFAULT_GROUP_ROWS, widest, chunk_cap)
    groups = [(cut[g], cut[g + 1]) for g in range(len(cut) - 1)]
    plan = Plan(groups, [], [], None, {}, {})
    todo = groups[::-1]
    while todo:
        lo, hi = todo.pop()
        S, why, cells, _ = group_boxes(xyz, off, lo, hi, radius, first_trip_only)
        plan.blocks[(lo, hi)] = S
        refused = np.nonzero(why)[0]
        if refused.size:
            plan.error = (lo + int(refused[0]), int(why[refused[0]]))
            plan.cells[(lo, hi)] = 0
            break
        total = int(cells.sum())
        plan.cells[(lo, hi)] = total
        if hi - lo > 1 and (total >= CELL_LIMIT if split_ge else total > CELL_LIMIT):
            plan.split.append((lo, hi))
            mid = lo + (hi - lo + 1) // 2 if mid_up else lo + (hi - lo) // 2
            todo.append((mid, hi))
            todo.append((lo, mid))
            continue
        plan.built.append((lo, hi))
    return plan


# ------------------------------------------------------------------------------------------------- the group's sort
def group_order(clouds, radius=RADIUS, key_bits=None):
    """order[p] = row of the group's input at position p: a stable sort on the low ``key_bits`` bits of ``chunk << 30 | Morton
    key`` (every chunk on its own grid).  None: the library's ``30 + bits_for(chunks)``."""
    nc = len(clouds)
    key_bits = KEY_BITS + bits_for(nc) if key_bits is None else key_bits
    keys = np.concatenate([(np.uint64(c) << np.uint64(KEY_BITS)) | ac.morton_keys(ac.grid_of(p, radius)[3]) for c, p in enumerate(clouds)])
    return np.argsort(keys & np.uint64((1 << key_bits) - 1), kind="stable")


def order_keeps_chunks(order, clouds, radius=RADIUS):
    """Whether every chunk's range of positions holds that chunk's rows in the single build's order."""
    r0 = 0
    for p in clouds:
        n = p.shape[0]
        if not np.array_equal(order[r0:r0 + n] - r0, ac.library_order(p, radius)):
            return False
        r0 += n
    return True


# ------------------------------------------------------------------------------------------------- fixtures
@dataclass
class Chunk:
    name: str
    points: np.ndarray
    tarl: np.ndarray | None = None
    dino: np.ndarray | None = None
    _cases: dict = field(default_factory=dict)

    @property
    def n(self):
        return self.points.shape[0]

    def case(self, theta, gamma):
        """The chunk as an `affinity_cases.Case`, for `check_affinity`."""
        k = (theta, gamma)
        if k not in self._cases:
            self._cases[k] = ac.Case(self.name, self.points, self.tarl if theta else None, self.dino if gamma else None, theta=theta, gamma=gamma,
                                     radius=RADIUS)
        return self._cases[k]


@dataclass
class Call:
    name: str
    chunks: list
    theta: float = 0.0
    gamma: float = 0.0
    group_rows: int | None = None
    built: list | None = None          # the claimed plan
    split: list = field(default_factory=list)
    error: tuple | None = None
    blocks: int | None = None          # claimed S of the first group
    anchors: tuple = ()                # chunks that also go through `check_affinity`
    big: bool = False                  # needs the 2^28-cell workspace: runs on a context of its own
    note: str = ""
    _plans: dict = field(default_factory=dict)

    @property
    def kw(self):
        return dict(alpha=1.0, theta=self.theta, gamma=self.gamma, radius=RADIUS)

    @property
    def widest(self):
        return max(16 if self.theta else 0, 32 if self.gamma else 0)

    @property
    def offsets(self):
        return np.cumsum([0] + [c.n for c in self.chunks])

    def plan(self, **variant):
        k = tuple(sorted(variant.items()))
        if k not in self._plans:
            self._plans[k] = group_plan(self.offsets, [c.points for c in self.chunks], RADIUS, self.group_rows, self.widest, **variant)
        return self._plans[k]


def _features(rng, n):
    return ac._features(rng, n, 16, 32)


def _with_features(name, points, seed):
    t, d = _features(np.random.default_rng(seed), points.shape[0])
    return Chunk(name, points, t, d)


_MEMO = {}


def _memo(key, make):
    if key not in _MEMO:
        _MEMO[key] = make()
    return _MEMO[key]


# ---- 1. the axis limit
LINE_STEPS = 2046      # points 0, 0.5, .. 1022.5, then the one that carries the extent


def line(axis, over=False, shift=None):
    """A line along `axis`: 2046 points 0.5 apart from the minimum, and a last one at the largest coordinate that `affinity_grid`
    accepts (``over``: the next double up).  The other two coordinates are constant."""
    mn = np.zeros(3) if shift is None else np.asarray(shift, dtype=np.float64)
    a = "xyz".index(axis)
    top = axis_limit(mn[a])
    x = np.concatenate([mn[a] + 0.5 * np.arange(LINE_STEPS), [np.nextafter(top, np.inf) if over else top]])
    p = np.tile(mn, (x.size, 1))
    p[:, a] = x
    return p


def line_chunk(axis, over=False, shifted=False):
    name = f"long_{axis}" + ("_map" if shifted else "") + ("_over" if over else "")
    return _memo(name, lambda: _with_features(name, line(axis, over, ac.MAP_SHIFT if shifted else None), 40 + "xyz".index(axis)))


LINE_NAMES = ["long_x", "long_y", "long_z", "long_x_map"]


# ---- 2. and 4.: boxes
def box(a, b, c, seed, corners=(0, 7)):
    """A handful of points whose grid has a x b x c cells: the box [0, a - 0.5] x [0, b - 0.5] x [0, c - 0.5], both extreme
    corners themselves, a cluster of 10 points within 0.25 of every corner listed in `corners` (bit k of a corner's number: the
    far side of axis k), one point on the far end of every axis and one in the middle."""
    rng = np.random.default_rng(seed)
    E = np.array([a, b, c], dtype=np.float64) - 0.5
    pts = [np.zeros((1, 3)), E[None], np.diag(E), E[None] / 2]
    for k in corners:
        far = np.array([(k >> i) & 1 for i in range(3)], dtype=np.float64)
        j = rng.integers(0, 257, (10, 3)).astype(np.float64) * G
        pts.append(far * (E - j) + (1 - far) * j)
    p = np.concatenate(pts)
    return p[rng.permutation(p.shape[0])]


def box_chunk(a, b, c, seed, corners=(0, 7)):
    name = f"box_{a}_{b}_{c}_s{seed}"
    return _memo(name, lambda: _with_features(name, box(a, b, c, seed, corners), seed))


def cells_at_limit():
    return box_chunk(1023, 512, 512, 60, corners=tuple(range(8)))


def cells_over():
    return box_chunk(1023, 513, 512, 61, corners=tuple(range(8)))


def nan_chunk(seed=70):
    def make():
        p = np.random.default_rng(seed).integers(0, 4096, (20, 3)).astype(np.float64) * G
        p[7, 2] = np.nan
        return Chunk("nan_chunk", p)
    return _memo(("nan", seed), make)


def mix_chunks():
    """The chunks of tests/test_gpu_affinity_batch.py's MIX, points only."""
    names = ["walk_line", "walk_sheet", "walk_3d", "walk_3d_negative", "walk_3d_map", "tail_1", "tail_2", "tail_15", "tail_16", "tail_17",
             "tail_31", "tail_32", "tail_33", "tail_1025", "tail_1023"]
    return _memo("mix", lambda: [Chunk("mix_" + n, ac.case(n).points) for n in names])


# ---- 3. one cloud cut into many chunks
CUT_CHUNKS = 257
CHUNK_COUNTS = [1, 2, 3, 16, 17, 255, 256, 257]
ONE_ROW_RUNS = [(4, 8), (13, 16), (251, 256)]


def cut_chunks():
    """257 chunks of 1 .. 40 rows of ONE random cloud (every chunk spans the whole cloud), with runs of one-row chunks."""
    def make():
        rng = np.random.default_rng(31)
        sizes = rng.integers(1, 41, CUT_CHUNKS)
        for a, b in ONE_ROW_RUNS:
            sizes[a:b] = 1
        n = int(sizes.sum())
        p = np.round(rng.normal(0, 1.2, (n, 3)) / G) * G
        t, d = _features(rng, n)
        off = np.cumsum(np.r_[0, sizes])
        return [Chunk(f"cut_{k}", p[off[k]:off[k + 1]], t[off[k]:off[k + 1]], d[off[k]:off[k + 1]]) for k in range(CUT_CHUNKS)]
    return _memo("cut", make)


def chunks_call(nc):
    ch = list(cut_chunks()[:nc])
    if nc in (17, 257):       # the top Morton bits under the highest chunk id, and under chunk 0
        ch[0], ch[-1] = line_chunk("x"), line_chunk("z")
    return Call(f"chunks_{nc}", ch, theta=0.5, gamma=0.1, built=[(0, nc)], blocks=1, anchors=tuple(sorted({0, nc // 2, nc - 1})))


# ---- 5. k_b_bounds with several blocks per chunk
BOUNDS_NS = [4096, 4097, 8193]
BOUNDS_VARIANTS = ["plain", "over", "nan", "+inf", "-inf"]
LATTICE = (102, 101, 102)
LATTICE_STEP = 0.75


def bounds_long(n, variant="plain"):
    """n points along x (y, z inside half a cell).  The point that alone carries the minimum of x sits in the row `extreme_rows`
    names first, the one that alone carries the maximum (the axis limit itself) in the second."""
    rng = np.random.default_rng(500 + n)
    p = np.c_[rng.integers(1024, 1022 * 1024, n), rng.integers(0, 513, (n, 2))].astype(np.float64) * G
    r_min, r_max = extreme_rows(n)
    top = axis_limit(0.0)
    p[r_min] = [0.0, 0.25, 0.25]
    p[r_max] = [top, 0.25, 0.25]
    if variant == "over":
        p[r_max, 0] = np.nextafter(top, np.inf)
    elif variant == "nan":
        p[r_max, 1] = np.nan
    elif variant == "+inf":
        p[r_max, 0] = np.inf
    elif variant == "-inf":
        p[r_min, 2] = -np.inf
    else:
        assert variant == "plain"
    return p


def _small_chunks(seed):
    rng = np.random.default_rng(seed)
    one = Chunk("one_point", rng.integers(0, 4096, (1, 3)).astype(np.float64) * G)
    small = Chunk("small_300", np.round(rng.normal(0, 1.5, (300, 3)) / G) * G + np.array([500.0, 0, 0]))
    return one, small


def bounds_call(n, variant="plain"):
    one, small = _memo(("small", n), lambda: _small_chunks(600 + n))
    long = _memo(("bounds", n, variant), lambda: Chunk(f"bounds_{n}_{variant}", bounds_long(n, variant)))
    why = {"plain": None, "over": AXIS}.get(variant, NOT_FINITE)
    name = f"bounds_{n}" + ("" if variant == "plain" else "_" + variant)
    return Call(name, [one, long, small], built=[(0, 3)] if why is None else [], error=None if why is None else (1, why),
                blocks=bounds_blocks(n), anchors=(1,) if why is None else ())


def lattice():
    def make():
        g = np.stack(np.meshgrid(*[np.arange(k) for k in LATTICE], indexing="ij"), axis=-1).reshape(-1, 3)
        return Chunk("lattice", g.astype(np.float64) * LATTICE_STEP)
    return _memo("lattice", make)


def bounds_cap_call():
    _, small = _memo(("small", 0), lambda: _small_chunks(600))
    return Call("bounds_cap", [small, lattice()], built=[(0, 2)], blocks=BOUNDS_MAX_BLOCKS)


# ---- 6. more chunks than a grid has rows
MANY = 65536


def many_chunks(nan_at=None):
    """65 536 one-point chunks as concatenated rows: (points, offsets)."""
    p = np.random.default_rng(80).integers(0, 30 * 1024, (MANY, 3)).astype(np.float64) * G
    if nan_at is not None:
        p[nan_at, 1] = np.nan
    return p, np.arange(MANY + 1, dtype=np.int64)


# ---- the calls
def _split_calls():
    b512 = lambda s: box_chunk(512, 512, 512, s)
    pair = [box_chunk(512, 512, 513, 91), b512(92)]            # the larger first: see the workspace bound in the GPU test
    deep = [box_chunk(512, 512, 256, 100 + k) for k in range(4)] + [box_chunk(1023, 512, 168, 104 + k) for k in range(4)]
    mix = mix_chunks()
    mix_rows = sum(c.n for c in mix)
    out = [
        Call("split_pair", pair, theta=0.5, gamma=0.1, built=[(0, 1), (1, 2)], split=[(0, 2)], anchors=(0, 1), big=True,
             note="2^27 + 2^18 and 2^27 cells: 2^18 over"),
        Call("split_control", [b512(93), b512(94)], built=[(0, 2)], anchors=(1,), big=True, note="exactly 2^28 cells: the test is >"),
        Call("split_three", [b512(95), box_chunk(1023, 512, 256, 96), b512(97)], theta=0.5, gamma=0.1, built=[(0, 1), (1, 3)], split=[(0, 3)],
             anchors=(2,), big=True),
        Call("split_five", [b512(93), box_chunk(1023, 256, 512, 98), b512(94), box_chunk(256, 1023, 512, 99), b512(95)],
             built=[(0, 2), (2, 3), (3, 5)], split=[(0, 5), (2, 5)], anchors=(3,), big=True),
        Call("split_deep", deep, built=[(0, 4), (4, 6), (6, 8)], split=[(0, 8), (4, 8)], anchors=(7,), big=True,
             note="four boxes of 2^26 cells fit exactly; of the four of 87 994 368 cells any three fit, four do not"),
        Call("split_second_group", mix + pair, group_rows=mix_rows, built=[(0, 15), (15, 16), (16, 17)], split=[(15, 17)], big=True),
        Call("split_then_error", pair + [nan_chunk()], group_rows=pair[0].n + pair[1].n, built=[(0, 1), (1, 2)], split=[(0, 2)],
             error=(2, NOT_FINITE), big=True),
        Call("cells_over_in_the_middle", [box_chunk(4, 5, 6, 110), cells_over(), box_chunk(6, 5, 4, 111)], built=[], error=(1, CELLS), big=True),
    ]
    return out


def _limit_calls():
    out = []
    for nm in LINE_NAMES:
        ax = nm[5]
        ch = line_chunk(ax, shifted=nm.endswith("_map"))
        out.append(Call(nm, [ch], built=[(0, 1)], blocks=1, anchors=(0,)))
        over = line_chunk(ax, over=True, shifted=nm.endswith("_map"))
        out.append(Call(nm + "_over", [cut_chunks()[0], over], built=[], error=(1, AXIS)))
    out.append(Call("cells_at_limit", [cells_at_limit()], built=[(0, 1)], anchors=(0,), big=True))
    out.append(Call("cells_over", [cut_chunks()[0], cut_chunks()[1], cells_over()], built=[], error=(2, CELLS), big=True))
    return out


def calls():
    """name -> Call, built once per process."""
    def make():
        out = _limit_calls() + [chunks_call(nc) for nc in CHUNK_COUNTS] + _split_calls()
        out += [bounds_call(n, v) for n in BOUNDS_NS for v in BOUNDS_VARIANTS] + [bounds_cap_call()]
        return {c.name: c for c in out}
    return _memo("calls", make)


def call(name):
    return calls()[name]


# ------------------------------------------------------------------------------------------------- wrong models
VARIANTS = {
    "key_bits_short": "the sort covers 30 + bits_for(chunks - 1) bits",
    "split_ge": "a group splits at >= 2^28 cells",
    "mid_up": "the middle of a split is rounded up",
    "first_trip_only": "a thread of k_b_bounds stops after its first row",
    "no_chunk_cap": "a group takes any number of chunks",
}
REJECTED_BY = {
    "key_bits_short": ("chunks_2", "chunks_3", "chunks_17", "chunks_257", "split_control", "bounds_4096", "bounds_4097", "bounds_8193", "bounds_cap"),
    "split_ge": ("split_control", "split_deep"),
    "mid_up": ("split_three", "split_five"),
    "first_trip_only": tuple(f"bounds_{n}{v}" for n in BOUNDS_NS for v in ("", "_over", "_nan", "_+inf", "_-inf")) + ("bounds_cap",),
    "no_chunk_cap": ("many_chunks",),
}


def rejects(c: Call, variant):
    """Whether the wrong model `variant` gives this call another plan, or another result, than the shipped model."""
    if variant == "key_bits_short":
        clouds = [ch.points for ch in c.chunks]
        if c.error is not None or c.plan().key() != ((((0, len(clouds)),), ((0, len(clouds)),), (), None)):
            return False       # the sort is modelled for calls that are one group
        return not order_keeps_chunks(group_order(clouds, RADIUS, KEY_BITS + bits_for(len(clouds) - 1)), clouds)
    if variant == "first_trip_only":
        if c.plan(first_trip_only=True).key() != c.plan().key():
            return True
        xyz, off = np.concatenate([ch.points for ch in c.chunks]), c.offsets
        a = group_boxes(xyz, off, 0, len(c.chunks))
        b = group_boxes(xyz, off, 0, len(c.chunks), first_trip_only=True)
        return not all(np.array_equal(x, y) for x, y in zip(a[1:], b[1:]))     # another box: another grid
    kw = {"split_ge": dict(split_ge=True), "mid_up": dict(mid_up=True), "no_chunk_cap": dict(chunk_cap=None)}[variant]
    return c.plan(**kw).key() != c.plan().key()
