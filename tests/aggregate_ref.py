"""NumPy restatement of ai_aggregate_scans (rules A1-A6 of include/autoinst_hip.h) and the cases the CPU
and GPU suites share.  float32 steps are explicit np.float32 array operations; the transform is camera_api.transform_points."""
import numpy as np

from autoinst_amd import camera_api

CLOUDS = ("ground", "nonground")
KINDS = ("seg", "instance", "panoptic")
TILE = 1024                # AG_TILE of csrc/ai_aggregate.hip: the points of one block
SCAN_TILE = 2048           # csrc/ai_scan.hip: the elements one block of the shared scan handles
SCAN_MAX_DIRECT_TILES = 4096


def decode_labels(words):
    """A6: (seg, instance, panoptic) of raw label words, all uint32; the instance product wraps modulo 2^32."""
    w = np.asarray(words, dtype=np.uint32)
    hi, lo = w & np.uint32(0xFFFF0000), w & np.uint32(0xFFFF)
    return lo, hi * (w & np.uint32(0x10009)), np.where(hi != 0, hi, lo)


def range_norm(xyz):
    """A2: the float32 norm, s = (x*x + y*y) + z*z with every step rounded to float32, then the float32 square root."""
    p = np.asarray(xyz, dtype=np.float32).reshape(-1, 3)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    s = (x * x + y * y) + z * z
    assert s.dtype == np.float32
    return np.sqrt(s)


def keep_mask(xyz, words=None, moving_index=None, range_min=None, range_max=None):
    """A1 and A2 on (M, 3) float32 points: True where a point is kept."""
    keep = np.ones(np.asarray(xyz).reshape(-1, 3).shape[0], dtype=bool)
    if moving_index is not None:
        keep &= (np.asarray(words, dtype=np.uint32) & np.uint32(0xFFFF)) < np.uint32(moving_index)
    if range_min is not None or range_max is not None:
        r = range_norm(xyz)
        lo = np.float32(0.0 if range_min is None else range_min)
        hi = np.float32(np.inf if range_max is None else range_max)
        keep &= (r >= lo) & (r <= hi)
    return keep


def aggregate(scans, poses, labels=None, ground=None, moving_index=None, range_min=None, range_max=None):
    """Every output of prep_api.aggregate_scans(..., return_source=True) as host arrays: xyz_*, seg_*, instance_*, panoptic_*
    (when labels are given), source_*, offsets_* for ground and nonground.  `ground`: per-scan boolean masks."""
    off = np.zeros(len(scans) + 1, dtype=np.int64)
    np.cumsum([s.shape[0] for s in scans], out=off[1:])
    xyz = np.concatenate([np.asarray(s, dtype=np.float32)[:, :3] for s in scans]) if scans else np.zeros((0, 3), np.float32)
    words = None if labels is None else (np.concatenate([np.asarray(a, dtype=np.uint32).reshape(-1) for a in labels])
                                         if labels else np.zeros(0, np.uint32))
    keep = keep_mask(xyz, words, moving_index, range_min, range_max)
    flag = np.concatenate([np.asarray(g, dtype=bool) for g in ground]) if ground else np.zeros(xyz.shape[0], dtype=bool)
    moved = np.zeros((xyz.shape[0], 3), dtype=np.float64)
    for s in range(len(scans)):                                    # A4, scan by scan (a non-finite point is dropped or is not fed)
        with np.errstate(invalid="ignore"):
                moved[off[s]:off[s + 1]] = camera_api.transform_points(xyz[off[s]:off[s + 1]].astype(np.float64), poses[s])
    out = {}
    for cloud, member in (("ground", keep & flag), ("nonground", keep & ~flag)):
        src = np.flatnonzero(member)                               # A5: ascending input position
        out[f"xyz_{cloud}"] = moved[src]
        out[f"source_{cloud}"] = src.astype(np.int64)
        out[f"offsets_{cloud}"] = np.concatenate([[0], np.cumsum(member)])[off].astype(np.int64)
        if words is not None:
            for kind, a in zip(KINDS, decode_labels(words[src])):
                out[f"{kind}_{cloud}"] = a
    return out


# ----------------------------------------------------------------------------- inputs

SEMANTIC = np.array([0, 1, 10, 40, 48, 70, 250, 251, 252, 259], dtype=np.uint32)


def rotation(axis, angle):
    a = np.asarray(axis, dtype=np.float64)
    a = a / np.linalg.norm(a)
    k = np.array([[0, -a[2], a[1]], [a[2], 0, -a[0]], [-a[1], a[0], 0]])
    return np.eye(3) + np.sin(angle) * k + (1.0 - np.cos(angle)) * (k @ k)


def pose(kind, seed=0):
    T = np.eye(4)
    if kind == "translation":     # values with long mantissas
        T[:3, 3] = [1.0 / 3.0, -2.0 / 7.0, 1000.0 + 1.0 / 9.0]
    elif kind == "rotation":
        rng = np.random.default_rng(seed)
        T[:3, :3] = rotation(rng.normal(size=3), 0.7 + 0.1 * seed)
        T[:3, 3] = rng.normal(size=3) * 50.0
    else:
        assert kind == "identity"
    return T


def make_scan(rng, n):
    """n float32 points of a sensor frame, their label words and a ground mask (an irregular pattern)."""
    p = np.empty((n, 3), dtype=np.float32)
    p[:, :2] = rng.uniform(-40.0, 40.0, (n, 2))
    p[:, 2] = rng.uniform(-3.0, 5.0, n)
    inst = rng.integers(0, 1 << 16, n, dtype=np.uint32)
    inst[rng.random(n) < 0.3] = 0                                  # instance part zero
    words = (inst << np.uint32(16)) | rng.choice(SEMANTIC, n)
    words[rng.random(n) < 0.01] = np.uint32(0xFFFFFFFF)
    return p, words.astype(np.uint32), rng.random(n) < 0.4


def special_words():
    """Instance part zero; semantic part 250, 251, 252; 0xFFFFFFFF; words whose instance product wraps (and one that does not)."""
    w = [0, 40, 250, 251, 252, 0xFFFFFFFF, 0x0001000A, 0x00010001, (0xFFFF << 16) | 9, 0x80000009,
         (1234 << 16) | 250, (1234 << 16) | 251, (1234 << 16) | 252, (77 << 16) | 0xFFFF, 1 << 31, (3 << 16) | 8, (3 << 16) | 1]
    return np.array(w, dtype=np.uint32)


def ulp_points():
    """Points whose float32 r equals 3 and 25 exactly, and their one-ulp neighbours on both sides; the neighbours of (15, 20, 0)
    within three ulps per axis (some have a float32 r of exactly 25 and a true norm that is not 25)."""
    f = np.float32
    pts = [(3, 0, 0), (np.nextafter(f(3), f(0)), 0, 0), (np.nextafter(f(3), f(9)), 0, 0), (0, 0, -3), (0, np.nextafter(f(3), f(9)), 0),
           (15, 20, 0), (25, 0, 0), (np.nextafter(f(25), f(0)), 0, 0), (np.nextafter(f(25), f(99)), 0, 0), (0, 7, 24), (0, 0, 0)]
    for i in range(-3, 4):
        for j in range(-3, 4):
            x, y = f(15), f(20)
            for _ in range(abs(i)):
                x = np.nextafter(x, f(15 + i))
            for _ in range(abs(j)):
                y = np.nextafter(y, f(20 + j))
            pts.append((x, y, 0))
    return np.array(pts, dtype=np.float32)


def _case(rng, sizes, poses=None, **kw):
    made = [make_scan(rng, n) for n in sizes]
    c = {"scans": [m[0] for m in made], "labels": [m[1] for m in made], "ground": [m[2] for m in made],
         "poses": np.array([pose("rotation", k) for k in range(len(sizes))] if poses is None else poses).reshape(-1, 4, 4),
         "moving_index": 251, "range_min": 3.0, "range_max": 25.0}
    c.update(kw)
    return c


def cases():
    """name -> keyword arguments of `aggregate` (and, with per-scan masks as `ground`, of prep_api.aggregate_scans)."""
    rng = np.random.default_rng(20)
    out = {}
    for n in (1, 255, 256, 257, 1023, 1024, 1025, 2047, 2048, 2049):       # one scan around the wave pass, the tile and two tiles
        out[f"one_scan_{n}"] = _case(rng, [n])
    out["three_scans_2047_2048_2049"] = _case(rng, [2047, 2048, 2049])     # block and scan boundaries disagree
    out["three_scans_1023_1024_1025"] = _case(rng, [1023, 1024, 1025])
    out["many_small_scans"] = _case(rng, [3, 1, 700, 2, 64, 65, 500, 1, 1])  # several scans inside one tile
    out["empty_first"] = _case(rng, [0, 300, 1100])
    out["empty_middle"] = _case(rng, [300, 0, 0, 1100])
    out["empty_last"] = _case(rng, [1100, 300, 0])
    out["only_empty_scans"] = _case(rng, [0, 0])
    out["no_scans"] = _case(rng, [])
    c = _case(rng, [1500, 700])
    c["ground"] = [np.ones(1500, bool), np.ones(700, bool)]
    out["all_ground"] = c
    c = _case(rng, [1500, 700])
    c["ground"] = [np.zeros(1500, bool), np.zeros(700, bool)]
    out["all_nonground"] = c
    out["ground_none"] = _case(rng, [1500, 700], ground=None)
    out["all_dropped"] = _case(rng, [1500, 700], moving_index=0)
    c = _case(rng, [2100, 900], moving_index=None, range_min=None, range_max=None)
    c["ground"] = [np.arange(n) % 2 == 0 for n in (2100, 900)]
    out["alternate_per_point"] = c
    c = _case(rng, [2100, 900], moving_index=None, range_min=None, range_max=None)
    c["ground"] = [(np.arange(n) // 64) % 2 == 1 for n in (2100, 900)]
    out["alternate_per_64"] = c
    u = ulp_points()
    out["range_ulps"] = {"scans": [u, u[::-1].copy()], "labels": None, "ground": [np.arange(u.shape[0]) % 3 == 0] * 2,
                         "poses": np.stack([pose("identity"), pose("translation")]), "moving_index": None, "range_min": 3.0,
                         "range_max": 25.0}
    nan = np.array([[np.nan, 0, 0], [4, np.nan, 0], [0, 4, np.nan], [4, 0, 0], [np.inf, 0, 0], [0, -np.inf, 1]], dtype=np.float32)
    out["nan_is_dropped"] = {"scans": [nan], "labels": None, "ground": None, "poses": np.stack([pose("identity")]),
                             "moving_index": None, "range_min": 0.0, "range_max": 1e30}
    w = special_words()
    pw = np.zeros((w.shape[0], 3), dtype=np.float32)
    pw[:, 0] = 5.0
    out["special_words"] = {"scans": [pw], "labels": [w], "ground": [np.arange(w.shape[0]) % 2 == 1],
                            "poses": np.stack([pose("rotation", 3)]), "moving_index": 251, "range_min": None, "range_max": None}
    out["special_words_unfiltered"] = dict(out["special_words"], moving_index=None)
    out["moving_filter_off"] = _case(rng, [1300, 900], moving_index=None)
    out["range_filter_off"] = _case(rng, [1300, 900], range_min=None, range_max=None)
    out["both_filters_off"] = _case(rng, [1300, 900], moving_index=None, range_min=None, range_max=None)
    out["no_labels"] = _case(rng, [1300, 900], labels=None, moving_index=None)
    out["range_min_only"] = _case(rng, [1300], range_max=None)
    out["range_max_only"] = _case(rng, [1300], range_min=None)
    for kind in ("identity", "translation", "rotation"):
        out[f"pose_{kind}"] = _case(rng, [1300, 900], poses=[pose(kind, 1), pose(kind, 2)])
    return out


# The shared scan works on the tile counts, one element per 1024-point tile.  Its recursive path starts above
# SCAN_MAX_DIRECT_TILES * SCAN_TILE = 8 388 608 tile counts, i.e. above 2^33 points: out of reach, M < 2^31 - 256.  What a call can
# reach is the step from one scan block to two, above SCAN_TILE = 2048 tile counts, i.e. above 2 097 152 points: from there on
# k_scan_add_direct adds a non-zero sum of earlier blocks' totals.
BIG_POINTS = SCAN_TILE * TILE + TILE + 1    # 2 098 177 points, 2050 tile counts


def big_case():
    """Three scans of BIG_POINTS points in all; filters on, irregular ground pattern."""
    rng = np.random.default_rng(21)
    sizes = [BIG_POINTS // 2, 0, BIG_POINTS - BIG_POINTS // 2]
    return _case(rng, sizes)
