"""NumPy restatement of ai_ground_planes (rules G1-G7 of include/autoinst_hip.h) and the cases the CPU and
GPU suites share.  G2 is uint64 array arithmetic (which wraps modulo 2^64) in the vectorised form and Python integers in the plain
loop; G3 and G4 are float64 array operations, one ufunc per step, so nothing is fused; G1 is aggregate_ref.keep_mask."""
import numpy as np

import aggregate_ref

SLAB = 1024                # GR_SLAB of csrc/ai_ground.hip: the input points of one scoring block
HYPS = 256                 # GR_HYPS: the hypotheses of one scoring block
MAX_HYP = 4096
MASK = (1 << 64) - 1
GOLDEN, MIX1, MIX2 = 0x9E3779B97F4A7C15, 0xBF58476D1CE4E5B9, 0x94D049BB133111EB


# ----------------------------------------------------------------------------- G2

def mix(seed, c):
    """The generator's word for counter c, in Python integers."""
    z = (seed + (c + 1) * GOLDEN) & MASK
    z ^= z >> 30
    z = (z * MIX1) & MASK
    z ^= z >> 27
    z = (z * MIX2) & MASK
    z ^= z >> 31
    return z


def ranks(seed, key, h, m):
    """The three ranks of hypothesis h of the scan with key `key` among m >= 3 kept points, in Python integers."""
    c = ((key * MAX_HYP + h) * 4) & MASK

    def draw(j, n):
        return ((mix(seed & MASK, (c + j) & MASK) >> 32) * n) >> 32
    r0 = draw(0, m)
    r1 = draw(1, m - 1)
    if r1 >= r0:
        r1 += 1
    r2 = draw(2, m - 2)
    for r in sorted((r0, r1)):
        if r2 >= r:
            r2 += 1
    return r0, r1, r2


def ranks_all(seed, key, n_hyp, m):
    """(n_hyp, 3) int64: `ranks` for every hypothesis, in uint64 array arithmetic."""
    u = np.uint64
    with np.errstate(over="ignore"):
        c = (u(key & MASK) * u(MAX_HYP) + np.arange(n_hyp, dtype=np.uint64)) * u(4)

        def draw(j, n):
            z = u(seed & MASK) + (c + u(j) + u(1)) * u(GOLDEN)
            z = z ^ (z >> u(30))
            z = z * u(MIX1)
            z = z ^ (z >> u(27))
            z = z * u(MIX2)
            z = z ^ (z >> u(31))
            return ((z >> u(32)) * u(n)) >> u(32)
        r0 = draw(0, m)
        r1 = draw(1, m - 1)
        r1 = r1 + (r1 >= r0).astype(np.uint64)
        r2 = draw(2, m - 2)
        lo, hi = np.minimum(r0, r1), np.maximum(r0, r1)
        r2 = r2 + (r2 >= lo).astype(np.uint64)
        r2 = r2 + (r2 >= hi).astype(np.uint64)
    return np.stack([r0, r1, r2], 1).astype(np.int64)


# ----------------------------------------------------------------------------- G3, G4

def planes_of(p0, p1, p2):
    """G3 on (k, 3) float64 arrays: ((k, 4) planes with NaN rows for degenerate hypotheses, (k,) bool: not degenerate)."""
    with np.errstate(all="ignore"):
        e0, e1 = p1 - p0, p2 - p0
        nx = (e0[:, 1] * e1[:, 2]) - (e0[:, 2] * e1[:, 1])
        ny = (e0[:, 2] * e1[:, 0]) - (e0[:, 0] * e1[:, 2])
        nz = (e0[:, 0] * e1[:, 1]) - (e0[:, 1] * e1[:, 0])
        length = np.sqrt((nx * nx + ny * ny) + nz * nz)
        ok = (length > 0) & (length < np.inf)
        a, b, c = nx / length, ny / length, nz / length
        d = -((a * p0[:, 0] + b * p0[:, 1]) + c * p0[:, 2])
    out = np.stack([a, b, c, d], 1)
    out[~ok] = np.nan
    return out, ok


def inliers(plane, pts, threshold):
    """G4: (k, n) bool for (k, 4) planes and (n, 3) float64 points."""
    with np.errstate(all="ignore"):
        dist = np.abs(((plane[:, 0:1] * pts[:, 0] + plane[:, 1:2] * pts[:, 1]) + plane[:, 2:3] * pts[:, 2]) + plane[:, 3:4])
        return dist < threshold


def segment_scan(kept, key, n_hyp, threshold, seed):
    """One scan's kept points (m, 3) float32 -> (hyp_count (n_hyp,) int32, best_hyp, best_count, plane (4,), inlier mask (m,))."""
    m = kept.shape[0]
    counts = np.full(n_hyp, -1, dtype=np.int32)
    none = (counts, -1, 0, np.zeros(4), np.zeros(m, dtype=bool))
    if m < 3:
        return none
    pts = kept.astype(np.float64)
    r = ranks_all(seed, key, n_hyp, m)
    planes, ok = planes_of(pts[r[:, 0]], pts[r[:, 1]], pts[r[:, 2]])
    for a in range(0, n_hyp, 512):
        counts[a:a + 512] = inliers(planes[a:a + 512], pts, threshold).sum(1)
    counts[~ok] = -1
    if not ok.any():
        return none
    best = int(np.argmax(counts))                                   # G5: the first of the largest
    return counts, best, int(counts[best]), planes[best], inliers(planes[best:best + 1], pts, threshold)[0]


def segment_scan_loop(kept, key, n_hyp, threshold, seed):
    """`segment_scan` as a plain loop over the hypotheses, one scalar step at a time: (hyp_count, best_hyp, best_count, plane)."""
    f = np.float64
    m = kept.shape[0]
    pts = kept.astype(np.float64)
    counts, best, best_count, best_plane = np.full(n_hyp, -1, dtype=np.int32), -1, 0, np.zeros(4)
    for h in range(n_hyp if m >= 3 else 0):
        (x0, y0, z0), p1, p2 = (pts[r] for r in ranks(seed, key, h, m))
        with np.errstate(all="ignore"):
            ax, ay, az = p1[0] - x0, p1[1] - y0, p1[2] - z0
            bx, by, bz = p2[0] - x0, p2[1] - y0, p2[2] - z0
            nx, ny, nz = f(ay * bz) - f(az * by), f(az * bx) - f(ax * bz), f(ax * by) - f(ay * bx)
            length = np.sqrt(f(f(nx * nx) + f(ny * ny)) + f(nz * nz))
            if not (length > 0 and length < np.inf):
                continue
            a, b, c = nx / length, ny / length, nz / length
            d = -(f(f(a * x0) + f(b * y0)) + f(c * z0))
            n = 0
            for x, y, z in pts:
                n += bool(abs(f(f(f(a * x) + f(b * y)) + f(c * z)) + d) < threshold)
        counts[h] = n
        if best < 0 or n > best_count:
            best, best_count, best_plane = h, n, np.array([a, b, c, d])
    return counts, best, best_count, best_plane


def ground_planes(scans, labels=None, moving_index=None, range_min=None, range_max=None, distance_threshold=0.4, num_iterations=2000,
                  seed=0, scan_base=0):
    """Every output of prep_api.ground_planes(..., return_counts=True) as host arrays: flags (M,) bool, planes, best_hyp,
    best_count, hyp_count."""
    n_scans = len(scans)
    out = {"flags": [], "planes": np.zeros((n_scans, 4)), "best_hyp": np.full(n_scans, -1, np.int32),
           "best_count": np.zeros(n_scans, np.int32), "hyp_count": np.full((n_scans, num_iterations), -1, np.int32)}
    for s, scan in enumerate(scans):
        xyz = np.asarray(scan, dtype=np.float32)[:, :3]
        keep = aggregate_ref.keep_mask(xyz, None if labels is None else labels[s], moving_index, range_min, range_max)   # G1
        counts, best, best_count, plane, inl = segment_scan(xyz[keep], scan_base + s, num_iterations, distance_threshold, seed)
        flags = np.zeros(xyz.shape[0], dtype=bool)
        flags[np.flatnonzero(keep)[inl]] = True
        out["flags"].append(flags)
        out["planes"][s], out["best_hyp"][s], out["best_count"][s], out["hyp_count"][s] = plane, best, best_count, counts
    out["flags"] = np.concatenate(out["flags"]) if scans else np.zeros(0, dtype=bool)
    return out


# ----------------------------------------------------------------------------- inputs

THRESHOLD_F32 = float(np.float32(0.4))     # a threshold that float32 coordinates can hit exactly


def make_scan(rng, n, ground_frac=0.6):
    """n float32 points: a slightly tilted road near z = -1.7 with a few centimetres of noise, and clutter above it; label words."""
    p = np.empty((n, 3), dtype=np.float32)
    p[:, :2] = rng.uniform(-30.0, 30.0, (n, 2))
    road = rng.random(n) < ground_frac
    p[:, 2] = np.where(road, -1.7 + 0.01 * p[:, 0] + 0.03 * rng.standard_normal(n), rng.uniform(-1.5, 6.0, n))
    words = np.where(road, 40, rng.choice(aggregate_ref.SEMANTIC, n)).astype(np.uint32)
    return p, words


def _case(rng, sizes, **kw):
    made = [make_scan(rng, n) for n in sizes]
    c = {"scans": [m[0] for m in made], "labels": None, "moving_index": None, "range_min": None, "range_max": None,
         "distance_threshold": 0.4, "num_iterations": 64, "seed": 0, "scan_base": 0}
    if kw.pop("with_labels", False):
        c["labels"] = [m[1] for m in made]
    c.update(kw)
    return c


def grid_points(n, z, shift=0):
    """n points (i mod 16 + shift, i div 16, z): small integers, so every cross product of them is exact."""
    i = np.arange(n)
    return np.stack([i % 16 + shift, i // 16, np.full(n, z)], 1).astype(np.float32)


def ulp_scan():
    """200 points with z = 0 exactly on an integer grid, and in the middle of them points at the threshold THRESHOLD_F32, one
    float32 below it and one above it, on both sides of the plane.  A hypothesis of three grid points has the normal (0, 0, +-1)
    exactly and dist = |z|."""
    f = np.float32
    t = f(THRESHOLD_F32)
    zs = [t, np.nextafter(t, f(0)), np.nextafter(t, f(1)), -t, -np.nextafter(t, f(0)), -np.nextafter(t, f(1))]
    extra = np.array([[7.5 + 0.25 * k, 6.5, z] for k, z in enumerate(zs)], dtype=np.float32)
    return np.concatenate([grid_points(100, 0.0), extra, grid_points(100, 0.0) + np.array([0, 7, 0], dtype=np.float32)])


ULP_ROWS = slice(100, 106)                      # the rows of ulp_scan's six off-plane points
ULP_FLAGS = [False, True, False, False, True, False]


def cases():
    """name -> keyword arguments of `ground_planes` (and of prep_api.ground_planes)."""
    rng = np.random.default_rng(18)
    out = {}
    out["tiny_scans_0_to_4"] = _case(rng, [0, 1, 2, 3, 4])
    out["slab_minus_1_one_hypothesis"] = _case(rng, [SLAB - 1], num_iterations=1)
    out["slab_255_hypotheses"] = _case(rng, [SLAB], num_iterations=HYPS - 1)
    out["slab_plus_1_256_hypotheses"] = _case(rng, [SLAB + 1], num_iterations=HYPS)
    out["two_slabs_plus_1_257_hypotheses"] = _case(rng, [2 * SLAB + 1], num_iterations=HYPS + 1)
    out["all_4096_hypotheses"] = _case(rng, [600, 5], num_iterations=MAX_HYP, seed=7)
    out["boundaries_disagree"] = _case(rng, [700, SLAB, 1500, 3, 0, 900], seed=0)
    out["empty_first_and_last"] = _case(rng, [0, 300, 0, 1100, 0])
    out["only_empty_scans"] = _case(rng, [0, 0])
    out["no_scans"] = _case(rng, [])
    out["other_seed_and_base"] = _case(rng, [700, 900], seed=(1 << 64) - 3, scan_base=(1 << 48) - 2)
    i = np.arange(300)
    line = np.stack([i, 2 * i, 3 * i], 1).astype(np.float32)
    out["collinear"] = dict(_case(rng, [400]), scans=[line, make_scan(rng, 400)[0]])
    dup = make_scan(rng, 40)[0]
    dup[5:35] = dup[5]
    out["duplicates"] = dict(_case(rng, []), scans=[dup])
    both = np.concatenate([grid_points(160, 0.0), grid_points(160, 10.0)])
    out["parallel_planes"] = dict(_case(rng, []), scans=[both[rng.permutation(320)], both])
    out["threshold_ulps"] = dict(_case(rng, []), scans=[ulp_scan()], distance_threshold=THRESHOLD_F32)
    bad = make_scan(rng, 500)[0]
    bad[::7, 0] = np.nan
    bad[3::11, 2] = np.inf
    bad[5::13, 1] = -np.inf
    out["nan_and_inf"] = dict(_case(rng, []), scans=[bad, make_scan(rng, 300)[0]])
    out["moving_filter"] = _case(rng, [1300, 900], with_labels=True, moving_index=251)
    out["range_filter"] = _case(rng, [1300, 900], range_min=3.0, range_max=25.0)
    out["both_filters"] = _case(rng, [1300, 2, 900], with_labels=True, moving_index=251, range_min=3.0, range_max=25.0)
    out["range_min_only"] = _case(rng, [1300], range_min=20.0)
    out["all_filtered"] = _case(rng, [500, 300], with_labels=True, moving_index=0)
    u = aggregate_ref.ulp_points()
    out["range_ulps"] = dict(_case(rng, []), scans=[np.concatenate([u, make_scan(rng, 200)[0]]), u[::-1].copy()], range_min=3.0,
                             range_max=25.0)
    return out
