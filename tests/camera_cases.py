"""Fixtures, a host model and the brute-force truth for the camera projection (``autoinst_amd/csrc/ai_camera.hip``, DESIGN.md
section 12) at its kernel limits.

Plain NumPy, seeded, no GPU and no library: tests/test_camera_cases.py proves on the CPU that every fixture sits in the regime
its name claims, that the model of the device's search equals the truth on all of them, and that a list of deliberately wrong
searches is rejected; tests/test_gpu_camera_cases.py compares the device's answers with the same truth, bit for bit.

The limits are READ from the sources (`constants`): a changed constant moves the fixtures with it.

* `sigma_min_bound` restates the host's lower bound of the smallest singular value, `search_radius` the pcd-frame radius;
* `visible_model` restates `kc_view_bits` / `kc_visible`: the grid of `build_cells` (`points_cases.grid_of` / `cells_of`), the
  clamped +-1 ring walked in the device's order, 16 points of a cell per step, the pcd-frame prefilter, rule 2 per view, the OR
  and the early exit of the group -- or one of `VARIANTS`, each a search that is wrong in one place;
* the truth is brute force: rule 2 (`camera_ref.transform`, `camera_ref.rule_dist`) over ALL pairs of a view, no tree and no
  grid (`seen_brute`), and the projection, labels, cells and means of `camera_ref.camera_features` on top of it.
"""
from __future__ import annotations

import functools
import math
import re
from dataclasses import dataclass, field

import numpy as np

import camera_ref
import edge_geometry as eg
import points_cases as pc

MAXD = camera_ref.MAX_DIST


# ------------------------------------------------------------------------------------------------- constants from the sources
def constants():
    """The limits of ``ai_camera.hip`` (and, through `points_cases`, of `build_cells`), parsed out of the sources."""
    cam = pc._read(pc._CSRC, "ai_camera.hip")
    f = pc._find
    lanes = int(f(cam, r"for \(int32_t base = s; base < e; base \+= (\d+)\)", "the points per step of kc_visible"))
    if not re.search(r"gid >> 4;", cam) or not re.search(r"gid & 15\)", cam) or not re.search(r"grid_for\(nq \* 16\)", cam) or lanes != 16:
        raise RuntimeError("kc_visible no longer gives 16 lanes to a query")
    wave = int(f(cam, r"const int c = c0 \+ lane \+ (\d+) \* k;", "the lanes of a kc_project wave"))
    narrow_k = int(f(cam, r"if \(P\.fdim <= \d+\)\s*hipLaunchKernelGGL\(kc_project<(\d+)>", "the narrow kc_project"))
    wide_k = int(f(cam, r"else\s*hipLaunchKernelGGL\(kc_project<(\d+)>", "the wide kc_project"))
    c = dict(MAX_VIEWS=int(f(cam, r"^\s*#define\s+AI_CAM_MAX_VIEWS\s+(\d+)", "AI_CAM_MAX_VIEWS")), LANES=lanes, WAVE=wave,
             AI_BLOCK=pc.K["AI_BLOCK"], NARROW=int(f(cam, r"if \(P\.fdim <= (\d+)\)", "the width limit of the narrow kc_project")),
             WIDE=wave * wide_k, CELL_CAP=pc.K["CELL_CAP"], GROW=pc.K["GROW"],
             SINGULAR=float(f(cam, r"if \(!\(s > ([0-9.e-]+)\)\)", "the singularity limit")),
             SLACK_REL=float(f(cam, r"radius = radius \* \(1\.0 \+ ([0-9.e-]+)\) \+ [0-9.e-]+;", "the relative radius slack")),
             SLACK_ABS=float(f(cam, r"radius = radius \* \(1\.0 \+ [0-9.e-]+\) \+ ([0-9.e-]+);", "the absolute radius slack")))
    if c["NARROW"] != wave * narrow_k:
        raise RuntimeError("the narrow kc_project no longer serves 64 lanes x K columns")
    if not re.search(r"n_views == 64 \? ~0ull", cam) or c["MAX_VIEWS"] != wave:
        raise RuntimeError("one lane per view and the V == 64 case of all_views are gone")
    return c


K = constants()
MAX_VIEWS = K["MAX_VIEWS"]
LANES = K["LANES"]
QUERIES_PER_BLOCK = K["AI_BLOCK"] // LANES          # kc_visible
WAVES_PER_BLOCK = K["AI_BLOCK"] // K["WAVE"]        # kc_project: one wave per query
NARROW, WIDE = K["NARROW"], K["WIDE"]
SINGULAR = K["SINGULAR"]


# ------------------------------------------------------------------------------------------------- the host part of the entry
def sigma_min_bound(T):
    """`sigma_min_bound` of ai_camera.hip in its order of operations: the larger of sqrt(1 - ||R^T R - I||_F) and
    |det R| / ||adj R||_F, 0 for a singular R."""
    R = [[float(T[r][c]) for c in range(3)] for r in range(3)]
    e2 = 0.0
    for a in range(3):
        for b in range(3):
            s = 0.0
            for r in range(3):
                s += R[r][a] * R[r][b]
            d = s - (1.0 if a == b else 0.0)
            e2 += d * d
    e = math.sqrt(e2)
    s1 = math.sqrt(1.0 - e) if e < 1.0 else 0.0
    det = (R[0][0] * (R[1][1] * R[2][2] - R[1][2] * R[2][1]) - R[0][1] * (R[1][0] * R[2][2] - R[1][2] * R[2][0]) +
           R[0][2] * (R[1][0] * R[2][1] - R[1][1] * R[2][0]))
    s2 = 0.0
    if det != 0.0 and math.isfinite(det):
        f2 = 0.0
        for r in range(3):
            for c in range(3):
                r1, r2, c1, c2 = (r + 1) % 3, (r + 2) % 3, (c + 1) % 3, (c + 2) % 3
                m = R[r1][c1] * R[r2][c2] - R[r1][c2] * R[r2][c1]
                f2 += m * m
        if f2 > 0.0:
            s2 = abs(det) / math.sqrt(f2)
    return max(s1, s2)


REFUSAL = "is (nearly) singular"        # the entry's message for a view whose bound is not above SINGULAR


def search_radius(case, rule="shipped"):
    """The pcd-frame radius of the entry: max over the views of max_dist / sigma, times 1 + SLACK_REL, plus SLACK_ABS.
    ValueError with the entry's words when a view is refused."""
    radius = 0.0
    for v, T in enumerate(case.T):
        s = sigma_min_bound(T)
        if not s > SINGULAR:
            raise ValueError(f"ai_camera_project: T_pcd2cam of view {v} {REFUSAL}")
        radius = max(radius, case.max_dist if rule == "plain_radius" else case.max_dist / s)
    return radius if rule == "no_slack" else radius * (1.0 + K["SLACK_REL"]) + K["SLACK_ABS"]


# ------------------------------------------------------------------------------------------------- kc_view_bits + kc_visible
VARIANTS = ("plain_radius", "no_slack", "squared", "le", "no_clamp", "mask32", "all_views_zero", "early_exit_any", "first16")
"""Searches that are wrong in one place:
plain_radius    the pcd-frame radius is max_dist, not max_dist / sigma;
no_slack        the radius without its (1 + 1e-6), + 1e-9 slack;
squared         the squared camera-frame distance compared with max_dist * max_dist, not its root with max_dist;
le              ``<=`` for ``<`` in rule 2;
no_clamp        a query outside the cloud's bounds has no cell (the ring is not clamped to the edge cell);
mask32          ``1u << lo`` in kc_view_bits: the shift takes the count modulo 32, so view v >= 32 sets bit v - 32;
all_views_zero  ``(1ull << V) - 1`` for V = 64 taken as the hardware shifts it (a count of 64 is a count of 0): all_views = 0;
early_exit_any  the group leaves the walk as soon as any view is found;
first16         only the first 16 points of a cell are taken."""


def _cam(case, v, pts):
    return camera_ref.transform(pts, case.T[v])


def _pair_matrix(a, b):
    """Rule 2's squared distance and its root for every (a, b) pair, in rule_dist's order."""
    d = a[:, None, :] - b[None, :, :]
    s = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return s, np.sqrt(s)


def visible_model(case, rule="shipped"):
    """The device's search on the CPU: seen (nq, V) bool.  Not rule 2 over all pairs (that is `seen_brute`), but what `kc_visible`
    does: bits per cloud point, the cell list, the ring in walk order, steps of 16, prefilter, rule 2, OR, early exit."""
    assert rule == "shipped" or rule in VARIANTS, rule
    q, c, V = case.points, case.cloud, case.n_views
    nq, nc = q.shape[0], c.shape[0]
    seen = np.zeros((nq, V), dtype=bool)
    radius = search_radius(case, rule)
    if nq == 0 or nc == 0 or V == 0 or sum(len(ix) for ix in case.vis) == 0:
        return seen
    g = pc.grid_of(c, radius)
    n = [int(t) for t in g.n[0]]
    sc = pc.cells_of(g, c[None])[0]
    key = (sc[:, 2] * n[1] + sc[:, 1]) * n[0] + sc[:, 0]
    cells = {}
    for p in np.argsort(key, kind="stable").tolist():       # the stable radix sort: ascending index inside a cell
        cells.setdefault(int(key[p]), []).append(p)
    bits = [0] * nc
    for v, ix in enumerate(case.vis):
        b = v & 31 if rule == "mask32" else v
        for p in np.asarray(ix).tolist():
            bits[p] |= 1 << b
    all_views = 0 if (rule == "all_views_zero" and V == 64) else (1 << V) - 1
    pre = (eg.sq_plain(q[:, None, :], c[None, :, :]) <= radius * radius).tolist()
    near = np.zeros((nq, nc), dtype=np.uint64)
    for v in range(V):                                       # bit v: the pair passes rule 2 under view v's transform
        s, d = _pair_matrix(_cam(case, v, q), _cam(case, v, c))
        ok = s < case.max_dist * case.max_dist if rule == "squared" else d <= case.max_dist if rule == "le" else d < case.max_dist
        near |= ok.astype(np.uint64) << np.uint64(v)
    near = near.tolist()
    qc = pc.cells_of(g, q[None])[0]
    inside = (pc.cells_of(g, q[None], clamp=False)[0] == qc).all(axis=1)
    for i in range(nq):
        found = 0
        done = rule == "no_clamp" and not inside[i]
        cx, cy, cz = (int(t) for t in qc[i])
        for dz in (-1, 0, 1):
            for dy in (-1, 0, 1):
                for dx in (-1, 0, 1):
                    xx, yy, zz = cx + dx, cy + dy, cz + dz
                    if done or not (0 <= xx < n[0] and 0 <= yy < n[1] and 0 <= zz < n[2]):
                        continue
                    run = cells.get((zz * n[1] + yy) * n[0] + xx, ())
                    for base in range(0, len(run), LANES):
                        if rule == "first16" and base:
                            break
                        new = 0
                        for p in run[base:base + LANES]:     # every lane masks with the group's `found` of the step before
                            m = bits[p] & ~found
                            if m and pre[i][p]:
                                new |= m & near[i][p]
                        found |= new
                        if found == all_views or (rule == "early_exit_any" and found):
                            done = True
                            break
        for v in range(V):
            seen[i, v] = bool((found >> v) & 1)
    return seen


# ------------------------------------------------------------------------------------------------- the truth
def _seen_all_pairs(q_cam, p_cam, max_dist):
    """Rule 2 over every pair, query by query, with `camera_ref.rule_dist`: no tree, no grid."""
    out = np.zeros(q_cam.shape[0], dtype=bool)
    if p_cam.shape[0]:
        for i in range(q_cam.shape[0]):
            out[i] = bool((camera_ref.rule_dist(np.repeat(q_cam[i:i + 1], p_cam.shape[0], 0), p_cam) < max_dist).any())
    return out


def seen_brute(case):
    """(nq, V) bool: rule 2 per view over all pairs in the camera frame."""
    out = np.zeros((case.points.shape[0], case.n_views), dtype=bool)
    for v in range(case.n_views):
        out[:, v] = _seen_all_pairs(_cam(case, v, case.points), _cam(case, v, case.cloud[case.vis[v]]), case.max_dist)
    return out


@dataclass
class CamCase:
    name: str
    points: np.ndarray
    cloud: np.ndarray
    vis: list
    T: np.ndarray                      # (V, 4, 4)
    K: np.ndarray
    image_hw: tuple
    feature_maps: np.ndarray = None
    sam_images: np.ndarray = None
    max_dist: float = MAXD
    refused: bool = False              # the entry refuses the call (REFUSAL)
    claims: dict = field(default_factory=dict)

    @property
    def n_views(self):
        return len(self.vis)

    def args(self):
        return (self.points, self.cloud, self.vis, self.T, self.K, self.image_hw)

    @functools.cached_property
    def truth(self):
        """`camera_ref.camera_features` with rule 2 over all pairs in place of its tree: pixels, sam, dino, dino_views."""
        return camera_ref.camera_features(*self.args(), feature_maps=self.feature_maps, sam_images=self.sam_images, max_dist=self.max_dist,
                                          check_mean_rows=min(self.points.shape[0], 64), seen_fn=_seen_all_pairs)


# ------------------------------------------------------------------------------------------------- building blocks
def rot(yaw, pitch=0.0, roll=0.0):
    cy, sy, cp, sp, cr, sr = np.cos(yaw), np.sin(yaw), np.cos(pitch), np.sin(pitch), np.cos(roll), np.sin(roll)
    return (np.array([[cy, -sy, 0], [sy, cy, 0], [0, 0, 1.0]]) @ np.array([[cp, 0, sp], [0, 1.0, 0], [-sp, 0, cp]]) @
            np.array([[1.0, 0, 0], [0, cr, -sr], [0, sr, cr]]))


def view_of(A, centre, half_extent):
    """A 4x4 with linear part A that puts the pcd-frame ball (centre, half_extent) in front of the camera, inside |x/z|, |y/z| <=
    1/4: the camera looks along +z from 4 (camera-frame) half extents away."""
    A = np.asarray(A, dtype=np.float64)
    T = np.eye(4)
    T[:3, :3] = A
    reach = float(np.linalg.norm(A, 2)) * half_extent
    T[:3, 3] = -A @ np.asarray(centre, dtype=np.float64) + [0.0, 0.0, 4.0 * reach + 1.0]
    return T


def intrinsics(h, w):
    """Focal length min(h, w) / 2 * 4 / 2: |x/z| <= 1/4 lands within the middle half of the image on both axes."""
    f = float(min(h, w))
    return np.array([[f, 0.0, w / 2.0], [0.0, f, h / 2.0], [0.0, 0.0, 1.0]])


def maps_for(rng, V, h, w, fh=3, fw=4, F=8):
    sam = rng.integers(0, 4, (V, h, w)).astype(np.int32)
    feat = rng.standard_normal((V, fh, fw, F)).astype(np.float32)
    feat[:, 0, 0] = 0.0
    return feat, sam


def _simple(name, rng, q, cloud, vis, T, hw=(24, 32), claims=None, **kw):
    V = len(vis)
    feat, sam = maps_for(rng, V, *hw)
    return CamCase(name, np.ascontiguousarray(q, dtype=np.float64), np.ascontiguousarray(cloud, dtype=np.float64),
                   [np.asarray(v, dtype=np.int64) for v in vis], np.asarray(T, dtype=np.float64).reshape(V, 4, 4), intrinsics(*hw), hw,
                   feat if V else None, sam if V else None, claims=claims or {}, **kw)


# ------------------------------------------------------------------------------------------------- views_N
VIEW_COUNTS = (1, MAX_VIEWS // 2 - 1, MAX_VIEWS // 2, MAX_VIEWS // 2 + 1, MAX_VIEWS - 1, MAX_VIEWS)


@functools.lru_cache(maxsize=None)
def views_case(V, empty=False):
    """40 queries 1 m apart on a plane, each with its own cloud points a few centimetres away; every view has its own rotation,
    its own image and its own visible set.  Queries 0-3 are seen by the last view alone, 4-7 by the first alone, 8-11 by every
    view, 12-15 by none (a point in no set, or a point of the first view's set 0.3 m away); 16-19 have a point of the first
    view's set 0.29 m away in the cell the walk visits first and their only finder (of a middle view) in a later cell; 20-39
    have one to three points in random sets.  ``empty``: the first, a middle and the last view have empty visible sets (V = 1: the
    only one), and "first" / "last" are the views next to them."""
    rng = np.random.default_rng([51, V, int(empty)])
    hollow = sorted({0, V // 2, V - 1}) if empty else []
    live = [v for v in range(V) if v not in hollow]
    first, last, mid = (live[0], live[-1], live[len(live) // 2]) if live else (None, None, None)
    ij = np.stack(np.meshgrid(np.arange(8), np.arange(5), indexing="ij"), -1).reshape(-1, 2)
    q = np.concatenate([ij * 1.0, np.zeros((40, 1))], 1) + rng.uniform(-0.05, 0.05, (40, 3))
    cloud, sets, kind = [], [[] for _ in range(V)], {}

    def add(p, views):
        for v in views:
            sets[v].append(len(cloud))
        cloud.append(p)
    near = lambda i: q[i] + rng.uniform(0.02, 0.05, 3) * rng.choice([-1.0, 1.0], 3)
    for i in range(40):
        if not live:
            add(near(i), [])
        elif i < 4:
            add(near(i), [last])
        elif i < 8:
            add(near(i), [first])
        elif i < 12:
            add(near(i), live)
        elif i < 14:
            add(near(i), [])
        elif i < 16:
            add(q[i] + [0.3, 0.0, 0.0], [first])
        elif i < 20:
            add(q[i] - 0.17, [first])
            add(q[i] + [0.05, 0.04, 0.03], [mid])
        else:
            for _ in range(int(rng.integers(1, 4))):
                add(near(i), [v for v in live if rng.random() < 0.3])
    cloud = np.array(cloud)
    centre = np.array([3.5, 2.0, 0.0])
    T = [view_of(rot(0.04 * v, 0.01 * (v % 7), -0.005 * (v % 5)), centre + [0.02 * v, 0.0, 0.0], 5.0) for v in range(V)]
    return _simple(f"views_{V}" + ("_empty" if empty else ""), rng, q, cloud, sets, T,
                   claims=dict(first=first, last=last, mid=mid, hollow=hollow, live=live))


# ------------------------------------------------------------------------------------------------- pairs at the threshold
PAIR_KINDS = ("below", "at", "above", "at_sq_below")


def threshold_pairs(T, nodes, rng, want, max_dist=MAXD, tries=300_000, along=None):
    """Pcd-frame pairs (q, p), q within 1 cm of a node, whose camera-frame rule distance under T is exactly one of
    ``below`` = nextafter(max_dist, 0), ``at`` = max_dist, ``above`` = nextafter(max_dist, inf), or ``at_sq_below`` = max_dist
    while the squared distance is below fl(max_dist * max_dist).  The rounding of the transforms scatters the distance over
    some tens of ulps around the aim, so a seeded random search meets every one of them; ``want`` {kind: count}; one pair per
    node.  ``along``: half of the directions are taken near this one.  Returns {kind: [(q, p, node index), ...]}."""
    A = np.asarray(T)[:3, :3]
    m = int(tries)
    node = rng.integers(0, len(nodes), m)
    q = np.asarray(nodes)[node] + rng.uniform(-0.01, 0.01, (m, 3))
    u = rng.standard_normal((m, 3))
    if along is not None:
        half = rng.random(m) < 0.5
        u = np.where(half[:, None], np.asarray(along)[None] + 0.05 * u, u)
    u /= np.linalg.norm(u, axis=1, keepdims=True)
    t0 = max_dist / np.linalg.norm(u @ A.T, axis=1)
    p = q + u * (t0 * (1.0 + rng.uniform(-1e-14, 1e-14, m)))[:, None]
    dlt = camera_ref.transform(q, T) - camera_ref.transform(p, T)
    s = (dlt[:, 0] * dlt[:, 0] + dlt[:, 1] * dlt[:, 1]) + dlt[:, 2] * dlt[:, 2]
    d = np.sqrt(s)
    is_kind = {"below": d == np.nextafter(max_dist, 0.0), "at": d == max_dist, "above": d == np.nextafter(max_dist, np.inf),
               "at_sq_below": (d == max_dist) & (s < max_dist * max_dist)}
    out, used = {}, set()
    for kind, count in want.items():
        got = []
        for j in np.flatnonzero(is_kind[kind]).tolist():
            if len(got) == count:
                break
            if int(node[j]) not in used:
                used.add(int(node[j]))
                got.append((q[j], p[j], int(node[j])))
        if len(got) < count:
            raise RuntimeError(f"threshold_pairs: only {len(got)} of {count} pairs of kind {kind} found")
        out[kind] = got
    return out


def _lattice(centre, spacing, count):
    side = int(np.ceil(count ** (1 / 3)))
    ijk = np.stack(np.meshgrid(*[np.arange(side)] * 3, indexing="ij"), -1).reshape(-1, 3)[:count]
    return np.asarray(centre) + (ijk - (side - 1) / 2.0) * spacing


AFFINE = {
    "scale_0.5": lambda: 0.5 * rot(0.3, 0.1, -0.2),
    "scale_2": lambda: 2.0 * rot(-0.4, 0.05, 0.3),
    "scale_0.01": lambda: 0.01 * rot(0.7, -0.1, 0.1),
    "anisotropic": lambda: np.diag([1.0, 0.25, 4.0]) @ rot(0.5, 0.2, -0.1),
    "sheared": lambda: np.array([[1.0, 1.5, 0.0], [0.0, 1.0, 0.0], [0.0, 0.0, 1.0]]) @ rot(-0.2, 0.15, 0.25),
    "rotation": lambda: rot(0.9, -0.05, 0.02),
}
AFFINE_CASES = {"scaled": ("scale_0.5", "scale_2", "scale_0.01"), "anisotropic": ("anisotropic", "rotation"),
                "sheared": ("sheared", "rotation"), "mixed_sigma": tuple(AFFINE)}


@functools.lru_cache(maxsize=None)
def affine_case(name):
    """One call whose views have the linear parts ``AFFINE_CASES[name]``.  Per view a lattice of nodes, far enough apart (four
    times max_dist over the view's true smallest singular value) that a node's pair is alone in the view's frame; at the nodes,
    pairs at the threshold (`threshold_pairs`: 3 below, 2 at, 2 above, 1 at with the square below), half of them along the
    direction the view shrinks most.  The view's visible set holds its own pairs' cloud points only.  claims: per pair (query,
    cloud point, view, kind, pcd-frame distance)."""
    which = AFFINE_CASES[name]
    rng = np.random.default_rng([52, sorted(AFFINE_CASES).index(name)])
    want = {"below": 3, "at": 2, "above": 2, "at_sq_below": 1}
    q, cloud, sets, Ts, pairs = [], [], [], [], []
    for v, key in enumerate(which):
        A = AFFINE[key]()
        _, sv, vt = np.linalg.svd(A)
        spacing = 4.0 * MAXD / sv[-1]
        centre = np.array([40.0 * v, -10.0, 5.0])
        nodes = _lattice(centre, spacing, 27)
        T = view_of(A, centre, 2.0 * spacing)
        found = threshold_pairs(T, nodes, rng, want, along=vt[-1])
        ids = []
        for kind, lst in found.items():
            for (a, b, _) in lst:
                pairs.append(dict(query=len(q), point=len(cloud), view=v, kind=kind, pcd_dist=float(np.linalg.norm(a - b))))
                ids.append(len(cloud))
                q.append(a)
                cloud.append(b)
        sets.append(ids)
        Ts.append(T)
    return _simple(name, rng, np.array(q), np.array(cloud), sets, Ts, hw=(48, 64), claims=dict(pairs=pairs, which=which))


@functools.lru_cache(maxsize=None)
def boundary_case():
    """Rigid views, the second 1 234 m in front of its camera (the camera-frame z then carries 2e-13 m of rounding): pairs at
    the threshold as in `affine_case`, and for the far view pairs whose pcd-frame distance is ABOVE max_dist by up to 2e-13 m
    while the rounded camera-frame distance is below it -- inside the entry's slack, outside a radius without it."""
    rng = np.random.default_rng(53)
    want = {"below": 3, "at": 2, "above": 2, "at_sq_below": 2}
    q, cloud, sets, Ts, pairs = [], [], [], [], []
    for v, (A, shift) in enumerate(((rot(0.3, 0.1, -0.2), 0.0), (rot(-0.6, 0.05, 0.1), 1234.5))):
        centre = np.array([10.0 * v, 3.0, -2.0])
        nodes = _lattice(centre, 1.0, 64)
        T = view_of(A, centre, 3.0)
        T[2, 3] += shift                                    # along the optical axis: the pixels stay inside the image
        found = threshold_pairs(T, nodes[:32], rng, want)
        if shift:
            # beyond max_dist in the pcd frame, seen in the camera frame
            m = 200_000
            node = 32 + rng.integers(0, 32, m)
            a = nodes[node] + rng.uniform(-0.01, 0.01, (m, 3))
            u = rng.standard_normal((m, 3))
            u /= np.linalg.norm(u, axis=1, keepdims=True)
            b = a + u * (MAXD * (1.0 + rng.uniform(2e-13, 1e-12, m)))[:, None]
            pcd = np.sqrt(eg.sq_plain(a, b))
            cam = camera_ref.rule_dist(camera_ref.transform(a, T), camera_ref.transform(b, T))
            hit, used, lst = np.flatnonzero((cam < MAXD) & (pcd > MAXD)), set(), []
            for j in hit.tolist():
                if int(node[j]) not in used and len(lst) < 4:
                    used.add(int(node[j]))
                    lst.append((a[j], b[j], int(node[j])))
            if len(lst) < 4:
                raise RuntimeError("boundary_case: no pair beyond max_dist in the pcd frame and below it in the camera frame")
            found["pcd_above"] = lst
        ids = []
        for kind, lst in found.items():
            for (a, b, _) in lst:
                pairs.append(dict(query=len(q), point=len(cloud), view=v, kind=kind, pcd_dist=float(np.sqrt(eg.sq_plain(a, b)))))
                ids.append(len(cloud))
                q.append(a)
                cloud.append(b)
        sets.append(ids)
        Ts.append(T)
    return _simple("boundary", rng, np.array(q), np.array(cloud), sets, Ts, hw=(48, 64), claims=dict(pairs=pairs))


@functools.lru_cache(maxsize=None)
def near_singular_case(side):
    """T = s R with the entry's bound s / sqrt(3) one part in a thousand ``above`` or ``below`` the singularity limit.  Above: the
    call is computed (the radius is 175 km, one cell holds the cloud; every camera-frame distance is micrometres, so every query
    sees every view with a visible point).  Below: refused with `REFUSAL`, the outputs unwritten."""
    rng = np.random.default_rng(54)
    s = SINGULAR * math.sqrt(3.0) * (1.001 if side == "above" else 0.999)
    cloud = rng.uniform(-2.0, 2.0, (60, 3))
    q = np.concatenate([cloud[:10] + 0.05, rng.uniform(-2.0, 2.0, (11, 3))])
    T = [view_of(s * rot(0.2, 0.1, 0.1), np.zeros(3), 4.0), view_of(rot(0.1), np.zeros(3), 4.0)]
    return _simple(f"near_singular_{side}", rng, q, cloud, [np.arange(0, 60, 2), np.arange(20)], T,
                   refused=side == "below", claims=dict(scale=s))


# ------------------------------------------------------------------------------------------------- the 16-lane walk
RUN_LENGTHS = (LANES - 1, LANES, LANES + 1, 2 * LANES, 2 * LANES + 1)


@functools.lru_cache(maxsize=None)
def cell_runs_case():
    """Three views under one rigid transform.  Per run length L (15, 16, 17, 32, 33) a query 2 cm inside the (+, +, +) corner
    of its cell; the neighbouring cell across that corner -- the 27th and last of the walk -- holds exactly L cloud points within
    5 cm of the corner.  The last of them (lane (L - 1) % 16 of the last step) is the only point of view 1's set near the
    query; the others are in view 0's set, as is a point 0.16 m below the query, in the cell under its own: the first occupied
    cell of the walk, so view 0 is found in the first step.  View 2 has a set of its own that no query is near: all_views is never reached early."""
    rng = np.random.default_rng(55)
    A = rot(0.0)
    T = view_of(A, np.array([4.0, 1.0, 1.0]), 6.0)
    probe = _simple("probe", rng, np.zeros((1, 3)), np.zeros((1, 3)), [[0]] * 3, [T] * 3)
    cell = search_radius(probe)
    anchor = np.zeros(3)
    q, cloud, sets, runs = [], [anchor, anchor + [40 * cell, 12 * cell, 12 * cell]], [[], [], [1]], []
    for k, L in enumerate(RUN_LENGTHS):
        home = np.array([5 + 6 * k, 5, 5])
        corner = anchor + (home + 1) * cell
        q.append(corner - 0.02)
        sets[0].append(len(cloud))
        cloud.append(q[-1] - [0.0, 0.0, 0.16])                                     # across the low z face of the query's cell
        members = []
        for j in range(L):
            members.append(len(cloud))
            sets[1 if j == L - 1 else 0].append(len(cloud))
            cloud.append(corner + rng.uniform(0.005, 0.03, 3))
        runs.append(dict(L=L, query=k, home=home.tolist(), members=members))
    return _simple("cell_runs", rng, np.array(q), np.array(cloud), sets, [T] * 3, claims=dict(runs=runs, cell=cell))


QUERY_COUNTS = (1, WAVES_PER_BLOCK - 1, WAVES_PER_BLOCK, WAVES_PER_BLOCK + 1, QUERIES_PER_BLOCK - 1, QUERIES_PER_BLOCK, QUERIES_PER_BLOCK + 1,
                4 * QUERIES_PER_BLOCK + 1)


@functools.lru_cache(maxsize=None)
def query_tail_case(nq):
    """200 cloud points in a 1.5 m cube, three views with random visible sets, ``nq`` queries within 0.1 m of cloud points."""
    rng = np.random.default_rng([56, nq])
    cloud = rng.uniform(0.0, 1.5, (200, 3))
    q = cloud[rng.integers(0, 200, nq)] + rng.uniform(-0.1, 0.1, (nq, 3))
    vis = [np.flatnonzero(rng.random(200) < 0.4) for _ in range(3)]
    T = [view_of(rot(0.2 * v, 0.03 * v, 0.01), np.full(3, 0.75), 1.5) for v in range(3)]
    return _simple(f"query_tail_{nq}", rng, q, cloud, vis, T, claims=dict(nq=nq))


@functools.lru_cache(maxsize=None)
def clamped_case():
    """A 5 x 5 x 5 lattice of cloud points 0.5 m apart (about 12 cells a side), two rigid views that each see every second
    point.  Per face, edge and corner of the box: a query 0.09 m outside it on each of the direction's axes (at most 0.156 m from
    the lattice point there: seen), one 0.2 m outside (not seen), and one 1e6 m outside."""
    rng = np.random.default_rng(57)
    ijk = np.stack(np.meshgrid(*[np.arange(5)] * 3, indexing="ij"), -1).reshape(-1, 3)
    cloud = ijk * 0.5
    d = pc._directions()
    base = np.where(d == 0, 1.0, np.where(d > 0, 2.0, 0.0))
    q = np.concatenate([base + d * 0.09, base + d * 0.2, base + d * 1e6])
    where = ["near"] * len(d) + ["beyond"] * len(d) + ["far"] * len(d)
    vis = [np.arange(0, 125, 2), np.arange(125)]
    T = [view_of(rot(0.1 + 0.2 * v, 0.05, 0.02), np.full(3, 1.0), 2.0) for v in range(2)]
    return _simple("clamped", rng, q, cloud, vis, T, claims=dict(where=where))


@functools.lru_cache(maxsize=None)
def grown_grid_case(side):
    """A sparse cloud whose two corner points span exactly the cell cap (``under``: 2048 x 2048 x 32 cells of the search radius,
    not grown) or one cell more on x (``over``: the cell grows once, by 1.5).  The device's two dense tables are 2 x 4 B x 2^27 =
    1 GB for ``under`` (0.32 GB after the growth).  30 clusters of 40 cloud points; queries within 0.15 m of a cloud point on
    every axis; and, along x, pairs at chosen places in the OLD grid (cell = the radius): the query 1 mm below old border k, a
    point 0.09 m beyond it (seen; one old cell apart: in the grown grid the same cell or the next), and a point 1 mm beyond
    border k + 1 (TWO old cells apart and so, the cell being the radius, 2 mm too far: the grown ring walks it all the same, and
    the search must refuse it).  View 0's set holds both points, view 1's only the second: its answer hangs on the refusal.
    No accepted pair can lie two old cells apart: that is more than one radius."""
    rng = np.random.default_rng([58, side == "over"])
    probe = _simple("probe", rng, np.zeros((1, 3)), np.zeros((1, 3)), [[0]] * 2, [view_of(rot(0.3), np.zeros(3), 1.0)] * 2)
    cell = search_radius(probe)
    ext = pc.under_cap_extent(cell) + ([cell, 0.0, 0.0] if side == "over" else [0.0, 0.0, 0.0])
    o = np.array([-100.0, 50.0, 2.0])
    cloud = pc._clusters(rng, o, o + ext, 30, 40, 0.1)
    q = cloud[rng.integers(2, cloud.shape[0], 120)] + rng.uniform(-0.15, 0.15, (120, 3))
    extra_q, extra_c, placed = [], [], []
    for k in (100, 101, 102, 103, 500, 1001):
        border = o[0] + k * cell
        y, z = o[1] + 0.3 * ext[1] + 3.0 * len(placed), o[2] + 0.5 * ext[2]
        placed.append(dict(query=120 + len(extra_q), seen=cloud.shape[0] + len(extra_c), refused=cloud.shape[0] + len(extra_c) + 1, k=k))
        extra_q.append([border - 0.001, y, z])
        extra_c += [[border + 0.09, y, z], [border + cell + 0.001, y, z]]
    cloud = np.concatenate([cloud, np.array(extra_c)])
    q = np.concatenate([q, np.array(extra_q)])
    n = cloud.shape[0]
    refused = np.array([p["refused"] for p in placed])
    seen = np.array([p["seen"] for p in placed])
    vis = [np.arange(2, n), np.setdiff1d(np.arange(2, n, 1), seen)]
    centre = o + ext / 2.0
    T = [view_of(rot(0.3 + 0.1 * v, 0.02, 0.01), centre, float(np.linalg.norm(ext)) / 2.0) for v in range(2)]
    return _simple(f"grown_grid_{side}", rng, q, cloud, vis, T, hw=(96, 128), claims=dict(cell=cell, placed=placed, refused=refused.tolist()))


# ------------------------------------------------------------------------------------------------- kc_project: widths, cells
WIDTHS = (1, K["WAVE"] - 1, K["WAVE"], K["WAVE"] + 1, NARROW - 1, NARROW, NARROW + 1, WIDE - 1, WIDE, WIDE + 1, 2 * WIDE, 2 * WIDE + 1)
ROW_KINDS = ("first_column", "last_column", "zero", "negative_zero", "nan", "random", "random_and_zero")


@functools.lru_cache(maxsize=None)
def width_case(F):
    """Identity transforms, K = I, z = 1: query j sits on pixel (4 j + 1, 1) of a 4 x 4n image over a 1 x n map, so cell (0, j) is
    its own in each of the three views.  Per query one row kind (`ROW_KINDS`): a row whose only non-zero element is column 0
    (view 0; zero rows in the others), is column F - 1, or is the first column of a later pass (``pass_<c>``: columns 384, 768 of
    the wide kernel); all-zero rows; -0.0 rows; a lone NaN; random rows in all views; random rows in two views and a zero row."""
    rng = np.random.default_rng([59, F])
    kinds = list(ROW_KINDS) + [f"pass_{c}" for c in range(WIDE, F, WIDE) if F > WIDE] + (["pass_and_first"] if F > WIDE else [])
    n = len(kinds)
    maps = np.zeros((3, 1, n, F), np.float32)
    for j, kind in enumerate(kinds):
        if kind == "first_column":
            maps[0, 0, j, 0] = 1.5
        elif kind == "last_column":
            maps[1, 0, j, F - 1] = -2.5
        elif kind == "negative_zero":
            maps[:, 0, j] = -0.0
        elif kind == "nan":
            maps[2, 0, j, F // 2] = np.nan
        elif kind == "random":
            maps[:, 0, j] = rng.standard_normal((3, F))
        elif kind == "random_and_zero":
            maps[0, 0, j] = rng.standard_normal(F)
            maps[2, 0, j] = rng.standard_normal(F)
        elif kind.startswith("pass_") and kind != "pass_and_first":
            maps[1, 0, j, int(kind[5:])] = 3.0
        elif kind == "pass_and_first":                      # view 0: column 0 only; view 2: the last pass's first column only
            maps[0, 0, j, 0] = 1.0
            maps[2, 0, j, (F - 1) // WIDE * WIDE] = 2.0
    h, w = 4, 4 * n
    pts = np.stack([4.0 * np.arange(n) + 1.0, np.ones(n), np.ones(n)], 1)
    sam = rng.integers(0, 4, (3, h, w)).astype(np.int32)
    return CamCase(f"width_{F}", pts, pts.copy(), [np.arange(n)] * 3, np.repeat(np.eye(4)[None], 3, 0), np.eye(3), (h, w), maps, sam,
                   claims=dict(kinds=kinds, F=F))


# fh, fw, rows and columns of pixels per cell.  49 is the smallest patch size for which int(fh / h * v) != v // patch somewhere.
PATCH_SHAPES = ((16, 16, 14, 14), (37, 26, 14, 14), (27, 88, 11, 13), (8, 6, 49, 49))


@functools.lru_cache(maxsize=None)
def patch_case(fh, fw, ph, pw):
    """An image of exactly ph x pw pixels per cell of an fh x fw map (DINOv2: 14 x 14).  fh / h is then the rounded reciprocal
    of ph, and ``fh / h * v`` lands within an ulp of an integer at every patch border.  Point k sits on pixel (k % w, k % h), k <
    max(h, w): every row and every column is met.  Each cell's row holds (row + 1, column + 1)."""
    h, w = fh * ph, fw * pw
    n = max(h, w)
    k = np.arange(n)
    pts = np.stack([k % w, k % h, np.ones(n)], 1).astype(np.float64)
    maps = np.zeros((1, fh, fw, 2), np.float32)
    maps[0, :, :, 0] = np.arange(1, fh + 1)[:, None]
    maps[0, :, :, 1] = np.arange(1, fw + 1)[None, :]
    rows = np.array([int(fh / h * v) for v in range(h)])
    cols = np.array([int(fw / w * u) for u in range(w)])
    return CamCase(f"patch_{fh}x{fw}_{ph}x{pw}", pts, pts.copy(), [k], np.eye(4)[None], np.eye(3), (h, w), maps, None,
                   claims=dict(rows=rows, cols=cols, off_rows=int((rows != np.arange(h) // ph).sum()),
                               off_cols=int((cols != np.arange(w) // pw).sum())))


# ------------------------------------------------------------------------------------------------- every fixture
def cases():
    """name -> builder of every fixture that the entry computes or refuses."""
    out = {}
    for V in VIEW_COUNTS:
        out[f"views_{V}"] = functools.partial(views_case, V)
        out[f"views_{V}_empty"] = functools.partial(views_case, V, True)
    for name in AFFINE_CASES:
        out[name] = functools.partial(affine_case, name)
    out["boundary"] = boundary_case
    out["near_singular_above"] = functools.partial(near_singular_case, "above")
    out["near_singular_below"] = functools.partial(near_singular_case, "below")
    out["cell_runs"] = cell_runs_case
    for nq in QUERY_COUNTS:
        out[f"query_tail_{nq}"] = functools.partial(query_tail_case, nq)
    out["clamped"] = clamped_case
    out["grown_grid_under"] = functools.partial(grown_grid_case, "under")
    out["grown_grid_over"] = functools.partial(grown_grid_case, "over")
    for F in WIDTHS:
        out[f"width_{F}"] = functools.partial(width_case, F)
    for shape in PATCH_SHAPES:
        out["patch_%dx%d_%dx%d" % shape] = functools.partial(patch_case, *shape)
    return out


# which fixtures each wrong search must fail on (tests/test_camera_cases.py asserts the table and prints what it finds)
REJECTED_BY = {
    "plain_radius": ("scaled", "anisotropic", "sheared", "mixed_sigma"),
    "no_slack": ("boundary",),
    "squared": ("boundary",),
    "le": ("boundary", "scaled"),
    "no_clamp": ("clamped",),
    "mask32": ("views_33", "views_63", "views_64"),
    "all_views_zero": ("views_64",),
    "early_exit_any": ("cell_runs",),
    "first16": ("cell_runs",),
}
