"""The device's hidden point removal (csrc/ai_hidden.hip, rules H1-H6 of include/autoinst_hip.h) restated in NumPy, bit for bit:
the same float64 operations in the same order per constraint, exact min / max per re-solve, the same lists of constraints.
One Python loop turn per point, NumPy over the constraints of a re-solve.  Nothing here comes from the reference."""
import numpy as np

GRID = 64        # cells per axis of the direction grid over [-1, 1]^3
BOX = 1e12       # |t_k| <= BOX
F = np.float64


def transform(points, T):
    """H1: row r = ((T[r,0]*x + T[r,1]*y) + T[r,2]*z) + T[r,3], divided by row 3, every step rounded on its own."""
    p = np.asarray(points, dtype=F).reshape(-1, 3)
    T = np.asarray(T, dtype=F)
    x, y, z = p[:, 0], p[:, 1], p[:, 2]
    with np.errstate(all="ignore"):
        rows = [((T[r, 0] * x + T[r, 1] * y) + T[r, 2] * z) + T[r, 3] for r in range(4)]
        return np.stack([rows[0] / rows[3], rows[1] / rows[3], rows[2] / rows[3]], 1)


def _cell(e):
    return np.minimum(np.maximum(np.floor((e + 1.0) * 32.0), 0), GRID - 1).astype(np.int64)


def prepare(p, radius_factor):
    """H2, H5, H6 for one view's camera-frame points: None for a skipped view, else the sorted records and the cell table."""
    p = np.asarray(p, dtype=F).reshape(-1, 3)
    n = p.shape[0]
    if n < 4:
        return None
    with np.errstate(all="ignore"):
        v = np.where(np.abs(p) < np.inf, p, np.inf)
        mn, mx = v.min(axis=0), v.max(axis=0)
        dx, dy, dz = mx - mn
        D = np.sqrt((dx * dx + dy * dy) + dz * dz)
        R = F(radius_factor) * D
        two_R = F(2.0) * R
        S = two_R * two_R
        fx, fy, fz = np.maximum(np.abs(mn), np.abs(mx))
        far = np.sqrt((fx * fx + fy * fy) + fz * fz)
        if not (R > 0.0 and abs(S) < np.inf and fx < np.inf and fy < np.inf and fz < np.inf and far < two_R):
            return None
        x, y, z = p[:, 0], p[:, 1], p[:, 2]
        d = np.sqrt((x * x + y * y) + z * z)
        d[d == 0.0] = 0.0001
        e = p / d[:, None]
        u = S / (two_R - d)
    c = _cell(e)
    key = (c[:, 2] * GRID + c[:, 1]) * GRID + c[:, 0]
    order = np.argsort(key, kind="stable")
    skey = key[order]
    return {"n": n, "order": order, "E": np.ascontiguousarray(e[order]), "U": np.ascontiguousarray(u[order]), "skey": skey,
            "cell": c[order]}


def basis(ex, ey, ez):
    """H3: a = (e x axis) / |e x axis| with the axis of the smallest |component| (the lower axis on a tie), b = e x a."""
    fx, fy, fz = abs(ex), abs(ey), abs(ez)
    zero = F(0.0)
    if fx <= fy and fx <= fz:
        cx, cy, cz = zero, ez, -ey
    elif fy <= fz:
        cx, cy, cz = -ez, zero, ex
    else:
        cx, cy, cz = ey, -ex, zero
    with np.errstate(all="ignore"):
        nrm = np.sqrt((cx * cx + cy * cy) + cz * cz)
        ax, ay, az = cx / nrm, cy / nrm, cz / nrm
    bx = ey * az - ez * ay
    by = ez * ax - ex * az
    bz = ex * ay - ey * ax
    return (ax, ay, az), (bx, by, bz)


def constraints(ex, ey, ez, u, E, U):
    """H3 for one query against the records (E, U): A0, A1, g."""
    (ax, ay, az), (bx, by, bz) = basis(ex, ey, ez)
    Ex, Ey, Ez = E[:, 0], E[:, 1], E[:, 2]
    c = (ex * Ex + ey * Ey) + ez * Ez
    c = np.where((Ex == ex) & (Ey == ey) & (Ez == ez), 1.0, c)
    wx, wy, wz = Ex - c * ex, Ey - c * ey, Ez - c * ez
    A0 = (wx * ax + wy * ay) + wz * az
    A1 = (wx * bx + wy * by) + wz * bz
    g = U - c * u
    return A0, A1, g


_BOX0 = np.array([1.0, -1.0, 0.0, 0.0])
_BOX1 = np.array([0.0, 0.0, 1.0, -1.0])
_BOXG = np.full(4, BOX)


def seidel(A0, A1, g, t0, t1, trace=None):
    """H4 over the list (A0, A1, g) from the start (t0, t1): (feasible, t0, t1, re-solves).  ``trace`` (a list) receives the list
    position of every re-solve, the infeasible one included."""
    t0, t1 = F(t0), F(t1)
    n, pos, nres = g.shape[0], 0, 0
    with np.errstate(all="ignore"):
        while pos < n:
            viol = (t0 * A0[pos:] + t1 * A1[pos:]) > g[pos:]
            if not viol.any():
                break
            k = pos + int(np.argmax(viol))
            nres += 1
            if trace is not None:
                trace.append(k)
            ok, t0, t1 = _resolve(A0, A1, g, t0, t1, k)
            if not ok:
                return False, t0, t1, nres
            pos = k + 1
    return True, t0, t1, nres


# the 27 cells of the local list: the point's own cell first, then the others in (dz, dy, dx) order
_OFFSETS = [(0, 0, 0)] + [(dx, dy, dz) for dz in (-1, 0, 1) for dy in (-1, 0, 1) for dx in (-1, 0, 1) if (dx, dy, dz) != (0, 0, 0)]


def visible_flags(p_cam, radius_factor, stats=None, rows=None):
    """The flags of one view's camera-frame points (uint8, input order), or None for a skipped view.  ``stats`` (a dict) receives
    what the library's stats_out holds: local_hidden, resolves, max_resolves, at_camera.  With ``rows`` only those input rows
    are decided, each against all points of the view, and their flags are returned in the order of ``rows``."""
    pr = prepare(p_cam, radius_factor)
    if pr is None:
        return None
    n, E, U, order = pr["n"], pr["E"], pr["U"], pr["order"]
    flags = np.zeros(n, dtype=np.uint8)
    st = {"local_hidden": 0, "resolves": 0, "max_resolves": 0, "at_camera": 0}
    local = _local_lists(pr)
    if rows is None:
        todo = range(n)
    else:
        where = np.empty(n, dtype=np.int64)
        where[order] = np.arange(n)
        todo = where[np.asarray(rows, dtype=np.int64).reshape(-1)]
    for p in todo:
        ex, ey, ez, u = E[p, 0], E[p, 1], E[p, 2], U[p]
        if ex == 0.0 and ey == 0.0 and ez == 0.0:
            st["at_camera"] += 1
            continue
        A0, A1, g = constraints(ex, ey, ez, u, E, U)
        loc = local(p)
        ok, t0, t1, nres = seidel(A0[loc], A1[loc], g[loc], 0.0, 0.0)
        if not ok:
            st["local_hidden"] += 1
        else:
            ok, t0, t1, more = seidel(A0, A1, g, t0, t1)
            nres += more
        st["resolves"] += nres
        st["max_resolves"] = max(st["max_resolves"], nres)
        flags[order[p]] = 1 if ok else 0
    if stats is not None:
        stats.update(st)
    return flags if rows is None else flags[np.asarray(rows, dtype=np.int64).reshape(-1)]


def hidden_point_removal(points, camera=(0.0, 0.0, 0.0), radius_factor=1000.0, stats=None):
    """Ascending indices of the visible points, as `camera_api.hidden_point_removal_device` gives them; ValueError for a skipped
    cloud."""
    T = np.eye(4)
    T[:3, 3] = -np.asarray(camera, dtype=F).reshape(3)
    flags = visible_flags(transform(points, T), radius_factor, stats)
    if flags is None:
        raise ValueError("skipped")
    return np.flatnonzero(flags).astype(np.int64)


def visible_sets(cloud, T_pcd2cam, subset=None, radius_factor=1000.0):
    """`camera_api.visible_sets`: per view the ascending rows of ``cloud``, None for a skipped view."""
    cloud = np.asarray(cloud, dtype=F).reshape(-1, 3)
    sub = np.arange(cloud.shape[0]) if subset is None else np.asarray(subset, dtype=np.int64).reshape(-1)
    out = []
    for T in np.asarray(T_pcd2cam, dtype=F).reshape(-1, 4, 4):
        flags = visible_flags(transform(cloud[sub], T), radius_factor)
        out.append(None if flags is None else sub[np.flatnonzero(flags)].astype(np.int64))
    return out


# ------------------------------------------------------------------------------------------ the skip rule of the global pass
TILE = 256        # sorted records per tile
SKIP_EPS = 1e-9


def tile_boxes(E):
    """Per tile of TILE sorted records: min x, y, z, max x, y, z of the directions."""
    return np.array([np.concatenate([E[a:a + TILE].min(axis=0), E[a:a + TILE].max(axis=0)]) for a in range(0, E.shape[0], TILE)])


def can_skip(ex, ey, ez, u, t0, t1, b, u_min, variant="rule"):
    """hp_can_skip of csrc/ai_hidden.hip, operation for operation.  The other variants are wrong in one place each; the fixtures
    of tests/test_hpr_ref.py reject them."""
    with np.errstate(all="ignore"):
        cu = ((max(ex * b[0], ex * b[3]) + max(ey * b[1], ey * b[4])) + max(ez * b[2], ez * b[5])) + 1e-15
        s2 = 1.0 - cu * cu
        if not (cu < 1.0 and s2 >= 1e-6):
            return False
        sl = np.sqrt(s2)
        tn = np.sqrt(t0 * t0 + t1 * t1)
        if variant == "own_u":          # the point's own u in place of the view's smallest
            u_min = u
        if variant == "no_t":           # the |t| sin term dropped
            tn = F(0.0)
        rising = cu <= 0.0 or sl * u >= (tn * cu) * (1.0 + SKIP_EPS)
        if variant == "no_rising":      # f may fall again beyond the box's nearest angle
            rising = True
        clear = (u_min - u * cu) - tn * sl > SKIP_EPS * ((u_min + u) + tn)
    return bool(rising and clear)


def skip_audit(p_cam, radius_factor, variant="rule"):
    """The global pass of every survivor, tile by tile as kh_global walks it: (tiles met, tiles passed over, tiles passed over
    that hold a constraint violated at the lane's t, points whose flag a wrong pass-over changes)."""
    pr = prepare(p_cam, radius_factor)
    E, U, n = pr["E"], pr["U"], pr["n"]
    boxes, u_min = tile_boxes(E), U.min()
    full = visible_flags(p_cam, radius_factor)[pr["order"]]
    met = passed = unsound = changed = 0
    local = _local_lists(pr)
    for p in range(n):
        ex, ey, ez, u = E[p, 0], E[p, 1], E[p, 2], U[p]
        if ex == 0.0 and ey == 0.0 and ez == 0.0:
            continue
        A0, A1, g = constraints(ex, ey, ez, u, E, U)
        loc = local(p)
        ok, t0, t1, _ = seidel(A0[loc], A1[loc], g[loc], 0.0, 0.0)
        if not ok:
            continue
        for k, a in enumerate(range(0, n, TILE)):
            b = min(a + TILE, n)
            met += 1
            if can_skip(ex, ey, ez, u, t0, t1, boxes[k], u_min, variant):
                passed += 1
                with np.errstate(all="ignore"):
                    unsound += int(((t0 * A0[a:b] + t1 * A1[a:b]) > g[a:b]).any())
                continue
            ok, t0, t1, _ = _seidel_range(A0, A1, g, t0, t1, a, b)
            if not ok:
                break
        changed += int(bool(ok) != bool(full[p]))
    return met, passed, unsound, changed


def _seidel_range(A0, A1, g, t0, t1, a, b, trace=None):
    """`seidel` over positions a .. b - 1 of the list, the earlier constraints being all positions below the violated one.
    ``trace`` (a list) receives the position of every re-solve, the infeasible one included."""
    pos = a
    with np.errstate(all="ignore"):
        while pos < b:
            viol = (t0 * A0[pos:b] + t1 * A1[pos:b]) > g[pos:b]
            if not viol.any():
                break
            k = pos + int(np.argmax(viol))
            if trace is not None:
                trace.append(k)
            ok, t0, t1 = _resolve(A0, A1, g, t0, t1, k)
            if not ok:
                return False, t0, t1, 0
            pos = k + 1
    return True, t0, t1, 0


def _resolve(A0, A1, g, t0, t1, k):
    """One re-solve of H4 at constraint k."""
    a0, a1, gk = A0[k], A1[k], g[k]
    nn = a0 * a0 + a1 * a1
    if nn == 0.0:
        return False, t0, t1
    f = ((t0 * a0 + t1 * a1) - gk) / nn
    p0, p1 = t0 - a0 * f, t1 - a1 * f
    d0, d1 = -a1, a0
    B0, B1, G = np.concatenate([_BOX0, A0[:k]]), np.concatenate([_BOX1, A1[:k]]), np.concatenate([_BOXG, g[:k]])
    den = B0 * d0 + B1 * d1
    num = G - (B0 * p0 + B1 * p1)
    up, down = den > 0.0, den < 0.0
    hi = np.fmin.reduce(num[up] / den[up], initial=np.inf)
    lo = np.fmax.reduce(num[down] / den[down], initial=-np.inf)
    if ((den == 0.0) & (num < 0.0)).any() or lo > hi:
        return False, t0, t1
    s = np.fmin(np.fmax(F(0.0), lo), hi)
    return True, p0 + s * d0, p1 + s * d1


def _local_lists(pr):
    E, skey, cell = pr["E"], pr["skey"], pr["cell"]

    def local(p):
        cx, cy, cz = cell[p]
        parts = []
        for dx, dy, dz in _OFFSETS:
            xx, yy, zz = cx + dx, cy + dy, cz + dz
            if 0 <= xx < GRID and 0 <= yy < GRID and 0 <= zz < GRID:
                k = (zz * GRID + yy) * GRID + xx
                a, b = np.searchsorted(skey, k, "left"), np.searchsorted(skey, k, "right")
                if b > a:
                    parts.append(np.arange(a, b))
        return np.concatenate(parts)
    return local
