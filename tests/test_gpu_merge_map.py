"""``ai_merge_map`` / ``labels_api.merge_map`` on the device against the NumPy restatement of rules M1-M10
(``tests/merge_map_ref.py``), which ``tests/test_merge_map_ref.py`` holds against the reference's merge.

Every fixture has at most 6 chunks of at most 2 000 points, except the one map with 70 000 provisional ids (7 x 10 000 points)
and the one chunk that spans a second row of reduction slots (65 539 points); one case has 3 005 points in two chunks.  Equality is exact everywhere: coordinates bit
for bit, ids, sources, tables and statistics as integers, device-computed centres bit for bit.  The kernel limits (box tile,
reduction shape) are read from the source.
"""
import ctypes as C
import os
import re

import numpy as np
import pytest

import merge_map_cases as mc
import merge_map_ref as ref

pytestmark = pytest.mark.gpu

_CSRC = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autoinst_amd", "csrc")


def _define(text, name):
    m = re.search(r"^\s*#define\s+" + name + r"\s+\(?(\d+)\)?\s*(?://.*)?$", text, re.M)
    assert m, f"#define {name} <integer> not found"
    return int(m.group(1))


def _constants():
    with open(os.path.join(_CSRC, "ai_merge.hip")) as f:
        merge = f.read()
    with open(os.path.join(_CSRC, "ai_common.h")) as f:
        common = f.read()
    return dict(BOX_TILE=_define(merge, "MM_BOX_TILE"), RED_BLOCKS=_define(merge, "MM_RED_BLOCKS"), BLOCK=_define(common, "AI_BLOCK"),
                HIST=_define(merge, "MM_HIST"), DISTINCT_TILE=_define(merge, "MM_DISTINCT_TILE"),
                LDS_BOXES=_define(merge, "MM_LDS_BOXES"), SCALAR_TILE=_define(merge, "MM_SCALAR_TILE"))


ALL = ("xyz", "inst", "src", "table", "stats")


def c_merge(ctx, points, instances, centers=None, mem="host", side_length=mc.SIDE, iou_min=0.01, want=ALL, off=None, n_out=True):
    """One raw ``ai_merge_map`` call: (status, dict of the outputs asked for + centers).  mem = "host" or "device"."""
    from autoinst_amd import _ffi
    lib = _ffi.load()
    pts = [np.ascontiguousarray(p, dtype=np.float64).reshape(-1, 3) for p in points]
    ins = [np.ascontiguousarray(i, dtype=np.int32).reshape(-1) for i in instances]
    n = len(pts)
    if off is None:
        off = np.zeros(n + 1, dtype=np.int64)
        off[1:] = np.cumsum([p.shape[0] for p in pts])
    off = np.ascontiguousarray(off, dtype=np.int64)
    m = int(sum(p.shape[0] for p in pts))
    xyz = np.concatenate(pts) if n else np.zeros((0, 3))
    loc = np.concatenate(ins) if n else np.zeros(0, dtype=np.int32)
    goff = mc.goff_of([np.maximum(i, 0) for i in ins])
    cen = None if centers is None else np.ascontiguousarray(centers, dtype=np.float64).reshape(n, 3)
    table = np.full(int(goff[-1]) + 1, -7, dtype=np.int32)
    stats = np.full((max(n, 1), 4), -7, dtype=np.int64)
    used = np.full((max(n, 1), 3), -7.0)
    total = C.c_int64(-7)
    if mem == "device":
        import torch
        dx, di = torch.as_tensor(xyz, device="cuda"), torch.as_tensor(loc, device="cuda")
        ox = torch.full((max(m, 1), 3), -7.0, dtype=torch.float64, device="cuda")
        oi = torch.full((max(m, 1),), -7, dtype=torch.int32, device="cuda")
        os_ = torch.full((max(m, 1),), -7, dtype=torch.int64, device="cuda")
        torch.cuda.synchronize()
        ptr = lambda t: C.c_void_p(t.data_ptr())  # noqa: E731
        kind = _ffi.AI_MEM_DEVICE
    else:
        dx, di = xyz, loc
        ox, oi, os_ = np.full((max(m, 1), 3), -7.0), np.full(max(m, 1), -7, np.int32), np.full(max(m, 1), -7, np.int64)
        ptr = lambda a: C.c_void_p(a.ctypes.data)  # noqa: E731
        kind = _ffi.AI_MEM_HOST
    status = lib.ai_merge_map(
        ctx._h, ptr(dx) if m else None, ptr(di) if m else None, off.ctypes.data, n, cen.ctypes.data if cen is not None else None,
        float(side_length), float(iou_min), kind, ptr(ox) if "xyz" in want else None, ptr(oi) if "inst" in want else None,
        ptr(os_) if "src" in want else None, C.byref(total) if n_out else None, table.ctypes.data if "table" in want else None,
        stats.ctypes.data if "stats" in want else None, used.ctypes.data)
    if status != 0:
        return status, lib.ai_last_error().decode()
    k = int(total.value)
    host = (lambda t: t.cpu().numpy()) if mem == "device" else (lambda a: a)
    out = {"n_out": k, "centers": used[:n]}
    # what was not asked for must not have been written, and nothing beyond n_out rows
    for name, arr, fill in (("xyz", host(ox), -7.0), ("inst", host(oi), -7), ("src", host(os_), -7)):
        assert (arr[k:] == fill).all() and (name in want or (arr == fill).all()), name
        if name in want:
            out[name] = arr[:k]
    if "table" in want:
        out["table"] = [np.concatenate([[0], table[goff[c] + 1:goff[c + 1] + 1]]).astype(np.int32) for c in range(n)]
        assert table[0] == 0
    else:
        assert (table == -7).all()
    if "stats" in want:
        out["stats"] = stats[:n]
    else:
        assert (stats == -7).all()
    return 0, out


def assert_equal(got, exp, want=ALL, what=""):
    assert got["n_out"] == exp["src"].size, what
    if "xyz" in want:
        assert np.ascontiguousarray(got["xyz"]).tobytes() == np.ascontiguousarray(exp["points"]).tobytes(), what
    if "inst" in want:
        assert np.array_equal(got["inst"], exp["inst"]), what
    if "src" in want:
        assert np.array_equal(got["src"], exp["src"]), what
    if "table" in want:
        assert len(got["table"]) == len(exp["table"]) and all(np.array_equal(a, b) for a, b in zip(got["table"], exp["table"])), what
    if "stats" in want:
        assert np.array_equal(got["stats"], exp["stats"]), what


def run_and_check(ctx, points, instances, centers=None, mems=("host", "device"), what="", **kw):
    exp = ref.merge_map(points, instances, centers=centers, **kw)
    for mem in mems:
        status, got = c_merge(ctx, points, instances, centers, mem, **kw)
        assert status == 0, (what, got)
        assert_equal(got, exp, what=(what, mem))
    return exp, got


@pytest.fixture(scope="module")
def random25():
    maps = mc.random_maps(25, seed=77)
    return [(p, i, mc.mean_centers(p)) for p, i in maps]


# ------------------------------------------------------------------------------------------------- the CPU cases on the device
@pytest.mark.parametrize("mem", ["host", "device"])
def test_hand_made_cases(ctx, mem):
    for name, case in mc.hand_cases().items():
        exp = ref.merge_map(case["points"], case["instances"], centers=case["centers"])
        assert exp["inst"].tolist() == list(case["inst"]) and exp["src"].tolist() == list(case["src"])
        status, got = c_merge(ctx, case["points"], case["instances"], case["centers"], mem)
        assert status == 0, (name, got)
        assert_equal(got, exp, what=name)
        status, again = c_merge(ctx, case["points"], case["instances"], case["centers"], mem)     # reproducible
        assert status == 0
        assert_equal(again, exp, what=name)
        for leave_out in ALL:                                                                       # each optional output NULL
            want = tuple(w for w in ALL if w != leave_out)
            status, part = c_merge(ctx, case["points"], case["instances"], case["centers"], mem, want=want)
            assert status == 0, (name, leave_out, part)
            assert_equal(part, exp, want=want, what=(name, leave_out))
        status, none = c_merge(ctx, case["points"], case["instances"], case["centers"], mem, want=())
        assert status == 0 and none["n_out"] == exp["src"].size


@pytest.mark.parametrize("mem", ["host", "device"])
def test_random_maps_equal_the_restatement(ctx, random25, mem):
    for k, (points, instances, centers) in enumerate(random25):
        exp = ref.merge_map(points, instances, centers=centers)
        for rep in range(2):
            status, got = c_merge(ctx, points, instances, centers, mem)
            assert status == 0, (k, got)
            assert_equal(got, exp, what=(k, rep))


def test_merge_map_matches_the_colour_merge(ctx, random25):
    """Through M11's colours, `merge_map` is the existing `merge_chunks_unite_instances2`: same points bit for bit, and the
    colours are colour(instance).  The colour merge takes np.mean of each chunk itself; the same values go in as centres."""
    from autoinst_amd import labels_api
    for k, (points, instances, centers) in enumerate(random25):
        assert mc.face_distance(points, centers) > 1e-6
        p, inst, src = labels_api.merge_map(points, instances, centers=centers, ctx=ctx)
        ep, ec = labels_api.merge_chunks_unite_instances2(mc.colour_chunks(points, instances), ctx=ctx)
        assert p.tobytes() == np.ascontiguousarray(ep).tobytes(), k
        assert np.array_equal(mc.colour(inst), ec), k
        assert np.concatenate(points)[src].tobytes() == p.tobytes(), k


def test_python_entry_device_tensors_tables_and_export(ctx, random25):
    import torch
    import autoinst_amd
    assert autoinst_amd.merge_map is autoinst_amd.labels_api.merge_map
    points, instances, centers = max(random25, key=lambda t: len(t[0]))
    exp = ref.merge_map(points, instances, centers=centers)
    tp = [torch.as_tensor(p, device="cuda") for p in points]
    ti = [torch.as_tensor(i.astype(np.int64), device="cuda") for i in instances]
    p, inst, src, table, stats = autoinst_amd.merge_map(tp, ti, centers=centers, return_table=True, return_stats=True, ctx=ctx)
    assert p.is_cuda and inst.is_cuda and src.is_cuda and inst.dtype == torch.int32 and src.dtype == torch.int64
    got = {"n_out": int(p.shape[0]), "xyz": p.cpu().numpy(), "inst": inst.cpu().numpy(), "src": src.cpu().numpy(), "table": table,
           "stats": stats}
    assert_equal(got, exp)
    gt = torch.cat([torch.arange(x.shape[0], device="cuda") + 1000 * c for c, x in enumerate(tp)])    # any per-point value
    assert torch.equal(gt[src].cpu(), torch.as_tensor(np.concatenate([np.arange(x.shape[0]) + 1000 * c
                                                                      for c, x in enumerate(points)])[exp["src"]]))
    hp, hi, hs = autoinst_amd.merge_map(points, instances, ctx=ctx)                                     # host arrays, M4 centres
    own = ref.merge_map(points, instances)
    assert hp.tobytes() == own["points"].tobytes() and np.array_equal(hi, own["inst"]) and np.array_equal(hs, own["src"])


# ------------------------------------------------------------------------------------------------- M4
def test_device_centres_are_the_stated_reduction(ctx):
    K = _constants()
    assert K["RED_BLOCKS"] * K["BLOCK"] == ref.SLOTS and K["BLOCK"] == ref.BLOCK
    rng = np.random.default_rng(4)
    sizes = [1, 2, K["BLOCK"] - 1, K["BLOCK"], K["BLOCK"] + 1, 4 * K["BLOCK"] + 1, ref.SLOTS + 3]
    points = [rng.normal([50.0, -30.0, 2.0], [30.0, 20.0, 1.0], (n, 3)) for n in sizes]
    instances = [np.zeros(n, dtype=np.int32) for n in sizes]
    for mem in ("host", "device"):
        status, got = c_merge(ctx, points, instances, None, mem, want=("src",))
        assert status == 0, got
        for c, p in enumerate(points):
            exp = ref.center_m4(p)
            assert got["centers"][c].tobytes() == exp.tobytes(), (mem, sizes[c])
            bound = sizes[c] * 2.0 ** -52 * np.abs(p).max(0)
            assert (np.abs(got["centers"][c] - p.mean(0)) <= bound).all(), (mem, sizes[c])
    # independent of what else shares the call: the last chunk alone
    status, alone = c_merge(ctx, points[-2:-1], instances[-2:-1], None, "device", want=())
    assert status == 0 and alone["centers"][0].tobytes() == got["centers"][-2].tobytes()


def test_device_centres_decide_the_crop(ctx, random25):
    for k, (points, instances, _) in enumerate(random25[:8]):
        run_and_check(ctx, points, instances, None, mems=("device",), what=k)


# ------------------------------------------------------------------------------------------------- kernel limits
def _many_instances(n_inst, seed):
    """A map chunk of n_inst two-point instances on a line (all inside the crop) and a chunk whose instances meet some of them."""
    rng = np.random.default_rng(seed)
    x = np.arange(n_inst) * 0.03125 - 8.0
    a = np.stack([x, np.zeros(n_inst), np.zeros(n_inst)], 1)
    b = a + [0.015625, 1.0, 1.0]
    ids = rng.permutation(n_inst) + 1
    map_p, map_i = np.concatenate([a, b]), np.concatenate([ids, ids])
    pick = np.unique(np.concatenate([[np.argmin(ids), np.argmax(ids), 0, n_inst - 1], rng.integers(0, n_inst, 12)]))   # first and last rank
    new_p = np.concatenate([a[pick] + [0.0078125, 0.5, 0.5], a[pick] + [0.0078125, 0.25, 0.75], [[0.0, 30.0, 0.0]]])
    new_i = np.concatenate([np.arange(pick.size) + 1, np.arange(pick.size) + 1, [pick.size + 1]])
    return [map_p, new_p], [map_i.astype(np.int32), new_i.astype(np.int32)], np.zeros((2, 3))


@pytest.mark.parametrize("delta", [-1, 0, 1])
@pytest.mark.parametrize("limit", ["BOX_TILE", "LDS_BOXES"])
def test_instances_in_the_crop_at_the_box_tile(ctx, limit, delta):
    """The number of map instances present in a crop at `kg_inside`'s LDS tile of boxes, and at the number of boxes up to which
    `kg_scalars_map` gathers them in LDS (beyond it: global atomics).  Two points per instance; with 513 instances the 1 026
    cropped points also cross `kg_scalars_map`'s tile of points."""
    K = _constants()
    n_inst = K[limit] + delta
    assert K["BOX_TILE"] + 1 < K["LDS_BOXES"] - 1 and 2 * (K["LDS_BOXES"] + 1) > K["SCALAR_TILE"] > 2 * (K["BOX_TILE"] + 1)
    points, instances, centers = _many_instances(n_inst, 10 + delta)
    exp, _ = run_and_check(ctx, points, instances, centers, what=n_inst)
    assert exp["stats"][1, 1] == n_inst and exp["stats"][1, 3] >= 3       # the last box of the last tile is met too


@pytest.mark.parametrize("where", ["below", "above", "blocks"])
def test_scalar_entries_at_the_distinct_tile(ctx, where):
    """`kg_distinct` takes MM_DISTINCT_TILE sorted (value, instance) entries per block, three per selected point, and counts
    them in LDS while the counters fit (here) and in global memory otherwise (the 70 000-id map below): one block nearly
    full, one entry into the second block, several blocks."""
    K = _constants()
    selected = {"below": K["DISTINCT_TILE"] // 3, "above": K["DISTINCT_TILE"] // 3 + 1, "blocks": 3000}[where]
    assert (3 * selected <= K["DISTINCT_TILE"]) == (where == "below") and 5 + 5 + 1 <= K["HIST"]
    rng = np.random.default_rng(selected)
    n0 = selected // 2
    cloud = np.round(rng.uniform(-6, 6, (selected, 3)) * 8) / 8              # 1/8 m grid: many shared scalars
    points = [cloud[:n0], np.concatenate([cloud[n0:], cloud[:5]])]          # every point carries an instance and is cropped
    instances = [rng.integers(1, 6, n0).astype(np.int32), rng.integers(1, 6, selected - n0 + 5).astype(np.int32)]
    exp, _ = run_and_check(ctx, points, instances, np.zeros((2, 3)))
    assert exp["stats"][1, 0] == n0 and exp["stats"][1, 1] == 5


def test_chunk_whose_instances_are_all_outside_the_crop(ctx):
    points, instances, centers = _many_instances(40, 3)
    centers = centers.copy()
    centers[1] = [500.0, 0.0, 0.0]
    exp, _ = run_and_check(ctx, points, instances, centers)
    assert exp["stats"][1].tolist() == [0, 0, 0, 0] and np.array_equal(exp["table"][1][1:], 40 + np.arange(1, exp["table"][1].size))


def test_tables_scale_with_the_crop_not_with_the_ids_of_the_map(ctx):
    """7 chunks of 10 000 one-point instances: 70 000 provisional ids, of which 3 lie in a chunk's crop.  A table over all ids
    of the map would have 60 000 x 10 001 entries at the last step, more than the entry allows."""
    n, chunks = 10_000, 7
    points, instances, centers = [], [], np.zeros((chunks, 3))
    for c in range(chunks):
        p = np.stack([c * 1000.0 + np.arange(n) / 16.0, np.full(n, float(c)), np.zeros(n)], 1)
        if c:
            p[:3] = points[c - 1][100:103]                       # meets three one-point instances of the chunk before
            centers[c] = points[c - 1][101]
        points.append(p)
        instances.append((np.random.default_rng(c).permutation(n) + 1).astype(np.int32))
    exp, got = run_and_check(ctx, points, instances, centers, mems=("device",), side_length=3.0 / 16.0)
    assert exp["stats"][1:, :2].tolist() == [[3, 3]] * (chunks - 1) and exp["stats"][1:, 3].tolist() == [3] * (chunks - 1)
    assert exp["src"].size == chunks * n - 3 * (chunks - 1) and exp["inst"].max() > 60_000


@pytest.mark.parametrize("where", ["first", "middle", "last", "all"])
def test_empty_chunks(ctx, random25, where):
    points, instances, centers = next(t for t in random25 if len(t[0]) >= 3)
    points, instances, centers = list(points), list(instances), centers.copy()
    empty_p, empty_i = np.zeros((0, 3)), np.zeros(0, dtype=np.int32)
    if where == "all":
        points, instances = [empty_p] * 3, [empty_i] * 3
        centers = None
    else:
        at = {"first": 0, "middle": 1, "last": len(points)}[where]
        points.insert(at, empty_p)
        instances.insert(at, empty_i)
        centers = np.insert(centers, at, 0.0, axis=0)
    exp, got = run_and_check(ctx, points, instances, centers, what=where)
    if where == "all":
        assert got["n_out"] == 0
    status, got = c_merge(ctx, [], [], None, "host")
    assert status == 0 and got["n_out"] == 0


def test_chunk_with_only_id_0(ctx, random25):
    points, instances, centers = next(t for t in random25 if len(t[0]) >= 3)
    instances = list(instances)
    instances[1] = np.zeros_like(instances[1])
    exp, _ = run_and_check(ctx, points, instances, centers)
    assert exp["stats"][1].tolist() == [0, 0, 0, 0]
    run_and_check(ctx, points, [np.zeros_like(i) for i in instances], centers)


def test_a_far_chunk_changes_no_earlier_row(ctx, random25):
    points, instances, centers = max(random25, key=lambda t: len(t[0]))
    status, base = c_merge(ctx, points, instances, None, "device")
    assert status == 0
    far = points[0] + [1000.0, 0.0, 0.0]
    assert np.abs(far - np.concatenate(points).mean(0)).max() > 40.0
    status, more = c_merge(ctx, list(points) + [far], list(instances) + [instances[0]], None, "device")
    assert status == 0
    k = base["n_out"]
    assert more["n_out"] == k + np.unique(far, axis=0).shape[0]
    assert more["xyz"][:k].tobytes() == base["xyz"].tobytes()
    assert np.array_equal(more["inst"][:k], base["inst"]) and np.array_equal(more["src"][:k], base["src"])
    assert all(np.array_equal(a, b) for a, b in zip(more["table"], base["table"]))
    assert np.array_equal(more["stats"][:-1], base["stats"]) and more["stats"][-1].tolist() == [0, 0, 0, 0]
    assert more["centers"][:-1].tobytes() == base["centers"].tobytes()


# ------------------------------------------------------------------------------------------------- M10
def test_errors(ctx):
    from autoinst_amd import labels_api
    p = [np.zeros((2, 3)), np.ones((3, 3))]
    i = [np.array([1, 1], np.int32), np.array([1, 2, 2], np.int32)]
    nan = [p[0], np.array([[1.0, np.nan, 1.0], [1, 1, 1], [2, 2, 2]])]
    inf = [np.array([[np.inf, 0, 0], [1, 1, 1]]), p[1]]
    neg = [i[0], np.array([1, -2, 2], np.int32)]
    cases = [
        (dict(points=p, instances=i, off=[1, 2, 5]), "do not start at 0"),
        (dict(points=p, instances=i, off=[0, 3, 2]), "decrease at chunk 1"),
        (dict(points=p, instances=neg), "chunk 1 has a negative"),
        (dict(points=nan, instances=i), "chunk 1 has a coordinate that is not finite"),
        (dict(points=inf, instances=i), "chunk 0 has a coordinate that is not finite"),
        (dict(points=p, instances=i, centers=[[0, 0, 0], [0, np.nan, 0]]), "centre of chunk 1 is not finite"),
        (dict(points=p, instances=i, centers=[[np.inf, 0, 0], [0, 0, 0]]), "centre of chunk 0 is not finite"),
        (dict(points=p, instances=i, side_length=0.0), "side_length"),
        (dict(points=p, instances=i, side_length=-1.0), "side_length"),
        (dict(points=p, instances=i, iou_min=float("nan")), "iou_min"),
        (dict(points=p, instances=i, iou_min=float("inf")), "iou_min"),
        (dict(points=p, instances=i, n_out=False), "n_out"),
    ]
    for kw, text in cases:
        for mem in ("host", "device"):
            status, msg = c_merge(ctx, kw["points"], kw["instances"], kw.get("centers"), mem,
                                  **{k: v for k, v in kw.items() if k not in ("points", "instances", "centers")})
            assert status == -1 and "ai_merge_map" in msg and text in msg, (kw, msg)
    for kw, text in cases:
        if "off" in kw or "n_out" in kw:
            continue
        args = {k: v for k, v in kw.items() if k not in ("points", "instances")}
        with pytest.raises(ValueError, match=text.split(" ")[-1] if " " in text else text):
            labels_api.merge_map(kw["points"], kw["instances"], ctx=ctx, **args)
    with pytest.raises(ValueError):
        labels_api.merge_map(p, i[:1], ctx=ctx)
    with pytest.raises(ValueError):
        labels_api.merge_map(p, [i[0], i[1][:2]], ctx=ctx)
    # a good call after the refused ones
    run_and_check(ctx, p, i, np.zeros((2, 3)))
