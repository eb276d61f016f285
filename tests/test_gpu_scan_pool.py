"""GPU: ai_scan_pool (points_api.tarl_pool_map / tarl_features_per_map) against the restatement tests/scan_pool_ref.py.

Counts are exact.  Means agree within ``count * 2^-52 * max|f|`` per query: two float64 sums of the same ``count`` float32
values in different orders, each followed by one division (scan_pool_ref.bound).  The order rule R4 is checked with array_equal.
"""
import numpy as np
import pytest

import scan_pool_ref as sp

pytestmark = pytest.mark.gpu

SHIFTS = {"origin": (0.0, 0.0, 0.0), "far": (1234.0, -1234.0, 0.0)}


@pytest.fixture(scope="module", params=sorted(SHIFTS))
def base(request):
    case = sp.base_case(shift=SHIFTS[request.param])
    return {"case": case, "ref": sp.pool(case), "name": request.param}


def _run(case, ctx, **kw):
    from autoinst_amd import points_api
    return points_api.tarl_pool_map(case["scans"], case["feats"], case["T"], case["chunks"], case["boxes"], case["wins"],
                                    radius=case["radius"], return_count=True, ctx=ctx, **kw)


def _check(case, ref, got, cnt):
    assert len(got) == len(ref) == len(cnt)
    for c, (r, g, n) in enumerate(zip(ref, got, cnt)):
        g, n = np.asarray(g), np.asarray(n)
        assert g.shape == r["mean"].shape and g.dtype == np.float64 and n.dtype == np.int32
        bad = np.flatnonzero(n != r["count"])
        assert bad.size == 0, f"chunk {c}: {bad.size} counts differ, e.g. query {bad[:5]}: {n[bad[:5]]} vs {r['count'][bad[:5]]}"
        err = np.abs(g - r["mean"])
        assert np.all(err <= sp.bound(r)), f"chunk {c}: worst excess {np.max(err - sp.bound(r))}"
        assert not g[n == 0].any()


def test_fixture_discriminates(base):
    d = sp.discrimination(base["case"])
    assert all(v > 0 for v in d.values()), d
    assert all(1400 < c.shape[0] < 1600 for c in base["case"]["chunks"]) and all(s.shape[0] == 4000 for s in base["case"]["scans"])
    assert sum(int((r["count"] > 0).sum()) for r in base["ref"]) > 1000


def test_counts_and_means(base, ctx):
    got, cnt = _run(base["case"], ctx)
    _check(base["case"], base["ref"], got, cnt)


class _Cloud:
    def __init__(self, points):
        self.points = points


class _Dataset:
    """get_tarl_features / get_point_cloud / get_pose of a case's scans under the ids ``ids``; counts the reads."""

    def __init__(self, case, ids, T_pcd):
        self.case, self.pos, self.T_pcd = case, {i: k for k, i in enumerate(ids)}, T_pcd
        self.reads = {"get_tarl_features": [], "get_point_cloud": [], "get_pose": []}

    def get_tarl_features(self, i):
        self.reads["get_tarl_features"].append(i)
        return self.case["feats"][self.pos[i]]

    def get_point_cloud(self, i):
        self.reads["get_point_cloud"].append(i)
        return self.case["scans"][self.pos[i]]

    def get_pose(self, i):
        self.reads["get_pose"].append(i)
        return self.T_pcd @ self.case["T"][self.pos[i]]


def test_per_chunk_composition(base, ctx):
    """Each chunk's rows against the existing per-chunk path with the fixed-order transform (the same membership rule)."""
    from autoinst_amd import camera_api, points_api
    case = base["case"]
    got, _ = _run(case, ctx)
    ds = _Dataset(case, list(range(len(case["scans"]))), np.eye(4))
    for c, r in enumerate(base["ref"]):
        w0, w1 = case["wins"][c]
        one = points_api.tarl_features_per_patch(ds, _Cloud(case["chunks"][c]), np.eye(4), case["centers"][c], list(range(w0, w1)),
                                                 transform_pcd=camera_api.transform_points, ctx=ctx)
        assert np.all(np.abs(got[c] - one) <= sp.bound(r)), c


def test_map_level_call(ctx):
    """tarl_features_per_map reads each scan of the union of the windows once and returns the per-chunk drop-in's list."""
    from autoinst_amd import camera_api, points_api
    case = sp.base_case(n_scans=8, per_scan=1500, per_chunk=500, seed=4)
    ids = [100 + 7 * k for k in range(8)]                       # the sampled scans' dataset indices
    T_pcd = sp.pose(0.2, 0.01, -0.03, (3.0, -2.0, 0.5))        # get_pose = T_pcd @ T, so inv(T_pcd) @ get_pose ~ T
    center_ids = [ids[1], ids[2], ids[5]]                       # windows (2, 1): [0, 2), [0, 3), [3, 6); scans 6, 7 are never read
    cd = {"center_ids": center_ids, "center_positions": case["centers"],
          "pcd_nonground_chunks_major_downsampling": [_Cloud(c) for c in case["chunks"]]}
    # the transforms the call forms, and the restatement's bound for them
    T_eff = np.array([np.linalg.inv(T_pcd) @ (T_pcd @ t) for t in case["T"]])
    assert np.all(T_eff[:, 3] == [0.0, 0.0, 0.0, 1.0])
    wins = [points_api.tarl_window(ids, cid, (2, 1)) for cid in center_ids]
    assert wins == [(0, 2), (0, 3), (3, 6)]
    ref = sp.pool({**case, "T": T_eff, "wins": np.array(wins)})
    ds = _Dataset(case, ids, T_pcd)
    got = points_api.tarl_features_per_map(ds, cd, T_pcd, ids, adjacent_frames=(2, 1), ctx=ctx)
    for name, reads in ds.reads.items():
        assert sorted(reads) == ids[:6], (name, reads)
    assert len(got) == 3 and sum(int(g.any(axis=1).sum()) for g in got) > 300
    for c, cid in enumerate(center_ids):
        i = ids.index(cid)
        tarl_indices = ids[max(0, i - 2):i + 1]                                            # chunk_generation.py:263-266
        one = points_api.tarl_features_per_patch(_Dataset(case, ids, T_pcd), cd["pcd_nonground_chunks_major_downsampling"][c], T_pcd,
                                                 case["centers"][c], tarl_indices, transform_pcd=camera_api.transform_points, ctx=ctx)
        assert np.all(np.abs(got[c] - ref[c]["mean"]) <= sp.bound(ref[c])) and np.all(np.abs(got[c] - one) <= sp.bound(ref[c])), c
    # tarl_norm: the per-chunk drop-in's lines on the same rows
    normed = points_api.tarl_features_per_map(_Dataset(case, ids, T_pcd), cd, T_pcd, ids, adjacent_frames=(2, 1), tarl_norm=True, ctx=ctx)
    for g, n in zip(got, normed):
        exp = g.copy()
        has = exp.any(axis=1)
        exp[has] /= np.linalg.norm(exp, axis=1)[has, None]
        assert np.array_equal(n, exp)


def test_map_level_last_row(ctx):
    """inv(T_pcd) @ pose with a last row within rounding of 0 0 0 1 is taken as affine; anything else is refused, not pooled."""
    from autoinst_amd import points_api
    case = sp.base_case(n_scans=3, per_scan=600, per_chunk=200, seed=6)
    ids = [0, 1, 2]
    cd = {"center_ids": [1], "center_positions": case["centers"][:1], "pcd_nonground_chunks_major_downsampling": case["chunks"][:1]}

    class Posed(_Dataset):
        def __init__(self, last_row):
            super().__init__(case, ids, np.eye(4))
            self.last_row = last_row

        def get_pose(self, i):
            T = super().get_pose(i).copy()
            T[3] = self.last_row
            return T
    exact = points_api.tarl_features_per_map(Posed([0.0, 0.0, 0.0, 1.0]), cd, np.eye(4), ids, ctx=ctx)
    near = points_api.tarl_features_per_map(Posed([1e-17, 0.0, -1e-17, 1.0 + 2.0 ** -52]), cd, np.eye(4), ids, ctx=ctx)
    assert np.array_equal(exact[0], near[0]) and exact[0].any()
    with pytest.raises(ValueError, match="not affine"):
        points_api.tarl_features_per_map(Posed([0.0, 0.0, 1e-3, 1.0]), cd, np.eye(4), ids, ctx=ctx)


def test_order_rule(base, ctx):
    """R4: a chunk alone, the chunk with only its window's scans, and the chunk in the full call are bit-identical; so are two
    calls, and host and device inputs."""
    import torch
    case = base["case"]
    full, cnt = _run(case, ctx)
    again, _ = _run(case, ctx)
    assert all(np.array_equal(a, b) for a, b in zip(full, again))
    for c in range(len(case["chunks"])):
        alone, n1 = _run(sp.sub_case(case, [c]), ctx)
        w0, w1 = case["wins"][c]
        window, n2 = _run(sp.sub_case(case, [c], range(w0, w1)), ctx)
        assert np.array_equal(alone[0], full[c]) and np.array_equal(window[0], full[c]), c
        assert np.array_equal(n1[0], cnt[c]) and np.array_equal(n2[0], cnt[c])
    dev = {"scans": [torch.from_numpy(s).cuda() for s in case["scans"]], "feats": [torch.from_numpy(f).cuda() for f in case["feats"]],
           "chunks": [torch.from_numpy(q).cuda() for q in case["chunks"]]}
    got, n = _run({**case, **dev}, ctx)
    assert all(g.is_cuda and g.dtype == torch.float64 for g in got) and all(k.is_cuda for k in n)
    assert all(np.array_equal(g.cpu().numpy(), f) for g, f in zip(got, full))
    assert all(np.array_equal(k.cpu().numpy(), f) for k, f in zip(n, cnt))
    # the concatenated form
    from autoinst_amd import points_api
    soff = np.concatenate([[0], np.cumsum([s.shape[0] for s in case["scans"]])])
    qoff = np.concatenate([[0], np.cumsum([q.shape[0] for q in case["chunks"]])])
    cat = points_api.tarl_pool_map(torch.cat(dev["scans"]), torch.cat(dev["feats"]), case["T"], torch.cat(dev["chunks"]), case["boxes"],
                                   case["wins"], scan_offsets=soff, chunk_offsets=qoff, ctx=ctx)
    assert all(np.array_equal(g.cpu().numpy(), f) for g, f in zip(cat, full))


HAND_MADE = {
    "radius_pairs_map": lambda: sp.case_radius_pairs(),
    "radius_pairs_near": lambda: sp.case_radius_pairs(origin=(25.0, -18.0, 1.0), seed=4, translation=(32.0, 0.0, 1.0)),
    "blas_one_ulp": sp.case_blas_one_ulp,
    "box_face": sp.case_box_face,
    "window_last": sp.case_window_last,
    "cell_borders": sp.case_cell_borders,
    "iz_rows_1": lambda: sp.case_iz_rows(1),
    "iz_rows_2": lambda: sp.case_iz_rows(2),
    "neighbours_only": sp.case_neighbours_only,
    "repeated": sp.case_repeated,
}


@pytest.mark.parametrize("name", sorted(HAND_MADE))
def test_hand_made(name, ctx):
    case = HAND_MADE[name]()
    ref = sp.pool(case)
    got, cnt = _run(case, ctx)
    _check(case, ref, got, cnt)
    if "expect" in case:
        assert np.array_equal(np.concatenate(cnt), case["expect"])


@pytest.mark.parametrize("dim", [40, 384])
def test_other_widths(dim, ctx):
    case = sp.base_case(dim=dim, per_scan=1200, per_chunk=400, seed=2)
    got, cnt = _run(case, ctx)
    _check(case, sp.pool(case), got, cnt)
    assert sum(int(n.sum()) for n in cnt) > 200


def test_empties(ctx):
    from autoinst_amd import points_api
    case = sp.base_case(per_scan=800, per_chunk=300, seed=3)
    edit = {**case, "scans": list(case["scans"]), "feats": list(case["feats"]), "chunks": list(case["chunks"]), "wins": case["wins"].copy()}
    edit["scans"][2], edit["feats"][2] = np.zeros((0, 3)), np.zeros((0, 96), np.float32)      # a scan with no points
    edit["chunks"][1] = np.zeros((0, 3))                                                        # a chunk with no queries
    edit["wins"][2] = [4, 4]                                                                    # an empty window
    got, cnt = _run(edit, ctx)
    _check(edit, sp.pool(edit), got, cnt)
    assert got[1].shape == (0, 96) and not got[2].any() and not cnt[2].any() and cnt[0].sum() > 0
    # M == 0: zero rows
    none = {**case, "scans": [np.zeros((0, 3))] * 6, "feats": [np.zeros((0, 96), np.float32)] * 6}
    got, cnt = _run(none, ctx)
    assert [g.shape for g in got] == [(c.shape[0], 96) for c in case["chunks"]] and not any(g.any() for g in got) and not any(n.any() for n in cnt)
    # no scans at all, and no chunks at all
    got = points_api.tarl_pool_map([], [], np.zeros((0, 4, 4)), case["chunks"], case["boxes"], np.zeros((3, 2), np.int32), ctx=ctx)
    assert [g.shape for g in got] == [(c.shape[0], 96) for c in case["chunks"]] and not any(g.any() for g in got)
    assert points_api.tarl_pool_map(case["scans"], case["feats"], case["T"], [], np.zeros((0, 6)), np.zeros((0, 2), np.int32), ctx=ctx) == []


def test_errors(ctx):
    """Every bad argument of R5 raises ValueError through _ffi.check, and the context stays usable."""
    from autoinst_amd import _ffi, points_api
    case = sp.base_case(per_scan=200, per_chunk=60, seed=5)

    def call(**over):
        a = {**case, **over}
        kw = {k: a[k] for k in ("scan_offsets", "chunk_offsets") if k in a}
        return points_api.tarl_pool_map(a["scans"], a["feats"], a["T"], a["chunks"], a["boxes"], a["wins"], radius=a["radius"], ctx=ctx, **kw)

    def edited(key, index, value):
        out = [np.array(x, copy=True) for x in case[key]] if isinstance(case[key], list) else np.array(case[key], copy=True)
        out[index] = value
        return out
    Tbad = edited("T", (3, 3, 1), 1e-9)
    soff = np.concatenate([[0], np.cumsum([s.shape[0] for s in case["scans"]])])
    qoff = np.concatenate([[0], np.cumsum([q.shape[0] for q in case["chunks"]])])
    soff_bad, qoff_bad = soff.copy(), qoff.copy()
    soff_bad[2], qoff_bad[1] = soff[3] + 1, qoff[2] + 1
    cat = {"scans": np.concatenate(case["scans"]), "feats": np.concatenate(case["feats"]), "chunks": np.concatenate(case["chunks"])}
    wide = [np.zeros((s.shape[0], 385), np.float32) for s in case["scans"]]
    bad = {
        "last row of T": dict(T=Tbad),
        "dim > 384": dict(feats=wide),
        "radius 0": dict(radius=0.0),
        "radius < 0": dict(radius=-1.0),
        "radius inf": dict(radius=np.inf),
        "radius nan": dict(radius=np.nan),
        "window past the scans": dict(wins=edited("wins", (1, 1), 7)),
        "window below 0": dict(wins=edited("wins", (0, 0), -1)),
        "window first > last": dict(wins=edited("wins", 2, [5, 4])),
        "scan_off not monotone": dict(**{**cat, "chunks": case["chunks"]}, scan_offsets=soff_bad),
        "query_off not monotone": dict(chunks=cat["chunks"], chunk_offsets=qoff_bad),
        "nan scan coordinate": dict(scans=edited("scans", 1, np.where(np.arange(200)[:, None] == 7, np.nan, case["scans"][1]))),
        "inf scan coordinate": dict(scans=edited("scans", 4, np.where(np.arange(200)[:, None] == 0, np.inf, case["scans"][4]))),
        "nan query coordinate": dict(chunks=edited("chunks", 0, np.where(np.arange(60)[:, None] == 59, np.nan, case["chunks"][0]))),
        "cell index beyond its field (box)": dict(boxes=edited("boxes", (0, 3), 1e12)),
        "cell index beyond its field (query)": dict(chunks=edited("chunks", 2, case["chunks"][2] + 1e12)),
        "nan scan coordinate and no query": dict(scans=edited("scans", 1, np.where(np.arange(200)[:, None] == 7, np.nan, case["scans"][1])),
                                                 chunks=[np.zeros((0, 3))] * 3),
    }
    good = call()
    for what, over in bad.items():
        with pytest.raises(ValueError, match="ai_scan_pool"):
            call(**over)
        assert _ffi.load().ai_last_error(), what
        again = call()                                              # the context is usable and computes the same
        assert all(np.array_equal(a, b) for a, b in zip(again, good)), what
    # dim < 1 cannot be said through arrays: the entry point itself
    one = np.zeros(2, np.int64)
    st = _ffi.load().ai_scan_pool(ctx._h, None, one.ctypes.data, 0, None, None, 0, None, one.ctypes.data, 0, None, None, 0.175,
                                  _ffi.AI_MEM_HOST, None, None)
    assert st == -1
    with pytest.raises(ValueError):
        _ffi.check(st, "ai_scan_pool")


def test_hand_over_to_run_chunks(base, ctx):
    """The device-tensor outputs go into run_chunks as they are and give the labels of the per-chunk path's features."""
    import torch
    from autoinst_amd import camera_api, ncuts_api, points_api, sharding
    case = base["case"]
    dev_chunks = [torch.from_numpy(q).cuda() for q in case["chunks"]]
    got = points_api.tarl_pool_map([torch.from_numpy(s).cuda() for s in case["scans"]], [torch.from_numpy(f).cuda() for f in case["feats"]],
                                   case["T"], dev_chunks, case["boxes"], case["wins"], ctx=ctx)
    g = ncuts_api.build_affinity(dev_chunks[0], got[0], alpha=1.0, theta=0.5, gamma=0.0, ctx=ctx)     # accepted as it is
    assert g.n == case["chunks"][0].shape[0]
    g.free()
    ds = _Dataset(case, list(range(len(case["scans"]))), np.eye(4))
    per_chunk = [points_api.tarl_features_per_patch(ds, _Cloud(case["chunks"][c]), np.eye(4), case["centers"][c],
                                                    list(range(*case["wins"][c])), transform_pcd=camera_api.transform_points, ctx=ctx)
                 for c in range(len(case["chunks"]))]
    cfg = dict(alpha=1.0, theta=0.5, gamma=0.0, T=0.03)
    lab_map = sharding.run_chunks(list(zip(dev_chunks, got)), **cfg)
    lab_one = sharding.run_chunks(list(zip(case["chunks"], per_chunk)), **cfg)
    for a, b in zip(lab_map, lab_one):
        assert np.array_equal(np.asarray(a), np.asarray(b)) and np.unique(np.asarray(a)).size > 1
