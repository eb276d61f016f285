"""GPU suite: ``ai_chunk_finish`` (csrc/ai_finish.hip, `points_api.finish_chunks` / `finish_map`) -- the tail of ``ncuts_chunk`` for
all chunks of a map in one call -- against the NumPy restatement tests/finish_ref.py (rules F1-F6), against the single-cloud
entries it batches (``ai_nn1_project``, ``ai_statistical_inliers``: bit-equal, F2 / F3), and against itself (F7).

Tolerances: indices, labels, offsets, distances and copied coordinates are equal bit for bit; the per-point kNN averages and the
threshold agree with the restatement to rel 1e-12 (test_gpu_prep.py's tolerance: cKDTree forms the distances in another order).
The conditions under which equal index sets follow are asserted on the restatement: no fine point with two equidistant nearest
majors, no avg within 1e-12 x threshold of the threshold.  mean_z and z_limit are EQUAL to the restatement's: it sums z over the
inliers in F4's order (`finish_ref.f4_sum`), and with equal inlier sets that order fixes the bits, so no inlier's z needs a
margin around the limit."""
import ctypes as C

import numpy as np
import pytest

import finish_ref
from autoinst_amd import _ffi, points_api, prep_api

pytestmark = pytest.mark.gpu

WORKERS = 16
STATS = points_api.FINISH_STATS
OUTPUTS = ("fine_nn", "fine_dist", "fine_label", "ground_avg", "ground_keep", "keep_off", "ground_stats", "merged")


def _offsets(parts):
    off = np.zeros(len(parts) + 1, dtype=np.int64)
    np.cumsum([int(np.asarray(a).reshape(-1, 3).shape[0]) for a in parts], out=off[1:])
    return off


def _cat(parts, width, dtype):
    parts = [np.asarray(a, dtype=dtype).reshape((-1, width) if width else -1) for a in parts]
    return np.ascontiguousarray(np.concatenate(parts)) if parts else np.zeros((0, width) if width else 0, dtype=dtype)


def c_finish(ctx, fine, major, labels, ground, *, nb=20, std_ratio=2.0, mean_height=0.6, device=False, skip=(), offsets=None,
             only_merged=None, fill=None):
    """The C entry as it is: lists of per-chunk arrays in, (status, dict of host arrays) out.  ``skip``: outputs passed as NULL;
    ``labels=None``: major_label NULL; ``offsets``: (fine_off, major_off, ground_off) instead of the lists' own;
    ``only_merged``: the members of the merged trio that are given; ``fill``: what the outputs hold before the call."""
    n = len(ground)
    f, m, g = _cat(fine, 3, np.float64), _cat(major, 3, np.float64), _cat(ground, 3, np.float64)
    foff, moff, goff = offsets if offsets is not None else (_offsets(fine), _offsets(major), _offsets(ground))
    foff, moff, goff = (np.ascontiguousarray(o, dtype=np.int64) for o in (foff, moff, goff))
    lab = _cat(labels, 0, np.int32) if labels is not None else None
    nf, ng = f.shape[0], g.shape[0]
    out = {"fine_nn": np.zeros(max(nf, 1), np.int32), "fine_dist": np.zeros(max(nf, 1)), "fine_label": np.zeros(max(nf, 1), np.int32),
           "ground_avg": np.zeros(max(ng, 1)), "ground_keep": np.zeros(max(ng, 1), np.int32),
           "merged_xyz": np.zeros((max(nf + ng, 1), 3)), "merged_label": np.zeros(max(nf + ng, 1), np.int32)}
    host = {"keep_off": np.zeros(n + 1, np.int64), "ground_stats": np.zeros((max(n, 1), 6)), "merged_off": np.zeros(n + 1, np.int64)}
    if fill is not None:
        for a in list(out.values()) + list(host.values()):
            a[...] = fill
    given = set(OUTPUTS) - set(skip)
    if labels is None:
        given -= {"fine_label", "merged"}
    trio = ("merged_xyz", "merged_label", "merged_off")
    want = {k: k in given for k in out if k not in trio}
    want.update({k: k in given for k in ("keep_off", "ground_stats")})
    want.update({k: ("merged" in given) if only_merged is None else (k in only_merged) for k in trio})
    if device:
        import torch
        dev = torch.device("cuda", ctx.device)
        keepalive = [torch.as_tensor(a, device=dev) for a in (f, m, g)] + [torch.as_tensor(lab, device=dev) if lab is not None else None]
        dout = {k: torch.as_tensor(v, device=dev) for k, v in out.items()}
        torch.cuda.synchronize()

        def ptr(a):
            return C.c_void_p(a.data_ptr()) if a is not None and a.numel() else None

        def optr(k):
            return C.c_void_p(dout[k].data_ptr()) if want[k] else None
        mem = _ffi.AI_MEM_DEVICE
    else:
        keepalive = [f, m, g, lab]

        def ptr(a):
            return a.ctypes.data if a is not None and a.size else None

        def optr(k):
            return out[k].ctypes.data if want[k] else None
        mem = _ffi.AI_MEM_HOST

    def hptr(k):
        return host[k].ctypes.data if want[k] else None
    dummy = np.zeros(1, np.int32)
    lab_ptr = None if lab is None else (ptr(keepalive[3]) or dummy.ctypes.data)
    status = _ffi.load().ai_chunk_finish(
        ctx._h, ptr(keepalive[0]), foff.ctypes.data, ptr(keepalive[1]), moff.ctypes.data, lab_ptr, ptr(keepalive[2]), goff.ctypes.data,
        n, nb, float(std_ratio), float(mean_height), mem, optr("fine_nn"), optr("fine_dist"), optr("fine_label"), optr("ground_avg"),
        optr("ground_keep"), hptr("keep_off"), hptr("ground_stats"), optr("merged_xyz"), optr("merged_label"), hptr("merged_off"))
    if device:
        import torch
        torch.cuda.synchronize()
        out = {k: v.cpu().numpy() for k, v in dout.items()}
    res = {"status": status, "error": _ffi.load().ai_last_error().decode() if status else "", "raw": {**out, **host}}
    if status or fill is not None:
        return res
    n_keep = int(host["keep_off"][n]) if want["keep_off"] else (int(host["merged_off"][n]) - nf if want["merged_off"] else None)
    for k in ("fine_nn", "fine_dist", "fine_label"):
        if want[k]:
            res[k] = out[k][:nf]
    if want["ground_avg"]:
        res["ground_avg"] = out["ground_avg"][:ng]
    if want["ground_keep"] and n_keep is not None:
        res["ground_keep"] = out["ground_keep"][:n_keep]
    if want["keep_off"]:
        res["keep_off"] = host["keep_off"]
    if want["ground_stats"]:
        res["ground_stats"] = host["ground_stats"][:n]
    if want["merged_off"]:
        res["merged_off"] = host["merged_off"]
        res["merged_xyz"] = out["merged_xyz"][:nf + n_keep]
        res["merged_label"] = out["merged_label"][:nf + n_keep]
    return res


def same_bytes(a, b, keys=None, tag=""):
    for k in keys or [k for k in a if k not in ("status", "error", "raw")]:
        assert np.ascontiguousarray(a[k]).tobytes() == np.ascontiguousarray(b[k]).tobytes(), f"{tag} {k}"


def chunk_slice(res, offs, c):
    """Chunk c's part of a batched result, in the shape of a one-chunk result."""
    foff, goff = offs
    out = {}
    for k in ("fine_nn", "fine_dist", "fine_label"):
        out[k] = res[k][foff[c]:foff[c + 1]]
    out["ground_avg"] = res["ground_avg"][goff[c]:goff[c + 1]]
    ko, mo = res["keep_off"], res["merged_off"]
    out["ground_keep"] = res["ground_keep"][ko[c]:ko[c + 1]]
    out["ground_stats"] = res["ground_stats"][c:c + 1]
    out["merged_xyz"] = res["merged_xyz"][mo[c]:mo[c + 1]]
    out["merged_label"] = res["merged_label"][mo[c]:mo[c + 1]]
    out["keep_off"] = np.array([0, ko[c + 1] - ko[c]], np.int64)
    out["merged_off"] = np.array([0, mo[c + 1] - mo[c]], np.int64)
    return out


def check_against_restatement(res, ref, fine, ground, tag=""):
    """`res`: the batched result; `ref`: finish_ref.finish_chunks' list.  The conditions of the module docstring are asserted."""
    foff, goff = _offsets(fine), _offsets(ground)
    for c, r in enumerate(ref):
        t = f"{tag} chunk {c}"
        got = chunk_slice(res, (foff, goff), c)
        st = dict(zip(STATS, got["ground_stats"][0]))
        n = r["inliers"].size
        tied = int((r["fine_tied"] > 0).sum())
        near_thr = int(((r["avg"] > 0) & (np.abs(r["avg"] - r["threshold"]) <= 1e-12 * abs(r["threshold"]))).sum()) if r["avg"].size > 1 else 0
        print(f"{t}: nf={r['fine_nn'].size} ng={r['avg'].size} inliers={n} kept={r['keep'].size} tied={tied} near_thr={near_thr} "
              f"mean_z={st['mean_z']!r} (ref {r['mean_z']!r}) thr={st['threshold']!r} (ref {r['threshold']!r})")
        assert tied == 0 and near_thr == 0, t
        np.testing.assert_array_equal(got["fine_nn"], r["fine_nn"], err_msg=t)
        np.testing.assert_array_equal(got["fine_label"], r["fine_label"], err_msg=t)
        assert got["fine_dist"].tobytes() == r["fine_dist"].tobytes(), t
        np.testing.assert_allclose(got["ground_avg"], r["avg"], rtol=1e-12, atol=0.0, err_msg=t)
        if r["avg"].size > 1:
            assert abs(st["threshold"] - r["threshold"]) <= 1e-12 * abs(r["threshold"]), t
        assert st["n_inliers"] == n, t
        if n:
            assert st["mean_z"] == r["mean_z"] and st["z_limit"] == r["z_limit"], (t, st["mean_z"], r["mean_z"])
        else:
            assert np.isnan(st["mean_z"]) and np.isnan(st["z_limit"]), t
        np.testing.assert_array_equal(got["ground_keep"], r["keep"], err_msg=t)
        assert got["merged_xyz"].tobytes() == r["merged_points"].tobytes(), t
        np.testing.assert_array_equal(got["merged_label"], r["merged_label"], err_msg=t)
    np.testing.assert_array_equal(res["keep_off"], np.concatenate([[0], np.cumsum([r["keep"].size for r in ref])]))
    np.testing.assert_array_equal(res["merged_off"], foff + res["keep_off"])


@pytest.fixture(scope="module")
def street():
    m, d = finish_ref.street_fixture(workers=WORKERS)
    fine, major, ground = d["pcd_nonground_chunks"], d["pcd_nonground_chunks_major_downsampling"], d["pcd_ground_chunks"]
    labels = [np.arange(a.shape[0], dtype=np.int32) for a in major]
    ref = finish_ref.finish_chunks(fine, major, labels, ground, workers=WORKERS)
    return {"map": m, "dict": d, "fine": fine, "major": major, "ground": ground, "labels": labels, "ref": ref}


@pytest.fixture(scope="module")
def street_gpu(street, ctx):
    return c_finish(ctx, street["fine"], street["major"], street["labels"], street["ground"])


def test_street_against_the_restatement(street, street_gpu):
    assert street_gpu["status"] == 0
    assert [a.shape[0] for a in street["fine"]] == [45570, 52704, 33195]
    assert [a.shape[0] for a in street["major"]] == [4052, 4600, 3593] and [a.shape[0] for a in street["ground"]] == [38789, 38832, 28660]
    check_against_restatement(street_gpu, street["ref"], street["fine"], street["ground"], "street")
    for r in street["ref"]:   # the kerb: some 7 % of the inliers are cut by height, and the outlier filter removed points before
        assert 0.05 < 1.0 - r["keep"].size / r["n_inliers"] < 0.10 and r["n_inliers"] < r["avg"].size


def test_bit_equal_to_the_single_cloud_entries(street, street_gpu, ctx):
    """F2 / F3: per chunk, `nn1_index` and `statistical_inlier_indices` on the chunk alone."""
    foff, goff = _offsets(street["fine"]), _offsets(street["ground"])
    for c in range(3):
        got = chunk_slice(street_gpu, (foff, goff), c)
        idx, dist = points_api.nn1_index(street["fine"][c], street["major"][c], ctx=ctx)
        np.testing.assert_array_equal(got["fine_nn"], idx)
        assert got["fine_dist"].tobytes() == dist.tobytes()
        inl, avg, st = prep_api.statistical_inlier_indices(street["ground"][c], 20, 2.0, return_stats=True, ctx=ctx)
        assert got["ground_avg"].tobytes() == avg.tobytes()
        assert got["ground_stats"][0, :3].tobytes() == np.array([st["mean"], st["std"], st["threshold"]]).tobytes()
        assert got["ground_stats"][0, 3] == inl.size
        assert np.isin(got["ground_keep"], inl).all()


def test_independence(street, street_gpu, ctx):
    """F7: each chunk alone, all together, reversed; host and device memory; every optional output NULL in turn; twice."""
    S = street
    foff, goff = _offsets(S["fine"]), _offsets(S["ground"])
    same_bytes(c_finish(ctx, S["fine"], S["major"], S["labels"], S["ground"]), street_gpu, tag="twice")
    same_bytes(c_finish(ctx, S["fine"], S["major"], S["labels"], S["ground"], device=True), street_gpu, tag="device")
    rev = c_finish(ctx, S["fine"][::-1], S["major"][::-1], S["labels"][::-1], S["ground"][::-1], device=True)
    rfoff, rgoff = _offsets(S["fine"][::-1]), _offsets(S["ground"][::-1])
    for c in range(3):
        part = chunk_slice(street_gpu, (foff, goff), c)
        alone = c_finish(ctx, [S["fine"][c]], [S["major"][c]], [S["labels"][c]], [S["ground"][c]])
        same_bytes(alone, part, tag=f"alone {c}")
        same_bytes(chunk_slice(rev, (rfoff, rgoff), 2 - c), part, tag=f"reversed {c}")
    for out in OUTPUTS:
        res = c_finish(ctx, S["fine"], S["major"], S["labels"], S["ground"], skip=(out,), device=(out in ("fine_nn", "ground_avg")))
        assert res["status"] == 0, out
        keys = [k for k in res if k not in ("status", "error", "raw")]
        assert keys and not any(k.startswith(out) for k in keys), out
        same_bytes(res, street_gpu, keys, tag=f"without {out}")
    res = c_finish(ctx, S["fine"], S["major"], None, S["ground"])          # no labels: the searches and the ground remain
    same_bytes(res, street_gpu, ["fine_nn", "fine_dist", "ground_avg", "ground_keep", "keep_off", "ground_stats"], tag="no labels")


def test_hand_cases_segmentation_and_ties(ctx):
    rng = np.random.default_rng(13)
    fine = np.round(rng.random((700, 3)) * 4.0 * 1024) / 1024
    major0 = np.round(rng.random((90, 3)) * 4.0 * 1024) / 1024
    major = [major0, major0 + [0.2, 0.0, 0.0]]          # F1: the same fine points, majors 0.2 m apart, as overlapping chunks have
    labels = [np.arange(90, dtype=np.int32), np.arange(90, dtype=np.int32) + 100]
    empty = np.zeros((0, 3))
    res = c_finish(ctx, [fine, fine], major, labels, [empty, empty])
    ref = finish_ref.finish_chunks([fine, fine], major, labels, [empty, empty], brute=True)
    check_against_restatement(res, ref, [fine, fine], [empty, empty], "shifted majors")
    a, b = res["fine_nn"][:700], res["fine_nn"][700:]
    assert (a != b).any() and (res["fine_label"][:700] < 100).all() and (res["fine_label"][700:] >= 100).all()
    wrong = finish_ref.finish_chunks([fine, fine], major, labels, [empty, empty], brute=True, variant="neighbour_chunk")
    assert (wrong[0]["fine_label"] != res["fine_label"][:700]).any()
    # exact midpoints of two (or four) majors on dyadic coordinates: the smaller index
    maj = np.array([[0.0, 0, 0], [2.0, 0, 0], [0.0, 2.0, 0], [2.0, 2.0, 0], [1.0, 1.0, 4.0], [0.0, 0.0, 0.0]]) + [3.0, -5.0, 0.5]
    fin = np.array([[1.0, 0, 0], [0.0, 1.0, 0], [1.0, 1.0, 0], [1.0, 2.0, 0], [1.75, 0.25, 0.0], [2.0, 1.0, 0.0]]) + [3.0, -5.0, 0.5]
    res = c_finish(ctx, [fin], [maj], [np.arange(6, dtype=np.int32) * 7], [empty])
    r = finish_ref.finish_chunk(fin, maj, np.arange(6) * 7, empty, brute=True)
    assert (r["fine_tied"] > 0).sum() == 5
    np.testing.assert_array_equal(res["fine_nn"], [0, 0, 0, 2, 1, 1])
    np.testing.assert_array_equal(res["fine_nn"], r["fine_nn"])
    np.testing.assert_array_equal(res["fine_label"], r["fine_label"])
    assert res["fine_dist"].tobytes() == r["fine_dist"].tobytes()
    np.testing.assert_array_equal(res["merged_label"], res["fine_label"] + 1)


def test_hand_cases_ground(ctx):
    empty = np.zeros((0, 3))
    # 41 copies of one point: avg == 0 for k = 20, so they are no inliers and not in mean_z (their z would move it)
    rng = np.random.default_rng(20)
    p = rng.random((3000, 3)) * [6.0, 6.0, 0.05]
    p[:41] = [3.0, 3.0, 40.0]
    res = c_finish(ctx, [empty], [empty], [np.zeros(0, np.int32)], [p])
    ref = finish_ref.finish_chunks([empty], [empty], [np.zeros(0, np.int32)], [p])
    check_against_restatement(res, ref, [empty], [p], "copies")
    assert (res["ground_avg"][:41] == 0).all() and not np.isin(np.arange(41), res["ground_keep"]).any()
    assert res["ground_stats"][0, 4] < 0.05
    # z on multiples of 2^-10 and mean_height = 0.5: every order of summation is exact
    xx, yy = np.meshgrid(np.arange(48.0), np.arange(48.0), indexing="ij")
    g = np.stack([xx.ravel() * 0.25, yy.ravel() * 0.25, np.round(rng.random(xx.size) * 64) / 1024], 1)
    r0 = finish_ref.corrected_ground(g, 20, 100.0, 0.5)
    assert r0["n_inliers"] == g.shape[0]                     # std_ratio 100: every point is an inlier
    lim = r0["z_limit"]
    assert lim == np.mean(g[:, 2]) + 0.5
    # mean_z equals NumPy's bit for bit
    res = c_finish(ctx, [empty], [empty], [np.zeros(0, np.int32)], [g], std_ratio=100.0, mean_height=0.5)
    st = dict(zip(STATS, res["ground_stats"][0]))
    assert st["mean_z"] == np.mean(g[:, 2]) == finish_ref.corrected_ground(g, 20, 100.0, 0.5)["mean_z"] and st["z_limit"] == lim
    assert res["ground_keep"].size == g.shape[0]


def test_dyadic_limit_is_strict(ctx):
    """A point at exactly z_limit is dropped, the next double below is kept: z in {0, 2^-3} on a grid, mean_z = 2^-4 exactly,
    mean_height = 2^-4, so half of the points sit ON the limit 2^-3; then one of them is lowered by one ulp (which leaves the
    float64 sum, hence the limit, where it was: 2^-56 is below half an ulp of 16)."""
    xx, yy = np.meshgrid(np.arange(16.0), np.arange(16.0), indexing="ij")
    g = np.stack([xx.ravel(), yy.ravel(), ((xx + yy) % 2).ravel() * 0.125], 1)
    g[16, 2] = np.nextafter(0.125, 0.0)
    empty = np.zeros((0, 3))
    res = c_finish(ctx, [empty], [empty], [np.zeros(0, np.int32)], [g], std_ratio=100.0, mean_height=0.0625)
    st = dict(zip(STATS, res["ground_stats"][0]))
    r = finish_ref.corrected_ground(g, 20, 100.0, 0.0625)
    assert st["n_inliers"] == 256 and st["mean_z"] == r["mean_z"] == np.mean(g[:, 2]) and st["z_limit"] == 0.125
    np.testing.assert_array_equal(res["ground_keep"], r["keep"])
    np.testing.assert_array_equal(res["ground_keep"], np.flatnonzero(g[:, 2] < 0.125))
    assert 16 in res["ground_keep"] and res["ground_keep"].size == 129 and 1 not in res["ground_keep"]


def test_reduction_and_size_boundaries(ctx):
    """One call with ground chunks of 70 001 points (above 256 x 256: a second trip per thread of a partial block), 12 (k = n),
    1 and 0 points, beside chunks with and without fine points; and n_chunks == 0."""
    rng = np.random.default_rng(31)

    def plane(n):
        p = rng.random((n, 3)) * [np.sqrt(n) * 0.1, np.sqrt(n) * 0.1, 0.04]
        p[: n // 10, 2] += 0.9
        return p[rng.permutation(n)]
    ground = [plane(70_001), plane(12), np.array([[1.0, 2.0, 3.0]]), np.zeros((0, 3)), plane(300)]
    major = [rng.random((50, 3)) * 5.0, np.zeros((0, 3)), rng.random((3, 3)), rng.random((1, 3)), np.zeros((0, 3))]
    fine = [rng.random((600, 3)) * 5.0, np.zeros((0, 3)), rng.random((257, 3)), np.zeros((0, 3)), np.zeros((0, 3))]
    labels = [np.arange(m.shape[0], dtype=np.int32)[::-1].copy() for m in major]
    res = c_finish(ctx, fine, major, labels, ground)
    assert res["status"] == 0, res["error"]
    ref = finish_ref.finish_chunks(fine, major, labels, ground, workers=WORKERS)
    check_against_restatement(res, ref, fine, ground, "sizes")
    st = res["ground_stats"]
    assert st[0, 3] > 60_000 and res["keep_off"][1] > 50_000
    assert res["ground_avg"][70_013] == 0.0 and st[2, 0] == 0.0 and np.isnan(st[2, 1:3]).all() and st[2, 3] == 0    # one point
    assert np.isnan(st[3]).sum() == 5 and st[3, 3] == 0                                                            # no ground
    foff, goff = _offsets(fine), _offsets(ground)
    for c in (0, 1, 4):     # bit-equal to the single entry at each size
        inl, avg, s1 = prep_api.statistical_inlier_indices(ground[c], 20, 2.0, return_stats=True, ctx=ctx)
        assert res["ground_avg"][goff[c]:goff[c + 1]].tobytes() == avg.tobytes()
        assert st[c, :3].tobytes() == np.array([s1["mean"], s1["std"], s1["threshold"]]).tobytes() and st[c, 3] == inl.size
    for c in range(5):
        alone = c_finish(ctx, [fine[c]], [major[c]], [labels[c]], [ground[c]], device=(c % 2 == 0))
        same_bytes(alone, chunk_slice(res, (foff, goff), c), tag=f"alone {c}")
    none = c_finish(ctx, [], [], [], [])
    assert none["status"] == 0 and none["keep_off"].tolist() == [0] and none["merged_off"].tolist() == [0]
    assert points_api.finish_chunks([], [], [], [], ctx=ctx) == []


def test_errors(ctx):
    rng = np.random.default_rng(41)
    fine, major, ground = [rng.random((40, 3))], [rng.random((9, 3))], [rng.random((100, 3))]
    labels = [np.arange(9, dtype=np.int32)]
    ok = (_offsets(fine), _offsets(major), _offsets(ground))

    def bad(a, where=(3, 1), value=np.nan):
        b = [a[0].copy()]
        b[0][where] = value
        return b
    cases = [
        (dict(offsets=(np.array([1, 40]), ok[1], ok[2])), "fine_off must start at 0"),
        (dict(offsets=(ok[0], np.array([2, 9]), ok[2])), "major_off must start at 0"),
        (dict(offsets=(ok[0], ok[1], np.array([0, -1]))), "ground_off decreases"),
        (dict(fine=bad(fine)), "fine coordinates of chunk 0 are not finite"),
        (dict(major=bad(major, value=np.inf)), "major coordinates of chunk 0 are not finite"),
        (dict(ground=bad(ground, value=-np.inf)), "ground coordinates of chunk 0 are not finite"),
        (dict(major=[np.zeros((0, 3))], labels=[np.zeros(0, np.int32)]), "fine points and no major points"),
        (dict(nb=0), "nb_neighbors must be >= 1"),
        (dict(std_ratio=0.0), "std_ratio > 0"),
        (dict(std_ratio=-1.0), "std_ratio > 0"),
        (dict(nb=65), "nb_neighbors > 64"),
        (dict(mean_height=np.nan), "mean_height is not finite"),
        (dict(mean_height=np.inf), "mean_height is not finite"),
        (dict(labels=None, skip=()), None),                       # not an error: fine_label and the trio are NULL with it
        (dict(only_merged=("merged_xyz", "merged_off")), "all NULL or all given"),
        (dict(only_merged=("merged_label",)), "all NULL or all given"),
    ]
    for kw, text in cases:
        args = dict(fine=fine, major=major, labels=labels, ground=ground, fill=77)
        args.update(kw)
        res = c_finish(ctx, args.pop("fine"), args.pop("major"), args.pop("labels"), args.pop("ground"), **args)
        if text is None:
            assert res["status"] == 0
            continue
        assert res["status"] == -1 and text in res["error"], (kw, res["error"])
        for k, a in res["raw"].items():     # checked in full before any output is written
            assert (a == 77).all(), (kw, k)
    # the NULL combinations that need major_label == NULL with an output that depends on it
    lib, h = _ffi.load(), ctx._h
    f, m, g = fine[0], major[0], ground[0]
    out_i, out_d, off = np.zeros(200, np.int32), np.zeros((200, 3)), np.zeros(2, np.int64)
    base = [h, f.ctypes.data, ok[0].ctypes.data, m.ctypes.data, ok[1].ctypes.data, None, g.ctypes.data, ok[2].ctypes.data, 1, 20, 2.0, 0.6, 0]
    assert lib.ai_chunk_finish(*base, None, None, out_i.ctypes.data, None, None, None, None, None, None, None) == -1
    assert "fine_label needs major_label" in lib.ai_last_error().decode()
    assert lib.ai_chunk_finish(*base, None, None, None, None, None, None, None, out_d.ctypes.data, out_i.ctypes.data, off.ctypes.data) == -1
    assert "merged outputs need major_label" in lib.ai_last_error().decode()
    assert lib.ai_chunk_finish(*base[:8], 65536, *base[9:], *([None] * 10)) == -1
    # nb_neighbors > 64 is fine while no chunk has more than 64 ground points (k = n)
    assert c_finish(ctx, fine, major, labels, [ground[0][:64]], nb=100)["status"] == 0
    # the same through points_api: ValueError
    f_ = points_api.finish_chunks
    for kw in (dict(nb_neighbors=0), dict(std_ratio=0.0), dict(nb_neighbors=65), dict(mean_height=float("nan"))):
        with pytest.raises(ValueError):
            f_(fine, major, labels, ground, ctx=ctx, **kw)
    for args in ((bad(fine), major, labels, ground), (fine, bad(major), labels, ground), (fine, major, labels, bad(ground)),
                 (fine, [np.zeros((0, 3))], [np.zeros(0, np.int32)], ground), (fine, major, [np.arange(8)], ground),
                 (fine, major, labels, ground + ground)):
        with pytest.raises(ValueError):
            f_(*args, ctx=ctx)


def test_hand_over_from_the_cut_to_the_merge(street, ctx):
    """prep_api.chunk_and_downsample_point_clouds -> run_chunks (spatial) -> finish_map -> merge_chunks_unite_instances2 on
    device tensors, without open3d."""
    import torch
    from autoinst_amd import labels_api, sharding
    from autoinst_amd.config import CONFIG_SPATIAL

    m = street["map"]
    dev = torch.device("cuda", ctx.device)
    kl = {k: torch.as_tensor(v, device=dev) for k, v in m["labels"].items()}
    d = prep_api.chunk_and_downsample_point_clouds(torch.as_tensor(m["nonground"], device=dev), torch.as_tensor(m["ground"], device=dev),
                                                   m["T_pcd"], m["positions"], m["first_position"], m["indices"], kl, ctx=ctx)
    major = d["pcd_nonground_chunks_major_downsampling"]
    groups = sharding.run_chunks([(p, None) for p in major], alpha=CONFIG_SPATIAL["alpha"], theta=0.0, gamma=0.0, T=CONFIG_SPATIAL["T"])
    chunks, pairs = points_api.finish_map(d, groups, ctx=ctx)
    assert len(chunks) == len(pairs) == 3
    ref_kl = street["dict"]["kitti_labels"]["ground"]
    for c, (out, (pts, col)) in enumerate(zip(chunks, pairs)):
        r = street["ref"][c]              # the street's restatement ran with labels = arange: its fine_label is the nearest major
        assert out["merged_chunk"].is_cuda and out["ground_keep"].dtype == torch.int64
        assert len(np.unique(np.asarray(groups[c]))) > 1
        np.testing.assert_array_equal(out["fine_instance"].cpu().numpy(), np.asarray(groups[c])[r["fine_nn"]])
        nf = street["fine"][c].shape[0]
        np.testing.assert_array_equal(out["merged_instance"].cpu().numpy()[:nf], np.asarray(groups[c])[r["fine_nn"]] + 1)
        assert not out["merged_instance"].cpu().numpy()[nf:].any()
        assert out["merged_chunk"].cpu().numpy().tobytes() == np.concatenate([street["fine"][c], street["ground"][c][r["keep"]]]).tobytes()
        assert out["pcd_chunk"].cpu().numpy().tobytes() == street["fine"][c].tobytes()
        assert out["cut_hight"].cpu().numpy().tobytes() == street["ground"][c][r["keep"]].tobytes()
        np.testing.assert_array_equal(out["ground_keep"].cpu().numpy(), r["keep"])
        np.testing.assert_array_equal(out["inst_ground"].cpu().numpy(), ref_kl["instance"][c][r["keep"]])
        np.testing.assert_array_equal(out["seg_ground"].cpu().numpy(), ref_kl["semantic"][c][r["keep"]])
        assert pts.tobytes() == out["merged_chunk"].cpu().numpy().tobytes() and col.shape == pts.shape
        assert (col[nf:] == 0).all() and (col[:nf].sum(axis=1) > 0).all()
    mp, mc = labels_api.merge_chunks_unite_instances2(pairs, ctx=ctx)
    uniq = np.unique(np.concatenate([p for p, _ in pairs]), axis=0)
    assert mp.shape == mc.shape == uniq.shape            # one label per unique point
    assert np.unique(mp, axis=0).shape == uniq.shape
    # get_corrected_ground: the one-chunk call with no fine points
    pcd, inst = points_api.get_corrected_ground(d, 1, ctx=ctx)
    r = street["ref"][1]
    assert pcd.cpu().numpy().tobytes() == np.concatenate([street["fine"][1], street["ground"][1][r["keep"]]]).tobytes()
    np.testing.assert_array_equal(inst.cpu().numpy(), ref_kl["instance"][1][r["keep"]])
