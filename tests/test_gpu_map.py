"""GPU suite: the minor-voxel map on the device (prep_api.voxel_down_sample_nearest / downsample_map, csrc/ai_prep.hip) against
the CPU restatement tests/map_ref.py on a raw-density street (synth.street_map(24, step=0.02): 1.25 M non-ground and 0.96 M
ground points, 5.4 and 4.0 per minor voxel) and on the hand-made clouds of map_ref.edge_cases.

Every comparison is an equality: the means, the trace, the nearest raw index and its distance are all defined bit for bit."""
import ctypes as C

import numpy as np
import pytest
from scipy.spatial import cKDTree

import map_ref
import prep_ref
from autoinst_amd import _ffi, points_api, prep_api, synth
from test_gpu_prep import _compare_dict

pytestmark = pytest.mark.gpu

WORKERS = 16
CLOUDS = ("nonground", "ground")


@pytest.fixture(scope="module")
def street():
    m = synth.street_map(24.0, seed=0, step=0.02)
    assert m["nonground"].shape[0] == 1_252_624 and m["ground"].shape[0] == 961_144
    return m


@pytest.fixture(scope="module")
def oracle(street):
    g, ng, kitti, nearest = map_ref.downsample_map(street["nonground"], street["ground"], street["labels"], workers=WORKERS)
    return {"ground": g, "nonground": ng, "kitti": kitti, "nearest": nearest,
            "trace": {c: prep_ref.voxel_down_sample(street[c], 0.05)[1] for c in CLOUDS}}


@pytest.fixture(scope="module")
def device(street, ctx):
    return {c: prep_api.voxel_down_sample_nearest(street[c], 0.05, return_trace=True, return_dist=True, ctx=ctx) for c in CLOUDS}


def test_the_fixture_discriminates(street, oracle):
    """Counted on the restatement: voxels whose nearest raw point lies in a neighbouring voxel, centroids with an exact distance
    tie, and voxels whose transferred instance label differs from their first member's."""
    for cloud in CLOUDS:
        p, out = street[cloud], oracle[cloud]
        idx, _ = oracle["nearest"][cloud]
        trace = oracle["trace"][cloud]
        elsewhere = int(np.sum(trace[idx] != np.arange(out.shape[0])))
        _, i2 = cKDTree(p).query(out, k=2, workers=WORKERS)
        d2 = map_ref.sq_dist(out[:, None, :], p[i2])
        tied = int(np.sum(d2[:, 0] == d2[:, 1]))
        first = np.full(out.shape[0], p.shape[0], np.int64)
        np.minimum.at(first, trace, np.arange(p.shape[0]))
        inst = street["labels"][f"instance_{cloud}"]
        relabelled = int(np.sum(inst[idx] != inst[first]))
        print(f"{cloud}: {p.shape[0]} points, {out.shape[0]} voxels, nearest in a neighbouring voxel: {elsewhere}, tied: {tied}, "
              f"instance label differs from the first member's: {relabelled}")
        assert elsewhere > 0 and tied > 0
        if cloud == "nonground":
            assert relabelled > 0


def test_means_and_trace_are_voxel_down_samples(street, device, ctx):
    for cloud in CLOUDS:
        ref, rtr = prep_api.voxel_down_sample(street[cloud], 0.05, return_trace=True, ctx=ctx)
        out, _, tr, _ = device[cloud]
        assert out.shape == ref.shape and out.shape[0] > 200_000
        assert out.tobytes() == ref.tobytes(), cloud
        assert tr.dtype == np.int32 and tr.tobytes() == rtr.tobytes(), cloud


def test_nearest_point_equals_the_restatement(street, oracle, device):
    for cloud in CLOUDS:
        idx, dist = oracle["nearest"][cloud]
        map_ref.check_nearest(cloud, device[cloud], (oracle[cloud], idx, oracle["trace"][cloud], dist))


def test_nearest_point_equals_nn1_index(street, device, ctx):
    """The same rule by an independent kernel (ai_nn1_project's ring search over a 0.5 m cell list)."""
    for cloud in CLOUDS:
        out, idx, _, dist = device[cloud]
        sub = np.random.default_rng(1).choice(out.shape[0], 200_000, replace=False)
        i2, d2 = points_api.nn1_index(out[sub], street[cloud], ctx=ctx)
        np.testing.assert_array_equal(idx[sub], i2)
        assert dist[sub].tobytes() == d2.tobytes()


def test_downsample_map_feeds_the_chunk_preparation(street, oracle, ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    got = prep_api.downsample_map(street["nonground"], street["ground"], street["labels"], ctx=ctx)
    assert got[0].tobytes() == oracle["ground"].tobytes() and got[1].tobytes() == oracle["nonground"].tobytes()
    for k in map_ref.LABEL_KEYS:
        assert got[2][k].dtype == street["labels"][k].dtype and got[2][k].ndim == 1
        np.testing.assert_array_equal(got[2][k], oracle["kitti"][k], err_msg=k)
    # (n, 1) columns of another dtype, on the device, clouds resident: nothing comes back to the host
    labels_d = {k: torch.as_tensor(v.astype(np.int64).reshape(-1, 1), device=dev) for k, v in street["labels"].items()}
    g_d, ng_d, kitti_d = prep_api.downsample_map(torch.as_tensor(street["nonground"], device=dev),
                                                 torch.as_tensor(street["ground"], device=dev), labels_d, ctx=ctx)
    assert g_d.is_cuda and ng_d.is_cuda and all(v.is_cuda and v.dim() == 1 for v in kitti_d.values())
    assert g_d.cpu().numpy().tobytes() == oracle["ground"].tobytes() and ng_d.cpu().numpy().tobytes() == oracle["nonground"].tobytes()
    for k in map_ref.LABEL_KEYS:
        np.testing.assert_array_equal(kitti_d[k].cpu().numpy(), oracle["kitti"][k], err_msg=k)
    args = (street["T_pcd"], street["positions"], street["first_position"], street["indices"])
    d = prep_api.chunk_and_downsample_point_clouds(ng_d, g_d, *args, kitti_labels=kitti_d, ctx=ctx)
    ref = prep_ref.chunk_and_downsample_point_clouds(oracle["nonground"], oracle["ground"], *args, oracle["kitti"], workers=WORKERS)
    assert len(ref["pcd_nonground_chunks"]) >= 1 and ref["pcd_nonground_chunks"][0].shape[0] > 100_000
    assert all(c.is_cuda for c in d["pcd_nonground_chunks"]) and all(x.is_cuda for x in d["kitti_labels"]["ground"]["semantic"])
    _compare_dict(d, ref)
    with pytest.raises(ValueError):
        prep_api.downsample_map(street["nonground"], street["ground"], {k: v[:-1] for k, v in street["labels"].items()}, ctx=ctx)
    with pytest.raises(ValueError):
        prep_api.downsample_map(street["nonground"], street["ground"], {"seg_ground": street["labels"]["seg_ground"]}, ctx=ctx)


@pytest.mark.parametrize("name", sorted(map_ref.edge_cases()))
def test_hand_made_edges(name, ctx):
    c = map_ref.edge_cases()[name]
    p, voxel, claims = c["points"], c["voxel"], c["claims"]
    got = prep_api.voxel_down_sample_nearest(p, voxel, return_trace=True, return_dist=True, ctx=ctx)
    exp = map_ref.voxel_down_sample_nearest(p, voxel, brute=True)
    map_ref.check_nearest(name, got, exp)
    if "expect" in claims:
        assert got[1][exp[2][claims["member"]]] == claims["expect"]
    if "expect_all" in claims:
        assert got[1].tolist() == claims["expect_all"]
    if claims.get("ulps") == 0:     # equal distance from an own member and from a neighbour: labels differ, the order decides
        labels = np.arange(100, 100 + p.shape[0])
        assert labels[got[1]][exp[2][claims["member"]]] == 100 + claims["expect"]


def test_association_order_on_the_device(ctx):
    from test_map_ref import association_case
    p, _ = association_case()
    map_ref.check_nearest("association", prep_api.voxel_down_sample_nearest(p, 1.0, return_trace=True, return_dist=True, ctx=ctx),
                          map_ref.voxel_down_sample_nearest(p, 1.0, brute=True))


def test_empty_and_illegal_inputs(ctx):
    out, idx, tr, dist = prep_api.voxel_down_sample_nearest(np.zeros((0, 3)), 0.05, return_trace=True, return_dist=True, ctx=ctx)
    assert out.shape == (0, 3) and idx.shape == (0,) and idx.dtype == np.int64 and tr.shape == (0,) and dist.shape == (0,)
    g, ng, kitti = prep_api.downsample_map(np.zeros((0, 3)), np.zeros((0, 3)), {k: np.zeros(0, np.int32) for k in map_ref.LABEL_KEYS},
                                           ctx=ctx)
    assert g.shape == ng.shape == (0, 3) and all(v.shape == (0,) for v in kitti.values())
    p = np.random.default_rng(0).random((50, 3))
    for v in (0.0, -0.05, float("nan"), float("inf")):
        with pytest.raises(ValueError):
            prep_api.voxel_down_sample_nearest(p, v, ctx=ctx)
    with pytest.raises(ValueError):
        prep_api.voxel_down_sample_nearest(np.array([[0.0, 0, 0], [1e7, 0, 0]]), 1e-5, ctx=ctx)   # index beyond the int range
    with pytest.raises(ValueError):
        prep_api.voxel_down_sample_nearest(np.array([[0.0, 0, 0], [np.inf, 0, 0]]), 0.05, ctx=ctx)
    lib = _ffi.load()
    m = C.c_int64(7)
    assert lib.ai_voxel_down_sample_nearest(ctx._h, None, 0, 0.05, _ffi.AI_MEM_HOST, None, C.byref(m), None, None, None) == 0
    assert m.value == 0
    assert lib.ai_voxel_down_sample_nearest(ctx._h, None, 5, 0.05, _ffi.AI_MEM_HOST, None, C.byref(m), None, None, None) == -1
    assert lib.ai_voxel_down_sample_nearest(ctx._h, p.ctypes.data, 2 ** 31 - 256, 0.05, _ffi.AI_MEM_HOST, p.ctypes.data, C.byref(m),
                                            None, p.ctypes.data, None) == -1   # ai_box_select's bound on n


def test_call_variants(street, device, ctx):
    import torch
    dev = torch.device("cuda", ctx.device)
    p = street["nonground"]
    out, idx, tr, dist = device["nonground"]
    again = prep_api.voxel_down_sample_nearest(p, 0.05, return_trace=True, return_dist=True, ctx=ctx)
    for a, b in zip(again, device["nonground"]):
        assert a.tobytes() == b.tobytes()                                   # two calls: bit-identical
    d = prep_api.voxel_down_sample_nearest(torch.as_tensor(p, device=dev), 0.05, return_trace=True, return_dist=True, ctx=ctx)
    assert all(x.is_cuda for x in d) and d[1].dtype == torch.int64 and d[2].dtype == torch.int32
    for a, b in zip(d, device["nonground"]):
        assert a.cpu().numpy().tobytes() == b.tobytes()                     # device inputs: the same arrays
    only = prep_api.voxel_down_sample_nearest(p, 0.05, ctx=ctx)
    assert len(only) == 2 and only[0].tobytes() == out.tobytes() and only[1].tobytes() == idx.tobytes()
    # trace = NULL and nearest_dist = NULL straight through the binding, each alone and both, host and device buffers
    lib = _ffi.load()
    n = p.shape[0]
    p_d = torch.as_tensor(p, device=dev)
    for want_trace, want_dist in ((False, False), (True, False), (False, True)):
        for on_device in (False, True):
            if on_device:
                o, ni = torch.empty((n, 3), dtype=torch.float64, device=dev), torch.empty(n, dtype=torch.int32, device=dev)
                t, dd = torch.empty(n, dtype=torch.int32, device=dev), torch.empty(n, dtype=torch.float64, device=dev)
                ptr = lambda a: C.c_void_p(a.data_ptr())   # noqa: E731
                src, mem = ptr(p_d), _ffi.AI_MEM_DEVICE
            else:
                o, ni, t, dd = np.empty((n, 3)), np.empty(n, np.int32), np.empty(n, np.int32), np.empty(n)
                ptr = lambda a: a.ctypes.data              # noqa: E731
                src, mem = ptr(p), _ffi.AI_MEM_HOST
            m = C.c_int64(0)
            _ffi.check(lib.ai_voxel_down_sample_nearest(ctx._h, src, n, 0.05, mem, ptr(o), C.byref(m), ptr(t) if want_trace else None,
                                                        ptr(ni), ptr(dd) if want_dist else None), "ai_voxel_down_sample_nearest")
            if on_device:
                torch.cuda.synchronize()
                o, ni, t, dd = (x.cpu().numpy() for x in (o, ni, t, dd))
            assert m.value == out.shape[0]
            assert o[:m.value].tobytes() == out.tobytes() and np.array_equal(ni[:m.value], idx)
            assert not want_trace or t.tobytes() == tr.tobytes()
            assert not want_dist or dd[:m.value].tobytes() == dist.tobytes()


def test_label_file_round_trip_from_the_device(street, ctx, tmp_path):
    import torch
    from autoinst_amd import formats
    dev = torch.device("cuda", ctx.device)
    sub = {c: street[c][:50_000] for c in CLOUDS}
    labels = {k: torch.as_tensor(v[:50_000], device=dev) for k, v in street["labels"].items()}
    _, _, kitti = prep_api.downsample_map(torch.as_tensor(sub["nonground"], device=dev), torch.as_tensor(sub["ground"], device=dev),
                                          labels, ctx=ctx)
    path = tmp_path / "kitti_labels_preprocessed7_0.npz"
    formats.write_kitti_labels_preprocessed_npz(path, kitti)
    back = formats.read_kitti_labels_preprocessed_npz(path)
    for k in map_ref.LABEL_KEYS:
        assert back[k].shape == (kitti[k].shape[0], 1)
        np.testing.assert_array_equal(back[k].reshape(-1), kitti[k].cpu().numpy())
