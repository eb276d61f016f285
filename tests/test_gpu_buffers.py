"""GPU suite: ``autoinst_amd/_buffers.py`` with one torch device as the place, and the two NULL conventions of the bindings through
it.  Everything here is equality of bytes between the host form and the device form of the same call; the missing-wait race is not
looked for (tests/test_buffers.py guards the single ``sync()`` site by structure)."""
import numpy as np
import pytest
import torch

from autoinst_amd import _buffers, _ffi, points_api, prep_api

pytestmark = pytest.mark.gpu

NP_TO_TORCH = [(np.float64, torch.float64), (np.float32, torch.float32), (np.int64, torch.int64), (np.int32, torch.int32),
               (np.uint32, torch.int32), (np.uint8, torch.uint8)]


def _dev(a):
    return torch.as_tensor(a, device="cuda")


def _points(n, seed=0):
    return np.random.default_rng(seed + n).normal(size=(n, 3))


def _same(a, b):
    """The device result holds the bytes of the host result, in the same dtype and shape."""
    a = a.cpu().numpy()
    assert a.dtype == b.dtype and a.shape == b.shape and a.tobytes() == b.tobytes()


@pytest.mark.parametrize("n", [0, 1, 5])
def test_the_device_place(ctx, n):
    pts = _dev(_points(n))
    place = _buffers.place_of(None, np.zeros(3), pts)
    assert place.device == pts.device and place.mem == _ffi.AI_MEM_DEVICE
    for np_dtype, torch_dtype in NP_TO_TORCH:
        for shape in (n, (n, 3), max(n, 1)):
            a = place.new(shape, np_dtype)
            assert a.device == pts.device and a.dtype == torch_dtype and tuple(a.shape) == (shape if isinstance(shape, tuple) else (shape,))
    assert place.addr(None) is None and place.addr_or_null(None) is None
    assert (place.addr_or_null(pts) is None) == (n == 0)
    if n:
        assert place.addr(pts).value == pts.data_ptr() == place.addr_or_null(pts).value
    ids = np.arange(n, dtype=np.int32)[::-1].copy()
    got = place.index64(_dev(ids))
    assert got.device == pts.device and got.dtype == torch.int64
    _same(got, _buffers.HOST.index64(ids))
    place.sync()


@pytest.mark.parametrize("lengths", [(0, 1, 5), (5, 0, 1, 0), (0, 0), (1,)])
def test_concat_and_cat_int32_of_mixed_parts_hold_the_host_bytes(ctx, lengths):
    place = _buffers.Place(torch.device("cuda", torch.cuda.current_device()))
    parts = [_points(n, k) for k, n in enumerate(lengths)]
    want, want_off = _buffers.concat(parts, 3, np.float64, "x", _buffers.HOST)
    got, off = _buffers.concat([_dev(p) for p in parts], 3, np.float64, "x", place)   # points on the device must be tensors there
    assert np.array_equal(off, want_off) and got.is_contiguous()
    _same(got, want)
    with pytest.raises(ValueError, match="x on the device must be torch.float64"):
        _buffers.concat(parts, 3, np.float64, "x", place)
    ids = [np.arange(n, dtype=np.int64) * 7 - 3 for n in lengths]
    want = _buffers.cat_int32(ids, _buffers.HOST)
    for mixed in ([_dev(a) if k % 2 else a for k, a in enumerate(ids)], [_dev(a) for a in ids], ids,
                  [_dev(a.astype(np.int16)) if k % 2 == 0 else a.astype(np.int32) for k, a in enumerate(ids)]):
        got = _buffers.cat_int32(mixed, place)
        assert got.device == place.device and got.is_contiguous()
        _same(got, want)


# 5 fine points in 2 chunks; chunk 1 has no ground, chunk 0 no major point beyond one: both NULL conventions are on the path
FINE = [np.array([[0.0, 0.0, 0.0], [1.0, 0.0, 0.0], [0.0, 2.0, 0.0]]), np.array([[5.0, 5.0, 0.0], [6.0, 5.5, 0.5]])]
MAJOR = [np.array([[0.1, 0.0, 0.0], [0.9, 0.1, 0.0], [0.0, 1.9, 0.1]]), np.array([[5.1, 5.0, 0.0]])]
LABELS = [np.array([2, 0, 1]), np.array([0])]
GROUND = [np.array([[0.0, 0.0, -1.0], [0.5, 0.0, -1.0], [0.0, 0.5, -1.1], [0.5, 0.5, -0.9], [0.25, 0.25, -1.0]]), np.zeros((0, 3))]


@pytest.mark.parametrize("labels", [None, LABELS], ids=["no labels", "labels"])
def test_finish_chunks_on_device_tensors_returns_the_host_bytes(ctx, labels):
    kw = dict(nb_neighbors=3, std_ratio=2.0, return_stats=True, ctx=ctx)
    host = points_api.finish_chunks(FINE, MAJOR, labels, GROUND, **kw)
    dev = points_api.finish_chunks([_dev(a) for a in FINE], [_dev(a) for a in MAJOR], None if labels is None else [_dev(a) for a in labels],
                                   [_dev(a) for a in GROUND], **kw)
    assert len(host) == len(dev) == 2
    for h, d in zip(host, dev):
        assert sorted(h) == sorted(d)
        for key, want in h.items():
            if key == "stats":
                assert np.array_equal(np.array(list(want.values())), np.array(list(d[key].values())), equal_nan=True)
            elif want is None:
                assert d[key] is None and labels is None
            else:
                _same(d[key], want)
    assert host[1]["ground_keep"].shape == (0,) and host[0]["ground_keep"].dtype == np.int64
    if labels is not None:
        assert host[0]["merged_instance"][:3].tolist() == [3, 1, 2] and host[1]["merged_points"].shape == (2, 3)


def test_finish_chunks_without_any_major_point_passes_a_label_buffer_all_the_same(ctx):
    """major_label is not NULL when labels are given for no point: NULL would mean "no labels" and the merged outputs would go."""
    empty = np.zeros((0, 3))
    for to in (lambda a: a, _dev):
        out = points_api.finish_chunks([to(empty)], [to(empty)], [to(np.zeros(0, np.int32))], [to(GROUND[0])], nb_neighbors=3, ctx=ctx)[0]
        assert out["merged_points"] is not None and tuple(out["merged_points"].shape) == (int(out["ground_keep"].shape[0]), 3)


def test_voxel_down_sample_nearest_on_a_device_tensor_returns_the_host_bytes(ctx):
    pts = np.concatenate(FINE)
    for kw in (dict(), dict(return_trace=True), dict(return_trace=True, return_dist=True)):
        host = prep_api.voxel_down_sample_nearest(pts, 1.5, ctx=ctx, **kw)
        dev = prep_api.voxel_down_sample_nearest(_dev(pts), 1.5, ctx=ctx, **kw)
        assert len(host) == len(dev) == 2 + len(kw)
        for h, d in zip(host, dev):
            _same(d, h)
        assert host[1].dtype == np.int64 and 0 < host[0].shape[0] <= 5
