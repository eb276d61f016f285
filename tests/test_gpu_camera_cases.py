"""GPU: `ai_camera_project` (csrc/ai_camera.hip) at its kernel limits.  Fixtures and truth: tests/camera_cases.py, proven on the CPU
by tests/test_camera_cases.py (which also shows which fixture fails for which wrong search).

Every fixture goes through `camera_api.camera_features` from NumPy arrays, twice, and from resident tensors.  Pixels, SAM labels,
view counts and means are bit-equal to the truth: rule 2 over all pairs in the camera frame, then `camera_ref`'s projection,
labels, cells and means.  The two host calls and the device call are bit-identical.  The fixture the entry refuses is refused
with its message, its outputs unwritten, and the context computes afterwards.
"""
import numpy as np
import pytest

import camera_cases as cc
from test_gpu_camera import bits_equal

pytestmark = pytest.mark.gpu

KEYS = ("pixels", "sam", "dino_views", "dino")


def _kw(c, ctx):
    return dict(feature_maps=c.feature_maps, sam_images=c.sam_images, max_dist=c.max_dist, return_pixels=True, ctx=ctx)


def _assert_truth(name, got, ref):
    for k in KEYS:
        if ref[k] is None:
            assert got[k] is None, (name, k)
            continue
        want = ref[k] if k in ("pixels", "dino") else np.asarray(ref[k]).astype(np.int32)
        g = np.asarray(got[k])
        if not bits_equal(g, want):
            bad = np.argwhere(~((g == want) | (np.isnan(g) & np.isnan(want)))) if g.shape == want.shape else []
            raise AssertionError(f"{name}: {k} differs from the truth at {len(bad)} places, first {bad[:1].tolist()}: "
                                 f"{g[tuple(bad[0])] if len(bad) else g.shape!r} instead of {want[tuple(bad[0])] if len(bad) else want.shape!r}")


@pytest.mark.parametrize("name", sorted(n for n, b in cc.cases().items() if not n.startswith("near_singular_below")))
def test_fixture_is_bit_equal_to_the_truth(name, ctx):
    import torch
    from autoinst_amd import camera_api
    c = cc.cases()[name]()
    ref = c.truth
    host = camera_api.camera_features(*c.args(), **_kw(c, ctx))
    _assert_truth(name, host, ref)
    again = camera_api.camera_features(*c.args(), **_kw(c, ctx))
    dev = torch.device("cuda", ctx.device)
    t = lambda a: None if a is None else torch.as_tensor(np.ascontiguousarray(a), device=dev)
    kw = dict(_kw(c, ctx), feature_maps=t(c.feature_maps), sam_images=t(c.sam_images))
    res = camera_api.camera_features(t(c.points), t(c.cloud), [t(v) for v in c.vis], c.T, c.K, c.image_hw, **kw)
    for k in KEYS:
        if ref[k] is None:
            continue
        assert bits_equal(again[k], host[k]), f"{name}: two calls differ in {k}"
        assert res[k].is_cuda and bits_equal(res[k].cpu().numpy(), host[k]), f"{name}: resident tensors give another {k}"


def test_nearly_singular_view_is_refused_and_nothing_is_written(ctx):
    from autoinst_amd import _ffi, camera_api
    c = cc.near_singular_case("below")
    with pytest.raises(ValueError, match=r"view 0 is \(nearly\) singular"):
        camera_api.camera_features(*c.args(), **_kw(c, ctx))
    # the entry itself, on outputs filled beforehand
    q, cl = np.ascontiguousarray(c.points), np.ascontiguousarray(c.cloud)
    vi = np.ascontiguousarray(np.concatenate(c.vis).astype(np.int32))
    off = np.concatenate([[0], np.cumsum([len(v) for v in c.vis])]).astype(np.int64)
    T, K = np.ascontiguousarray(c.T), np.ascontiguousarray(c.K)
    V, N = c.n_views, q.shape[0]
    h, w = c.image_hw
    fh, fw, F = c.feature_maps.shape[1:]
    pix, sam = np.full((N, V, 2), -7, np.int32), np.full((N, V), -7, np.int32)
    mean, views = np.full((N, F), -7.0), np.full(N, -7, np.int32)
    rc = _ffi.load().ai_camera_project(ctx._h, q.ctypes.data, N, cl.ctypes.data, cl.shape[0], vi.ctypes.data, off.ctypes.data, V, T.ctypes.data,
                                       K.ctypes.data, h, w, float(c.max_dist), c.feature_maps.ctypes.data, fh, fw, F, c.sam_images.ctypes.data,
                                       _ffi.AI_MEM_HOST, pix.ctypes.data, sam.ctypes.data, mean.ctypes.data, views.ctypes.data)
    assert rc == -1 and cc.REFUSAL in _ffi.load().ai_last_error().decode("utf-8", "replace")
    assert (pix == -7).all() and (sam == -7).all() and (mean == -7.0).all() and (views == -7).all()
    # the context is usable: the fixture just above the limit computes
    up = cc.near_singular_case("above")
    _assert_truth(up.name, camera_api.camera_features(*up.args(), **_kw(up, ctx)), up.truth)
