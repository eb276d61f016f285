"""CPU, no library: the argument checks of ``ncuts_api.build_affinity_batch`` and the ``batched_build`` switch of
``sharding.run_chunks``.  Every ValueError here is raised before the shared library is touched."""
import inspect

import numpy as np
import pytest

import autoinst_amd
from autoinst_amd import _ffi, ncuts_api, sharding


@pytest.fixture()
def no_library(monkeypatch):
    def load():
        raise AssertionError("the library was loaded before the arguments were checked")
    monkeypatch.setattr(_ffi, "load", load)


def _chunks(sizes=(5, 3), tdim=16, ddim=32):
    rng = np.random.default_rng(0)
    return ([rng.normal(size=(n, 3)) for n in sizes], [rng.normal(size=(n, tdim)) for n in sizes],
            [rng.normal(size=(n, ddim)) for n in sizes])


def test_exported_from_the_package():
    assert autoinst_amd.build_affinity_batch is ncuts_api.build_affinity_batch
    assert "build_affinity_batch" in ncuts_api.__all__ and "ai_affinity_build_batch" in _ffi.SYMBOLS
    p = inspect.signature(ncuts_api.build_affinity_batch).parameters
    assert [k for k in p][:3] == ["points", "tarl", "dino"]
    for k in ("offsets", "alpha", "theta", "gamma", "radius", "group_rows", "ctx"):
        assert p[k].kind is inspect.Parameter.KEYWORD_ONLY, k
    assert p["group_rows"].default is None and p["offsets"].default is None


def test_feature_rows_must_match_the_points(no_library):
    pts, tarl, dino = _chunks()
    with pytest.raises(ValueError, match="tarl"):
        ncuts_api.build_affinity_batch(pts, [tarl[0], tarl[1][:-1]], dino, alpha=1.0, theta=0.5, gamma=0.1)
    with pytest.raises(ValueError, match="dino"):
        ncuts_api.build_affinity_batch(np.concatenate(pts), np.concatenate(tarl), np.concatenate(dino)[:-1], offsets=[0, 5, 8],
                                       alpha=1.0, theta=0.5, gamma=0.1)
    # the same number of rows, split differently
    with pytest.raises(ValueError, match="tarl"):
        ncuts_api.build_affinity_batch(pts, [tarl[0][:4], np.concatenate([tarl[0][4:], tarl[1]])], dino, alpha=1.0, theta=0.5, gamma=0.1)
    with pytest.raises(ValueError, match="offsets"):
        ncuts_api.build_affinity_batch(np.concatenate(pts), offsets=[0, 5, 9], alpha=1.0, theta=0.0, gamma=0.0)
    with pytest.raises(ValueError, match="offsets"):
        ncuts_api.build_affinity_batch(np.concatenate(pts), offsets=[1, 5, 8], alpha=1.0, theta=0.0, gamma=0.0)


def test_weights_need_their_features(no_library):
    pts, tarl, dino = _chunks()
    with pytest.raises(ValueError, match="theta != 0 needs TARL features"):
        ncuts_api.build_affinity_batch(pts, None, dino, alpha=1.0, theta=0.5, gamma=0.1)
    with pytest.raises(ValueError, match="The length should be longer than 0!"):   # the reference's message
        ncuts_api.build_affinity_batch(pts, tarl, None, alpha=1.0, theta=0.5, gamma=0.1)
    with pytest.raises(ValueError, match="The length should be longer than 0!"):
        ncuts_api.build_affinity_batch(pts, tarl, [], alpha=1.0, theta=0.5, gamma=0.1)


def test_a_list_of_cameras_is_refused(no_library):
    pts, tarl, dino = _chunks()
    cat = np.concatenate
    with pytest.raises(ValueError, match="camera"):   # concatenated input: a list for dino can only mean cameras
        ncuts_api.build_affinity_batch(cat(pts), cat(tarl), [cat(dino), cat(dino)], offsets=[0, 5, 8], alpha=1.0, theta=0.5, gamma=0.1)
    with pytest.raises(ValueError, match="camera"):   # per-chunk lists: one matrix per chunk, not one more per camera
        ncuts_api.build_affinity_batch(pts, tarl, dino + [dino[0]], alpha=1.0, theta=0.5, gamma=0.1)
    with pytest.raises(ValueError, match="one matrix per chunk"):
        ncuts_api.build_affinity_batch(pts, tarl, cat(dino), alpha=1.0, theta=0.5, gamma=0.1)


class _FakeDeviceTensor:
    """What `_buffers.is_device_tensor` looks at, without a device."""
    is_cuda = True
    device = "cuda:0"

    def __init__(self, shape):
        self.shape = shape

    def data_ptr(self):
        return 0


def test_host_and_device_inputs_do_not_mix(no_library):
    pts, tarl, dino = _chunks()
    with pytest.raises(ValueError, match="mixed"):
        ncuts_api.build_affinity_batch(pts, [tarl[0], _FakeDeviceTensor((3, 16))], dino, alpha=1.0, theta=0.5, gamma=0.1)
    with pytest.raises(ValueError, match="mixed"):
        ncuts_api.build_affinity_batch(pts, tarl, _FakeDeviceTensor((8, 32)), alpha=1.0, theta=0.5, gamma=0.1)


def test_run_chunks_accepts_batched_build():
    p = inspect.signature(sharding.run_chunks).parameters["batched_build"]
    assert p.default is False and p.kind is inspect.Parameter.KEYWORD_ONLY
    assert sharding.run_chunks([], batched_build=True) == []
    with pytest.raises(ValueError):
        sharding.run_chunks([(np.zeros((3, 3)), None)], threads=0, batched_build=True)
