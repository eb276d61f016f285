"""CPU, no library: ``autoinst_amd/_buffers.py`` on the host, and the structure it gives the bindings -- each shared piece of the
host-or-device plumbing is defined once, there, and no ``*_api.py`` takes a pointer or waits for a stream itself."""
import ctypes
import glob
import os
import re

import numpy as np
import pytest

from autoinst_amd import _buffers, _ffi

_PKG = os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "autoinst_amd")
HOST = _buffers.HOST


def test_the_host_place():
    assert HOST.device is None and HOST.mem == _ffi.AI_MEM_HOST
    assert _buffers.place_of() is HOST and _buffers.place_of(None, np.zeros(3), [1, 2]) is HOST
    for dtype in (np.float64, np.float32, np.int64, np.int32, np.uint32, np.uint8):
        for shape in (0, 5, (2, 3), (0, 3)):
            a = HOST.new(shape, dtype)
            assert isinstance(a, np.ndarray) and a.dtype == dtype and a.shape == (shape if isinstance(shape, tuple) else (shape,))
            assert a.flags.c_contiguous
    HOST.sync()   # nothing to wait for


def test_host_addresses():
    a = np.arange(6, dtype=np.int32)
    assert HOST.addr(None) is None and HOST.addr_or_null(None) is None
    assert HOST.addr(a) == a.ctypes.data and HOST.addr_or_null(a) == a.ctypes.data
    assert ctypes.cast(HOST.addr(a), ctypes.POINTER(ctypes.c_int32))[4] == 4
    for empty in (np.zeros(0, np.int32), np.zeros((0, 3))):
        assert HOST.addr_or_null(empty) is None
        assert HOST.addr(empty) is not None   # the buffer's own pointer: "empty" is not "not wanted"


def test_index64_on_the_host():
    a = np.array([3, 0, 2 ** 31 - 1, 7], dtype=np.int32)
    b = HOST.index64(a)
    assert b.dtype == np.int64 and np.array_equal(a, b)
    assert HOST.index64(a[:0]).dtype == np.int64 and HOST.index64(a[:0]).shape == (0,)


def _segments(lengths, width=3, dtype=np.float64):
    rng = np.random.default_rng(sum(lengths) + len(lengths))
    return [rng.normal(size=(n, width)).astype(dtype) for n in lengths]


@pytest.mark.parametrize("lengths", [(0, 1, 5), (0, 0, 1, 5, 0), (5, 0, 1), (1,), (0,), (0, 0), ()])
def test_concat_and_its_offsets(lengths):
    parts = _segments(lengths)
    full, off = _buffers.concat(parts, 3, np.float64, "x", HOST)
    assert off.dtype == np.int64 and off.tolist() == [0] + list(np.cumsum(lengths, dtype=np.int64))
    assert full.dtype == np.float64 and full.shape == (sum(lengths), 3) and full.flags.c_contiguous
    for k, p in enumerate(parts):
        assert np.array_equal(full[off[k]:off[k + 1]], p)
    assert np.array_equal(_buffers.offsets_of(list(lengths)), off) and _buffers.offsets_of(list(lengths)).dtype == np.int64
    # the same segments as the caller's own concatenation with its offsets
    own, own_off = _buffers.segmented(full, off.tolist(), 3, np.float64, "x", HOST)
    assert np.array_equal(own, full) and own_off.dtype == np.int64 and np.array_equal(own_off, off)


def test_concat_converts_and_reshapes_empties():
    full, off = _buffers.concat([np.zeros(0), [[1, 2, 3]], np.zeros((0, 3), np.float32)], 3, np.float64, "x", HOST)
    assert full.dtype == np.float64 and full.tolist() == [[1.0, 2.0, 3.0]] and off.tolist() == [0, 0, 1, 1]


def test_the_width_of_an_all_empty_concat_is_that_of_the_first_part():
    for parts, cols, width in (([np.zeros((0, 7)), np.zeros((0, 4))], None, 7), ([np.zeros(0), np.zeros((0, 4))], None, 0),
                               ([], None, 0), ([], 3, 3), ([np.zeros(0)], 3, 3)):
        full, off = _buffers.concat(parts, cols, np.float32, "x", HOST)
        assert full.shape == (0, width) and full.dtype == np.float32 and off.tolist() == [0] * (len(parts) + 1)
    # segments with rows fix the width; the empty ones do not count
    full, _ = _buffers.concat([np.zeros((0, 7)), np.ones((2, 4))], None, np.float32, "x", HOST)
    assert full.shape == (2, 4)
    with pytest.raises(ValueError, match="x: every segment must have the same width"):
        _buffers.concat([np.ones((1, 7)), np.ones((2, 4))], None, np.float32, "x", HOST)


@pytest.mark.parametrize("lengths", [(0, 1, 5), (0, 0, 1, 5, 0), (5, 0, 1), (1,), (0,), (0, 0), ()])
def test_cat_int32(lengths):
    rng = np.random.default_rng(len(lengths))
    dtypes = (np.int64, np.int32, np.uint8, np.int16)
    parts = [rng.integers(0, 100, size=n).astype(dtypes[k % 4]) for k, n in enumerate(lengths)]
    out = _buffers.cat_int32(parts, HOST)
    assert out.dtype == np.int32 and out.shape == (sum(lengths),) and out.flags.c_contiguous
    assert out.tolist() == [int(v) for p in parts for v in p]


def test_cat_int32_takes_the_empty_list_of_a_chunk_without_points():
    out = _buffers.cat_int32([np.asarray([]), np.asarray([4, 5])], HOST)   # np.asarray([]) is float64
    assert out.dtype == np.int32 and out.tolist() == [4, 5]


def test_points_f64():
    class Cloud:
        points = [[0, 1, 2], [3, 4, 5]]
    for given in (Cloud(), Cloud.points, np.asarray(Cloud.points, dtype=np.float32), np.asfortranarray(np.asarray(Cloud.points, dtype=np.float64))):
        a = _buffers.points_f64(given, "cloud")
        assert a.dtype == np.float64 and a.shape == (2, 3) and a.flags.c_contiguous and a.tolist() == [[0, 1, 2], [3, 4, 5]]
    assert _buffers.points_f64(np.zeros(0)).shape == (0, 3) and _buffers.points_f64([]).shape == (0, 3)
    for bad in (np.zeros((2, 2)), np.zeros(3), np.zeros((1, 3, 1))):
        with pytest.raises(ValueError, match=r"^cloud must be \(n, 3\)$"):
            _buffers.points_f64(bad, "cloud")


def test_grow_asks_once_when_the_capacity_suffices():
    asked = []

    def call(cap):
        asked.append(cap)
        return 7, "result of %d" % cap
    assert _buffers.grow(call, 7) == (7, "result of 7") and asked == [7]
    asked.clear()
    assert _buffers.grow(call, 100) == (7, "result of 100") and asked == [100]


def test_grow_asks_again_with_the_reported_total():
    asked = []

    def call(cap):
        asked.append(cap)
        return 1000, list(range(min(cap, 1000)))
    total, result = _buffers.grow(call, 16)
    assert asked == [16, 1000] and total == 1000 and len(result) == 1000


# ------------------------------------------------------------------------------------------------------------------ structure
def _sources():
    out = {}
    for path in sorted(glob.glob(os.path.join(_PKG, "*.py"))):
        with open(path) as f:
            out[os.path.basename(path)] = f.read()
    return out


SOURCES = _sources()
APIS = sorted(n for n in SOURCES if n.endswith("_api.py"))
HELPERS = ["is_device_tensor", "place_of", "points_f64", "rows", "concat", "segmented", "offsets_of", "cat_int32", "grow"]
PLACE_METHODS = ["new", "addr", "addr_or_null", "index64", "sync"]
FORMER_NAMES = ["_points", "_f64_points", "_call_args", "_rows", "_concat", "_segmented", "_chunk_labels", "_scan_offsets", "_dev_f64"]


def _files_with(pattern):
    return [name for name, text in SOURCES.items() for _ in re.finditer(pattern, text, re.M)]


def test_the_five_bindings_are_the_ones_looked_at():
    assert APIS == ["camera_api.py", "labels_api.py", "ncuts_api.py", "points_api.py", "prep_api.py"]


def test_only_buffers_takes_a_device_pointer():
    assert _files_with(r"data_ptr\(") == ["_buffers.py"]


def test_only_buffers_waits_for_torch():
    # sharding.py's one wait follows its own gather and feeds a thread, not a library call
    assert _files_with(r"current_stream\(") == ["_buffers.py", "sharding.py"]
    assert len(_files_with(r"\.synchronize\(")) == 2


@pytest.mark.parametrize("helper", HELPERS)
def test_a_helper_is_defined_once(helper):
    assert _files_with(r"^def %s\(" % helper) == ["_buffers.py"]
    assert _files_with(r"^\s*def _?%s\(" % helper) == ["_buffers.py"], "a second definition, nested or underscored"


@pytest.mark.parametrize("method", PLACE_METHODS)
def test_a_place_method_is_defined_once(method):
    assert _files_with(r"^    def %s\(self" % method) == ["_buffers.py"]


@pytest.mark.parametrize("name", FORMER_NAMES)
def test_no_copy_is_left_under_its_former_name(name):
    assert _files_with(r"^\s*def %s\(" % name) == []
    assert not any(re.search(r"(?<![\w.])%s\(" % name, text) for text in SOURCES.values()), name


@pytest.mark.parametrize("api", APIS)
def test_a_binding_defines_no_plumbing_of_its_own(api):
    text = SOURCES[api]
    assert not re.search(r"^\s*def (new|addr|ptr|out_ptr|empty)\(", text, re.M)
    assert not re.search(r"^\s*(new|addr|ptr|out_ptr)\s*=", text, re.M)
    assert not re.search(r"from \.\w+_api import [^\n]*\b_(concat|rows|segmented)\b", text)
    assert "AI_MEM_DEVICE" not in text   # the place knows


def test_the_wait_stands_directly_before_the_call_of_every_device_entry():
    """Between ``place.sync()`` and the library call that follows it there is nothing but the call's own opening line, and every
    entry that passes ``place.mem`` waits first."""
    waited, unwaited = [], []
    for api in APIS:
        text = SOURCES[api]
        for m in re.finditer(r"\b(?:lib|_ffi\.load\(\))\.(ai_\w+)\(", text):
            end, depth = m.end(), 1
            while depth:   # the call's arguments, to its closing parenthesis
                depth += {"(": 1, ")": -1}.get(text[end], 0)
                end += 1
            if "place.mem" not in text[m.end():end]:
                continue   # a host-only or handle-only entry
            before = text[:text.rfind("\n", 0, m.start())].rsplit("\n", 1)[-1].strip()
            (waited if before.startswith("place.sync()") else unwaited).append((api, m.group(1)))
    assert unwaited == []
    assert sorted(set(name for _, name in waited)) == [
        "ai_affinity_apply_camera", "ai_affinity_build_sam", "ai_aggregate_scans", "ai_box_select", "ai_camera_project", "ai_chunk_finish",
        "ai_ground_planes", "ai_merge_map", "ai_scan_pool", "ai_statistical_inliers", "ai_voxel_down_sample", "ai_voxel_down_sample_nearest"]
