"""CPU: the minor-voxel map entry point is declared, bound and exported, and its label file has the reference's layout."""
import os
import re

import numpy as np

from conftest import ROOT
from autoinst_amd import _ffi, formats


def test_entry_point_is_declared_bound_and_exported():
    txt = open(os.path.join(ROOT, "include", "autoinst_hip.h")).read()
    txt = re.sub(r"/\*.*?\*/", "", txt, flags=re.S)
    m = re.search(r"\bint\s+ai_voxel_down_sample_nearest\s*\(([^)]*)\)\s*;", txt)
    assert m, "include/autoinst_hip.h does not declare ai_voxel_down_sample_nearest"
    args = [re.sub(r"\s+", " ", a).strip() for a in m.group(1).split(",")]
    assert args == ["ai_ctx* ctx", "const double* xyz", "int64_t n", "double voxel_size", "int mem_kind", "double* out_xyz",
                    "int64_t* n_out", "int32_t* trace", "int32_t* nearest_index", "double* nearest_dist"]
    assert "ai_voxel_down_sample_nearest" in _ffi.SYMBOLS
    lib = _ffi.load()
    assert hasattr(lib, "ai_voxel_down_sample_nearest")
    assert len(lib.ai_voxel_down_sample_nearest.argtypes) == len(args)
    assert int(re.search(r"#define AI_ABI_VERSION (\d+)", txt).group(1)) == 6   # no struct changed


def test_python_surface():
    import inspect

    import autoinst_amd
    from autoinst_amd import prep_api
    from autoinst_amd.config import MINOR_VOXEL_SIZE
    assert autoinst_amd.downsample_map is prep_api.downsample_map
    assert autoinst_amd.voxel_down_sample_nearest is prep_api.voxel_down_sample_nearest
    sig = inspect.signature(prep_api.voxel_down_sample_nearest)
    assert list(sig.parameters) == ["points", "voxel_size", "return_trace", "return_dist", "ctx"]
    assert sig.parameters["voxel_size"].default == MINOR_VOXEL_SIZE == 0.05
    assert list(inspect.signature(prep_api.downsample_map).parameters) == ["pcd_nonground", "pcd_ground", "labels", "voxel_size", "ctx"]


def test_kitti_labels_preprocessed_npz_round_trip(tmp_path):
    rng = np.random.default_rng(0)
    lab = {"seg_ground": rng.integers(0, 60, 7).astype(np.int32), "seg_nonground": rng.integers(0, 60, 11).astype(np.uint16),
           "instance_ground": np.zeros(7, np.int64), "instance_nonground": rng.integers(0, 2 ** 40, 11).reshape(-1, 1)}
    path = tmp_path / "kitti_labels_preprocessed0_0.npz"
    formats.write_kitti_labels_preprocessed_npz(path, lab)
    with np.load(path) as z:                                   # the reference's reader: four keys, (m, 1) columns
        assert sorted(z.files) == sorted(["instance_ground", "instance_nonground", "seg_nonground", "seg_ground"])
        for k in z.files:
            assert z[k].shape == (lab[k].size, 1) and z[k].dtype == lab[k].dtype
            assert np.array_equal(z[k].reshape(-1), np.asarray(lab[k]).reshape(-1))
        # what load_downsampled_pcds does with them (dataset_utils.py:442-451)
        inst = np.hstack((z["instance_nonground"].reshape(-1), z["instance_ground"].reshape(-1)))
        assert inst.shape == (18,)
    back = formats.read_kitti_labels_preprocessed_npz(path)
    assert set(back) == set(lab) and all(np.array_equal(back[k].reshape(-1), np.asarray(lab[k]).reshape(-1)) for k in lab)
    # a reference-style file: lists of 1-element rows saved by np.savez (dataset_utils.py:311, :378-384)
    ref_style = tmp_path / "ref.npz"
    np.savez(ref_style, **{k: [np.asarray(lab[k]).reshape(-1, 1)[i] for i in range(np.asarray(lab[k]).size)] for k in lab})
    ref_back = formats.read_kitti_labels_preprocessed_npz(ref_style)
    assert all(ref_back[k].shape == back[k].shape and np.array_equal(ref_back[k], back[k]) for k in lab)
