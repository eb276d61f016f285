"""CPU suite: the argument checks of `CutTree` and `relabel` that are made before anything reaches the device."""
import numpy as np
import pytest

import autoinst_amd
from autoinst_amd import ncuts_api as api


def _tree(T_max=0.1):
    return api.CutTree(np.array([0, 1, 1, 2, 0], dtype=np.int32), 3, [-np.inf, 0.02, 0.05], [0.3, np.nan, np.inf], T_max)


def test_exports():
    for name in ("CutTree", "ncuts_tree", "ncuts_tree_batch", "relabel", "normalized_cut_sweep"):
        assert getattr(autoinst_amd, name) is getattr(api, name)
        assert name in api.__all__


def test_cut_tree_checks_its_arrays():
    with pytest.raises(ValueError):
        api.CutTree(np.zeros(4, dtype=np.int32), 2, [-np.inf], None, 0.1)            # one height per group
    with pytest.raises(ValueError):
        api.CutTree(np.zeros(4, dtype=np.int32), 2, [0.0, 0.01], None, 0.1)          # the first boundary is none
    t = api.CutTree(np.zeros(0, dtype=np.int32), 0, [], None, 0.1)                     # a chunk without points
    assert t.n_groups_at(0.05) == 0 and t.leaf_cost is None


def test_group_counts_come_from_the_heights():
    t = _tree()
    assert [t.n_groups_at(T) for T in (-1.0, 0.0, 0.02, np.nextafter(0.02, 1.0), 0.05, np.nextafter(0.05, 1.0), 0.1)] == [1, 1, 1, 2, 2, 3, 3]


@pytest.mark.parametrize("T", [0.2, np.nextafter(0.1, 1.0), np.nan, np.inf, -np.inf])
def test_thresholds_the_tree_cannot_answer(T):
    t = _tree()
    for f in (t.n_groups_at, t.labels_at, t.groups_at):
        with pytest.raises(ValueError):
            f(T)
    with pytest.raises(ValueError):
        api.relabel([t], [0.01, T])


def test_relabel_arguments():
    t = _tree()
    with pytest.raises(ValueError):
        api.relabel([], [0.01])
    with pytest.raises(ValueError):
        api.relabel([t], [])
    with pytest.raises(ValueError):
        api.relabel([t.labels], [0.01])                       # trees, not label arrays
    with pytest.raises(ValueError):
        api.relabel([t, _tree(0.03)], [0.04])                 # above the smaller T_max of the two
    with pytest.raises(ValueError):
        api.normalized_cut_sweep(None, 5, np.arange(5), [])
    with pytest.raises(ValueError):
        api.normalized_cut_sweep(None, 5, np.arange(5), [0.01, np.nan])
