"""CPU suite: labels derived from ONE cut tree equal the model's direct cut at every threshold where the answer changes.

The yardstick is `gpu_model.normalized_cut_model` run at T' itself -- never the goldens' labels at another T: the reference's own
partitions are not nested (its SuperLU-decided remainder of disconnected segments)."""
import numpy as np
import pytest

import gpu_model
import tree_ref


def _direct(A, T):
    n = A.shape[0]
    return tree_ref.labels_of_groups(gpu_model.normalized_cut_model(A, n, np.arange(n), T=T), n)


def _check(A, tm, thresholds):
    for T in thresholds:
        lab, ng = tree_ref.relabel_ref(tm.labels, tm.cut_height, T)
        d = _direct(A, T)
        assert ng == int(d.max()) + 1, T
        assert np.array_equal(lab, d), T


@pytest.mark.parametrize("name,T_max", [("g1_blob_pair_spatial", 0.5), ("g2_multicomp_spatial", 0.3)])
def test_every_height_and_its_successor(name, T_max):
    A = tree_ref.load_graph(name)
    with tree_ref.cached_solver():
        tm = tree_ref.tree_model(A, A.shape[0], T_max)
        assert tm.n_cheaper >= 1, "the fixture no longer has a cut cheaper than an ancestor's: the max over the path is not exercised"
        assert tm.cut_height[0] == -np.inf and np.all(tm.cut_height[1:] < T_max) and np.all(tm.cut_height[1:] >= 0.0)
        solved = ~np.isnan(tm.leaf_cost)
        assert np.all(tm.leaf_cost[solved] >= T_max)
        _check(A, tm, tree_ref.sweep_thresholds(tm.cut_height, T_max))   # includes T' = 0 and T' = T_max


def test_g5_configuration_values_and_masked_heights():
    """g5 at T_max = 0.3: the three shipped configuration values, and the heights of the boundaries whose own cut is cheaper than
    an ancestor's (where `own cost` and `height` differ: a tree that stored the own cost would answer these wrongly)."""
    A = tree_ref.load_graph("g5_surface3k_T003")
    with tree_ref.cached_solver():
        tm = tree_ref.tree_model(A, A.shape[0], 0.3)
        assert tm.n_cheaper >= 1 and tm.masked.any()
        hs = np.unique(tm.cut_height[tm.masked])
        _check(A, tm, [0.005, 0.03, 0.075] + [float(h) for h in hs] + [float(np.nextafter(h, np.inf)) for h in hs])


def test_own_cost_is_not_the_height():
    """The non-monotone case by hand: a boundary made by a cheap cut below an expensive one appears only with the expensive one."""
    labels = np.array([0, 1, 2, 2, 1, 0])
    h = np.array([-np.inf, 0.04, 0.04])       # root cut 0.04 -> {0} | {1, 2}; the cut of {1, 2} cost 0.01 < 0.04
    lab, ng = tree_ref.relabel_ref(labels, h, 0.02)
    assert ng == 1 and not lab.any()
    lab, ng = tree_ref.relabel_ref(labels, h, np.nextafter(0.04, 1.0))
    assert ng == 3 and np.array_equal(lab, labels)
    lab, ng = tree_ref.relabel_ref(labels, h, 0.04)   # strict
    assert ng == 1
