"""GPU: the affinity build at its kernel thresholds, on every weights path (fixtures: tests/affinity_cases.py).

Every case goes through ``ncuts_api.get_affinity_matrix`` and `affinity_cases.check_affinity`: the reference's pattern
exactly, every value within the DERIVED `affinity_cases.bound` of the longdouble value, ``A == A.T`` bit for bit, unit
diagonal.  The three weight paths -- `k_weights_lanes` with 16-row tiles (default), with 32-row tiles
(``AI_WEIGHTS_TILE=32``) and the wave-per-row `k_weights` (``AI_WEIGHTS_ROWWISE=1``) -- are held to the promises the
source makes: 16- and 32-row tiles give the same bits, the staged and the fallback branch of one graph give the same bits
for a pair and its mirror, the register form of `k_weights` gives the bits of the generic loop on zero-padded features.
Row-wise and tiled sum in different orders: both are held to the bound.  The two variables are read once per process,
so each setting builds every case in a fresh child process that writes its matrices to an ``.npz``.

The largest error / bound ratio per case and path is printed (``-s``)."""
import os
import subprocess
import sys

import numpy as np
import pytest
import scipy.sparse as sp

import affinity_cases as ac

pytestmark = pytest.mark.gpu

NAMES = [c.name for c in ac.cases()]
# zero-padded features under AI_WEIGHTS_ROWWISE=1: (case, TARL width, DINO width) -- the extra terms are fma(0, 0, s) = s
PADDED = [("width_96_384", 112, 400), ("width_96_0", 112, 0), ("width_0_384", 0, 400), ("cliques16", 112, 400), ("width_100_112", 112, 112)]


def _pad(f, w):
    return f if f is None or not w else np.concatenate([f, np.zeros((f.shape[0], w - f.shape[1]))], axis=1)


def _build(api, c, tarl=None, dino=None):
    return api.get_affinity_matrix(c.points, c.tarl if tarl is None else tarl, c.dino if dino is None else dino, sam=c.sam, **c.kw())


def _bits_equal(A, B):
    return np.array_equal(A.indptr, B.indptr) and np.array_equal(A.indices, B.indices) and \
        np.array_equal(A.data.view(np.int64), B.data.view(np.int64))


def _first_difference(c, A, B):
    e = int(np.nonzero(A.data.view(np.int64) != B.data.view(np.int64))[0][0])
    return f"{A.data[e]!r} vs {B.data[e]!r} at {ac._where(c, e)}"


@pytest.fixture(scope="module")
def api(ctx):
    from autoinst_amd import ncuts_api
    assert "AI_WEIGHTS_TILE" not in os.environ and "AI_WEIGHTS_ROWWISE" not in os.environ, "this process must run the default paths"
    return ncuts_api


@pytest.fixture(scope="module")
def default_mats(api):
    """Every case through the default build, once."""
    return {c.name: _build(api, c) for c in ac.cases()}


_CHILD = r"""
import sys
sys.path[:0] = [sys.argv[1], sys.argv[1] + "/tests"]
import numpy as np
import affinity_cases as ac
import test_gpu_affinity as tg
from autoinst_amd import ncuts_api as api
api.default_context()
out = {}
def keep(key, A):
    out[key + "/indptr"], out[key + "/indices"], out[key + "/data"] = A.indptr, A.indices, A.data
for c in ac.cases():
    keep(c.name, tg._build(api, c))
if sys.argv[3] == "padded":
    for name, tw, dw in tg.PADDED:
        c = ac.case(name)
        keep("pad:" + name, tg._build(api, c, tg._pad(c.tarl, tw), tg._pad(c.dino, dw)))
np.savez(sys.argv[2], **out)
print(f"AFFINITY_CHILD {len(out) // 3} matrices")
"""


def _child(tmp_path_factory, setting, padded=False):
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    path = str(tmp_path_factory.mktemp("affinity") / (setting.replace("=", "_") + ".npz"))
    key, val = setting.split("=")
    env = dict(os.environ, **{key: val})
    r = subprocess.run([sys.executable, "-c", _CHILD, root, path, "padded" if padded else "plain"], env=env, timeout=600,
                       capture_output=True, text=True)
    assert r.returncode == 0, f"{setting}: exit {r.returncode}\n" + r.stdout[-3000:] + r.stderr[-3000:]
    assert "AFFINITY_CHILD" in r.stdout, r.stdout[-3000:]
    z = np.load(path)
    names = sorted({k.split("/")[0] for k in z.files})
    return {k: sp.csr_matrix((z[k + "/data"], z[k + "/indices"], z[k + "/indptr"]), shape=(z[k + "/indptr"].size - 1,) * 2) for k in names}


@pytest.fixture(scope="module")
def tile32_mats(tmp_path_factory):
    return _child(tmp_path_factory, "AI_WEIGHTS_TILE=32")


@pytest.fixture(scope="module")
def rowwise_mats(tmp_path_factory):
    return _child(tmp_path_factory, "AI_WEIGHTS_ROWWISE=1", padded=True)


def _report(c, path, m):
    per = ", ".join(f"{k} {v:.3f}" for k, v in sorted(m.items()) if k != "max_ratio")
    print(f"\n[affinity {c.name} {path}] n {c.n} largest error / bound {m['max_ratio']:.3f} ({per})")


# ------------------------------------------------------------------------------------------------ default path
@pytest.mark.parametrize("name", NAMES)
def test_default_build_matches_reference(api, default_mats, name):
    c = ac.case(name)
    A = default_mats[name]
    m = ac.check_affinity(c, A, "tile16" if c.tiled() else "rowwise")
    _report(c, "default", m)
    B = _build(api, c)
    assert _bits_equal(A, B), "the same call twice: " + _first_difference(c, A, B)


def test_underflowing_weights_are_stored(default_mats):
    """exp underflows to a subnormal for (0, 1) and to 0.0 for (0, 2), (1, 2): the entries stay, as in affinity_sparse."""
    c = ac.case("underflow")
    A, r = default_mats["underflow"], c.ref()
    assert A.indptr[1] - A.indptr[0] == 6 and A.nnz == r.indices.size
    assert 0.0 < A[0, 1] < 2.0 ** -1022 and abs(A[0, 1] - r.data[1]) <= r.bound[1]
    assert A[0, 2] == 0.0 and A[1, 2] == 0.0


@pytest.mark.parametrize("name", ["walk_3d_map", "walk_3d_negative"])
def test_translated_chunk_gives_the_untranslated_bits(default_mats, name):
    """The translation is exact on the 2^-10 grid: same cells, same order, same distances, same bits."""
    assert _bits_equal(default_mats[name], default_mats["walk_3d"]), _first_difference(ac.case(name), default_mats[name], default_mats["walk_3d"])


@pytest.mark.parametrize("name,rows", [("cliques16", 16), ("cliques32", 16), ("random_mixed", 16)])
def test_staged_and_fallback_branch_agree_on_mirrored_pairs(default_mats, name, rows):
    """(i, j) from a staged tile and (j, i) from a fallback tile of the same graph: equal bits (aw_sqdist_tree's promise)."""
    c = ac.case(name)
    e, m = ac.mirror_pairs(c, rows)
    assert e.size > 0
    d = default_mats[name].data
    bad = np.nonzero(d[e].view(np.int64) != d[m].view(np.int64))[0]
    assert bad.size == 0, f"{bad.size} of {e.size} pairs differ; first {d[e[bad[0]]]!r} vs {d[m[bad[0]]]!r} at {ac._where(c, int(e[bad[0]]))}"
    print(f"\n[affinity {name}] {e.size} staged entries with a fallback mirror, all equal")


# ------------------------------------------------------------------------------------------------ 32-row tiles
@pytest.mark.parametrize("name", NAMES)
def test_tile32_build_matches_reference_and_the_default_bits(default_mats, tile32_mats, name):
    c = ac.case(name)
    A = tile32_mats[name]
    m = ac.check_affinity(c, A, "tile32" if c.tiled() else "rowwise")
    _report(c, "AI_WEIGHTS_TILE=32", m)
    assert _bits_equal(A, default_mats[name]), "16- vs 32-row tiles: " + _first_difference(c, A, default_mats[name])


def test_tile32_staged_and_fallback_branch_agree_on_mirrored_pairs(tile32_mats):
    c = ac.case("cliques32")
    e, m = ac.mirror_pairs(c, 32)
    assert e.size > 0
    d = tile32_mats["cliques32"].data
    assert np.array_equal(d[e].view(np.int64), d[m].view(np.int64))


# ------------------------------------------------------------------------------------------------ wave per row
@pytest.mark.parametrize("name", NAMES)
def test_rowwise_build_matches_reference(default_mats, rowwise_mats, name):
    """Row-wise and tiled sum in different orders: the row-wise matrix is held to the bound, not to the tiled bits.  A case
    the default build already sends row-wise (SAM ids, a width that is not a multiple of 16) must give the same bits."""
    c = ac.case(name)
    A = rowwise_mats[name]
    m = ac.check_affinity(c, A, "rowwise")
    _report(c, "AI_WEIGHTS_ROWWISE=1", m)
    if not c.tiled():
        assert _bits_equal(A, default_mats[name]), _first_difference(c, A, default_mats[name])


@pytest.mark.parametrize("name,tw,dw", PADDED)
def test_rowwise_register_form_equals_generic_loop_on_padded_features(rowwise_mats, name, tw, dw):
    """96-d TARL / 384-d DINO keep the row's features in registers (k_weights<6, 24>, <6, 0>, <0, 24>); zero-padded to
    112 / 400 columns the generic loop runs (k_weights<0, 0>) and adds fma(0, 0, s): every bit is the same.  The 100-d
    case pads within the generic loop."""
    c = ac.case(name)
    A, B = rowwise_mats[name], rowwise_mats["pad:" + name]
    assert _bits_equal(A, B), _first_difference(c, A, B)


# ------------------------------------------------------------------------------------------------ device inputs, cameras
@pytest.mark.parametrize("name", ["cliques16", "sam_one_camera", "two_cameras_100"])
def test_device_resident_inputs_give_the_host_bits(api, default_mats, name):
    import torch
    c = ac.case(name)
    dev = lambda a, dt: None if a is None else torch.as_tensor(np.ascontiguousarray(a), dtype=dt).cuda()
    dino = [dev(d, torch.float64) for d in c.dino] if isinstance(c.dino, list) else dev(c.dino, torch.float64)
    sam = [dev(s, torch.int32) for s in c.sam] if isinstance(c.sam, list) else dev(c.sam, torch.int32)
    g = api.build_affinity(dev(c.points, torch.float64), dev(c.tarl, torch.float64), dino, sam=sam, **c.kw())
    try:
        A = g.to_scipy()
    finally:
        g.free()
    assert _bits_equal(A, default_mats[name]), _first_difference(c, A, default_mats[name])


@pytest.mark.parametrize("name", ["two_cameras_384", "two_cameras_100"])
def test_second_camera_is_applied_to_a_threshold_graph(default_mats, name):
    """ai_affinity_apply_camera (k_weights<0, 24> for a 384-d camera, <0, 0> for a 100-d one) on a graph with rows of 65 and
    129 entries: the reference multiplies the second camera's SAM and DINO factors in, the bound counts their roundings."""
    c = ac.case(name)
    assert len(c.dino) == 2 and len(c.sam) == 2 and (c.plan(16)["rowlen"] == 129).any()
    one = ac.Case("first_camera_only", c.points, c.tarl, c.dino[0], sam=c.sam[0], beta=c.beta, theta=c.theta, gamma=c.gamma)
    A = default_mats[name]
    m = ac.check_affinity(c, A, "two cameras")
    assert m["max_ratio"] <= 1.0
    assert np.abs(A.data - one.ref().data).max() > 1e-3       # the second camera really changed the values


# ------------------------------------------------------------------------------------------------ end to end
def test_ncuts_never_joins_two_far_apart_cliques(api):
    # every two clusters together hold more than split_lim = 1 % of the points, so the recursion cannot stop on a segment of two
    c = ac.case("cliques_no_row_over")
    groups = api.ncuts(c.points, c.tarl, c.dino, alpha=c.alpha, theta=c.theta, gamma=c.gamma, radius=c.radius)
    cluster = np.repeat(np.arange(len(c.sizes)), c.sizes)
    assert sorted(np.concatenate(groups).tolist()) == list(range(c.n))
    for g in groups:
        assert np.unique(cluster[g]).size == 1, f"a group spans clusters {np.unique(cluster[g])}"
    assert {int(cluster[g[0]]) for g in groups} == set(range(len(c.sizes)))
