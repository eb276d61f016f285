"""CPU: the eigensolver fixtures of tests/eig_cases.py have the spectra they claim, reach the solver branches they are meant
to reach, and `check_eigs` rejects answers that residual and orthogonality checks alone would pass.
tests/test_gpu_eigs.py runs the same fixtures through ``ai_eigs_smallest``."""
import numpy as np
import pytest
from scipy.sparse.csgraph import connected_components

import eig_cases as ec


CLOSED = [ec.ring(200), ec.torus(12, 15), ec.torus(16, 16), ec.torus(31, 33), ec.torus(32, 32), ec.torus(33, 34),
          ec.complete(5), ec.complete(24), ec.star(9), ec.star(40), ec.star(2001)]


@pytest.mark.parametrize("c", CLOSED, ids=lambda c: c.name)
def test_closed_form_spectrum_equals_eigh(c):
    lam = ec.reference(c.w)[0]
    assert np.abs(lam - c.closed).max() <= 1e-12


@pytest.mark.parametrize("c", [c for c in CLOSED if c.w.shape[0] <= 1024], ids=lambda c: c.name)
def test_permuted_closed_form_keeps_the_spectrum(c):
    lam = ec.reference(ec.variant(c, "perm").w)[0]
    assert np.abs(lam - c.closed).max() <= 1e-12


def _repeat_inside(lam, k, sep):
    return bool(np.any(np.diff(lam[:k]) <= sep))


def test_multiplicity_fixtures_repeat_inside_the_wanted_range():
    by = {c.name: c for c in ec.cases()}
    # exact repeats (closed form): some k of each case has two equal eigenvalues among its first k
    for name in ("ring200", "torus12x15", "torus16x16", "torus31x33", "torus32x32", "torus33x34", "complete5", "complete24",
                 "star9", "star40", "star2001"):
        c = by[name]
        ks = [k for k in c.ks if k >= 3 and _repeat_inside(c.closed, k, 1e-12)]
        assert ks, name
    # on the square torus a cluster of 4 straddles k = 3 and one of 8 straddles k = 10 or 34
    cl = ec.clusters(by["torus32x32"].closed, 1e-12)
    sizes = {e - s for s, e in cl}
    assert 8 in sizes and any(s < 3 < e for s, e in cl) and any(s < k < e and e - s == 8 for s, e in cl for k in (10, 34))
    # near repeats of the twins (closer than 1e-6, apart by more than 1e-13) inside the wanted range
    for name in ("twin500_eps1e-06", "twin750_eps1e-09"):
        c = by[name]
        lam = ec.reference(c.w)[0]
        d = np.diff(lam[1:max(c.ks)])
        assert np.any((d < 1e-6) & (d > 0)), name
    # the bridges' lambda_2 is below the tolerance
    for name in ("bridge300+500_eps1e-08", "bridge300+500_eps1e-12"):
        lam = ec.reference(by[name].w)[0]
        assert lam[1] < 1e-10 < lam[2], name
    # the mixture holds two identical components: every eigenvalue of the 120-row piece twice
    assert connected_components(by["mixture"].w, directed=False)[0] == 12


def test_every_case_reaches_its_branch():
    all_cases = ec.cases() + ec.variants()
    got = {}
    for c in all_cases:
        for k in c.ks:
            assert k <= c.w.shape[0]
            got[(c.name, k)] = ec.branches(c.w, k)
    # the branch rule at its boundaries
    assert got[("torus16x16", 3)] == {"dense"} and got[("torus16x16", 33)] == {"dense"}          # 256 rows: last dense size
    assert got[("surface257", 3)] == {"chfsi1"} and got[("surface257", 64)] == {"chfsi2"}         # 257: first block size
    assert got[("surface257", 2)] == {"lanczos"} and got[("ring200", 2)] == {"dense"}             # one pair
    assert got[("torus32x32", 3)] == {"chfsi1"}                                                   # k1 = 2 on a large graph
    assert got[("torus32x32", 33)] == {"chfsi1"} and got[("torus32x32", 34)] == {"chfsi2"}        # CPL boundary k1 = 32 / 33
    assert got[("complete5", 5)] == {"dense"} and got[("star9", 9)] == {"dense"}                  # k == n
    assert got[("mixture", 12)] == set() and got[("mixture", 13)] == {"lanczos", "dense"}         # ncomp == k, == k - 1
    assert got[("mixture", 20)] == {"dense", "chfsi1"}                                            # mixed branches, one call
    assert got[("mixture", 64)] == {"dense", "chfsi2"}
    assert set().union(*got.values()) == {"lanczos", "dense", "chfsi1", "chfsi2"}
    # the row shapes the block kernels branch on
    by = {c.name: c for c in all_cases}
    assert by["torus33x34"].w.shape[0] % 8 == 2
    assert np.diff(by["star2001"].w.indptr).max() == 2000
    for name in ("torus12x15_shuffled", "torus33x34_shuffled", "surface1500_shuffled"):
        w = by[name].w
        desc = [np.any(np.diff(w.indices[w.indptr[i]:w.indptr[i + 1]]) < 0) for i in range(w.shape[0])]
        assert np.mean(desc) > 0.5, name
        assert (w != by[name.replace("_shuffled", "")].w).nnz == 0
    assert by["surface1500_nodiag"].w.diagonal().max() == 0.0 and by["torus12x15_diag"].w.diagonal().min() == 1.0


# --------------------------------------------------------------------------- the checker against mutated answers
def _good(c, k, ref):
    """A correct answer built from the reference: exact zero pairs, then the next reference pairs."""
    lam, U, L, d = ref
    ncomp, comp = connected_components(c.w, directed=False)
    nz = min(ncomp, k)
    n = c.w.shape[0]
    V = np.zeros((n, k))
    ev = np.zeros(k)
    for j in range(nz):
        on = comp == j
        V[on, j] = np.sqrt(d[on] / d[on].sum())
    V[:, nz:] = U[:, nz:k]
    ev[nz:] = lam[nz:k]
    res = np.linalg.norm(L @ V - V * ev[None, :], axis=0).max()
    return ev, V, float(res)


@pytest.fixture(scope="module")
def ring_ref():
    c = ec.ring(200)
    return c, ec.reference(c.w)


@pytest.fixture(scope="module")
def mix_ref():
    c = ec.mixture()
    return c, ec.reference(c.w)


def test_check_accepts_the_reference(ring_ref, mix_ref):
    for (c, ref), k in ((ring_ref, 3), (ring_ref, 64), (mix_ref, 5), (mix_ref, 20), (mix_ref, 64)):
        ev, V, res = _good(c, k, ref)
        ec.check_eigs(c.w, k, ev, V, res, ref=ref)


def test_rejects_a_missing_copy_of_a_double_eigenvalue(ring_ref):
    c, ref = ring_ref
    lam, U, _, _ = ref
    ev, V, res = _good(c, 3, ref)
    assert abs(lam[1] - lam[2]) < 1e-15
    ev[2], V[:, 2] = lam[3], U[:, 3]           # the next distinct pair: orthonormal, tiny residual, ascending
    with pytest.raises(ec.CheckError, match="eigenvalue 2"):
        ec.check_eigs(c.w, 3, ev, V, res, ref=ref)


def test_rejects_two_equal_columns(ring_ref):
    c, ref = ring_ref
    ev, V, res = _good(c, 3, ref)
    V[:, 2] = V[:, 1]
    with pytest.raises(ec.CheckError, match="V\\^T V"):
        ec.check_eigs(c.w, 3, ev, V, res, ref=ref)


def test_rejects_a_vector_rotated_out_of_its_eigenspace(ring_ref):
    c, ref = ring_ref
    lam, U, _, _ = ref
    ev, V, res = _good(c, 8, ref)
    s = 1e-6
    V[:, 3] = np.sqrt(1 - s * s) * U[:, 3] + s * U[:, 40]
    with pytest.raises(ec.CheckError):
        ec.check_eigs(c.w, 8, ev, V, res, ref=ref)


def test_rejects_a_shifted_eigenvalue(ring_ref):
    c, ref = ring_ref
    ev, V, res = _good(c, 8, ref)
    bound = np.sqrt(8) * res + 1e-13
    ev[5] += 10 * bound
    with pytest.raises(ec.CheckError):
        ec.check_eigs(c.w, 8, ev, V, res, ref=ref)


def test_rejects_wrong_zero_vectors(mix_ref):
    c, ref = mix_ref
    ev, V, res = _good(c, 5, ref)
    bad = V.copy()
    bad[:, 0] = V[:, 1]                          # two zero vectors on one component
    with pytest.raises(ec.CheckError, match="zero vector"):
        ec.check_eigs(c.w, 5, ev, bad, res, ref=ref)
    _, comp = connected_components(c.w, directed=False)
    big = int(np.bincount(comp).argmax())
    ev, V, res = _good(c, 12, ref)
    j = [jj for jj in range(12) if comp[np.flatnonzero(V[:, jj])[0]] == big][0]
    on = comp == big
    bad = V.copy()
    bad[:, j] = np.where(on, 1.0 / np.sqrt(on.sum()), 0.0)     # unit, on the right component, but not sqrt(d / vol)
    with pytest.raises(ec.CheckError, match="zero vector"):
        ec.check_eigs(c.w, 12, ev, bad, res, ref=ref)


def test_rejects_descending_order(ring_ref):
    c, ref = ring_ref
    ev, V, res = _good(c, 8, ref)
    with pytest.raises(ec.CheckError, match="ascending"):
        ec.check_eigs(c.w, 8, ev[::-1].copy(), V[:, ::-1].copy(), res, ref=ref)


def test_rejects_a_pair_of_the_wrong_component(mix_ref):
    c, ref = mix_ref
    lam, U, _, _ = ref
    k = 20
    ev, V, res = _good(c, k, ref)
    _, comp = connected_components(c.w, directed=False)
    here = np.unique(comp[np.abs(V[:, k - 1]) > 1e-8])
    # a correct eigenpair, of another component, just above the wanted range
    j = next(j for j in range(k, lam.size)
             if lam[j] - lam[k - 1] > 1e-6 and lam[j + 1] - lam[j] > 1e-9 and lam[j] - lam[j - 1] > 1e-9
             and not np.isin(np.unique(comp[np.abs(U[:, j]) > 1e-8]), here).any())
    ev[k - 1], V[:, k - 1] = lam[j], U[:, j]
    with pytest.raises(ec.CheckError, match="eigenvalue"):
        ec.check_eigs(c.w, k, ev, V, res, ref=ref)
