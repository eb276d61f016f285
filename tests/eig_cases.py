"""Seeded graphs for ``ai_eigs_smallest``, each with a complete float64 reference spectrum, and one checker.

Residual and orthogonality checks cannot see a wrong *set* of eigenpairs: single-vector Lanczos on a graph with a repeated
eigenvalue returns one copy and then the next distinct value, every residual tiny and every vector orthonormal.  Only the
whole spectrum can tell, and below a few thousand rows a dense ``numpy.linalg.eigh`` of ``ncuts_ref.laplacian_sym(w)`` gives
it cheaply; rings, tori, complete graphs and stars have it in closed form as well.

Every fixture is a float64 ``scipy.sparse.csr_matrix`` built on the CPU (point-cloud graphs through
``ncuts_ref.affinity_sparse``, never the device).  The solver branch a (case, k) reaches is restated from ``eigs_connected``
(``csrc/ai_eigs.inc``) in `branches`.
"""
from __future__ import annotations

import math
import re
from dataclasses import dataclass

import numpy as np
import scipy.sparse as sp
from scipy.sparse.csgraph import breadth_first_order, connected_components

from oracle import ncuts_ref

DENSE_ROWS = 256        # AI_EIGS_DENSE_ROWS: components up to this size are solved densely on the host
KS = (1, 2, 3, 4, 8, 32, 33, 34, 63, 64)
DEFAULT_TOL = 1e-10     # ai_ncut_opts' default tolerance


@dataclass
class Case:
    name: str
    w: sp.csr_matrix
    closed: np.ndarray | None = None          # ascending closed-form spectrum of L_sym, if there is one
    ks: tuple = ()

    @property
    def family(self) -> str:
        if any(t in self.name for t in ("_perm", "_shuffled", "_diag", "_nodiag")):
            return "variant"
        return re.match(r"[a-z]+", self.name).group(0)


# --------------------------------------------------------------------------- closed-form families
def ring(n: int, wt: float = 1.0) -> Case:
    i = np.arange(n)
    w = sp.coo_matrix((np.full(2 * n, wt), (np.r_[i, i], np.r_[(i + 1) % n, (i - 1) % n])), shape=(n, n)).tocsr()
    lam = 1.0 - (1.0 + 2.0 * wt * np.cos(2.0 * np.pi * i / n)) / (2.0 * wt + 1.0)
    return Case(f"ring{n}", w, np.sort(lam))


def torus(a: int, b: int, wt: float = 1.0) -> Case:
    idx = np.arange(a * b).reshape(a, b)
    r, c, v = [], [], []
    for da, db in ((1, 0), (-1, 0), (0, 1), (0, -1)):
        r.append(idx.ravel())
        c.append(np.roll(np.roll(idx, -da, axis=0), -db, axis=1).ravel())
    r, c = np.concatenate(r), np.concatenate(c)
    w = sp.coo_matrix((np.full(r.size, wt), (r, c)), shape=(a * b, a * b)).tocsr()
    p, q = np.meshgrid(np.arange(a), np.arange(b), indexing="ij")
    lam = 1.0 - (1.0 + 2.0 * wt * (np.cos(2 * np.pi * p / a) + np.cos(2 * np.pi * q / b))) / (4.0 * wt + 1.0)
    return Case(f"torus{a}x{b}", w, np.sort(lam.ravel()))


def complete(m: int) -> Case:
    """K_m with unit weights: W + I is all ones, so L_sym = I - J/m: 0 once, 1 with multiplicity m - 1."""
    w = sp.csr_matrix(np.ones((m, m)) - np.eye(m))
    return Case(f"complete{m}", w, np.r_[0.0, np.ones(m - 1)])


def star(m: int, wt: float = 1.0) -> Case:
    """A centre and m - 1 leaves: lambda = wt / (1 + wt) with multiplicity m - 2, 0, and the rest of the trace."""
    r = np.r_[np.zeros(m - 1, int), np.arange(1, m)]
    c = np.r_[np.arange(1, m), np.zeros(m - 1, int)]
    w = sp.coo_matrix((np.full(r.size, wt), (r, c)), shape=(m, m)).tocsr()
    theta_leaf = 1.0 / (1.0 + wt)
    theta_other = 1.0 / (1.0 + wt) + 1.0 / (1.0 + (m - 1) * wt) - 1.0     # trace of M = sum 1 / d
    lam = np.r_[0.0, np.full(m - 2, 1.0 - theta_leaf), 1.0 - theta_other]
    return Case(f"star{m}", w, np.sort(lam))


# --------------------------------------------------------------------------- point-cloud families
_SURF_CACHE: dict = {}


def _cloud(seed: int, tarl: bool, alpha: float, theta: float):
    key = (seed, tarl, alpha, theta)
    if key not in _SURF_CACHE:
        from autoinst_amd import synth
        ch = synth.synthetic_chunk(9000, seed=seed, tarl=True, extent=22.0)
        feats = ch["tarl"] if tarl else None
        A = ncuts_ref.affinity_sparse(ch["points"], feats, alpha=alpha, theta=theta if tarl else 0.0, gamma=0.0)
        _, comp = connected_components(A, directed=False)
        idx = np.flatnonzero(comp == np.bincount(comp).argmax())
        _SURF_CACHE[key] = sp.csr_matrix(A[idx][:, idx])
    return _SURF_CACHE[key]


def surface(n: int, seed: int = 0, tarl: bool = False, alpha: float = 1.0, theta: float = 0.5, name: str | None = None) -> Case:
    """A connected piece of exactly n rows of a synthetic LiDAR surface: the first n rows in breadth-first order from row 0
    of the largest component (a BFS prefix is connected), kept in their original order, diagonal 1 stored."""
    A = _cloud(seed, tarl, alpha, theta)
    if n > A.shape[0]:
        raise ValueError(f"the largest component has only {A.shape[0]} rows")
    keep = np.sort(breadth_first_order(A, 0, directed=False, return_predecessors=False)[:n])
    w = sp.csr_matrix(A[keep][:, keep])
    w.sort_indices()
    return Case(name or f"surface{n}{'_tarl' if tarl else ''}", w)


def twin(n: int, eps: float, seed: int = 0) -> Case:
    """Two copies of one surface piece, every row joined to its twin by weight eps: near-repeated pairs."""
    g = surface(n, seed).w
    link = sp.identity(n, format="csr") * eps
    w = sp.bmat([[g, link], [link, g]], format="csr")
    w.sort_indices()
    return Case(f"twin{n}_eps{eps:g}", w)


def bridge(n1: int, n2: int, eps: float) -> Case:
    """Two different surface pieces joined by ONE edge of weight eps: lambda_2 = O(eps), far below the tolerance."""
    a, b = surface(n1, seed=1).w, surface(n2, seed=2).w
    w = sp.lil_matrix(sp.block_diag([a, b], format="csr"))
    w[n1 - 1, n1] = eps
    w[n1, n1 - 1] = eps
    w = sp.csr_matrix(w)
    w.sort_indices()
    return Case(f"bridge{n1}+{n2}_eps{eps:g}", w)


def mixture() -> Case:
    """Singletons, pairs, triangles, 50 / 600 / 1100-row pieces and two identical 120-row pieces, interleaved row-wise."""
    parts = [sp.csr_matrix((1, 1)), sp.csr_matrix((1, 1)), sp.csr_matrix((1, 1)),
             sp.csr_matrix(np.array([[0.0, 0.7], [0.7, 0.0]])), sp.csr_matrix(np.array([[0.0, 0.3], [0.3, 0.0]])),
             complete(3).w, complete(3).w * 0.5,
             surface(50, seed=3).w, surface(600, seed=4).w, surface(1100, seed=5).w,
             surface(120, seed=6).w, surface(120, seed=6).w]
    w = sp.block_diag(parts, format="csr")
    # interleave: a fixed permutation, so components are not contiguous row ranges
    return Case("mixture", permute(w, seed=7))


# --------------------------------------------------------------------------- variants (the same spectrum)
def permute(w, seed: int) -> sp.csr_matrix:
    p = np.random.default_rng(seed).permutation(w.shape[0])
    out = sp.csr_matrix(w[p][:, p])
    out.sort_indices()
    return out


def shuffle_columns(w, seed: int) -> sp.csr_matrix:
    """The same matrix with every row's columns in a random order (has_sorted_indices False): the plain k_cf_spmm path."""
    w = sp.csr_matrix(w, copy=True)
    rng = np.random.default_rng(seed)
    for i in range(w.shape[0]):
        a, b = w.indptr[i], w.indptr[i + 1]
        o = rng.permutation(b - a)
        w.indices[a:b] = w.indices[a:b][o]
        w.data[a:b] = w.data[a:b][o]
    w.has_sorted_indices = False
    return w


def without_diagonal(w) -> sp.csr_matrix:
    w = sp.csr_matrix(w, copy=True)
    w.setdiag(0.0)
    w.eliminate_zeros()
    return w


def with_diagonal(w, val: float = 1.0) -> sp.csr_matrix:
    w = sp.csr_matrix(w + val * sp.identity(w.shape[0]))
    w.sort_indices()
    return w


def variant(c: Case, kind: str, seed: int = 11) -> Case:
    if kind == "perm":
        # a permuted closed form stays the same spectrum
        return Case(c.name + "_perm", permute(c.w, seed), c.closed, c.ks)
    if kind == "shuffled":
        return Case(c.name + "_shuffled", shuffle_columns(c.w, seed), c.closed, c.ks)
    if kind == "nodiag":
        return Case(c.name + "_nodiag", without_diagonal(c.w), None, c.ks)
    if kind == "diag":
        return Case(c.name + "_diag", with_diagonal(c.w), None, c.ks)
    raise ValueError(kind)


# --------------------------------------------------------------------------- the cases
def _ks(n: int, *extra) -> tuple:
    return tuple(sorted({k for k in KS + tuple(extra) if k <= n}))


def cases() -> list[Case]:
    """Every (case, k) the GPU suite runs; built on the CPU in a few seconds."""
    out = []
    def add(c, ks):
        c.ks = tuple(ks)
        out.append(c)
    add(ring(200), (2, 3, 4, 33, 64))                     # dense, every non-zero lambda double
    add(torus(12, 15), (2, 3, 5, 9, 33, 64))
    add(torus(16, 16), (3, 4, 9, 10, 33))                 # DENSE_ROWS: the last dense size, eigenvalues of multiplicity 8
    add(torus(31, 33), (2, 3, 5, 34, 64))                 # 1023 rows, ChFSI
    add(torus(32, 32), (2, 3, 4, 9, 10, 33, 34))          # 1024 rows, multiplicity 8 straddling k
    add(torus(33, 34), (3, 5, 33, 64))                    # n % 8 == 2: a partial 8-row group
    add(complete(5), (5,))                                # k == n
    add(complete(24), (1, 2, 24))
    add(star(9), (9,))
    add(star(40), (8, 40))
    add(star(2001), (3, 33, 64))                          # one row of 2000 entries; multiplicity 1999 > the block
    add(twin(500, 1e-6), (3, 8, 33))
    add(twin(750, 1e-9), (4, 34))
    add(bridge(300, 500, 1e-8), (2, 3, 8))
    add(bridge(300, 500, 1e-12), (3, 33))
    add(surface(257), (2, 3, 32, 33, 64))                 # the first ChFSI size
    add(surface(300, tarl=True), (3, 64))
    add(surface(900), (4, 33))
    add(surface(1023, tarl=True), (8, 63))
    add(surface(1500), (2, 34))
    add(surface(3000, tarl=True), (2, 32, 64))
    # weights 1e-10 .. 1; at k = 8 the block solver stagnates at a residual of ~1e-9 (CPL = 1 block of 64), an open limit
    add(surface(1200, alpha=6.0, theta=3.0, tarl=True, name="surface1200_steep"), (64,))
    m = mixture()
    add(m, (1, 3, 11, 12, 13, 20, 64))                    # 12 components: ncomp > k, = k, < k
    return out


def variants() -> list[Case]:
    """Row-permuted, column-shuffled and diagonal variants of cases in both the dense and the ChFSI range."""
    out = []
    for c, kinds, ks in ((torus(12, 15), ("perm", "shuffled", "diag"), (3, 33)),
                         (torus(33, 34), ("perm", "shuffled", "diag"), (5, 64)),
                         (surface(1500), ("shuffled", "nodiag"), (3, 34)),
                         (surface(200), ("nodiag",), (8,))):
        for kd in kinds:
            v = variant(c, kd)
            v.ks = ks
            out.append(v)
    return out


def chfsi_cases() -> list[Case]:
    """Connected cases whose every (case, k) runs the block solver (the children with other solver settings run these)."""
    return [c for c in cases() + variants()
            if connected_components(c.w, directed=False)[0] == 1 and c.w.shape[0] > DENSE_ROWS
            and any(k >= 3 for k in c.ks)]


# --------------------------------------------------------------------------- branches
def branches(w, k: int) -> set:
    """The solver each component of w reaches for k pairs (``eigs_connected`` restated): k1 = min(need, rows - 1) with
    need = k - min(k, components); no solve for k1 == 0, dense for rows <= DENSE_ROWS, else Lanczos for k1 == 1 and ChFSI
    with CPL = 1 for k1 <= 32 and CPL = 2 above."""
    ncomp, comp = connected_components(w, directed=False)
    need = k - min(k, ncomp)
    out = set()
    if need == 0:
        return out
    for size in np.bincount(comp):
        k1 = min(need, int(size) - 1)
        if k1 <= 0:
            continue
        if size <= DENSE_ROWS:
            out.add("dense")
        elif k1 == 1:
            out.add("lanczos")
        else:
            out.add("chfsi1" if k1 <= 32 else "chfsi2")
    return out


# --------------------------------------------------------------------------- reference and checker
def reference(w):
    """(lambda ascending, U, L_sym, d) by dense float64 eigh."""
    L, d = ncuts_ref.laplacian_sym(w)
    lam, U = np.linalg.eigh(L.toarray())
    return lam, U, sp.csr_matrix(L), d


def clusters(lam, sep: float):
    """[start, end) index ranges of eigenvalues no more than `sep` apart from their neighbour."""
    out, s = [], 0
    for i in range(1, lam.size + 1):
        if i == lam.size or lam[i] - lam[i - 1] > sep:
            out.append((s, i))
            s = i
    return out


class CheckError(AssertionError):
    pass


def check_eigs(w, k, evals, V, reported_resid, tol=DEFAULT_TOL, ref=None, sep: float = 1e-6):
    """Assert that (evals, V) are the k smallest eigenpairs of L_sym(w); returns a dict of the measured quantities.

    `ref` = reference(w) when the caller caches it.  Eigenvalues closer than `sep` form one cluster."""
    def need(cond, msg):
        if not cond:
            raise CheckError(msg)
    lam, U, L, d = ref if ref is not None else reference(w)
    n = w.shape[0]
    evals = np.asarray(evals, dtype=np.float64)
    V = np.asarray(V, dtype=np.float64)
    need(evals.shape == (k,) and V.shape == (n, k), f"shapes {evals.shape} {V.shape}")
    need(np.all(np.diff(evals) >= 0.0), f"eigenvalues not ascending: {evals}")
    # zero pairs: exactly 0.0, each the D^1/2 1_C / sqrt(vol_C) of one distinct component
    ncomp, comp = connected_components(w, directed=False)
    nzero = min(ncomp, k)
    need(np.all(evals[:nzero] == 0.0), f"zero pairs not exactly 0: {evals[:nzero]}")
    seen = set()
    for j in range(nzero):
        sup = np.flatnonzero(V[:, j] != 0.0)
        cs = np.unique(comp[sup])
        need(cs.size == 1 and cs[0] not in seen, f"zero vector {j} lies on components {cs} (already used: {sorted(seen)})")
        c = int(cs[0])
        seen.add(c)
        on = comp == c
        z = np.where(on, np.sqrt(np.where(on, d, 0.0) / d[on].sum()), 0.0)
        need(np.abs(V[:, j] - z).max() <= 1e-15, f"zero vector {j}: off sqrt(d / vol) by {np.abs(V[:, j] - z).max():.3e}")
    # true residuals, orthonormality
    R = L @ V - V * evals[None, :]
    res = np.linalg.norm(R, axis=0)
    rmax = float(res.max())
    need(rmax <= 10 * tol, f"true residual {rmax:.3e} above 10 tol")
    need(rmax <= 10 * max(reported_resid, 1e-14), f"true residual {rmax:.3e} above 10x the reported {reported_resid:.3e}")
    orth = float(np.abs(V.T @ V - np.eye(k)).max())
    need(orth <= 1e-10, f"|V^T V - I| = {orth:.3e}")
    # the eigenvalue set (Kahan: k orthonormal Ritz vectors with residuals r lie within sqrt(k) max r of k eigenvalues)
    bound = math.sqrt(k) * rmax + 1e-13
    err = np.abs(evals - lam[:k])
    need(err.max() <= bound, f"eigenvalue {int(err.argmax())}: {evals[err.argmax()]!r} vs {lam[err.argmax()]!r} (bound {bound:.3e})")
    # eigenspaces: a cluster inside the first k is spanned; the one straddling k lies inside its eigenspace
    worst = 0.0
    for s, e in clusters(lam, sep):
        if s >= k:
            break
        lo = lam[s] - lam[s - 1] if s > 0 else np.inf
        hi = lam[e] - lam[e - 1] if e < n else np.inf
        gap = min(lo, hi)
        Vc = V[:, s:min(e, k)]
        Uc = U[:, s:e]
        P = Vc - Uc @ (Uc.T @ Vc)
        sin = float(np.linalg.norm(P, 2)) if P.size else 0.0
        lim = 2.0 * math.sqrt(k) * rmax / gap + 1e-10
        need(sin <= lim, f"cluster [{s}, {e}) (lambda {lam[s]:.6g}): sin theta {sin:.3e} above {lim:.3e}")
        worst = max(worst, sin / lim)
    return {"eig_err": float(err.max()), "resid": rmax, "sin_frac": worst, "orth": orth}
