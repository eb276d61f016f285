"""Writes tests/golden/dbscan_sklearn.npz: seeded clouds with scikit-learn's own DBSCAN labels (CPU only, needs scikit-learn).

    python tests/tools/gen_dbscan_golden.py

Per cloud k: ``points_k`` (float64), ``eps_k``, ``min_samples_k``, ``labels_k`` (``sklearn.cluster.DBSCAN(eps, min_samples)
.fit(points).labels_``), ``margin_k`` and ``name_k``; plus ``n_clouds`` and the scikit-learn / NumPy versions.

The golden must not depend on anyone's rounding of a distance: the generator asserts that no pair of a cloud has
|d^2 - eps^2| <= 1e-9 * eps^2 and records the smallest margin.  The lattice clouds are the exception: their coordinates are
multiples of 0.25 and eps is 0.5, so every d^2 and eps^2 is exact in binary and the pairs at exactly eps are exact ties
(margin 0 is recorded for them).
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]


def blobs(rng, n, k, spread, noise_frac):
    centres = rng.uniform(-6, 6, (k, 3))
    p = centres[rng.integers(0, k, n)] + rng.normal(0, spread, (n, 3))
    m = int(noise_frac * n)
    p[:m] = rng.uniform(-9, 9, (m, 3))
    return p[rng.permutation(n)]


def lattice(rng, keep):
    g = np.stack(np.meshgrid(np.arange(8), np.arange(8), np.arange(3), indexing="ij"), -1).reshape(-1, 3) * 0.5
    return g[rng.permutation(len(g))][:keep].astype(np.float64)


def margin_of(p, eps):
    d = p[:, None, :] - p[None, :, :]
    d2 = (d[..., 0] * d[..., 0] + d[..., 1] * d[..., 1]) + d[..., 2] * d[..., 2]
    return float(np.abs(d2 - eps * eps).min() / (eps * eps))


def main():
    import sklearn
    from sklearn.cluster import DBSCAN
    rng = np.random.default_rng(20251020)
    clouds = []
    for name, n, k, spread, noise, eps, ms in (("blobs_a", 1500, 6, 0.6, 0.10, 0.7, 20), ("blobs_b", 1200, 9, 0.4, 0.15, 0.5, 3),
                                                ("blobs_c", 900, 4, 0.3, 0.20, 0.3, 1), ("blobs_d", 1400, 5, 0.8, 0.05, 0.7, 3),
                                                ("blobs_e", 700, 3, 0.5, 0.10, 0.5, 20), ("blobs_f", 257, 2, 0.3, 0.10, 0.3, 3)):
        clouds.append((name, blobs(rng, n, k, spread, noise), eps, ms, False))
    p = blobs(rng, 1000, 5, 0.5, 0.1)
    clouds.append(("duplicates", np.concatenate([p, p[:150], p[:40]])[rng.permutation(1190)], 0.5, 3, False))
    p = blobs(rng, 600, 3, 0.4, 0.1)
    clouds.append(("duplicates_ms20", np.concatenate([p, p[:300]]), 0.7, 20, False))
    lat = lattice(rng, 150)
    for ms in (1, 3, 20):
        clouds.append((f"lattice_ms{ms}", lat, 0.5, ms, True))
    out = {"n_clouds": np.int64(len(clouds)), "sklearn_version": np.str_(sklearn.__version__), "numpy_version": np.str_(np.__version__)}
    for k, (name, p, eps, ms, exact) in enumerate(clouds):
        p = np.ascontiguousarray(p, dtype=np.float64)
        assert p.shape[0] <= 1500
        m = margin_of(p, eps)
        if exact:
            assert np.array_equal(p * 4, np.round(p * 4)) and eps == 0.5, "lattice coordinates must be multiples of 0.25"
            d = p[:, None, :] - p[None, :, :]
            assert int(((d * d).sum(-1) == 0.25).sum()) > 0, "the lattice must have pairs at exactly eps"
            m = 0.0
        else:
            assert m > 1e-9, (name, m)
        labels = DBSCAN(eps=eps, min_samples=ms).fit(p).labels_.astype(np.int32)
        out.update({f"name_{k}": np.str_(name), f"points_{k}": p, f"eps_{k}": np.float64(eps), f"min_samples_{k}": np.int32(ms),
                    f"labels_{k}": labels, f"margin_{k}": np.float64(m)})
        print(f"{name}: n={p.shape[0]} eps={eps} min_samples={ms} clusters={labels.max() + 1} noise={(labels < 0).sum()} margin={m:.2e}")
    path = os.path.join(ROOT, "tests", "golden", "dbscan_sklearn.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
