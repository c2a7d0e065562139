"""Writes tests/golden/hdbscan_ref.npz: scikit-learn 1.7.2 HDBSCAN pins for cryo_ralib_amd.hdbscan.

    python tests/golden/make_hdbscan_pins.py

sklearn.cluster.HDBSCAN(min_cluster_size, min_samples, cluster_selection_method, allow_single_cluster=False, copy=True) is fitted
on X.astype(float64) with algorithm="brute" and with algorithm="kd_tree".  All data lies on a 1/1024 grid with |x| <= 16:
differences, squares and sums are exact in double up to d = 2048, so fused and unfused arithmetic agree bit for bit and the device
must equal the numpy checker.

sklearn's labels depend on the order an unstable argsort gives equal weights (hdbscan.py's docstring); the contract differs from
them on the tie set T of rule 9 only.  For every case and both algorithms this script ASSERTS
  - the partition outside T equals sklearn's (labels up to a renaming of the ids, noise to noise),
  - |T| <= 3 % of n,
  - probabilities outside T within max(1000 x the brute-vs-kd_tree discrepancy outside T, 1e-12) of sklearn's.
A seed that fails an assertion is replaced, never excused.  The file records T and the discrepancy.

Per case c: X_c, min_cluster_size_c, min_samples_c (-1 for None), method_c, labels_c / probabilities_c / tie_mask_c (the numpy
checker's), sk_labels_brute_c, sk_labels_kd_c, sk_prob_brute_c, sk_prob_kd_c, discrepancy_c.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import HDBSCAN

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
from cryo_ralib_amd import hdbscan  # noqa: E402


def grid(v):
    return (np.clip(np.round(np.asarray(v, np.float64) * 1024), -16 * 1024, 16 * 1024) / 1024).astype(np.float32)


def islands(n, seed):
    """three Gaussian islands of spread 0.3, 1.0 and 0.1 plus 10 % uniform scatter"""
    rng = np.random.default_rng(seed)
    ns = n // 10
    m = n - ns
    sizes = [m // 2, m // 3, m - m // 2 - m // 3]
    centres, sig = np.array([[-5.0, -2.0], [4.0, 3.0], [2.0, -6.0]]), (0.3, 1.0, 0.1)
    parts = [centres[j] + sig[j] * rng.normal(size=(sizes[j], 2)) for j in range(3)]
    parts.append(rng.uniform(-10.0, 10.0, (ns, 2)))
    return grid(np.concatenate(parts)[rng.permutation(n)])


def arcs(n, seed):
    """two arcs (half circles) of different noise"""
    rng = np.random.default_rng(seed)
    na = n // 2
    t1, t2 = rng.uniform(0, np.pi, na), rng.uniform(0, np.pi, n - na)
    a = np.stack([4 * np.cos(t1), 4 * np.sin(t1)], 1) + 0.1 * rng.normal(size=(na, 2))
    b = np.stack([4 - 4 * np.cos(t2), 2 - 4 * np.sin(t2)], 1) + 0.4 * rng.normal(size=(n - na, 2))
    return grid(np.concatenate([a, b])[rng.permutation(n)])


def factors(n, seed, d=8):
    """five clusters in d = 8 with spreads 0.3 .. 1.9"""
    rng = np.random.default_rng(seed)
    c = rng.normal(0.0, 4.0, (5, d))
    which = rng.integers(0, 5, n)
    sig = np.linspace(0.3, 1.9, 5)
    return grid(c[which] + sig[which, None] * rng.normal(size=(n, d)))


# name: generator, n, seed, min_cluster_size, min_samples, method
CASES = [
    ("a", islands, 600, 1, 15, 5, "eom"),
    ("b", islands, 1500, 2, 25, 10, "eom"),
    ("c", arcs, 500, 3, 10, None, "eom"),
    ("d", arcs, 130, 12, 5, 5, "eom"),
    ("e", factors, 700, 5, 20, 5, "eom"),
    ("f", factors, 1200, 16, 10, 3, "eom"),
    ("g", factors, 65, 7, 5, 3, "eom"),
    ("h", islands, 300, 8, 10, 1, "eom"),
    ("i", islands, 600, 9, 15, 5, "leaf"),
]


def same_partition(a, b):
    """a and b give the same partition: noise to noise, and a bijection between the cluster ids"""
    if not np.array_equal(a < 0, b < 0):
        return False
    pairs = np.unique(np.stack([a, b], 1), axis=0)
    return len(np.unique(pairs[:, 0])) == len(pairs) == len(np.unique(pairs[:, 1]))


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = {"cases": np.array([c[0] for c in CASES])}
    for name, gen, n, seed, mcs, ms, method in CASES:
        X = gen(n, seed)
        assert np.all(np.abs(X) <= 16) and np.array_equal(X * 1024, np.round(X * 1024))
        r = hdbscan.hdbscan(X, mcs, ms, method, backend="numpy")
        T = r.tie_mask
        sk = {}
        for alg in ("brute", "kd_tree"):
            sk[alg] = HDBSCAN(min_cluster_size=mcs, min_samples=ms, cluster_selection_method=method, algorithm=alg,
                              allow_single_cluster=False, copy=True).fit(X.astype(np.float64))
        disc = float(np.abs(sk["brute"].probabilities_ - sk["kd_tree"].probabilities_)[~T].max())
        bound = max(1000 * disc, 1e-12)
        assert T.sum() <= 0.03 * n, (name, int(T.sum()))
        for alg in ("brute", "kd_tree"):
            assert same_partition(r.labels[~T], sk[alg].labels_[~T]), (name, alg, "partition outside T")
            err = float(np.abs(r.probabilities - sk[alg].probabilities_)[~T].max())
            assert err <= bound, (name, alg, err, bound)
        assert r.n_clusters >= 2, name
        print("case %s: n = %d, d = %d, min_cluster_size = %d, min_samples = %s, %s: %d clusters, %d noise, |T| = %d, brute-vs-kd_tree "
              "discrepancy %.3g" % (name, n, X.shape[1], mcs, ms, method, r.n_clusters, r.n_noise, int(T.sum()), disc))
        out.update({"X_" + name: X, "min_cluster_size_" + name: np.int64(mcs), "min_samples_" + name: np.int64(-1 if ms is None else ms),
                    "method_" + name: np.str_(method), "labels_" + name: r.labels, "probabilities_" + name: r.probabilities,
                    "tie_mask_" + name: T, "sk_labels_brute_" + name: sk["brute"].labels_.astype(np.int32),
                    "sk_labels_kd_" + name: sk["kd_tree"].labels_.astype(np.int32), "sk_prob_brute_" + name: sk["brute"].probabilities_,
                    "sk_prob_kd_" + name: sk["kd_tree"].probabilities_, "discrepancy_" + name: np.float64(disc)})
    np.savez_compressed(os.path.join(HERE, "hdbscan_ref.npz"), **out)


if __name__ == "__main__":
    main()
