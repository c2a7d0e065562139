"""Golden k-means values from scikit-learn 1.7 (KMeans(algorithm="lloyd")), for tests/test_kmeans_cpu.py and
tests/test_gpu_kmeans.py, which never import sklearn for them:

    python tests/golden/make_kmeans_pins.py

Every case c stores its data as `X_<xkey_c>` (float32; sklearn runs on its float64 cast, so every backend sees the same
values), `k_c`, the run's settings (`init_c`: "k-means++", "random" or "array" with the array in `init_array_c`; `seed_c`, `n_init_c`) and sklearn's result:
`labels_c`, `centers_c`, `inertia_c`, `n_iter_c`, and the rows the kept run started from, `init_indices_c` (k-means++: from
sklearn.cluster.kmeans_plusplus with the same RandomState; random: the choice of each run replayed on one RandomState).  The
generator checks that KMeans started from those rows gives the labels of KMeans with the seed.  Cases:
  a1, a2   2000 x 50 in 12 clusters, k-means++ with seeds 0 and 1 (truth `y_a`; purity `purity_a1`, `c_purity_a1`,
           `contingency_a1` by utils_ralib's formulas over sklearn.metrics.cluster.contingency_matrix)
  ar       the same data, init="random", n_init=3, seed 5
  b        1500 x 2 in 8 clusters, k = 8, k-means++ seed 3
  e        300 x 3, an explicit init whose last centre is far from every point: exactly one cluster empty in the first iteration
  u        40 points x 3 with 5 distinct rows (integers), k = 8, k-means++ seed 0: fewer distinct labels than k
  o        500 x 1 in 4 clusters, k = 4, k-means++ seed 2
"""
import os
import warnings

import numpy as np
import sklearn
from sklearn.cluster import KMeans, kmeans_plusplus
from sklearn.metrics.cluster import contingency_matrix

HERE = os.path.dirname(os.path.abspath(__file__))


def clustered(n, d, ncl, seed, spread=4.0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (ncl, d))
    y = rng.integers(0, ncl, n)
    X = centres[y] + rng.normal(0.0, 1.0, (n, d)) * rng.uniform(0.5, 1.5, ncl)[y, None]
    return (np.round(X * 64) / 64).astype(np.float32), y.astype(np.int16)


def fit(X, k, **kw):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return KMeans(k, algorithm="lloyd", **kw).fit(X.astype(np.float64))


def plusplus_indices(X, k, seed):
    _, idx = kmeans_plusplus(X.astype(np.float64), k, random_state=np.random.RandomState(seed))
    return idx.astype(np.int64)


def random_indices(X, k, seed, n_init):
    """the runs of init="random" replayed: each run's choice, and the kept run by sklearn's rule"""
    from sklearn.cluster._k_means_common import _is_same_clustering
    rs = np.random.RandomState(seed)
    n = X.shape[0]
    best = None
    for _ in range(n_init):
        idx = rs.choice(n, size=k, replace=False, p=np.ones(n) / n).astype(np.int64)
        km = fit(X, k, init=X[idx].astype(np.float64), n_init=1)
        if best is None or (km.inertia_ < best[1] and not _is_same_clustering(km.labels_.astype(np.int32), best[0], k)):
            best = (km.labels_.astype(np.int32), km.inertia_, idx)
    return best[2], best[0]


def store(out, c, X, k, km, init, idx, seed=-1, n_init=1, init_array=None, xkey=None):
    xkey = xkey or c
    out["X_" + xkey], out["xkey_" + c], out["k_" + c] = X, np.str_(xkey), np.int64(k)
    out["init_" + c], out["seed_" + c], out["n_init_" + c] = np.str_(init), np.int64(seed), np.int64(n_init)
    if init_array is not None:
        out["init_array_" + c] = init_array
    out["labels_" + c] = km.labels_.astype(np.int16)
    out["centers_" + c] = km.cluster_centers_.astype(np.float64)
    out["inertia_" + c], out["n_iter_" + c] = np.float64(km.inertia_), np.int64(km.n_iter_)
    out["init_indices_" + c] = np.zeros(0, np.int64) if idx is None else idx
    print(c, X.shape, "k", k, init, "n_iter", km.n_iter_, "inertia %.6f" % km.inertia_, "distinct", len(set(km.labels_)))


def main():
    assert sklearn.__version__.startswith("1.7"), sklearn.__version__
    out = {}
    Xa, ya = clustered(2000, 50, 12, 11)
    out["y_a"] = ya
    for c, seed in (("a1", 0), ("a2", 1)):
        km = fit(Xa, 12, init="k-means++", n_init=1, random_state=seed)
        idx = plusplus_indices(Xa, 12, seed)
        assert np.array_equal(fit(Xa, 12, init=Xa[idx].astype(np.float64), n_init=1).labels_, km.labels_), c
        store(out, c, Xa, 12, km, "k-means++", idx, seed, xkey="a")
    M = contingency_matrix(ya, out["labels_a1"])
    out["contingency_a1"] = M.astype(np.int64)
    out["purity_a1"] = np.float64(np.sum(np.amax(M, axis=0)) / np.sum(M))
    out["c_purity_a1"] = np.float64(np.sum(np.amax(M, axis=1)) / np.sum(M))
    km = fit(Xa, 12, init="random", n_init=3, random_state=5)
    idx, lab = random_indices(Xa, 12, 5, 3)
    assert np.array_equal(lab, km.labels_)
    store(out, "ar", Xa, 12, km, "random", idx, 5, 3, xkey="a")

    Xb, _ = clustered(1500, 2, 8, 12, spread=6.0)
    km = fit(Xb, 8, init="k-means++", n_init=1, random_state=3)
    idx = plusplus_indices(Xb, 8, 3)
    assert np.array_equal(fit(Xb, 8, init=Xb[idx].astype(np.float64), n_init=1).labels_, km.labels_)
    store(out, "b", Xb, 8, km, "k-means++", idx, 3)

    Xe, _ = clustered(300, 3, 4, 13)
    C0 = np.concatenate([Xe[[0, 100, 200, 250]].astype(np.float64), np.full((1, 3), 1000.0)])
    km = fit(Xe, 5, init=C0, n_init=1)
    store(out, "e", Xe, 5, km, "array", None, init_array=C0)

    rng = np.random.default_rng(14)
    Xu = rng.integers(-3, 4, (5, 3)).astype(np.float32)[rng.integers(0, 5, 40)]
    km = fit(Xu, 8, init="k-means++", n_init=1, random_state=0)
    idx = plusplus_indices(Xu, 8, 0)
    assert np.array_equal(fit(Xu, 8, init=Xu[idx].astype(np.float64), n_init=1).labels_, km.labels_)
    assert len(set(km.labels_)) < 8
    store(out, "u", Xu, 8, km, "k-means++", idx, 0)

    Xo, _ = clustered(500, 1, 4, 15, spread=8.0)
    km = fit(Xo, 4, init="k-means++", n_init=1, random_state=2)
    idx = plusplus_indices(Xo, 4, 2)
    assert np.array_equal(fit(Xo, 4, init=Xo[idx].astype(np.float64), n_init=1).labels_, km.labels_)
    store(out, "o", Xo, 4, km, "k-means++", idx, 2)

    path = os.path.join(HERE, "kmeans_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
