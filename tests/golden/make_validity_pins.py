"""Golden cluster-validity values from scikit-learn 1.7 (sklearn.metrics, metric="euclidean"), for tests/test_validity_cpu.py and
tests/test_gpu_validity.py, which never import sklearn for them:

    python tests/golden/make_validity_pins.py

The data is quantised to 1/64 (float32) and sklearn runs on its float64 cast: products and sums of such values are exact in
float64, so sklearn's Gram expansion of the pair distances gives what the difference form gives (the generator prints the largest
deviation of the two; it is 0.0 on every case).  Every case c stores `X_c`, `labels_c` (values in 0 .. k - 1), `k_c` and sklearn's
`silhouette_samples_c`, `silhouette_score_c`, `calinski_harabasz_score_c`, `davies_bouldin_score_c`.  Cases:
  a    700 x 50 in 5 clusters, labelled by KMeans with k = 7 (seed 0)
  b    600 x 2 in 8 clusters, KMeans k = 8
  o    300 x 1 in 4 clusters, KMeans k = 4
  s    300 x 3 in 4 clusters with +1000 on every coordinate, KMeans k = 4: large norms, small distances
  u    the data of b labelled by KMeans k = 7 with the ids from 3 on moved up by one: k = 8 with id 3 unused
  g    300 x 3 in 4 clusters, KMeans k = 4, and row 0 a cluster of its own (id 4, k = 5): a singleton
  d    120 x 3, planted labels, k = 3: cluster 0 is 30 copies of one row (a = 0), cluster 1 holds 10 duplicated rows
  t    3 x 2, labels 0 0 1: n = 3, m = 2
  ss   the data and labels of a with sample_size = 200, random_state = 3: `silhouette_score_ss` alone (the permutation rule)
"""
import os
import warnings

import numpy as np
import sklearn
from sklearn.cluster import KMeans
from sklearn.metrics import calinski_harabasz_score, davies_bouldin_score, silhouette_samples, silhouette_score

HERE = os.path.dirname(os.path.abspath(__file__))


def clustered(n, d, ncl, seed, spread=4.0):
    rng = np.random.default_rng(seed)
    centres = rng.normal(0.0, spread, (ncl, d))
    y = rng.integers(0, ncl, n)
    X = centres[y] + rng.normal(0.0, 1.0, (n, d)) * rng.uniform(0.5, 1.5, ncl)[y, None]
    return (np.round(X * 64) / 64).astype(np.float32), y.astype(np.int16)


def km_labels(X, k, seed=0):
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")
        return KMeans(k, algorithm="lloyd", random_state=seed, n_init=1).fit(X.astype(np.float64)).labels_.astype(np.int16)


def difference_form(X, labels):
    """silhouette_samples in float64 from x_i - x_j, to compare with sklearn's Gram expansion"""
    X = X.astype(np.float64)
    ids, lab = np.unique(labels, return_inverse=True)
    D = np.sqrt(((X[:, None, :] - X[None, :, :]) ** 2).sum(-1))
    cnt = np.bincount(lab)
    S = np.stack([D[:, lab == c].sum(1) for c in range(len(ids))], axis=1)
    rows = np.arange(len(X))
    with np.errstate(divide="ignore", invalid="ignore"):
        a = S[rows, lab] / (cnt[lab] - 1)
        M = S / cnt
        M[rows, lab] = np.inf
        b = M.min(1)
        return np.nan_to_num((b - a) / np.maximum(a, b))


def main():
    assert sklearn.__version__.startswith("1.7"), sklearn.__version__
    cases = {}
    Xa, _ = clustered(700, 50, 5, 11)
    cases["a"] = (Xa, km_labels(Xa, 7), 7)
    Xb, _ = clustered(600, 2, 8, 12, spread=6.0)
    cases["b"] = (Xb, km_labels(Xb, 8), 8)
    Xo, _ = clustered(300, 1, 4, 13, spread=8.0)
    cases["o"] = (Xo, km_labels(Xo, 4), 4)
    Xs, _ = clustered(300, 3, 4, 14)
    cases["s"] = ((Xs + np.float32(1000.0)).astype(np.float32), km_labels(Xs, 4), 4)
    lu = km_labels(Xb, 7, seed=1)
    cases["u"] = (Xb, (lu + (lu >= 3)).astype(np.int16), 8)
    Xg, _ = clustered(300, 3, 4, 15)
    lg = km_labels(Xg, 4)
    lg[0] = 4
    cases["g"] = (Xg, lg, 5)
    rng = np.random.default_rng(16)
    q = lambda v: (np.round(v * 64) / 64).astype(np.float32)
    c1 = q(rng.normal(3.0, 1.0, (30, 3)))
    c1 = np.concatenate([c1, c1[:10]])
    Xd = np.concatenate([np.repeat(q(rng.normal(-3.0, 1.0, (1, 3))), 30, axis=0), c1, q(rng.normal(0.0, 1.0, (50, 3)) + [0, 6, 0])])
    ld = np.concatenate([np.zeros(30), np.ones(40), np.full(50, 2)]).astype(np.int16)
    perm = rng.permutation(120)
    cases["d"] = (Xd[perm], ld[perm], 3)
    cases["t"] = (np.array([[0.0, 0.0], [1.0, 0.5], [4.0, 3.0]], np.float32), np.array([0, 0, 1], np.int16), 2)

    out = {}
    for c, (X, lab, k) in cases.items():
        X64 = X.astype(np.float64)
        assert np.array_equal(X64 * 64, np.round(X64 * 64)) and lab.min() >= 0 and lab.max() < k
        sv = silhouette_samples(X64, lab, metric="euclidean")
        print("%-2s %4d x %-2d k = %d  silhouette %.6f  sklearn vs difference form %.1e" % (
            c, X.shape[0], X.shape[1], k, sv.mean(), np.abs(sv - difference_form(X, lab)).max()))
        out["X_" + c], out["labels_" + c], out["k_" + c] = X, lab, np.int64(k)
        out["silhouette_samples_" + c] = sv
        out["silhouette_score_" + c] = np.float64(silhouette_score(X64, lab, metric="euclidean"))
        out["calinski_harabasz_score_" + c] = np.float64(calinski_harabasz_score(X64, lab))
        out["davies_bouldin_score_" + c] = np.float64(davies_bouldin_score(X64, lab))
    out["silhouette_score_ss"] = np.float64(silhouette_score(Xa.astype(np.float64), cases["a"][1], metric="euclidean", sample_size=200,
                                                             random_state=3))
    out["sample_size_ss"], out["random_state_ss"] = np.int64(200), np.int64(3)
    out["sklearn_version"] = np.str_(sklearn.__version__)
    path = os.path.join(HERE, "validity_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
