"""Writes tests/golden/gmm_ref.npz: scikit-learn 1.7 GaussianMixture results on small anisotropic, rotated blobs of unequal
weights, for tests/test_gmm_cpu.py and tests/test_gpu_gmm.py (which never import sklearn).

    python tests/golden/make_gmm_pins.py

The data are float32 rounded to 1 / 64 (stored as int16 = 64 x); sklearn is fed their float64 cast.  For every case the generator
asserts that no iteration's |change| of the lower bound lies within 1e-6 of tol (so n_iter is a fair exact comparison) and that
the float64 numpy backend reproduces sklearn's n_iter_, converged_, labels and k-means start.  It stores sklearn's results, the
measured numpy-vs-sklearn discrepancy of every pinned array, and the bars tol_<name> = max(1000 x discrepancy, 1e-12 x scale)
that both backends are held to.
"""
import os
import sys
import warnings

import numpy as np
from sklearn.cluster import KMeans
from sklearn.mixture import GaussianMixture

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cryo_ralib_amd import gmm  # noqa: E402

TOL = 1e-3
#        name       n     d   k  cov     init      n_init max_iter data-seed fit-seed
CASES = [("full3", 600, 3, 4, "full", "kmeans", 1, 100, 1, 0),
         ("diag3", 600, 3, 4, "diag", "kmeans", 1, 100, 1, 0),
         ("full16", 2000, 16, 6, "full", "kmeans", 1, 100, 2, 1),
         ("diag50", 2000, 50, 8, "diag", "kmeans", 1, 100, 3, 2),
         ("full33", 1500, 33, 5, "full", "kmeans", 1, 100, 4, 3),
         ("full1", 300, 1, 3, "full", "kmeans", 1, 100, 5, 4),
         ("random3", 600, 3, 4, "full", "random", 3, 100, 1, 5),
         ("maxiter5", 2000, 16, 6, "diag", "random", 1, 5, 2, 6)]


def blobs(n, d, k, seed):
    """k anisotropic Gaussians with random rotations, axis scales over a decade and weights 1 : 2 : 4 : ..., rounded to 1 / 64"""
    rng = np.random.default_rng(seed)
    w = 2.0 ** np.arange(k)
    w /= w.sum()
    counts = np.maximum(d + 2, np.floor(w * n).astype(int))
    counts[-1] += n - counts.sum()
    parts = []
    for c in range(k):
        Q, _ = np.linalg.qr(rng.standard_normal((d, d)))
        scales = np.logspace(-0.5, 0.5, d)[rng.permutation(d)] if d > 1 else np.array([0.6])
        centre = rng.standard_normal(d) * 3.0 / np.sqrt(d) + (c * 2.5 if d == 1 else 0.0)
        parts.append(centre + (rng.standard_normal((counts[c], d)) * scales) @ Q.T)
    X = np.concatenate(parts)[rng.permutation(n)]
    q = np.clip(np.round(X * 64.0), -32767, 32767).astype(np.int16)
    return q


def main():
    out = {"names": np.array([c[0] for c in CASES])}
    for name, n, d, k, cov, init, n_init, max_iter, dseed, seed in CASES:
        q = blobs(n, d, k, dseed)
        X32 = q.astype(np.float32) / np.float32(64.0)
        X = X32.astype(np.float64)
        with warnings.catch_warnings():
            warnings.simplefilter("ignore")
            sk = GaussianMixture(n_components=k, covariance_type=cov, tol=TOL, reg_covar=1e-6, max_iter=max_iter, n_init=n_init,
                                 init_params=init, random_state=seed).fit(X)
            mine = gmm.gmm(X32, k, covariance_type=cov, tol=TOL, reg_covar=1e-6, max_iter=max_iter, n_init=n_init, init_params=init,
                           random_state=seed, backend="numpy")
        for hist in (np.asarray(sk.lower_bounds_), mine.lower_bounds):
            change = np.abs(np.diff(np.concatenate([[-np.inf], hist])))
            gap = np.min(np.abs(change - TOL))
            assert gap > 1e-6, (name, gap)
        labels = sk.predict(X)
        assert mine.n_iter == sk.n_iter_ and mine.converged == sk.converged_, (name, mine.n_iter, sk.n_iter_)
        assert np.array_equal(mine.labels, labels), name
        if init == "kmeans":
            km = KMeans(n_clusters=k, n_init=1, random_state=np.random.RandomState(seed)).fit(X).labels_
            assert np.array_equal(km, mine.init_labels), name
        pins = dict(means=sk.means_, covariances=sk.covariances_, weights=sk.weights_, lower_bound=np.float64(sk.lower_bound_),
                    score_samples=sk.score_samples(X), bic=np.float64(sk.bic(X)), aic=np.float64(sk.aic(X)))
        got = dict(means=mine.means, covariances=mine.covariances, weights=mine.weights, lower_bound=np.float64(mine.lower_bound),
                   score_samples=gmm.score_samples(X32, mine, backend="numpy"), bic=np.float64(gmm.bic(X32, mine, backend="numpy")),
                   aic=np.float64(gmm.aic(X32, mine, backend="numpy")))
        out[name + "_x64"] = q
        out[name + "_opts"] = np.array([k, n_init, max_iter, seed], np.int64)
        out[name + "_cov"], out[name + "_init"] = np.str_(cov), np.str_(init)
        out[name + "_labels"] = labels.astype(np.int16)
        out[name + "_init_labels"] = (mine.init_labels if mine.init_labels is not None else np.zeros(0)).astype(np.int16)
        out[name + "_n_iter"], out[name + "_converged"] = np.int64(sk.n_iter_), np.bool_(sk.converged_)
        line = "%-9s n_iter %3d converged %d gap %.2e" % (name, sk.n_iter_, sk.converged_, gap)
        for key, want in pins.items():
            disc = float(np.max(np.abs(np.asarray(got[key]) - want)))
            scale = float(np.max(np.abs(want)))
            out["%s_%s" % (name, key)] = want
            out["%s_disc_%s" % (name, key)] = np.float64(disc)
            out["%s_tol_%s" % (name, key)] = np.float64(max(1000.0 * disc, 1e-12 * scale))
            line += " %s %.1e" % (key[:5], disc)
        print(line)
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "gmm_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
