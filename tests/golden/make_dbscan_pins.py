"""Golden DBSCAN results from scikit-learn 1.7 (sklearn.cluster.DBSCAN, metric="euclidean"), for tests/test_dbscan_cpu.py and
tests/test_gpu_dbscan.py, which never import sklearn for them:

    python tests/golden/make_dbscan_pins.py

The data is quantised to 1/64 (float32) and eps is a multiple of 1/16, so eps^2 and every squared distance are exact in float64
whichever way they are formed: sklearn's decisions are the ones of the difference form.  sklearn runs on the float64 cast, with
algorithm="auto" and algorithm="brute"; the script asserts that both give the same labels and core samples before it writes.
Every case c stores `X_c`, `eps_c`, `min_samples_c`, `labels_c` and `core_sample_indices_c`.  Cases:
  a    make_moons(1500, noise=0.06, random_state=1), eps 0.125, min_samples 5: pairs at exactly eps
  b    make_blobs(2000, centers=6, n_features=3, cluster_std=0.6, random_state=2), eps 0.5, min_samples 8: noise and border points
  c    make_blobs(1200, centers=5, n_features=50, cluster_std=1.0, random_state=3), eps 9.0, min_samples 10: sklearn's brute path
  d    2500 uniform points on [0, 8]^2 (seed 4), eps 0.1875, min_samples 4: about 100 clusters
  e    the shuffled 3000-point spiral t (cos t, sin t) / 3, t in [0, 6 pi], sigma 0.03 (seed 5), eps 0.25, min_samples 4: one long chain
  f    the data and eps of a with min_samples 1: no noise
  g    60 uniform points (seed 6), eps 0.5, min_samples 61 > n: all noise
  h    40 copies each of 5 distinct rows, shuffled (seed 7), two of the rows exactly eps = 0.25 apart, min_samples 10: duplicates
"""
import os

import numpy as np
import sklearn
from sklearn.cluster import DBSCAN
from sklearn.datasets import make_blobs, make_moons

HERE = os.path.dirname(os.path.abspath(__file__))


def q(v):
    return (np.round(np.asarray(v, np.float64) * 64) / 64).astype(np.float32)


def main():
    assert sklearn.__version__.startswith("1.7"), sklearn.__version__
    cases = {}
    Xa = q(make_moons(1500, noise=0.06, random_state=1)[0])
    cases["a"] = (Xa, 0.125, 5)
    cases["b"] = (q(make_blobs(2000, centers=6, n_features=3, cluster_std=0.6, random_state=2)[0]), 0.5, 8)
    cases["c"] = (q(make_blobs(1200, centers=5, n_features=50, cluster_std=1.0, random_state=3)[0]), 9.0, 10)
    cases["d"] = (q(np.random.default_rng(4).uniform(0.0, 8.0, (2500, 2))), 0.1875, 4)
    rng = np.random.default_rng(5)
    t = np.linspace(0.0, 6.0 * np.pi, 3000)
    sp = np.stack([t * np.cos(t), t * np.sin(t)], axis=1) / 3.0 + rng.normal(0.0, 0.03, (3000, 2))
    cases["e"] = (q(sp[rng.permutation(3000)]), 0.25, 4)
    cases["f"] = (Xa, 0.125, 1)
    cases["g"] = (q(np.random.default_rng(6).uniform(0.0, 4.0, (60, 2))), 0.5, 61)
    rows = np.array([[0.0, 0.0, 0.0], [0.25, 0.0, 0.0], [3.0, 1.0, -2.0], [-4.0, 2.5, 1.0], [5.0, -5.0, 0.5]])
    cases["h"] = (q(np.repeat(rows, 40, axis=0)[np.random.default_rng(7).permutation(200)]), 0.25, 10)

    out = {}
    for c, (X, eps, ms) in cases.items():
        X64 = X.astype(np.float64)
        assert np.array_equal(X64 * 64, np.round(X64 * 64)) and eps * 16 == round(eps * 16)
        fits = [DBSCAN(eps=eps, min_samples=ms, metric="euclidean", algorithm=alg).fit(X64) for alg in ("auto", "brute")]
        assert np.array_equal(fits[0].labels_, fits[1].labels_), c
        assert np.array_equal(fits[0].core_sample_indices_, fits[1].core_sample_indices_), c
        lab, core = fits[0].labels_, fits[0].core_sample_indices_
        D2 = ((X64[:, None, :] - X64[None, :, :]) ** 2).sum(-1) if len(X) <= 3000 and X.shape[1] <= 3 else None
        at_eps = -1 if D2 is None else int(np.count_nonzero(np.triu(D2 == eps * eps, 1)))
        print("%-2s %4d x %-2d eps %-6g min_samples %-2d  clusters %3d  core %4d  border %4d  noise %4d  pairs at eps %d" % (
            c, X.shape[0], X.shape[1], eps, ms, lab.max() + 1, len(core), np.count_nonzero(lab >= 0) - len(core),
            np.count_nonzero(lab < 0), at_eps))
        out["X_" + c], out["eps_" + c], out["min_samples_" + c] = X, np.float64(eps), np.int64(ms)
        out["labels_" + c], out["core_sample_indices_" + c] = lab.astype(np.int32), core.astype(np.int32)
    out["sklearn_version"] = np.str_(sklearn.__version__)
    path = os.path.join(HERE, "dbscan_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")


if __name__ == "__main__":
    main()
