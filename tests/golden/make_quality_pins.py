"""Writes tests/golden/quality_ref.npz: scikit-learn 1.7.2's trustworthiness of four small pairs (X, Y), in both directions, with the
numpy checker's rank tables.  Run from the repository root:  python tests/golden/make_quality_pins.py

Both spaces sit on a 1/1024 grid inside (-8, 8), so every term of D2 and every D2 is exact in double and equal distances are equal
bit for bit, whichever way they are formed.  sklearn's unstable argsort leaves ties undefined, so a case is kept only if
  (a) in either direction no column other than the listed entry itself has a D2 equal to a listed entry's threshold in its row,
      and the k-th and (k+1)-th neighbour distances of every row differ (the list itself is then unambiguous);
  (b) the checker's T and C equal sklearn's within 1e-12.
A seed that fails (a) is replaced by seed + 1000 and the replacement is recorded in the fixture (rejected_<case>)."""
import os
import sys

import numpy as np
import sklearn
from sklearn.manifold import trustworthiness

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.dirname(os.path.abspath(__file__)))))
from cryo_ralib_amd import quality  # noqa: E402
from cryo_ralib_amd._common import d2_rows  # noqa: E402

CASES = dict(a=(300, 8, 2, 10, 11), b=(257, 50, 2, 31, 12), c=(130, 3, 2, 64, 13), d=(60, 1, 2, 5, 14))     # n, d_X, d_Y, k, seed


def grid(v):
    return (np.clip(np.round(np.asarray(v, np.float64) * 1024), -8191, 8191) / 1024).astype(np.float32)


def make(n, dx, dy, seed):
    rng = np.random.default_rng(seed)
    # one feature: spread over the whole grid, or some l mirrors a listed j about i (|x_i - x_l| = |x_i - x_j|) in nearly every draw
    X = grid(rng.normal(size=(n, dx)) if dx > 1 else rng.uniform(-7.9, 7.9, size=(n, dx)))
    P = np.zeros((n, dy))
    P[:, :min(dx, dy)] = X[:, :min(dx, dy)]
    return X, grid(P + 0.4 * rng.normal(size=(n, dy)))


def tie_free(A, idx, k):
    """(a) for ranks in A of the lists idx, and for A's own k-th / (k+1)-th neighbours"""
    A = np.asarray(A, np.float64)
    n = A.shape[0]
    D = d2_rows(A, 0, n)
    np.fill_diagonal(D, np.inf)
    thr = np.take_along_axis(D, idx, axis=1)
    for t in range(idx.shape[1]):
        if np.any(np.count_nonzero(D == thr[:, t, None], axis=1) != 1):
            return False
    S = np.sort(D, axis=1)
    return bool(np.all(S[:, k - 1] < S[:, k]))


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = dict(sklearn_version=np.str_(sklearn.__version__), cases=np.str_("".join(sorted(CASES))))
    for c, (n, dx, dy, k, seed) in sorted(CASES.items()):
        rejected = []
        while True:
            X, Y = make(n, dx, dy, seed)
            ny, nx = quality.knn_numpy(Y, k), quality.knn_numpy(X, k)
            if tie_free(X, ny, k) and tie_free(Y, nx, k):
                break
            rejected.append(seed)
            seed += 1000
            assert len(rejected) < 40, (c, rejected)
        t = quality.trustworthiness(X, Y, k, backend="numpy", details=True)
        cc = quality.continuity(X, Y, k, backend="numpy", details=True)
        T = trustworthiness(X.astype(np.float64), Y.astype(np.float64), n_neighbors=k)
        C = trustworthiness(Y.astype(np.float64), X.astype(np.float64), n_neighbors=k)
        assert abs(t.score - T) <= 1e-12 and abs(cc.score - C) <= 1e-12, (c, t.score - T, cc.score - C)
        assert np.array_equal(t.neighbors, ny) and np.array_equal(cc.neighbors, nx)
        print("case %s: n = %d, d_X = %d, d_Y = %d, k = %d, seed %d (rejected %s): T = %.15f (checker %+.1e), C = %.15f (%+.1e)" % (
            c, n, dx, dy, k, seed, rejected, T, t.score - T, C, cc.score - C))
        out.update({"X_" + c: X, "Y_" + c: Y, "k_" + c: np.int64(k), "seed_" + c: np.int64(seed),
                    "rejected_" + c: np.asarray(rejected, np.int64), "T_" + c: np.float64(T), "C_" + c: np.float64(C),
                    "rank_t_" + c: t.ranks, "rank_c_" + c: cc.ranks})
    path = os.path.join(os.path.dirname(os.path.abspath(__file__)), "quality_ref.npz")
    np.savez_compressed(path, **out)
    print("%s: %d bytes" % (path, os.path.getsize(path)))


if __name__ == "__main__":
    main()
