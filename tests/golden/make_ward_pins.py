"""Golden Ward trees from scipy 1.15.3 (scipy.cluster.hierarchy.ward) and cuts from scikit-learn 1.7.2
(AgglomerativeClustering(linkage="ward")), for tests/test_ward_cpu.py and tests/test_gpu_ward.py, which never import either:

    python tests/golden/make_ward_pins.py

Both run on the float64 cast of the float32 data (tests/ward_cases.pin_inputs).  Every case c stores `X_c`, `Z_c` (scipy's
linkage), `labels_c` [len(ks_c)][n] with `ks_c` (the k of {2, 5, 17} that are <= n), and `thresholds_c` [2] with `tlabels_c`
[2][n]: sklearn's labels for two distance_threshold cuts placed midway between two consecutive heights (at a third and at two
thirds of the merge list).  Cases:
  gauss2    300 x 2 Gaussian
  gauss5    1000 x 5 Gaussian
  blobs50   600 x 50, eight blobs
  islands   2500 x 2, three islands of spread 0.3, 1.0 and 0.1 plus 10 % uniform scatter
  two       n = 2
  three     n = 3
A pin is written only for inputs on which the reference itself is unambiguous: the script asserts that the numpy checker
(ward.linkage(backend="numpy", details=True)) reports margin >= 1e-9 and height_gap >= 1e-9 and that its merge list equals
scipy's.  Fused and unfused chains differ by at most about (d + 8) 2^-52 kappa with kappa = |c|^2 / D2 <= 1e4 for these
generators: below 1e-10 for d <= 128, so no decision of the device can differ from the checker's on these inputs.  If a seed
fails, pick another.
"""
import os
import sys

import numpy as np
import scipy
import sklearn
from scipy.cluster.hierarchy import ward as scipy_ward
from sklearn.cluster import AgglomerativeClustering

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from cryo_ralib_amd import ward  # noqa: E402
import ward_cases  # noqa: E402


def main():
    assert scipy.__version__ == "1.15.3" and sklearn.__version__ == "1.7.2", (scipy.__version__, sklearn.__version__)
    out = {}
    for c, X in ward_cases.pin_inputs().items():
        n = len(X)
        X64 = X.astype(np.float64)
        Z = scipy_ward(X64)
        tree = ward.linkage(X, backend="numpy", details=True)
        assert tree.margin >= ward_cases.MARGIN and tree.height_gap >= ward_cases.MARGIN, (c, tree.margin, tree.height_gap)
        assert np.array_equal(tree.Z[:, :2], Z[:, :2]) and np.array_equal(tree.Z[:, 3], Z[:, 3]), c
        rel = float(np.max(np.abs(tree.heights - Z[:, 2]) / Z[:, 2]))
        ks = [k for k in ward_cases.PIN_KS if k <= n]
        labels = np.stack([AgglomerativeClustering(n_clusters=k, linkage="ward").fit(X64).labels_ for k in ks]).astype(np.int32)
        h = Z[:, 2]
        at = sorted({min(max((n - 1) // 3, 1), n - 2), min(max(2 * (n - 1) // 3, 1), n - 2)}) if n > 2 else [0]
        thr = np.array([0.5 * (h[r - 1] + h[r]) if n > 2 else 0.5 * h[0] for r in at] + ([1.5 * h[-1]] if len(at) < 2 else []))
        tl = []
        for t in thr:
            fit = AgglomerativeClustering(n_clusters=None, distance_threshold=float(t), linkage="ward").fit(X64)
            assert fit.n_clusters_ == int(np.count_nonzero(h >= t)) + 1, c
            tl.append(fit.labels_)
        out["X_" + c], out["Z_" + c], out["ks_" + c], out["labels_" + c] = X, Z, np.array(ks, np.int64), labels
        out["thresholds_" + c], out["tlabels_" + c] = thr, np.stack(tl).astype(np.int32)
        print("%-8s %4d x %-2d rounds %3d  rows / n %.2f  margin %.2e  height gap %.2e  heights vs scipy %.2e  thresholds -> %s clusters" % (
            c, n, X.shape[1], tree.n_rounds, tree.rows_evaluated / n, tree.margin, tree.height_gap, rel,
            [int(np.count_nonzero(h >= t)) + 1 for t in thr]))
    out["scipy_version"], out["sklearn_version"] = np.str_(scipy.__version__), np.str_(sklearn.__version__)
    path = os.path.join(HERE, "ward_ref.npz")
    np.savez_compressed(path, **out)
    print(path, os.path.getsize(path), "bytes")
    assert os.path.getsize(path) < 500 * 1024


if __name__ == "__main__":
    main()
