"""Golden spectral embeddings from scikit-learn 1.7.2 (SpectralEmbedding / SpectralClustering with affinity="nearest_neighbors") and
from the literal dense definition (spectral.dense_numpy), for tests/test_spectral_cpu.py and tests/test_gpu_spectral.py, which
never import sklearn:

    python tests/golden/make_spectral_pins.py

sklearn runs on the float64 cast of the float32 data (tests/spectral_cases.pin_cases), with eigen_tol=1e-12.  Every case c stores
`X_c` (selftune and alpha1 use X_gauss3), `dense_E_c` [n][comp] (dense_numpy's embedding), `theta_c` [comp], `gap_c` [comp] (the distance from theta_t to the nearest
other eigenvalue of the WHOLE spectrum of M, the trivial 1 included), `dense_res_c` [comp] (the residual of the dense eigenpair
itself: the reference's own error) and, for the cases sklearn has a counterpart of, `sk_E_c` (its embedding_), `sk_res_c` [comp]
(the residual |M y - (y.My) y| of its unit vectors) and its symmetrised graph without the diagonal (`sk_indptr_c`, `sk_indices_c`
int16, `sk_twice_c` uint8 = 2 a_ij).  Cases:
  gauss3    400 x 3 Gaussian, n_neighbors 10, 5 components
  gauss5    1500 x 5 Gaussian, n_neighbors 15, 4 components
  ring      1200-point noisy, unevenly sampled ring in 2-D, n_neighbors 12, 4 components
  blobs50   600 x 50, eight overlapping blobs, n_neighbors 15, 4 components
  selftune  gauss3's data, affinity="gaussian", local_scale 7 (no sklearn counterpart: pinned to dense_numpy only)
  alpha1    gauss3's data, alpha = 1 (no sklearn counterpart)
and `arcs_X`, `arcs_labels`: sklearn's SpectralClustering partition of two interleaved arcs into 2 classes.

These are conditions on the inputs, asserted here, not measurements: the graph is connected; the neighbour lists have no tie at the
last place (D2 margin >= 1e-9); min gap >= 1e-4; sklearn's unit vectors lie within 2 r_t / gap_t + n 2^-52 of the dense ones; the
arcs partition is the same for three random_states.  If a seed fails, pick another.  Gaps found with the seeds of
spectral_cases.pin_cases (smallest per case): gauss3 3.3e-03, gauss5 2.2e-03, ring 2.8e-04, blobs50 1.6e-02, selftune 2.9e-03,
alpha1 4.1e-03; the least neighbour margin is the ring's, 7.5e-09.
"""
import os
import sys

import numpy as np
import sklearn
from sklearn.cluster import SpectralClustering
from sklearn.manifold import SpectralEmbedding

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
sys.path.insert(0, os.path.dirname(HERE))
from cryo_ralib_amd import spectral, tsne  # noqa: E402
import spectral_cases as sc  # noqa: E402


def knn_margin(X, n_neighbors):
    k = n_neighbors - 1
    if k + 1 > len(X) - 1:
        return np.inf
    _, d2 = tsne.knn_numpy(X, k + 1)
    return float(np.min(d2[:, k] - d2[:, k - 1]))


def main():
    assert sklearn.__version__ == "1.7.2", sklearn.__version__
    out = {}
    for c, (X, opt, with_sklearn) in sc.pin_cases().items():
        n, comp = len(X), opt["n_components"]
        gopt = sc.graph_options(opt)
        indptr, indices, a, component = spectral.graph(X, backend="numpy", **gopt)
        assert component.max() == 0, c
        margin = knn_margin(X, opt["n_neighbors"])
        assert margin >= sc.KNN_MARGIN, (c, margin)
        E, theta, Y, spectrum = spectral.dense_numpy(indptr, indices, a, comp)
        gap = np.array([np.min(np.abs(np.delete(spectrum, t + 1) - theta[t])) for t in range(comp)])
        assert gap.min() >= sc.MIN_GAP, (c, gap)
        op = spectral._NumpyOperator(indptr, indices, a)
        dres = op.residuals(Y, theta)
        out["dense_E_" + c], out["theta_" + c], out["gap_" + c], out["dense_res_" + c] = E, theta, gap, dres
        if with_sklearn:                                        # selftune and alpha1 run on X_gauss3
            out["X_" + c] = X
        line = "%-8s %4d x %-2d  gap %.2e  knn margin %.2e  dense residual %.1e" % (c, n, X.shape[1], gap.min(), margin, dres.max())
        if with_sklearn:
            se = SpectralEmbedding(comp, affinity="nearest_neighbors", n_neighbors=opt["n_neighbors"], eigen_tol=1e-12, random_state=0)
            E_sk = se.fit(X.astype(np.float64)).embedding_
            A = se.affinity_matrix_.tocsr().copy()
            A.setdiag(0.0)
            A.eliminate_zeros()
            A.sort_indices()
            assert np.array_equal(A.indptr, indptr) and np.array_equal(A.indices, indices) and np.array_equal(A.data, a), c
            Ysk = sc.unit_vectors(E_sk, op.s)
            th_sk = np.array([y @ op.mv(y) for y in Ysk])
            rsk = op.residuals(Ysk, th_sk)
            diff = np.linalg.norm(Ysk - sc.unit_vectors(E, op.s), axis=1)
            assert np.all(diff <= sc.vector_bound(rsk, gap, n)), (c, diff, sc.vector_bound(rsk, gap, n))
            out["sk_E_" + c], out["sk_res_" + c] = E_sk, rsk
            out["sk_indptr_" + c], out["sk_indices_" + c] = A.indptr.astype(np.int32), A.indices.astype(np.int16)
            out["sk_twice_" + c] = np.round(2.0 * A.data).astype(np.uint8)
            line += "  sklearn residual %.1e  |sklearn - dense| %.1e" % (rsk.max(), diff.max())
        print(line)
    X, truth = sc.arcs(sc.ARCS["n"], sc.ARCS["seed"], sc.ARCS["noise"])
    _, _, _, component = spectral.graph(X, n_neighbors=sc.ARCS["n_neighbors"], backend="numpy")
    assert component.max() == 0 and knn_margin(X, sc.ARCS["n_neighbors"]) >= sc.KNN_MARGIN
    labs = [SpectralClustering(2, affinity="nearest_neighbors", n_neighbors=sc.ARCS["n_neighbors"], random_state=s)
            .fit(X.astype(np.float64)).labels_ for s in (0, 1, 2)]
    assert all(sc.same_partition(labs[0], l) for l in labs[1:])
    print("arcs     %4d x 2   agreement with the truth %.3f" % (len(X), max(np.mean(labs[0] == truth), np.mean(labs[0] != truth))))
    out["arcs_X"], out["arcs_labels"] = X, labs[0].astype(np.int32)
    out["sklearn_version"] = np.str_(sklearn.__version__)
    np.savez_compressed(sc.GOLDEN, **out)
    print(sc.GOLDEN, os.path.getsize(sc.GOLDEN), "bytes")
    assert os.path.getsize(sc.GOLDEN) < 500 * 1024


if __name__ == "__main__":
    main()
